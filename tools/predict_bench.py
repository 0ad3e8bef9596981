"""Out-of-sample prediction (repeated k-fold cross-validation) on the headline model (10k x 60 x 6, Mode A, Scheme.PATH, scaled): 10 folds x 10
and 10 folds x 500 repetitions.  Per size: ms per call of the training fits + training moments (plspm_cv_device) and of the PLS prediction errors
(plspm_cv_predict: compose + apply + the download of the sums), per-stage kernel times from the library's HIP events (plspm_profile_*: "resample"
= folds + count rows, "reduce" = training moments | compose + apply), and the bootstrap's ms per call of the same number of problems on the same
handle in the same process, the calls alternating -- the yardstick.  One JSON line per size, appended to profiles/predict_bench.jsonl.

    python tools/predict_bench.py [rounds]
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "plspm-python_amd")); sys.path.insert(0, os.path.join(ROOT, "tools"))
from plspm import _native  # noqa: E402
from synthetic import satisfaction_C, synth  # noqa: E402

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 10
N, K = 10000, 10
C = satisfaction_C()
X, blocks = synth(N, C, 10, seed=0)
boff = np.concatenate(([0], np.cumsum([len(b) for b in blocks]))).astype(np.int32)
nm = _native.NativeModel(boff, C.astype(np.uint8), np.zeros(6, dtype=np.int32), 2, True, 100, 1e-6, 0)
nm.upload(X)
OUT = os.path.join(ROOT, "profiles", "predict_bench.jsonl")


def kernels():
    return {k: (round(ms, 4), n) for k in _native.KERNELS for ms, n in [nm.profile_read(k)] if n}


for reps in (10, 500):
    B = reps * K
    for w in range(2):                                         # warm-up: planes of both floors, buffers, tile plans
        nm.cv(reps, K, seed=1, rep_offset=w * reps); nm.cv_predict(reps, K)
        nm.bootstrap_device(B, seed=1, rep_offset=w * B); nm.sync()
    t_cv, t_pred, t_boot = [], [], []

    def run_cv(r):
        t = time.perf_counter()
        nm.cv(reps, K, seed=7, rep_offset=(2 + r) * reps); nm.sync()
        t_cv.append((time.perf_counter() - t) * 1e3)
        t = time.perf_counter()
        nm.cv_predict(reps, K)
        t_pred.append((time.perf_counter() - t) * 1e3)

    def run_boot(r):
        t = time.perf_counter()
        nm.bootstrap_device(B, seed=7, rep_offset=(2 + r) * B); nm.sync()
        t_boot.append((time.perf_counter() - t) * 1e3)

    for r in range(ROUNDS):
        for step in (run_cv, run_boot) if r % 2 == 0 else (run_boot, run_cv):
            step(r)
    # one instrumented call of each (HIP events around every kernel)
    nm.profile(True); nm.profile_reset()
    nm.cv(reps, K, seed=7, rep_offset=1000 * reps); nm.sync()
    k_cv = kernels()
    nm.profile_reset()
    sse, sae, sst, rows, _, _ = nm.cv_predict(reps, K)
    k_pred = kernels()
    nm.profile_reset()
    nm.bootstrap_device(B, seed=7, rep_offset=1000 * B); nm.sync()
    k_boot = kernels()
    nm.profile(False)
    cv, pr, bo = float(np.median(t_cv)), float(np.median(t_pred)), float(np.median(t_boot))
    line = json.dumps({"workload": "10k x 60 x 6, Mode A, PATH, scaled", "folds": K, "repetitions": reps, "problems": B, "rounds": ROUNDS,
                       "cv_ms_per_call_median": round(cv, 4), "cv_ms_per_call_min": round(min(t_cv), 4),
                       "predict_ms_per_call_median": round(pr, 4), "predict_ms_per_call_min": round(min(t_pred), 4),
                       "bootstrap_ms_per_call_median": round(bo, 4), "bootstrap_ms_per_call_min": round(min(t_boot), 4),
                       "cv_plus_predict_over_bootstrap": round((cv + pr) / bo, 3), "problems_used": int((rows > 0).sum()),
                       "cv_kernel_ms_launches": k_cv, "predict_kernel_ms_launches": k_pred, "bootstrap_kernel_ms_launches": k_boot})
    print(line)
    with open(OUT, "a") as f:
        f.write(line + "\n")
