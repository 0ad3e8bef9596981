"""Confidence intervals and the jackknife on the headline model (10k x 60 x 6, Mode A, Scheme.PATH, scaled), two comparisons, each with its
yardstick on the same handle in the same process, the calls alternating:
  * plspm_bootstrap_intervals (each of the four methods, 5,000 replicates in HBM) against plspm_bootstrap_summary on the same records -- ms per call
    on the host clock (both calls wait for their result);
  * plspm_jackknife_device at G = N = 10,000 against a bootstrap of 10,000 replicates -- ms per call, and the per-stage kernel times from the
    library's HIP events (plspm_profile_*) of one instrumented call of each.
One JSON line, appended to profiles/ci_bench.jsonl.

    python tools/ci_bench.py [rounds]
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

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 20
N, B = 10000, 5000
C = satisfaction_C()
X, blocks = synth(N, C, 10, seed=0)
boff = np.concatenate(([0], np.cumsum([len(b) for b in blocks]))).astype(np.int32)
nm = _native.NativeModel(boff, C.astype(np.uint8), np.zeros(6, dtype=np.int32), 2, True, 100, 1e-6, 0)
nm.upload(X)
OUT = os.path.join(ROOT, "profiles", "ci_bench.jsonl")
fit = nm.fit(want_scores=False)
original = np.concatenate((fit["weights"], fit["r2"], fit["total"], fit["direct"], fit["loadings"]))


def kernels():
    return {k: (round(ms, 4), n) for k in _native.KERNELS for ms, n in [nm.profile_read(k)] if n}


def timed(f):
    t = time.perf_counter()
    f()
    return (time.perf_counter() - t) * 1e3


# ---- the jackknife against a bootstrap of as many problems
for w in range(2):                                             # warm-up: planes of both floors, buffers, tile plans
    nm.jackknife(N); nm.sync()
    nm.bootstrap_device(N, seed=1, rep_offset=w * N); nm.sync()
t_jack, t_boot = [], []
for r in range(ROUNDS):
    steps = [(t_jack, lambda: (nm.jackknife(N), nm.sync())), (t_boot, lambda: (nm.bootstrap_device(N, seed=7, rep_offset=(2 + r) * N), nm.sync()))]
    for sink, step in (steps if r % 2 == 0 else steps[::-1]):
        sink.append(timed(step))
nm.profile(True); nm.profile_reset()
nm.jackknife(N); nm.sync()
k_jack = kernels()
nm.profile_reset()
nm.bootstrap_device(N, seed=7, rep_offset=1000 * N); nm.sync()
k_boot = kernels()
nm.profile(False)
t_stats = [timed(lambda: nm.jackknife_stats(N)) for _ in range(ROUNDS)]
_, _, accel, jack_used = nm.jackknife_stats(N)

# ---- the intervals against the summary, on the records of one bootstrap of 5,000 replicates
nm.bootstrap_device(B, seed=3); nm.sync()
for method in _native.CI_METHODS:
    nm.intervals(B, original, method, 0.95, accel)
nm.summary(B, original)
t_ci = {method: [] for method in _native.CI_METHODS}
t_sum = []
for r in range(ROUNDS):
    steps = [(t_ci[method], (lambda method=method: nm.intervals(B, original, method, 0.95, accel))) for method in _native.CI_METHODS]
    steps.insert(r % (len(steps) + 1), (t_sum, lambda: nm.summary(B, original)))
    for sink, step in steps:
        sink.append(timed(step))
table, used = nm.intervals(B, original, "bca", 0.95, accel)
med = lambda v: round(float(np.median(v)), 4)      # noqa: E731
line = json.dumps({"workload": "10k x 60 x 6, Mode A, PATH, scaled", "rounds": ROUNDS, "replicates": B, "replicates_used": used,
                   "summary_ms_per_call_median": med(t_sum), "summary_ms_per_call_min": round(min(t_sum), 4),
                   "intervals_ms_per_call_median": {k: med(v) for k, v in t_ci.items()}, "intervals_ms_per_call_min": {k: round(min(v), 4) for k, v in t_ci.items()},
                   "intervals_over_summary": {k: round(float(np.median(v)) / float(np.median(t_sum)), 3) for k, v in t_ci.items()},
                   "jackknife_problems": N, "jackknife_used": jack_used,
                   "jackknife_ms_per_call_median": med(t_jack), "jackknife_ms_per_call_min": round(min(t_jack), 4),
                   "bootstrap_ms_per_call_median": med(t_boot), "bootstrap_ms_per_call_min": round(min(t_boot), 4),
                   "jackknife_over_bootstrap": round(float(np.median(t_jack)) / float(np.median(t_boot)), 3),
                   "jackknife_stats_ms_per_call_median": med(t_stats),
                   "jackknife_kernel_ms_launches": k_jack, "bootstrap_kernel_ms_launches": k_boot,
                   "bca_columns_finite": int(np.isfinite(table[:, 0]).sum()), "max_abs_accel": float(np.nanmax(np.abs(accel)))})
print(line)
with open(OUT, "a") as f:
    f.write(line + "\n")
