"""The two-group permutation test on the headline model (10k x 60 x 6, Mode A, Scheme.PATH, scaled): permutations per second at 50/50 and
20/80 splits, 5,000 permutations per call (= 10,000 problems), per-kernel times from the library's HIP events (plspm_profile_*), the
exceedance-count call, and the bootstrap's ms per 5,000 replicates on the same data in the same process, the calls alternating.  The
permutation calls and the bootstrap calls run on two handles of the same data (each keeps its own digit planes: seven for the permutations,
the automatic six for the bootstrap).  One JSON line per split.

    python tools/mga_bench.py [permutations] [rounds]
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

B = int(sys.argv[1]) if len(sys.argv) > 1 else 5000
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 10
N = 10000
C = satisfaction_C()
X, blocks = synth(N, C, 10, seed=0)
boff = np.concatenate(([0], np.cumsum([len(b) for b in blocks]))).astype(np.int32)


def handle():
    nm = _native.NativeModel(boff, C.astype(np.uint8), np.zeros(6, dtype=np.int32), 2, True, 100, 1e-6, 0)
    nm.upload(X)
    return nm


perm, boot = handle(), handle()
diff = np.zeros(perm.row_width)           # (the counts kernel's work does not depend on the observed differences)


def kernels(nm):
    out = {}
    for k in _native.KERNELS:
        ms, n = nm.profile_read(k)
        if n:
            out[k] = round(ms / n, 4)
    return out


for n1 in (N // 2, N // 5):
    # warm-up: planes, buffers, tile plans
    for w in range(2):
        perm.permutation(B, n1, seed=1, rep_offset=w * B); perm.sync()
        boot.bootstrap_device(B, seed=1, rep_offset=w * B); boot.sync()
    t_perm, t_boot, t_cnt, k_perm, k_boot = [], [], [], [], []
    for r in range(ROUNDS):
        for nm, times in ((perm, t_perm), (boot, t_boot)) if r % 2 == 0 else ((boot, t_boot), (perm, t_perm)):
            t = time.perf_counter()
            if nm is perm:
                nm.permutation(B, n1, seed=7, rep_offset=(2 + r) * B)
            else:
                nm.bootstrap_device(B, seed=7, rep_offset=(2 + r) * B)
            nm.sync()
            times.append((time.perf_counter() - t) * 1e3)
        t = time.perf_counter()
        exceed, used = perm.permutation_counts(B, diff)
        t_cnt.append((time.perf_counter() - t) * 1e3)
    # one instrumented call of each (HIP events around every kernel)
    for nm, store in ((perm, k_perm), (boot, k_boot)):
        nm.profile(True); nm.profile_reset()
        if nm is perm:
            nm.permutation(B, n1, seed=7, rep_offset=100 * B); nm.sync()
            nm.permutation_counts(B, diff)
        else:
            nm.bootstrap_device(B, seed=7, rep_offset=100 * B); nm.sync()
        store.append(kernels(nm))
        nm.profile(False)
    pm, bm = float(np.median(t_perm)), float(np.median(t_boot))
    print(json.dumps({"workload": "10k x 60 x 6, Mode A, PATH, scaled", "split": "%d/%d" % (n1, N - n1), "permutations_per_call": B, "rounds": ROUNDS,
                      "perm_ms_per_call_median": round(pm, 4), "perm_ms_per_call_min": round(min(t_perm), 4),
                      "permutations_per_s": round(B / pm * 1e3), "counts_ms_median": round(float(np.median(t_cnt)), 4), "n_used_last": int(used),
                      "perm_digit_planes": 7, "perm_kernel_ms": k_perm[0],
                      "bootstrap_ms_per_call_median": round(bm, 4), "bootstrap_ms_per_call_min": round(min(t_boot), 4),
                      "bootstrap_replicates_per_s": round(B / bm * 1e3), "bootstrap_kernel_ms": k_boot[0],
                      "perm_over_replicate": round(pm / bm, 3)}))
