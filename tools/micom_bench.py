"""MICOM on the headline model (10k x 60 x 6, Mode A, Scheme.PATH, scaled): ms per permutation call of 5,000 permutations (= 10,000 problems) at a
5,000 / 5,000 split with the MICOM records on and off, the two alternating in one process on two handles of the same data; per-kernel times from the
library's HIP events (plspm_profile_*: the MICOM kernel is timed under "assess", the counts under "reduce"); the plspm_micom_counts and
plspm_micom_intervals calls.  One JSON line.

    python tools/micom_bench.py [permutations] [rounds]
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
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 40
N, n1 = 10000, 5000
C = satisfaction_C()
X, blocks = synth(N, C, 10, seed=0)
boff = np.concatenate(([0], np.cumsum([len(b) for b in blocks]))).astype(np.int32)


def handle(micom):
    nm = _native.NativeModel(boff, C.astype(np.uint8), np.zeros(6, dtype=np.int32), 2, True, 100, 1e-6, 0)
    nm.upload(X)
    nm.micom_enable(micom)
    return nm


def kernels(nm):
    out = {}
    for k in _native.KERNELS:
        ms, n = nm.profile_read(k)
        if n:
            out[k] = round(ms / n, 4)
    return out


on, off = handle(True), handle(False)
# the observed split's record (a one-permutation call with explicit memberships); it also builds the pooled inputs, once per upload
member = np.zeros((1, N), dtype=bool)
member[0, :n1] = True
on.permutation(1, n1, member=member)
observed = on.micom_fetch(0, 1)[0][0]
for w in range(2):                        # warm-up: planes, buffers, tile plans
    for nm in (on, off):
        nm.permutation(B, n1, seed=1, rep_offset=w * B); nm.sync()
t_on, t_off, t_cnt, t_ci = [], [], [], []
for r in range(ROUNDS):
    for nm, times in ((on, t_on), (off, t_off)) if r % 2 == 0 else ((off, t_off), (on, t_on)):
        t = time.perf_counter()
        nm.permutation(B, n1, seed=7, rep_offset=(2 + r) * B)
        nm.sync()
        times.append((time.perf_counter() - t) * 1e3)
    t = time.perf_counter()
    below, exceed, used = on.micom_counts(B, observed)
    t_cnt.append((time.perf_counter() - t) * 1e3)
    t = time.perf_counter()
    on.micom_intervals(B, observed, "percentile", 0.95)
    t_ci.append((time.perf_counter() - t) * 1e3)
# one instrumented call of each (HIP events around every kernel)
prof = {}
for name, nm in (("on", on), ("off", off)):
    nm.profile(True); nm.profile_reset()
    nm.permutation(B, n1, seed=7, rep_offset=100 * B); nm.sync()
    step = kernels(nm)
    if nm is on:
        nm.profile_reset()
        nm.micom_counts(B, observed)
        step["counts_kernel"] = kernels(nm).get("reduce")
    prof[name] = step
    nm.profile(False)
m_on, m_off = float(np.median(t_on)), float(np.median(t_off))
print(json.dumps({"workload": "10k x 60 x 6, Mode A, PATH, scaled", "split": "%d/%d" % (n1, N - n1), "permutations_per_call": B, "rounds": ROUNDS,
                  "permutations_used": int(used), "micom_width": on.micom_width,
                  "call_ms_median_off": round(m_off, 4), "call_ms_median_on": round(m_on, 4), "call_ms_min_off": round(min(t_off), 4), "call_ms_min_on": round(min(t_on), 4),
                  "on_over_off_median": round(m_on / m_off, 4), "kernel_ms_per_launch_off": prof["off"], "kernel_ms_per_launch_on": prof["on"],
                  "micom_counts_ms_per_call_median": round(float(np.median(t_cnt)), 4), "micom_intervals_ms_per_call_median": round(float(np.median(t_ci)), 4)}))
