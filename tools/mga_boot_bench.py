"""The two-group bootstrap on the headline model (10k x 60 x 6, Mode A, Scheme.PATH, scaled): ms per call of 5,000 resamples per group (= 10,000
problems) at 50/50 and 20/80 splits, per-kernel times from the library's HIP events (plspm_profile_*: draws, Gram, solver; Henseler's pair
counts), the two per-group summaries (timed on the host: they return their results), and the permutation call of the same size on the same data
in the same process, the calls alternating.  Both calls run on handles of their own (each keeps its digit planes; seven for both).  The row lists of the draws kernel are measured from LDS
and through L2 ("strat_rows" 2 / 1).  One JSON line per split.

    python tools/mga_boot_bench.py [resamples] [rounds]
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


strat, perm = handle(), handle()
RS, R = strat.row_stride, strat.row_width
orig = np.zeros(R)


def kernels(nm):
    out = {}
    for k in _native.KERNELS:
        ms, n = nm.profile_read(k)
        if n:
            out[k] = round(ms / n, 4)
    return out


def post(nm, d_out):
    """The two per-group summaries and the pair counts, as GroupComparison runs them."""
    sa, _ = nm.summary(B, orig, d_rows=d_out, stride=2 * RS)
    sb, _ = nm.summary(B, orig, d_rows=d_out + 8 * RS, stride=2 * RS)
    return nm.stratified_pair_counts(B, sa[:, 1], sb[:, 1])


for n_a in (N // 2, N // 5):
    member = np.zeros(N, dtype=bool)
    member[np.random.default_rng(1).permutation(N)[:n_a]] = True
    for w in range(2):
        strat.stratified_bootstrap(B, member, seed=1, rep_offset=w * B); strat.sync()
        perm.permutation(B, n_a, seed=1, rep_offset=w * B); perm.sync()
    t_strat, t_perm, t_post = [], [], []
    for r in range(ROUNDS):
        for nm, times in ((strat, t_strat), (perm, t_perm)) if r % 2 == 0 else ((perm, t_perm), (strat, t_strat)):
            t = time.perf_counter()
            if nm is strat:
                d_out, _, _ = nm.stratified_bootstrap(B, member, seed=7, rep_offset=(2 + r) * B)
            else:
                nm.permutation(B, n_a, seed=7, rep_offset=(2 + r) * B)
            nm.sync()
            times.append((time.perf_counter() - t) * 1e3)
        t = time.perf_counter()
        above, used_a, used_b = post(strat, d_out)
        t_post.append((time.perf_counter() - t) * 1e3)
    # instrumented calls (HIP events around every kernel): the stratified call, the summaries, the pair counts, per row-list placement
    k_strat = {}
    strat.profile(True)
    for name, opt in (("lds", 2), ("l2", 1)):
        strat.set_option("strat_rows", opt)
        strat.profile_reset()
        d_out, _, _ = strat.stratified_bootstrap(B, member, seed=7, rep_offset=100 * B); strat.sync()
        k_strat[name] = kernels(strat)
        k_strat[name]["rows_from"] = strat.get_option("last_strat_rows")
    strat.set_option("strat_rows", 0)
    strat.stratified_bootstrap(B, member, seed=7, rep_offset=100 * B); strat.sync()
    auto = strat.get_option("last_strat_rows")
    t = time.perf_counter()
    sa, _ = strat.summary(B, orig, d_rows=d_out, stride=2 * RS)
    strat.summary(B, orig, d_rows=d_out + 8 * RS, stride=2 * RS)
    summ_ms = (time.perf_counter() - t) * 1e3                  # (host-timed: both summaries return their results to the host)
    strat.profile_reset()
    strat.stratified_pair_counts(B, sa[:, 1], sa[:, 1])
    k_pair = kernels(strat)
    strat.profile(False)
    perm.profile(True); perm.profile_reset()
    perm.permutation(B, n_a, seed=7, rep_offset=100 * B); perm.sync()
    k_perm = kernels(perm)
    perm.profile(False)
    sm, pm = float(np.median(t_strat)), float(np.median(t_perm))
    print(json.dumps({"workload": "10k x 60 x 6, Mode A, PATH, scaled", "split": "%d/%d" % (n_a, N - n_a), "resamples_per_group": B, "rounds": ROUNDS,
                      "boot_ms_per_call_median": round(sm, 4), "boot_ms_per_call_min": round(min(t_strat), 4),
                      "perm_ms_per_call_median": round(pm, 4), "perm_ms_per_call_min": round(min(t_perm), 4), "boot_over_perm": round(sm / pm, 3),
                      "post_ms_median": round(float(np.median(t_post)), 4), "used_last": [int(used_a), int(used_b)],
                      "rows_auto": {1: "l2", 2: "lds"}.get(auto, auto), "boot_kernel_ms": k_strat, "summaries_ms_two_calls": round(summ_ms, 4),
                      "pair_counts_kernel_ms": k_pair, "perm_kernel_ms": k_perm}))
