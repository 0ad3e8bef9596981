"""What the importance-performance map analysis (plspm_ipma_enable; csrc/kernels_ipma.h) adds to a bootstrap step on the headline model (10k x 60 x 6, Mode A,
Scheme.PATH, scaled): 5,000 replicates per step with the switch off and on (every LV with a predecessor a target, observed bounds), on the same handle in the
same process, the two alternating; ms per step on the host clock (plspm_bootstrap_device + plspm_sync) and the per-step time of the wave-per-replicate kernels
from the library's HIP events (plspm_profile_*; the IPMA kernel is launched through the "assess" slot, which holds nothing else here) of instrumented steps of
each kind.  One JSON line, appended to profiles/ipma_bench.jsonl.

    python tools/ipma_bench.py [rounds]
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

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 40
N, B = 10000, 5000
C = satisfaction_C()
X, blocks = synth(N, C, 10, seed=0)
boff = np.concatenate(([0], np.cumsum([len(b) for b in blocks]))).astype(np.int32)
nm = _native.NativeModel(boff, C.astype(np.uint8), np.zeros(6, dtype=np.int32), 2, True, 100, 1e-6, 0)
nm.upload(X)
LO, HI = X.min(axis=0), X.max(axis=0)
OUT = os.path.join(ROOT, "profiles", "ipma_bench.jsonl")
KINDS = ("off", "on")


def step(kind, rep):
    if kind == "off":
        nm.ipma_enable(False)
    else:
        nm.ipma_enable(True, None, LO, HI)
    t = time.perf_counter()
    nm.bootstrap_device(B, seed=7, rep_offset=rep * B)
    nm.sync()
    return (time.perf_counter() - t) * 1e3


def kernels(kind, steps=10):
    """Per step: the total time of every kernel slot (a slot's launches of one step added up)."""
    nm.profile(True); nm.profile_reset()
    for s in range(steps):
        step(kind, 1000 + s)
    out = {k: round(ms / steps, 4) for k in _native.KERNELS for ms, n in [nm.profile_read(k)] if n}
    nm.profile(False)
    return out


for w in range(3):                                             # warm-up: digit planes, buffers, tile plans, the kernels' code
    for kind in KINDS:
        step(kind, w)
times = {kind: [] for kind in KINDS}
for r in range(ROUNDS):
    for kind in KINDS[r % 2:] + KINDS[:r % 2]:
        times[kind].append(step(kind, 10 + r))
kern = {kind: kernels(kind) for kind in KINDS}
step("on", 5000)
original, status = nm.ipma_fit()
_, used = nm.ipma_summary(B, original)
_, st = nm.ipma_fetch(0, B)
med = lambda v: round(float(np.median(v)), 4)      # noqa: E731
line = json.dumps({"workload": "10k x 60 x 6, Mode A, PATH, scaled", "rounds": ROUNDS, "replicates": B, "replicates_used": used,
                   "replicates_inadmissible": int(np.count_nonzero(st == 4)), "full_sample_status": status, "ipma_width": nm.ipma_width,
                   "step_ms_median": {kind: med(times[kind]) for kind in KINDS}, "step_ms_min": {kind: round(min(times[kind]), 4) for kind in KINDS},
                   "added_ms_per_step_median": round(float(np.median(times["on"])) - float(np.median(times["off"])), 4),
                   "kernel_ms_per_step": kern,
                   "ipma_kernel_ms_per_step": round(kern["on"].get("assess", 0.0) - kern["off"].get("assess", 0.0), 4)})
print(line)
with open(OUT, "a") as f:
    f.write(line + "\n")
