"""What the structural-model assessment (plspm_structural_enable; csrc/kernels_structural.h) adds to a bootstrap step on the headline model (10k x 60 x 6,
Mode A, Scheme.PATH, scaled): 5,000 replicates per step with the assessment on, with and without the structural stage, on the same handle in the same
process, the two alternating; ms per step on the host clock (plspm_bootstrap_device + plspm_sync) and the per-step time of the wave-per-replicate kernels
from the library's HIP events (plspm_profile_*; the assessment and the structural kernel share the "assess" slot) of instrumented steps of each kind.  One
JSON line, appended to profiles/structural_bench.jsonl.

    python tools/structural_bench.py [rounds]
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
nm.assess_enable(True)
OUT = os.path.join(ROOT, "profiles", "structural_bench.jsonl")


def step(on, rep):
    nm.structural_enable(on)
    t = time.perf_counter()
    nm.bootstrap_device(B, seed=7, rep_offset=rep * B)
    nm.sync()
    return (time.perf_counter() - t) * 1e3


def kernels(on, steps=10):
    """Per step: the total time of every kernel slot (a slot's launches of one step added up)."""
    nm.profile(True); nm.profile_reset()
    for s in range(steps):
        step(on, 1000 + s)
    out = {k: round(ms / steps, 4) for k in _native.KERNELS for ms, n in [nm.profile_read(k)] if n}
    nm.profile(False)
    return out


for w in range(3):                                             # warm-up: digit planes, buffers, tile plans, both kernels' code
    step(True, w); step(False, w)
t_on, t_off = [], []
for r in range(ROUNDS):
    order = [(t_on, True), (t_off, False)]
    for sink, on in (order if r % 2 == 0 else order[::-1]):
        sink.append(step(on, 10 + r))
k_on, k_off = kernels(True), kernels(False)
step(True, 5000)
original, _ = nm.structural_fit()
t_sum = []
for _ in range(10):
    t = time.perf_counter(); table, used = nm.structural_summary(B, original); t_sum.append((time.perf_counter() - t) * 1e3)
med = lambda v: round(float(np.median(v)), 4)      # noqa: E731
line = json.dumps({"workload": "10k x 60 x 6, Mode A, PATH, scaled", "rounds": ROUNDS, "replicates": B, "replicates_used": used, "structural_width": nm.structural_width,
                   "step_ms_median_assess_only": med(t_off), "step_ms_median_with_structural": med(t_on), "step_ms_min_assess_only": round(min(t_off), 4),
                   "step_ms_min_with_structural": round(min(t_on), 4), "added_ms_per_step_median": round(float(np.median(t_on)) - float(np.median(t_off)), 4),
                   "with_over_without_median": round(float(np.median(t_on)) / float(np.median(t_off)), 4),
                   "kernel_ms_per_step_assess_only": k_off, "kernel_ms_per_step_with_structural": k_on,
                   "structural_kernel_ms_per_step": round(k_on.get("assess", 0.0) - k_off.get("assess", 0.0), 4),
                   "structural_summary_ms_per_call_median": med(t_sum)})
print(line)
with open(OUT, "a") as f:
    f.write(line + "\n")
