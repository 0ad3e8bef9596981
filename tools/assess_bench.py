"""What the measurement-model assessment (plspm_assess_enable; csrc/kernels_assess.h) adds to a bootstrap step on the headline model (10k x 60 x 6, Mode A,
Scheme.PATH, scaled): 5,000 replicates per step with assessment on and off, on the same handle in the same process, the two alternating; ms per step on
the host clock (plspm_bootstrap_device + plspm_sync) and the per-stage kernel times from the library's HIP events (plspm_profile_*) of instrumented steps
of each kind.  One JSON line, appended to profiles/assess_bench.jsonl.

    python tools/assess_bench.py [rounds]
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
OUT = os.path.join(ROOT, "profiles", "assess_bench.jsonl")


def step(on, rep):
    nm.assess_enable(on)
    t = time.perf_counter()
    nm.bootstrap_device(B, seed=7, rep_offset=rep * B)
    nm.sync()
    return (time.perf_counter() - t) * 1e3


def kernels(on, steps=10):
    nm.profile(True); nm.profile_reset()
    for s in range(steps):
        step(on, 1000 + s)
    out = {k: round(ms / n, 4) for k in _native.KERNELS for ms, n in [nm.profile_read(k)] if n}
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
nm.assess_enable(True)
step(True, 5000)
original, _ = nm.assess_fit()
t_sum = []
for _ in range(10):
    t = time.perf_counter(); table, used = nm.assess_summary(B, original); t_sum.append((time.perf_counter() - t) * 1e3)
med = lambda v: round(float(np.median(v)), 4)      # noqa: E731
kernel_step_off = sum(k_off.get(k, 0.0) for k in ("resample", "gram", "solver"))
line = json.dumps({"workload": "10k x 60 x 6, Mode A, PATH, scaled", "rounds": ROUNDS, "replicates": B, "replicates_used": used, "assess_width": nm.assess_width,
                   "step_ms_median_off": med(t_off), "step_ms_median_on": med(t_on), "step_ms_min_off": round(min(t_off), 4), "step_ms_min_on": round(min(t_on), 4),
                   "on_over_off_median": round(float(np.median(t_on)) / float(np.median(t_off)), 4),
                   "kernel_ms_per_launch_off": k_off, "kernel_ms_per_launch_on": k_on,
                   "assess_kernel_over_kernels_of_a_step": round(k_on.get("assess", 0.0) / kernel_step_off, 4) if kernel_step_off else None,
                   "assess_summary_ms_per_call_median": med(t_sum)})
print(line)
with open(OUT, "a") as f:
    f.write(line + "\n")
