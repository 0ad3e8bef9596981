"""What the geodesic discrepancy (plspm_geodesic_enable; csrc/kernels_geodesic.h) adds to a bootstrap step on the headline model (10k x 60 x 6, Mode A,
Scheme.PATH, scaled; the composite model: an all-zero factor mask): 5,000 replicates per step in two settings -- model fit alone, and model fit + d_G -- on the
same handle in the same process, alternating; ms per step on the host clock (plspm_bootstrap_device + plspm_sync) and the per-stage kernel times from the
library's HIP events (plspm_profile_*) of instrumented steps of each kind.  The geodesic kernel is timed under the assessment's id, so its time is that id's
per-step total with the stage on minus the other setting's.  One JSON line, appended to profiles/geodesic_bench.jsonl.

    python tools/geodesic_bench.py [rounds]
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
OUT = os.path.join(ROOT, "profiles", "geodesic_bench.jsonl")
SETTINGS = ("modelfit", "geodesic")
MASK = np.zeros(6, dtype=np.uint8)


def step(setting, rep):
    nm.modelfit_enable(True, MASK)
    nm.geodesic_enable(setting == "geodesic")
    t = time.perf_counter()
    nm.bootstrap_device(B, seed=7, rep_offset=rep * B)
    nm.sync()
    return (time.perf_counter() - t) * 1e3


def kernels(setting, steps=10):
    """ms per STEP of every kernel id (the assessment's id counts three launches per step with model fit on, four with d_G)."""
    nm.profile(True); nm.profile_reset()
    for s in range(steps):
        step(setting, 1000 + s)
    out = {k: round(ms / steps, 4) for k in _native.KERNELS for ms, n in [nm.profile_read(k)] if n}
    nm.profile(False)
    return out


for w in range(3):                                             # warm-up: digit planes, buffers, tile plans, every kernel's code
    for setting in SETTINGS:
        step(setting, w)
times = {setting: [] for setting in SETTINGS}
for r in range(ROUNDS):
    for k in range(2):                                         # the order alternates from round to round
        setting = SETTINGS[(r + k) % 2]
        times[setting].append(step(setting, 10 + r))
kern = {setting: kernels(setting) for setting in SETTINGS}
step("geodesic", 5000)
original, status = nm.geodesic_fit()
records, st = nm.geodesic_fetch(0, B)
table, used = nm.geodesic_summary(B, original)
med = lambda v: round(float(np.median(v)), 4)      # noqa: E731
kernel = round(kern["geodesic"].get("assess", 0.0) - kern["modelfit"].get("assess", 0.0), 4)
line = json.dumps({"workload": "10k x 60 x 6, Mode A, PATH, scaled, all-zero factor mask", "rounds": ROUNDS, "replicates": B, "replicates_used": used,
                   "replicates_inadmissible": int(np.count_nonzero(st == 4)), "full_sample_status": status, "full_sample_record": [round(float(x), 6) for x in original],
                   "step_ms_median": {s: med(times[s]) for s in SETTINGS}, "step_ms_min": {s: round(min(times[s]), 4) for s in SETTINGS},
                   "geodesic_over_modelfit_median": round(float(np.median(times["geodesic"])) / float(np.median(times["modelfit"])), 4),
                   "geodesic_added_ms_median": round(float(np.median(times["geodesic"])) - float(np.median(times["modelfit"])), 4),
                   "kernel_ms_per_step": kern, "geodesic_kernel_ms_per_step": kernel,
                   "geodesic_kernel_over_step": round(kernel / float(np.median(times["geodesic"])), 4)})
print(line)
with open(OUT, "a") as f:
    f.write(line + "\n")
