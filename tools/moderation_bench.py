"""What the moderation analysis (plspm_moderation_enable; csrc/kernels_moderation.h) adds to a bootstrap call on the headline model (10k x 60 x 6, Mode A,
Scheme.PATH, scaled): 5,000 replicates per call, moderation off and on with one term (IMAG x EXPE -> SAT) and with three (+ QUAL x VAL -> SAT, IMAG x SAT ->
LOY), on handles of their own in one process, the calls alternating; ms per call on the host clock (plspm_bootstrap_device + plspm_sync) and the per-call time
of the four moderation kernels from the library's HIP events (plspm_profile_*) of instrumented calls.  One JSON line, appended to
profiles/moderation_bench.jsonl.

    python tools/moderation_bench.py [rounds]
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
TERMS = [(0, 1, 4), (2, 3, 4), (0, 4, 5)]
OUT = os.path.join(ROOT, "profiles", "moderation_bench.jsonl")


def handle(terms):
    nm = _native.NativeModel(boff, C.astype(np.uint8), np.zeros(6, dtype=np.int32), 2, True, 100, 1e-6, 0)
    nm.upload(X)
    if terms:
        nm.moderation_enable(terms)
    return nm


HANDLES = {"off": handle(None), "one_term": handle(TERMS[:1]), "three_terms": handle(TERMS)}


def step(nm, rep):
    t = time.perf_counter()
    nm.bootstrap_device(B, seed=7, rep_offset=rep * B)
    nm.sync()
    return (time.perf_counter() - t) * 1e3


def kernels(nm, steps=5):
    """Per call: the total time of every kernel slot (a slot's launches of one call added up)."""
    nm.profile(True); nm.profile_reset()
    for s in range(steps):
        step(nm, 1000 + s)
    out = {k: round(ms / steps, 4) for k in _native.KERNELS for ms, n in [nm.profile_read(k)] if n}
    nm.profile(False)
    return out


for w in range(3):                                             # warm-up: digit planes, buffers, tile plans, every kernel's code
    for nm in HANDLES.values():
        step(nm, w)
times = {name: [] for name in HANDLES}
names = list(HANDLES)
for r in range(ROUNDS):
    for name in (names if r % 2 == 0 else names[::-1]):
        times[name].append(step(HANDLES[name], 10 + r))
med = lambda v: round(float(np.median(v)), 4)      # noqa: E731
line = {"workload": "10k x 60 x 6, Mode A, PATH, scaled", "rounds": ROUNDS, "replicates": B}
for name, nm in HANDLES.items():
    line["call_ms_median_" + name] = med(times[name])
    line["call_ms_min_" + name] = round(min(times[name]), 4)
    line["call_ms_max_" + name] = round(max(times[name]), 4)
    line["kernel_ms_per_call_" + name] = kernels(nm)
for name in ("one_term", "three_terms"):
    line["on_over_off_median_" + name] = round(float(np.median(times[name])) / float(np.median(times["off"])), 4)
    line["moderation_width_" + name] = HANDLES[name].moderation_width
print(json.dumps(line))
os.makedirs(os.path.dirname(OUT), exist_ok=True)
with open(OUT, "a") as f:
    f.write(json.dumps(line) + "\n")
