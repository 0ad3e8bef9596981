"""Times REBUS-PLS on the headline model (10k x 60 x 6, satisfaction-shaped; K = 4 from a random start): one round -- K local models, the row pass, the
assignment, the read-back -- as the difference between runs of max_iter = 1 and max_iter = 0 (a run of max_iter = t is t iterations and the final pass: t + 1
rounds), a whole run to its stop, and the kernels' share by the handle's profile.  Host clock around plspm_rebus_device (the fetch is not timed), medians.

    python tools/rebus_time.py [--n 10000] [--classes 4] [--repeat 10]
prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for sub in ("plspm-python_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, sub))

import plspm_oracle as orc          # noqa: E402
from helpers_rebus import native_model, random_start          # noqa: E402
from plspm import _native          # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--classes", type=int, default=4)
    ap.add_argument("--repeat", type=int, default=10)
    args = ap.parse_args()
    C = orc.satisfaction_C()
    X, blocks = orc.synth(args.n, C, 10, seed=5)
    model = orc.Model(blocks, C, "AAAAAA", "path", True)
    nm = native_model(X, model)
    start = np.ascontiguousarray(random_start(args.n, args.classes, seed=1), dtype=np.int32)

    def device(max_iter):
        t0 = time.perf_counter()
        nm._check(nm._lib.plspm_rebus_device(nm._h, args.classes, start.ctypes.data, max_iter, 0.005, 10, None, None), "plspm_rebus_device")
        return (time.perf_counter() - t0) * 1e3

    device(1)                                              # digit planes, buffers, code objects
    t0 = np.median([device(0) for _ in range(args.repeat)])
    t1 = np.median([device(1) for _ in range(args.repeat)])
    t10 = np.median([device(10) for _ in range(args.repeat)])
    whole = [device(100) for _ in range(args.repeat)]
    nm.last_rebus = (args.classes, 100)
    run = nm.rebus_fetch()
    nm.profile(True)
    nm.profile_reset()
    device(10)
    prof = {}
    for name in _native.KERNELS:
        ms, launches = nm.profile_read(name)
        if launches:
            prof[name] = dict(ms=round(ms, 4), launches=launches)
    print(json.dumps(dict(n=args.n, classes=args.classes, final_pass_ms=round(float(t0), 4), one_iteration_ms=round(float(t1 - t0), 4), ten_iterations_ms=round(float(t10 - t0), 4),
                          whole_run_ms=round(float(np.median(whole)), 4), status=run["status"], iterations=run["iterations"], sizes=[int(v) for v in run["sizes"]],
                          profile_of_11_rounds=prof)))


if __name__ == "__main__":
    main()
