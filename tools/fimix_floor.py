"""The floor behind the bar of the FIMIX-PLS tests (tests/test_gpu_fimix.py), measured on the CPU: per case and per iteration count the largest
|fp64 mirror - longdouble mirror| over the records of the case's problems, both mirrors (plspm.fimix._fimix) on the same fp64 columns and the same starts.  The
cases are the GPU tests' (their generators' columns stand in for the device's scores, which equal them up to sign).  The bar of a comparison is ten times this
figure on the comparison's own inputs, at least 1e-12 max(1, |value|)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for sub in ("plspm-python_amd", "tests", "oracle"):
    sys.path.insert(0, os.path.join(ROOT, sub))

import helpers_fimix as hf                     # noqa: E402
from test_gpu_fimix import CASES, problems_of  # noqa: E402


def main():
    print("%-12s %s" % ("case", "  ".join("t = %-8d" % t for t in hf.ITERATIONS)))
    for name in CASES:
        Y, C, problems, solve = problems_of(name)
        worst = {t: 0.0 for t in hf.ITERATIONS}
        seen = set()
        for K, init in problems:
            if (K, init.tobytes()) in seen:
                continue
            seen.add((K, init.tobytes()))
            m64, mld = hf.mirror_pair(Y, C, K, init, 25, 0.0, solve=solve, snapshots=(1, 2, 5))
            for t in hf.ITERATIONS:
                a, b = hf.at(m64, t), hf.at(mld, t)
                assert a["status"] == b["status"] and a["iterations"] == b["iterations"], (name, K, t)
                worst[t] = max(worst[t], hf.difference(*hf.records(a, b, K)))
        print("%-12s %s" % (name, "  ".join("%-12.2g" % worst[t] for t in hf.ITERATIONS)))


if __name__ == "__main__":
    main()
