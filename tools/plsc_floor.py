"""CPU: the figures behind the bar of tests/test_gpu_plsc.py.  For every case of tests/helpers_plsc.py, on its nine resamples and on all rows, with the
ORACLE's weights and loadings in place of the device's: the largest |fp64 mirror - longdouble mirror| over the PLSc record (plspm.plsc._plsc), whether
every resample is admissible and whether every predecessor matrix passes the pivot test.  The floor of the bar is the largest of these differences,
never below 1e-12.

    python tools/plsc_floor.py [case ...]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "plspm-python_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]

import plspm_oracle as orc                                     # noqa: E402
from helpers_plsc import CASES, case, mirror_difference, mirror_pair, negative_pair_model, resamples      # noqa: E402


def oracle_inputs(Xr, model):
    f = orc.fit(Xr, model, orc.correction(Xr.shape[0]))
    return f["weights"][model.mv_order], f["loadings"][model.mv_order]


def main(names):
    worst_all = 0.0
    for name in names:
        X, model, _, _, _, factor = case(name)
        idx = resamples(X)
        worst, admissible, pivots = 0.0, True, True
        for rows in [X] + [X[idx[r]] for r in range(idx.shape[0])]:
            w, lam = oracle_inputs(rows, model)
            m64, mld = mirror_pair(rows[:, model.mv_order], model, w, lam, factor)
            admissible = admissible and m64["status"] == 0 and mld["status"] == 0
            pivots = pivots and m64["pivots_pass"]
            if m64["status"] == 0 and mld["status"] == 0:
                worst = max(worst, mirror_difference(m64, mld))
        worst_all = max(worst_all, worst)
        print("%-18s max |fp64 - longdouble| %.3e   all admissible: %s   all pivots pass: %s" % (name, worst, admissible, pivots), flush=True)
    print("floor: max(%.3e, 1e-12)" % worst_all)
    X, model = negative_pair_model()
    idx = resamples(X, 24, seed=3)
    signs = []
    for rows in [X] + [X[idx[r]] for r in range(idx.shape[0])]:
        w, lam = oracle_inputs(rows, model)
        m64, _ = mirror_pair(rows[:, model.mv_order], model, w, lam, None)
        signs.append((float(m64["quality"]["rho_a"][0]), m64["status"]))
    print("negative pair: rho_A of LV 0 on all rows %.4f (status %d); resamples with rho_A < 0: %d of %d; item correlation %.4f"
          % (signs[0][0], signs[0][1], sum(s[0] < 0 for s in signs[1:]), len(signs) - 1, np.corrcoef(X[:, 0], X[:, 1])[0, 1]))


if __name__ == "__main__":
    main(sys.argv[1:] or CASES)
