"""CPU: the figures behind the bars of tests/test_gpu_moderation.py.  For every case of tests/helpers_moderation.py, on its nine resamples and on all rows, with
the ORACLE's records in place of the device's: the largest |fp64 mirror - longdouble mirror| over the moderation record (plspm.moderation._moderation),
whether every data set has status 0 and finite values, and whether every regression passes the pivot test.  The bar of a case is ten times its figure,
never below 1e-12.  With `--oracle`: for the satisfaction case, how far the moderated coefficients of the full sample move when the oracle's record moves
inside the record bar (helpers_moderation.perturbation_figure) -- the figure behind the end-to-end bar.

    python tools/moderation_floor.py [--oracle] [case ...]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "plspm-python_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]

from helpers_moderation import CASES, case, counts_of, mirror_difference, mirror_pair, oracle_record, perturbation_figure, resamples      # noqa: E402


def main(names):
    worst_all = 0.0
    for name in names:
        X, model, terms = case(name)
        idx = resamples(X)
        n = X.shape[0]
        worst, fine, pivots = 0.0, True, True
        for rows in [np.arange(n)] + [idx[r] for r in range(idx.shape[0])]:
            _, rec = oracle_record(X, model, rows, n)
            m64, mld = mirror_pair(X, model, terms, counts_of(rows, n), rec)
            fine = fine and m64["status"] == 0 and mld["status"] == 0 and bool(np.all(np.isfinite(m64["record"])))
            pivots = pivots and m64["pivots_pass"]
            worst = max(worst, mirror_difference(m64, mld))
        worst_all = max(worst_all, worst)
        print("%-14s N %5d  P %4d  T %d  max |fp64 - longdouble| %.3e   all status 0 and finite: %s   all pivots pass: %s" % (name, n, model.P, len(terms), worst, fine, pivots),
              flush=True)
        assert fine and pivots, name
    print("largest figure: %.3e (the floor of every bar: 1e-12)" % worst_all)


def oracle_figure():
    X, model, terms = case("satisfaction")
    print("satisfaction: the moderated coefficients move by at most %.3e when the oracle's full-sample record moves inside rtol 1e-8 / atol 1e-11 (20 draws)"
          % perturbation_figure(X, model, terms))


if __name__ == "__main__":
    args = sys.argv[1:]
    if "--oracle" in args:
        oracle_figure()
    else:
        main(args or CASES)
