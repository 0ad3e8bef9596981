"""CPU: the figures behind the bars of tests/test_gpu_structural.py.  For every case of tests/helpers_structural.py, on its nine resamples and on all rows,
with the ORACLE's construct correlations and direct effects in place of the device's: the largest |fp64 mirror - longdouble mirror| over the structural
record (plspm.structural._structural), whether every data set has status 0 and finite values, and whether every regression passes the pivot test.  The
floor of the bar is the largest of these differences, never below 1e-12.  With `--oracle`: for the satisfaction case, how far the statistics move when the
oracle's records move inside the record bar (helpers_structural.perturbation_figure), and how far the least-squares statistics of the oracle's scores are
from the mirror's on the oracle's records.

    python tools/structural_floor.py [--oracle] [case ...]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "plspm-python_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]

from helpers_structural import (CASES, case, lstsq_statistics, mirror_difference, mirror_pair, oracle_fit_record, oracle_lv_cor, perturbation_figure,      # noqa: E402
                                record_direct, resamples)


def main(names):
    worst_all = 0.0
    for name in names:
        X, model = case(name)
        idx = resamples(X)
        worst, fine, pivots, n_dir, n_spec = 0.0, True, True, 0, 0
        for rows in [np.arange(X.shape[0])] + [idx[r] for r in range(idx.shape[0])]:
            _, rec = oracle_fit_record(X, model, rows, X.shape[0])
            lv_cor = oracle_lv_cor(X[rows][:, model.mv_order], model, rec[:model.P], rec[-model.P:])
            m64, mld = mirror_pair(model, lv_cor, record_direct(model, rec))
            fine = fine and m64["status"] == 0 and mld["status"] == 0 and bool(np.all(np.isfinite(m64["record"])))
            pivots = pivots and m64["pivots_pass"]
            worst = max(worst, mirror_difference(m64, mld))
            n_dir, n_spec = len(m64["paths"]), len(m64["chains"])
        worst_all = max(worst_all, worst)
        print("%-14s n_dir %3d  n_spec %4d  max |fp64 - longdouble| %.3e   all status 0 and finite: %s   all pivots pass: %s" % (name, n_dir, n_spec, worst, fine, pivots),
              flush=True)
    print("floor: max(%.3e, 1e-12)" % worst_all)


def oracle_figures():
    X, model = case("satisfaction")
    idx = resamples(X)
    print("satisfaction: the statistics move by at most %.3e when the oracle's records move inside rtol 1e-8 / atol 1e-11 (20 draws per resample)"
          % perturbation_figure(X, model, idx))
    worst = 0.0
    for r in range(idx.shape[0]):
        f, rec = oracle_fit_record(X, model, idx[r], X.shape[0])
        lv_cor = oracle_lv_cor(X[idx[r]][:, model.mv_order], model, rec[:model.P], rec[-model.P:])
        m64, _ = mirror_pair(model, lv_cor, record_direct(model, rec))
        worst = max(worst, float(np.max(np.abs(lstsq_statistics(model, f["scores"], f["path_coef"]) - m64["record"]))))
    print("satisfaction: least squares on the oracle's scores against the mirror on the oracle's records: max |difference| %.3e" % worst)


if __name__ == "__main__":
    args = sys.argv[1:]
    if "--oracle" in args:
        oracle_figures()
    else:
        main(args or CASES)
