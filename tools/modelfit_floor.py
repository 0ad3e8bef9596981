"""CPU: the figures behind the bars of tests/test_gpu_modelfit.py.

floor      for every case of tests/helpers_plsc.py, on its nine resamples and on all rows, with the ORACLE's weights and loadings in place of the device's: the
           largest |fp64 mirror - longdouble mirror| over the model-fit record (plspm.modelfit._model_fit), and whether every resample is admissible.  The
           floor of the kernel-against-mirror bar is the largest of these, never below 1e-12.
oracle     satisfaction, 20 resamples: the largest movement of a statistic when the oracle's weights and loadings are perturbed inside the project's record bar
           (rtol 1e-8, atol 1e-11; 20 draws each).  The bar of the comparison with the oracle's fits is ten times that.
transform  the all-factor model on the Bollen-Stine transform of satisfaction (null: the estimated model): srmr_est of the mirror on the oracle's fit of the
           transformed rows.  PLSc recovers Lambda and Phi from the implied matrix up to the iteration's stop tolerance.
power      seeds for the test that the test does its job: 300 Gaussian rows from the closed-form population, the correct model and the model without 0 -> 2,
           an oracle-driven bootstrap of the transformed rows (the mirror on the oracle's fits, 200 resamples): the p-values.

    python tools/modelfit_floor.py [floor|oracle|transform|power ...] [seed=N]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "plspm-python_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]

import plspm_oracle as orc                                     # noqa: E402
from helpers import satisfaction_oracle_inputs                 # noqa: E402
from helpers_modelfit import (PATH, PATH_WITHOUT_02, mirror_difference, mirror_fit_pair, oracle_fit, oracle_model_fit, perturbation_bar,      # noqa: E402
                              population_model, population_sample)
from helpers_plsc import CASES, case, resamples                # noqa: E402
from plspm.modelfit import _bollen_stine                       # noqa: E402


def floor():
    worst_all = 0.0
    for name in CASES:
        X, model, _, _, _, factor = case(name)
        idx = resamples(X)
        worst, admissible = 0.0, True
        for rows in [X] + [X[idx[r]] for r in range(idx.shape[0])]:
            w, lam, _ = oracle_fit(rows, model)
            m64, mld = mirror_fit_pair(rows[:, model.mv_order], model, w, lam, factor)
            admissible = admissible and m64["status"] == 0 and mld["status"] == 0
            if m64["status"] == 0 and mld["status"] == 0:
                worst = max(worst, mirror_difference(m64, mld))
        worst_all = max(worst_all, worst)
        print("%-18s max |fp64 - longdouble| %.3e   all admissible: %s" % (name, worst, admissible), flush=True)
    print("floor: max(%.3e, 1e-12)" % worst_all)


def satisfaction():
    X, blocks, _ = satisfaction_oracle_inputs()
    return X, orc.Model(blocks, orc.satisfaction_C(), "AAAAAA", "path", True)


def oracle():
    X, model = satisfaction()
    idx = resamples(X, 20, seed=11)
    worst = 0.0
    for r in range(idx.shape[0]):
        rows = X[idx[r]]
        w, lam, _ = oracle_fit(rows, model)
        worst = max(worst, perturbation_bar(rows[:, model.mv_order], model, w, lam, None) / 10.0)
    print("oracle: largest movement of a statistic under a perturbation inside the record bar %.3e (bar: ten times that)" % worst)


def transform():
    X, model = satisfaction()
    fit = oracle_model_fit(X, model, None)
    Xt = np.empty_like(X)
    Xt[:, model.mv_order] = _bollen_stine(X[:, model.mv_order], fit["implied"]["estimated"])
    again = oracle_model_fit(Xt, model, None)
    print("transform: observed srmr_est %.6f; on the transformed rows srmr_est %.3e, d_uls_est %.3e (status %d)" % (fit["srmr_est"], again["srmr_est"], again["d_uls_est"], again["status"]))


def p_value(X, C, resamples_n=200, seed=1):
    """The oracle-driven Bollen-Stine bootstrap of d_uls_est: (p, observed, 99 % quantile, used)."""
    model = population_model(C)
    factor = [1, 1, 1]
    fit = oracle_model_fit(X, model, factor)
    Xt = _bollen_stine(X, fit["implied"]["estimated"])
    rng = np.random.default_rng(seed)
    stars = []
    for _ in range(resamples_n):
        try:
            f = oracle_model_fit(Xt[rng.integers(0, X.shape[0], X.shape[0])], model, factor)
        except orc.NotConverged:
            continue
        if f["status"] == 0:
            stars.append(float(f["d_uls_est"]))
    stars = np.array(stars)
    return (1.0 + np.count_nonzero(stars >= fit["d_uls_est"])) / (1.0 + stars.size), float(fit["d_uls_est"]), float(np.quantile(stars, 0.99)), stars.size


def power(seed):
    X = population_sample(300, seed)
    for label, C in (("correct model", PATH), ("model without 0 -> 2", PATH_WITHOUT_02)):
        p, observed, q99, used = p_value(X, C)
        print("power seed %d, %-22s d_uls_est %.5f   p %.4f   99 %% quantile %.5f   used %d (smallest possible p %.4f)" % (seed, label, observed, p, q99, used, 1.0 / (1.0 + used)), flush=True)


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if "=" not in a] or ["floor", "oracle", "transform", "power"]
    seed = int(dict(a.split("=") for a in sys.argv[1:] if "=" in a).get("seed", 3))
    for what in args:
        {"floor": floor, "oracle": oracle, "transform": transform, "power": lambda: power(seed)}[what]()
