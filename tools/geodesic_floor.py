"""CPU: the figures behind the bars of tests/test_gpu_geodesic.py and tests/test_geodesic.py (needs mpmath; the tests do not).

floor      for every case of tests/helpers_plsc.py under an all-zero factor mask, on its nine resamples and on all rows, with the ORACLE's fits: d_G of both
           models evaluated in 40 digits (mpmath: Cholesky of R, G^-1 Sigma G^-T, its eigenvalues, 1/2 sum ln^2) on the fp64 R and the fp64 mirror's implied
           matrices, and against it the fp64 mirror (plspm.modelfit._geodesic) and the stand-alone host program of csrc/geodesic_core.h.  Two figures per
           case: max |mirror - 40-digit| and max |host program - 40-digit|.  The bar between device and mirror is ten times the larger, never below 1e-12
           (tests/helpers_geodesic.py FLOOR_FIGURES).
transform  the all-factor model on the Bollen-Stine transform of satisfaction (null: the estimated model): d_g_est of the mirror on the oracle's fit of the
           transformed rows -- the near-identity case of the Householder guard.
power      seeds 1..6 for the test that the test does its job: 300 Gaussian rows from the closed-form population, the correct model and the model without
           0 -> 2, an oracle-driven bootstrap of the transformed rows (the mirror on the oracle's fits, 200 resamples): the p-values of d_g_est.

    python tools/geodesic_floor.py [floor|transform|power ...] [case=NAME]
"""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "plspm-python_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]

import plspm_oracle as orc                                     # noqa: E402
from helpers import satisfaction_oracle_inputs                 # noqa: E402
from helpers_geodesic import data_sets, host_values, oracle_problem      # noqa: E402
from helpers_modelfit import PATH, PATH_WITHOUT_02, population_model, population_sample      # noqa: E402
from helpers_plsc import CASES, dev_blocks                     # noqa: E402
from plspm.modelfit import _bollen_stine                       # noqa: E402


def d_g_40_digits(R, implied):
    import mpmath as mp
    mp.mp.dps = 40
    P = R.shape[0]
    G = mp.cholesky(mp.matrix(R.tolist()))
    Ginv = mp.inverse(G)
    C = Ginv * mp.matrix(implied.tolist()) * Ginv.T
    C = (C + C.T) / 2
    phi = mp.eigsy(C, eigvals_only=True)
    return sum(mp.log(phi[k]) ** 2 for k in range(P)) / 2


def floor(only=None):
    tmp = tempfile.mkdtemp()
    for name in CASES:
        if only and name != only:
            continue
        model, _, sets = data_sets(name)
        zero = np.zeros(model.L, dtype=int)
        worst_mirror, worst_host, largest = 0.0, 0.0, 0.0
        for k, rows in enumerate(sets):
            R, plsc, fit, geo = oracle_problem(rows, model, zero)
            assert fit["status"] == 0 and geo["status"] == 0, (name, k)
            record, _ = host_values(tmp, R, plsc, dev_blocks(model), model.C, zero, "%s_%d" % (name, k))
            assert record[2] == 0.0
            for column, which in enumerate(("saturated", "estimated")):
                exact = d_g_40_digits(R, fit["implied"][which])
                worst_mirror = max(worst_mirror, abs(float(geo["record"][column] - exact)))
                worst_host = max(worst_host, abs(float(record[column] - exact)))
                largest = max(largest, float(exact))
        print("%-18s P %3d  largest d_G %8.4f   max |mirror - 40-digit| %.3e   max |host program - 40-digit| %.3e" % (name, model.P, largest, worst_mirror, worst_host), flush=True)


def satisfaction():
    X, blocks, _ = satisfaction_oracle_inputs()
    return X, orc.Model(blocks, orc.satisfaction_C(), "AAAAAA", "path", True)


def transform():
    X, model = satisfaction()
    _, _, fit, geo = oracle_problem(X, model, None)
    Xt = np.empty_like(X)
    Xt[:, model.mv_order] = _bollen_stine(X[:, model.mv_order], fit["implied"]["estimated"])
    _, _, again, geo_t = oracle_problem(Xt, model, None)
    print("transform: observed d_g %s (status %d); on the transformed rows d_g_sat %.3e, d_g_est %.3e (status %d), srmr_est %.3e" %
          (geo["record"], geo["status"], geo_t["record"][0], geo_t["record"][1], geo_t["status"], again["srmr_est"]))


def p_value(X, C, resamples_n=200, seed=1):
    """The oracle-driven Bollen-Stine bootstrap of d_g_est: (p, observed, 99 % quantile, used)."""
    model = population_model(C)
    factor = [1, 1, 1]
    _, _, fit, geo = oracle_problem(X, model, factor)
    assert geo["status"] == 0
    Xt = _bollen_stine(X, fit["implied"]["estimated"])
    rng = np.random.default_rng(seed)
    stars = []
    for _ in range(resamples_n):
        try:
            g = oracle_problem(Xt[rng.integers(0, X.shape[0], X.shape[0])], model, factor)[3]
        except orc.NotConverged:
            continue
        if g["status"] == 0:
            stars.append(float(g["record"][1]))
    stars = np.array(stars)
    observed = float(geo["record"][1])
    return (1.0 + np.count_nonzero(stars >= observed)) / (1.0 + stars.size), observed, float(np.quantile(stars, 0.99)), stars.size


def power():
    for seed in range(1, 7):
        X = population_sample(300, seed)
        for label, C in (("correct model", PATH), ("model without 0 -> 2", PATH_WITHOUT_02)):
            p, observed, q99, used = p_value(X, C)
            print("power seed %d, %-22s d_g_est %.5f   p %.4f   99 %% quantile %.5f   used %d (smallest possible p %.4f)" % (seed, label, observed, p, q99, used, 1.0 / (1.0 + used)), flush=True)


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if "=" not in a] or ["floor", "transform", "power"]
    only = dict(a.split("=") for a in sys.argv[1:] if "=" in a).get("case")
    for what in args:
        {"floor": lambda: floor(only), "transform": transform, "power": power}[what]()
