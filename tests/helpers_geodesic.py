"""Shared by the geodesic tests (tests/test_geodesic.py, tests/test_gpu_geodesic.py) and the CPU measurements behind their bars (tools/geodesic_floor.py):
the NumPy mirror of one data set (plspm.modelfit._geodesic_fit on _model_fit on plspm.plsc._plsc), the stand-alone host program of csrc/geodesic_core.h as a
child process, the data sets of a case, and the bars.  The shapes are tests/helpers_plsc.py's."""
import os
import subprocess

import numpy as np

from helpers_modelfit import mirror_fit, oracle_fit
from helpers_plsc import case, resamples
from plspm.modelfit import _geodesic_fit
from plspm.plsc import _effect_pairs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tests", "geodesic_host")

# |d_G - its 40-digit value| (mpmath; tools/geodesic_floor.py floor), the larger of both models, per case over its nine resamples and its full sample with the
# oracle's fits under an all-zero factor mask: (the fp64 mirror, the host program of csrc/geodesic_core.h).
FLOOR_FIGURES = {
    "single_items": (6.715e-32, 9.543e-32),
    "wave_60x6": (5.199e-15, 1.021e-14),
    "quad_120x12": (3.278e-14, 1.022e-13),
    "lds_65_5": (2.450e-15, 4.670e-15),
    "packed_40": (4.236e-15, 5.760e-15),
    "fp64_gram": (8.232e-16, 5.990e-16),
    "mode_b": (8.087e-16, 3.945e-16),
    "nine_predecessors": (8.328e-16, 3.082e-16),
    "lv_33": (5.276e-15, 9.276e-15),
    "mixed_mask": (5.199e-15, 1.021e-14),
}
FLOOR = 1e-12                                       # the project's floor of every mirror bar


def bar(name):
    """The bar between the device and the mirror on a case: ten times the larger of its two figures, never below the project's 1e-12."""
    return max(10.0 * max(FLOOR_FIGURES[name]), FLOOR)


# A replicate whose implied matrix is this close to singular may fall either way on either side: left out of the status comparison, one in ten at most per case.
NEAR_SINGULAR = 1e-6


def mirror_geodesic(Xr, model, w, lam, factor):
    """(geodesic dict, model-fit dict) of the fp64 mirror on the rows Xr (device column order) with the weights w and loadings lam."""
    fit, _ = mirror_fit(Xr, model, w, lam, factor)
    R = np.corrcoef(Xr, rowvar=False).reshape(Xr.shape[1], Xr.shape[1])
    return _geodesic_fit(R, fit), fit


def smallest_phi(geo):
    """The smallest |phi_k| of both models in a mirror's geodesic dict (inf where there are none: the model fit itself is inadmissible, or R is singular)."""
    values = [np.min(np.abs(phi)) for phi in geo["phi"].values() if phi is not None]
    return float(min(values)) if values else np.inf


def comparable(geos):
    """Which of the mirror's geodesic dicts of one case take part in the status comparison with the device: [bool].  One whose smallest |phi_k| is below
    NEAR_SINGULAR is left out -- and this asserts, on the mirror alone, that at most one data set in ten is (none of fewer than ten)."""
    keep = [smallest_phi(geo) >= NEAR_SINGULAR for geo in geos]
    left_out = keep.count(False)
    assert left_out <= len(geos) // 10, "%d of %d data sets are within %.0e of singular in the mirror: more than one in ten" % (left_out, len(geos), NEAR_SINGULAR)
    return keep


def data_sets(name, B=9):
    """The rows (data column order) of a case's full sample and of its B resamples."""
    X, model, _, _, _, factor = case(name)
    idx = resamples(X, B)
    return model, factor, [X] + [X[idx[r]] for r in range(B)]


def oracle_problem(rows, model, factor):
    """One data set (data column order) with the oracle's fit: (R, plsc dict, model-fit dict, geodesic dict) of the mirror; factor None: PLSc's default mask."""
    w, lam, _ = oracle_fit(rows, model)
    Xr = rows[:, model.mv_order]
    fit, plsc = mirror_fit(Xr, model, w, lam, factor)
    R = np.corrcoef(Xr, rowvar=False).reshape(model.P, model.P)
    return R, plsc, fit, _geodesic_fit(R, fit)


def host_text(R, plsc, blocks, C, factor, status, iterations=7):
    P, L = R.shape[0], len(blocks)
    pairs = _effect_pairs(C)
    boff = np.concatenate(([0], np.cumsum([len(b) for b in blocks])))
    numbers = lambda a: " ".join(repr(float(x)) for x in np.asarray(a, dtype=np.float64).ravel())      # noqa: E731
    return "\n".join(["%d %d" % (P, L), " ".join(str(int(x)) for x in boff), " ".join(str(int(x)) for x in np.asarray(C).ravel()),
                      " ".join(str(int(x)) for x in factor), numbers(plsc["loadings"]), numbers(plsc["lv_cor"][np.triu_indices(L, 1)]),
                      numbers([plsc["path"][t, f] for f, t in pairs]), numbers(R), "%d %d" % (status, iterations)]) + "\n"


def host_values(directory, R, plsc, blocks, C, factor, tag, status=0):
    """What csrc/geodesic_core.h computes from the mirror's PLSc estimates: written as text, run as a child process under the sanitizers.
    (record [4]: d_g_sat, d_g_est, status, iterations; eigenvalues [2, P])"""
    subprocess.check_call(["make", "-s", "-C", HOST, "geodesic_host"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    path = os.path.join(str(directory), tag + ".txt")
    with open(path, "w") as f:
        f.write(host_text(R, plsc, blocks, C, np.asarray(factor).astype(int), status))
    run = subprocess.run([os.path.join(HOST, "geodesic_host"), path], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr
    assert "ERROR" not in run.stderr and "runtime error" not in run.stderr, run.stderr
    P = R.shape[0]
    values = np.array([float(x) for x in run.stdout.split()])
    assert values.shape == (4 + 2 * P,)
    return values[:4], values[4:].reshape(2, P)
