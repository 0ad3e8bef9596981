"""CPU: the geodesic discrepancy d_G -- the NumPy mirror (plspm.modelfit._geodesic, _geodesic_fit) against closed forms, the portable part of the kernel
(csrc/geodesic_core.h) as a stand-alone host program under AddressSanitizer and UndefinedBehaviorSanitizer against the mirror, the inadmissible paths of both,
the declarations of the new C-ABI symbols, and the host surface that needs no device.

The bar between the host program and the mirror is helpers_geodesic.bar: ten times the larger of the two distances from a 40-digit evaluation that
tools/geodesic_floor.py measured per case (the figures: helpers_geodesic.FLOOR_FIGURES), never below 1e-12.  mpmath is needed by that tool only."""
import fnmatch
import functools
import inspect
import os
import re

import numpy as np
import pytest

from helpers_geodesic import FLOOR_FIGURES, bar, comparable, data_sets, host_values, oracle_problem
from helpers_modelfit import PATH, mask_of, population
from helpers_plsc import CASES, dev_blocks
from plspm import _native
from plspm.modelfit import ModelFit, _d_g, _geodesic, _geodesic_fit, _model_fit
from plspm.plsc import _plsc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("plspm_geodesic_enable", "plspm_geodesic_width", "plspm_geodesic_fit", "plspm_geodesic_fetch", "plspm_geodesic_summary", "plspm_geodesic_intervals")
# The cases whose full sample and first resample are admissible under their own masks (lv_33: all 33 two-item blocks factors, the largest common-factor input).
# Under the other cases' own masks the corrected loadings leave no positive definite Sigma on those two data sets: test_own_mask_admissibility_is_what_is_listed.
OWN_MASK_ADMISSIBLE = ("single_items", "mode_b", "nine_predecessors", "lv_33")
INADMISSIBLE = 4


@functools.lru_cache(maxsize=None)
def problems(name, own_mask):
    """The full sample and the first resample of a case with the oracle's fits: [(R, plsc, fit, geo)], the model and the mask."""
    model, factor, sets = data_sets(name, 1)
    mask = mask_of(model, factor).astype(int) if own_mask else np.zeros(model.L, dtype=int)
    return [oracle_problem(rows, model, mask) for rows in sets], model, mask


# ------------------------------------------------------------------ 1. closed forms
def test_two_by_two():
    r = 0.3
    R = np.array([[1.0, r], [r, 1.0]])
    status, phi = _geodesic(R, np.eye(2))                    # the eigenvalues of R^-1: 1 / (1 + r), 1 / (1 - r)
    assert status == 0
    np.testing.assert_allclose(phi, [1 / (1 + r), 1 / (1 - r)], rtol=1e-14)
    np.testing.assert_allclose(_d_g(phi), 0.5 * (np.log1p(r) ** 2 + np.log1p(-r) ** 2), rtol=1e-14)
    status, phi = _geodesic(R, R)
    assert status == 0 and _d_g(phi) <= 1e-30


def test_closed_form_population(tmp_path):
    """The population of tests/test_plsc.py with an all-factor mask and the population weights: Sigma^ = R, so d_G of both models is a sum of squared
    logarithms of 1 +- a few ulp."""
    R, blocks, w, lam, _ = population(np.float64)
    plsc = _plsc(R, w, lam, blocks, "AAA", PATH, [1, 1, 1])
    fit = _model_fit(R, plsc, blocks, PATH, [1, 1, 1])
    geo = _geodesic_fit(R, fit)
    assert geo["status"] == 0 and np.all(np.abs(geo["record"]) <= 1e-24), geo["record"]
    record, eig = host_values(tmp_path, R, plsc, blocks, PATH, [1, 1, 1], "population")
    assert record[2] == 0.0 and record[3] == 7.0 and np.all(np.abs(record[:2]) <= 1e-24), record
    np.testing.assert_allclose(eig, 1.0, rtol=0, atol=1e-13)


def test_identity_needs_no_reflection(tmp_path):
    """One composite block: Sigma^ is R entry by entry.  With R = I the reduced matrix is I exactly and every column below the subdiagonal is zero -- the
    Householder guard; with a correlated R it is I up to rounding, columns of 1e-17 or of exact zeros."""
    for tag, R in (("identity", np.eye(5)), ("correlated", 0.4 * np.ones((5, 5)) + 0.6 * np.eye(5))):
        plsc = {"status": 0, "loadings": np.full(5, 0.7), "lv_cor": np.eye(1), "path": np.zeros((1, 1))}
        record, eig = host_values(tmp_path, R, plsc, [np.arange(5)], np.zeros((1, 1), dtype=int), [0], tag)
        assert record[2] == 0.0 and np.all(np.isfinite(eig)), (tag, record, eig)
        np.testing.assert_allclose(eig, 1.0, rtol=0, atol=1e-14)
        assert np.all(record[:2] <= 1e-28), (tag, record)
    assert np.all(host_values(tmp_path, np.eye(5), plsc, [np.arange(5)], np.zeros((1, 1), dtype=int), [0], "identity")[0][:2] == 0.0)


# ------------------------------------------------------------------ 2. the host program under sanitizers against the mirror
def check_host_against_mirror(tmp_path, name, own_mask):
    sets, model, mask = problems(name, own_mask)
    worst = 0.0
    for k, (R, plsc, fit, geo) in enumerate(sets):
        assert fit["status"] == 0 and geo["status"] == 0, (name, k)
        record, eig = host_values(tmp_path, R, plsc, dev_blocks(model), model.C, mask, "%s_%d" % (name, k))
        assert record[2] == 0.0 and record[3] == 7.0
        diff = float(np.max(np.abs(record[:2] - geo["record"])))
        worst = max(worst, diff)
        assert diff <= bar(name), "%s data set %d: |host program - mirror| %.3e above the bar %.3e" % (name, k, diff, bar(name))
        for row, which in enumerate(("saturated", "estimated")):
            assert np.all(np.diff(eig[row]) >= 0)
            np.testing.assert_allclose(eig[row], geo["phi"][which], rtol=1e-11, atol=0)
    print("%s: max |host program - mirror| %.3e (bar %.3e)" % (name, worst, bar(name)))


@pytest.mark.parametrize("name", CASES)
def test_host_program_against_the_mirror_composites(tmp_path, name):
    assert set(FLOOR_FIGURES) == set(CASES)
    check_host_against_mirror(tmp_path, name, False)
    if name == "single_items":                               # two single items: both models reproduce r_01
        assert np.all(problems(name, False)[0][0][3]["record"] <= 1e-24)


@pytest.mark.parametrize("name", OWN_MASK_ADMISSIBLE)
def test_host_program_against_the_mirror_own_mask(tmp_path, name):
    check_host_against_mirror(tmp_path, name, True)


@pytest.mark.parametrize("name", CASES)
def test_own_mask_admissibility_is_what_is_listed(name):
    """Every case that is admissible under its own mask is in OWN_MASK_ADMISSIBLE, and no data set is near enough to singular to be left out of the device's
    status comparison (helpers_geodesic.comparable asserts the one-in-ten cap on the mirror alone)."""
    sets, _, _ = problems(name, True)
    geos = [geo for _, _, _, geo in sets]
    assert all(comparable(geos)), name
    assert all(geo["status"] == 0 for geo in geos) == (name in OWN_MASK_ADMISSIBLE), (name, [geo["status"] for geo in geos])


# ------------------------------------------------------------------ 3. the inadmissible paths, host program and mirror on the same inputs
def test_implied_matrix_that_is_not_positive_definite(tmp_path):
    sets, model, mask = problems("wave_60x6", True)
    R, plsc, fit, geo = sets[0]
    assert fit["status"] == 0                                # the model fit itself is fine: d_uls needs no positive definite Sigma
    assert geo["status"] == INADMISSIBLE and np.all(np.isnan(geo["record"]))
    assert min(geo["phi"]["saturated"].min(), geo["phi"]["estimated"].min()) < -1e-3
    record, eig = host_values(tmp_path, R, plsc, dev_blocks(model), model.C, mask, "not_definite")
    assert record[2] == float(INADMISSIBLE) and record[3] == 7.0 and np.all(np.isnan(record[:2]))
    np.testing.assert_allclose(eig[0], geo["phi"]["saturated"], rtol=1e-9, atol=1e-11)      # (the eigenvalues themselves are there, negative ones included)


def test_singular_correlation_matrix(tmp_path):
    sets, model, mask = problems("fp64_gram", False)
    R, plsc, _, _ = sets[0]
    Rs = R.copy()
    Rs[1, :], Rs[:, 1] = R[0, :], R[:, 0]                    # column 1 duplicates column 0: r_01 = 1
    Rs[0, 1] = Rs[1, 0] = Rs[1, 1] = 1.0
    blocks = dev_blocks(model)
    fit = _model_fit(Rs, plsc, blocks, model.C, mask)
    geo = _geodesic_fit(Rs, fit)
    assert fit["status"] == 0 and geo["status"] == INADMISSIBLE and np.all(np.isnan(geo["record"])) and geo["phi"]["saturated"] is None
    record, eig = host_values(tmp_path, Rs, plsc, blocks, model.C, mask, "singular")
    assert record[2] == float(INADMISSIBLE) and np.all(np.isnan(record[:2])) and np.all(np.isnan(eig))


def test_status_passes_through_and_not_finite(tmp_path):
    sets, model, mask = problems("fp64_gram", False)
    R, plsc, fit, geo = sets[0]
    blocks = dev_blocks(model)
    record, _ = host_values(tmp_path, R, plsc, blocks, model.C, mask, "singular_regression", status=2)      # the model-fit record's status stands beside finite values
    assert record[2] == 2.0 and np.array_equal(record[:2], host_values(tmp_path, R, plsc, blocks, model.C, mask, "fine")[0][:2])
    Rn = R.copy()
    Rn[0, 5] = Rn[5, 0] = np.nan
    assert _geodesic(Rn, fit["implied"]["saturated"]) == (INADMISSIBLE, None)
    record, _ = host_values(tmp_path, Rn, plsc, blocks, model.C, mask, "not_finite")
    assert record[2] == float(INADMISSIBLE) and np.all(np.isnan(record[:2]))
    bad = dict(fit, status=INADMISSIBLE)
    assert _geodesic_fit(R, bad)["status"] == INADMISSIBLE and np.all(np.isnan(_geodesic_fit(R, bad)["record"]))


# ------------------------------------------------------------------ 4. the surface
def test_new_symbols_are_declared_everywhere():
    header = open(os.path.join(ROOT, "include", "plspm_hip.h")).read()
    declared = set(re.findall(r"\b(plspm_[a-z_]+)\s*\(", header))
    exports_map = open(os.path.join(ROOT, "plspm-python_amd", "csrc", "exports.map")).read()
    pattern = re.search(r"global:\s*([^;]+);", exports_map).group(1).strip()
    lib = _native.load()
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in _native.EXPORTS, name
        assert fnmatch.fnmatchcase(name, pattern), (name, pattern)
        assert hasattr(lib, name), name
    assert lib.plspm_abi_version() == 4 and _native.ABI_VERSION == 4
    assert int(re.search(r"#define PLSPM_ABI_VERSION (\d+)", header).group(1)) == 4


def test_argument_errors_without_a_handle():
    lib = _native.load()
    out = np.zeros(32)
    assert lib.plspm_geodesic_enable(None, 1, None) == 100   # PLSPM_E_ARG
    assert lib.plspm_geodesic_width(None) == 0
    assert lib.plspm_geodesic_fit(None, out.ctypes.data, None) == 100
    assert lib.plspm_geodesic_fetch(None, 0, 1, out.ctypes.data, None) == 100
    assert lib.plspm_geodesic_summary(None, 10, out.ctypes.data, out.ctypes.data, None) == 100
    assert lib.plspm_geodesic_intervals(None, 10, out.ctypes.data, 0, 0.95, out.ctypes.data, None) == 100


def test_keyword_is_off_by_default():
    assert inspect.signature(ModelFit.__init__).parameters["geodesic"].default is False
    for method in ("records", "used", "inadmissible"):
        assert inspect.signature(getattr(ModelFit, method)).parameters["measure"].default is None
