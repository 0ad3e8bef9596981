"""CPU: the host surface of the bootstrap confidence intervals and the jackknife -- the NumPy mirrors of the kernels (plspm.bootstrap._intervals,
_jackknife_stats) against a direct SciPy restatement (tests/helpers_ci.py) and closed forms, the NaN rules, and the declarations of the new C-ABI
symbols."""
import os
import re

import numpy as np
import pandas as pd
import pytest

from helpers_ci import intervals as ref_intervals, jackknife_stats as ref_jackknife_stats, levels
from plspm import _native
from plspm.bootstrap import INTERVAL_METHODS, _ci_levels, _create_summary, _intervals, _jackknife_stats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("plspm_jackknife_device", "plspm_jackknife_fetch", "plspm_jackknife_stats", "plspm_bootstrap_intervals")


def _samples(seed, m, R=7):
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((m, R)) * rng.uniform(0.05, 4.0, R) + rng.uniform(-2.0, 2.0, R)
    v[:, 3] = np.exp(v[:, 3] / 4.0)                        # a skewed column
    original = v.mean(axis=0) + rng.uniform(-0.3, 0.3, R) * v.std(axis=0)
    accel = rng.uniform(-0.08, 0.08, R)
    return v, original, accel


def _check(mine, ref):
    assert mine.shape == ref.shape
    assert np.array_equal(np.isnan(mine), np.isnan(ref))
    np.testing.assert_allclose(mine[:, :2], ref[:, :2], rtol=1e-9, atol=0)
    np.testing.assert_allclose(mine[:, 2:], ref[:, 2:], rtol=0, atol=1e-12)


@pytest.mark.parametrize("method", INTERVAL_METHODS)
@pytest.mark.parametrize("m", [1, 2, 40, 1001])
@pytest.mark.parametrize("level", [0.9, 0.95, 0.99])
def test_intervals_against_the_scipy_restatement(method, m, level):
    v, original, accel = _samples(m, m)
    _check(_intervals(v, original, accel, method, level), ref_intervals(v, original, method, level, accel))


@pytest.mark.parametrize("level", [0.5, 0.8, 0.9, 0.95, 0.99, 0.999])
def test_levels_are_exact_decimals(level):
    assert _ci_levels(level) == levels(level)
    assert _ci_levels(0.95) == (0.025, 0.975)


@pytest.mark.parametrize("m", [1, 2, 3, 40, 999])
def test_percentile_at_095_is_the_summary(m):
    v, original, _ = _samples(11, m)
    out = _intervals(v, original, None, "percentile", 0.95)
    summary = _create_summary(pd.DataFrame(v), original)
    assert np.array_equal(out[:, 0], summary["perc.025"].values)
    assert np.array_equal(out[:, 1], summary["perc.975"].values)


def test_basic_is_the_reflection_of_percentile():
    v, original, _ = _samples(5, 300)
    pct, bas = _intervals(v, original, None, "percentile", 0.9), _intervals(v, original, None, "basic", 0.9)
    assert np.array_equal(bas[:, 0], 2.0 * original - pct[:, 1])
    assert np.array_equal(bas[:, 1], 2.0 * original - pct[:, 0])
    assert np.array_equal(bas[:, 2:], pct[:, 2:], equal_nan=True)


def test_bc_is_bca_with_zero_acceleration():
    v, original, _ = _samples(6, 300)
    assert np.array_equal(_intervals(v, original, None, "bc", 0.95), _intervals(v, original, np.zeros(v.shape[1]), "bca", 0.95), equal_nan=True)
    with pytest.raises(ValueError, match="needs the acceleration"):
        _intervals(v, original, None, "bca", 0.95)
    with pytest.raises(ValueError, match="method must be one of"):
        _intervals(v, original, None, "student", 0.95)
    for level in (0.0, 1.0, 1.5):
        with pytest.raises(ValueError, match="level must lie"):
            _intervals(v, original, None, "percentile", level)


@pytest.mark.parametrize("method", INTERVAL_METHODS)
def test_intervals_widen_with_the_level(method):
    v, original, accel = _samples(8, 500)
    prev = None
    for level in (0.5, 0.8, 0.9, 0.95, 0.99):
        out = _intervals(v, original, accel, method, level)
        assert np.all(out[:, 0] <= out[:, 1])
        if prev is not None:
            assert np.all(out[:, 0] <= prev[:, 0]) and np.all(out[:, 1] >= prev[:, 1])
            assert np.all(out[:, 4] <= prev[:, 4]) and np.all(out[:, 5] >= prev[:, 5])
        prev = out


def test_nan_rules():
    v, original, accel = _samples(9, 60, R=6)
    v[:, 0] = 0.0; original[0] = 0.0                       # a constant column (an absent path): proportion 0
    v[:, 1] = original[1] - 1.0 - np.abs(v[:, 1])          # every replicate below the estimate: proportion 1
    original[2] = np.nan
    accel[3] = np.nan
    for method in INTERVAL_METHODS:
        out = _intervals(v, original, accel, method, 0.95)
        assert np.all(np.isnan(out[2]))                    # original NaN: all six
        adjusted = method in ("bc", "bca")
        for c, z0 in ((0, -np.inf), (1, np.inf)):
            assert out[c, 2] == z0
            assert np.all(np.isnan(out[c, [0, 1, 4, 5]])) == adjusted
            assert not adjusted or np.all(np.isnan(out[c, [0, 1, 4, 5]]))
        if method == "bca":
            assert np.all(np.isnan(out[3, [0, 1, 3, 4, 5]])) and np.isfinite(out[3, 2])
        else:
            assert np.all(np.isfinite(out[3, [0, 1, 2, 4, 5]]))
        assert np.all(np.isfinite(out[4:, [0, 1, 2, 4, 5]]))
        empty = _intervals(v[:0], original, accel, method, 0.95)
        assert empty.shape == (6, 6) and np.all(np.isnan(empty))


def test_a_large_acceleration_drives_a_level_to_the_end_of_the_sample():
    v, original, _ = _samples(10, 50, R=4)
    z0 = _intervals(v, original, None, "percentile", 0.95)[:, 2]
    z = 1.959963984540054                                   # Phi^-1(0.975)
    accel = np.array([0.999 / (z0[0] + z), 0.999 / (z0[1] - z), 0.0, 0.01])      # 1 - a (z0 + z) = 0.001: the adjusted level is Phi(+-1000 or so)
    out = _intervals(v, original, accel, "bca", 0.95)
    assert out[0, 5] == 1.0 and out[0, 1] == v[:, 0].max()
    assert out[1, 4] == 0.0 and out[1, 0] == v[:, 1].min()
    _check(out, ref_intervals(v, original, "bca", 0.95, accel))


# ------------------------------------------------------------------ jackknife statistics
def test_jackknife_stats_closed_forms_for_the_sample_mean():
    """theta = the sample mean: theta_(g) = (n xbar - x_g) / (n - 1), so se_jk = sd / sqrt(n) and accel = skewness / (6 sqrt(n))."""
    rng = np.random.default_rng(3)
    n = 250
    x = np.column_stack((rng.standard_normal(n), rng.exponential(2.0, n), rng.uniform(-1, 1, n) ** 3))
    loo = (x.sum(axis=0)[None, :] - x) / (n - 1)
    mean, se, accel = _jackknife_stats(loo)
    np.testing.assert_allclose(mean, x.mean(axis=0), rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(se, x.std(axis=0, ddof=1) / np.sqrt(n), rtol=1e-10)
    dev = x - x.mean(axis=0)
    skew = (dev ** 3).mean(axis=0) / (dev ** 2).mean(axis=0) ** 1.5
    np.testing.assert_allclose(accel, skew / (6.0 * np.sqrt(n)), rtol=1e-9, atol=1e-12)
    ref = ref_jackknife_stats(loo)
    for mine, theirs in zip((mean, se, accel), ref):
        np.testing.assert_allclose(mine, theirs, rtol=1e-12, atol=1e-12)


def test_jackknife_stats_edge_cases():
    mean, se, accel = _jackknife_stats(np.zeros((0, 4)))
    assert np.all(np.isnan(mean)) and np.all(np.isnan(se)) and np.all(np.isnan(accel))
    rec = np.column_stack((np.full(9, 0.25), np.arange(9.0), np.full(9, np.nan)))
    mean, se, accel = _jackknife_stats(rec)
    assert mean[0] == 0.25 and se[0] == 0.0 and np.isnan(accel[0])           # a constant column: sum d^2 = 0
    assert mean[1] == 4.0 and abs(accel[1]) < 1e-15 and se[1] > 0            # a symmetric column: no acceleration
    assert np.isnan(mean[2]) and np.isnan(se[2]) and np.isnan(accel[2])


# ------------------------------------------------------------------ the C-ABI's declarations
def test_new_symbols_are_declared_everywhere():
    header = open(os.path.join(ROOT, "include", "plspm_hip.h")).read()
    declared = set(re.findall(r"\b(plspm_[a-z_]+)\s*\(", header))
    exports_map = open(os.path.join(ROOT, "plspm-python_amd", "csrc", "exports.map")).read()
    pattern = re.search(r"global:\s*([^;]+);", exports_map).group(1).strip()
    import fnmatch
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in _native.EXPORTS, name
        assert fnmatch.fnmatchcase(name, pattern), (name, pattern)
    lib = _native.load()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
    assert lib.plspm_abi_version() == 4
    # the LDS capacity the tests of the intervals kernel cross is the launch code's
    kernels = open(os.path.join(ROOT, "plspm-python_amd", "csrc", "kernels_intervals.h")).read()
    assert int(re.search(r"CI_LDS_VALUES\s*=\s*(\d+)", kernels).group(1)) == _native.CI_LDS_VALUES


def test_argument_errors_without_a_handle():
    lib = _native.load()
    out = np.zeros(6)
    assert lib.plspm_bootstrap_intervals(None, None, 10, 0, out.ctypes.data, None, 0, 0.95, out.ctypes.data, None) == 100      # PLSPM_E_ARG
    assert lib.plspm_jackknife_device(None, 5, None, None, None) == 100
    assert lib.plspm_jackknife_fetch(None, 0, 1, None, None, None) == 100
    assert lib.plspm_jackknife_stats(None, 5, None, None, None, None) == 100
