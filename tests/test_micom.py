"""CPU: the host surface of MICOM -- the NumPy mirror of the MICOM record (plspm.micom._micom) on hand-checkable inputs, the frames built from a record
and its quantiles, the argument checks of Micom that raise before the device is touched, and the declarations of the new C-ABI symbols."""
import fnmatch
import os
import re

import numpy as np
import pandas as pd
import pytest

import plspm.config as c
from plspm import _native
from plspm.micom import Micom, _frames, _micom, _p_values
from plspm.mode import Mode
from plspm.scale import Scale

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("plspm_micom_enable", "plspm_micom_width", "plspm_micom_fetch", "plspm_micom_summary", "plspm_micom_intervals", "plspm_micom_counts")
BLOCKS = [np.arange(0, 3), np.arange(3, 7)]


def two_block_data(seed=0, n=240):
    rng = np.random.default_rng(seed)
    lv = rng.standard_normal((n, 2))
    X = np.concatenate([0.8 * lv[:, [0]] + 0.6 * rng.standard_normal((n, 3)), 0.7 * lv[:, [1]] + 0.7 * rng.standard_normal((n, 4))], axis=1) + rng.uniform(-2, 2, 7)
    member = np.zeros(n, dtype=bool)
    member[rng.permutation(n)[:90]] = True
    return X, member, rng


@pytest.mark.parametrize("dtype", [np.float64, np.longdouble])
def test_identical_standardised_weights_give_c_one(dtype):
    X, member, rng = two_block_data()
    v = rng.uniform(0.2, 1.0, 7)
    # the same standardised weights v = w s in both groups (a per-group constant on top cancels): the two composites are one
    w_a, w_b = v / X[member].std(axis=0), 3.0 * v / X[~member].std(axis=0)
    rec = _micom(X, member, w_a, w_b, rng.uniform(0.2, 1.0, 7), BLOCKS, dtype)
    assert rec.dtype == np.dtype(dtype) and rec.shape == (6,)
    np.testing.assert_allclose(rec[:2].astype(np.float64), 1.0, rtol=0, atol=4e-16)
    # one group's weights negated: the composites are opposite, and c carries the sign
    rec = _micom(X, member, -w_a, w_b, np.ones(7), BLOCKS, dtype)
    np.testing.assert_allclose(rec[:2].astype(np.float64), -1.0, rtol=0, atol=4e-16)
    # exactly equal group data and weights: exactly 1
    Y = np.concatenate((X[:100], X[:100]))
    half = np.arange(200) < 100
    assert np.all(_micom(Y, half, v, v, v, BLOCKS, dtype)[:2] == 1.0)
    assert np.all(_micom(Y, half, v, v, v, BLOCKS, dtype)[2:] == 0.0)


def pooled_u(X, w_0, blocks):
    """u = v_0 / s_0 with v_0 = w_0 s_0 normalised per block so that v_0' R_0 v_0 = 1 -- from the definition."""
    s_0 = X.std(axis=0)
    R_0 = np.corrcoef(X, rowvar=False)
    u = np.empty(X.shape[1])
    for cols in blocks:
        v = w_0[cols] * s_0[cols]
        u[cols] = v / np.sqrt(v @ R_0[np.ix_(cols, cols)] @ v) / s_0[cols]
    return u


def test_dmean_and_dlogvar_are_the_pooled_composites():
    X, member, rng = two_block_data(3)
    w_a, w_b, w_0 = (rng.uniform(0.2, 1.0, 7) for _ in range(3))
    rec = _micom(X, member, w_a, w_b, w_0, BLOCKS)
    u = pooled_u(X, w_0, BLOCKS)
    for l, cols in enumerate(BLOCKS):
        y = X[:, cols] @ u[cols]
        np.testing.assert_allclose(np.var(y), 1.0, rtol=1e-13)
        np.testing.assert_allclose(rec[2 + l], y[member].mean() - y[~member].mean(), rtol=0, atol=1e-13)
        np.testing.assert_allclose(rec[4 + l], np.log(y[member].var(ddof=1) / y[~member].var(ddof=1)), rtol=0, atol=1e-13)


def test_a_constant_shift_of_one_group_moves_dmean_only():
    """A constant added to group a's rows leaves the group's own covariances and sds -- hence v_a, v_b, u' C_a u, u' C_b u for a given u -- where they were and
    moves mu_a by the shift: dmean moves by u' shift, c and dlogvar do not see the shift but through the pooled s_0 and R_0.  With one item per block those
    cancel as well: c and dlogvar stay put exactly and dmean s_0 moves by the shift."""
    X, member, rng = two_block_data(5)
    w_a, w_b, w_0 = (rng.uniform(0.2, 1.0, 7) for _ in range(3))
    shift = rng.uniform(-1.0, 1.0, 7)
    Xs = X.copy()
    Xs[member] += shift
    moved = _micom(Xs, member, w_a, w_b, w_0, BLOCKS)
    u = pooled_u(Xs, w_0, BLOCKS)
    R_0 = np.corrcoef(Xs, rowvar=False)
    A, B = X[member], X[~member]                              # the UNSHIFTED groups
    v_a, v_b = w_a * A.std(axis=0), w_b * B.std(axis=0)
    C_a, C_b = np.cov(A, rowvar=False, ddof=1), np.cov(B, rowvar=False, ddof=1)
    for l, cols in enumerate(BLOCKS):
        R = R_0[np.ix_(cols, cols)]
        np.testing.assert_allclose(moved[l], v_a[cols] @ R @ v_b[cols] / np.sqrt((v_a[cols] @ R @ v_a[cols]) * (v_b[cols] @ R @ v_b[cols])), rtol=0, atol=1e-13)
        np.testing.assert_allclose(moved[2 + l], u[cols] @ (A.mean(axis=0) - B.mean(axis=0))[cols] + u[cols] @ shift[cols], rtol=0, atol=1e-13)
        ua, ub = u[cols] @ C_a[np.ix_(cols, cols)] @ u[cols], u[cols] @ C_b[np.ix_(cols, cols)] @ u[cols]
        np.testing.assert_allclose(moved[4 + l], np.log(ua) - np.log(ub), rtol=0, atol=1e-13)
    single = [np.array([0]), np.array([1])]
    X1 = X[:, [0, 3]]
    X2 = X1.copy()
    d = np.array([0.75, -1.25])
    X2[member] += d
    w = np.ones(2)
    r1, r2 = _micom(X1, member, w, w, w, single), _micom(X2, member, w, w, w, single)
    np.testing.assert_allclose(np.concatenate((r1[:2], r2[:2])), 1.0, rtol=0, atol=4e-16)
    np.testing.assert_allclose(r2[4:], r1[4:], rtol=0, atol=1e-13)
    np.testing.assert_allclose(r2[2:4] * X2.std(axis=0), r1[2:4] * X1.std(axis=0) + d, rtol=0, atol=1e-13)


def test_scaling_one_group_by_two_gives_log_four():
    rng = np.random.default_rng(11)
    n = 200
    Y = rng.standard_normal((n, 5)) @ rng.uniform(-1, 1, (5, 5))
    Y -= Y.mean(axis=0)
    X = np.concatenate((2.0 * Y, Y))                         # group a = the rows of group b times 2 (both centred: a scaling of the rows about their mean)
    member = np.arange(2 * n) < n
    blocks = [np.arange(0, 2), np.arange(2, 5)]
    w_0 = rng.uniform(0.2, 1.0, 5)
    rec = _micom(X, member, rng.uniform(0.2, 1, 5), rng.uniform(0.2, 1, 5), w_0, blocks)
    np.testing.assert_allclose(rec[4:], np.log(4.0), rtol=0, atol=1e-13)
    np.testing.assert_allclose(rec[2:4], 0.0, rtol=0, atol=1e-13)
    # the same group weights on proportional data: v_a = 2 v_b, c = 1
    wa = rng.uniform(0.2, 1, 5)
    np.testing.assert_allclose(_micom(X, member, wa, wa, w_0, blocks)[:2], 1.0, rtol=0, atol=4e-16)


def test_frames_follow_their_defining_comparisons():
    lvs = ["X", "Y"]
    observed = np.array([0.99, 0.90, 0.1, -0.5, 0.0, np.nan])
    quantile = np.array([0.95, 0.95])
    lower = np.array([np.nan, np.nan, -0.2, -0.2, -0.3, -0.3])
    upper = np.array([np.nan, np.nan, 0.2, 0.2, 0.3, 0.3])
    p = _p_values(observed, np.array([40, 2, 0, 0, 0, 0]), np.array([0, 0, 30, 1, 99, 0]), 99, 2)
    np.testing.assert_allclose(p[:5], [0.41, 0.03, 0.31, 0.02, 1.0])
    assert np.isnan(p[5])
    f = _frames(lvs, observed, p, quantile, lower, upper)
    assert list(f["compositional"].columns) == ["c", "quantile", "p.value", "invariant"]
    assert list(f["means"].columns) == list(f["variances"].columns) == ["diff", "lower", "upper", "p.value", "equal"]
    assert list(f["summary"].columns) == ["compositional", "equal.means", "equal.variances", "invariance"]
    assert list(f["compositional"]["invariant"]) == [True, False]
    assert list(f["means"]["equal"]) == [True, False]
    assert list(f["variances"]["equal"]) == [True, False]                    # a NaN observed value is never "equal"
    assert list(f["summary"]["invariance"]) == ["full", "none"]
    observed[3], observed[5] = 0.0, 0.0
    assert list(_frames(lvs, observed, p, quantile, lower, upper)["summary"]["invariance"]) == ["full", "none"]      # step 2 fails: none, whatever step 3 says
    observed[1], observed[3] = 0.97, 0.9
    assert list(_frames(lvs, observed, p, quantile, lower, upper)["summary"]["invariance"]) == ["full", "partial"]


# ------------------------------------------------------------------ argument checks that raise before the device is touched
def _data_and_config(scale=None, n=60):
    rng = np.random.default_rng(0)
    data = pd.DataFrame(rng.standard_normal((n, 4)), columns=["x1", "x2", "y1", "y2"])
    data["grp"] = np.where(np.arange(n) < n // 2, "a", "b")
    s = c.Structure()
    s.add_path(["X"], ["Y"])
    cfg = c.Config(s.path(), scaled=True, default_scale=scale)
    cfg.add_lv_with_columns_named("X", Mode.A, data, "x")
    cfg.add_lv_with_columns_named("Y", Mode.A, data, "y")
    return data, cfg


def test_micom_argument_checks_need_no_device():
    data, cfg = _data_and_config()
    with pytest.raises(ValueError, match="permutations"):
        Micom(data, cfg, "grp", permutations=0)
    with pytest.raises(ValueError, match="alpha"):
        Micom(data, cfg, "grp", alpha=0.5)
    with pytest.raises(ValueError, match="column label"):
        Micom(data, cfg, "nope")
    three = data.copy()
    three.loc[:9, "grp"] = "c"
    with pytest.raises(ValueError, match="exactly two"):
        Micom(three, cfg, "grp")
    small = data.copy()
    small["grp"] = np.where(np.arange(60) < 5, "a", "b")
    with pytest.raises(ValueError, match="at least 10 rows"):
        Micom(small, cfg, "grp")
    with pytest.raises(ValueError, match="aligned"):
        Micom(data, cfg, pd.Series(["a", "b"] * 30, index=np.arange(60) + 1))
    holes = data.copy()
    holes.loc[3, "x1"] = np.nan
    with pytest.raises(NotImplementedError, match="MICOM needs complete data"):
        Micom(holes, cfg, "grp")
    data_nm, cfg_nm = _data_and_config(Scale.NUM)
    with pytest.raises(NotImplementedError, match="MICOM covers metric data only"):
        Micom(data_nm, cfg_nm, "grp")


# ------------------------------------------------------------------ the C-ABI's declarations
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
    out = np.zeros(16)
    assert lib.plspm_micom_enable(None, 1) == 100             # PLSPM_E_ARG
    assert lib.plspm_micom_width(None) == 0
    assert lib.plspm_micom_fetch(None, 0, 1, out.ctypes.data, None) == 100
    assert lib.plspm_micom_summary(None, 10, out.ctypes.data, out.ctypes.data, None) == 100
    assert lib.plspm_micom_intervals(None, 10, out.ctypes.data, 0, 0.95, out.ctypes.data, None) == 100
    assert lib.plspm_micom_counts(None, 10, out.ctypes.data, out.ctypes.data, out.ctypes.data, None) == 100
