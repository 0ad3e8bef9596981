"""CPU: the host surface of the k-fold out-of-sample prediction -- the folds of a repetition (plspm_cv_folds, the host mirror of the device's
draw) against the NumPy restatement of their definition (tests/helpers_predict.py), the new C-ABI symbols, the argument checks of
plspm.predict.PLSpredict, which all happen before anything runs on a device, and the restatement itself on a case small enough to write
the expected predictions out by hand."""
import numpy as np
import pytest

import plspm.config as c
import plspm_oracle as orc
from plspm import _native
from plspm.mode import Mode
from plspm.predict import PLSpredict, linear_model_coefficients
from plspm.scale import Scale
from plspm.scheme import Scheme

from helpers import SAT_ADD_ORDER, SAT_PREFIX, satisfaction_frame
from helpers_mga import find_tie, permutation_keys, philox4x32_10
from helpers_predict import _find_cv_tie, cross_validate, cv_folds, cv_keys, lm_predict, metrics, pls_predict


@pytest.mark.parametrize("seed,rep,n,k", [(0, 0, 250, 10), (7, 3, 250, 7), (7, 4, 251, 2), (0xC0FFEE, 12345, 10000, 10), (2 ** 63 + 5, 2 ** 33 + 1, 10007, 256),
                                          (11, 1, 70001, 3), (99, 5, 131075, 5), (3, 0, 12, 3), (3, 1, 9, 9)])
def test_folds_match_the_numpy_philox_restatement(seed, rep, n, k):
    mine = _native.cv_folds(seed, rep, n, k)
    assert mine.dtype == np.uint8 and mine.shape == (n,)
    assert np.array_equal(mine, cv_folds(seed, rep, n, k))
    sizes = np.bincount(mine, minlength=k)
    assert sizes.sum() == n and sizes.min() >= 1 and sizes.max() - sizes.min() <= 1


def test_folds_break_key_ties_by_row():
    """Two rows that share a key, with a fold boundary between them: the lower row index goes to the lower fold."""
    n = 200000
    assert find_tie(5, n, range(4)) is not None              # (ties exist at this size: the permutation stream's helper finds them too)
    found = _find_cv_tie(5, n, range(64))
    assert found is not None
    rep, k, a, b = found
    keys = cv_keys(5, rep, n)
    assert keys[a] == keys[b] and a < b
    mine = _native.cv_folds(5, rep, n, k)
    assert np.array_equal(mine, cv_folds(5, rep, n, k))
    assert mine[a] + 1 == mine[b]


def test_cv_stream_is_neither_the_permutation_nor_the_bootstrap_stream():
    """Counter word 1 = 3: the keys are not the words of the bootstrap (0), the permutation (1) or the stratified draws (2)."""
    q = np.arange(64, dtype=np.uint64)
    mine = cv_keys(9, 3, 256)
    for word in (0, 1, 2):
        other = np.stack(philox4x32_10(q, word, 3, 0, 9, 0), axis=1).reshape(-1).astype(np.uint32)
        assert not np.array_equal(mine, other)
    assert np.array_equal(np.stack(philox4x32_10(q, 1, 3, 0, 9, 0), axis=1).reshape(-1).astype(np.uint32), permutation_keys(9, 3, 256))
    # and the library's folds are this stream's, not the permutation's
    order = np.lexsort((np.arange(256), permutation_keys(9, 3, 256)))
    other = np.empty(256, dtype=np.uint8)
    other[order] = (np.arange(256) * 4) // 256
    assert not np.array_equal(_native.cv_folds(9, 3, 256, 4), other)


def test_folds_reject_bad_sizes():
    lib = _native.load()
    out = np.empty(300, dtype=np.uint8)
    for n, k in ((10, 1), (10, 257), (10, 11), (0, 2), (10, 0)):
        assert lib.plspm_cv_folds(1, 0, n, k, out.ctypes.data) == 100           # PLSPM_E_ARG
    assert lib.plspm_cv_folds(1, -1, 10, 2, out.ctypes.data) == 100
    assert lib.plspm_cv_folds(1, 0, 10, 2, None) == 100


def test_new_symbols_are_exported_and_declared():
    lib = _native.load()
    for name in ("plspm_cv_folds", "plspm_cv_device", "plspm_cv_fold_ids", "plspm_cv_moments", "plspm_cv_targets", "plspm_cv_predict"):
        assert name in _native.EXPORTS
        assert hasattr(lib, name)
    assert lib.plspm_abi_version() == 4


# ------------------------------------------------------------------ PLSpredict: argument checks (no device needed)
def _sat():
    sat = satisfaction_frame()
    s = c.Structure()
    s.add_path(["IMAG"], ["EXPE", "SAT", "LOY"]); s.add_path(["EXPE"], ["QUAL", "VAL", "SAT"])
    s.add_path(["QUAL"], ["VAL", "SAT"]); s.add_path(["VAL"], ["SAT"]); s.add_path(["SAT"], ["LOY"])
    cfg = c.Config(s.path(), scaled=False)
    for lv in SAT_ADD_ORDER:
        cfg.add_lv_with_columns_named(lv, Mode.A, sat, SAT_PREFIX[lv])
    return sat, cfg


def test_argument_errors():
    sat, cfg = _sat()
    with pytest.raises(ValueError, match="technique must be one of"):
        PLSpredict(sat, cfg, Scheme.PATH, technique="latest", seed=1)
    for folds in (1, 257, 0):
        with pytest.raises(ValueError, match="folds must be between 2 and 256"):
            PLSpredict(sat, cfg, Scheme.PATH, folds=folds, seed=1)
    with pytest.raises(ValueError, match="repetitions must be at least 1"):
        PLSpredict(sat, cfg, Scheme.PATH, repetitions=0, seed=1)
    with pytest.raises(ValueError, match="every training set needs at least"):
        PLSpredict(sat.iloc[:5], cfg, Scheme.PATH, folds=2, seed=1)


def test_models_outside_the_scope_raise_not_implemented():
    sat, cfg = _sat()
    num = c.Config(cfg.path(), scaled=True, default_scale=Scale.NUM)
    for lv in SAT_ADD_ORDER:
        num.add_lv_with_columns_named(lv, Mode.A, sat, SAT_PREFIX[lv])
    with pytest.raises(NotImplementedError):
        PLSpredict(sat, num, Scheme.PATH, seed=1)
    holes = sat.copy()
    holes.iloc[5, 2] = np.nan
    _, cfg2 = _sat()
    with pytest.raises(NotImplementedError):
        PLSpredict(holes, cfg2, Scheme.PATH, seed=1)
    st = c.Structure()
    st.add_path(["IMAG"], ["H"]); st.add_path(["H"], ["LOY"])
    hoc = c.Config(st.path(), default_scale=Scale.NUM)
    hoc.add_higher_order("H", Mode.A, ["SAT", "VAL"])
    for lv in ("IMAG", "SAT", "VAL", "LOY"):
        hoc.add_lv_with_columns_named(lv, Mode.A, sat, SAT_PREFIX[lv])
    with pytest.raises(NotImplementedError):
        PLSpredict(sat, hoc, Scheme.PATH, seed=1)


# ------------------------------------------------------------------ the restatement on a hand-made case
@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("slope_sign", [1.0, -1.0])
def test_helper_on_two_single_indicator_lvs(scaled, slope_sign):
    """Two LVs with one indicator each, x1 -> x2, N = 12, k = 3: a score is its standardised column, the path coefficient the correlation, the
    loading 1 -- so the PLS prediction of x2 for a held-out row is the ordinary regression line of x2 on x1 in the training rows, and the
    benchmark is that same line."""
    rng = np.random.default_rng(4)
    x1 = rng.standard_normal(12) * 2.0 + 5.0
    x2 = slope_sign * 0.7 * x1 + rng.standard_normal(12) + 1.0
    X = np.column_stack((x1, x2))
    model = orc.Model([np.array([0]), np.array([1])], np.array([[0, 0], [1, 0]]), "AA", "path", scaled)
    fold = np.arange(12) % 3
    for f in range(3):
        train = fold != f
        a, b = X[train, 0], X[train, 1]
        slope = ((a - a.mean()) * (b - b.mean())).sum() / ((a - a.mean()) ** 2).sum()
        expected = b.mean() + slope * (X[~train, 0] - a.mean())
        for technique in ("direct", "earliest"):
            pred, fit = pls_predict(X, model, train, technique)
            assert pred.shape == (4, 1)
            assert np.allclose(pred[:, 0], expected, rtol=1e-12, atol=1e-12)
        assert np.allclose(lm_predict(X, model, train)[:, 0], expected, rtol=1e-10, atol=1e-12)
    problems = cross_validate(X, model, fold[None, :].astype(np.uint8), 3)
    m, (used, rows) = metrics(problems)
    assert used == 3 and rows == 12
    e = np.concatenate([X[p["rows"], 1] - p["pred"][:, 0] for p in problems])
    assert np.allclose(m["rmse"], np.sqrt((e ** 2).mean())) and np.allclose(m["mae"], np.abs(e).mean())
    sst = sum(((X[p["rows"], 1] - np.delete(X[:, 1], p["rows"]).mean()) ** 2).sum() for p in problems)
    assert np.allclose(m["q2_predict"], 1 - (e ** 2).sum() / sst)
    assert np.allclose(m["lm.rmse"], m["rmse"], rtol=1e-9)


def test_linear_model_coefficients_from_moments_equal_lstsq_on_rows():
    """The benchmark's normal equations (centred cross-products, as plspm_cv_moments returns them) against lstsq on the raw rows."""
    rng = np.random.default_rng(8)
    X = rng.standard_normal((40, 5)) + np.array([3.0, -2.0, 0.5, 10.0, 0.0])
    X[:, 3] += 0.8 * X[:, 0] - 0.3 * X[:, 1]
    X[:, 4] += 0.5 * X[:, 1]
    mean = X.mean(axis=0)[None, :]
    Sc = (X - mean).T @ (X - mean)
    cross = Sc[np.triu_indices(5)][None, :]
    coef = linear_model_coefficients(np.array([40.0]), mean, cross, [0, 1], [3, 4], 5)
    beta = np.linalg.lstsq(np.column_stack((np.ones(40), X[:, :2])), X[:, 3:], rcond=None)[0]
    assert np.allclose(coef[0][:, 0], beta[0], rtol=1e-10) and np.allclose(coef[0][:, 1:3], beta[1:].T, rtol=1e-10)
    assert np.all(coef[0][:, 3:] == 0)
