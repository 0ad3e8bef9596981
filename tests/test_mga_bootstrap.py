"""CPU: the two-group bootstrap's host surface -- the stratified draws (plspm_stratified_draws, the host mirror of the device's draws) against a
NumPy restatement of their definition, the new C-ABI symbols, the argument checks of GroupComparison(method="bootstrap"), which all happen
before anything runs on a device, and the three tests' formulas (plspm.mga.bootstrap_tests) against hand-computed values."""
import numpy as np
import pandas as pd
import pytest
from scipy import stats

from plspm import _native
from plspm.mga import GroupComparison, bootstrap_tests
from plspm.scheme import Scheme

from helpers_mga import philox4x32_10
from test_mga import _sat


def strat_words(seed, s, n):
    """Words 0 .. n - 1 of problem s: word j & 3 of Philox(counter = (j >> 2, 2, lo32(s), hi32(s)), key = (lo32(seed), hi32(seed)))."""
    q = np.arange((n + 3) // 4, dtype=np.uint64)
    words = philox4x32_10(q, 2, s & 0xFFFFFFFF, s >> 32, seed & 0xFFFFFFFF, seed >> 32)
    return np.stack(words, axis=1).reshape(-1)[:n].astype(np.uint64)


def strat_draws(seed, rep, member):
    """Resample rep: group a's n_a draws rows_a[(u * n_a) >> 32] from problem 2 rep, then group b's from problem 2 rep + 1."""
    member = np.asarray(member, dtype=bool)
    out = []
    for g, rows in ((0, np.flatnonzero(member)), (1, np.flatnonzero(~member))):
        n = rows.size
        k = (strat_words(seed, 2 * rep + g, n) * np.uint64(n)) >> np.uint64(32)
        out.append(rows[k.astype(np.int64)])
    return np.concatenate(out).astype(np.int32)


def _member(n, n_a, seed):
    member = np.zeros(n, dtype=bool)
    member[np.random.default_rng(seed).permutation(n)[:n_a]] = True
    return member


@pytest.mark.parametrize("seed,rep,n,n_a", [(0, 0, 250, 148), (7, 3, 250, 2), (7, 4, 250, 248), (0xC0FFEE, 12345, 10000, 5000),
                                            (2 ** 63 + 5, 2 ** 33 + 1, 10000, 2000), (11, 1, 70001, 10), (99, 2 ** 40 + 7, 131075, 40000)])
def test_draws_match_the_numpy_philox_restatement(seed, rep, n, n_a):
    member = _member(n, n_a, seed % 1000 + n_a)
    mine = _native.stratified_draws(seed, rep, member)
    assert mine.dtype == np.int32 and mine.shape == (n,)
    assert np.array_equal(mine, strat_draws(seed, rep, member))
    # every draw lies in its group
    assert np.all(member[mine[:n_a]]) and not np.any(member[mine[n_a:]])


def test_draws_of_contiguous_groups_cover_their_rows():
    member = np.arange(1000) < 300
    d = _native.stratified_draws(5, 0, member)
    assert d[:300].min() >= 0 and d[:300].max() < 300 and d[300:].min() >= 300 and d[300:].max() < 1000
    assert np.unique(d[:300]).size > 150                                    # a resample, not a constant


def test_stratified_stream_is_neither_the_bootstrap_nor_the_permutation_stream():
    q = np.arange(64, dtype=np.uint64)
    boot = np.stack(philox4x32_10(q, 0, 6, 0, 9, 0), axis=1).reshape(-1)
    perm = np.stack(philox4x32_10(q, 1, 6, 0, 9, 0), axis=1).reshape(-1)
    strat = strat_words(9, 6, 256)
    assert not np.array_equal(strat, boot) and not np.array_equal(strat, perm)
    # with one group of all-but-two rows, group a's draws would equal the bootstrap's mapping of the same words if the streams were shared
    member = np.ones(258, dtype=bool); member[-2:] = False
    d = _native.stratified_draws(9, 3, member)[:256]
    assert not np.array_equal(d, _native.bootstrap_indices(9, 6, 256))


def test_draws_reject_bad_groups():
    lib = _native.load()
    out = np.empty(10, dtype=np.int32)
    for member in (np.r_[np.ones(1), np.zeros(9)], np.r_[np.ones(9), np.zeros(1)], np.full(10, 2)):
        m = np.ascontiguousarray(member, dtype=np.uint8)
        assert lib.plspm_stratified_draws(1, 0, 10, m.ctypes.data, out.ctypes.data) != 0


def test_new_symbols_are_exported_and_declared():
    lib = _native.load()
    for name in ("plspm_stratified_bootstrap_device", "plspm_stratified_pair_counts", "plspm_stratified_draws"):
        assert name in _native.EXPORTS
        assert hasattr(lib, name)
    assert lib.plspm_abi_version() == 4


# ------------------------------------------------------------------ GroupComparison(method="bootstrap"): argument checks (no device needed)
def test_bad_method_test_or_resamples_raise_value_error():
    sat, cfg = _sat()
    with pytest.raises(ValueError, match="method"):
        GroupComparison(sat, cfg, "gender", Scheme.PATH, method="jackknife", seed=1)
    with pytest.raises(ValueError, match="test"):
        GroupComparison(sat, cfg, "gender", Scheme.PATH, method="bootstrap", test="mann-whitney", seed=1)
    for bad in (0, -3):
        with pytest.raises(ValueError, match="resamples"):
            GroupComparison(sat, cfg, "gender", Scheme.PATH, method="bootstrap", resamples=bad, seed=1)
    lab = pd.Series(np.where(np.arange(len(sat)) < 9, "x", "y"), index=sat.index)
    with pytest.raises(ValueError, match="at least 10 rows"):
        GroupComparison(sat, cfg, lab, Scheme.PATH, method="bootstrap", resamples=10, seed=1)


def test_bootstrap_models_outside_the_scope_raise_not_implemented():
    import plspm.config as c
    from plspm.mode import Mode
    from plspm.scale import Scale
    from helpers import SAT_ADD_ORDER, SAT_PREFIX
    sat, cfg = _sat()
    num = c.Config(cfg.path(), scaled=True, default_scale=Scale.NUM)
    for lv in SAT_ADD_ORDER:
        num.add_lv_with_columns_named(lv, Mode.A, sat, SAT_PREFIX[lv])
    with pytest.raises(NotImplementedError, match="bootstrap"):
        GroupComparison(sat, num, "gender", Scheme.PATH, method="bootstrap", resamples=10, seed=1)
    holes = sat.copy()
    holes.iloc[5, 2] = np.nan
    with pytest.raises(NotImplementedError, match="bootstrap"):
        GroupComparison(holes, cfg, "gender", Scheme.PATH, method="bootstrap", resamples=10, seed=1)


# ------------------------------------------------------------------ the three tests' formulas
def test_parametric_and_welch_match_hand_computed_values():
    d, se_a, se_b, n_a, n_b = np.array([0.3, -0.1]), np.array([0.1, 0.05]), np.array([0.2, 0.05]), 40, 60
    out = bootstrap_tests(d, se_a, se_b, np.zeros(2), np.zeros(2), n_a, n_b, np.zeros(2), 10, 10)
    # parametric, column 0 by hand: s_p = sqrt(39^2/98 * 0.01 + 59^2/98 * 0.04), t = 0.3 / (s_p sqrt(1/40 + 1/60)), df = 98
    sp = np.sqrt(39.0 ** 2 / 98 * 0.01 + 59.0 ** 2 / 98 * 0.04)
    t = 0.3 / (sp * np.sqrt(1 / 40 + 1 / 60))
    tp, dfp, pp = out["parametric"]
    assert tp[0] == pytest.approx(t, rel=1e-14) and dfp[0] == 98
    assert pp[0] == pytest.approx(2 * stats.t.sf(t, 98), rel=1e-12)
    assert tp[1] > 0                                                      # |d|
    # welch, column 0: v = 39/40 0.01 + 59/60 0.04, df = v^2 / (39/1600 1e-4 + 59/3600 16e-4) - 2
    v = 39 / 40 * 0.01 + 59 / 60 * 0.04
    tw, dfw, pw = out["welch"]
    assert tw[0] == pytest.approx(0.3 / np.sqrt(v), rel=1e-14)
    assert dfw[0] == pytest.approx(v ** 2 / (39 / 1600 * 1e-4 + 59 / 3600 * 16e-4) - 2, rel=1e-13)
    assert pw[0] == pytest.approx(2 * stats.t.sf(0.3 / np.sqrt(v), dfw[0]), rel=1e-12)
    assert 0 < pw[1] < 1 and 0 < pp[1] < 1


def test_henseler_matches_hand_computed_values():
    d = np.array([0.2, 0.2, -0.2, 0.0])
    above = np.array([90, 3, 50, 100])                                     # of used_a * used_b = 100 pairs
    out = bootstrap_tests(d, np.full(4, 0.1), np.full(4, 0.1), np.zeros(4), np.zeros(4), 50, 50, above, 10, 10)
    p = out["henseler"]
    # p_one = 1 - above / 100 -> 0.1, 0.97, 0.5, 0.0;  p = 2 min(p_one, 1 - p_one)
    assert np.allclose(p, [0.2, 0.06, 1.0, 0.0], rtol=0, atol=1e-15)


def test_nan_and_zero_over_zero_give_nan():
    d = np.array([np.nan, 0.1, 0.1, 0.1, 0.0, 0.1])
    se_a = np.array([0.1, np.nan, 0.1, 0.1, 0.0, 0.0])
    se_b = np.array([0.1, 0.1, 0.1, 0.1, 0.0, 0.0])
    mean_a = np.array([0.0, 0.0, np.nan, 0.0, 0.0, 0.0])
    mean_b = np.zeros(6)
    out = bootstrap_tests(d, se_a, se_b, mean_a, mean_b, 30, 30, np.full(6, 40), 10, 10)
    for name in ("parametric", "welch"):
        t, df, p = out[name]
        assert np.all(np.isnan(p[:3])), name                               # NaN d / se / centre
        assert np.isfinite(p[3]), name
        assert np.isnan(t[4]) and np.isnan(p[4]), name                     # 0 / 0
        assert p[5] == 0.0 or np.isnan(p[5]), name                          # |d| / 0 = inf: p = 0 (welch: df 0 / 0 -> NaN)
    assert out["parametric"][2][5] == 0.0
    ph = out["henseler"]
    assert np.all(np.isnan(ph[:3])) and np.all(np.isfinite(ph[3:]))
    # no valid pairs: Henseler's p is NaN
    assert np.all(np.isnan(bootstrap_tests(d, se_a, se_b, mean_a, mean_b, 30, 30, np.zeros(6), 0, 10)["henseler"]))
