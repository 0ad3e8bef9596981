"""GPU: the two-group bootstrap (include/plspm_hip.h plspm_stratified_bootstrap_device / plspm_stratified_pair_counts,
plspm.mga.GroupComparison(method="bootstrap")).

The on-device draws are the host mirror's bit for bit (records identical to the explicit-draws seam, any sharding of the resample range
reproduces the stream), both records of a resample are the oracle's fits on X[draws_a] / X[draws_b] (rtol 1e-8 and identical iteration
counts), the per-group device summaries and Henseler's pair counts are NumPy's on the fetched records, and the API's frames are the tests'
formulas around ordinary fits of the groups."""
import numpy as np
import pytest

import plspm_oracle as orc
from helpers import assert_close, case_modes, satisfaction_oracle_inputs
from test_gpu_mga import _sat_config, _two_groups, native_model

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-8, 1e-11


def _member(n, n_a, seed):
    member = np.zeros(n, dtype=bool)
    member[np.random.default_rng(seed).permutation(n)[:n_a]] = True
    return member


def run_strat(nm, B, member, seed=0, rep_offset=0, draws=None):
    nm.stratified_bootstrap(B, member, seed, rep_offset, draws)
    return nm.fetch(0, 2 * B)


def oracle_rec(X, model, rows):
    r = orc.fit(X[rows], model, orc.correction(rows.size))
    return np.concatenate((r["weights"][model.mv_order], r["r2"], r["total"], r["direct"], r["loadings"][model.mv_order])), r["iterations"]


def check_vs_oracle(nm, X, model, B, member, seed, sample, rep_offset=0):
    from plspm import _native
    rows, status, iters = run_strat(nm, B, member, seed, rep_offset)
    assert nm.get_option("last_gram_path") == 2
    n_a = int(member.sum())
    for p in sample:
        d = _native.stratified_draws(seed, rep_offset + p, member)
        for k, rows_k in ((0, d[:n_a]), (1, d[n_a:])):
            mine, its = oracle_rec(X, model, rows_k)
            assert status[2 * p + k] == 0, (p, k)
            assert iters[2 * p + k] == its, "resample %d group %d: iterations %d vs oracle %d" % (p, k, iters[2 * p + k], its)
            assert_close(rows[2 * p + k], mine, RTOL, ATOL, what="resample %d group %d" % (p, k))
    return rows, status, iters


# ------------------------------------------------------------------ the draws
@pytest.mark.parametrize("strat_rows", [0, 1, 2])
def test_device_draws_are_the_host_mirror_bit_for_bit(strat_rows):
    """Row lists through L2 (1), from LDS (2) and the automatic choice (0) give the same records as the explicit draws of the mirror."""
    from plspm import _native
    X, blocks = orc.synth(3000, orc.satisfaction_C(), 10, seed=2)
    model = orc.Model(blocks, orc.satisfaction_C(), "AAAAAA", "path", True)
    nm = native_model(model, X)
    nm.set_option("strat_rows", strat_rows)
    member = _member(3000, 1100, 1)
    B, seed = 24, 0xFACE
    rows, status, iters = run_strat(nm, B, member, seed)
    if strat_rows:
        assert nm.get_option("last_strat_rows") == strat_rows
    draws = np.stack([_native.stratified_draws(seed, p, member) for p in range(B)])
    rows2, status2, iters2 = run_strat(nm, B, member, draws=draws)
    assert np.array_equal(rows, rows2, equal_nan=True) and np.array_equal(status, status2) and np.array_equal(iters, iters2)
    a = run_strat(nm, 10, member, seed, 0)
    b = run_strat(nm, 14, member, seed, 10)
    for k in range(3):
        assert np.array_equal(np.concatenate((a[k], b[k])), (rows, status, iters)[k], equal_nan=True)   # [0, 10) + [10, 24) == [0, 24)


# ------------------------------------------------------------------ parity with the oracle
@pytest.mark.parametrize("modes", ["A", "B", "M"])
@pytest.mark.parametrize("scheme", ["centroid", "factorial", "path"])
@pytest.mark.parametrize("scaled", [False, True])
def test_satisfaction_resamples_vs_oracle(modes, scheme, scaled):
    X, blocks, _ = satisfaction_oracle_inputs()
    model = orc.Model(blocks, orc.satisfaction_C(), case_modes(modes), scheme, scaled)
    nm = native_model(model, X, model.mv_order.astype(np.int32))
    check_vs_oracle(nm, X, model, 6, _member(X.shape[0], 120, 4), seed=31, sample=(0, 5), rep_offset=2)


@pytest.mark.parametrize("n_a", [5000, 2000])
def test_headline_model_resamples_vs_oracle(n_a):
    """10k x 60, 6 LVs, Mode A, PATH, scaled: 5,000/5,000 and 2,000/8,000 groups."""
    X, blocks = orc.synth(10000, orc.satisfaction_C(), 10, seed=0)
    model = orc.Model(blocks, orc.satisfaction_C(), "AAAAAA", "path", True)
    nm = native_model(model, X)
    rows, status, _ = check_vs_oracle(nm, X, model, 40, _member(10000, n_a, 7), seed=4, sample=(0, 39))
    assert np.all(status == 0)


def test_resamples_beyond_one_count_window_vs_oracle():
    """N = 70,000 > 65,536: the counts of a problem span two windows of the fragment layout."""
    C = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0]])
    X, blocks = orc.synth(70000, C, 4, seed=11)
    model = orc.Model(blocks, C, "ABA", "path", True)
    nm = native_model(model, X)
    check_vs_oracle(nm, X, model, 5, _member(70000, 20000, 3), seed=99, sample=(0, 4), rep_offset=3)


def test_a_multiplicity_above_127_is_refused():
    from plspm import _native
    X, blocks = orc.synth(1000, orc.satisfaction_C(), 4, seed=3)
    model = orc.Model(blocks, orc.satisfaction_C(), "AAAAAA", "path", True)
    nm = native_model(model, X)
    member = _member(1000, 400, 2)
    draws = _native.stratified_draws(5, 0, member)[None, :].copy()
    draws[0, :128] = np.flatnonzero(member)[0]                              # one row of group a drawn 128 times
    with pytest.raises(_native.NativeBackendError, match="127"):
        run_strat(nm, 1, member, draws=draws)
    draws[0, :128] = np.flatnonzero(~member)[0]                             # a row of the other group
    with pytest.raises(_native.NativeBackendError, match="its group"):
        run_strat(nm, 1, member, draws=draws)
    ok = np.concatenate((_native.stratified_draws(5, 0, member)[None, :],) * 2)
    assert np.all(run_strat(nm, 2, member, draws=ok)[1] == 0)              # the handle still works


def test_stratified_call_leaves_bootstrap_and_permutation_unchanged():
    X, blocks = orc.synth(10000, orc.satisfaction_C(), 10, seed=0)
    model = orc.Model(blocks, orc.satisfaction_C(), "AAAAAA", "path", True)
    nm = native_model(model, X)
    boot0 = nm.bootstrap(64, seed=3)
    nm.permutation(16, 5000, 1); perm0 = nm.fetch(0, 32)
    run_strat(nm, 16, _member(10000, 5000, 1), seed=1)
    boot1 = nm.bootstrap(64, seed=3)
    nm.permutation(16, 5000, 1); perm1 = nm.fetch(0, 32)
    for x, y in zip(boot0 + perm0, boot1 + perm1):
        assert np.array_equal(x, y, equal_nan=True)


# ------------------------------------------------------------------ summaries and pair counts on the device
def test_group_summaries_and_pair_counts_equal_numpy():
    X, blocks = orc.synth(2000, orc.satisfaction_C(), 5, seed=6)
    model = orc.Model(blocks, orc.satisfaction_C(), "ABABAB", "factorial", True)
    nm = native_model(model, X)
    B = 300
    d_out, _, _ = nm.stratified_bootstrap(B, _member(2000, 700, 5), seed=21)
    rows, status, _ = nm.fetch(0, 2 * B)
    RS, R = nm.row_stride, nm.row_width
    orig = np.zeros(R)
    sa, ua = nm.summary(B, orig, d_rows=d_out, stride=2 * RS)
    sb, ub = nm.summary(B, orig, d_rows=d_out + 8 * RS, stride=2 * RS)
    for s, u, recs, st in ((sa, ua, rows[0::2], status[0::2]), (sb, ub, rows[1::2], status[1::2])):
        v = recs[st == 0]
        assert u == v.shape[0]
        assert_close(s[:, 1], v.mean(axis=0), 1e-12, 1e-15, what="mean")
        assert_close(s[:, 2], v.std(axis=0, ddof=1), 1e-10, 1e-15, what="std.error")
    # pair counts with the device's centres (a NaN centre in column 3 counts nothing)
    ca, cb = sa[:, 1].copy(), sb[:, 1].copy()
    ca[3] = np.nan
    rows_a, rows_b = rows[0::2][status[0::2] == 0], rows[1::2][status[1::2] == 0]
    above, used_a, used_b = nm.stratified_pair_counts(B, ca, cb)
    assert used_a == rows_a.shape[0] and used_b == rows_b.shape[0]
    for j in range(R):
        u_a, u_b = 2.0 * ca[j] - rows_a[:, j], np.sort(2.0 * cb[j] - rows_b[:, j])
        u_a = u_a[~np.isnan(u_a)]
        u_b = u_b[~np.isnan(u_b)]
        assert above[j] == int(np.searchsorted(u_b, u_a, side="left").sum()), j
    assert above[3] == 0


def test_pair_counts_with_ties_and_failed_records():
    """Records stored with duplicated values and failed statuses: ties never count, failed records and NaN values count nothing."""
    X, blocks = orc.synth(600, orc.satisfaction_C(), 4, seed=1)
    model = orc.Model(blocks, orc.satisfaction_C(), "AAAAAA", "path", True)
    nm = native_model(model, X)
    R, RS, B = nm.row_width, nm.row_stride, 2500
    rng = np.random.default_rng(0)
    rec = np.zeros((2 * B, RS))
    rec[:, :R] = rng.integers(-3, 4, size=(2 * B, R)) * 0.25               # many exact ties
    rec[7, 2] = np.nan; rec[8, 2] = np.nan
    rec[11, R] = 1.0; rec[40, R] = 2.0                                      # failed: group b of resample 5, group a of resample 20
    nm.store(rec)
    ca, cb = rng.standard_normal(R) * 0.1, rng.standard_normal(R) * 0.1
    cb[0] = ca[0]
    above, used_a, used_b = nm.stratified_pair_counts(B, ca, cb)
    ok = rec[:, R] == 0
    ra, rb = rec[0::2][ok[0::2]], rec[1::2][ok[1::2]]
    assert used_a == B - 1 and used_b == B - 1
    for j in range(R):
        u_a = 2.0 * ca[j] - ra[:, j]; u_b = np.sort(2.0 * cb[j] - rb[:, j])
        u_a, u_b = u_a[~np.isnan(u_a)], u_b[~np.isnan(u_b)]
        assert above[j] == int(np.searchsorted(u_b, u_a, side="left").sum()), j


# ------------------------------------------------------------------ the API
def test_satisfaction_by_gender_frames():
    from plspm.mga import GroupComparison, bootstrap_tests
    from plspm.plspm import Plspm
    from plspm.scheme import Scheme
    sat, cfg = _sat_config()
    res = GroupComparison(sat, cfg, "gender", Scheme.PATH, method="bootstrap", resamples=400, seed=17)
    assert res.groups() == ("female", "male") and res.seed() == 17
    ua, ub = res.used()
    assert 0 < ua <= 400 and 0 < ub <= 400
    t_cols = ["global", "group.female", "group.male", "diff.abs", "t.stat", "deg.fr", "p.value", "sig.05"]
    h_cols = ["global", "group.female", "group.male", "diff.abs", "p.value", "sig.05"]
    for test, cols in (("parametric", t_cols), ("welch", t_cols), ("henseler", h_cols)):
        frames = dict(paths=res.paths(test), weights=res.weights(test), loading=res.loading(test), r_squared=res.r_squared(test),
                      total_effects=res.total_effects(test))
        for name, f in frames.items():
            assert list(f.columns) == cols, (test, name)
            assert np.all(np.isfinite(f[cols[:-1]].values.astype(np.float64))), (test, name)
            assert np.all((f["p.value"] >= 0) & (f["p.value"] <= 1)), (test, name)
            assert np.array_equal(f["sig.05"].values, np.where(f["p.value"] < 0.05, "yes", "no")), (test, name)
        assert len(frames["paths"]) == 10
    for name in ("paths", "weights", "loading", "r_squared", "total_effects"):
        assert getattr(res, name)().equals(getattr(res, name)("parametric"))
    # the groups: ordinary fits, as Plspm on the subsets
    for col, rows in (("global", sat), ("group.female", sat[sat["gender"] == "female"]), ("group.male", sat[sat["gender"] == "male"])):
        ref = Plspm(rows, cfg, Scheme.PATH)
        eff = ref.effects()
        assert_close(res.paths()[col], eff.loc[res.paths().index, "direct"], 1e-12, 1e-14, what=col + " paths")
        om = ref.outer_model()
        assert_close(res.weights("henseler")[col], om.loc[res.weights().index, "weight"], 1e-12, what=col + " weights")
        assert_close(res.loading("welch")[col], om.loc[res.loading().index, "loading"], 1e-12, what=col + " loadings")
    # t and p recompute from raw; raw's summaries are NumPy's on the fetched records
    raw = res.raw
    again = bootstrap_tests(raw["observed_diff"], raw["se_a"], raw["se_b"], raw["mean_a"], raw["mean_b"], raw["n_a"], raw["n_b"], raw["above"],
                            raw["used_a"], raw["used_b"])
    for k in ("parametric", "welch"):
        for a, b in zip(again[k], (raw["t_" + k], raw["df_" + k], raw["p_" + k])):
            assert np.array_equal(a, b, equal_nan=True)
    assert np.array_equal(again["henseler"], raw["p_henseler"], equal_nan=True)
    rows, status, _ = res.bootstrap_records()
    va = rows[0::2][status[0::2] == 0]
    assert_close(raw["mean_a"], va.mean(axis=0), 1e-12, 1e-15, what="mean_a")
    assert_close(raw["se_a"], va.std(axis=0, ddof=1), 1e-10, 1e-15, what="se_a")
    with pytest.raises(ValueError):
        res.permutation_records()
    perm = GroupComparison(sat, cfg, "gender", Scheme.PATH, permutations=50, seed=17)
    with pytest.raises(ValueError):
        perm.paths(test="welch")


@pytest.mark.parametrize("test", ["parametric", "welch", "henseler"])
def test_a_differing_path_is_found_under_both_label_orders(test):
    from plspm.mga import GroupComparison
    from plspm.scheme import Scheme
    data, cfg = _two_groups(3)
    swapped = data.copy()
    swapped["grp"] = swapped["grp"].map({"g1": "g2", "g2": "g1"})
    for d in (data, swapped):
        res = GroupComparison(d, cfg, "grp", Scheme.PATH, method="bootstrap", resamples=500, seed=9, test=test)
        paths = res.paths()
        assert paths.loc["X -> Y", "p.value"] < 0.01 and paths.loc["X -> Y", "sig.05"] == "yes", (test, paths)
        assert paths.loc["Y -> Z", "p.value"] >= 0.01, (test, paths)
