"""GPU: the two-group permutation test (include/plspm_hip.h plspm_permutation_device / plspm_permutation_counts, plspm.mga.GroupComparison).

The on-device splits are the host mirror's bit for bit (records identical to the explicit-membership seam, any sharding of the permutation
range reproduces the stream), both records of a permutation are the oracle's fits on X[member] / X[~member] (rtol 1e-8 and identical
iteration counts, as tests/test_gpu_parity.py holds the bootstrap), the device's exceedance counts are the host's on the fetched records, and
the API's frames are the restatement's p-values around ordinary fits of the groups."""
import numpy as np
import pandas as pd
import pytest

import plspm_oracle as orc
from helpers import SAT_ADD_ORDER, SAT_PREFIX, assert_close, case_modes, satisfaction_frame, satisfaction_oracle_inputs
from helpers_mga import exceedance, find_tie, oracle_record, p_values

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-8, 1e-11
SCHEME_ID = {"centroid": 0, "factorial": 1, "path": 2}


def native_model(model, X, col_index=None):
    from plspm import _native
    boff = np.concatenate(([0], np.cumsum([len(b) for b in model.blocks]))).astype(np.int32)
    modes = np.array([0 if m == "A" else 1 for m in model.modes], dtype=np.int32)
    nm = _native.NativeModel(boff, model.C.astype(np.uint8), modes, SCHEME_ID[model.scheme], model.scaled, model.max_iter, model.tol, 0)
    nm.upload(X, col_index)
    return nm


def run_perm(nm, B, n1, seed=0, rep_offset=0, member=None):
    nm.permutation(B, n1, seed, rep_offset, member)
    return nm.fetch(0, 2 * B)


def check_vs_oracle(nm, X, model, B, n1, seed, sample, rep_offset=0):
    from plspm import _native
    rows, status, iters = run_perm(nm, B, n1, seed, rep_offset)
    assert nm.get_option("last_gram_path") == 2
    for p in sample:
        member = _native.permutation_members(seed, rep_offset + p, X.shape[0], n1)
        for k, rows_k in ((0, member), (1, ~member)):
            mine, its = oracle_record(X, model, rows_k)
            assert status[2 * p + k] == 0, (p, k)
            assert iters[2 * p + k] == its, "permutation %d group %d: iterations %d vs oracle %d" % (p, k, iters[2 * p + k], its)
            assert_close(rows[2 * p + k], mine, RTOL, ATOL, what="permutation %d group %d" % (p, k))
    return rows, status, iters


# ------------------------------------------------------------------ the splits
def test_device_splits_are_the_host_mirror_bit_for_bit():
    from plspm import _native
    X, blocks = orc.synth(3000, orc.satisfaction_C(), 10, seed=2)
    model = orc.Model(blocks, orc.satisfaction_C(), "AAAAAA", "path", True)
    nm = native_model(model, X)
    B, seed, n1 = 24, 0xFACE, 1100
    rows, status, iters = run_perm(nm, B, n1, seed)
    member = np.stack([_native.permutation_members(seed, p, 3000, n1) for p in range(B)])
    rows2, status2, iters2 = run_perm(nm, B, n1, member=member)
    assert np.array_equal(rows, rows2, equal_nan=True) and np.array_equal(status, status2) and np.array_equal(iters, iters2)
    a = run_perm(nm, 10, n1, seed, 0)[0]
    b = run_perm(nm, 14, n1, seed, 10)[0]
    assert np.array_equal(np.concatenate((a, b)), rows, equal_nan=True)  # permutations [0, 10) + [10, 24) == [0, 24)


@pytest.mark.parametrize("n,cached", [(6000, True), (200000, False)])
def test_device_splits_with_key_ties_at_the_cut(n, cached):
    """A permutation where two rows share the key of the cut (the row index decides): with the keys in LDS and drawn again per pass."""
    from plspm import _native
    seed = 5
    found = find_tie(seed, n, range(4000))
    assert found is not None
    perm, n1 = found
    C = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0]])
    X, blocks = orc.synth(n, C, 3, seed=8)
    model = orc.Model(blocks, C, "AAA", "path", True)
    nm = native_model(model, X)
    rows, status, iters = run_perm(nm, 1, n1, seed, perm)
    member = _native.permutation_members(seed, perm, n, n1)[None, :]
    rows2, status2, iters2 = run_perm(nm, 1, n1, member=member)
    assert np.array_equal(rows, rows2, equal_nan=True) and np.array_equal(status, status2) and np.array_equal(iters, iters2)


@pytest.mark.parametrize("n1", [1, 36])
def test_device_splits_with_a_tail_piece_and_a_ragged_problem_group(n1):
    """N = 37: two whole 16-row pieces and a tail of five rows, whose mask also bounds the complement's bits; B = 9: a second group of eight permutations
    with one member; n1 = 1 and N - 1: the smallest and the largest rank, and a group of one row, whose fit fails alike in either call."""
    from plspm import _native
    n, B, seed = 37, 9, 41
    C = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0]])
    X, blocks = orc.synth(n, C, 2, seed=14)
    model = orc.Model(blocks, C, "AAA", "path", True)
    nm = native_model(model, X)
    rows, status, iters = run_perm(nm, B, n1, seed)
    member = np.stack([_native.permutation_members(seed, p, n, n1) for p in range(B)])
    assert np.all(member.sum(axis=1) == n1)
    rows2, status2, iters2 = run_perm(nm, B, n1, member=member)
    print("n1 %d: status %s" % (n1, status.tolist()))
    assert np.array_equal(status, status2) and np.array_equal(iters, iters2) and np.array_equal(rows, rows2, equal_nan=True)
    big = 0 if n1 > 1 else 1                                             # the group of 36 rows: the oracle's fit (the tail mask is the same in both calls)
    assert np.all(status[1 - big::2] != 0)                               # the group of one row: a failure, the same in both calls (above)
    for p in (0, B - 1):
        mine, its = oracle_record(X, model, member[p] if big == 0 else ~member[p])
        assert status[2 * p + big] == 0 and iters[2 * p + big] == its, (p, status[2 * p + big], iters[2 * p + big], its)
        assert_close(rows[2 * p + big], mine, RTOL, ATOL, what="permutation %d, the group of 36 rows" % p)


# ------------------------------------------------------------------ parity with the oracle
@pytest.mark.parametrize("modes", ["A", "B", "M"])
@pytest.mark.parametrize("scheme", ["centroid", "factorial", "path"])
@pytest.mark.parametrize("scaled", [False, True])
def test_satisfaction_permutations_vs_oracle(modes, scheme, scaled):
    X, blocks, _ = satisfaction_oracle_inputs()
    model = orc.Model(blocks, orc.satisfaction_C(), case_modes(modes), scheme, scaled)
    nm = native_model(model, X, model.mv_order.astype(np.int32))
    check_vs_oracle(nm, X, model, 6, 148, seed=31, sample=(0, 5), rep_offset=2)


@pytest.mark.parametrize("n1", [5000, 2000])
def test_headline_model_permutations_vs_oracle(n1):
    """10k x 60, 6 LVs, Mode A, PATH, scaled: 50/50 and 20/80 splits."""
    X, blocks = orc.synth(10000, orc.satisfaction_C(), 10, seed=0)
    model = orc.Model(blocks, orc.satisfaction_C(), "AAAAAA", "path", True)
    nm = native_model(model, X)
    rows, status, _ = check_vs_oracle(nm, X, model, 40, n1, seed=4, sample=(0, 39))
    assert np.all(status == 0)


def test_permutations_beyond_one_count_window_vs_oracle():
    """N = 70,000 > 65,536: the counts of a problem span two windows of the fragment layout."""
    C = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0]])
    X, blocks = orc.synth(70000, C, 4, seed=11)
    model = orc.Model(blocks, C, "ABA", "path", True)
    nm = native_model(model, X)
    check_vs_oracle(nm, X, model, 5, 20000, seed=99, sample=(0, 4), rep_offset=3)


def test_permutation_call_leaves_the_bootstrap_unchanged():
    """The permutation call cuts seven digit planes at least; the bootstrap on the same handle keeps its own (automatic) planes and rows."""
    X, blocks = orc.synth(10000, orc.satisfaction_C(), 10, seed=0)
    model = orc.Model(blocks, orc.satisfaction_C(), "AAAAAA", "path", True)
    nm = native_model(model, X)
    before = nm.bootstrap(64, seed=3)
    run_perm(nm, 16, 5000, seed=1)
    after = nm.bootstrap(64, seed=3)
    for x, y in zip(before, after):
        assert np.array_equal(x, y)
    again = run_perm(nm, 16, 5000, seed=1)
    assert np.array_equal(run_perm(nm, 16, 5000, seed=1)[0], again[0])


def test_permutation_refuses_models_outside_the_scope():
    from plspm import _native
    X, blocks = orc.synth(500, orc.satisfaction_C(), 4, seed=3)
    model = orc.Model(blocks, orc.satisfaction_C(), "AAAAAA", "path", True)
    boff = np.concatenate(([0], np.cumsum([len(b) for b in model.blocks]))).astype(np.int32)
    nm = _native.NativeModel(boff, model.C.astype(np.uint8), np.zeros(6, dtype=np.int32), 2, True, 100, 1e-6, 0, nonmetric=True)
    nm.upload(X)
    with pytest.raises(_native.NativeBackendError, match="plain metric"):
        nm.permutation(4, 200, 1)
    nm2 = native_model(model, X)
    with pytest.raises(_native.NativeBackendError, match="n1"):
        nm2.permutation(4, 500, 1)
    bad = np.zeros((1, 500), dtype=bool); bad[0, :199] = True
    with pytest.raises(_native.NativeBackendError, match="n1 ones"):
        nm2.permutation(1, 200, 1, member=bad)


# ------------------------------------------------------------------ exceedance counts
def test_device_exceedance_counts_equal_the_host_counts():
    X, blocks = orc.synth(2000, orc.satisfaction_C(), 5, seed=6)
    model = orc.Model(blocks, orc.satisfaction_C(), "ABABAB", "factorial", True)
    nm = native_model(model, X)
    B, n1 = 300, 700
    rows, status, _ = run_perm(nm, B, n1, seed=21)
    a, _ = oracle_record(X, model, np.arange(2000) < n1)
    b, _ = oracle_record(X, model, np.arange(2000) >= n1)
    d = a - b
    d[3] = np.nan                                                          # NaN observed difference: counts nothing, p is NaN
    d[4] = 0.0                                                             # every valid permutation counts
    exceed, used = nm.permutation_counts(B, d)
    mine, mine_used = exceedance(rows, status, d)
    assert used == mine_used and np.array_equal(exceed, mine)
    assert exceed[3] == 0 and exceed[4] == used
    p = p_values(exceed, used, d)
    assert np.isnan(p[3]) and p[4] == 1.0 and np.all((p[~np.isnan(d)] > 0) & (p[~np.isnan(d)] <= 1))


# ------------------------------------------------------------------ the API
def _sat_config(modes="AAAAAA", scaled=False):
    import plspm.config as c
    from plspm.mode import Mode
    sat = satisfaction_frame()
    s = c.Structure()
    s.add_path(["IMAG"], ["EXPE", "SAT", "LOY"]); s.add_path(["EXPE"], ["QUAL", "VAL", "SAT"])
    s.add_path(["QUAL"], ["VAL", "SAT"]); s.add_path(["VAL"], ["SAT"]); s.add_path(["SAT"], ["LOY"])
    cfg = c.Config(s.path(), scaled=scaled)
    per_lv = dict(zip(orc.SAT_LVS, modes))
    for lv in SAT_ADD_ORDER:
        cfg.add_lv_with_columns_named(lv, Mode.A if per_lv[lv] == "A" else Mode.B, sat, SAT_PREFIX[lv])
    return sat, cfg


def test_satisfaction_by_gender_frames():
    from plspm.mga import GroupComparison
    from plspm.plspm import Plspm
    from plspm.scheme import Scheme
    sat, cfg = _sat_config()
    res = GroupComparison(sat, cfg, "gender", Scheme.PATH, permutations=400, seed=17)
    assert res.groups() == ("female", "male") and res.seed() == 17
    assert 0 < res.used() <= 400
    cols = ["global", "group.female", "group.male", "diff.abs", "p.value", "sig.05"]
    frames = dict(paths=res.paths(), weights=res.weights(), loading=res.loading(), r_squared=res.r_squared(), total_effects=res.total_effects())
    for name, f in frames.items():
        assert list(f.columns) == cols, name
        v = f[cols[:5]].values.astype(np.float64)
        assert np.all(np.isfinite(v)), name
        assert np.all((f["p.value"] > 0) & (f["p.value"] <= 1)), name
        assert np.array_equal(f["sig.05"].values, np.where(f["p.value"] < 0.05, "yes", "no")), name
        assert np.allclose(f["diff.abs"], np.abs(f["group.female"] - f["group.male"]), rtol=0, atol=1e-15), name
    assert len(res.paths()) == 10                                         # the ten structural paths
    # global / the groups: ordinary fits, as Plspm on all rows / the subsets
    for col, rows in (("global", sat), ("group.female", sat[sat["gender"] == "female"]), ("group.male", sat[sat["gender"] == "male"])):
        ref = Plspm(rows, cfg, Scheme.PATH)
        eff = ref.effects()
        assert_close(res.paths()[col], eff.loc[res.paths().index, "direct"], 1e-12, 1e-14, what=col + " paths")
        assert_close(res.total_effects()[col], eff.loc[res.total_effects().index, "total"], 1e-12, 1e-14, what=col + " total")
        om = ref.outer_model()
        assert_close(res.weights()[col], om.loc[res.weights().index, "weight"], 1e-12, what=col + " weights")
        assert_close(res.loading()[col], om.loc[res.loading().index, "loading"], 1e-12, what=col + " loadings")
        assert_close(res.r_squared()[col], ref.inner_summary().loc[res.r_squared().index, "r_squared"], 1e-12, 1e-14, what=col + " r2")
    # p.value = the restatement on the fetched records
    rows, status, _ = res.permutation_records()
    exceed, used = exceedance(rows, status, res.raw["observed_diff"])
    assert used == res.used() and np.array_equal(exceed, res.raw["exceed"])
    p = p_values(exceed, used, res.raw["observed_diff"])
    assert np.array_equal(p, res.raw["p_value"], equal_nan=True)


def _two_groups(seed, n=300, beta_a=0.6, beta_b=0.0):
    """Three LVs in a chain X -> Y -> Z, three MVs each; the groups share every coefficient but X -> Y (beta_a / beta_b)."""
    import plspm.config as c
    from plspm.mode import Mode
    rng = np.random.default_rng(seed)
    frames = []
    for beta, label in ((beta_a, "g1"), (beta_b, "g2")):
        x = rng.standard_normal(n)
        y = beta * x + np.sqrt(1 - beta ** 2) * rng.standard_normal(n)
        z = 0.5 * y + np.sqrt(0.75) * rng.standard_normal(n)
        cols = {}
        for name, lv in (("x", x), ("y", y), ("z", z)):
            for k in range(3):
                cols["%s%d" % (name, k + 1)] = 0.8 * lv + 0.6 * rng.standard_normal(n)
        f = pd.DataFrame(cols)
        f["grp"] = label
        frames.append(f)
    data = pd.concat(frames, ignore_index=True)
    s = c.Structure()
    s.add_path(["X"], ["Y"]); s.add_path(["Y"], ["Z"])
    cfg = c.Config(s.path(), scaled=False)
    for lv, name in (("X", "x"), ("Y", "y"), ("Z", "z")):
        cfg.add_lv_with_columns_named(lv, Mode.A, data, name)
    return data, cfg


def test_a_differing_path_is_found_and_label_swaps_change_nothing():
    from plspm.mga import GroupComparison
    from plspm.scheme import Scheme
    data, cfg = _two_groups(3)
    res = GroupComparison(data, cfg, "grp", Scheme.PATH, permutations=500, seed=9)
    paths = res.paths()
    assert paths.loc["X -> Y", "p.value"] < 0.01 and paths.loc["X -> Y", "sig.05"] == "yes"
    assert paths.loc["Y -> Z", "p.value"] >= 0.01
    swapped = data.copy()
    swapped["grp"] = swapped["grp"].map({"g1": "g2", "g2": "g1"})
    res2 = GroupComparison(swapped, cfg, "grp", Scheme.PATH, permutations=500, seed=9)
    assert np.array_equal(res.raw["p_value"], res2.raw["p_value"], equal_nan=True)
    assert np.array_equal(res.raw["observed_diff"], -res2.raw["observed_diff"])
    for f, g in ((res.paths(), res2.paths()), (res.weights(), res2.weights()), (res.loading(), res2.loading())):
        assert np.array_equal(f["p.value"].values, g["p.value"].values)
        assert np.array_equal(f["group.g1"].values, g["group.g2"].values)
