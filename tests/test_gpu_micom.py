"""GPU: MICOM, the permutation test of measurement invariance (include/plspm_hip.h plspm_micom_*, plspm.micom.Micom).

Kernel against the mirror.  The int8 moments are exact sums, so the device owes only the fp64 arithmetic of the formulas: per permutation the bar is ten times
the largest difference between the fp64 mirror (plspm.micom._micom, computed from the data, not from moment matrices) and the same mirror in np.longdouble,
with a floor of 1e-12 absolute.  On the CPU that difference is at most 5.5e-16 on these shapes, so the floor is the bar everywhere.

Against the ORACLE's fits of the same splits the values can only agree as far as the records do (rtol 1e-8, atol 1e-11, the project's record bar): perturbing
the oracle's weights of the 36 satisfaction splits below inside that bar (20 uniform draws each, helpers_micom.perturbation_figure) moves a MICOM value by
2.001e-9 at most, measured on the CPU; the bar is ten times that."""
import numpy as np
import pandas as pd
import pytest

import helpers_ci
import plspm_oracle as orc
from helpers import SAT_ADD_ORDER, SAT_PREFIX, case_modes, satisfaction_frame, satisfaction_oracle_inputs
from helpers_mga import oracle_record
from helpers_micom import counts, dev_blocks, mirror_bar, mirror_pair, p_values

pytestmark = pytest.mark.gpu
SCHEME_ID = {"centroid": 0, "factorial": 1, "path": 2}
ORACLE_BAR = 10 * 2.001e-9
E_ARG, E_STATE, E_LIMIT = 100, 101, 102
PACKED = dict(solver_wave=0, solver_rows=0, solver_quad=0)      # no dense solver: the batch keeps the tile-packed moments


def native_model(model, X=None, **options):
    from plspm import _native
    boff = np.concatenate(([0], np.cumsum([len(b) for b in model.blocks]))).astype(np.int32)
    modes = np.array([0 if m == "A" else 1 for m in model.modes], dtype=np.int32)
    nm = _native.NativeModel(boff, model.C.astype(np.uint8), modes, SCHEME_ID[model.scheme], model.scaled, model.max_iter, model.tol, 0)
    for key, value in options.items():
        nm.set_option(key, value)
    if X is not None:
        nm.upload(X, model.mv_order.astype(np.int32))
    return nm


def tri(L):
    """Every LV is driven by the one before it."""
    C = np.zeros((L, L), dtype=np.int64)
    for j in range(1, L):
        C[j, j - 1] = 1
    return C


def run(nm, B, n1, seed=0, rep_offset=0, member=None):
    """One permutation call: (MICOM records, their status, the 2B permutation records, status, iterations)."""
    nm.permutation(B, n1, seed, rep_offset, member)
    recs, st = nm.micom_fetch(0, B)
    return (recs, st) + tuple(nm.fetch(0, 2 * B))


def case(name):
    """(X, model, n1, handle options, expected last_micom_layout (None: either), expected last_solver (None: any))."""
    sat = orc.satisfaction_C()
    if name in ("sat24_A_scaled", "sat24_AB_factorial_raw", "sat24_B_centroid"):
        X, blocks = orc.synth(400, sat, 4, seed=21)
        modes, scheme, scaled = {"sat24_A_scaled": ("AAAAAA", "path", True), "sat24_AB_factorial_raw": ("ABABAB", "factorial", False),
                                 "sat24_B_centroid": ("BBBBBB", "centroid", True)}[name]
        return X, orc.Model(blocks, sat, modes, scheme, scaled), 150, {}, 1, None
    if name == "tiny_60x9":                                   # groups of 12 and 48 rows: no slack in n / (n - 1)
        X, blocks = orc.synth(60, tri(3), 3, seed=13)
        return X, orc.Model(blocks, tri(3), "AAA", "centroid", True), 12, {}, 1, None
    if name == "single_item":
        X, _ = orc.synth(300, tri(3), 3, seed=22)
        X = np.ascontiguousarray(X[:, [0, 3, 4, 5, 6, 7, 8]])
        return X, orc.Model([np.arange(1), np.arange(1, 4), np.arange(4, 7)], tri(3), "AAA", "path", True), 110, {}, 1, None
    if name == "block_of_65":                                 # a block that spans two lane windows, behind a block (its R_0 block does not start the buffer)
        X, _ = orc.synth(300, tri(3), 65, seed=23)
        X = np.ascontiguousarray(X[:, np.concatenate((np.arange(5), np.arange(65, 130), np.arange(130, 135)))])
        return X, orc.Model([np.arange(5), np.arange(5, 70), np.arange(70, 75)], tri(3), "AAA", "factorial", True), 130, {}, None, None
    if name == "quad_120x12":
        X, blocks = orc.synth(1500, orc.chain_C(12), 10, seed=24)
        return X, orc.Model(blocks, orc.chain_C(12), "A" * 12, "centroid", True), 600, {}, 1, 5
    if name == "packed_40":
        X, blocks = orc.synth(300, tri(4), 10, seed=25)
        return X, orc.Model(blocks, tri(4), "AAAA", "path", False), 140, PACKED, 2, 1
    raise KeyError(name)


CASES = ["sat24_A_scaled", "sat24_AB_factorial_raw", "sat24_B_centroid", "tiny_60x9", "single_item", "block_of_65", "quad_120x12", "packed_40"]


def check_against_mirror(recs, rows, Xdev, model, members, w_0, tag):
    P, worst, bar = model.P, 0.0, np.inf
    blocks = dev_blocks(model)
    for r, member in enumerate(members):
        m64, mld = mirror_pair(Xdev, member, rows[2 * r, :P], rows[2 * r + 1, :P], w_0, blocks)
        this_bar = mirror_bar(m64, mld)
        diff = float(np.max(np.abs(recs[r] - m64)))
        worst, bar = max(worst, diff), min(bar, this_bar)
        assert np.all(np.isfinite(recs[r])), (tag, r)
        assert diff <= this_bar, "%s permutation %d: max |device - mirror| %.3e above the bar %.3e" % (tag, r, diff, this_bar)
    print("%s: max |device - mirror| %.3e over %d permutations (smallest bar %.3e)" % (tag, worst, len(members), bar))


# ------------------------------------------------------------------ 1. the kernel against the mirror
@pytest.mark.parametrize("name", CASES)
def test_kernel_against_the_mirror(name):
    from plspm import _native
    X, model, n1, options, layout, solver = case(name)
    nm = native_model(model, X, **options)
    nm.micom_enable(True)
    assert nm.micom_width == 3 * model.L
    B, seed, N = 9, 0xC0DE, X.shape[0]                        # two workgroups and one wave
    recs, st, rows, status, _ = run(nm, B, n1, seed)
    assert recs.shape == (B, 3 * model.L) and np.all(st == 0) and np.all(status == 0)
    assert nm.get_option("last_gram_path") == 2
    got = nm.get_option("last_micom_layout")
    assert got == layout if layout is not None else got in (1, 2)
    if solver is not None:
        assert nm.get_option("last_solver") == solver
    fit = nm.fit(want_scores=False)
    assert fit["status"] == 0
    members = [_native.permutation_members(seed, p, N, n1) for p in range(B)]
    check_against_mirror(recs, rows, X[:, model.mv_order], model, members, fit["weights"], name)
    if name == "single_item":
        assert np.all(np.abs(recs[:, 0] - 1.0) <= 4e-16)      # one item: both composites are the item


def test_both_layouts_run():
    """The two instantiations of the kernel on ONE model and one set of splits: dense moments under the wave solver, tile-packed ones under the LDS solver."""
    from plspm import _native
    X, model, n1, _, _, _ = case("sat24_A_scaled")
    B, seed = 9, 5
    members = [_native.permutation_members(seed, p, X.shape[0], n1) for p in range(B)]
    for name, options in (("dense", {}), ("packed", PACKED)):
        nm = native_model(model, X, **options)
        nm.micom_enable(True)
        recs, st, rows, status, _ = run(nm, B, n1, seed)
        assert nm.get_option("last_micom_layout") == (1 if name == "dense" else 2)
        assert (nm.get_option("last_solver") == 1) == (name == "packed")
        assert np.all(st == 0)
        check_against_mirror(recs, rows, X[:, model.mv_order], model, members, nm.fit(want_scores=False)["weights"], name)


# ------------------------------------------------------------------ 2. against the oracle's fits
@pytest.mark.parametrize("modes", ["A", "B", "M"])
@pytest.mark.parametrize("scheme", ["centroid", "factorial", "path"])
@pytest.mark.parametrize("scaled", [False, True])
def test_satisfaction_against_the_oracles_fits(modes, scheme, scaled):
    from plspm import _native
    from plspm.micom import _micom
    X, blocks, _ = satisfaction_oracle_inputs()
    model = orc.Model(blocks, orc.satisfaction_C(), case_modes(modes), scheme, scaled)
    nm = native_model(model, X)
    nm.micom_enable(True)
    B, n1, seed, rep_offset, N, P = 6, 148, 31, 2, X.shape[0], model.P
    recs, st, _, _, _ = run(nm, B, n1, seed, rep_offset)
    assert np.all(st == 0)
    w_0 = oracle_record(X, model, np.ones(N, dtype=bool))[0][:P]
    worst = 0.0
    for p in (0, 5):
        member = _native.permutation_members(seed, rep_offset + p, N, n1)
        w_a, w_b = oracle_record(X, model, member)[0][:P], oracle_record(X, model, ~member)[0][:P]
        worst = max(worst, float(np.max(np.abs(recs[p] - _micom(X[:, model.mv_order], member, w_a, w_b, w_0, dev_blocks(model))))))
    print("MICOM against the mirror on the oracle's fits: max |difference| %.3e (bar %.3e)" % (worst, ORACLE_BAR))
    assert worst <= ORACLE_BAR


# ------------------------------------------------------------------ 3. the hook
def test_three_passes_equal_one():
    X, model, n1, _, _, _ = case("sat24_A_scaled")
    B, seed = 300, 8
    one = native_model(model, X)
    one.micom_enable(True)
    whole = run(one, B, n1, seed)
    assert one.get_option("last_boot_passes") == 1
    nm = native_model(model, X, boot_pass=256)
    nm.micom_enable(True)
    cut = run(nm, B, n1, seed)
    assert nm.get_option("last_boot_passes") == 3             # 600 problems as 256 + 256 + 88: permutations 0, 128 and 256 start a pass
    for x, y in zip(whole, cut):
        assert np.array_equal(x, y, equal_nan=True)
    assert np.all(whole[1] == 0) and np.all(np.isfinite(whole[0]))
    assert len(np.unique(whole[0][[0, 128, 256], 0])) == 3    # every pass wrote its own permutations' records
    tail, _ = nm.micom_fetch(255, 3)
    assert np.array_equal(tail, whole[0][255:258])


def test_ranges_with_rep_offset_and_micom_off_and_the_bootstrap():
    from plspm import _native
    X, model, n1, _, _, _ = case("sat24_AB_factorial_raw")
    seed = 0xFACE
    nm = native_model(model, X)
    before = nm.bootstrap(64, seed=3)
    plain = run_plain(nm, 24, n1, seed)
    with pytest.raises(_native.NativeBackendError, match=r"plspm_micom_fetch failed \(%d\)" % E_STATE):
        nm.micom_fetch(0, 1)                                  # MICOM off: nothing written, nothing allocated
    nm.micom_enable(True)
    recs, st, rows, status, iters = run(nm, 24, n1, seed)
    # the permutation's own records, status and iteration counts: bit-identical with MICOM on and off
    assert np.array_equal(plain[0], rows, equal_nan=True) and np.array_equal(plain[1], status) and np.array_equal(plain[2], iters)
    a = run(nm, 10, n1, seed, 0)
    b = run(nm, 14, n1, seed, 10)
    assert np.array_equal(np.concatenate((a[0], b[0])), recs, equal_nan=True)      # permutations [0, 10) + [10, 24) == [0, 24)
    assert np.array_equal(np.concatenate((a[1], b[1])), st)
    # explicit memberships: the same records as the on-device splits
    member = np.stack([_native.permutation_members(seed, p, X.shape[0], n1) for p in range(24)])
    c = run(nm, 24, n1, member=member)
    assert np.array_equal(c[0], recs, equal_nan=True)
    after = nm.bootstrap(64, seed=3)
    for x, y in zip(before, after):
        assert np.array_equal(x, y)
    with pytest.raises(_native.NativeBackendError, match=r"plspm_micom_fetch failed \(%d\)" % E_STATE):
        nm.micom_fetch(0, 1)                                  # the bootstrap replaced the handle's records
    nm.micom_enable(False)
    nm.permutation(24, n1, seed)
    with pytest.raises(_native.NativeBackendError, match=r"plspm_micom_fetch failed \(%d\)" % E_STATE):
        nm.micom_fetch(0, 1)


def run_plain(nm, B, n1, seed):
    nm.permutation(B, n1, seed)
    return nm.fetch(0, 2 * B)


# ------------------------------------------------------------------ 4. a failed half
def test_a_failed_half_is_nan_and_not_used():
    """60 x 9 with groups of 12 and 48 rows, tolerance 1e-10 and at most 12 iterations: on the oracle, of the 16 splits of seed 77, two (permutations 1 and 2)
    have a half that needs more (39 and 13 iterations; the others 7 .. 11).  Such a permutation's record is NaN with that half's status; summary, intervals and
    counts leave it out."""
    from plspm import _native
    from plspm.bootstrap import _create_summary
    X, model, n1, _, _, _ = case("tiny_60x9")
    model.tol, model.max_iter = 1e-10, 12
    nm = native_model(model, X)
    nm.micom_enable(True)
    B, seed = 16, 77
    recs, st, rows, status, iters = run(nm, B, n1, seed)
    failed = (status[0::2] != 0) | (status[1::2] != 0)
    assert 1 <= failed.sum() <= B // 2
    assert np.array_equal(failed, np.isin(np.arange(B), (1, 2)))
    expect = np.where(status[0::2] != 0, status[0::2], status[1::2])
    assert np.array_equal(st, expect)
    assert np.all(np.isnan(recs[failed])) and np.all(np.isfinite(recs[~failed]))
    ok = np.flatnonzero(~failed)
    members = [_native.permutation_members(seed, int(p), X.shape[0], n1) for p in ok]
    keep = np.stack((2 * ok, 2 * ok + 1), axis=1).reshape(-1)
    # (the pooled fit under the same settings: 60 rows, converged)
    fit = nm.fit(want_scores=False)
    assert fit["status"] == 0
    check_against_mirror(recs[ok], rows[keep], X[:, model.mv_order], model, members, fit["weights"], "beside failed permutations")
    original = recs[ok[0]]
    table, used = nm.micom_summary(B, original)
    assert used == B - failed.sum()
    host = _create_summary(pd.DataFrame(recs[ok]), pd.Series(original)).values
    np.testing.assert_allclose(table, host, rtol=1e-12, atol=1e-15)
    below, exceed, used_c = nm.micom_counts(B, original)
    mine = counts(recs, st, original)
    assert used_c == used and np.array_equal(below, mine[0]) and np.array_equal(exceed, mine[1])
    _, used_i = nm.micom_intervals(B, original, "percentile", 0.9)
    assert used_i == used


# ------------------------------------------------------------------ 5. counts and quantiles
def test_counts_and_intervals_equal_the_restatement():
    from plspm import _native
    X, model, n1, _, _, _ = case("sat24_AB_factorial_raw")
    L = model.L
    nm = native_model(model, X)
    with pytest.raises(_native.NativeBackendError, match=r"plspm_micom_counts failed \(%d\)" % E_STATE):
        nm.micom_counts(10, np.zeros(3 * L))
    nm.micom_enable(True)
    B = 300
    recs, st, _, _, _ = run(nm, B, n1, 21)
    member = np.arange(X.shape[0]) < n1
    observed = run(nm, 1, n1, member=member[None, :])[0][0]
    assert np.all(np.isfinite(observed))
    recs2, st2, _, _, _ = run(nm, B, n1, 21)
    assert np.array_equal(recs, recs2) and np.array_equal(st, st2)
    observed = observed.copy()
    observed[1] = np.nan                                      # a NaN observed value: counts nothing, p is NaN
    observed[L + 2] = 0.0                                     # an observed dmean of 0: every valid permutation is at least as far out
    below, exceed, used = nm.micom_counts(B, observed)
    mine = counts(recs, st, observed)
    assert used == mine[2] == int((st == 0).sum()) and np.array_equal(below, mine[0]) and np.array_equal(exceed, mine[1])
    assert below[1] == 0 and exceed[1] == 0 and exceed[L + 2] == used
    p = p_values(below, exceed, used, observed, L)
    assert np.isnan(p[1]) and p[L + 2] == 1.0
    fin = ~np.isnan(observed)
    assert np.all((p[fin] > 0) & (p[fin] <= 1))
    ok = recs[st == 0]
    for method in ("percentile", "basic", "bc"):
        for level in (0.9, 0.95):
            out, used_i = nm.micom_intervals(B, observed, method, level)
            mirror = helpers_ci.intervals(ok, observed, method, level)
            assert used_i == used and np.array_equal(np.isnan(out), np.isnan(mirror)), method
            np.testing.assert_allclose(out[:, :2], mirror[:, :2], rtol=1e-12, atol=1e-15, err_msg=method)
            np.testing.assert_allclose(out[:, 2:], mirror[:, 2:], rtol=1e-12, atol=1e-12, err_msg=method)      # (z0 and the levels: atol as tests/test_gpu_ci.py)
    # ... and bit for bit plspm_bootstrap_intervals' rule on the same columns: the MICOM records stored as bootstrap records of another handle
    with pytest.raises(_native.NativeBackendError, match=r"plspm_micom_intervals failed \(%d\)" % E_ARG):
        nm.micom_intervals(B, observed, "bca", 0.95)
    with pytest.raises(_native.NativeBackendError, match=r"plspm_micom_summary failed \(%d\)" % E_ARG):
        nm.micom_summary(B - 1, observed)
    with pytest.raises(_native.NativeBackendError, match=r"plspm_micom_counts failed \(%d\)" % E_ARG):
        nm.micom_counts(B + 1, observed)
    with pytest.raises(_native.NativeBackendError, match=r"plspm_micom_fetch failed \(%d\)" % E_ARG):
        nm.micom_fetch(B - 1, 2)
    # a jackknife leaves the handle's records alone, and with them the MICOM records; an upload voids both
    nm.jackknife(16)
    again, _ = nm.micom_fetch(0, B)
    assert np.array_equal(again, recs, equal_nan=True)
    nm.upload(X, model.mv_order.astype(np.int32))
    with pytest.raises(_native.NativeBackendError, match=r"plspm_micom_fetch failed \(%d\)" % E_STATE):
        nm.micom_fetch(0, 1)


def test_intervals_are_the_bootstrap_rule_bit_for_bit():
    """plspm_micom_intervals against plspm_bootstrap_intervals on the same numbers: a model whose bootstrap record is as wide as the MICOM record of another."""
    X, model, n1, _, _, _ = case("sat24_A_scaled")
    nm = native_model(model, X)
    nm.micom_enable(True)
    B, W = 200, 3 * model.L
    recs, st, _, _, _ = run(nm, B, n1, 4)
    original = recs[0].copy()
    # a two-LV model with one item per block has records of 2 P + L + 2 n_eff = 4 + 2 + 2 = 8 columns; the MICOM columns go through it eight at a time
    Y, _ = orc.synth(50, tri(2), 1, seed=1)
    other = native_model(orc.Model([np.arange(1), np.arange(1, 2)], tri(2), "AA", "centroid", True), Y)
    R = other.row_width
    for level in (0.9, 0.95):
        mine, used = nm.micom_intervals(B, original, "percentile", level)
        for c0 in range(0, W, R):
            cols = np.arange(c0, min(c0 + R, W))
            block = np.zeros((B, R + 2))
            block[:, :cols.size] = recs[:, cols]
            block[:, R] = st
            other.store(block)
            orig = np.zeros(R)
            orig[:cols.size] = original[cols]
            theirs, used_b = other.intervals(B, orig, "percentile", level)
            assert used_b == used
            assert np.array_equal(mine[cols], theirs[:cols.size], equal_nan=True)


# ------------------------------------------------------------------ 6. scope
def test_scope_and_limits():
    from plspm import _native
    boff = np.array([0, 4, 8, 12], dtype=np.int32)
    path, modes = tri(3).astype(np.uint8), np.zeros(3, dtype=np.int32)
    nonmetric = _native.NativeModel(boff, path, modes, 0, True, 100, 1e-6, 0, nonmetric=True)
    with pytest.raises(_native.NativeBackendError, match="plain metric"):
        nonmetric.micom_enable(True)
    ind_of = np.full(12, -1, dtype=np.int32)
    ind_of[2] = 12
    missing = _native.NativeModel(boff, path, modes, 0, True, 100, 1e-6, 0, missing=ind_of)
    with pytest.raises(_native.NativeBackendError, match="plain metric"):
        missing.micom_enable(True)
    with pytest.raises(_native.NativeBackendError, match="plain metric"):
        missing.micom_counts(4, np.zeros(9))
    from test_gpu_hoc import handles
    first, second, *_ = handles("path_B")                     # a two-stage (higher-order construct) pair: neither handle takes MICOM
    first.attach_second_stage(second, [0, 1, 2, 4, 5, 6])
    for handle in (first, second):
        with pytest.raises(_native.NativeBackendError, match="plain metric"):
            handle.micom_enable(True)
    X, model, n1, _, _, _ = case("tiny_60x9")
    nm = native_model(model, X)
    with pytest.raises(_native.NativeBackendError, match=r"plspm_micom_fetch failed \(%d\)" % E_STATE):
        nm.micom_fetch(0, 1)
    # The LDS limit cannot be reached: a wave's slice is 4 k_max doubles (csrc/kernels_micom.h micom_wave_doubles), four waves a workgroup, and a handle has at most
    # 1,022 MVs -- 4 x 4 x 1,022 x 8 = 130,816 bytes, below the 160 KiB.  So there is no shape that must get PLSPM_E_LIMIT; the widest block the route of the
    # 65-item case takes is covered above.
    assert 4 * 4 * 1022 * 8 < 160 * 1024


# ------------------------------------------------------------------ 7. the API
def sat_config():
    import plspm.config as c
    from plspm.mode import Mode
    sat = satisfaction_frame()
    s = c.Structure()
    s.add_path(["IMAG"], ["EXPE", "SAT", "LOY"]); s.add_path(["EXPE"], ["QUAL", "VAL", "SAT"])
    s.add_path(["QUAL"], ["VAL", "SAT"]); s.add_path(["VAL"], ["SAT"]); s.add_path(["SAT"], ["LOY"])
    cfg = c.Config(s.path(), scaled=False)
    for lv in SAT_ADD_ORDER:
        cfg.add_lv_with_columns_named(lv, Mode.A, sat, SAT_PREFIX[lv])
    return sat, cfg


def check_frames(res, lvs):
    comp, means, var, summ = res.compositional(), res.means(), res.variances(), res.summary()
    assert list(comp.columns) == ["c", "quantile", "p.value", "invariant"]
    assert list(means.columns) == list(var.columns) == ["diff", "lower", "upper", "p.value", "equal"]
    assert list(summ.columns) == ["compositional", "equal.means", "equal.variances", "invariance"]
    for f in (comp, means, var, summ):
        assert list(f.index) == lvs
    assert np.all(np.isfinite(comp[["c", "quantile", "p.value"]].values.astype(np.float64)))
    assert np.array_equal(comp["invariant"].values, comp["c"].values >= comp["quantile"].values)
    for f in (means, var):
        assert np.all(np.isfinite(f[["diff", "lower", "upper", "p.value"]].values.astype(np.float64)))
        assert np.array_equal(f["equal"].values, (f["lower"].values <= f["diff"].values) & (f["diff"].values <= f["upper"].values))
    for f in (comp, means, var):
        assert np.all((f["p.value"] > 0) & (f["p.value"] <= 1))
    full = comp["invariant"].values & means["equal"].values & var["equal"].values
    assert np.array_equal(summ["invariance"].values, np.where(full, "full", np.where(comp["invariant"].values, "partial", "none")))


def test_satisfaction_by_gender_frames():
    from plspm.micom import Micom
    from plspm.scheme import Scheme
    sat, cfg = sat_config()
    B = 400
    res = Micom(sat, cfg, "gender", Scheme.PATH, permutations=B, seed=17)
    assert res.groups() == ("female", "male") and res.seed() == 17
    assert 0 < res.used() <= B
    check_frames(res, orc.SAT_LVS)
    # the frames are the restatement on the fetched records
    recs, st = res.records()
    L, observed = 6, res.raw["observed"]
    assert recs.shape == (B, 3 * L) and res.raw["observed_status"] == 0
    below, exceed, used = counts(recs, st, observed)
    assert used == res.used() and np.array_equal(below, res.raw["below"]) and np.array_equal(exceed, res.raw["exceed"])
    p = p_values(below, exceed, used, observed, L)
    assert np.array_equal(p, res.raw["p_value"])
    ok = recs[st == 0]
    one = helpers_ci.intervals(ok, observed, "percentile", 0.9)
    two = helpers_ci.intervals(ok, observed, "percentile", 0.95)
    np.testing.assert_allclose(res.compositional()["quantile"].values, one[:L, 0], rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(res.means()["lower"].values, two[L:2 * L, 0], rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(res.variances()["upper"].values, two[2 * L:, 1], rtol=1e-12, atol=1e-15)
    assert np.array_equal(res.compositional()["p.value"].values, p[:L]) and np.array_equal(res.means()["p.value"].values, p[L:2 * L])
    assert np.array_equal(res.variances()["p.value"].values, p[2 * L:])
    assert np.array_equal(res.compositional()["c"].values, observed[:L]) and np.array_equal(res.variances()["diff"].values, observed[2 * L:])


def two_groups(seed, n=300):
    """Three LVs in a chain X -> Y -> Z, three MVs each (loadings 0.8).  In group g2 the third indicator of X loads 0.1 instead, and its Y indicators are shifted
    by +1."""
    import plspm.config as c
    from plspm.mode import Mode
    rng = np.random.default_rng(seed)
    frames = []
    for label in ("g1", "g2"):
        x = rng.standard_normal(n)
        y = 0.5 * x + np.sqrt(0.75) * rng.standard_normal(n)
        z = 0.5 * y + np.sqrt(0.75) * rng.standard_normal(n)
        cols = {}
        for name, lv in (("x", x), ("y", y), ("z", z)):
            for k in range(3):
                lam = 0.1 if (label == "g2" and name == "x" and k == 2) else 0.8
                cols["%s%d" % (name, k + 1)] = lam * lv + np.sqrt(1 - lam ** 2) * rng.standard_normal(n) + (1.0 if (label == "g2" and name == "y") else 0.0)
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


def test_a_broken_indicator_and_a_shifted_block_are_found_and_label_swaps_change_nothing():
    from plspm.micom import Micom
    from plspm.scheme import Scheme
    data, cfg = two_groups(3)
    res = Micom(data, cfg, "grp", Scheme.PATH, permutations=500, seed=9)
    check_frames(res, ["X", "Y", "Z"])
    comp, means = res.compositional(), res.means()
    assert not comp.loc["X", "invariant"] and comp.loc["X", "p.value"] < 0.01
    assert not means.loc["Y", "equal"] and means.loc["Y", "p.value"] < 0.01
    assert means.loc["X", "equal"] and means.loc["Z", "equal"]
    assert res.summary().loc["X", "invariance"] == "none" and res.summary().loc["Y", "invariance"] in ("partial", "none")
    swapped = data.copy()
    swapped["grp"] = swapped["grp"].map({"g1": "g2", "g2": "g1"})
    res2 = Micom(swapped, cfg, "grp", Scheme.PATH, permutations=500, seed=9)
    L = 3
    assert np.array_equal(res.raw["p_value"], res2.raw["p_value"])
    assert np.array_equal(res.raw["observed"][:L], res2.raw["observed"][:L])              # c: bit-identical
    assert np.array_equal(res.raw["observed"][L:], -res2.raw["observed"][L:])             # dmean, dlogvar: the sign flips
    assert np.array_equal(res.compositional()["invariant"].values, res2.compositional()["invariant"].values)
