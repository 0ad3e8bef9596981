"""GPU: confirmatory tetrad analysis of bootstrap replicates (include/plspm_hip.h plspm_tetrad_*; csrc/kernels_tetrad.h, csrc/tetrad_core.h; plspm.tetrad).

Kernel against the mirror.  The int8 moments are exact sums, so the device owes only the fp64 arithmetic of the definitions.  Tetrads cancel, so the bar is
absolute: per replicate ten times the largest difference, on the same resampled rows, between the fp64 mirror (plspm.tetrad._tetrads) and the same mirror in
np.longdouble, never below 1e-12 (the project's mirror_bar rule).  That difference measured on the CPU (tools/tetrad_floor.py), per case over the nine
resamples and all rows, correlation / covariance:

    k4 6.6e-16 / 5.1e-16   k3_4_13 1.0e-15 / 5.9e-16   all_7 1.3e-15 / 1.2e-15   lds_65_5 1.3e-15 / 9.6e-16   wave_60x6 1.1e-15 / 2.4e-15
    quad_120x12 1.1e-15 / 1.6e-15   packed_40 1.1e-15 / 9.1e-16   fp64_gram 8.8e-16 / 8.3e-16   mode_b 8.3e-16 / 6.3e-16   two_waves 9.2e-16 / 8.7e-16

so the floor of 1e-12 is the bar everywhere.  The shapes are the smallest at which the kernel takes another path: one testable block of four beside a block
of three (one lane pair of work, a skipped block); blocks of 3, 4 and 13 (2 + 65 basis tetrads: the lanes go round twice, one tetrad in the second round);
"all" on a block of 7 (70 tetrads); a block of 65 items (its 64 staged columns -- the first column has no row above it -- fill one window, every lane busy;
tile-packed layout, odd tile count, LDS solver) and one of 66 (64 + 2: the first size whose last column is staged by a second trip of the window loop); the routes and layouts of tests/test_gpu_quality.py (dense wave, quad with MVs past column 64, tile-packed with every dense solver off, fp64 Gram, a
Mode-B block); and 16 blocks of 24 items (384 MVs, 4,032 tetrads), the smallest equal-block model whose slice of 5,185 doubles makes tetrad_plan give two
waves per workgroup.  B = 9 replicates on explicit indices: more than one workgroup and a workgroup that is not full."""
import numpy as np
import pandas as pd
import pytest

import plspm_oracle as orc
from helpers import SAT_ADD_ORDER, SAT_PREFIX, satisfaction_frame
from helpers_tetrad import CASES, FLOOR, MATRICES, case, dev_blocks, mirror_bar, mirror_pair, native_model, resamples, tri
from plspm.tetrad import _decision_table, _tetrads

pytestmark = pytest.mark.gpu
E_ARG, E_STATE, E_LIMIT = 100, 101, 102


def check_against_mirror(recs, X, model, idx, tetrads, matrix, tag):
    """Every tetrad record against the mirror on that replicate's rows; returns the fp64 mirrors."""
    worst, bar, mirrors = 0.0, np.inf, []
    for r in range(recs.shape[0]):
        m64, mld = mirror_pair(X[idx[r]][:, model.mv_order], model, tetrads, matrix)
        assert m64["status"] == 0 and mld["status"] == 0, (tag, r)
        this_bar = mirror_bar(m64, mld)
        diff = float(np.max(np.abs(recs[r] - m64["tetrads"])))
        worst, bar = max(worst, diff), min(bar, this_bar)
        assert np.all(np.isfinite(recs[r])), (tag, r)
        assert diff <= this_bar, "%s replicate %d: max |device - mirror| %.3e above the bar %.3e" % (tag, r, diff, this_bar)
        mirrors.append(m64)
    print("%s: max |device - mirror| %.3e over %d replicates (smallest bar %.3e)" % (tag, worst, recs.shape[0], bar))
    return mirrors


def device_list(nm):
    block, a, b, c, d = nm.tetrad_list()
    return [tuple(int(v) for v in row) for row in np.stack((block, a, b, c, d), axis=1)]


@pytest.mark.parametrize("matrix", MATRICES)
@pytest.mark.parametrize("name", CASES)
def test_kernel_against_the_mirror(name, matrix):
    X, model, options, tetrads, solver, gram_path = case(name)
    nm = native_model(model, X, **options)
    assert nm.tetrad_width == 0
    nm.tetrad_enable(True, None, tetrads, matrix)
    B = 9
    idx = resamples(X, B)
    rows, status, iters = nm.bootstrap(B, idx=idx)
    assert np.all(status == 0)
    if gram_path is not None:
        assert nm.get_option("last_gram_path") == gram_path
    if solver is not None:
        assert nm.get_option("last_solver") == solver
    recs, st = nm.tetrad_fetch(0, B)
    assert np.all(st == 0) and recs.shape == (B, nm.tetrad_width)
    mirrors = check_against_mirror(recs, X, model, idx, tetrads, matrix, "%s %s" % (name, matrix))
    # the host's lists against the mirror's
    assert device_list(nm) == mirrors[0]["list"]
    widths = {"k4": 2, "k3_4_13": 67, "all_7": 70, "lds_65_5": 2015 + 5, "window_66": 2079 + 5, "wave_60x6": 210, "quad_120x12": 420, "two_waves": 4032}
    if name in widths:
        assert nm.tetrad_width == widths[name]
    # the full-sample record: the same kernel on the moments of all rows
    full, fst = nm.tetrad_fit()
    m64, mld = mirror_pair(X[:, model.mv_order], model, tetrads, matrix)
    diff = float(np.max(np.abs(full - m64["tetrads"])))
    print("%s %s: plspm_tetrad_fit max |device - mirror| %.3e (bar %.3e)" % (name, matrix, diff, mirror_bar(m64, mld)))
    assert fst == 0 and diff <= mirror_bar(m64, mld)


def test_a_mask_and_the_refusals():
    from plspm import _native
    X, model, _, _, _, _ = case("k3_4_13")
    nm = native_model(model, X)
    with pytest.raises(_native.NativeBackendError, match=r"plspm_tetrad_list failed \(%d\)" % E_STATE):
        nm.tetrad_list()
    with pytest.raises(_native.NativeBackendError, match=r"plspm_tetrad_enable failed \(%d\).*LV 0" % E_ARG):
        nm.tetrad_enable(True, [1, 1, 0])
    with pytest.raises(_native.NativeBackendError, match=r"plspm_tetrad_enable failed \(%d\)" % E_ARG):
        nm.tetrad_enable(True, [0, 0, 0])
    with pytest.raises(_native.NativeBackendError, match=r"plspm_tetrad_enable failed \(%d\)" % E_ARG):
        nm.tetrad_enable(True, None, 2, 0)
    nm.tetrad_enable(True, [0, 0, 1])                        # the block of 13 alone
    B = 9
    idx = resamples(X, B)
    nm.bootstrap(B, idx=idx)
    recs, st = nm.tetrad_fetch(0, B)
    whole = native_model(model, X)
    whole.tetrad_enable(True)
    whole.bootstrap(B, idx=idx)
    both, _ = whole.tetrad_fetch(0, B)
    assert recs.shape == (B, 65) and np.array_equal(recs, both[:, 2:]) and {row[0] for row in device_list(nm)} == {2}
    # no testable block; too many tetrads (the count is in the message); a handle kind the analysis does not cover
    X3, _ = orc.synth(50, tri(2), 3, seed=1)
    small = native_model(orc.Model([np.arange(3), np.arange(3, 6)], tri(2), "AA", "centroid", True), X3)
    with pytest.raises(_native.NativeBackendError, match=r"plspm_tetrad_enable failed \(%d\)" % E_ARG):
        small.tetrad_enable(True)
    X17, _ = orc.synth(50, tri(2), 17, seed=1)
    wide = native_model(orc.Model([np.arange(17), np.arange(17, 34)], tri(2), "AA", "centroid", True), X17)
    with pytest.raises(_native.NativeBackendError, match=r"plspm_tetrad_enable failed \(%d\).*9520 tetrads" % E_LIMIT):
        wide.tetrad_enable(True, None, "all")
    boff = np.array([0, 4, 8, 12], dtype=np.int32)
    other = _native.NativeModel(boff, tri(3).astype(np.uint8), np.zeros(3, dtype=np.int32), 0, True, 100, 1e-6, 0, nonmetric=True)
    with pytest.raises(_native.NativeBackendError, match=r"plspm_tetrad_enable failed \(%d\).*plain metric models only" % E_ARG):
        other.tetrad_enable(True)


def run_stages(X, model, idx, tetrad, stages):
    """One bootstrap with every derived stage and a moderation term on or off and the tetrad switch on or off: every record there is."""
    nm = native_model(model, X)
    if stages:
        nm.assess_enable(True); nm.structural_enable(True); nm.plsc_enable(True); nm.modelfit_enable(True); nm.geodesic_enable(True)
        nm.moderation_enable([(0, 1, 4)])
    if tetrad:
        nm.tetrad_enable(True)
    B = idx.shape[0]
    out = {"rows": nm.bootstrap(B, idx=idx)}
    if stages:
        for family in ("assess", "structural", "plsc", "modelfit", "geodesic", "moderation"):
            out[family] = getattr(nm, family + "_fetch")(0, B)
    if tetrad:
        out["tetrad"] = nm.tetrad_fetch(0, B)
    else:
        with pytest.raises(Exception, match=r"plspm_tetrad_fetch failed \(%d\)" % E_STATE):
            nm.tetrad_fetch(0, 1)
    return out


def test_the_switch_changes_no_other_record_and_no_stage_changes_the_tetrads():
    X, model, _, _, _, _ = case("wave_60x6")
    idx = resamples(X, 9)
    tetrads = []
    for stages in (False, True):
        off, on = run_stages(X, model, idx, False, stages), run_stages(X, model, idx, True, stages)
        for key, value in off.items():
            for a, b in zip(value, on[key]):
                assert np.array_equal(a, b, equal_nan=True), (stages, key)
        tetrads.append(on["tetrad"])
    assert np.array_equal(tetrads[0][0], tetrads[1][0]) and np.array_equal(tetrads[0][1], tetrads[1][1])
    assert np.all(tetrads[0][1] == 0) and np.all(np.isfinite(tetrads[0][0]))


def small_model(seed=9, n=320):
    X, blocks = orc.synth(n, tri(3), 4, seed=seed)
    return X, orc.Model(blocks, tri(3), "AAA", "centroid", True)


def test_a_second_pass_of_one_replicate():
    from plspm import _native
    X, model = small_model()
    one = native_model(model, X)
    one.tetrad_enable(True)
    B, seed = 257, 41
    one.bootstrap_device(B, seed, 0)
    one.sync()
    whole, st = one.tetrad_fetch(0, B)
    assert one.get_option("last_boot_passes") == 1
    two = native_model(model, X, boot_pass=256)
    two.tetrad_enable(True)
    rows, status, _ = two.bootstrap(B, seed=seed)
    assert two.get_option("last_boot_passes") == 2
    passes, st2 = two.tetrad_fetch(0, B)
    assert np.array_equal(whole, passes, equal_nan=True) and np.array_equal(st, st2) and np.array_equal(st2, status) and np.all(status == 0)
    pick = np.array([0, 255, 256])
    idx = np.stack([_native.bootstrap_indices(seed, int(r), X.shape[0]) for r in pick])
    check_against_mirror(passes[pick], X, model, idx, "basis", "correlation", "second pass")
    tail, _ = two.tetrad_fetch(255, 2)                       # a range that starts behind the first pass
    assert np.array_equal(tail, passes[255:])


def test_sub_batches_write_at_their_offset_and_leave_the_bootstrap_alone():
    """plspm_bootstrap() as three sub-batches against one plspm_bootstrap_device batch.  The planner makes no part shorter than 512 replicates, so three
    parts take 1,537 replicates of this 12-MV model (a few milliseconds)."""
    from plspm import _native
    X, model = small_model()
    B, seed = 1537, 7
    plain = native_model(model, X, boot_chunks=3, boot_align=64)
    rows0, status0, iters0 = plain.bootstrap(B, seed=seed)
    nm = native_model(model, X, boot_chunks=3, boot_align=64)
    nm.tetrad_enable(True)
    parts = _native.chunk_plan(B, nm.row_stride * 8, 3, 60, 64)
    assert len(parts) == 3 and sum(parts) == B, parts
    rows1, status1, iters1 = nm.bootstrap(B, seed=seed)      # three sub-batches, each with its offset
    chunked, st1 = nm.tetrad_fetch(0, B)
    assert np.array_equal(rows0, rows1) and np.array_equal(status0, status1) and np.array_equal(iters0, iters1)
    nm.bootstrap_device(B, seed, 0)                          # one batch
    nm.sync()
    whole, st2 = nm.tetrad_fetch(0, B)
    assert np.array_equal(chunked, whole, equal_nan=True) and np.array_equal(st1, st2) and np.array_equal(st1, status1)
    assert np.all(np.isfinite(whole[st2 == 0]))
    pick = np.array([0, parts[0], parts[0] + parts[1], B - 1])
    assert np.all(st1[pick] == 0)
    idx = np.stack([_native.bootstrap_indices(seed, int(r), X.shape[0]) for r in pick])
    check_against_mirror(chunked[pick], X, model, idx, "basis", "correlation", "sub-batches")


def test_failed_replicates_are_nan_and_not_used():
    from plspm.bootstrap import _create_summary
    X, model = small_model()
    B = 24
    idx = np.random.default_rng(3).integers(0, X.shape[0], (B, X.shape[0])).astype(np.int32)
    _, status, iters = native_model(model, X).bootstrap(B, idx=idx)
    assert np.all(status == 0) and iters.min() < iters.max()
    cut = int(iters.min())                                   # replicates that need more iterations than this do not converge below
    model.max_iter = cut
    nm = native_model(model, X)
    nm.tetrad_enable(True)
    rows, status, _ = nm.bootstrap(B, idx=idx)
    failed = status != 0
    assert 0 < failed.sum() < B and np.array_equal(failed, iters > cut)
    recs, st = nm.tetrad_fetch(0, B)
    assert np.array_equal(st, status)
    assert np.all(np.isnan(recs[failed])) and np.all(np.isfinite(recs[~failed]))
    check_against_mirror(recs[~failed], X, model, idx[~failed], "basis", "correlation", "beside failed replicates")
    original = recs[~failed][0]
    table, used = nm.tetrad_summary(B, original)
    assert used == B - failed.sum()
    host = _create_summary(pd.DataFrame(recs[~failed]), pd.Series(original)).values
    np.testing.assert_allclose(table, host, rtol=1e-12, atol=1e-15)


@pytest.mark.parametrize("matrix", MATRICES)
def test_a_column_that_is_constant_in_a_resample(matrix):
    """The metric solver keeps status PLSPM_OK for such a replicate; its standard deviation is zero, so under "correlation" the tetrads of the block are not
    finite and the record's status is 3, and under "covariance" they are finite numbers, the mirror's."""
    X, model = small_model()
    X = X.copy()
    X[:6, 0] = 1.25                                          # six rows share one value in column 0
    nm = native_model(model, X)
    nm.tetrad_enable(True, None, "basis", matrix)
    B = 5
    idx = np.random.default_rng(3).integers(0, X.shape[0], (B, X.shape[0])).astype(np.int32)
    idx[2] = np.random.default_rng(4).integers(0, 6, X.shape[0])      # replicate 2 draws those rows only
    rows, status, _ = nm.bootstrap(B, idx=idx)
    assert np.all(status == 0)
    recs, st = nm.tetrad_fetch(0, B)
    keep = np.array([0, 1, 3, 4])
    assert np.all(st[keep] == 0)
    check_against_mirror(recs[keep], X, model, idx[keep], "basis", matrix, "beside a constant column")
    m64 = _tetrads(X[idx[2]][:, model.mv_order], dev_blocks(model), "basis", matrix)
    if matrix == "correlation":
        assert st[2] == 3 and m64["status"] == 3
        assert not np.any(np.isfinite(recs[2, :2])) and np.all(np.isfinite(recs[2, 2:]))          # both tetrads of block 0 have item 0 in them
        np.testing.assert_allclose(recs[2, 2:], m64["tetrads"][2:], rtol=0, atol=FLOOR)
        _, used = nm.tetrad_summary(B, recs[0])
        assert used == B - 1
    else:
        assert st[2] == 0 and m64["status"] == 0 and np.all(np.isfinite(recs[2]))
        np.testing.assert_allclose(recs[2], m64["tetrads"], rtol=0, atol=FLOOR)


def test_summary_intervals_and_errors():
    from plspm import _native
    from plspm.bootstrap import _create_summary, _intervals
    X, model = small_model(seed=12)
    nm = native_model(model, X)
    with pytest.raises(_native.NativeBackendError, match=r"plspm_tetrad_fit failed \(%d\)" % E_STATE):
        nm.tetrad_fit()
    nm.tetrad_enable(True)
    with pytest.raises(_native.NativeBackendError, match=r"plspm_tetrad_summary failed \(%d\)" % E_STATE):
        nm.tetrad_summary(100, np.zeros(nm.tetrad_width))
    B = 200
    nm.bootstrap_device(B, 5, 0)
    recs, st = nm.tetrad_fetch(0, B)
    original, _ = nm.tetrad_fit()
    ok = recs[st == 0]
    table, used = nm.tetrad_summary(B, original)
    assert used == ok.shape[0] and used >= B - 2
    host = _create_summary(pd.DataFrame(ok), pd.Series(original)).values
    np.testing.assert_allclose(table, host, rtol=1e-12, atol=1e-15)
    for method in ("percentile", "basic", "bc"):
        for level in (0.95, 1.0 - 0.05 / 2):                 # the second: the Bonferroni level of a block of four
            out, used_i = nm.tetrad_intervals(B, original, method, level)
            mirror = _intervals(ok, original, None, method, level)
            assert used_i == used and np.array_equal(np.isnan(out), np.isnan(mirror))
            np.testing.assert_allclose(out[:, :2], mirror[:, :2], rtol=1e-12, atol=1e-15, err_msg=method)
            np.testing.assert_allclose(out[:, 2:], mirror[:, 2:], rtol=1e-12, atol=1e-12, err_msg=method)      # (z0 and the levels: atol as tests/test_gpu_ci.py)
    with pytest.raises(_native.NativeBackendError, match=r"plspm_tetrad_intervals failed \(%d\)" % E_ARG):
        nm.tetrad_intervals(B, original, 3, 0.95)            # method 3: no bca
    with pytest.raises(_native.NativeBackendError, match=r"plspm_tetrad_summary failed \(%d\)" % E_ARG):
        nm.tetrad_summary(B - 1, original)                   # B differs
    with pytest.raises(_native.NativeBackendError, match=r"plspm_tetrad_fetch failed \(%d\)" % E_ARG):
        nm.tetrad_fetch(B - 1, 2)                            # the range
    # a jackknife leaves the records alone; switching off writes none and voids them with the next bootstrap; an upload voids them
    nm.jackknife(16)
    again, _ = nm.tetrad_fetch(0, B)
    assert np.array_equal(again, recs, equal_nan=True)
    nm.tetrad_enable(False)
    nm.bootstrap_device(B, 5, 0)
    with pytest.raises(_native.NativeBackendError, match=r"plspm_tetrad_fetch failed \(%d\)" % E_STATE):
        nm.tetrad_fetch(0, 1)
    nm.tetrad_enable(True)
    nm.bootstrap_device(B, 5, 0)
    back, _ = nm.tetrad_fetch(0, B)
    assert np.array_equal(back, recs, equal_nan=True)
    nm.upload(X, model.mv_order.astype(np.int32))
    with pytest.raises(_native.NativeBackendError, match=r"plspm_tetrad_fetch failed \(%d\)" % E_STATE):
        nm.tetrad_fetch(0, 1)


def sat_config():
    import plspm.config as c
    from plspm.mode import Mode
    sat = satisfaction_frame()
    s = c.Structure()
    s.add_path(["IMAG"], ["EXPE", "SAT", "LOY"]); s.add_path(["EXPE"], ["QUAL", "VAL", "SAT"])
    s.add_path(["QUAL"], ["VAL", "SAT"]); s.add_path(["VAL"], ["SAT"]); s.add_path(["SAT"], ["LOY"])
    cfg = c.Config(s.path(), scaled=True)
    for lv in SAT_ADD_ORDER:
        cfg.add_lv_with_columns_named(lv, Mode.A, sat, SAT_PREFIX[lv])
    return sat, cfg


def test_tetrad_frames_and_the_decision():
    from plspm import _native
    from plspm.bootstrap import INTERVAL_COLUMNS, SUMMARY_COLUMNS
    from plspm.plspm import Plspm
    from plspm.scheme import Scheme
    from plspm.tetrad import TetradAnalysis
    sat, cfg = sat_config()
    lvs = orc.SAT_LVS
    B, seed = 200, 3
    ta = TetradAnalysis(sat, cfg, Scheme.PATH, iterations=B, seed=seed)
    via = Plspm(sat, cfg, Scheme.PATH, bootstrap=True, bootstrap_iterations=B, seed=seed, tetrads=True, quality=True, structural=True).tetrads()
    cm = ta._cm
    sizes = np.diff(cm.block_offset)
    n_tet = int(sum(k * (k - 3) // 2 for k in sizes))
    frame = ta.tetrads()
    assert list(frame.columns) == ["block", "a", "b", "c", "d", "tetrad"] and frame.shape[0] == n_tet and ta.status() == 0
    first = cm.dev_mvs[:4]
    assert frame.index[0] == "%s: %s,%s,%s,%s" % (lvs[0], first[0], first[2], first[3], first[1]) and frame["block"].iloc[0] == lvs[0]
    for name in ("tetrads", "summary", "decision"):
        pd.testing.assert_frame_equal(getattr(ta, name)(), getattr(via, name)())
    pd.testing.assert_frame_equal(ta.intervals(), via.intervals())
    assert ta.used() == via.used() == B and ta.records().shape == (B, n_tet) and ta.seed() == seed
    s = ta.summary()
    assert list(s.columns) == SUMMARY_COLUMNS and list(s.index) == list(frame.index) and np.array_equal(s["original"].values, frame["tetrad"].values)
    iv = ta.intervals()
    assert list(iv.columns) == INTERVAL_COLUMNS + ["level"] and np.all(iv["lower"].values <= iv["upper"].values)
    fixed = ta.intervals("percentile", 0.95)
    assert list(fixed.columns) == INTERVAL_COLUMNS and np.array_equal(fixed["lower"].values, s["perc.025"].values)
    with pytest.raises(NotImplementedError):
        ta.intervals("bca")
    with pytest.raises(Exception, match="tetrads"):
        Plspm(sat, cfg, Scheme.PATH).tetrads()
    # the mirror on the same resamples: the full sample, the records, the Bonferroni levels and the decision
    Xd = cfg.filter(sat).values[:, cm.col_index].astype(np.float64)
    blocks = [np.arange(cm.block_offset[l], cm.block_offset[l + 1]) for l in range(cm.L)]
    full = _tetrads(Xd, blocks)
    assert float(np.max(np.abs(frame["tetrad"].values - full["tetrads"]))) <= FLOOR
    idx = np.stack([_native.bootstrap_indices(seed, r, Xd.shape[0]) for r in range(B)])
    records = np.stack([_tetrads(Xd[rows], blocks)["tetrads"] for rows in idx])
    assert float(np.max(np.abs(ta.records() - records))) <= FLOOR
    block_of = np.array([l for l, *_ in full["list"]])
    rows, table = _decision_table(full["tetrads"], records, block_of, 0.05)
    decision = ta.decision()
    assert list(decision.index) == lvs and list(decision.columns) == ["items", "tetrads", "level", "nonvanishing", "reflective"]
    assert decision["items"].tolist() == sizes.tolist() and decision["tetrads"].tolist() == [r[1] for r in rows]
    assert decision["level"].tolist() == [r[2] for r in rows] and np.array_equal(iv["level"].values, table[:, 0])
    margin = np.minimum(np.abs(table[:, 1]), np.abs(table[:, 2]))
    print("decision: nonvanishing device %s mirror %s; the mirror's bound nearest to zero %.3e" % (decision["nonvanishing"].tolist(), [r[3] for r in rows], margin.min()))
    assert decision["nonvanishing"].tolist() == [r[3] for r in rows]
    assert decision["reflective"].tolist() == ["rejected" if r[3] > 0 else "not rejected" for r in rows]
    # a subset of blocks and the other set through the class
    sub = TetradAnalysis(sat, cfg, Scheme.PATH, iterations=100, seed=seed, blocks=["VAL", "LOY"], tetrads="all", matrix="covariance", alpha=0.1)
    d = sub.decision()
    assert list(d.index) == ["VAL", "LOY"] and d["tetrads"].tolist() == [2, 2] and d["level"].tolist() == [0.95, 0.95]
