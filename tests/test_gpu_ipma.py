"""GPU: importance-performance map analysis of bootstrap replicates (include/plspm_hip.h plspm_ipma_*; csrc/kernels_ipma.h, csrc/ipma_core.h; plspm.ipma).

Kernel against the mirror.  The int8 moments are exact sums, so the device owes only the fp64 arithmetic of the definitions.  The bar is the project's
mirror_bar rule per field (tests/helpers_ipma.py): per replicate ten times the largest difference, on the same resampled rows and the device's own bootstrap
record, between the fp64 mirror (plspm.ipma._ipma) and the same mirror in np.longdouble, never below 1e-12 times the field's scale -- 100 for perf, mvperf
and sd, 1 for the rest.  That difference measured on the CPU (tools/ipma_floor.py, on the oracle's fits of the nine resamples and all rows, observed
bounds) stays below 4e-14 on the 0-100 scale and below 3e-16 on the rest in every case, so the floors, 1e-10 and 1e-12, are the bars everywhere.

Statuses are compared with the mirror's wherever the mirror's smallest |weight_r_p| exceeds the bar of the weights; at most one of a case's nine replicates
may be left out on that ground (on the oracle's fits the smallest of any case is 8e-4, so none should be).

The shapes are those of tests/test_gpu_tetrad.py (the generators are copied into tests/helpers_ipma.py): blocks of 3 and 4; of 3, 4 and 13; a block of 65
items (lane 0 of phase 2 takes a second item of the same block; tile-packed layout, LDS solver) and one of 66; the routes and layouts of
tests/test_gpu_quality.py (dense wave, quad with MVs past column 64, tile-packed with every dense solver off, fp64 Gram, a Mode-B block, whose negative
weights make replicates inadmissible); and 16 blocks of 24 items (384 MVs: six rounds of the lanes over the MVs, fifteen targets).  B = 9 replicates on
explicit indices: more than one workgroup and a workgroup that is not full.  Every case runs with the observed bounds and with fixed bounds wider than
the data."""
import numpy as np
import pandas as pd
import pytest

import plspm_oracle as orc
from helpers import SAT_ADD_ORDER, SAT_PREFIX, satisfaction_frame
from helpers_ipma import (CASES, case, check_record, dev_blocks, field_bars, mirror_pair, native_model, observed_bounds, resamples, status_is_decided, tri, wider_bounds)
from plspm.ipma import FIELDS, _ipma, _layout

pytestmark = pytest.mark.gpu
E_ARG, E_STATE, E_LIMIT = 100, 101, 102
BOUNDS = {"observed": observed_bounds, "wider": wider_bounds}


def pairs_of(nm):
    return list(zip(nm.eff_from.tolist(), nm.eff_to.tolist()))


def full_record(nm):
    fit = nm.fit(want_scores=False)
    assert fit["status"] == 0
    return np.concatenate((fit["weights"], fit["r2"], fit["total"], fit["direct"], fit["loadings"]))


def check_against_mirror(recs, st, rows, X, model, idx, pairs, lo, hi, tag, targets=None):
    """Every IPMA record against the mirror on that replicate's rows and the device's own bootstrap record; returns (the fp64 mirrors, replicates left out
    of the status comparison)."""
    worst, mirrors, left_out = {name: 0.0 for name in FIELDS}, [], 0
    for r in range(recs.shape[0]):
        m64, mld = mirror_pair(X[idx[r]][:, model.mv_order], model, rows[r], pairs, lo, hi, targets)
        for name, diff in check_record(recs[r], m64, mld, "%s replicate %d" % (tag, r)).items():
            worst[name] = max(worst[name], diff)
        if status_is_decided(m64, mld):
            assert st[r] == m64["status"], "%s replicate %d: status %d, the mirror's %d (smallest |weight_r| %.3e)" % (tag, r, st[r], m64["status"], m64["min_abs_weight"])
        else:
            left_out += 1
        mirrors.append(m64)
    print("%s: max |device - mirror| per field %s over %d replicates" % (tag, {k: "%.1e" % v for k, v in worst.items()}, recs.shape[0]))
    return mirrors, left_out


@pytest.mark.parametrize("bounds", ["observed", "wider"])
@pytest.mark.parametrize("name", CASES)
def test_kernel_against_the_mirror(name, bounds):
    X, model, options, solver, gram_path = case(name)
    nm = native_model(model, X, **options)
    assert nm.ipma_width == 0
    lo, hi = BOUNDS[bounds](X, model)
    nm.ipma_enable(True, None, lo, hi)
    pairs = pairs_of(nm)
    targets = sorted({t for _, t in pairs})
    assert nm.ipma_targets().tolist() == targets and nm.ipma_width == _layout(model.P, model.L, len(pairs), len(targets))[1]
    B = 9
    idx = resamples(X, B)
    rows, status, iters = nm.bootstrap(B, idx=idx)
    assert np.all(status == 0)
    if gram_path is not None:
        assert nm.get_option("last_gram_path") == gram_path
    if solver is not None:
        assert nm.get_option("last_solver") == solver
    recs, st = nm.ipma_fetch(0, B)
    assert recs.shape == (B, nm.ipma_width) and np.all(np.isfinite(recs)) and set(st.tolist()) <= {0, 4}
    mirrors, left_out = check_against_mirror(recs, st, rows, X, model, idx, pairs, lo, hi, "%s %s" % (name, bounds))
    assert left_out <= 1
    admissible = int(np.count_nonzero(st == 0))
    full, fst = nm.ipma_fit()
    _, used = nm.ipma_summary(B, full)
    assert used == admissible                              # an inadmissible replicate is counted and not used
    if name == "mode_b":
        assert int(np.count_nonzero(st == 4)) >= 1 and used >= 7
    else:
        assert admissible == B
    # the full-sample record: the same kernel on the moments of all rows
    m64, mld = mirror_pair(X[:, model.mv_order], model, full_record(nm), pairs, lo, hi)
    worst = check_record(full, m64, mld, "%s %s plspm_ipma_fit" % (name, bounds))
    print("%s %s: plspm_ipma_fit max |device - mirror| per field %s" % (name, bounds, {k: "%.1e" % v for k, v in worst.items()}))
    assert fst == m64["status"] == 0


def test_a_target_mask_and_the_refusals():
    from plspm import _native
    X, model, _, _, _ = case("wave_60x6")
    lo, hi = observed_bounds(X, model)
    nm = native_model(model, X)
    with pytest.raises(_native.NativeBackendError, match=r"plspm_ipma_targets failed \(%d\)" % E_STATE):
        nm.ipma_targets()
    with pytest.raises(_native.NativeBackendError, match=r"plspm_ipma_fit failed \(%d\)" % E_STATE):
        nm.ipma_fit()
    with pytest.raises(_native.NativeBackendError, match=r"plspm_ipma_enable failed \(%d\).*LV 0 has no predecessor" % E_ARG):
        nm.ipma_enable(True, [1, 0, 0, 0, 0, 1], lo, hi)
    with pytest.raises(_native.NativeBackendError, match=r"plspm_ipma_enable failed \(%d\).*names no LV" % E_ARG):
        nm.ipma_enable(True, [0] * 6, lo, hi)
    bad = hi.copy(); bad[17] = lo[17]
    with pytest.raises(_native.NativeBackendError, match=r"plspm_ipma_enable failed \(%d\).*MV 17" % E_ARG):
        nm.ipma_enable(True, None, lo, bad)
    bad = lo.copy(); bad[3] = np.nan
    with pytest.raises(_native.NativeBackendError, match=r"plspm_ipma_enable failed \(%d\).*MV 3" % E_ARG):
        nm.ipma_enable(True, None, bad, hi)
    assert nm.ipma_width == 0
    nm.ipma_enable(True, [0, 0, 0, 0, 0, 1], lo, hi)         # LOY alone
    assert nm.ipma_targets().tolist() == [5]
    B = 9
    idx = resamples(X, B)
    rows, _, _ = nm.bootstrap(B, idx=idx)
    recs, st = nm.ipma_fetch(0, B)
    whole = native_model(model, X)
    whole.ipma_enable(True, None, lo, hi)
    whole.bootstrap(B, idx=idx)
    both, _ = whole.ipma_fetch(0, B)
    pairs = pairs_of(nm)
    at1, w1 = _layout(60, 6, len(pairs), 1)
    at5, w5 = _layout(60, 6, len(pairs), 5)
    assert recs.shape == (B, w1) and both.shape == (B, w5)
    assert np.array_equal(recs[:, :at1["mvimp"].start], both[:, :at5["mvimp"].start]) and np.array_equal(recs[:, at1["mvimp"]], both[:, at5["mvimp"].start + 4 * 60:])
    check_against_mirror(recs, st, rows, X, model, idx, pairs, lo, hi, "LOY alone", targets=[5])
    # a handle kind the analysis does not cover
    boff = np.array([0, 4, 8, 12], dtype=np.int32)
    other = _native.NativeModel(boff, tri(3).astype(np.uint8), np.zeros(3, dtype=np.int32), 0, True, 100, 1e-6, 0, nonmetric=True)
    with pytest.raises(_native.NativeBackendError, match=r"plspm_ipma_enable failed \(%d\).*plain metric models only" % E_ARG):
        other.ipma_enable(True, None, np.zeros(12), np.ones(12))


def run_stages(X, model, idx, ipma, others, lo, hi):
    """One bootstrap with every derived stage, a moderation term and the tetrads on or off and the IPMA switch on or off: every record there is."""
    nm = native_model(model, X)
    if others:
        nm.assess_enable(True); nm.structural_enable(True); nm.plsc_enable(True); nm.modelfit_enable(True); nm.geodesic_enable(True)
        nm.moderation_enable([(0, 1, 4)])
        nm.tetrad_enable(True)
    if ipma:
        nm.ipma_enable(True, None, lo, hi)
    B = idx.shape[0]
    out = {"rows": nm.bootstrap(B, idx=idx)}
    if others:
        for family in ("assess", "structural", "plsc", "modelfit", "geodesic", "moderation", "tetrad"):
            out[family] = getattr(nm, family + "_fetch")(0, B)
    if ipma:
        out["ipma"] = nm.ipma_fetch(0, B)
    else:
        with pytest.raises(Exception, match=r"plspm_ipma_fetch failed \(%d\)" % E_STATE):
            nm.ipma_fetch(0, 1)
    return out


def test_the_switch_changes_no_other_record_and_no_other_switch_changes_the_ipma():
    X, model, _, _, _ = case("wave_60x6")
    idx = resamples(X, 9)
    lo, hi = observed_bounds(X, model)
    records = []
    for others in (False, True):
        off, on = run_stages(X, model, idx, False, others, lo, hi), run_stages(X, model, idx, True, others, lo, hi)
        for key, value in off.items():
            for a, b in zip(value, on[key]):
                assert np.array_equal(a, b, equal_nan=True), (others, key)
        records.append(on["ipma"])
    assert np.array_equal(records[0][0], records[1][0]) and np.array_equal(records[0][1], records[1][1])
    assert np.all(records[0][1] == 0) and np.all(np.isfinite(records[0][0]))


def small_model(seed=9, n=320):
    X, blocks = orc.synth(n, tri(3), 4, seed=seed)
    return X, orc.Model(blocks, tri(3), "AAA", "centroid", True)


def test_a_second_pass_of_one_replicate():
    from plspm import _native
    X, model = small_model()
    lo, hi = wider_bounds(X, model)
    one = native_model(model, X)
    one.ipma_enable(True, None, lo, hi)
    B, seed = 257, 41
    one.bootstrap_device(B, seed, 0)
    one.sync()
    whole, st = one.ipma_fetch(0, B)
    assert one.get_option("last_boot_passes") == 1
    two = native_model(model, X, boot_pass=256)
    two.ipma_enable(True, None, lo, hi)
    rows, status, _ = two.bootstrap(B, seed=seed)
    assert two.get_option("last_boot_passes") == 2
    passes, st2 = two.ipma_fetch(0, B)
    assert np.array_equal(whole, passes, equal_nan=True) and np.array_equal(st, st2) and np.all(status == 0)
    pick = np.array([0, 255, 256])
    idx = np.stack([_native.bootstrap_indices(seed, int(r), X.shape[0]) for r in pick])
    check_against_mirror(passes[pick], st2[pick], rows[pick], X, model, idx, pairs_of(two), lo, hi, "second pass")
    tail, _ = two.ipma_fetch(255, 2)                         # a range that starts behind the first pass
    assert np.array_equal(tail, passes[255:])


def test_sub_batches_write_at_their_offset_and_leave_the_bootstrap_alone():
    """plspm_bootstrap() as three sub-batches against one plspm_bootstrap_device batch.  The planner makes no part shorter than 512 replicates, so three
    parts take 1,537 replicates of this 12-MV model (a few milliseconds)."""
    from plspm import _native
    X, model = small_model()
    lo, hi = observed_bounds(X, model)
    B, seed = 1537, 7
    plain = native_model(model, X, boot_chunks=3, boot_align=64)
    rows0, status0, iters0 = plain.bootstrap(B, seed=seed)
    nm = native_model(model, X, boot_chunks=3, boot_align=64)
    nm.ipma_enable(True, None, lo, hi)
    parts = _native.chunk_plan(B, nm.row_stride * 8, 3, 60, 64)
    assert len(parts) == 3 and sum(parts) == B, parts
    rows1, status1, iters1 = nm.bootstrap(B, seed=seed)      # three sub-batches, each with its offset
    chunked, st1 = nm.ipma_fetch(0, B)
    assert np.array_equal(rows0, rows1) and np.array_equal(status0, status1) and np.array_equal(iters0, iters1)
    nm.bootstrap_device(B, seed, 0)                          # one batch
    nm.sync()
    whole, st2 = nm.ipma_fetch(0, B)
    assert np.array_equal(chunked, whole, equal_nan=True) and np.array_equal(st1, st2)
    assert np.all(np.isfinite(whole[status1 == 0]))
    pick = np.array([0, parts[0], parts[0] + parts[1], B - 1])
    assert np.all(status1[pick] == 0)
    idx = np.stack([_native.bootstrap_indices(seed, int(r), X.shape[0]) for r in pick])
    check_against_mirror(chunked[pick], st1[pick], rows1[pick], X, model, idx, pairs_of(nm), lo, hi, "sub-batches")


def test_failed_replicates_are_nan_and_not_used():
    from plspm.bootstrap import _create_summary
    X, model = small_model()
    lo, hi = observed_bounds(X, model)
    B = 24
    idx = np.random.default_rng(3).integers(0, X.shape[0], (B, X.shape[0])).astype(np.int32)
    _, status, iters = native_model(model, X).bootstrap(B, idx=idx)
    assert np.all(status == 0) and iters.min() < iters.max()
    cut = int(iters.min())                                   # replicates that need more iterations than this do not converge below
    model.max_iter = cut
    nm = native_model(model, X)
    nm.ipma_enable(True, None, lo, hi)
    rows, status, _ = nm.bootstrap(B, idx=idx)
    failed = status != 0
    assert 0 < failed.sum() < B and np.array_equal(failed, iters > cut)
    recs, st = nm.ipma_fetch(0, B)
    assert np.array_equal(st[failed], status[failed])
    assert np.all(np.isnan(recs[failed])) and np.all(np.isfinite(recs[~failed])) and np.all(st[~failed] == 0)
    check_against_mirror(recs[~failed], st[~failed], rows[~failed], X, model, idx[~failed], pairs_of(nm), lo, hi, "beside failed replicates")
    original = recs[~failed][0]
    table, used = nm.ipma_summary(B, original)
    assert used == B - failed.sum()
    host = _create_summary(pd.DataFrame(recs[~failed]), pd.Series(original)).values
    vary = recs[~failed].std(axis=0) > 0                     # (a column of exact zeros -- the target's own importances -- has no t statistic to compare)
    np.testing.assert_allclose(table[vary], host[vary], rtol=1e-12, atol=1e-13)
    assert np.array_equal(table[~vary, :2], host[~vary, :2])


def test_a_column_that_is_constant_in_a_resample():
    """The metric solver keeps status PLSPM_OK for such a replicate and gives the item weight 0; its standard deviation is zero, so its block's rescaled
    weights are 0 * inf: status 3, the values standing -- the entries of the other blocks are the mirror's -- and the replicate is not used."""
    X, model = small_model()
    X = X.copy()
    X[:6, 0] = 1.25                                          # six rows share one value in column 0
    lo, hi = observed_bounds(X, model)
    nm = native_model(model, X)
    nm.ipma_enable(True, None, lo, hi)
    B = 5
    idx = np.random.default_rng(3).integers(0, X.shape[0], (B, X.shape[0])).astype(np.int32)
    idx[2] = np.random.default_rng(4).integers(0, 6, X.shape[0])      # replicate 2 draws those rows only
    rows, status, _ = nm.bootstrap(B, idx=idx)
    assert np.all(status == 0)
    recs, st = nm.ipma_fetch(0, B)
    keep = np.array([0, 1, 3, 4])
    pairs = pairs_of(nm)
    assert np.all(st[keep] == 0)
    check_against_mirror(recs[keep], st[keep], rows[keep], X, model, idx[keep], pairs, lo, hi, "beside a constant column")
    m64, mld = mirror_pair(X[idx[2]][:, model.mv_order], model, rows[2], pairs, lo, hi)
    at, _ = _layout(12, 3, len(pairs), 2)
    assert st[2] == 3 and m64["status"] == 3 and mld["status"] == 3
    assert not np.any(np.isfinite(recs[2][at["weight_r"]][:4])) and np.all(np.isfinite(recs[2][at["weight_r"]][4:])) and np.all(np.isfinite(recs[2][at["mvperf"]]))
    worst = check_record(recs[2], m64, mld, "the replicate with the constant column")      # (the same entries finite, and those within the bar of their field)
    print("the replicate with the constant column: max |device - mirror| per field %s" % {k: "%.1e" % v for k, v in worst.items()})
    _, used = nm.ipma_summary(B, recs[0])
    assert used == B - 1


def test_summary_intervals_and_errors():
    from plspm import _native
    from plspm.bootstrap import _create_summary, _intervals
    X, model = small_model(seed=12)
    lo, hi = wider_bounds(X, model)
    nm = native_model(model, X)
    nm.ipma_enable(True, None, lo, hi)
    with pytest.raises(_native.NativeBackendError, match=r"plspm_ipma_summary failed \(%d\)" % E_STATE):
        nm.ipma_summary(100, np.zeros(nm.ipma_width))
    with pytest.raises(_native.NativeBackendError, match=r"plspm_ipma_intervals failed \(%d\)" % E_STATE):
        nm.ipma_intervals(100, np.zeros(nm.ipma_width))
    B = 200
    nm.bootstrap_device(B, 5, 0)
    recs, st = nm.ipma_fetch(0, B)
    original, _ = nm.ipma_fit()
    ok = recs[st == 0]
    table, used = nm.ipma_summary(B, original)
    assert used == ok.shape[0] and used >= B - 2
    host = _create_summary(pd.DataFrame(ok), pd.Series(original)).values
    vary = ok.std(axis=0) > 0                                # (a column of exact zeros -- the target's own importances -- has no t statistic and no interval to compare)
    np.testing.assert_allclose(table[vary], host[vary], rtol=1e-12, atol=1e-13)
    assert np.array_equal(table[~vary, :2], host[~vary, :2]) and np.all(table[~vary, :2] == 0.0)
    for method in ("percentile", "basic", "bc"):
        out, used_i = nm.ipma_intervals(B, original, method, 0.95)
        mirror = _intervals(ok, original, None, method, 0.95)
        assert used_i == used and np.array_equal(np.isnan(out[vary]), np.isnan(mirror[vary]))
        np.testing.assert_allclose(out[vary, :2], mirror[vary, :2], rtol=1e-12, atol=1e-13, err_msg=method)
        np.testing.assert_allclose(out[vary, 2:], mirror[vary, 2:], rtol=1e-12, atol=1e-12, err_msg=method)      # (z0 and the levels: atol as tests/test_gpu_ci.py)
    with pytest.raises(_native.NativeBackendError, match=r"plspm_ipma_intervals failed \(%d\)" % E_ARG):
        nm.ipma_intervals(B, original, 3, 0.95)              # method 3: no bca
    with pytest.raises(_native.NativeBackendError, match=r"plspm_ipma_summary failed \(%d\)" % E_ARG):
        nm.ipma_summary(B - 1, original)                     # B differs
    with pytest.raises(_native.NativeBackendError, match=r"plspm_ipma_fetch failed \(%d\)" % E_ARG):
        nm.ipma_fetch(B - 1, 2)                              # the range
    # a jackknife leaves the records alone; switching off writes none and voids them with the next bootstrap; an upload voids them
    nm.jackknife(16)
    again, _ = nm.ipma_fetch(0, B)
    assert np.array_equal(again, recs, equal_nan=True)
    nm.ipma_enable(False)
    nm.bootstrap_device(B, 5, 0)
    with pytest.raises(_native.NativeBackendError, match=r"plspm_ipma_fetch failed \(%d\)" % E_STATE):
        nm.ipma_fetch(0, 1)
    nm.ipma_enable(True, None, lo, hi)
    nm.bootstrap_device(B, 5, 0)
    back, _ = nm.ipma_fetch(0, B)
    assert np.array_equal(back, recs, equal_nan=True)
    nm.upload(X, model.mv_order.astype(np.int32))
    with pytest.raises(_native.NativeBackendError, match=r"plspm_ipma_fetch failed \(%d\)" % E_STATE):
        nm.ipma_fetch(0, 1)


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


def test_ipma_frames_and_scores():
    from plspm import _native
    from plspm.bootstrap import INTERVAL_COLUMNS, SUMMARY_COLUMNS
    from plspm.ipma import Ipma
    from plspm.plspm import Plspm
    from plspm.scheme import Scheme
    sat, cfg = sat_config()
    lvs = orc.SAT_LVS
    B, seed = 200, 3
    ip = Ipma(sat, cfg, Scheme.PATH, targets=["LOY"], scale=(0, 10), iterations=B, seed=seed)
    via = Plspm(sat, cfg, Scheme.PATH, bootstrap=True, bootstrap_iterations=B, seed=seed, ipma=dict(targets=["LOY"], scale=(0, 10)), quality=True, structural=True,
                tetrads=True).ipma()
    cm = ip._cm
    P, L = cm.P, cm.L
    assert ip.status() == 0 and ip.seed() == seed and ip.used() + ip.inadmissible() == B and ip.used() == via.used()
    for name in ("performance", "weights", "total_effects", "path_coefficients", "constructs", "indicators"):
        pd.testing.assert_frame_equal(getattr(ip, name)(), getattr(via, name)())
    pd.testing.assert_frame_equal(ip.summary("importance"), via.summary("importance"))
    pd.testing.assert_frame_equal(ip.intervals("performance"), via.intervals("performance"))
    pd.testing.assert_frame_equal(ip.scores(), via.scores(), check_exact=True)      # (the same kernels on the same rows: no switch changes the fit or the IPMA record)
    # the mirror on the full sample and on the same resamples, fed the device's own bootstrap records
    Xd = cfg.filter(sat).values[:, cm.col_index].astype(np.float64)
    blocks = [np.arange(cm.block_offset[l], cm.block_offset[l + 1]) for l in range(L)]
    lo, hi = np.zeros(P), np.full(P, 10.0)
    native = ip._native
    pairs = pairs_of(native)
    loy = lvs.index("LOY")
    full = _ipma(Xd, blocks, full_record(native), pairs, lo, hi, [loy])
    assert full["status"] == 0
    cons, ind, perf, wts = ip.constructs("LOY"), ip.indicators(), ip.performance(), ip.weights()
    ante = [f for f, t in pairs if t == loy]
    assert list(cons.index) == [lvs[f] for f in ante] and list(cons.columns) == ["importance", "performance"]
    np.testing.assert_allclose(cons["importance"].values, [full["total_u"][pairs.index((f, loy))] for f in ante], rtol=0, atol=1e-12)
    np.testing.assert_allclose(cons["performance"].values, full["perf"][ante], rtol=0, atol=1e-10)
    np.testing.assert_allclose(perf["performance"].values, full["perf"], rtol=0, atol=1e-10)
    np.testing.assert_allclose(perf["sd"].values, full["sd"], rtol=0, atol=1e-10)
    np.testing.assert_allclose(wts["weight"].values, full["weight_r"], rtol=0, atol=1e-12)
    assert list(wts.index) == list(cm.dev_mvs) and list(perf.index) == lvs and np.all(wts["weight"].values >= 0) and np.all((perf["performance"] >= 0) & (perf["performance"] <= 100))
    keep = np.flatnonzero(np.isin(np.repeat(np.arange(L), np.diff(cm.block_offset)), ante))
    assert list(ind.index) == [cm.dev_mvs[p] for p in keep] and list(ind.columns) == ["block", "importance", "performance"]
    np.testing.assert_allclose(ind["importance"].values, full["mvimp"][0][keep], rtol=0, atol=1e-12)
    np.testing.assert_allclose(ind["performance"].values, full["mvperf"][keep], rtol=0, atol=1e-10)
    te, pc = ip.total_effects(), ip.path_coefficients()
    np.testing.assert_allclose(te["total"].values, full["total_u"], rtol=0, atol=1e-12)
    direct = [e for e, (f, t) in enumerate(pairs) if np.asarray(cm.path)[t, f]]
    assert list(pc.index) == ["%s -> %s" % (lvs[pairs[e][0]], lvs[pairs[e][1]]) for e in direct]
    np.testing.assert_allclose(pc["direct"].values, full["direct_u"][direct], rtol=0, atol=1e-12)
    # the records
    rows, status, _ = native.fetch(0, B)
    recs, st = native.ipma_fetch(0, B)
    assert np.all(status == 0) and ip.records().shape == (ip.used(), native.ipma_width)
    model = orc.Model(blocks, np.asarray(cm.path), "A" * L, "path", True)
    pick = np.arange(0, B, 23)
    idx = np.stack([_native.bootstrap_indices(seed, int(r), Xd.shape[0]) for r in pick])
    check_against_mirror(recs[pick], st[pick], rows[pick], Xd, model, idx, pairs, lo, hi, "satisfaction", targets=[loy])
    # scores(): the rescaled scores are X~ weight_r, computed from the raw frame
    Y = np.column_stack([(100.0 * (Xd[:, b] - lo[b]) / (hi[b] - lo[b])) @ wts["weight"].values[b] for b in blocks])
    scores = ip.scores()
    assert list(scores.columns) == lvs and scores.shape == (Xd.shape[0], L)
    full64, fullld = mirror_pair(Xd, model, full_record(native), pairs, lo, hi, [loy])
    bar = field_bars(full64, fullld)["perf"]                 # (a rescaled score lives on the 0-100 scale of perf: the bar of that field on the full sample)
    print("scores: max |scores() - X~ weight_r| %.3e, max |column mean - perf| %.3e (bar %.3e)"
          % (np.max(np.abs(scores.values - Y)), np.max(np.abs(scores.values.mean(axis=0) - perf["performance"].values)), bar))
    np.testing.assert_allclose(scores.values, Y, rtol=0, atol=bar)
    np.testing.assert_allclose(scores.values.mean(axis=0), perf["performance"].values, rtol=0, atol=bar)
    # summary and intervals
    s = ip.summary("performance")
    assert list(s.columns) == SUMMARY_COLUMNS and list(s.index) == lvs and np.array_equal(s["original"].values, perf["performance"].values)
    imp = ip.summary("importance", "LOY")
    assert list(imp.index) == list(cm.dev_mvs) and np.array_equal(imp["original"].values, full_importance(ip))
    iv = ip.intervals("total")
    assert list(iv.columns) == INTERVAL_COLUMNS and np.all(iv["lower"].values <= iv["upper"].values)
    assert np.array_equal(ip.intervals("total", "percentile", 0.95)["lower"].values, ip.summary("total")["perc.025"].values)
    with pytest.raises(NotImplementedError):
        ip.intervals("total", "bca")
    with pytest.raises(ValueError):
        ip.summary("nothing")
    with pytest.raises(ValueError):
        ip.constructs("SAT")                                 # not a target of this map
    with pytest.raises(Exception, match="ipma"):
        Plspm(sat, cfg, Scheme.PATH).ipma()
    # every target, observed bounds
    every = Ipma(sat, cfg, Scheme.PATH, iterations=100, seed=seed)
    assert [lvs[t] for t in every._targets] == lvs[1:] and list(every.constructs("SAT").index) == ["IMAG", "EXPE", "QUAL", "VAL"]
    with pytest.raises(ValueError, match="name the target"):
        every.indicators()


def test_an_inadmissible_full_sample_is_refused_by_name():
    """A Mode-B block with a suppressor: b2 shares b1's noise and nothing else, so its regression weight is negative (the mirror on the oracle's fit, checked
    on the CPU: weight_r of b2 is -1.37 beside 1.78 and 0.59).  Ipma refuses before any replicate runs; Plspm(ipma=True) refuses as well."""
    import plspm.config as c
    from plspm.ipma import Ipma
    from plspm.mode import Mode
    from plspm.plspm import Plspm
    from plspm.scheme import Scheme
    n = 300
    rng = np.random.default_rng(11)
    f = rng.standard_normal(n)
    g = 0.7 * f + 0.7 * rng.standard_normal(n)
    A = f[:, None] * np.array([0.8, 0.7, 0.9]) + 0.5 * rng.standard_normal((n, 3))
    e = rng.standard_normal(n)
    b1 = g + 0.8 * e; b2 = e + 0.3 * rng.standard_normal(n); b3 = g + 0.6 * rng.standard_normal(n)
    frame = pd.DataFrame(np.column_stack((A, b1, b2, b3)), columns=["a1", "a2", "a3", "b1", "b2", "b3"])
    path = pd.DataFrame([[0, 0], [1, 0]], index=["A", "B"], columns=["A", "B"])
    cfg = c.Config(path, scaled=True)
    cfg.add_lv("A", Mode.A, c.MV("a1"), c.MV("a2"), c.MV("a3"))
    cfg.add_lv("B", Mode.B, c.MV("b1"), c.MV("b2"), c.MV("b3"))
    # the mirror on the oracle's fit says so without the device
    model = orc.Model([np.arange(3), np.arange(3, 6)], tri(2), "AB", "centroid", True)
    X = frame.values
    from helpers_ipma import oracle_record
    rec, pairs = oracle_record(X, model)
    m = _ipma(X, dev_blocks(model), rec, pairs, X.min(axis=0), X.max(axis=0))
    assert m["status"] == 4 and np.flatnonzero(m["weight_r"] < 0).tolist() == [4] and m["weight_r"][4] < -1.0
    with pytest.raises(ValueError, match=r"inadmissible.*negative rescaled weights in B \(b2\)$"):
        Ipma(frame, cfg, Scheme.CENTROID, iterations=100, seed=1)
    with pytest.raises(ValueError, match=r"inadmissible.*negative rescaled weights in B \(b2\)$"):
        Plspm(frame, cfg, Scheme.CENTROID, bootstrap=True, bootstrap_iterations=100, seed=1, ipma=True)


def full_importance(ip):
    return ip._original[ip._at["mvimp"]][:ip._cm.P]
