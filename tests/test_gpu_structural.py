"""GPU: structural-model assessment of bootstrap replicates (include/plspm_hip.h plspm_structural_*; csrc/kernels_structural.h, csrc/structural_core.h;
plspm.structural).

Kernel against the mirror.  Per replicate, the device's structural record against the fp64 mirror (plspm.structural._structural) fed the device's own
assessment lv_cor and the device's own record direct values of that replicate.  The bar is the project's rule for every derived stage: ten times the largest
difference, on those same inputs, between the fp64 mirror and the same mirror in np.longdouble, never below 1e-12.  That difference measured on the CPU with
the oracle's records in place of the device's (tools/structural_floor.py), per case over nine resamples and all rows:

    single_items 1.0e-18   satisfaction 4.0e-16   fan_in_10 2.0e-16   fan_in_11 2.3e-16   fan_in_20 4.9e-16   tri_33 2.9e-17   dense_7 2.2e-15   mode_b 3.9e-17

so the floor is 1e-12 and is the bar everywhere; every data set of every case has status 0, finite values and passes every pivot test by the oracle alone.
The shapes are the smallest at which the kernel takes another path: no chain and an empty drop-one list (tri(2), single items); several predecessors and
pairs with several chains (the satisfaction model, 400 x 60); drop-one solves of eight, in registers (fan_in(10)), and of nine, through the LDS scratch
(fan_in(11)); 19 predecessors, whose 20 slots of 751 doubles do not fit beside four waves' slices, so that a wave has 6 slots and its indices go round four
times (fan_in(20)); 560 record values on 64 lanes and chains of up to 33 nodes (tri(33)); 99 chains, more than one round of lanes (a dense 7-LV DAG); a Mode-B
block in the outer model.  B = 9 replicates on explicit indices: two workgroups and one wave.

Against the ORACLE's fits of the same resamples -- f2, vif and the specific effects from the oracle's scores by numpy.linalg.lstsq with and without the
predictor -- the statistics can only agree as far as the records do (rtol 1e-8, atol 1e-11, the project's record bar): perturbing the oracle's nine
satisfaction records inside that bar (20 uniform draws each, helpers_structural.perturbation_figure) moves a statistic by 3.04e-9 at most, measured on the
CPU (tools/structural_floor.py --oracle); the bar is ten times that."""
import numpy as np
import pytest

import plspm_oracle as orc
from helpers import SAT_ADD_ORDER, SAT_PREFIX, satisfaction_frame
from helpers_structural import (CASES, FLOOR, case, dense, lstsq_statistics, mirror_bar, mirror_pair, native_model, oracle_fit_record, record_direct, resamples,
                                tri)
from plspm.plsc import _effect_pairs

pytestmark = pytest.mark.gpu
E_ARG, E_STATE, E_LIMIT = 100, 101, 102
ORACLE_PERTURBED = 3.04e-9         # measured on the CPU (module docstring)
ORACLE_BAR = 10 * ORACLE_PERTURBED


def npairs(model):
    return model.L * (model.L - 1) // 2


def check_against_mirror(srecs, arecs, rows, model, tag):
    """Every structural record against the mirror on that replicate's own assessment lv_cor and record direct values; returns the mirrors."""
    worst, bar, mirrors = 0.0, np.inf, []
    for r in range(srecs.shape[0]):
        m64, mld = mirror_pair(model, arecs[r, -npairs(model):], record_direct(model, rows[r]))
        assert m64["status"] == 0 and mld["status"] == 0 and m64["pivots_pass"], (tag, r, "the inputs must have status 0 and pass the pivot test")
        this_bar = mirror_bar(m64, mld)
        diff = float(np.max(np.abs(srecs[r] - m64["record"])))
        print("%s replicate %d: max |device - mirror| %.3e (bar %.3e)" % (tag, r, diff, this_bar))
        worst, bar = max(worst, diff), min(bar, this_bar)
        assert np.all(np.isfinite(srecs[r])), (tag, r)
        assert diff <= this_bar, "%s replicate %d: max |device - mirror| %.3e above the bar %.3e" % (tag, r, diff, this_bar)
        mirrors.append(m64)
    print("%s: max |device - mirror| %.3e over %d replicates (smallest bar %.3e)" % (tag, worst, srecs.shape[0], bar))
    return mirrors


def device_paths(nm):
    dir_from, dir_to, chain_off, chain_nodes = nm.structural_paths()
    return list(zip(dir_from.tolist(), dir_to.tolist())), [tuple(chain_nodes[chain_off[s]:chain_off[s + 1]].tolist()) for s in range(len(chain_off) - 1)]


@pytest.mark.parametrize("name", CASES)
def test_kernel_against_the_mirror(name):
    X, model = case(name)
    nm = native_model(model, X)
    nm.structural_enable(True)
    P, L, B = model.P, model.L, 9                            # two workgroups and one wave
    idx = resamples(X, B)
    rows, status, _ = nm.bootstrap(B, idx=idx)
    assert np.all(status == 0)
    srecs, st = nm.structural_fetch(0, B)
    arecs, ast = nm.assess_fetch(0, B)                       # the assessment records are there as well, whether or not plspm_assess_enable was called
    assert np.all(st == 0) and np.all(ast == 0) and np.all(np.isfinite(arecs))
    mirrors = check_against_mirror(srecs, arecs, rows, model, name)
    # the host's enumeration against the mirror's
    paths, chains = device_paths(nm)
    assert paths == mirrors[0]["paths"] and chains == mirrors[0]["chains"]
    n_dir, n_spec = len(paths), len(chains)
    assert nm.structural_width == 2 * n_dir + n_spec and srecs.shape == (B, 2 * n_dir + n_spec)
    # identity: per pair, the chain values sum to the record's total - direct
    pairs = _effect_pairs(model.C)
    ne = len(pairs)
    total, direct = rows[:, P + L:P + L + ne], rows[:, P + L + ne:P + L + 2 * ne]
    sums = np.zeros((B, ne))
    for s, chain in enumerate(chains):
        sums[:, pairs.index((chain[0], chain[-1]))] += srecs[:, 2 * n_dir + s]
    gap = float(np.max(np.abs(sums - (total - direct)))) if ne else 0.0
    print("%s: max |sum of chains - (total - direct)| %.3e" % (name, gap))
    assert gap <= FLOOR
    if name == "single_items":                               # no chain, an empty drop-one list
        assert n_spec == 0 and np.all(srecs[:, 1] == 1.0)
        r2 = rows[:, P + 1]
        assert float(np.max(np.abs(srecs[:, 0] - r2 / (1.0 - r2)))) <= FLOOR
    if name == "tri_33":
        assert srecs.shape[1] == 560 and max(len(ch) for ch in chains) == 33 and np.all(srecs[:, 32:64] == 1.0)
    if name == "dense_7":
        assert n_spec == 99
    # the full-sample record: the same two kernels on the moments of all rows and plspm_fit's solver problem
    fit = nm.fit(want_scores=False)
    full, fst = nm.structural_fit()
    afull, _ = nm.assess_fit()
    assert fst == 0 and fit["status"] == 0
    m64, mld = mirror_pair(model, afull[-npairs(model):], fit["direct"])
    assert m64["status"] == 0 and m64["pivots_pass"]
    diff = float(np.max(np.abs(full - m64["record"])))
    print("%s: plspm_structural_fit max |device - mirror| %.3e (bar %.3e)" % (name, diff, mirror_bar(m64, mld)))
    assert diff <= mirror_bar(m64, mld)


def test_against_least_squares_on_the_oracles_scores():
    X, model = case("satisfaction")
    nm = native_model(model, X)
    nm.structural_enable(True)
    B = 9
    idx = resamples(X, B)
    _, status, _ = nm.bootstrap(B, idx=idx)
    srecs, st = nm.structural_fetch(0, B)
    assert np.all(status == 0) and np.all(st == 0)
    worst = 0.0
    for r in range(B):
        f, _ = oracle_fit_record(X, model, idx[r], X.shape[0])
        worst = max(worst, float(np.max(np.abs(srecs[r] - lstsq_statistics(model, f["scores"], f["path_coef"])))))
    print("statistics against least squares on the oracle's scores: max |difference| %.3e (bar %.3e)" % (worst, ORACLE_BAR))
    assert worst <= ORACLE_BAR


def run_stages(X, model, idx, structural, deeper):
    """One bootstrap with the deeper stage `deeper` (0 none, 2 PLSc, 3 model fit, 4 geodesic) and the structural branch on or off: every record there is."""
    nm = native_model(model, X)
    nm.assess_enable(True)
    if deeper == 2:
        nm.plsc_enable(True)
    if deeper == 3:
        nm.modelfit_enable(True)
    if deeper == 4:
        nm.geodesic_enable(True)
    if structural:
        nm.structural_enable(True)
    B = idx.shape[0]
    out = {"rows": nm.bootstrap(B, idx=idx), "assess": nm.assess_fetch(0, B)}
    if deeper >= 2:
        out["plsc"] = nm.plsc_fetch(0, B)
    if deeper >= 3:
        out["modelfit"] = nm.modelfit_fetch(0, B)
    if deeper >= 4:
        out["geodesic"] = nm.geodesic_fetch(0, B)
    if structural:
        out["structural"] = nm.structural_fetch(0, B)
    else:
        with pytest.raises(Exception, match=r"plspm_structural_fetch failed \(%d\)" % E_STATE):
            nm.structural_fetch(0, 1)
    return out


def test_the_branch_changes_no_other_record_and_no_stage_changes_the_branch():
    X, model = case("satisfaction")
    idx = resamples(X, 9)
    first = None
    for deeper in (0, 2, 3, 4):
        off, on = run_stages(X, model, idx, False, deeper), run_stages(X, model, idx, True, deeper)
        for key, value in off.items():
            for a, b in zip(value, on[key]):
                assert np.array_equal(a, b, equal_nan=True), (deeper, key)
        if first is None:
            first = on["structural"]
        assert np.array_equal(first[0], on["structural"][0]) and np.array_equal(first[1], on["structural"][1]), deeper
    assert np.all(first[1] == 0) and np.all(np.isfinite(first[0]))


def small_model(seed=9, n=320):
    X, blocks = orc.synth(n, tri(3), 4, seed=seed)
    return X, orc.Model(blocks, tri(3), "AAA", "centroid", True)


def test_passes_and_positions():
    """A second pass of one replicate behind the test-only boot_pass option, and plspm_bootstrap() as three sub-batches, against one batch: bit for bit."""
    from plspm import _native
    X, model = small_model()
    one = native_model(model, X)
    one.structural_enable(True)
    B, seed = 257, 41
    one.bootstrap_device(B, seed, 0)
    one.sync()
    whole, st = one.structural_fetch(0, B)
    assert one.get_option("last_boot_passes") == 1
    two = native_model(model, X, boot_pass=256)
    two.structural_enable(True)
    rows, status, _ = two.bootstrap(B, seed=seed)
    assert two.get_option("last_boot_passes") == 2
    passes, st2 = two.structural_fetch(0, B)
    assert np.array_equal(whole, passes, equal_nan=True) and np.array_equal(st, st2) and np.array_equal(st2, status)
    arecs, _ = two.assess_fetch(0, B)
    pick = np.array([0, 255, 256])
    assert np.all(st2[pick] == 0)
    check_against_mirror(passes[pick], arecs[pick], rows[pick], model, "second pass")
    # host output: sub-batches write from their position in the call (the planner makes no part shorter than 512 replicates)
    B = 1537
    parts = _native.chunk_plan(B, one.row_stride * 8, 3, 60, 64)
    assert len(parts) == 3 and sum(parts) == B, parts
    sub = native_model(model, X, boot_chunks=3, boot_align=64)
    sub.structural_enable(True)
    rows, status, _ = sub.bootstrap(B, seed=7)
    chunked, st1 = sub.structural_fetch(0, B)
    arecs, _ = sub.assess_fetch(0, B)
    sub.bootstrap_device(B, 7, 0)
    sub.sync()
    batch, st2 = sub.structural_fetch(0, B)
    assert np.array_equal(chunked, batch, equal_nan=True) and np.array_equal(st1, st2) and np.array_equal(st1, status)
    pick = np.array([0, parts[0], parts[0] + parts[1], B - 1])
    pick = pick[st1[pick] == 0]
    check_against_mirror(chunked[pick], arecs[pick], rows[pick], model, "sub-batches")
    tail, _ = sub.structural_fetch(B - 2, 2)
    assert np.array_equal(tail, batch[B - 2:], equal_nan=True)


def test_failed_replicates_keep_their_status_and_are_nan():
    """Replicates that stop at an iteration limit, as tests/test_gpu_jackknife_shapes.py makes them: the limit fails some and not all."""
    X, model = small_model()
    B = 24
    idx = resamples(X, B, seed=3)
    _, status, iters = native_model(model, X).bootstrap(B, idx=idx)
    assert np.all(status == 0) and iters.min() < iters.max()
    model.max_iter = int(iters.min())
    nm = native_model(model, X)
    nm.structural_enable(True)
    rows, status, _ = nm.bootstrap(B, idx=idx)
    failed = status != 0
    assert 0 < failed.sum() < B
    srecs, st = nm.structural_fetch(0, B)
    arecs, _ = nm.assess_fetch(0, B)
    assert np.array_equal(st, status)
    assert np.all(np.isnan(srecs[failed])) and np.all(np.isfinite(srecs[~failed]))
    check_against_mirror(srecs[~failed], arecs[~failed], rows[~failed], model, "beside failed replicates")
    _, used = nm.structural_summary(B, srecs[~failed][0])
    assert used == B - failed.sum()


def test_state_and_argument_errors():
    from plspm import _native
    X, model = small_model(seed=12)
    nm = native_model(model, X)
    with pytest.raises(_native.NativeBackendError, match=r"plspm_structural_fetch failed \(%d\)" % E_STATE):
        nm.structural_fetch(0, 1)                            # before any bootstrap
    nm.structural_enable(True)
    with pytest.raises(_native.NativeBackendError, match=r"plspm_structural_summary failed \(%d\)" % E_STATE):
        nm.structural_summary(100, np.zeros(nm.structural_width))
    B = 200
    nm.bootstrap_device(B, 5, 0)
    srecs, st = nm.structural_fetch(0, B)
    original, ost = nm.structural_fit()
    ok = srecs[st == 0]
    assert ost == 0 and ok.shape[0] >= B - 5
    table, used = nm.structural_summary(B, original)
    assert used == ok.shape[0] and np.array_equal(table[:, 0], original)
    np.testing.assert_allclose(table[:, 1], ok.mean(axis=0), rtol=1e-12, atol=1e-15)
    with pytest.raises(_native.NativeBackendError, match=r"plspm_structural_intervals failed \(%d\)" % E_ARG):
        nm.structural_intervals(B, original, "bca", 0.95)    # method 3
    with pytest.raises(_native.NativeBackendError, match=r"plspm_structural_summary failed \(%d\)" % E_ARG):
        nm.structural_summary(B - 1, original)               # a wrong B
    with pytest.raises(_native.NativeBackendError, match=r"plspm_structural_fetch failed \(%d\)" % E_ARG):
        nm.structural_fetch(B - 1, 2)
    nm.jackknife(16)                                         # a jackknife leaves the records alone
    assert np.array_equal(nm.structural_fetch(0, B)[0], srecs, equal_nan=True)
    nm.upload(X, model.mv_order.astype(np.int32))            # an upload voids them
    with pytest.raises(_native.NativeBackendError, match=r"plspm_structural_fetch failed \(%d\)" % E_STATE):
        nm.structural_fetch(0, 1)
    nm.bootstrap_device(B, 5, 0)
    assert np.array_equal(nm.structural_fetch(0, B)[0], srecs, equal_nan=True)
    nm.permutation(8, X.shape[0] // 2, seed=3)               # a later call of another kind replaces them and writes none
    with pytest.raises(_native.NativeBackendError, match=r"plspm_structural_fetch failed \(%d\)" % E_STATE):
        nm.structural_fetch(0, 1)
    nm.structural_enable(False)                              # off again: no records
    nm.bootstrap_device(B, 5, 0)
    with pytest.raises(_native.NativeBackendError, match=r"plspm_structural_fetch failed \(%d\)" % E_STATE):
        nm.structural_fetch(0, 1)
    other = _native.NativeModel(np.array([0, 4, 8, 12], dtype=np.int32), tri(3).astype(np.uint8), np.zeros(3, dtype=np.int32), 0, True, 100, 1e-6, 0, nonmetric=True)
    with pytest.raises(_native.NativeBackendError, match=r"plspm_structural_enable failed \(%d\)" % E_ARG):
        other.structural_enable(True)
    # a dense 16-LV single-item model: refused at enable from the count, and nothing is launched afterwards
    rng = np.random.default_rng(2)
    Xw = rng.standard_normal((200, 16)) + rng.standard_normal((200, 1))
    wide = orc.Model([np.array([l]) for l in range(16)], dense(16), "A" * 16, "centroid", True)
    nw = native_model(wide, Xw)
    with pytest.raises(_native.NativeBackendError, match=r"plspm_structural_enable failed \(%d\).*65399" % E_LIMIT):
        nw.structural_enable(True)
    assert nw.structural_width == 0
    nw.bootstrap_device(16, 5, 0)
    nw.sync()
    with pytest.raises(_native.NativeBackendError, match=r"plspm_structural_fetch failed \(%d\)" % E_STATE):
        nw.structural_fetch(0, 1)
    with pytest.raises(_native.NativeBackendError, match=r"plspm_assess_fetch failed \(%d\)" % E_STATE):
        nw.assess_fetch(0, 1)                                # not even the assessment the branch would have needed


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


def test_structural_frames_on_satisfaction():
    import pandas as pd
    from plspm.bootstrap import INTERVAL_COLUMNS, SUMMARY_COLUMNS
    from plspm.plspm import Plspm
    from plspm.scheme import Scheme
    from plspm.structural import Structural
    sat, cfg = sat_config()
    s = Structural(sat, cfg, Scheme.PATH, iterations=200, seed=3)
    plain = Plspm(sat, cfg, Scheme.PATH, bootstrap=True, bootstrap_iterations=200, seed=3, structural=True, quality=True, consistent=True)
    via = plain.structural()
    for name in ("effect_sizes", "specific_effects", "mediation"):
        pd.testing.assert_frame_equal(getattr(s, name)(), getattr(via, name)())
    for what in ("f2", "vif", "specific"):
        pd.testing.assert_frame_equal(s.summary(what), via.summary(what))      # same seed, same replicates
    assert plain.quality().used() == via.used() and plain.plsc().used() + plain.plsc().inadmissible() == via.used()      # the other stages on the same handle
    assert s.used() == via.used() and s.used() >= 190 and s.seed() == 3 and s.status() == 0
    paths = ["%s -> %s" % edge for edge in sorted(orc.SAT_EDGES, key=lambda e: (orc.SAT_LVS.index(e[0]), orc.SAT_LVS.index(e[1])))]
    es = s.effect_sizes()
    assert list(es.index) == paths and list(es.columns) == ["f2", "vif"] and es.shape == (10, 2)
    assert np.all(es["f2"].values > -1e-12) and np.all(es["vif"].values > 1.0 - 1e-12) and es.loc["IMAG -> EXPE", "vif"] == 1.0
    sp = s.specific_effects()
    assert list(sp.columns) == ["from", "to", "through", "effect"] and sp.shape == (24, 4)
    assert sp.index[0] == "IMAG -> EXPE -> QUAL" and sp.loc["IMAG -> EXPE -> QUAL", "through"] == "EXPE"
    assert "IMAG -> EXPE -> QUAL -> VAL -> SAT -> LOY" in sp.index and sp.loc["IMAG -> EXPE -> QUAL -> VAL -> SAT -> LOY", "through"] == "EXPE -> QUAL -> VAL -> SAT"
    med = s.mediation()
    assert list(med.columns) == ["from", "to", "direct", "indirect", "total", "effect", "share"] and list(med.index) == list(sp.index)
    eff = plain.effects()
    for label, row in med.iterrows():
        pair = "%s -> %s" % (row["from"], row["to"])
        np.testing.assert_allclose([row["direct"], row["indirect"], row["total"]], eff.loc[pair, ["direct", "indirect", "total"]].values.astype(float), rtol=0, atol=1e-10)
    np.testing.assert_allclose(med.groupby(["from", "to"])["share"].sum().values, 1.0, rtol=1e-12)
    for what, index in (("f2", paths), ("vif", paths), ("specific", list(sp.index))):
        table = s.summary(what)
        assert list(table.columns) == SUMMARY_COLUMNS and list(table.index) == index and np.all(np.isfinite(table["mean"].values))
        pct = s.intervals(what, "percentile", 0.95)
        assert list(pct.columns) == INTERVAL_COLUMNS and list(pct.index) == index
        assert np.array_equal(pct["lower"].values, table["perc.025"].values) and np.array_equal(pct["upper"].values, table["perc.975"].values)
        bc = s.intervals(what, "bc", 0.9)
        constant = table["std.error"].values == 0.0          # (the vif of a path into an LV with one predecessor is 1.0 in every replicate: bc has no z0 there)
        assert np.array_equal(np.isnan(bc["lower"].values), constant) and np.all(bc["lower"].values[~constant] <= bc["upper"].values[~constant])
        assert constant.sum() == (2 if what == "vif" else 0)
    assert np.array_equal(s.summary("specific")["original"].values, sp["effect"].values)
    assert np.array_equal(s.summary("f2")["original"].values, es["f2"].values)
    assert s.replicates().shape == (s.used(), 44) and np.all(np.isfinite(s.replicates()))
    with pytest.raises(NotImplementedError):
        s.intervals("f2", "bca")
    with pytest.raises(ValueError):
        s.intervals("f2", "student")
    with pytest.raises(ValueError):
        s.summary("q2")
    with pytest.raises(Exception, match="structural"):
        Plspm(sat, cfg, Scheme.PATH).structural()
