"""GPU: moderation analysis of bootstrap replicates by the two-stage approach (include/plspm_hip.h plspm_moderation_*; csrc/kernels_moderation.h,
csrc/moderation_core.h; plspm.moderation).

Kernel against the mirror.  Per replicate, the device's moderation record against the fp64 mirror (plspm.moderation._moderation, at the level of the data:
the rows weighted by the replicate's multiplicities) fed the device's own record weights, loadings, direct and r2 entries of that replicate.  The bar is the
project's rule for derived records: ten times the largest difference, on those same inputs, between the fp64 mirror and the same mirror in np.longdouble,
never below 1e-12.  That difference measured on the CPU with the oracle's records in place of the device's (tools/moderation_floor.py), per case over nine
resamples and all rows:

    one_term 1.2e-16   single_items 2.6e-16   mode_b 2.9e-16   satisfaction 5.2e-16   eight_terms 2.2e-16   fan_in_10 1.9e-16   wide_table 2.1e-16
    n63 1.9e-16   n64 1.6e-16   n65 2.7e-16   n1100 1.1e-16

so the floor 1e-12 is the bar everywhere (no case comes near 1e-13: the row sums' N 2^-53 is far below it at these sizes); every data set of every case has
status 0, finite values and passes every pivot test by the mirror alone on the oracle's records, and the test asserts the same on the device's.  The shapes
are the smallest at which a path changes: 70 rows of nine items, ragged against every row block; single-item blocks, the moderator included; a Mode-B
moderator; 400 x 60 with two terms on one target (a cross sum) and a third on another; eight terms on one target (92 sums: the 128-accumulator row pass);
ten regressors (the scratch route of the regression); 300 coefficients (table and values exceed the LDS together: the lanes read the table from memory);
63, 64, 65 and 1,100 rows (part of a wave's first 64 rows, exactly them, one more, and five row blocks with a ragged last one).  B = 9 on explicit
indices; B = 65 for two lane groups, the second with one live lane.

End to end against the project's own estimator: the full sample's scores(), their products formed on the host, and the stage-2 model fitted as a plain Plspm
of single-item LVs.  The two can only agree as far as the stage-1 record is determined: perturbing the oracle's full-sample record of the satisfaction case
inside the record bar (rtol 1e-8, atol 1e-11, 20 uniform draws; helpers_moderation.perturbation_figure) moves a moderated coefficient by 3.54e-9 at most,
measured on the CPU (tools/moderation_floor.py --oracle); the bar is ten times that."""
import numpy as np
import pandas as pd
import pytest

import plspm_oracle as orc
from helpers_moderation import CASES, FLOOR, case, counts_of, fan_in, mirror_bar, mirror_pair, native_model, philox_draws, planted, record_parts, resamples
from plspm.plsc import _effect_pairs

pytestmark = pytest.mark.gpu
E_ARG, E_STATE, E_LIMIT = 100, 101, 102
ORACLE_PERTURBED = 3.542e-9        # measured on the CPU (module docstring)
ORACLE_BAR = 10 * ORACLE_PERTURBED


def layout(model, terms):
    pairs = _effect_pairs(model.C)
    paths = [(f, t) for f, t in pairs if model.C[t, f]]
    return pairs, paths, len(paths), len(terms)


def check_against_mirror(mrecs, rows, X, model, terms, count_rows, tag):
    """Every moderation record against the mirror on that replicate's rows and its own bootstrap record; returns the mirrors."""
    worst, mirrors = 0.0, []
    pairs, paths, n_dir, T = layout(model, terms)
    targets = {j for _, _, j in terms}
    for r in range(mrecs.shape[0]):
        m64, mld = mirror_pair(X, model, terms, count_rows[r], rows[r])
        assert m64["status"] == 0 and mld["status"] == 0 and m64["pivots_pass"], (tag, r, "the inputs must have status 0 and pass the pivot test")
        bar = mirror_bar(m64, mld)
        diff = float(np.max(np.abs(mrecs[r] - m64["record"])))
        print("%s replicate %d: max |device - mirror| %.3e (bar %.3e)" % (tag, r, diff, bar))
        worst = max(worst, diff)
        assert np.all(np.isfinite(mrecs[r])), (tag, r)
        assert diff <= bar, "%s replicate %d: max |device - mirror| %.3e above the bar %.3e" % (tag, r, diff, bar)
        # identities: the slopes; a target without terms keeps the bootstrap record's entries bit for bit
        inter, low, high = (mrecs[r, n_dir + k * T:n_dir + (k + 1) * T] for k in (0, 2, 3))
        assert float(np.max(np.abs((high - low) - 2 * inter))) <= FLOOR
        _, r2, direct, _ = record_parts(model, rows[r])
        for d, (f, t) in enumerate(paths):
            if t not in targets:
                assert mrecs[r, d] == direct[pairs.index((f, t))], (tag, r, d)
        for l in range(model.L):
            if l not in targets:
                assert mrecs[r, n_dir + 4 * T + l] == r2[l], (tag, r, l)
        mirrors.append(m64)
    print("%s: max |device - mirror| %.3e over %d replicates" % (tag, worst, mrecs.shape[0]))
    return mirrors


def full_record(fit):
    return np.concatenate((fit["weights"], fit["r2"], fit["total"], fit["direct"], fit["loadings"]))


@pytest.mark.parametrize("name", CASES)
def test_kernel_against_the_mirror(name):
    X, model, terms = case(name)
    n = X.shape[0]
    nm = native_model(model, X)
    nm.moderation_enable(terms)
    _, paths, n_dir, T = layout(model, terms)
    W = n_dir + 4 * T + model.L
    assert nm.moderation_width == W
    B = 9
    idx = resamples(X, B)
    rows, status, _ = nm.bootstrap(B, idx=idx)
    assert np.all(status == 0)
    mrecs, st = nm.moderation_fetch(0, B)
    assert mrecs.shape == (B, W) and np.all(st == 0)
    mirrors = check_against_mirror(mrecs, rows, X, model, terms, [counts_of(idx[r], n) for r in range(B)], name)
    assert mirrors[0]["paths"] == paths
    # the full-sample record: the same kernels on one problem with every multiplicity 1
    fit = nm.fit(want_scores=False)
    full, fst = nm.moderation_fit()
    assert fst == 0 and fit["status"] == 0
    check_against_mirror(full[None, :], full_record(fit)[None, :], X, model, terms, [None], name + " plspm_moderation_fit")
    # the bootstrap's own records are the ones of a handle without moderation, bit for bit
    plain = native_model(model, X)
    rows0, status0, iters0 = plain.bootstrap(B, idx=idx)
    assert np.array_equal(rows, rows0) and np.array_equal(status, status0)
    with pytest.raises(Exception, match=r"plspm_moderation_fetch failed \(%d\)" % E_STATE):
        plain.moderation_fetch(0, 1)


def test_two_lane_groups_the_second_with_one_live_lane():
    X, model, terms = case("one_term")
    n, B = X.shape[0], 65
    idx = resamples(X, B, seed=5)
    nm = native_model(model, X)
    nm.moderation_enable(terms)
    rows, status, _ = nm.bootstrap(B, idx=idx)
    mrecs, st = nm.moderation_fetch(0, B)
    assert np.array_equal(st, status)
    pick = np.array([r for r in (0, 1, 63, 64) if status[r] == 0])
    assert 64 in pick
    check_against_mirror(mrecs[pick], rows[pick], X, model, terms, [counts_of(idx[r], n) for r in pick], "B = 65")
    # records do not depend on B: the first nine of 65 are the nine of a call of their own
    small = native_model(model, X)
    small.moderation_enable(terms)
    small.bootstrap(9, idx=idx[:9])
    assert np.array_equal(small.moderation_fetch(0, 9)[0], mrecs[:9], equal_nan=True)


def test_other_records_are_unchanged_beside_it():
    X, model, terms = case("satisfaction")
    idx = resamples(X, 9)

    def run(moderated):
        nm = native_model(model, X)
        nm.assess_enable(True)
        nm.structural_enable(True)
        if moderated:
            nm.moderation_enable(terms)
        out = [nm.bootstrap(9, idx=idx), nm.assess_fetch(0, 9), nm.structural_fetch(0, 9)]
        return out, (nm.moderation_fetch(0, 9) if moderated else None)
    off, _ = run(False)
    on, mod = run(True)
    for a, b in zip(off, on):
        for x, y in zip(a, b):
            assert np.array_equal(x, y, equal_nan=True)
    assert np.all(mod[1] == 0) and np.all(np.isfinite(mod[0]))
    # switched off again: no records, and the handle says so
    nm = native_model(model, X)
    nm.moderation_enable(terms)
    nm.moderation_enable(None)
    nm.bootstrap(9, idx=idx)
    with pytest.raises(Exception, match=r"plspm_moderation_fetch failed \(%d\)" % E_STATE):
        nm.moderation_fetch(0, 1)


def small_case(n=320, seed=9):
    X, blocks = planted(n, fan_in(3), [4, 4, 4], [(0, 1, 2)], seed)
    return X, orc.Model(blocks, fan_in(3), "AAA", "centroid", True), [(0, 1, 2)]


def test_replicate_ids_and_philox_draws():
    X, model, terms = small_case()
    n, seed = X.shape[0], 41
    whole = native_model(model, X)
    whole.moderation_enable(terms)
    whole.bootstrap_device(12, seed, 0)
    whole.sync()
    all12, st12 = whole.moderation_fetch(0, 12)
    part = native_model(model, X)
    part.moderation_enable(terms)
    part.bootstrap_device(5, seed, 7)                          # the pass's first record is 0, its first replicate 7
    part.sync()
    five, st5 = part.moderation_fetch(0, 5)
    assert np.array_equal(five, all12[7:12], equal_nan=True) and np.array_equal(st5, st12[7:12])
    # the draws on the host: the mirror on the restated Philox draws of replicates 0, 7 and 11
    rows, status, _ = whole.bootstrap(12, seed=seed)
    again, _ = whole.moderation_fetch(0, 12)
    assert np.array_equal(again, all12, equal_nan=True)
    pick = np.array([r for r in (0, 7, 11) if status[r] == 0])
    assert pick.size
    check_against_mirror(all12[pick], rows[pick], X, model, terms, [counts_of(philox_draws(seed, int(r), n), n) for r in pick], "philox draws")


def test_passes_and_sub_batches():
    """B = 600 behind the test-only boot_pass option (three passes of 256, 256 and 88), and plspm_bootstrap() as sub-batches, against one batch: bit for bit."""
    from plspm import _native
    X, model, terms = small_case()
    B, seed = 600, 23
    one = native_model(model, X)
    one.moderation_enable(terms)
    one.bootstrap_device(B, seed, 0)
    one.sync()
    whole, st = one.moderation_fetch(0, B)
    assert one.get_option("last_boot_passes") == 1
    three = native_model(model, X, boot_pass=256)
    three.moderation_enable(terms)
    rows, status, _ = three.bootstrap(B, seed=seed)
    assert three.get_option("last_boot_passes") == 3
    passes, st3 = three.moderation_fetch(0, B)
    assert np.array_equal(whole, passes, equal_nan=True) and np.array_equal(st, st3) and np.array_equal(st3, status)
    B = 1537
    parts = _native.chunk_plan(B, one.row_stride * 8, 3, 60, 64)
    assert len(parts) == 3 and sum(parts) == B, parts
    sub = native_model(model, X, boot_chunks=3, boot_align=64)
    sub.moderation_enable(terms)
    rows, status, _ = sub.bootstrap(B, seed=7)
    chunked, st1 = sub.moderation_fetch(0, B)
    sub.bootstrap_device(B, 7, 0)
    sub.sync()
    batch, st2 = sub.moderation_fetch(0, B)
    assert np.array_equal(chunked, batch, equal_nan=True) and np.array_equal(st1, st2) and np.array_equal(st1, status)
    pick = np.array([0, parts[0], parts[0] + parts[1], B - 1])
    pick = pick[st1[pick] == 0]
    n = X.shape[0]
    check_against_mirror(chunked[pick], rows[pick], X, model, terms, [counts_of(philox_draws(7, int(r), n), n) for r in pick], "sub-batches")


def test_failed_replicates_keep_their_status_and_are_nan():
    """60 x 9 with a tight iteration cap, as tests/test_gpu_structural.py makes failed replicates: the cap fails some and not all."""
    X, blocks = planted(60, fan_in(3), [3, 3, 3], [(0, 1, 2)], 12)
    model = orc.Model(blocks, fan_in(3), "AAA", "centroid", True)
    terms = [(0, 1, 2)]
    B = 24
    idx = resamples(X, B, seed=3)
    _, status, iters = native_model(model, X).bootstrap(B, idx=idx)
    assert np.all(status == 0) and iters.min() < iters.max()
    model.max_iter = int(iters.min())
    nm = native_model(model, X)
    nm.moderation_enable(terms)
    rows, status, _ = nm.bootstrap(B, idx=idx)
    failed = status != 0
    assert 0 < failed.sum() < B
    mrecs, st = nm.moderation_fetch(0, B)
    assert np.array_equal(st, status)
    assert np.all(np.isnan(mrecs[failed])) and np.all(np.isfinite(mrecs[~failed]))
    ok = np.flatnonzero(~failed)
    check_against_mirror(mrecs[ok], rows[ok], X, model, terms, [counts_of(idx[r], 60) for r in ok], "beside failed replicates")
    table, used = nm.moderation_summary(B, mrecs[ok[0]])
    assert used == B - failed.sum()
    np.testing.assert_allclose(table[:, 1], mrecs[ok].mean(axis=0), rtol=1e-12, atol=1e-15)


def test_state_and_argument_errors():
    from plspm import _native
    X, model, terms = small_case(seed=12)
    nm = native_model(model, X)
    with pytest.raises(_native.NativeBackendError, match=r"plspm_moderation_fetch failed \(%d\)" % E_STATE):
        nm.moderation_fetch(0, 1)                            # before any bootstrap
    with pytest.raises(_native.NativeBackendError, match=r"plspm_moderation_fit failed \(%d\)" % E_STATE):
        nm.moderation_fit()                                  # no terms yet
    for bad, word in (([(0, 0, 2)], "different"), ([(0, 1, 2), (1, 0, 2)], "same pair"), ([(2, 1, 0)], "add the path"), ([(0, 1, 7)], "out of range")):
        with pytest.raises(_native.NativeBackendError, match=r"plspm_moderation_enable failed \(%d\).*%s" % (E_ARG, word)):
            nm.moderation_enable(bad)
    nm.moderation_enable(terms)
    with pytest.raises(_native.NativeBackendError, match=r"plspm_moderation_summary failed \(%d\)" % E_STATE):
        nm.moderation_summary(100, np.zeros(nm.moderation_width))
    B = 200
    nm.bootstrap_device(B, 5, 0)
    mrecs, st = nm.moderation_fetch(0, B)
    original, ost = nm.moderation_fit()
    ok = mrecs[st == 0]
    assert ost == 0 and ok.shape[0] >= B - 5
    table, used = nm.moderation_summary(B, original)
    assert used == ok.shape[0] and np.array_equal(table[:, 0], original)
    with pytest.raises(_native.NativeBackendError, match=r"plspm_moderation_intervals failed \(%d\)" % E_ARG):
        nm.moderation_intervals(B, original, "bca", 0.95)    # method 3
    with pytest.raises(_native.NativeBackendError, match=r"plspm_moderation_summary failed \(%d\)" % E_ARG):
        nm.moderation_summary(B - 1, original)               # a wrong B
    with pytest.raises(_native.NativeBackendError, match=r"plspm_moderation_fetch failed \(%d\)" % E_ARG):
        nm.moderation_fetch(B - 1, 2)
    nm.jackknife(16)                                         # a jackknife leaves the records alone
    assert np.array_equal(nm.moderation_fetch(0, B)[0], mrecs, equal_nan=True)
    nm.upload(X, model.mv_order.astype(np.int32))            # an upload voids them
    with pytest.raises(_native.NativeBackendError, match=r"plspm_moderation_fetch failed \(%d\)" % E_STATE):
        nm.moderation_fetch(0, 1)
    nm.bootstrap_device(B, 5, 0)
    assert np.array_equal(nm.moderation_fetch(0, B)[0], mrecs, equal_nan=True)
    nm.permutation(8, X.shape[0] // 2, seed=3)               # a later call of another kind replaces them and writes none
    with pytest.raises(_native.NativeBackendError, match=r"plspm_moderation_fetch failed \(%d\)" % E_STATE):
        nm.moderation_fetch(0, 1)
    other = _native.NativeModel(np.array([0, 4, 8, 12], dtype=np.int32), fan_in(3).astype(np.uint8), np.zeros(3, dtype=np.int32), 0, True, 100, 1e-6, 0, nonmetric=True)
    with pytest.raises(_native.NativeBackendError, match=r"plspm_moderation_enable failed \(%d\).*plain metric models only" % E_ARG):
        other.moderation_enable(terms)
    # eight terms on a target of ten predecessors: 132 row sums, refused at enable, and nothing is launched afterwards
    rng = np.random.default_rng(2)
    Xw = rng.standard_normal((200, 11)) + 0.5 * rng.standard_normal((200, 1))
    wide = orc.Model([np.array([l]) for l in range(11)], fan_in(11), "A" * 11, "centroid", True)
    nw = native_model(wide, Xw)
    with pytest.raises(_native.NativeBackendError, match=r"plspm_moderation_enable failed \(%d\).*128 row sums" % E_LIMIT):
        nw.moderation_enable([(a, b, 10) for a in range(5) for b in range(a + 1, 5)][:8])
    nw.bootstrap_device(16, 5, 0)
    nw.sync()
    with pytest.raises(_native.NativeBackendError, match=r"plspm_moderation_fetch failed \(%d\)" % E_STATE):
        nw.moderation_fetch(0, 1)


# ------------------------------------------------------------------ the host package
SAT_NAMES = [("IMAG", "EXPE", "SAT"), ("QUAL", "VAL", "SAT"), ("IMAG", "SAT", "LOY")]


def planted_frame():
    import plspm.config as c
    from plspm.mode import Mode
    X, model, _ = case("satisfaction")
    cols = ["%s%d" % (lv, k + 1) for lv in orc.SAT_LVS for k in range(10)]
    frame = pd.DataFrame(X, columns=cols)
    s = c.Structure()
    s.add_path(["IMAG"], ["EXPE", "SAT", "LOY"]); s.add_path(["EXPE"], ["QUAL", "VAL", "SAT"])
    s.add_path(["QUAL"], ["VAL", "SAT"]); s.add_path(["VAL"], ["SAT"]); s.add_path(["SAT"], ["LOY"])
    cfg = c.Config(s.path(), scaled=True)
    for lv in orc.SAT_LVS:
        cfg.add_lv_with_columns_named(lv, Mode.A, frame, lv)
    return frame, cfg


def test_moderation_frames_and_plspm_wiring():
    from plspm.bootstrap import INTERVAL_COLUMNS, SUMMARY_COLUMNS
    from plspm.moderation import Moderation
    from plspm.plspm import Plspm
    from plspm.scheme import Scheme
    frame, cfg = planted_frame()
    m = Moderation(frame, cfg, Scheme.PATH, interactions=SAT_NAMES, iterations=200, seed=3)
    plain = Plspm(frame, cfg, Scheme.PATH, bootstrap=True, bootstrap_iterations=200, seed=3, interactions=SAT_NAMES, structural=True, quality=True, consistent=True)
    via = plain.moderation()
    for name in ("effects", "path_coefficients", "r_squared", "simple_slopes"):
        pd.testing.assert_frame_equal(getattr(m, name)(), getattr(via, name)())
    for what in ("direct", "interaction", "f2", "slope_low", "slope_high", "r2"):
        pd.testing.assert_frame_equal(m.summary(what), via.summary(what))      # same seed, same replicates
    assert plain.quality().used() == via.used() == plain.structural().used()
    assert m.used() >= 190 and m.seed() == 3 and m.status() == 0
    labels = ["IMAG x EXPE -> SAT", "QUAL x VAL -> SAT", "IMAG x SAT -> LOY"]
    paths = ["%s -> %s" % edge for edge in sorted(orc.SAT_EDGES, key=lambda e: (orc.SAT_LVS.index(e[0]), orc.SAT_LVS.index(e[1])))]
    eff = m.effects()
    assert list(eff.index) == labels and list(eff.columns) == ["predictor", "moderator", "target", "interaction", "f2", "slope.low", "slope.high"]
    assert list(eff["predictor"]) == ["IMAG", "QUAL", "IMAG"] and list(eff["target"]) == ["SAT", "SAT", "LOY"]
    assert np.all(eff["interaction"].values > 0.05) and np.all(eff["f2"].values > 0)      # the planted interactions
    pc = m.path_coefficients()
    assert list(pc.index) == paths and list(pc.columns) == ["main", "moderated"] and pc.shape == (10, 2)
    assert np.array_equal(pc.loc[["IMAG -> EXPE", "EXPE -> QUAL"], "main"].values, pc.loc[["IMAG -> EXPE", "EXPE -> QUAL"], "moderated"].values)      # targets without terms
    r2 = m.r_squared()
    assert list(r2.index) == orc.SAT_LVS and list(r2.columns) == ["main", "moderated"]
    assert np.all(r2.loc[["SAT", "LOY"], "moderated"].values > r2.loc[["SAT", "LOY"], "main"].values)
    ss = m.simple_slopes()
    assert list(ss.columns) == ["at -1", "at 0", "at 1"] and list(ss.index) == labels
    np.testing.assert_allclose(ss["at -1"].values, eff["slope.low"].values, rtol=0, atol=FLOOR)
    np.testing.assert_allclose(ss["at 1"].values, eff["slope.high"].values, rtol=0, atol=FLOOR)
    assert ss.loc["IMAG x EXPE -> SAT", "at 0"] == pc.loc["IMAG -> SAT", "moderated"]
    for what, index in (("direct", paths), ("interaction", labels), ("f2", labels), ("slope_low", labels), ("slope_high", labels), ("r2", orc.SAT_LVS)):
        table = m.summary(what)
        assert list(table.columns) == SUMMARY_COLUMNS and list(table.index) == index
        pct = m.intervals(what, "percentile", 0.95)
        assert list(pct.columns) == INTERVAL_COLUMNS and list(pct.index) == index
        assert np.array_equal(pct["lower"].values, table["perc.025"].values, equal_nan=True) and np.array_equal(pct["upper"].values, table["perc.975"].values, equal_nan=True)
    assert np.array_equal(m.summary("interaction")["original"].values, eff["interaction"].values)
    assert m.replicates().shape == (m.used(), 10 + 12 + 6) and np.all(np.isfinite(m.replicates()))
    with pytest.raises(NotImplementedError):
        m.intervals("f2", "bca")
    with pytest.raises(ValueError):
        m.summary("vif")
    with pytest.raises(ValueError, match="add the path"):
        Moderation(frame, cfg, Scheme.PATH, interactions=[("QUAL", "IMAG", "LOY")], iterations=100)
    with pytest.raises(Exception, match="moderation"):
        Plspm(frame, cfg, Scheme.PATH).moderation()


def test_end_to_end_against_a_stage_two_plspm_fit():
    """The full sample's scores(), the products formed on the host, and stage 2 as a plain Plspm of single-item LVs -- one per LV, one per term, term -> target."""
    import plspm.config as c
    from plspm.mode import Mode
    from plspm.moderation import Moderation
    from plspm.plspm import Plspm
    from plspm.scheme import Scheme
    frame, cfg = planted_frame()
    m = Moderation(frame, cfg, Scheme.PATH, interactions=SAT_NAMES, iterations=100, seed=1)
    scores = Plspm(frame, cfg, Scheme.PATH).scores()
    stage2 = pd.DataFrame({"s_" + lv: scores[lv].values for lv in orc.SAT_LVS})
    term_lv = ["T%d" % t for t in range(3)]
    for name, (a, b, _) in zip(term_lv, SAT_NAMES):
        stage2["t_" + name] = scores[a].values * scores[b].values
    s = c.Structure()
    s.add_path(["IMAG"], ["EXPE", "SAT", "LOY"]); s.add_path(["EXPE"], ["QUAL", "VAL", "SAT"])
    s.add_path(["QUAL"], ["VAL", "SAT"]); s.add_path(["VAL"], ["SAT"]); s.add_path(["SAT"], ["LOY"])
    for name, (_, _, j) in zip(term_lv, SAT_NAMES):
        s.add_path([name], [j])
    cfg2 = c.Config(s.path(), scaled=True)
    for lv in orc.SAT_LVS:
        cfg2.add_lv_with_columns_named(lv, Mode.A, stage2, "s_" + lv)
    for name in term_lv:
        cfg2.add_lv_with_columns_named(name, Mode.A, stage2, "t_" + name)
    coef = Plspm(stage2, cfg2, Scheme.PATH).path_coefficients()
    pc, eff = m.path_coefficients(), m.effects()
    worst = 0.0
    for label, row in pc.iterrows():
        f, t = label.split(" -> ")
        worst = max(worst, abs(row["moderated"] - coef.loc[t, f]))
    for name, (label, row) in zip(term_lv, eff.iterrows()):
        worst = max(worst, abs(row["interaction"] - coef.loc[row["target"], name]))
    print("moderated coefficients against the stage-2 Plspm fit: max |difference| %.3e (bar %.3e)" % (worst, ORACLE_BAR))
    assert worst <= ORACLE_BAR


def test_refusals_for_other_handle_kinds():
    import plspm.config as c
    from helpers import SAT_ADD_ORDER, SAT_PREFIX, satisfaction_frame
    from plspm.mode import Mode
    from plspm.moderation import Moderation
    from plspm.scale import Scale
    from plspm.scheme import Scheme
    sat = satisfaction_frame()

    def config(**kw):
        s = c.Structure()
        s.add_path(["IMAG"], ["EXPE", "SAT", "LOY"]); s.add_path(["EXPE"], ["QUAL", "VAL", "SAT"])
        s.add_path(["QUAL"], ["VAL", "SAT"]); s.add_path(["VAL"], ["SAT"]); s.add_path(["SAT"], ["LOY"])
        cfg = c.Config(s.path(), **kw)
        for lv in SAT_ADD_ORDER:
            cfg.add_lv_with_columns_named(lv, Mode.A, sat, SAT_PREFIX[lv])
        return cfg
    with pytest.raises(NotImplementedError, match="non-metric"):
        Moderation(sat, config(default_scale=Scale.NUM), Scheme.PATH, interactions=SAT_NAMES[:1], iterations=100)
    cfg = config(scaled=True)
    holes = sat.copy()
    holes.iloc[3, holes.columns.get_loc(cfg.filter(sat).columns[0])] = np.nan
    with pytest.raises(NotImplementedError, match="missing"):
        Moderation(holes, cfg, Scheme.PATH, interactions=SAT_NAMES[:1], iterations=100)
    with pytest.raises(NotImplementedError, match="one GPU"):
        Moderation(sat, cfg, Scheme.PATH, interactions=SAT_NAMES[:1], iterations=100, processes=2)
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    mobi = pd.read_csv(os.path.join(root, "tests", "golden", "ref_data", "mobi.csv"), index_col=0).astype(float)
    structure = c.Structure()
    structure.add_path(["Expectation", "Quality"], ["Satisfaction"])
    structure.add_path(["Satisfaction"], ["Complaints", "Loyalty"])
    hoc = c.Config(structure.path())
    hoc.add_higher_order("Satisfaction", Mode.A, ["Image", "Value"])
    for lv, prefix in (("Expectation", "CUEX"), ("Quality", "PERQ"), ("Loyalty", "CUSL"), ("Image", "IMAG"), ("Complaints", "CUSCO"), ("Value", "PERV")):
        hoc.add_lv_with_columns_named(lv, Mode.A, mobi, prefix)
    with pytest.raises(NotImplementedError, match="higher-order"):
        Moderation(mobi, hoc, Scheme.PATH, interactions=[("Expectation", "Quality", "Satisfaction")], iterations=100)
