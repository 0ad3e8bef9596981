"""GPU: consistent PLS of bootstrap replicates (include/plspm_hip.h plspm_plsc_*; csrc/kernels_plsc.h, csrc/plsc_core.h; plspm.plsc).

Kernel against the mirror.  Per replicate, the device's PLSc record against the fp64 mirror (plspm.plsc._plsc on NumPy's correlation matrix of the resampled
rows) fed the device's own record weights and loadings.  The bar is DESIGN.md 5m's: ten times the largest difference, on those same inputs, between the fp64
mirror and the same mirror in np.longdouble, with an absolute floor.  The floor is the largest such difference measured on the CPU with the oracle's weights and
loadings in place of the device's (tools/plsc_floor.py), never below 1e-12 -- the figures, per case over nine resamples and all rows:

    single_items 1.7e-16   wave_60x6 6.1e-16   quad_120x12 6.0e-16   lds_65_5 4.6e-16   packed_40 4.2e-16   fp64_gram 4.9e-16   mode_b 4.7e-16
    nine_predecessors 3.7e-15   lv_33 2.0e-15   mixed_mask 4.6e-16

so the floor is 1e-12 and is the bar everywhere.  The regressions amplify rounding by the conditioning of rc, which the two-mirror difference carries.  The
shapes are those at which the kernel takes another path: nothing to correct; one window of MVs in the dense layout; MVs on a second window; a block across the
64-lane boundary in the tile-packed layout; the packed layout with every dense solver off; the fp64 Gram; a Mode-B LV (uncorrected by default); nine
predecessors (the regression through the LDS scratch, not in registers); more LVs than half a wave; a mask that names two LVs as composites.  Every one of
the nine resamples of every case is admissible and every predecessor matrix passes the pivot test (asserted with the mirror)."""
import numpy as np
import pandas as pd
import pytest

import plspm_oracle as orc
from helpers import SAT_ADD_ORDER, SAT_PREFIX, satisfaction_frame
from helpers_plsc import ANY_DENSE, ANY_SOLVER, CASES, FLOOR, case, dev_blocks, mirror_bar, mirror_pair, native_model, negative_pair_model, resamples, tri

pytestmark = pytest.mark.gpu
E_ARG, E_STATE = 100, 101
INADMISSIBLE = 4


def check_against_mirror(recs, rows, X, model, idx, factor, tag):
    P, worst, bar = model.P, 0.0, np.inf
    for r in range(idx.shape[0]):
        m64, mld = mirror_pair(X[idx[r]][:, model.mv_order], model, rows[r, :P], rows[r, -P:], factor)
        assert m64["status"] == 0 and mld["status"] == 0 and m64["pivots_pass"], (tag, r, "the inputs must be admissible and pass the pivot test")
        this_bar = mirror_bar(m64, mld)
        diff = float(np.max(np.abs(recs[r] - m64["record"])))
        worst, bar = max(worst, diff), min(bar, this_bar)
        assert np.all(np.isfinite(recs[r])), (tag, r)
        assert diff <= this_bar, "%s replicate %d: max |device - mirror| %.3e above the bar %.3e" % (tag, r, diff, this_bar)
    print("%s: max |device - mirror| %.3e over %d replicates (smallest bar %.3e)" % (tag, worst, idx.shape[0], bar))


@pytest.mark.parametrize("name", CASES)
def test_kernel_against_the_mirror(name):
    X, model, options, solver, gram_path, factor = case(name)
    nm = native_model(model, X, **options)
    nm.plsc_enable(True, factor)
    L, P, R = model.L, model.P, nm.row_width
    W = R + L * (L - 1) // 2
    assert nm.plsc_width == W
    B = 9                                                    # two workgroups and one wave
    idx = resamples(X, B)
    rows, status, iters = nm.bootstrap(B, idx=idx)
    assert np.all(status == 0)
    assert nm.get_option("last_gram_path") == gram_path
    if solver is not ANY_SOLVER:
        assert (nm.get_option("last_solver") == solver) if solver is not ANY_DENSE else (nm.get_option("last_solver") != 1)
    recs, st = nm.plsc_fetch(0, B)
    assert recs.shape == (B, W) and np.all(st == 0)
    check_against_mirror(recs, rows, X, model, idx, factor, name)
    assert np.array_equal(recs[:, :P], rows[:, :P])          # the weights: copied
    mask = np.asarray(factor, dtype=bool) if factor is not None else np.array([m == "A" and len(b) >= 2 for m, b in zip(model.modes, model.blocks)])
    for l, blk in enumerate(dev_blocks(model)):
        if not mask[l]:
            assert np.array_equal(recs[:, R - P + blk], rows[:, R - P + blk])      # loadings of a composite: the record's
    if name == "single_items":                               # nothing to correct: the first R columns are the bootstrap's to the bar
        assert float(np.max(np.abs(recs[:, :R] - rows))) <= FLOOR
    if name == "mode_b":
        assert not mask[1] and mask[0] and mask[2]
    # the assessment records are there as well, whether or not plspm_assess_enable was called
    arec, ast = nm.assess_fetch(0, B)
    assert np.all(ast == 0) and np.all(np.isfinite(arec))
    # the full-sample record: the same two kernels on the moments of all rows and plspm_fit's solver problem
    fit = nm.fit(want_scores=False)
    full, fst = nm.plsc_fit()
    assert fst == 0 and fit["status"] == 0
    m64, mld = mirror_pair(X[:, model.mv_order], model, fit["weights"], fit["loadings"], factor)
    assert m64["status"] == 0 and m64["pivots_pass"]
    diff = float(np.max(np.abs(full - m64["record"])))
    print("%s: plspm_plsc_fit max |device - mirror| %.3e (bar %.3e)" % (name, diff, mirror_bar(m64, mld)))
    assert diff <= mirror_bar(m64, mld)


def test_all_zero_mask_is_the_bootstrap_record():
    """The kernel's construct correlations come from v'Rv, the solver's from its score covariance: the project's record bar (rtol 1e-8, atol 1e-11)."""
    X, model, options, _, _, _ = case("wave_60x6")
    nm = native_model(model, X, **options)
    nm.plsc_enable(True, np.zeros(model.L, dtype=np.uint8))
    B = 9
    rows, status, _ = nm.bootstrap(B, idx=resamples(X, B))
    recs, st = nm.plsc_fetch(0, B)
    assert np.all(status == 0) and np.all(st == 0)
    R = nm.row_width
    print("all-zero mask: max |PLSc - bootstrap| %.3e" % np.max(np.abs(recs[:, :R] - rows)))
    np.testing.assert_allclose(recs[:, :R], rows, rtol=1e-8, atol=1e-11)
    arec, _ = nm.assess_fetch(0, B)
    A, npairs = nm.assess_width, model.L * (model.L - 1) // 2
    assert np.array_equal(recs[:, R:], arec[:, A - npairs:])                        # uncorrected: lv_cor itself


def small_model(seed=9, n=320):
    X, blocks = orc.synth(n, tri(3), 4, seed=seed)
    return X, orc.Model(blocks, tri(3), "AAA", "centroid", True)


def test_inadmissible_replicates_have_status_4_and_are_not_used():
    from plspm.bootstrap import _create_summary
    X, model = negative_pair_model()
    assert -0.2 < np.corrcoef(X[:, 0], X[:, 1])[0, 1] < -0.05 and np.all(np.corrcoef(X, rowvar=False)[:2, 2:] > 0)
    nm = native_model(model, X)
    nm.plsc_enable(True)
    B, P = 24, model.P
    idx = resamples(X, B, seed=3)
    rows, status, _ = nm.bootstrap(B, idx=idx)
    assert np.all(status == 0)
    recs, st = nm.plsc_fetch(0, B)
    expect, negative = np.empty(B, dtype=np.int32), np.zeros(B, dtype=bool)
    for r in range(B):
        m64, _ = mirror_pair(X[idx[r]][:, model.mv_order], model, rows[r, :P], rows[r, -P:], None)
        expect[r], negative[r] = m64["status"], m64["quality"]["rho_a"][0] < 0
    bad = expect == INADMISSIBLE
    assert negative.sum() >= B // 2 and np.all(bad[negative]), "most resamples keep the negative item correlation, and a negative rho_A is inadmissible"
    assert np.array_equal(st, expect)
    assert np.all(np.isnan(recs[bad])) and np.all(np.isfinite(recs[~bad]))
    if (~bad).any():
        check_against_mirror(recs[~bad], rows[~bad], X, model, idx[~bad], None, "beside inadmissible replicates")
    original = np.where(np.isfinite(recs[~bad][0]), recs[~bad][0], 0.0) if (~bad).any() else np.zeros(nm.plsc_width)
    table, used = nm.plsc_summary(B, original)
    assert used == B - bad.sum()
    if used > 1:
        host = _create_summary(pd.DataFrame(recs[~bad]), pd.Series(original)).values
        np.testing.assert_allclose(table, host, rtol=1e-12, atol=1e-15)
    # the full sample: rho_A negative by the mirror, status 4 and NaN from plspm_plsc_fit
    fit = nm.fit(want_scores=False)
    m64, _ = mirror_pair(X[:, model.mv_order], model, fit["weights"], fit["loadings"], None)
    assert m64["quality"]["rho_a"][0] < 0
    full, fst = nm.plsc_fit()
    assert fst == INADMISSIBLE and np.all(np.isnan(full))
    # ... and admissible once that LV is declared a composite
    nm.plsc_enable(True, [0, 1])
    full, fst = nm.plsc_fit()
    assert fst == 0 and np.all(np.isfinite(full))


def test_failed_replicates_keep_their_status_and_are_nan():
    """Replicates that stop at max_iter, as tests/test_gpu_quality.py test_failed_replicates_are_nan_and_not_used makes them."""
    X, model = small_model()
    B = 24
    idx = resamples(X, B, seed=3)
    _, status, iters = native_model(model, X).bootstrap(B, idx=idx)
    assert np.all(status == 0) and iters.min() < iters.max()
    cut = int(iters.min())
    model.max_iter = cut
    nm = native_model(model, X)
    nm.plsc_enable(True)
    rows, status, _ = nm.bootstrap(B, idx=idx)
    failed = status != 0
    assert 0 < failed.sum() < B
    recs, st = nm.plsc_fetch(0, B)
    assert np.array_equal(st, status)
    assert np.all(np.isnan(recs[failed])) and np.all(np.isfinite(recs[~failed]))
    check_against_mirror(recs[~failed], rows[~failed], X, model, idx[~failed], None, "beside failed replicates")
    _, used = nm.plsc_summary(B, recs[~failed][0])
    assert used == B - failed.sum()


def test_sub_batches_passes_and_bit_identity():
    """plspm_bootstrap() as three sub-batches against one plspm_bootstrap_device batch, bit for bit on the PLSc records; the bootstrap's records, status and
    iteration counts, and the assessment records, bit-identical with PLSc on and off.  (The planner makes no part shorter than 512 replicates: 1,537 of this
    12-MV model, a few milliseconds.)"""
    from plspm import _native
    X, model = small_model()
    B, seed = 1537, 7
    plain = native_model(model, X, boot_chunks=3, boot_align=64)
    plain.assess_enable(True)
    rows0, status0, iters0 = plain.bootstrap(B, seed=seed)
    assess0, ast0 = plain.assess_fetch(0, B)
    with pytest.raises(_native.NativeBackendError, match=r"plspm_plsc_fetch failed \(%d\)" % E_STATE):
        plain.plsc_fetch(0, 1)                               # PLSc off: nothing written
    nm = native_model(model, X, boot_chunks=3, boot_align=64)
    nm.plsc_enable(True)
    parts = _native.chunk_plan(B, nm.row_stride * 8, 3, 60, 64)
    assert len(parts) == 3 and sum(parts) == B, parts
    rows1, status1, iters1 = nm.bootstrap(B, seed=seed)
    chunked, st1 = nm.plsc_fetch(0, B)
    assess1, ast1 = nm.assess_fetch(0, B)
    assert np.array_equal(rows0, rows1) and np.array_equal(status0, status1) and np.array_equal(iters0, iters1)
    assert np.array_equal(assess0, assess1, equal_nan=True) and np.array_equal(ast0, ast1)
    nm.bootstrap_device(B, seed, 0)                          # one batch
    nm.sync()
    whole, st2 = nm.plsc_fetch(0, B)
    assert np.array_equal(chunked, whole, equal_nan=True) and np.array_equal(st1, st2)
    assert np.all(np.isfinite(whole[st2 == 0])) and np.all(np.isnan(whole[st2 != 0]))
    assert np.all((st2 == status1) | ((status1 == 0) & (st2 == INADMISSIBLE)))
    pick = np.array([0, parts[0], parts[0] + parts[1], B - 1])
    pick = pick[st2[pick] == 0]
    idx = np.stack([_native.bootstrap_indices(seed, int(r), X.shape[0]) for r in pick])
    check_against_mirror(chunked[pick], rows1[pick], X, model, idx, None, "sub-batches")
    tail, _ = nm.plsc_fetch(B - 2, 2)
    assert np.array_equal(tail, whole[B - 2:], equal_nan=True)


def test_a_second_pass_of_one_replicate():
    from plspm import _native
    X, model = small_model()
    nm = native_model(model, X, boot_pass=256)
    nm.plsc_enable(True)
    B, seed = 257, 41
    rows, status, _ = nm.bootstrap(B, seed=seed)
    assert nm.get_option("last_boot_passes") == 2
    recs, st = nm.plsc_fetch(0, B)
    assert np.all(status == 0)
    pick = np.array([0, 255, 256])
    assert np.all(st[pick] == 0)
    idx = np.stack([_native.bootstrap_indices(seed, int(r), X.shape[0]) for r in pick])
    check_against_mirror(recs[pick], rows[pick], X, model, idx, None, "second pass")


def test_summary_intervals_and_errors():
    from plspm import _native
    from plspm.bootstrap import _create_summary, _intervals
    X, model = small_model(seed=12)
    nm = native_model(model, X)
    with pytest.raises(_native.NativeBackendError, match=r"plspm_plsc_fetch failed \(%d\)" % E_STATE):
        nm.plsc_fetch(0, 1)                                  # before any run
    with pytest.raises(_native.NativeBackendError, match=r"plspm_plsc_summary failed \(%d\)" % E_STATE):
        nm.plsc_summary(100, np.zeros(nm.plsc_width))
    nm.plsc_enable(True)
    B = 200
    nm.bootstrap_device(B, 5, 0)
    recs, st = nm.plsc_fetch(0, B)
    original, ost = nm.plsc_fit()
    assert ost == 0
    ok = recs[st == 0]
    table, used = nm.plsc_summary(B, original)
    assert used == ok.shape[0] and used >= B - 5
    host = _create_summary(pd.DataFrame(ok), pd.Series(original)).values
    fin = np.isfinite(host)
    assert np.array_equal(np.isfinite(table), fin)
    np.testing.assert_allclose(table[fin], host[fin], rtol=1e-12, atol=1e-15)
    for method in ("percentile", "basic", "bc"):
        for level in (0.9, 0.95):
            out, used_i = nm.plsc_intervals(B, original, method, level)
            mirror = _intervals(ok, original, None, method, level)
            assert used_i == used and np.array_equal(np.isnan(out), np.isnan(mirror))
            np.testing.assert_allclose(out[:, :2], mirror[:, :2], rtol=1e-12, atol=1e-15, err_msg=method)
            np.testing.assert_allclose(out[:, 2:], mirror[:, 2:], rtol=1e-12, atol=1e-12, err_msg=method)      # (z0 and the levels: atol as tests/test_gpu_ci.py)
    with pytest.raises(_native.NativeBackendError, match=r"plspm_plsc_intervals failed \(%d\)" % E_ARG):
        nm.plsc_intervals(B, original, "bca", 0.95)
    with pytest.raises(_native.NativeBackendError, match=r"plspm_plsc_summary failed \(%d\)" % E_ARG):
        nm.plsc_summary(B - 1, original)
    with pytest.raises(_native.NativeBackendError, match=r"plspm_plsc_fetch failed \(%d\)" % E_ARG):
        nm.plsc_fetch(B - 1, 2)
    # a jackknife leaves the bootstrap's records alone, and with them the PLSc records
    nm.jackknife(16)
    again, _ = nm.plsc_fetch(0, B)
    assert np.array_equal(again, recs, equal_nan=True)
    # permutation and stratified calls replace the bootstrap's records and write no PLSc records
    member = (np.arange(X.shape[0]) % 2).astype(np.uint8)
    nm.permutation(8, X.shape[0] // 2, seed=3)
    with pytest.raises(_native.NativeBackendError, match=r"plspm_plsc_fetch failed \(%d\)" % E_STATE):
        nm.plsc_fetch(0, 1)
    nm.bootstrap_device(B, 5, 0)
    assert np.array_equal(nm.plsc_fetch(0, B)[0], recs, equal_nan=True)
    nm.stratified_bootstrap(8, member, seed=3)
    with pytest.raises(_native.NativeBackendError, match=r"plspm_plsc_fetch failed \(%d\)" % E_STATE):
        nm.plsc_fetch(0, 1)
    # an upload voids them too
    nm.bootstrap_device(B, 5, 0)
    nm.upload(X, model.mv_order.astype(np.int32))
    with pytest.raises(_native.NativeBackendError, match=r"plspm_plsc_fetch failed \(%d\)" % E_STATE):
        nm.plsc_fetch(0, 1)
    # off again: no records
    nm.plsc_enable(False)
    nm.bootstrap_device(B, 5, 0)
    with pytest.raises(_native.NativeBackendError, match=r"plspm_plsc_fetch failed \(%d\)" % E_STATE):
        nm.plsc_fetch(0, 1)
    # bad masks, and the handle kinds PLSc does not cover
    boff = np.array([0, 4, 8, 9], dtype=np.int32)
    odd = _native.NativeModel(boff, tri(3).astype(np.uint8), np.array([0, 1, 0], dtype=np.int32), 0, True, 100, 1e-6, 0)
    odd.plsc_enable(True)                                    # the default mask: LV 0 only
    odd.plsc_enable(True, [1, 0, 0])
    for bad_mask in ([1, 1, 0], [1, 0, 1], [2, 0, 0]):       # Mode B; a single item; not 0 / 1
        with pytest.raises(_native.NativeBackendError, match=r"plspm_plsc_enable failed \(%d\)" % E_ARG):
            odd.plsc_enable(True, bad_mask)
    other = _native.NativeModel(np.array([0, 4, 8, 12], dtype=np.int32), tri(3).astype(np.uint8), np.zeros(3, dtype=np.int32), 0, True, 100, 1e-6, 0, nonmetric=True)
    with pytest.raises(_native.NativeBackendError, match=r"plspm_plsc_enable failed \(%d\)" % E_ARG):
        other.plsc_enable(True)


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


def test_plsc_frames_on_satisfaction():
    from plspm._compile import compile_model
    from plspm.bootstrap import INTERVAL_COLUMNS, SUMMARY_COLUMNS
    from plspm.plsc import PLSc, _plsc
    from plspm.plspm import Plspm
    from plspm.scheme import Scheme
    sat, cfg = sat_config()
    lvs = orc.SAT_LVS
    p = PLSc(sat, cfg, Scheme.PATH, iterations=200, seed=3)
    plain = Plspm(sat, cfg, Scheme.PATH, bootstrap=True, bootstrap_iterations=200, seed=3, consistent=True)
    via = plain.plsc()
    full_names = ("path_coefficients", "r_squared", "effects", "loadings", "weights", "reliabilities", "lv_correlations")
    for name in full_names:
        a, b = getattr(p, name)(), getattr(via, name)()
        (pd.testing.assert_frame_equal if isinstance(a, pd.DataFrame) else pd.testing.assert_series_equal)(a, b)
    boot_names = ("weights", "r_squared", "total_effects", "paths", "loading", "lv_correlations")
    for name in boot_names:
        pd.testing.assert_frame_equal(getattr(p.bootstrap(), name)(), getattr(via.bootstrap(), name)())      # same seed, same replicates
    # (a few of the 200 resamples of these 250 rows are inadmissible -- 3 with this seed; they are counted, not used)
    assert p.used() == via.used() and p.inadmissible() == via.inadmissible() and p.used() + p.inadmissible() == 200 and p.used() >= 190 and p.seed() == 3
    assert p.status() == 0 and p.factors() == lvs
    # the full-sample frames are the mirror's on the fit's weights and loadings
    data = cfg.filter(sat)
    cm = compile_model(cfg, cfg.path(), list(data.columns))
    X = data.values[:, cm.col_index].astype(np.float64)
    blocks = [np.arange(cm.block_offset[l], cm.block_offset[l + 1]) for l in range(cm.L)]
    om = plain.outer_model()
    w, lam = om.loc[cm.dev_mvs, "weight"].values, om.loc[cm.dev_mvs, "loading"].values
    m = _plsc(np.corrcoef(X, rowvar=False), w, lam, blocks, "A" * cm.L, cm.path, None, sd=X.std(axis=0))
    assert m["status"] == 0 and m["pivots_pass"]
    tol = dict(rtol=0, atol=1e-11)
    np.testing.assert_allclose(p.path_coefficients().values, m["path"], **tol)
    np.testing.assert_allclose(p.r_squared().values, m["r2"], **tol)
    np.testing.assert_allclose(p.lv_correlations().values, m["lv_cor"], **tol)
    np.testing.assert_allclose(p.reliabilities().values, m["reliabilities"], **tol)
    np.testing.assert_allclose(p.loadings().loc[cm.dev_mvs].values, m["loadings"], **tol)
    np.testing.assert_allclose(p.weights().loc[cm.dev_mvs].values, w, **tol)
    eff = p.effects()
    assert list(eff.columns) == ["from", "to", "direct", "indirect", "total"]
    np.testing.assert_allclose(eff["total"].values, [m["total"][t, f] for f, t in m["pairs"]], **tol)
    np.testing.assert_allclose(eff["indirect"].values, [m["indirect"][t, f] for f, t in m["pairs"]], **tol)
    assert list(p.path_coefficients().index) == lvs and list(p.lv_correlations().columns) == lvs
    # Corrected against uncorrected loadings.  The formula gives lambda_c,p = sigma v_p sqrt(Q) / (v'v) and the fit's loading is lambda_p = sigma (R_ll v)_p, with
    # v' R_ll v = 1: |lambda_c,p| < |lambda_p| exactly where |v_p| sqrt(Q) < (v'v) |(R_ll v)_p| -- no direction is assumed, the inequality is checked item by item.
    corrected, fitted = p.loadings().loc[cm.dev_mvs].values, lam
    R = np.corrcoef(X, rowvar=False)
    for l, blk in enumerate(blocks):
        v = w[blk] * X.std(axis=0)[blk]
        v = v / np.sqrt(v @ R[np.ix_(blk, blk)] @ v)
        smaller = np.abs(v) * np.sqrt(m["reliabilities"][l]) < (v @ v) * np.abs(R[np.ix_(blk, blk)] @ v)
        assert np.array_equal(np.abs(corrected[blk]) < np.abs(fitted[blk]), smaller), lvs[l]
    # the attenuation is undone: every corrected construct correlation is larger in magnitude than the composites' (all Q < 1)
    assert np.all(p.reliabilities().values < 1.0) and np.all(p.reliabilities().values > 0.5)
    boot = p.bootstrap()
    pairs = ["%s <-> %s" % (lvs[i], lvs[j]) for i in range(6) for j in range(i + 1, 6)]
    for name in boot_names:
        frame = getattr(boot, name)()
        assert list(frame.columns) == SUMMARY_COLUMNS and np.all(np.isfinite(frame["mean"].values))
    assert list(boot.lv_correlations().index) == pairs
    assert np.array_equal(boot.lv_correlations()["original"].values, p.lv_correlations().values[np.triu_indices(6, 1)])
    assert list(boot.paths().index) == list(plain.bootstrap().paths().index)
    assert list(boot.loading().index) == list(plain.bootstrap().loading().index)
    iv = boot.intervals("bc", 0.9)
    for name in boot_names:
        frame = getattr(iv, name)()
        assert list(frame.columns) == INTERVAL_COLUMNS and list(frame.index) == list(getattr(boot, name)().index)
        assert np.all(frame["lower"].values <= frame["upper"].values)
    pct = boot.intervals("percentile", 0.95)
    assert np.array_equal(pct.paths()["lower"].values, boot.paths()["perc.025"].values)
    assert p.replicates().shape == (p.used(), via._native.plsc_width) and np.all(np.isfinite(p.replicates()))
    with pytest.raises(NotImplementedError):
        boot.intervals("bca")
    with pytest.raises(ValueError):
        boot.intervals("student")
    only = PLSc(sat, cfg, Scheme.PATH, iterations=100, seed=3, factors=["IMAG", "SAT"])
    assert only.factors() == ["IMAG", "SAT"] and np.all(only.reliabilities()[["EXPE", "QUAL", "VAL", "LOY"]].values == 1.0)
    with pytest.raises(Exception, match="consistent"):
        Plspm(sat, cfg, Scheme.PATH).plsc()
