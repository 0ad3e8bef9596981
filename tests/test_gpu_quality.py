"""GPU: the measurement-model assessment of bootstrap replicates (include/plspm_hip.h plspm_assess_*; csrc/kernels_assess.h; plspm.quality).

Kernel against the mirror.  The int8 moments are exact sums, so the device owes only the fp64 arithmetic of the formulas: per case the bar is ten times
the largest difference, on these same inputs (the resampled rows and the device's own record weights and loadings), between the fp64 mirror
(plspm.quality._quality on NumPy's correlation matrix) and the same mirror in np.longdouble, with a floor of 1e-12 absolute.  On the CPU, with the
oracle's weights and loadings in place of the device's, that difference is at most 7.5e-16 on seven of the cases below and 3.9e-14 on the 120-MV chain
(distant LVs: correlations near zero under HTMT2's logarithm), so the floor is the bar everywhere.  The shapes are those at which the
kernel takes another path: single-item blocks; one window (60 MVs, dense layout, wave solver); MVs on a second window (120 MVs, quad solver); a block across the 64-lane boundary in the tile-packed layout with an odd tile count (65 + 5 MVs, LDS
solver); the packed layout with every dense solver switched off (40 MVs: four tiles -- the odd tile count is the 70-MV case's); the fp64 Gram; a Mode-B
block; a reverse-coded item.

Against the ORACLE's fits of the same resamples the criteria can only agree as far as the records do (rtol 1e-8, atol 1e-11, the project's record bar):
perturbing the oracle's 20 satisfaction records inside that bar (20 uniform draws each, helpers_quality.perturbation_figure) moves a criterion by
1.37e-8 at most, measured on the CPU; the bar is ten times that."""
import numpy as np
import pandas as pd
import pytest

import plspm_oracle as orc
from helpers import SAT_ADD_ORDER, SAT_PREFIX, satisfaction_frame, satisfaction_oracle_inputs
from helpers_quality import mirror_bar, mirror_pair, oracle_records

pytestmark = pytest.mark.gpu
SCHEME_ID = {"centroid": 0, "factorial": 1, "path": 2}
ORACLE_PERTURBED = 1.37e-8         # measured on the CPU (module docstring)
ORACLE_BAR = 10 * ORACLE_PERTURBED
E_ARG, E_STATE = 100, 101


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


def case(name):
    """(X, model, handle options, expected last_solver (None: any dense one), expected last_gram_path)."""
    if name == "single_items":
        X, blocks = orc.synth(300, tri(2), 1, seed=1)
        return X, orc.Model(blocks, tri(2), "AA", "centroid", True), {}, None, 2
    if name == "wave_60x6":
        X, blocks = orc.synth(400, orc.satisfaction_C(), 10, seed=2)
        return X, orc.Model(blocks, orc.satisfaction_C(), "AAAAAA", "path", True), {}, 7, 2
    if name == "quad_120x12":
        X, blocks = orc.synth(400, orc.chain_C(12), 10, seed=3)
        return X, orc.Model(blocks, orc.chain_C(12), "A" * 12, "centroid", True), {}, 5, 2
    if name == "lds_65_5":
        X, _ = orc.synth(300, tri(2), 65, seed=4)
        X = np.ascontiguousarray(X[:, :70])
        return X, orc.Model([np.arange(65), np.arange(65, 70)], tri(2), "AA", "factorial", True), {}, 1, 2
    if name == "packed_40":
        X, blocks = orc.synth(300, tri(4), 10, seed=5)
        return X, orc.Model(blocks, tri(4), "AAAA", "path", False), dict(solver_wave=0, solver_rows=0, solver_quad=0), 1, 2
    if name == "fp64_gram":
        X, blocks = orc.synth(300, tri(3), 4, seed=6)
        return X, orc.Model(blocks, tri(3), "AAA", "centroid", True), dict(gram_path=1), 1, 1
    if name == "mode_b":
        X, blocks = orc.synth(300, tri(3), 4, seed=7)
        return X, orc.Model(blocks, tri(3), "ABA", "path", True), {}, None, 2
    if name == "reverse_coded":
        X, blocks = orc.synth(300, tri(3), 4, seed=8)
        X[:, 1] *= -1.0; X[:, 6] *= -1.0
        return X, orc.Model(blocks, tri(3), "AAA", "centroid", True), {}, None, 2
    raise KeyError(name)


CASES = ["single_items", "wave_60x6", "quad_120x12", "lds_65_5", "packed_40", "fp64_gram", "mode_b", "reverse_coded"]


def check_against_mirror(recs, rows, X, model, idx, tag):
    P, worst, bar = model.P, 0.0, np.inf
    for r in range(idx.shape[0]):
        m64, mld = mirror_pair(X[idx[r]][:, model.mv_order], model, rows[r, :P], rows[r, -P:])
        this_bar = mirror_bar(m64, mld)
        diff = float(np.max(np.abs(recs[r] - m64)))
        worst, bar = max(worst, diff), min(bar, this_bar)
        assert np.all(np.isfinite(recs[r])), (tag, r)
        assert diff <= this_bar, "%s replicate %d: max |device - mirror| %.3e above the bar %.3e" % (tag, r, diff, this_bar)
    print("%s: max |device - mirror| %.3e over %d replicates (smallest bar %.3e)" % (tag, worst, idx.shape[0], bar))


@pytest.mark.parametrize("name", CASES)
def test_kernel_against_the_mirror(name):
    X, model, options, solver, gram_path = case(name)
    nm = native_model(model, X, **options)
    nm.assess_enable(True)
    A = 4 * model.L + 3 * (model.L * (model.L - 1) // 2)
    assert nm.assess_width == A
    B = 9                                                    # two workgroups and one wave
    idx = np.random.default_rng(17).integers(0, X.shape[0], (B, X.shape[0])).astype(np.int32)
    rows, status, _ = nm.bootstrap(B, idx=idx)
    assert np.all(status == 0)
    assert nm.get_option("last_gram_path") == gram_path
    assert (nm.get_option("last_solver") == solver) if solver is not None else (nm.get_option("last_solver") != 1)
    recs, st = nm.assess_fetch(0, B)
    assert recs.shape == (B, A) and np.all(st == 0)
    check_against_mirror(recs, rows, X, model, idx, name)
    L = model.L
    if name == "single_items":
        assert np.all(recs[:, :4 * L] == 1.0)
    if name == "mode_b":
        assert np.all(recs[:, L + 1] == 1.0) and np.all(recs[:, L] != 1.0)
    if name == "reverse_coded":
        R = np.corrcoef(X[:, model.mv_order], rowvar=False)
        assert R[0, 1] < -0.2 and R[4, 6] < -0.2              # the absolute values matter
        assert np.all(recs[:, 4 * L:4 * L + 3] > 0.0)
    # the full-sample record: the same kernel on the moments of all rows and plspm_fit's solver problem
    fit = nm.fit(want_scores=False)
    full, fst = nm.assess_fit()
    assert fst == 0 and fit["status"] == 0
    m64, mld = mirror_pair(X[:, model.mv_order], model, fit["weights"], fit["loadings"])
    diff = float(np.max(np.abs(full - m64)))
    print("%s: plspm_assess_fit max |device - mirror| %.3e (bar %.3e)" % (name, diff, mirror_bar(m64, mld)))
    assert diff <= mirror_bar(m64, mld)


def test_against_the_oracles_fits_of_the_resamples():
    X, blocks, _ = satisfaction_oracle_inputs()
    model = orc.Model(blocks, orc.satisfaction_C(), "AAAAAA", "path", True)
    nm = native_model(model, X)
    nm.assess_enable(True)
    B, P = 20, model.P
    idx = np.random.default_rng(23).integers(0, X.shape[0], (B, X.shape[0])).astype(np.int32)
    rows, status, iters = nm.bootstrap(B, idx=idx)
    recs, _ = nm.assess_fetch(0, B)
    oracle, its = oracle_records(X, model, idx)
    assert np.all(status == 0) and np.array_equal(iters, its)
    worst = 0.0
    for r in range(B):
        m64, _ = mirror_pair(X[idx[r]][:, model.mv_order], model, oracle[r, :P], oracle[r, -P:])
        worst = max(worst, float(np.max(np.abs(recs[r] - m64))))
    print("criteria against the mirror on the oracle's fits: max |difference| %.3e (bar %.3e)" % (worst, ORACLE_BAR))
    assert worst <= ORACLE_BAR


def small_model(seed=9, n=320):
    X, blocks = orc.synth(n, tri(3), 4, seed=seed)
    return X, orc.Model(blocks, tri(3), "AAA", "centroid", True)


def test_a_second_pass_of_one_replicate():
    from plspm import _native
    X, model = small_model()
    nm = native_model(model, X, boot_pass=256)
    nm.assess_enable(True)
    B, seed = 257, 41
    rows, status, _ = nm.bootstrap(B, seed=seed)
    assert nm.get_option("last_boot_passes") == 2
    recs, st = nm.assess_fetch(0, B)
    assert np.array_equal(st, status) and np.all(status == 0) and np.all(np.isfinite(recs))
    pick = np.array([0, 255, 256])
    idx = np.stack([_native.bootstrap_indices(seed, int(r), X.shape[0]) for r in pick])
    check_against_mirror(recs[pick], rows[pick], X, model, idx, "second pass")
    # a range that starts behind the first pass
    tail, _ = nm.assess_fetch(255, 2)
    assert np.array_equal(tail, recs[255:])


def test_sub_batches_write_at_their_offset_and_leave_the_bootstrap_alone():
    """plspm_bootstrap() as three sub-batches against one plspm_bootstrap_device batch.  The planner makes no part shorter than 512 replicates, so three
    parts take 1,537 replicates of this 12-MV model (a few milliseconds): the one test above the 513 of the others."""
    from plspm import _native
    X, model = small_model()
    B, seed = 1537, 7
    plain = native_model(model, X, boot_chunks=3, boot_align=64)
    rows0, status0, iters0 = plain.bootstrap(B, seed=seed)
    with pytest.raises(_native.NativeBackendError, match=r"plspm_assess_fetch failed \(%d\)" % E_STATE):
        plain.assess_fetch(0, 1)                             # assessment off: nothing written
    nm = native_model(model, X, boot_chunks=3, boot_align=64)
    nm.assess_enable(True)
    parts = _native.chunk_plan(B, nm.row_stride * 8, 3, 60, 64)
    assert len(parts) == 3 and sum(parts) == B, parts
    rows1, status1, iters1 = nm.bootstrap(B, seed=seed)      # three sub-batches, each with its offset
    chunked, st1 = nm.assess_fetch(0, B)
    # the bootstrap's own records, status and iteration counts: bit-identical with assessment on and off
    assert np.array_equal(rows0, rows1) and np.array_equal(status0, status1) and np.array_equal(iters0, iters1)
    nm.bootstrap_device(B, seed, 0)                          # one batch
    nm.sync()
    whole, st2 = nm.assess_fetch(0, B)
    rows2, status2, _ = nm.fetch(0, B)
    assert np.array_equal(rows2, rows1)
    assert np.array_equal(chunked, whole, equal_nan=True) and np.array_equal(st1, st2) and np.array_equal(st1, status1)
    assert np.all(np.isfinite(whole[st2 == 0]))
    # the records of every sub-batch are their own replicates' (not the first part's again)
    pick = np.array([0, parts[0], parts[0] + parts[1], B - 1])
    idx = np.stack([_native.bootstrap_indices(seed, int(r), X.shape[0]) for r in pick])
    check_against_mirror(chunked[pick], rows1[pick], X, model, idx, "sub-batches")


def test_failed_replicates_are_nan_and_not_used():
    """A replicate whose status is not PLSPM_OK: NaN in all A values, left out of n_used.  (Replicates that stop at max_iter; a column that is constant in a
    resample does NOT fail a metric replicate -- next test.)"""
    from plspm.bootstrap import _create_summary
    X, model = small_model()
    B = 24
    idx = np.random.default_rng(3).integers(0, X.shape[0], (B, X.shape[0])).astype(np.int32)
    _, status, iters = native_model(model, X).bootstrap(B, idx=idx)
    assert np.all(status == 0) and iters.min() < iters.max()
    cut = int(iters.min())                                   # replicates that need more iterations than this do not converge below
    model.max_iter = cut
    nm = native_model(model, X)
    nm.assess_enable(True)
    rows, status, _ = nm.bootstrap(B, idx=idx)
    failed = status != 0
    assert 0 < failed.sum() < B and np.array_equal(failed, iters > cut)
    recs, st = nm.assess_fetch(0, B)
    assert np.array_equal(st, status)
    assert np.all(np.isnan(recs[failed])) and np.all(np.isfinite(recs[~failed]))
    check_against_mirror(recs[~failed], rows[~failed], X, model, idx[~failed], "beside failed replicates")
    original = recs[~failed][0]
    table, used = nm.assess_summary(B, original)
    assert used == B - failed.sum()
    host = _create_summary(pd.DataFrame(recs[~failed]), pd.Series(original)).values
    np.testing.assert_allclose(table, host, rtol=1e-12, atol=0)


def test_a_column_that_is_constant_in_a_resample():
    """The metric solver gives such an item weight and loading 0 and keeps status PLSPM_OK (csrc/solver_core.h treated_sd, as the reference counts the replicate);
    its standard deviation is zero, so the criteria that divide by it are inf or NaN by IEEE's rules, and the others are the mirror's."""
    X, model = small_model()
    X = X.copy()
    X[:6, 0] = 1.25                                          # six rows share one value in column 0
    nm = native_model(model, X)
    nm.assess_enable(True)
    B = 5
    idx = np.random.default_rng(3).integers(0, X.shape[0], (B, X.shape[0])).astype(np.int32)
    idx[2] = np.random.default_rng(4).integers(0, 6, X.shape[0])      # replicate 2 draws those rows only
    rows, status, _ = nm.bootstrap(B, idx=idx)
    assert np.all(status == 0) and rows[2, 0] == 0.0 and rows[2, -model.P] == 0.0
    recs, st = nm.assess_fetch(0, B)
    L, A = model.L, recs.shape[1]
    touched = np.zeros(A, dtype=bool)
    touched[L] = True                                        # rho_a of LV 0 (rho_c and ave take the loadings: finite)
    for k in range(3):
        touched[4 * L + 3 * k + np.array([0, 1])] = True     # the pairs (0, 1) and (0, 2) of htmt, htmt2, lv_cor
    assert recs[2, 0] == 0.0                                 # alpha of LV 0: max(0, NaN) is 0, as Python's max in plspm/unidimensionality.py
    assert not np.any(np.isfinite(recs[2, touched])) and np.all(np.isfinite(recs[2, ~touched]))
    keep = np.array([0, 1, 3, 4])
    check_against_mirror(recs[keep], rows[keep], X, model, idx[keep], "beside a constant column")
    Xr = X[idx[2]][:, model.mv_order]
    m64, _ = mirror_pair(Xr[:, 4:], orc.Model([np.arange(4), np.arange(4, 8)], tri(2), "AA", "centroid", True), rows[2, 4:model.P], rows[2, -model.P + 4:])
    mine = recs[2, [1, 2, L + 1, L + 2, 2 * L + 1, 2 * L + 2, 3 * L + 1, 3 * L + 2, 4 * L + 2, 4 * L + 5, 4 * L + 8]]
    np.testing.assert_allclose(mine, m64, rtol=0, atol=1e-12)


def test_summary_intervals_and_errors():
    from plspm import _native
    from plspm.bootstrap import _create_summary, _intervals
    X, model = small_model(seed=12)
    nm = native_model(model, X)
    with pytest.raises(_native.NativeBackendError, match=r"plspm_assess_summary failed \(%d\)" % E_STATE):
        nm.assess_summary(100, np.zeros(nm.assess_width))
    nm.assess_enable(True)
    B = 200
    nm.bootstrap_device(B, 5, 0)
    recs, st = nm.assess_fetch(0, B)
    original, _ = nm.assess_fit()
    ok = recs[st == 0]
    table, used = nm.assess_summary(B, original)
    assert used == ok.shape[0] and used >= B - 2
    host = _create_summary(pd.DataFrame(ok), pd.Series(original)).values
    print("assess summary: max rel difference %.3e" % np.max(np.abs(table - host) / np.maximum(np.abs(host), 1e-300)))
    np.testing.assert_allclose(table, host, rtol=1e-12, atol=0)
    for method in ("percentile", "basic", "bc"):
        for level in (0.9, 0.95):
            out, used_i = nm.assess_intervals(B, original, method, level)
            mirror = _intervals(ok, original, None, method, level)
            assert used_i == used and np.array_equal(np.isnan(out), np.isnan(mirror))
            fin = ~np.isnan(mirror)
            print("assess intervals %s %.2f: max rel difference %.3e" % (method, level, np.max(np.abs(out[fin] - mirror[fin]) / np.maximum(np.abs(mirror[fin]), 1e-300))))
            np.testing.assert_allclose(out[:, :2], mirror[:, :2], rtol=1e-12, atol=0, err_msg=method)
            np.testing.assert_allclose(out[:, 2:], mirror[:, 2:], rtol=1e-12, atol=1e-12, err_msg=method)      # (z0 and the levels: atol as tests/test_gpu_ci.py)
    with pytest.raises(_native.NativeBackendError, match=r"plspm_assess_intervals failed \(%d\)" % E_ARG):
        nm.assess_intervals(B, original, "bca", 0.95)
    with pytest.raises(_native.NativeBackendError, match=r"plspm_assess_summary failed \(%d\)" % E_ARG):
        nm.assess_summary(B - 1, original)
    with pytest.raises(_native.NativeBackendError, match=r"plspm_assess_fetch failed \(%d\)" % E_ARG):
        nm.assess_fetch(B - 1, 2)
    # a jackknife leaves the bootstrap's records alone, and with them the assessment records; an upload voids both
    nm.jackknife(16)
    again, _ = nm.assess_fetch(0, B)
    assert np.array_equal(again, recs, equal_nan=True)
    nm.upload(X, model.mv_order.astype(np.int32))
    with pytest.raises(_native.NativeBackendError, match=r"plspm_assess_fetch failed \(%d\)" % E_STATE):
        nm.assess_fetch(0, 1)
    # the handle kinds the assessment does not cover
    boff = np.array([0, 4, 8, 12], dtype=np.int32)
    other = _native.NativeModel(boff, tri(3).astype(np.uint8), np.zeros(3, dtype=np.int32), 0, True, 100, 1e-6, 0, nonmetric=True)
    with pytest.raises(_native.NativeBackendError, match=r"plspm_assess_enable failed \(%d\)" % E_ARG):
        other.assess_enable(True)


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


def test_quality_frames():
    from plspm.bootstrap import INTERVAL_COLUMNS, SUMMARY_COLUMNS
    from plspm.plspm import Plspm
    from plspm.quality import Quality
    from plspm.scheme import Scheme
    sat, cfg = sat_config()
    lvs = orc.SAT_LVS
    pairs = ["%s <-> %s" % (lvs[i], lvs[j]) for i in range(6) for j in range(i + 1, 6)]
    q = Quality(sat, cfg, Scheme.PATH, iterations=200, seed=3)
    via = Plspm(sat, cfg, Scheme.PATH, bootstrap=True, bootstrap_iterations=200, seed=3, quality=True).quality()
    for name in ("reliability", "htmt", "htmt2", "lv_correlations", "fornell_larcker"):
        pd.testing.assert_frame_equal(getattr(q, name)(), getattr(via, name)())
    rel = q.reliability()
    assert list(rel.index) == lvs and list(rel.columns) == ["alpha", "rho_a", "rho_c", "ave"]
    assert np.all((rel.values > 0.3) & (rel.values < 1.0))
    for frame in (q.htmt(), q.htmt2(), q.lv_correlations()):
        assert frame.shape == (6, 6) and list(frame.index) == lvs and list(frame.columns) == lvs
        assert np.allclose(frame.values, frame.values.T) and np.all(np.diag(frame.values) == 1.0)
    fl = q.fornell_larcker()
    assert np.allclose(np.diag(fl.values), np.sqrt(rel["ave"].values))
    assert np.all(np.isnan(fl.values[np.triu_indices(6, 1)]))
    assert np.array_equal(fl.values[np.tril_indices(6, -1)], q.lv_correlations().values[np.tril_indices(6, -1)])
    assert q.used() == 200 and q.replicates().shape == (200, 4 * 6 + 3 * 15)
    for criterion in ("alpha", "rho_a", "rho_c", "ave"):
        s = q.summary(criterion)
        assert list(s.index) == lvs and list(s.columns) == SUMMARY_COLUMNS
        assert np.array_equal(s["original"].values, rel[criterion].values)
        pd.testing.assert_frame_equal(s, via.summary(criterion))          # same seed, same replicates
    for criterion in ("htmt", "htmt2", "lv_cor"):
        s = q.summary(criterion)
        assert list(s.index) == pairs and list(s.columns) == SUMMARY_COLUMNS
        iv = q.intervals(criterion, "bc", 0.9)
        assert list(iv.index) == pairs and list(iv.columns) == INTERVAL_COLUMNS
        assert np.all(iv["lower"].values <= iv["upper"].values)
    assert np.array_equal(q.summary("htmt")["original"].values, q.htmt().values[np.triu_indices(6, 1)])
    pct = q.intervals("htmt", "percentile", 0.95)
    assert np.array_equal(pct["lower"].values, q.summary("htmt")["perc.025"].values)
    with pytest.raises(NotImplementedError):
        q.intervals("htmt", "bca")
    with pytest.raises(NotImplementedError):
        Quality(sat, cfg, Scheme.PATH, iterations=100, processes=2)
    with pytest.raises(ValueError):
        q.summary("gof")
    with pytest.raises(Exception, match="quality"):
        Plspm(sat, cfg, Scheme.PATH).quality()
