"""GPU: the geodesic discrepancy d_G of bootstrap replicates (include/plspm_hip.h plspm_geodesic_*; csrc/kernels_geodesic.h, csrc/geodesic_core.h; plspm.modelfit).

Kernel against the mirror.  Per replicate, the device's geodesic record against the fp64 mirror (plspm.modelfit._geodesic_fit on _model_fit on plspm.plsc._plsc
on NumPy's correlation matrix of the resampled rows) fed the device's own record weights and loadings.  The bar is helpers_geodesic.bar: ten times the larger of
|fp64 mirror - 40-digit| and |host program of csrc/geodesic_core.h - 40-digit|, measured per case on the CPU with the oracle's fits (tools/geodesic_floor.py;
the figures: helpers_geodesic.FLOOR_FIGURES), never below the project's 1e-12 -- the device differs from the host program only by contraction and by the lane
order of its fixed-order sums.  The shapes are tests/helpers_plsc.py's, the smallest that reach the kernel's branches: P = 2 (nothing to tridiagonalise, equal
eigenvalues), one window of 64 columns, the 64 | 65 edge (P = 70), P = 120 on one wave per workgroup, L = 33, the tile-packed layout, the fp64 Gram."""
import numpy as np
import pandas as pd
import pytest

import plspm_oracle as orc
from helpers import SAT_ADD_ORDER, SAT_PREFIX, satisfaction_frame, satisfaction_oracle_inputs
from helpers_geodesic import bar, comparable, mirror_geodesic, oracle_problem, smallest_phi
from helpers_modelfit import PATH, PATH_WITHOUT_02, population_sample
from helpers_plsc import CASES, case, native_model, resamples, tri

pytestmark = pytest.mark.gpu
E_ARG, E_STATE, E_LIMIT = 100, 101, 102
INADMISSIBLE = 4


def zero_mask(model):
    return np.zeros(model.L, dtype=np.uint8)


# ------------------------------------------------------------------ 1. the kernel against the mirror
@pytest.mark.parametrize("name", CASES)
def test_kernel_against_the_mirror(name):
    X, model, options, _, gram_path, _ = case(name)
    mask = zero_mask(model)
    nm = native_model(model, X, **options)
    nm.geodesic_enable(True, mask)
    assert nm.geodesic_width == 2
    B, P = 9, model.P                                        # more than one workgroup at every waves-per-workgroup count
    idx = resamples(X, B)
    rows, status, iters = nm.bootstrap(B, idx=idx)
    assert np.all(status == 0)
    assert nm.get_option("last_gram_path") == gram_path
    recs, st = nm.geodesic_fetch(0, B)
    assert recs.shape == (B, 2) and np.all(st == 0) and np.all(np.isfinite(recs))
    worst = 0.0
    for r in range(B):
        geo, fit = mirror_geodesic(X[idx[r]][:, model.mv_order], model, rows[r, :P], rows[r, -P:], mask)
        assert fit["status"] == 0 and geo["status"] == 0, (name, r, "the inputs must be admissible")
        diff = float(np.max(np.abs(recs[r] - geo["record"])))
        worst = max(worst, diff)
        assert diff <= bar(name), "%s replicate %d: max |device - mirror| %.3e above the bar %.3e" % (name, r, diff, bar(name))
    print("%s: max |device - mirror| %.3e over %d replicates (bar %.3e; largest d_G %.4f)" % (name, worst, B, bar(name), recs.max()))
    if name == "single_items":                               # two single items: both models reproduce r_01
        assert np.all(recs <= 1e-24)
    # the three earlier stages' records are there as well
    for fetch in (nm.assess_fetch, nm.plsc_fetch, nm.modelfit_fetch):
        other, ost = fetch(0, B)
        assert np.all(ost == 0) and np.all(np.isfinite(other))
    # the full-sample record: the same four kernels on the moments of all rows and plspm_fit's solver problem
    fit = nm.fit(want_scores=False)
    full, fst = nm.geodesic_fit()
    assert fst == 0 and fit["status"] == 0
    geo, _ = mirror_geodesic(X[:, model.mv_order], model, fit["weights"], fit["loadings"], mask)
    assert geo["status"] == 0
    diff = float(np.max(np.abs(full - geo["record"])))
    print("%s: plspm_geodesic_fit max |device - mirror| %.3e" % (name, diff))
    assert diff <= bar(name)


# ------------------------------------------------------------------ 2. status agreement under the cases' own masks
@pytest.mark.parametrize("name", CASES)
def test_status_agrees_with_the_mirror_under_the_cases_own_mask(name):
    X, model, options, _, _, factor = case(name)
    nm = native_model(model, X, **options)
    nm.geodesic_enable(True, factor)                         # (None: the default mask of a handle that never had another)
    B, P = 9, model.P
    idx = resamples(X, B)
    rows, status, _ = nm.bootstrap(B, idx=idx)
    assert np.all(status == 0)
    recs, st = nm.geodesic_fetch(0, B)
    mst = nm.modelfit_fetch(0, B)[1]
    fit = nm.fit(want_scores=False)
    full, fst = nm.geodesic_fit()
    device = [(recs[r], st[r], X[idx[r]], rows[r, :P], rows[r, -P:]) for r in range(B)] + [(full, fst, X, fit["weights"], fit["loadings"])]
    mirrors = [mirror_geodesic(Xr[:, model.mv_order], model, w, lam, factor) for _, _, Xr, w, lam in device]
    keep = comparable([geo for geo, _ in mirrors])           # (asserts that the mirror alone leaves out one data set in ten at most)
    left_out, admissible = keep.count(False), 0
    for r, ((rec, dst, _, _, _), (geo, mfit)) in enumerate(zip(device, mirrors)):
        if r < B:
            assert mst[r] == mfit["status"], (name, r)
        if not keep[r]:                                      # within 1e-6 of singular: either side may fall either way
            continue
        assert dst == geo["status"], "%s data set %d: device status %d, mirror %d (smallest |phi| %.3e)" % (name, r, dst, geo["status"], smallest_phi(geo))
        if geo["status"] == 0:
            admissible += 1
            assert float(np.max(np.abs(rec - geo["record"]))) <= bar(name), (name, r, rec, geo["record"])
        else:
            assert dst == INADMISSIBLE and np.all(np.isnan(rec)), (name, r)
    print("%s: %d of %d data sets admissible, %d left out" % (name, admissible, len(device), left_out))
    _, used = nm.geodesic_summary(B, np.zeros(2))
    assert used == np.count_nonzero(st == 0)


def small_model(seed=9, n=320):
    X, blocks = orc.synth(n, tri(3), 4, seed=seed)
    return X, orc.Model(blocks, tri(3), "AAA", "centroid", True)


# ------------------------------------------------------------------ 3. offsets, and nothing else moves
def test_sub_batches_and_bit_identity():
    """plspm_bootstrap() as three sub-batches against one plspm_bootstrap_device batch, bit for bit on the geodesic records; the bootstrap's records, status and
    iteration counts and the assessment, PLSc and model-fit records bit-identical with the stage on and off."""
    from plspm import _native
    X, model = small_model()
    B, seed = 1537, 7
    mask = zero_mask(model)
    off = native_model(model, X, boot_chunks=3, boot_align=64)
    off.modelfit_enable(True, mask)
    rows0, status0, iters0 = off.bootstrap(B, seed=seed)
    before = [fetch(0, B) for fetch in (off.assess_fetch, off.plsc_fetch, off.modelfit_fetch)]
    with pytest.raises(_native.NativeBackendError, match=r"plspm_geodesic_fetch failed \(%d\)" % E_STATE):
        off.geodesic_fetch(0, 1)                             # the stage is off: nothing written
    nm = native_model(model, X, boot_chunks=3, boot_align=64)
    nm.geodesic_enable(True, mask)
    parts = _native.chunk_plan(B, nm.row_stride * 8, 3, 60, 64)
    assert len(parts) == 3 and sum(parts) == B, parts
    rows1, status1, iters1 = nm.bootstrap(B, seed=seed)
    chunked, st1 = nm.geodesic_fetch(0, B)
    after = [fetch(0, B) for fetch in (nm.assess_fetch, nm.plsc_fetch, nm.modelfit_fetch)]
    assert np.array_equal(rows0, rows1) and np.array_equal(status0, status1) and np.array_equal(iters0, iters1)
    for (r0, s0), (r1, s1) in zip(before, after):
        assert np.array_equal(r0, r1, equal_nan=True) and np.array_equal(s0, s1)
    nm.bootstrap_device(B, seed, 0)                          # one batch
    nm.sync()
    whole, st2 = nm.geodesic_fetch(0, B)
    assert np.array_equal(chunked, whole, equal_nan=True) and np.array_equal(st1, st2)
    assert np.all(np.isfinite(whole[st2 == 0])) and np.all(np.isnan(whole[st2 != 0])) and np.count_nonzero(st2 == 0) >= B - 8
    tail, _ = nm.geodesic_fetch(B - 2, 2)
    assert np.array_equal(tail, whole[B - 2:], equal_nan=True)
    P = model.P
    for r in (0, parts[0], parts[0] + parts[1], B - 1):
        if st2[r] == 0:
            geo, _ = mirror_geodesic(X[_native.bootstrap_indices(seed, int(r), X.shape[0])][:, model.mv_order], model, rows1[r, :P], rows1[r, -P:], mask)
            assert geo["status"] == 0 and float(np.max(np.abs(whole[r] - geo["record"]))) <= 1e-12


def test_two_passes_are_bit_identical_to_one():
    X, model = small_model()
    B, seed = 512, 41
    one = native_model(model, X)
    one.geodesic_enable(True, zero_mask(model))
    one.bootstrap(B, seed=seed)
    assert one.get_option("last_boot_passes") == 1
    want, wst = one.geodesic_fetch(0, B)
    two = native_model(model, X, boot_pass=256)
    two.geodesic_enable(True, zero_mask(model))
    two.bootstrap(B, seed=seed)
    assert two.get_option("last_boot_passes") == 2
    got, gst = two.geodesic_fetch(0, B)
    assert np.array_equal(got, want, equal_nan=True) and np.array_equal(gst, wst) and np.count_nonzero(gst == 0) >= B - 8


# ------------------------------------------------------------------ 4. failed replicates, summary and intervals, call kinds, errors
def test_failed_replicates_keep_their_status_and_are_nan():
    X, model = small_model()
    B = 24
    idx = resamples(X, B, seed=3)
    _, status, iters = native_model(model, X).bootstrap(B, idx=idx)
    assert np.all(status == 0) and iters.min() < iters.max()
    model.max_iter = int(iters.min())
    nm = native_model(model, X)
    nm.geodesic_enable(True, zero_mask(model))
    _, status, _ = nm.bootstrap(B, idx=idx)
    failed = status != 0
    assert 0 < failed.sum() < B
    recs, st = nm.geodesic_fetch(0, B)
    assert np.array_equal(st, status)
    assert np.all(np.isnan(recs[failed])) and np.all(np.isfinite(recs[~failed]))
    _, used = nm.geodesic_summary(B, recs[~failed][0])
    assert used == B - failed.sum()


def test_summary_intervals_call_kinds_and_errors():
    from plspm import _native
    from plspm.bootstrap import _create_summary, _intervals
    X, model = small_model(seed=12)
    N = X.shape[0]
    nm = native_model(model, X)
    with pytest.raises(_native.NativeBackendError, match=r"plspm_geodesic_fetch failed \(%d\)" % E_STATE):
        nm.geodesic_fetch(0, 1)                              # before any run
    nm.geodesic_enable(True, zero_mask(model))
    B = 200
    nm.bootstrap_device(B, 5, 0)
    recs, st = nm.geodesic_fetch(0, B)
    original, ost = nm.geodesic_fit()
    assert ost == 0
    ok = recs[st == 0]
    table, used = nm.geodesic_summary(B, original)
    assert used == ok.shape[0] and used >= B - 5
    np.testing.assert_allclose(table, _create_summary(pd.DataFrame(ok), pd.Series(original)).values, rtol=1e-12, atol=1e-15)
    for method in ("percentile", "basic", "bc"):
        out, used_i = nm.geodesic_intervals(B, original, method, 0.9)
        mirror = _intervals(ok, original, None, method, 0.9)
        assert used_i == used
        np.testing.assert_allclose(out[:, :2], mirror[:, :2], rtol=1e-12, atol=1e-15, err_msg=method)
    with pytest.raises(_native.NativeBackendError, match=r"plspm_geodesic_intervals failed \(%d\)" % E_ARG):
        nm.geodesic_intervals(B, original, "bca", 0.95)
    with pytest.raises(_native.NativeBackendError, match=r"plspm_geodesic_summary failed \(%d\)" % E_ARG):
        nm.geodesic_summary(B - 1, original)
    nm.jackknife(16)                                         # a jackknife leaves them alone
    assert np.array_equal(nm.geodesic_fetch(0, B)[0], recs, equal_nan=True)

    def gone():
        with pytest.raises(_native.NativeBackendError, match=r"plspm_geodesic_fetch failed \(%d\)" % E_STATE):
            nm.geodesic_fetch(0, 1)

    def back():
        nm.bootstrap_device(B, 5, 0)
        assert np.array_equal(nm.geodesic_fetch(0, B)[0], recs, equal_nan=True)

    member = np.arange(N) < N // 2
    nm.permutation(8, N // 2, seed=3)                        # the other call kinds replace the bootstrap's records and write none
    gone(); back()
    nm.stratified_bootstrap(8, member, seed=3)
    gone(); back()
    nm.cv(2, 4, seed=3)
    gone(); back()
    nm.bootstrap_moments(4, seed=3)
    gone(); back()
    nm.upload(X, model.mv_order.astype(np.int32))            # an upload voids them
    gone()
    nm.geodesic_enable(False)                                # off again: no records, and none of the records it brought along
    nm.bootstrap_device(B, 5, 0)
    for fetch, who in ((nm.geodesic_fetch, "geodesic"), (nm.modelfit_fetch, "modelfit"), (nm.plsc_fetch, "plsc"), (nm.assess_fetch, "assess")):
        with pytest.raises(_native.NativeBackendError, match=r"plspm_%s_fetch failed \(%d\)" % (who, E_STATE)):
            fetch(0, 1)
    # bad masks, and the handle kinds the stage does not cover
    odd = _native.NativeModel(np.array([0, 4, 8, 9], dtype=np.int32), tri(3).astype(np.uint8), np.array([0, 1, 0], dtype=np.int32), 0, True, 100, 1e-6, 0)
    odd.geodesic_enable(True)
    odd.geodesic_enable(True, [1, 0, 0])
    for bad_mask in ([1, 1, 0], [1, 0, 1], [2, 0, 0]):       # Mode B; a single item; not 0 / 1
        with pytest.raises(_native.NativeBackendError, match=r"plspm_geodesic_enable failed \(%d\)" % E_ARG):
            odd.geodesic_enable(True, bad_mask)
    other = _native.NativeModel(np.array([0, 4, 8, 12], dtype=np.int32), tri(3).astype(np.uint8), np.zeros(3, dtype=np.int32), 0, True, 100, 1e-6, 0, nonmetric=True)
    with pytest.raises(_native.NativeBackendError, match=r"plspm_geodesic_enable failed \(%d\)" % E_ARG):
        other.geodesic_enable(True)
    with pytest.raises(_native.NativeBackendError, match=r"plspm_geodesic_fetch failed \(%d\)" % E_ARG):
        other.geodesic_fetch(0, 1)


def test_a_model_beyond_one_workgroups_lds_is_refused():
    """P = 144: two triangles of 144 * 145 / 2 doubles and the vectors are 171 KB, above the 160 KiB of a workgroup."""
    from plspm import _native
    X, blocks = orc.synth(300, tri(2), 72, seed=4)
    model = orc.Model(blocks, tri(2), "AA", "centroid", True)
    nm = native_model(model, X)
    nm.geodesic_enable(True, zero_mask(model))
    with pytest.raises(_native.NativeBackendError, match=r"plspm_bootstrap_device failed \(%d\)" % E_LIMIT):
        nm.bootstrap_device(8, 1, 0)
    nm.geodesic_enable(False)
    nm.modelfit_enable(True)
    nm.bootstrap_device(8, 1, 0)                             # model fit alone still runs on it
    assert nm.modelfit_fetch(0, 8)[0].shape == (8, 4)


# ------------------------------------------------------------------ 5. - 7. the host API
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


def satisfaction_problem():
    X, blocks, _ = satisfaction_oracle_inputs()
    return X, orc.Model(blocks, orc.satisfaction_C(), "AAAAAA", "path", True)


def test_frames_on_satisfaction():
    from plspm.modelfit import FIT_COLUMNS, ModelFit
    from plspm.scheme import Scheme
    sat, cfg = sat_config()
    B = 200
    plain = ModelFit(sat, cfg, Scheme.PATH, iterations=B, seed=3)
    mf = ModelFit(sat, cfg, Scheme.PATH, iterations=B, seed=3, geodesic=True)
    frame = mf.fit()
    assert list(frame.index) == ["srmr", "d_uls", "d_g"] and list(frame.columns) == FIT_COLUMNS
    # the default call's frame and accessors are what they were, and the first two rows with the stage on are the same numbers
    assert list(plain.fit().index) == ["srmr", "d_uls"] and plain.fit().equals(frame.iloc[:2])
    assert np.array_equal(plain.records()[0], mf.records()[0], equal_nan=True) and plain.used() == mf.used() and plain.inadmissible() == mf.inadmissible()
    with pytest.raises(ValueError, match="geodesic=True"):
        plain.records(measure="d_g")
    with pytest.raises(ValueError, match="measure"):
        mf.used(measure="nfi")
    assert np.array_equal(mf.records(measure="srmr")[0], mf.records()[0], equal_nan=True)
    records, status = mf.records(measure="d_g")
    assert records.shape == (B, 2) and status.shape == (B,)
    second = mf._transformed.native
    observed = mf._g_observed
    assert np.array_equal(frame.loc["d_g", ["saturated", "estimated"]].values, observed) and np.all(observed > 0)
    for column, level in (("hi95", 0.90), ("hi99", 0.98)):
        table, used = second.geodesic_intervals(B, observed, 0, level)
        assert frame.loc["d_g", column] == table[1, 1] and used == mf.used(measure="d_g")
    ok = records[status == 0]
    p = (1.0 + np.count_nonzero(ok[:, 1] >= observed[1])) / (1.0 + ok.shape[0])
    assert frame.loc["d_g", "p.value"] == p and 0 < p <= 1
    assert frame.loc["d_g", "hi95"] <= frame.loc["d_g", "hi99"]
    assert mf.used(measure="d_g") == ok.shape[0] and mf.inadmissible(measure="d_g") == np.count_nonzero(status == INADMISSIBLE)
    assert mf.inadmissible(measure="d_g") >= mf.inadmissible() and mf.used(measure="d_g") >= B - 10
    # the observed values against the mirror on the frame's own implied matrices
    from plspm.modelfit import _d_g, _geodesic
    R = cfg.filter(sat)[list(mf.implied().columns)].corr().values
    for column, which in enumerate(("saturated", "estimated")):
        gst, phi = _geodesic(R, mf.implied(which).values)
        assert gst == 0
        np.testing.assert_allclose(_d_g(phi), observed[column], rtol=1e-9)
    # values only
    only = ModelFit(sat, cfg, Scheme.PATH, iterations=0, geodesic=True)
    values = only.fit()
    assert np.array_equal(values[["saturated", "estimated"]].values, frame[["saturated", "estimated"]].values)
    assert np.all(np.isnan(values[["hi95", "hi99", "p.value"]].values)) and only.used(measure="d_g") == 0


def test_full_sample_that_is_inadmissible_for_d_g_alone():
    """wave_60x6 under its own (default) mask: the corrected loadings leave no positive definite implied matrix; srmr and d_uls are fine as values.  (Without
    the keyword the same data stop one step later, at the Bollen-Stine transformation, which needs a positive definite implied matrix as well.)"""
    import plspm.config as c
    from plspm.mode import Mode
    from plspm.modelfit import ModelFit
    from plspm.scheme import Scheme
    from plspm.weights import NumericalConditionError
    X, model, _, _, _, _ = case("wave_60x6")
    names = ["x%d" % p for p in range(X.shape[1])]
    lvs = ["L%d" % l for l in range(model.L)]
    cfg = c.Config(pd.DataFrame(model.C, index=lvs, columns=lvs), scaled=True)
    for lv, blk in zip(lvs, model.blocks):
        cfg.add_lv(lv, Mode.A, *[c.MV(names[p]) for p in blk])
    frame = pd.DataFrame(X, columns=names)
    values = ModelFit(frame, cfg, Scheme.PATH, iterations=0, factors=None, geodesic=True).fit()
    assert np.all(np.isfinite(values.loc[["srmr", "d_uls"], ["saturated", "estimated"]].values))
    assert np.all(np.isnan(values.loc["d_g"].values))
    with pytest.raises(NumericalConditionError, match="d_g"):
        ModelFit(frame, cfg, Scheme.PATH, iterations=20, seed=1, factors=None, geodesic=True)


def test_transformed_handle_fits_exactly():
    """Satisfaction, all-factor, Bollen-Stine-transformed to its own estimated model: the reduced matrix is the identity up to rounding -- the near-identity
    case of the Householder guard.  The bar: ten times the d_g_est the mirror gives on the ORACLE's fit of the same rows (on the CPU: 3.6e-27,
    tools/geodesic_floor.py transform)."""
    from plspm.modelfit import ModelFit, _bollen_stine
    from plspm.scheme import Scheme
    sat, cfg = sat_config()
    mf = ModelFit(sat, cfg, Scheme.PATH, iterations=10, seed=1, factors=None, geodesic=True)
    X, model = satisfaction_problem()
    Xt = np.empty_like(X)
    Xt[:, model.mv_order] = _bollen_stine(X[:, model.mv_order], mf._mirror["implied"]["estimated"])
    on_cpu = oracle_problem(Xt, model, None)[3]
    assert on_cpu["status"] == 0
    limit = 10.0 * float(on_cpu["record"][1])
    full, status = mf._transformed.native.geodesic_fit()
    print("transformed handle: d_g_est %.3e on the device, %.3e by the mirror on the oracle's fit (bar %.3e); observed %.4f" % (full[1], on_cpu["record"][1], limit, mf.fit().loc["d_g", "estimated"]))
    assert status == 0 and mf.fit().loc["d_g", "estimated"] > 1.0
    assert 0.0 <= full[1] <= limit


def population_frame(seed):
    import plspm.config as c
    from plspm.mode import Mode
    X = population_sample(300, seed)
    names = ["x%d" % p for p in range(10)]
    lvs = ["A", "B", "C"]

    def config(C):
        cfg = c.Config(pd.DataFrame(C, index=lvs, columns=lvs), scaled=True)
        for lv, blk in zip(lvs, ([0, 1], [2, 3, 4], [5, 6, 7, 8, 9])):
            cfg.add_lv(lv, Mode.A, *[c.MV(names[p]) for p in blk])
        return cfg
    return pd.DataFrame(X, columns=names), config


def test_the_test_does_its_job():
    """300 Gaussian rows from the closed-form population, seed 3, 500 replicates: d_g does not reject the correct model (on the CPU, tools/geodesic_floor.py
    power: p = 0.72 with 200 oracle-driven resamples).  No seed of the first six separates the two models for d_g at n = 300 -- the model without 0 -> 2 gets
    p between 0.15 and 0.41, 0.28 at seed 3, where d_uls rejects it -- so only the correct model's side is asserted."""
    from plspm.modelfit import ModelFit
    from plspm.scheme import Scheme
    frame, config = population_frame(3)
    right = ModelFit(frame, config(PATH), Scheme.PATH, iterations=500, seed=1, factors=None, geodesic=True).fit()
    wrong = ModelFit(frame, config(PATH_WITHOUT_02), Scheme.PATH, iterations=500, seed=1, factors=None, geodesic=True).fit()
    print("correct model:\n%s\nwithout 0 -> 2:\n%s" % (right, wrong))
    assert right.loc["d_g", "p.value"] >= 0.10
    np.testing.assert_allclose(right.loc["d_g", "estimated"], 0.14815, atol=5e-5)
    np.testing.assert_allclose(wrong.loc["d_g", "estimated"], 0.24050, atol=5e-5)
    assert wrong.loc["d_g", "estimated"] > right.loc["d_g", "estimated"]
