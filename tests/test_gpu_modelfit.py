"""GPU: model fit of bootstrap replicates (include/plspm_hip.h plspm_modelfit_*; csrc/kernels_modelfit.h, csrc/modelfit_core.h; plspm.modelfit).

Kernel against the mirror.  Per replicate, the device's model-fit record against the fp64 mirror (plspm.modelfit._model_fit on plspm.plsc._plsc on NumPy's
correlation matrix of the resampled rows) fed the device's own record weights and loadings.  The bar is DESIGN.md 5m's: ten times the largest difference, on
those same inputs, between the fp64 mirror and the same mirror in np.longdouble, with an absolute floor.  The floor is the largest such difference measured on
the CPU with the oracle's weights and loadings in place of the device's (tools/modelfit_floor.py), never below 1e-12 -- the figures, per case over nine
resamples and all rows:

    single_items 1.3e-17   wave_60x6 1.4e-14   quad_120x12 3.8e-14   lds_65_5 5.0e-14   packed_40 7.1e-15   fp64_gram 9.6e-16   mode_b 7.9e-16
    nine_predecessors 1.0e-16   lv_33 2.4e-15   mixed_mask 9.0e-15

so the floor is 1e-12 (d_uls is a sum of up to 7,140 squares and reaches 40 or so on these shapes: the differences are a few units in its last place).  The
shapes are tests/helpers_plsc.py's, the smallest that reach the kernel's branches: single items (no block rule to apply), one window of 64 columns, the 64 | 65
window edge, two windows, the tile-packed layout, the fp64 Gram, a Mode-B composite among factors, nine predecessors, 33 LVs (33 rows of the recursion, more
LV pairs than lanes), a mask that mixes factors and composites.  Every one of the nine resamples of every case is admissible in the mirror (asserted)."""
import numpy as np
import pandas as pd
import pytest

import plspm_oracle as orc
from helpers import SAT_ADD_ORDER, SAT_PREFIX, satisfaction_frame, satisfaction_oracle_inputs
from helpers_modelfit import (PATH, PATH_WITHOUT_02, mirror_bar, mirror_fit, mirror_fit_pair, oracle_model_fit, perturbation_bar, population_sample)
from helpers_plsc import CASES, case, native_model, negative_pair_model, resamples, tri

pytestmark = pytest.mark.gpu
E_ARG, E_STATE = 100, 101
INADMISSIBLE = 4


def check_against_mirror(recs, rows, X, model, idx, factor, tag):
    P, worst, bar = model.P, 0.0, np.inf
    for r in range(idx.shape[0]):
        m64, mld = mirror_fit_pair(X[idx[r]][:, model.mv_order], model, rows[r, :P], rows[r, -P:], factor)
        assert m64["status"] == 0 and mld["status"] == 0, (tag, r, "the inputs must be admissible")
        this_bar = mirror_bar(m64, mld)
        diff = float(np.max(np.abs(recs[r] - m64["record"])))
        worst, bar = max(worst, diff), min(bar, this_bar)
        assert np.all(np.isfinite(recs[r])), (tag, r)
        assert diff <= this_bar, "%s replicate %d: max |device - mirror| %.3e above the bar %.3e" % (tag, r, diff, this_bar)
    print("%s: max |device - mirror| %.3e over %d replicates (smallest bar %.3e)" % (tag, worst, idx.shape[0], bar))


# ------------------------------------------------------------------ 1. the kernel against the mirror
@pytest.mark.parametrize("name", CASES)
def test_kernel_against_the_mirror(name):
    X, model, options, _, gram_path, factor = case(name)
    nm = native_model(model, X, **options)
    nm.modelfit_enable(True, factor)                         # (None: the default mask of a handle that never had another)
    assert nm.modelfit_width == 4
    B = 9                                                    # two workgroups and one wave
    idx = resamples(X, B)
    rows, status, _ = nm.bootstrap(B, idx=idx)
    assert np.all(status == 0)
    assert nm.get_option("last_gram_path") == gram_path
    recs, st = nm.modelfit_fetch(0, B)
    assert recs.shape == (B, 4) and np.all(st == 0)
    check_against_mirror(recs, rows, X, model, idx, factor, name)
    P = model.P
    np.testing.assert_allclose(recs[:, 0], np.sqrt(2.0 * recs[:, 1] / (P * (P + 1))), rtol=1e-15)
    np.testing.assert_allclose(recs[:, 2], np.sqrt(2.0 * recs[:, 3] / (P * (P + 1))), rtol=1e-15)
    if name == "single_items":                               # two single items: r_01 is reproduced by the saturated model and, with the one path, by the estimated one
        assert np.all(recs <= 1e-12)
    # the assessment and the PLSc records are there as well, whether or not their own switches are on
    arec, ast = nm.assess_fetch(0, B)
    prec, pst = nm.plsc_fetch(0, B)
    assert np.all(ast == 0) and np.all(np.isfinite(arec)) and np.all(pst == 0) and np.all(np.isfinite(prec))
    # the full-sample record: the same three kernels on the moments of all rows and plspm_fit's solver problem
    fit = nm.fit(want_scores=False)
    full, fst = nm.modelfit_fit()
    assert fst == 0 and fit["status"] == 0
    m64, mld = mirror_fit_pair(X[:, model.mv_order], model, fit["weights"], fit["loadings"], factor)
    assert m64["status"] == 0
    diff = float(np.max(np.abs(full - m64["record"])))
    print("%s: plspm_modelfit_fit max |device - mirror| %.3e (bar %.3e)" % (name, diff, mirror_bar(m64, mld)))
    assert diff <= mirror_bar(m64, mld)


# ------------------------------------------------------------------ 2. the mask is read
def test_all_zero_against_all_factor_mask():
    X, model, options, _, _, _ = case("wave_60x6")
    B = 9
    idx = resamples(X, B)
    records = {}
    for tag, mask in (("all-zero mask", np.zeros(model.L, dtype=np.uint8)), ("all-factor mask", np.ones(model.L, dtype=np.uint8))):
        nm = native_model(model, X, **options)
        nm.modelfit_enable(True, mask)
        rows, status, _ = nm.bootstrap(B, idx=idx)
        recs, st = nm.modelfit_fetch(0, B)
        assert np.all(status == 0) and np.all(st == 0)
        check_against_mirror(recs, rows, X, model, idx, mask, tag)
        records[tag] = recs
    assert np.all(records["all-zero mask"] != records["all-factor mask"])
    # NULL keeps the handle's mask: the one plspm_plsc_enable set
    nm = native_model(model, X, **options)
    nm.plsc_enable(True, np.zeros(model.L, dtype=np.uint8))
    nm.modelfit_enable(True)
    nm.bootstrap(B, idx=idx)
    assert np.array_equal(nm.modelfit_fetch(0, B)[0], records["all-zero mask"])


def small_model(seed=9, n=320):
    X, blocks = orc.synth(n, tri(3), 4, seed=seed)
    return X, orc.Model(blocks, tri(3), "AAA", "centroid", True)


# ------------------------------------------------------------------ 3. offsets, and nothing else changes
def test_sub_batches_and_bit_identity():
    """plspm_bootstrap() as three sub-batches against one plspm_bootstrap_device batch, bit for bit on the model-fit records; the bootstrap's records, status and
    iteration counts, and the assessment and PLSc records, bit-identical with model fit on and off.  (The planner makes no part shorter than 512 replicates:
    1,537 of this 12-MV model, a few milliseconds.)"""
    from plspm import _native
    X, model = small_model()
    B, seed = 1537, 7
    off = native_model(model, X, boot_chunks=3, boot_align=64)
    off.plsc_enable(True)
    rows0, status0, iters0 = off.bootstrap(B, seed=seed)
    assess0, ast0 = off.assess_fetch(0, B)
    plsc0, pst0 = off.plsc_fetch(0, B)
    with pytest.raises(_native.NativeBackendError, match=r"plspm_modelfit_fetch failed \(%d\)" % E_STATE):
        off.modelfit_fetch(0, 1)                             # model fit off: nothing written
    nm = native_model(model, X, boot_chunks=3, boot_align=64)
    nm.modelfit_enable(True)
    parts = _native.chunk_plan(B, nm.row_stride * 8, 3, 60, 64)
    assert len(parts) == 3 and sum(parts) == B, parts
    rows1, status1, iters1 = nm.bootstrap(B, seed=seed)
    chunked, st1 = nm.modelfit_fetch(0, B)
    assess1, ast1 = nm.assess_fetch(0, B)
    plsc1, pst1 = nm.plsc_fetch(0, B)
    assert np.array_equal(rows0, rows1) and np.array_equal(status0, status1) and np.array_equal(iters0, iters1)
    assert np.array_equal(assess0, assess1, equal_nan=True) and np.array_equal(ast0, ast1)
    assert np.array_equal(plsc0, plsc1, equal_nan=True) and np.array_equal(pst0, pst1)
    nm.bootstrap_device(B, seed, 0)                          # one batch
    nm.sync()
    whole, st2 = nm.modelfit_fetch(0, B)
    assert np.array_equal(chunked, whole, equal_nan=True) and np.array_equal(st1, st2)
    assert np.all(np.isfinite(whole[st2 == 0])) and np.all(np.isnan(whole[st2 == INADMISSIBLE]))
    assert np.array_equal(st2, pst1)                         # no constant column, no value that is not finite: the PLSc record's status
    pick = np.array([0, parts[0], parts[0] + parts[1], B - 1])
    pick = pick[st2[pick] == 0]
    idx = np.stack([_native.bootstrap_indices(seed, int(r), X.shape[0]) for r in pick])
    check_against_mirror(chunked[pick], rows1[pick], X, model, idx, None, "sub-batches")
    tail, _ = nm.modelfit_fetch(B - 2, 2)
    assert np.array_equal(tail, whole[B - 2:], equal_nan=True)


# ------------------------------------------------------------------ 4. two passes
def test_two_passes_are_bit_identical_to_one():
    X, model = small_model()
    B, seed = 512, 41
    one = native_model(model, X)
    one.modelfit_enable(True)
    one.bootstrap(B, seed=seed)
    assert one.get_option("last_boot_passes") == 1
    want, wst = one.modelfit_fetch(0, B)
    two = native_model(model, X, boot_pass=256)
    two.modelfit_enable(True)
    two.bootstrap(B, seed=seed)
    assert two.get_option("last_boot_passes") == 2
    got, gst = two.modelfit_fetch(0, B)
    assert np.array_equal(got, want, equal_nan=True) and np.array_equal(gst, wst) and np.count_nonzero(gst == 0) >= B - 8


# ------------------------------------------------------------------ 5. status
def test_inadmissible_replicates_have_the_mirrors_status():
    X, model = negative_pair_model()
    nm = native_model(model, X)
    nm.modelfit_enable(True)
    B, P = 24, model.P
    idx = resamples(X, B, seed=3)
    rows, status, _ = nm.bootstrap(B, idx=idx)
    assert np.all(status == 0)
    recs, st = nm.modelfit_fetch(0, B)
    expect = np.array([mirror_fit(X[idx[r]][:, model.mv_order], model, rows[r, :P], rows[r, -P:], None)[0]["status"] for r in range(B)], dtype=np.int32)
    bad = expect == INADMISSIBLE
    assert bad.sum() >= B // 2
    assert np.array_equal(st, expect)
    assert np.all(np.isnan(recs[bad])) and np.all(np.isfinite(recs[~bad]))
    if (~bad).any():
        check_against_mirror(recs[~bad], rows[~bad], X, model, idx[~bad], None, "beside inadmissible replicates")
    _, used = nm.modelfit_summary(B, np.zeros(4))
    assert used == B - bad.sum()
    full, fst = nm.modelfit_fit()                            # the full sample: rho_A negative
    assert fst == INADMISSIBLE and np.all(np.isnan(full))


def test_a_column_that_is_constant_in_the_replicate_is_inadmissible():
    """A rare 0 / 1 indicator and index lists that miss every one."""
    X, model = small_model()
    X = X.copy()
    col = int(model.mv_order[5])
    X[:, col] = 0.0
    X[:6, col] = 1.0
    nm = native_model(model, X)
    nm.modelfit_enable(True, np.zeros(model.L, dtype=np.uint8))
    B = 6
    idx = np.random.default_rng(2).integers(6, X.shape[0], (B, X.shape[0])).astype(np.int32)
    idx[0, :40] = np.arange(40)                              # replicate 0 keeps the ones
    rows, status, _ = nm.bootstrap(B, idx=idx)
    recs, st = nm.modelfit_fetch(0, B)
    print("bootstrap status %s, PLSc status %s, model-fit status %s" % (status, nm.plsc_fetch(0, B)[1], st))
    assert status[0] == 0 and st[0] == 0 and np.all(np.isfinite(recs[0]))
    ok = status[1:] == 0
    assert ok.any()
    assert np.all(st[1:][ok] == INADMISSIBLE) and np.all(np.isnan(recs[1:]))
    assert np.array_equal(st[1:][~ok], status[1:][~ok])


def test_failed_replicates_keep_their_status_and_are_nan():
    """Replicates that stop at max_iter, as tests/test_gpu_plsc.py makes them."""
    X, model = small_model()
    B = 24
    idx = resamples(X, B, seed=3)
    _, status, iters = native_model(model, X).bootstrap(B, idx=idx)
    assert np.all(status == 0) and iters.min() < iters.max()
    model.max_iter = int(iters.min())
    nm = native_model(model, X)
    nm.modelfit_enable(True)
    rows, status, _ = nm.bootstrap(B, idx=idx)
    failed = status != 0
    assert 0 < failed.sum() < B
    recs, st = nm.modelfit_fetch(0, B)
    assert np.array_equal(st, status)
    assert np.all(np.isnan(recs[failed])) and np.all(np.isfinite(recs[~failed]))
    check_against_mirror(recs[~failed], rows[~failed], X, model, idx[~failed], None, "beside failed replicates")
    _, used = nm.modelfit_summary(B, recs[~failed][0])
    assert used == B - failed.sum()


def test_summary_intervals_and_errors():
    from plspm import _native
    from plspm.bootstrap import _create_summary, _intervals
    X, model = small_model(seed=12)
    nm = native_model(model, X)
    with pytest.raises(_native.NativeBackendError, match=r"plspm_modelfit_fetch failed \(%d\)" % E_STATE):
        nm.modelfit_fetch(0, 1)                              # before any run
    nm.modelfit_enable(True)
    B = 200
    nm.bootstrap_device(B, 5, 0)
    recs, st = nm.modelfit_fetch(0, B)
    original, ost = nm.modelfit_fit()
    assert ost == 0
    ok = recs[st == 0]
    table, used = nm.modelfit_summary(B, original)
    assert used == ok.shape[0] and used >= B - 5
    np.testing.assert_allclose(table, _create_summary(pd.DataFrame(ok), pd.Series(original)).values, rtol=1e-12, atol=1e-15)
    for method in ("percentile", "basic", "bc"):
        out, used_i = nm.modelfit_intervals(B, original, method, 0.9)
        mirror = _intervals(ok, original, None, method, 0.9)
        assert used_i == used
        np.testing.assert_allclose(out[:, :2], mirror[:, :2], rtol=1e-12, atol=1e-15, err_msg=method)
    with pytest.raises(_native.NativeBackendError, match=r"plspm_modelfit_intervals failed \(%d\)" % E_ARG):
        nm.modelfit_intervals(B, original, "bca", 0.95)
    with pytest.raises(_native.NativeBackendError, match=r"plspm_modelfit_summary failed \(%d\)" % E_ARG):
        nm.modelfit_summary(B - 1, original)
    nm.jackknife(16)                                         # a jackknife leaves them alone
    assert np.array_equal(nm.modelfit_fetch(0, B)[0], recs, equal_nan=True)
    nm.permutation(8, X.shape[0] // 2, seed=3)               # a permutation call replaces the bootstrap's records and writes none
    with pytest.raises(_native.NativeBackendError, match=r"plspm_modelfit_fetch failed \(%d\)" % E_STATE):
        nm.modelfit_fetch(0, 1)
    nm.bootstrap_device(B, 5, 0)
    assert np.array_equal(nm.modelfit_fetch(0, B)[0], recs, equal_nan=True)
    nm.upload(X, model.mv_order.astype(np.int32))            # an upload voids them
    with pytest.raises(_native.NativeBackendError, match=r"plspm_modelfit_fetch failed \(%d\)" % E_STATE):
        nm.modelfit_fetch(0, 1)
    nm.modelfit_enable(False)                                # off again: no records, and none of the records it brought along
    nm.bootstrap_device(B, 5, 0)
    for fetch, who in ((nm.modelfit_fetch, "modelfit"), (nm.plsc_fetch, "plsc"), (nm.assess_fetch, "assess")):
        with pytest.raises(_native.NativeBackendError, match=r"plspm_%s_fetch failed \(%d\)" % (who, E_STATE)):
            fetch(0, 1)
    # bad masks, and the handle kinds model fit does not cover
    odd = _native.NativeModel(np.array([0, 4, 8, 9], dtype=np.int32), tri(3).astype(np.uint8), np.array([0, 1, 0], dtype=np.int32), 0, True, 100, 1e-6, 0)
    odd.modelfit_enable(True)
    odd.modelfit_enable(True, [1, 0, 0])
    for bad_mask in ([1, 1, 0], [1, 0, 1], [2, 0, 0]):       # Mode B; a single item; not 0 / 1
        with pytest.raises(_native.NativeBackendError, match=r"plspm_modelfit_enable failed \(%d\)" % E_ARG):
            odd.modelfit_enable(True, bad_mask)
    other = _native.NativeModel(np.array([0, 4, 8, 12], dtype=np.int32), tri(3).astype(np.uint8), np.zeros(3, dtype=np.int32), 0, True, 100, 1e-6, 0, nonmetric=True)
    with pytest.raises(_native.NativeBackendError, match=r"plspm_modelfit_enable failed \(%d\)" % E_ARG):
        other.modelfit_enable(True)
    with pytest.raises(_native.NativeBackendError, match=r"plspm_modelfit_fetch failed \(%d\)" % E_ARG):
        other.modelfit_fetch(0, 1)


# ------------------------------------------------------------------ 6. against the oracle's fits
def satisfaction_problem():
    X, blocks, _ = satisfaction_oracle_inputs()
    return X, orc.Model(blocks, orc.satisfaction_C(), "AAAAAA", "path", True)


def test_against_the_oracles_fits_on_satisfaction():
    """The mirror on the ORACLE's records against the device's records.  The bar: ten times the largest movement of a statistic when the oracle's weights and
    loadings are perturbed inside the project's record bar (rtol 1e-8, atol 1e-11; 20 draws per replicate) -- measured on the CPU (tools/modelfit_floor.py):
    the largest movement over these 20 replicates is 1.3e-7."""
    X, model = satisfaction_problem()
    B, P = 20, model.P
    idx = resamples(X, B, seed=11)
    nm = native_model(model, X)
    nm.modelfit_enable(True)
    rows, status, _ = nm.bootstrap(B, idx=idx)
    recs, st = nm.modelfit_fetch(0, B)
    assert np.all(status == 0)
    corr, worst, compared = orc.correction(X.shape[0]), 0.0, 0
    for r in range(B):
        mine, _ = orc.bootstrap_replicate(X, model, idx[r], corr)
        Xr = X[idx[r]][:, model.mv_order]
        w, lam = mine[:P][model.mv_order], mine[-P:][model.mv_order]      # (the oracle's record is in data column order)
        expect = mirror_fit(Xr, model, w, lam, None)[0]
        assert st[r] == expect["status"], r
        if expect["status"] == INADMISSIBLE:                 # (a few resamples of these 250 rows are: one of these 20)
            assert np.all(np.isnan(recs[r]))
            continue
        compared += 1
        bar = perturbation_bar(Xr, model, w, lam, None)
        diff = float(np.max(np.abs(recs[r] - expect["record"])))
        worst = max(worst, diff)
        assert diff <= bar, "replicate %d: max |device - mirror on the oracle's record| %.3e above the bar %.3e" % (r, diff, bar)
    print("oracle's fits: max |device - mirror on the oracle's record| %.3e over %d replicates" % (worst, compared))
    assert compared >= B - 2


# ------------------------------------------------------------------ 7. - 9. the host API
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


def test_frames_on_satisfaction():
    from plspm.modelfit import FIT_COLUMNS, ModelFit
    from plspm.scheme import Scheme
    sat, cfg = sat_config()
    B = 200
    mf = ModelFit(sat, cfg, Scheme.PATH, iterations=B, seed=3)
    frame = mf.fit()
    assert list(frame.columns) == FIT_COLUMNS == ["saturated", "estimated", "hi95", "hi99", "p.value"] and list(frame.index) == ["srmr", "d_uls"]
    assert mf.factors() == [] and mf.null() == "estimated" and mf.seed() == 3 and mf.status() == 0
    records, status = mf.records()
    assert records.shape == (B, 4) and status.shape == (B,)
    second = mf._transformed.native
    observed = mf._observed
    assert np.array_equal(frame["saturated"].values, observed[:2]) and np.array_equal(frame["estimated"].values, observed[2:])
    for column, level in (("hi95", 0.90), ("hi99", 0.98)):
        table, used = second.modelfit_intervals(B, observed, 0, level)
        assert np.array_equal(frame[column].values, table[2:, 1]) and used == mf.used()
    ok = records[status == 0]
    assert np.array_equal(mf.replicates(), ok)
    p = (1.0 + np.count_nonzero(ok[:, 2:] >= observed[2:], axis=0)) / (1.0 + ok.shape[0])
    assert np.array_equal(frame["p.value"].values, p) and np.all(p > 0) and np.all(p <= 1)
    assert np.all(frame["hi95"].values <= frame["hi99"].values)
    assert mf.used() == ok.shape[0] and mf.inadmissible() == np.count_nonzero(status == INADMISSIBLE)
    assert mf.used() + mf.inadmissible() == B - np.count_nonzero((status != 0) & (status != INADMISSIBLE)) and mf.used() >= B - 10
    # srmr and d_uls are monotone in each other: the two tests agree
    assert frame.loc["srmr", "p.value"] == frame.loc["d_uls", "p.value"]
    implied = mf.implied("estimated")
    assert implied.shape == (27, 27) and list(implied.index) == list(implied.columns) and np.all(np.diag(implied.values) == 1.0)
    R = cfg.filter(sat)[list(implied.columns)].corr().values
    P = 27
    np.testing.assert_allclose(0.5 * np.sum((R - implied.values) ** 2), observed[3], rtol=1e-9)
    np.testing.assert_allclose(np.sqrt(np.sum((R - mf.implied("saturated").values) ** 2) / (P * (P + 1))), observed[0], rtol=1e-9)
    with pytest.raises(ValueError):
        mf.implied("independence")
    # the saturated model as the null
    sat_null = ModelFit(sat, cfg, Scheme.PATH, iterations=B, seed=3, null="saturated").fit()
    assert np.array_equal(sat_null[["saturated", "estimated"]].values, frame[["saturated", "estimated"]].values)
    assert not np.array_equal(sat_null["hi95"].values, frame["hi95"].values)
    # values only
    only = ModelFit(sat, cfg, Scheme.PATH, iterations=0)
    values = only.fit()
    assert np.array_equal(values[["saturated", "estimated"]].values, frame[["saturated", "estimated"]].values)
    assert np.all(np.isnan(values[["hi95", "hi99", "p.value"]].values)) and only.used() == 0
    with pytest.raises(Exception, match="iterations=0"):
        only.records()
    # common factors change the values
    factors = ModelFit(sat, cfg, Scheme.PATH, iterations=0, factors=None)
    assert factors.factors() == orc.SAT_LVS and not np.array_equal(factors.fit()["estimated"].values, frame["estimated"].values)


def test_transformed_handle_fits_exactly():
    """On the transformed rows of an all-factor model PLSc recovers the loadings and construct correlations the implied matrix was built from, so the
    full-sample srmr_est of the second handle is zero up to rounding.  The bar: ten times what the mirror gives on the ORACLE's fit of the same rows (on the
    CPU: 1.7e-15, tools/modelfit_floor.py)."""
    from plspm.modelfit import ModelFit, _bollen_stine
    from plspm.scheme import Scheme
    sat, cfg = sat_config()
    mf = ModelFit(sat, cfg, Scheme.PATH, iterations=10, seed=1, factors=None)
    X, model = satisfaction_problem()
    Xt = np.empty_like(X)
    Xt[:, model.mv_order] = _bollen_stine(X[:, model.mv_order], mf._mirror["implied"]["estimated"])
    on_cpu = oracle_model_fit(Xt, model, None)
    assert on_cpu["status"] == 0
    bar = 10.0 * float(on_cpu["srmr_est"])
    full, status = mf._transformed.native.modelfit_fit()
    print("transformed handle: srmr_est %.3e on the device, %.3e by the mirror on the oracle's fit (bar %.3e); observed %.4f" % (full[2], on_cpu["srmr_est"], bar, mf.fit().loc["srmr", "estimated"]))
    assert status == 0 and mf.fit().loc["srmr", "estimated"] > 0.01
    assert full[2] <= bar


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
    """300 Gaussian rows from the closed-form population, 500 replicates: the correct model is not rejected, the model without the path 0 -> 2 is.  The seed
    was chosen on the CPU (tools/modelfit_floor.py power seed=3: an oracle-driven bootstrap of the transformed rows, the mirror on the oracle's fits, 200
    resamples): p = 0.75 for the correct model, and for the misspecified one the smallest possible p, 1 / 201, with d_uls_est 0.289 above the 99 % quantile 0.226."""
    from plspm.modelfit import ModelFit
    from plspm.scheme import Scheme
    frame, config = population_frame(3)
    right = ModelFit(frame, config(PATH), Scheme.PATH, iterations=500, seed=1, factors=None).fit()
    wrong = ModelFit(frame, config(PATH_WITHOUT_02), Scheme.PATH, iterations=500, seed=1, factors=None).fit()
    print("correct model:\n%s\nwithout 0 -> 2:\n%s" % (right, wrong))
    assert right.loc["d_uls", "p.value"] >= 0.10
    assert wrong.loc["d_uls", "p.value"] <= 0.01 and wrong.loc["d_uls", "estimated"] > wrong.loc["d_uls", "hi99"]
