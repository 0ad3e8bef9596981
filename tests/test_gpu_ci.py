"""GPU: the jackknife and the bootstrap confidence intervals (include/plspm_hip.h plspm_jackknife_device / _fetch / _stats,
plspm_bootstrap_intervals; plspm.bootstrap.Bootstrap.intervals, plspm.jackknife.Jackknife).

The jackknife's records are the oracle's fits on the kept rows (rtol 1e-8, atol 1e-11 and identical iteration counts, the project's record bar);
its statistics are the NumPy mirror's on the device's own records (mean, std.error rtol 1e-12; accel atol 1e-12: a fixed-order fp64 sum of
n <= 250 cubes relative to (sum d^2)^1.5 is off by n eps / 6 at most).  Against the ORACLE's leave-one-out fits the acceleration can only agree as
far as the d_g do, which come from estimates that agree to 1e-8: perturbing the oracle's 250 satisfaction records inside the record bar (rtol 1e-8,
atol 1e-11, 20 draws, both configurations below) moves the acceleration by 1.11e-7 at most (max |accel| 0.084), measured on the CPU; the bar is
ten times that.  The intervals are the mirror's (lower / upper rtol 1e-9) and SciPy's (levels, z0 atol 1e-12), and the percentile interval at 0.95
is the summary's two columns bit for bit."""
import os

import numpy as np
import pandas as pd
import pytest

import plspm_oracle as orc
from helpers import GOLDEN, SAT_ADD_ORDER, SAT_PREFIX, assert_close, satisfaction_frame, satisfaction_oracle_inputs
from helpers_ci import intervals as scipy_intervals, jackknife_stats as fsum_jackknife_stats, synthetic_records
from helpers_mga import oracle_record

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-8, 1e-11
ACCEL_PERTURBED = 1.11e-7          # measured on the CPU (module docstring)
ACCEL_BAR = 10 * ACCEL_PERTURBED
SCHEME_ID = {"centroid": 0, "factorial": 1, "path": 2}
METHODS = ("percentile", "basic", "bc", "bca")


def native_model(model, X=None):
    """The handle of `model` (on X; device column p = data column model.mv_order[p])."""
    from plspm import _native
    boff = np.concatenate(([0], np.cumsum([len(b) for b in model.blocks]))).astype(np.int32)
    modes = np.array([0 if m == "A" else 1 for m in model.modes], dtype=np.int32)
    nm = _native.NativeModel(boff, model.C.astype(np.uint8), modes, SCHEME_ID[model.scheme], model.scaled, model.max_iter, model.tol, 0)
    if X is not None:
        nm.upload(X, model.mv_order.astype(np.int32))
    return nm


def sat_model(scheme, scaled, modes="AAAAAA", **kw):
    X, blocks, _ = satisfaction_oracle_inputs()
    return X, orc.Model(blocks, orc.satisfaction_C(), modes, scheme, scaled, **kw)


def check_records(nm, X, model, G):
    n = X.shape[0]
    nm.jackknife(G)
    assert nm.get_option("last_gram_path") == 2
    rows, status, iters = nm.jackknife_fetch(0, G)
    oracle = np.empty_like(rows)
    for g in range(G):
        oracle[g], its = oracle_record(X, model, np.arange(n) % G != g)
        assert status[g] == 0 and iters[g] == its, (g, status[g], iters[g], its)
        assert_close(rows[g], oracle[g], RTOL, ATOL, what="jackknife problem %d of %d" % (g, G))
    return rows, oracle


def check_stats(nm, G, rows, status):
    from plspm.bootstrap import _jackknife_stats
    mean, se, accel, used = nm.jackknife_stats(G)
    ok = status == 0
    assert used == int(ok.sum())
    m_ref, se_ref, a_ref = _jackknife_stats(rows[ok])
    for mine, ref in ((mean, m_ref), (se, se_ref), (accel, a_ref)):
        assert np.array_equal(np.isnan(mine), np.isnan(ref))
    print("jackknife stats G=%d: max rel mean %.3e se %.3e, max abs accel %.3e" % (
        G, np.nanmax(np.abs(mean - m_ref) / np.maximum(np.abs(m_ref), 1e-300)), np.nanmax(np.abs(se - se_ref) / np.maximum(np.abs(se_ref), 1e-300)),
        np.nanmax(np.abs(accel - a_ref))))
    np.testing.assert_allclose(mean, m_ref, rtol=1e-12, atol=0)
    np.testing.assert_allclose(se, se_ref, rtol=1e-12, atol=1e-300)
    np.testing.assert_allclose(accel, a_ref, rtol=0, atol=1e-12)
    return mean, se, accel


# ------------------------------------------------------------------ jackknife records and statistics
@pytest.mark.parametrize("scheme,scaled,modes", [("path", True, "AABAAA"), ("centroid", False, "AAAAAA"), ("path", False, "AAAAAA"), ("centroid", True, "AABAAA")])
def test_satisfaction_jackknife_vs_oracle(scheme, scaled, modes):
    X, model = sat_model(scheme, scaled, modes)
    nm = native_model(model, X)
    for G in (250, 7):                                     # leave-one-out; unequal groups (250 % 7 != 0)
        rows, oracle = check_records(nm, X, model, G)
        mean, se, accel = check_stats(nm, G, rows, np.zeros(G, dtype=np.int32))
        # repeatable bit for bit
        again = nm.jackknife_stats(G)
        for a, b in zip((mean, se, accel), again[:3]):
            assert np.array_equal(a, b, equal_nan=True)
        if G == 250:
            a_orc = fsum_jackknife_stats(oracle)[2]
            assert np.array_equal(np.isnan(accel), np.isnan(a_orc))
            diff = np.nanmax(np.abs(accel - a_orc))
            print("accel against the oracle's leave-one-out fits (%s, scaled %s, %s): max |difference| %.3e (bar %.3e), max |accel| %.3e" % (
                scheme, scaled, modes, diff, ACCEL_BAR, np.nanmax(np.abs(a_orc))))
            assert diff <= ACCEL_BAR


def test_counts_across_two_row_windows():
    C = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0]])
    X, blocks = orc.synth(65600, C, 2, seed=4)
    model = orc.Model(blocks, C, "AAA", "path", True)
    nm = native_model(model, X)
    rows, _ = check_records(nm, X, model, 8)
    check_stats(nm, 8, rows, np.zeros(8, dtype=np.int32))


def test_short_data_set_leave_one_out():
    C = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0]])
    X, blocks = orc.synth(100, C, 3, seed=6)
    model = orc.Model(blocks, C, "AAA", "centroid", True)
    nm = native_model(model, X)
    rows, _ = check_records(nm, X, model, 100)
    check_stats(nm, 100, rows, np.zeros(100, dtype=np.int32))


def test_nothing_converges_nothing_is_used():
    X, model = sat_model("path", True, max_iter=1)
    nm = native_model(model, X)
    nm.jackknife(25)
    _, status, _ = nm.jackknife_fetch(0, 25)
    assert np.all(status != 0)
    mean, se, accel, used = nm.jackknife_stats(25)
    assert used == 0
    assert np.all(np.isnan(mean)) and np.all(np.isnan(se)) and np.all(np.isnan(accel))


def test_jackknife_argument_and_state_errors():
    from plspm import _native
    X, model = sat_model("path", True)
    nm = native_model(model, X)
    with pytest.raises(_native.NativeBackendError, match=r"plspm_jackknife_stats failed \(101\)"):      # PLSPM_E_STATE
        nm.jackknife_stats(250)
    with pytest.raises(_native.NativeBackendError, match=r"plspm_jackknife_fetch failed \(101\)"):
        nm.jackknife_fetch(0, 1)
    for G in (1, 251, 0):
        with pytest.raises(_native.NativeBackendError, match=r"plspm_jackknife_device failed \(100\)"):  # PLSPM_E_ARG
            nm.jackknife(G)
    nm.jackknife(10)
    with pytest.raises(_native.NativeBackendError, match=r"plspm_jackknife_stats failed \(100\)"):
        nm.jackknife_stats(11)
    with pytest.raises(_native.NativeBackendError, match=r"plspm_jackknife_fetch failed \(100\)"):
        nm.jackknife_fetch(5, 6)
    with pytest.raises(_native.NativeBackendError, match=r"plspm_bootstrap_intervals failed \(100\)"):
        nm._check(nm._lib.plspm_bootstrap_intervals(nm._h, None, 10, 0, np.zeros(nm.row_width).ctypes.data, None, 3, 0.95, np.zeros(nm.row_width * 6).ctypes.data, None),
                  "plspm_bootstrap_intervals")
    with pytest.raises(_native.NativeBackendError, match=r"plspm_bootstrap_intervals failed \(101\)"):
        nm.intervals(10, np.zeros(nm.row_width))
    C3 = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0]])
    Xs, blocks3 = orc.synth(40, C3, 2, seed=1)
    model3 = orc.Model(blocks3, C3, "AAA", "path", True)
    small = native_model(model3, Xs[:5])                    # leave-one-out of five rows keeps four; of four rows three
    small.jackknife(5)
    tiny = native_model(model3, Xs[:4])
    with pytest.raises(_native.NativeBackendError, match=r"plspm_jackknife_device failed \(100\)"):
        tiny.jackknife(4)
    nonmetric = _native.NativeModel(nm.block_offset, model.C.astype(np.uint8), np.zeros(6, dtype=np.int32), 2, True, 100, 1e-6, 0, nonmetric=True)
    nonmetric.upload(X, model.mv_order.astype(np.int32))
    with pytest.raises(_native.NativeBackendError, match=r"plspm_jackknife_device failed \(100\)"):
        nonmetric.jackknife(10)


# ------------------------------------------------------------------ intervals on synthetic records
def two_lv_handle():
    C = np.array([[0, 0], [1, 0]])
    model = orc.Model([[0, 1], [2, 3]], C, "AA", "path", True)
    return native_model(model)


def interval_case(B, seed):
    """Records of B replicates whose columns cover the kernel's cases, the estimates and accelerations that go with them."""
    from plspm.bootstrap import _intervals
    nm = two_lv_handle()
    R, stride = nm.row_width, nm.row_stride
    assert R >= 10
    rng = np.random.default_rng(seed)
    rec = synthetic_records(rng, B, R, stride)
    original = rec[:, :R].mean(axis=0) + rng.uniform(-0.4, 0.4, R) * (rec[:, :R].std(axis=0) if B > 1 else 1.0)
    rec[:, 0] = 0.0; original[0] = 0.0                                            # all equal (an absent path)
    rec[:, 1] = rng.integers(0, 3, B) * 0.5 - 0.25; original[1] = 0.3             # heavy ties, three values
    rec[:, 2] = original[2] - 0.5 - np.abs(rec[:, 2])                             # every replicate below the estimate
    rec[:, 3] = original[3] + 0.5 + np.abs(rec[:, 3])                             # ... above
    rec[:, 4] = np.round(rec[:, 4], 1)                                            # ties among a few dozen values
    original[5] = np.nan
    if B >= 40:                                                                   # failed replicates and the NaN padding of a ragged shard are skipped
        rec[3, R] = 1.0; rec[B // 2, R] = 2.0; rec[B - 1, R] = np.nan
        rec[3, :R] = 1e30; rec[B - 1, :R] = -1e30
    status = rec[:, R]
    ok = status == 0
    accel = rng.uniform(-0.05, 0.05, R)
    accel[6] = np.nan
    z0 = _intervals(rec[ok][:, :R], original, None, "percentile", 0.95)[:, 2]
    z = 1.959963984540054                                                         # Phi^-1(0.975)
    if np.isfinite(z0[7]) and np.isfinite(z0[8]):                                 # an adjusted level at position m - 1 / at position 0
        accel[7] = 0.999 / (z0[7] + z); accel[8] = 0.999 / (z0[8] - z)
    return nm, rec, ok, original, accel


def check_intervals(nm, rec, ok, original, accel, level):
    from plspm.bootstrap import _intervals
    B, R = rec.shape[0], nm.row_width
    used_rows = rec[ok][:, :R]
    for method in METHODS:
        out, used = nm.intervals(B, original, method, level, accel if method == "bca" else None)
        mirror = _intervals(used_rows, original, accel, method, level)
        scipy_ref = scipy_intervals(used_rows, original, method, level, accel)
        assert used == int(ok.sum())
        assert np.array_equal(np.isnan(out), np.isnan(mirror)), (method, np.argwhere(np.isnan(out) != np.isnan(mirror)))
        assert np.array_equal(np.isnan(out), np.isnan(scipy_ref)), method
        fin = np.isfinite(mirror[:, 0])
        rel = np.abs(out[fin, :2] - mirror[fin, :2]) / np.maximum(np.abs(mirror[fin, :2]), 1e-300)
        rel[out[fin, :2] == mirror[fin, :2]] = 0.0
        with np.errstate(invalid="ignore"):
            dz = np.abs(out[:, [2, 4, 5]] - scipy_ref[:, [2, 4, 5]])
        dz[out[:, [2, 4, 5]] == scipy_ref[:, [2, 4, 5]]] = 0.0
        print("B=%d m=%d %s level %.2f: lower/upper max rel %.3e, z0/levels max abs vs scipy %.3e" % (
            B, used, method, level, rel.max() if rel.size else 0.0, np.nanmax(dz) if np.isfinite(dz).any() else 0.0))
        np.testing.assert_allclose(out[:, :2], mirror[:, :2], rtol=1e-9, atol=0, err_msg=method)
        np.testing.assert_allclose(out[:, [2, 4, 5]], scipy_ref[:, [2, 4, 5]], rtol=0, atol=1e-12, err_msg=method)
        np.testing.assert_allclose(out[:, 3], mirror[:, 3], rtol=0, atol=0, err_msg=method)
        if method == "bca" and level == 0.95 and np.isfinite(accel[7]) and abs(accel[7]) > 0.1:      # (the accelerations were made for this level)
            assert out[7, 5] == 1.0 and out[7, 1] == used_rows[:, 7].max()
            assert out[8, 4] == 0.0 and out[8, 0] == used_rows[:, 8].min()
        if method in ("bc", "bca"):
            for c in (0, 2, 3):
                assert np.all(np.isnan(out[c, [0, 1, 4, 5]])) and np.isinf(out[c, 2])


def _lds_values():
    from plspm import _native
    return _native.CI_LDS_VALUES


# B: 1, 2, 40; 8,200: beyond the 8,192 values the kernel keeps in registers; the LDS buffer's capacity and one value above it (global scratch slice)
@pytest.mark.parametrize("B", [1, 2, 40, 8200, 16384, 16385])
def test_intervals_on_synthetic_records(B):
    assert _lds_values() == 16384
    nm, rec, ok, original, accel = interval_case(B, seed=B)
    nm.store(rec)
    for level in (0.95, 0.9):
        check_intervals(nm, rec, ok, original, accel, level)
    # percentile at 0.95 = the summary's quantiles, bit for bit
    summary, used = nm.summary(B, original)
    out, used2 = nm.intervals(B, original, "percentile", 0.95)
    assert used == used2
    fin = ~np.isnan(original)
    assert np.array_equal(out[fin, 0].view(np.int64), summary[fin, 3].view(np.int64)) and np.array_equal(out[fin, 1].view(np.int64), summary[fin, 4].view(np.int64))
    assert np.all(np.isnan(out[~fin]))                      # a NaN estimate blanks the interval; the summary's quantiles do not read the estimate
    # ... so every column is compared once more with finite estimates throughout
    finite_original = np.where(fin, original, 0.0)
    summary, used = nm.summary(B, finite_original)
    out, used2 = nm.intervals(B, finite_original, "percentile", 0.95)
    assert used == used2
    assert np.array_equal(out[:, 0].view(np.int64), summary[:, 3].view(np.int64)) and np.array_equal(out[:, 1].view(np.int64), summary[:, 4].view(np.int64))


def test_no_replicate_used_and_one_failed_of_two():
    nm = two_lv_handle()
    R, stride = nm.row_width, nm.row_stride
    rng = np.random.default_rng(2)
    rec = synthetic_records(rng, 2, R, stride)
    original = rec[0, :R].copy() + 0.1
    rec[1, R] = 1.0
    nm.store(rec)
    check_intervals(nm, rec, rec[:, R] == 0, original, np.full(R, 0.01), 0.95)
    rec[0, R] = 3.0
    nm.store(rec)
    for method in METHODS:
        out, used = nm.intervals(2, original, method, 0.95, np.zeros(R))
        assert used == 0 and np.all(np.isnan(out))


def test_intervals_on_an_explicit_device_buffer_with_a_wider_stride():
    """d_rows / stride as plspm_bootstrap_summary: the handle's own records read as records of twice the stride are every other replicate."""
    from plspm.bootstrap import _intervals
    X, model = sat_model("path", True)
    other = native_model(model, X)
    d_rows, _, _ = other.bootstrap_device(64, seed=9)
    rows, status, _ = other.fetch(0, 64)
    orig = rows.mean(axis=0)
    out, used = other.intervals(32, orig, "bc", 0.9, d_rows=d_rows, stride=2 * other.row_stride)
    mirror = _intervals(rows[0::2][status[0::2] == 0], orig, None, "bc", 0.9)
    assert used == int((status[0::2] == 0).sum())
    np.testing.assert_allclose(out, mirror, rtol=1e-9, atol=1e-12)


# ------------------------------------------------------------------ the bootstrap's records survive a jackknife
def test_bootstrap_records_survive_a_jackknife():
    X, model = sat_model("path", True, "AABAAA")
    nm = native_model(model, X)
    fit = nm.fit(want_scores=False)
    original = np.concatenate((fit["weights"], fit["r2"], fit["total"], fit["direct"], fit["loadings"]))
    B = 300
    nm.bootstrap_device(B, seed=21)
    before = nm.fetch(0, B)
    table_before = nm.summary(B, original)
    nm.jackknife(250)
    jack = nm.jackknife_fetch(0, 250)
    after = nm.fetch(0, B)
    table_after = nm.summary(B, original)
    for a, b in zip(before, after):
        assert np.array_equal(a, b, equal_nan=True)
    assert np.array_equal(table_before[0], table_after[0], equal_nan=True) and table_before[1] == table_after[1]
    # the digit planes belong to the call: a second bootstrap gives the first one's rows, and the jackknife's records stay where they are
    nm.bootstrap_device(B, seed=21)
    again = nm.fetch(0, B)
    for a, b in zip(before, again):
        assert np.array_equal(a, b, equal_nan=True)
    assert np.array_equal(nm.summary(B, original)[0], table_before[0], equal_nan=True)
    for a, b in zip(jack, nm.jackknife_fetch(0, 250)):
        assert np.array_equal(a, b, equal_nan=True)
    fresh = native_model(model, X)                          # ... and a jackknife behind a bootstrap is the jackknife of a fresh handle
    fresh.jackknife(250)
    for a, b in zip(jack, fresh.jackknife_fetch(0, 250)):
        assert np.array_equal(a, b, equal_nan=True)


# ------------------------------------------------------------------ host API
def _sat_config():
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


ACCESSORS = ("weights", "r_squared", "total_effects", "paths", "loading")


def test_host_api_intervals_and_jackknife_on_satisfaction():
    from plspm.bootstrap import INTERVAL_COLUMNS, _intervals, _jackknife_stats, _result_frames
    from plspm.jackknife import JACKKNIFE_COLUMNS, Jackknife
    from plspm.plspm import Plspm
    from plspm.scheme import Scheme
    sat, cfg = _sat_config()
    calc = Plspm(sat, cfg, Scheme.PATH, bootstrap=True, bootstrap_iterations=200, seed=1)
    boot = calc.bootstrap()
    reference_frames = {name: getattr(boot, name)().copy() for name in ACCESSORS}
    samples, original = boot.replicates(), boot._original_row
    jack = Jackknife(sat, cfg, Scheme.PATH)
    rows, status, _ = jack.estimates()
    assert jack.used() == 250 and np.all(status == 0)
    mean, se, accel = _jackknife_stats(rows[status == 0])
    accel7 = _jackknife_stats(Jackknife(sat, cfg, Scheme.PATH, groups=7).estimates()[0])[2]
    for method in METHODS:
        for groups in ((None, 7) if method == "bca" else (None,)):
            ci = boot.intervals(method, 0.9, groups=groups)
            assert boot.intervals(method, 0.9, groups=groups) is ci                      # cached
            assert ci.used() == boot.used() and ci.jackknife_used() == ((250 if groups is None else 7) if method == "bca" else None)
            a = (accel if groups is None else accel7) if method == "bca" else None
            table = np.column_stack((original, _intervals(samples, original, a, method, 0.9)))
            expected = _result_frames(boot._cm, boot._native.n_eff, boot._inner_model, table, INTERVAL_COLUMNS)
            for name in ACCESSORS:
                frame, ref = getattr(ci, name)(), reference_frames[name]
                assert list(frame.columns) == INTERVAL_COLUMNS
                assert list(frame.index) == list(ref.index), name
                exp = expected[name].loc[frame.index] if name in ("paths", "r_squared") else expected[name]
                assert list(exp.index) == list(frame.index)
                assert np.array_equal(frame["original"].values, ref["original"].values)
                np.testing.assert_allclose(frame.values, exp.values, rtol=1e-9, atol=1e-12, err_msg="%s %s" % (method, name))
    a_all, a_7 = boot.acceleration()[0], boot.acceleration(7)[0]
    assert np.nanmax(np.abs(a_all - a_7)) > 1e-4
    assert set(boot._accel) == {None, 7}
    np.testing.assert_allclose(a_all, accel, rtol=0, atol=1e-12)
    # the bootstrap's own accessors are what they were
    for name in ACCESSORS:
        pd.testing.assert_frame_equal(getattr(boot, name)(), reference_frames[name])
    # Jackknife frames = the mirror on its own records
    table = np.column_stack((original, mean, 249 * (mean - original), se, accel))
    expected = _result_frames(boot._cm, boot._native.n_eff, boot._inner_model, table, JACKKNIFE_COLUMNS)
    for name in ACCESSORS:
        frame = getattr(jack, name)()
        assert list(frame.columns) == JACKKNIFE_COLUMNS and list(frame.index) == list(reference_frames[name].index), name
        np.testing.assert_allclose(frame.values, expected[name].loc[frame.index].values, rtol=1e-9, atol=1e-12, err_msg=name)
    with pytest.raises(ValueError, match="method must be one of"):
        boot.intervals("student")
    with pytest.raises(ValueError, match="groups must lie"):
        Jackknife(sat, cfg, Scheme.PATH, groups=1)


def test_bca_is_refused_on_a_nonmetric_handle_and_the_other_methods_work():
    import plspm.config as c
    from plspm.bootstrap import _intervals
    from plspm.jackknife import Jackknife
    from plspm.mode import Mode
    from plspm.plspm import Plspm
    from plspm.scale import Scale
    from plspm.scheme import Scheme
    russa = pd.read_csv(os.path.join(GOLDEN, "ref_data", "russa.csv"), index_col=0)
    s = c.Structure(); s.add_path(["AGRI", "IND"], ["POLINS"])
    config = c.Config(s.path(), default_scale=Scale.NUM)
    config.add_lv("POLINS", Mode.A, c.MV("ecks"), c.MV("death"), c.MV("demo"), c.MV("inst"))
    config.add_lv("AGRI", Mode.A, c.MV("gini"), c.MV("rent"), c.MV("farm"))
    config.add_lv("IND", Mode.A, c.MV("gnpr"), c.MV("labo"))
    calc = Plspm(russa, config, Scheme.CENTROID, 100, 0.0000001, bootstrap=True, bootstrap_iterations=200, seed=1)
    boot = calc.bootstrap()
    with pytest.raises(NotImplementedError, match="non-metric"):
        boot.intervals("bca")
    with pytest.raises(NotImplementedError):
        Jackknife(russa, config, Scheme.CENTROID)
    samples, original = boot.replicates(), boot._original_row
    for method in ("percentile", "basic", "bc"):
        ci = boot.intervals(method, 0.95)
        table = _intervals(samples, original, None, method, 0.95)
        frame = ci.weights()
        assert list(frame.index) == list(boot.weights().index) and ci.used() == boot.used()
        inv = boot._cm.inv_index[boot._cm.inv_index >= 0]
        np.testing.assert_allclose(frame.values[:, 1:], table[:boot._cm.P][inv], rtol=1e-9, atol=1e-12, err_msg=method)
    pct = boot.intervals("percentile", 0.95).weights()
    assert np.array_equal(pct["lower"].values, boot.weights()["perc.025"].values) and np.array_equal(pct["upper"].values, boot.weights()["perc.975"].values)
