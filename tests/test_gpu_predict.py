"""GPU: out-of-sample prediction by k-fold cross-validation (include/plspm_hip.h plspm_cv_device / plspm_cv_predict, plspm.predict.PLSpredict).

The training fits are the oracle's on the training rows (rtol 1e-8 and identical iteration counts, the project's record bar), the device's
folds are the host mirror's, the held-out predictions and their error sums are the NumPy restatement's (tests/helpers_predict.py: 1e-7, the
project's score bar, for both techniques and where the sign rule flips a score), explicit coefficient matrices are applied as NumPy applies them,
the linear-model benchmark is lstsq on the raw training rows, problems that do not converge are left out, and a bootstrap on the same handle
is untouched by a prediction call."""
import numpy as np
import pytest

import plspm_oracle as orc
from helpers import SAT_ADD_ORDER, SAT_PREFIX, assert_close, load, satisfaction_frame, satisfaction_oracle_inputs
from helpers_mga import oracle_record
from helpers_predict import cross_validate, cv_folds, exogenous, mean_predictions, metrics, targets

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-8, 1e-11
SCHEME_ID = {"centroid": 0, "factorial": 1, "path": 2}


def native_model(model, X):
    """The handle of `model` on X; device column p = data column model.mv_order[p]."""
    from plspm import _native
    boff = np.concatenate(([0], np.cumsum([len(b) for b in model.blocks]))).astype(np.int32)
    modes = np.array([0 if m == "A" else 1 for m in model.modes], dtype=np.int32)
    nm = _native.NativeModel(boff, model.C.astype(np.uint8), modes, SCHEME_ID[model.scheme], model.scaled, model.max_iter, model.tol, 0)
    nm.upload(X, model.mv_order.astype(np.int32))
    return nm


def host_folds(seed, reps, n, k, rep_offset=0):
    return np.stack([cv_folds(seed, rep_offset + r, n, k) for r in range(reps)])


def check_predictions(nm, X, model, folds, k, technique, tol=1e-7):
    """cv_predict of the handle's last cv call against the restatement: per-problem sums, rows, and the averaged predictions."""
    reps, n = folds.shape
    problems = cross_validate(X, model, folds, k, technique)
    sse, sae, sst, rows, psum, pcnt = nm.cv_predict(reps, k, ("direct", "earliest").index(technique), predictions=True)
    for q, p in enumerate(problems):
        if p["pred"] is None:
            assert rows[q] == 0 and not sse[q].any() and not sae[q].any() and not sst[q].any(), q
            continue
        assert rows[q] == len(p["rows"]), q
        print("problem %d: max rel sse %.3e sae %.3e sst %.3e" % (q, np.max(np.abs(sse[q] / p["sse"] - 1)), np.max(np.abs(sae[q] / p["sae"] - 1)), np.max(np.abs(sst[q] / p["sst"] - 1))))
        assert_close(sse[q], p["sse"], RTOL, what="sse of problem %d" % q)
        assert_close(sae[q], p["sae"], RTOL, what="sae of problem %d" % q)
        assert_close(sst[q], p["sst"], RTOL, what="sst of problem %d" % q)
    expected = mean_predictions(problems, n)
    with np.errstate(invalid="ignore", divide="ignore"):
        mine = np.where(pcnt[:, None] > 0, psum / pcnt[:, None], np.nan)
    count = np.zeros(n, dtype=np.int64)
    for p in problems:
        if p["pred"] is not None:
            count[p["rows"]] += 1
    assert np.array_equal(pcnt, count)
    ok = count > 0
    print("predictions: max abs difference %.3e" % np.max(np.abs(mine[ok] - expected[ok])))
    assert_close(mine[ok], expected[ok], tol, tol, what="predictions (%s)" % technique)
    return problems, (sse, sae, sst, rows)


def sat_model(scheme, scaled, modes="AAAAAA"):
    X, blocks, _ = satisfaction_oracle_inputs()
    return X, orc.Model(blocks, orc.satisfaction_C(), modes, scheme, scaled)


# ------------------------------------------------------------------ the training fits and the folds
@pytest.mark.parametrize("scheme", ["path", "centroid"])
@pytest.mark.parametrize("scaled", [False, True])
def test_explicit_folds_records_vs_oracle(scheme, scaled):
    X, model = sat_model(scheme, scaled, "AABAAA")
    nm = native_model(model, X)
    reps, k = 2, 5
    folds = host_folds(13, reps, X.shape[0], k)
    nm.cv(reps, k, fold=folds)
    assert nm.get_option("last_gram_path") == 2
    rows, status, iters = nm.fetch(0, reps * k)
    for r in range(reps):
        for f in range(k):
            mine, its = oracle_record(X, model, folds[r] != f)
            q = r * k + f
            assert status[q] == 0 and iters[q] == its, (q, iters[q], its)
            assert_close(rows[q], mine, RTOL, ATOL, what="training fit of problem %d" % q)


@pytest.mark.parametrize("n,k,reps,offset", [(250, 10, 3, 0), (2003, 7, 4, 5), (20000, 256, 2, 2 ** 33), (300, 2, 2, 1)])
def test_device_folds_equal_the_host_mirror(n, k, reps, offset):
    from plspm import _native
    C = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0]])
    X, blocks = orc.synth(n, C, 3, seed=8)
    model = orc.Model(blocks, C, "AAA", "path", True)
    nm = native_model(model, X)
    nm.cv(reps, k, seed=77, rep_offset=offset)
    fold, order, offsets = nm.cv_fold_ids(reps, k)
    for r in range(reps):
        mirror = _native.cv_folds(77, offset + r, n, k)
        assert np.array_equal(fold[r], mirror)
        assert np.array_equal(mirror, cv_folds(77, offset + r, n, k))
        assert offsets[r, 0] == 0 and offsets[r, k] == n
        for f in range(k):
            assert np.array_equal(order[r, offsets[r, f]:offsets[r, f + 1]], np.flatnonzero(mirror == f))
    # the records of drawn folds are those of the same folds handed in
    a = nm.fetch(0, reps * k)
    nm.cv(reps, k, fold=fold)
    b = nm.fetch(0, reps * k)
    for x, y in zip(a, b):
        assert np.array_equal(x, y, equal_nan=True)


@pytest.mark.parametrize("k", [2, 9])
def test_device_folds_and_count_rows_with_a_tail_piece(k):
    """N = 37: two whole 16-row pieces and a tail of five rows; reps * k = 6 and 27 problems: a ragged last group of eight.  The folds are the host mirror's, the
    records those of the same folds handed in, and the first and the last problem the oracle's fits on their training rows."""
    from plspm import _native
    n, reps, seed = 37, 3, 19
    C = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0]])
    X, blocks = orc.synth(n, C, 2, seed=14)
    model = orc.Model(blocks, C, "AAA", "path", True)
    nm = native_model(model, X)
    mirror = np.stack([_native.cv_folds(seed, r, n, k) for r in range(reps)])
    assert all(n - np.bincount(mirror[r], minlength=k).max() >= 4 and np.bincount(mirror[r], minlength=k).min() >= 1 for r in range(reps))
    nm.cv(reps, k, seed=seed)
    assert np.array_equal(nm.cv_fold_ids(reps, k)[0], mirror)
    a = nm.fetch(0, reps * k)
    nm.cv(reps, k, fold=mirror)
    b = nm.fetch(0, reps * k)
    for x, y in zip(a, b):
        assert np.array_equal(x, y, equal_nan=True)
    rows, status, iters = a
    for q in (0, reps * k - 1):
        mine, its = oracle_record(X, model, mirror[q // k] != q % k)
        assert status[q] == 0 and iters[q] == its, (q, status[q], iters[q], its)
        assert_close(rows[q], mine, RTOL, ATOL, what="training fit of problem %d" % q)


# ------------------------------------------------------------------ predictions and error sums
@pytest.mark.parametrize("scheme,scaled,modes", [("path", False, "AAAAAA"), ("path", True, "AABAAA"), ("centroid", True, "AAAAAA"), ("centroid", False, "AABAAA")])
def test_satisfaction_predictions_vs_helper(scheme, scaled, modes):
    X, model = sat_model(scheme, scaled, modes)
    nm = native_model(model, X)
    reps, k = 2, 5
    nm.cv(reps, k, seed=3)
    folds = nm.cv_fold_ids(reps, k)[0]
    assert np.array_equal(folds, host_folds(3, reps, X.shape[0], k))
    da, _ = check_predictions(nm, X, model, folds, k, "direct")
    ea, _ = check_predictions(nm, X, model, folds, k, "earliest")
    # EXPE's only predecessor has none itself: both techniques agree on its indicators; QUAL ... LOY hang on predicted scores and differ
    n_expe = len(model.blocks[1])
    assert np.allclose(da[0]["pred"][:, :n_expe], ea[0]["pred"][:, :n_expe], rtol=1e-12, atol=1e-12)
    assert np.max(np.abs(da[0]["pred"][:, n_expe:] - ea[0]["pred"][:, n_expe:])) > 1e-3


def test_synth2000_predictions_metrics_and_benchmark():
    X, blocks = orc.synth(2000, orc.satisfaction_C(), 10, seed=0)
    model = orc.Model(blocks, orc.satisfaction_C(), "AAAAAA", "path", True)
    nm = native_model(model, X)
    reps, k = 2, 4
    nm.cv(reps, k, seed=11)
    folds = nm.cv_fold_ids(reps, k)[0]
    problems, (sse, sae, sst, rows) = check_predictions(nm, X, model, folds, k, "direct")
    # the benchmark: coefficients from the device's training moments against lstsq on the raw training rows, scored by the same kernel
    from plspm.predict import linear_model_coefficients
    n_train, mean, cross = nm.cv_moments(reps, k)
    tg_dev, P = nm.cv_targets(), X.shape[1]
    assert np.array_equal(model.mv_order[tg_dev], targets(model))
    for q, p in enumerate(problems):
        train = np.ones(2000, dtype=bool); train[p["rows"]] = False
        assert n_train[q] == train.sum()
        assert_close(mean[q], X[train][:, model.mv_order].mean(axis=0), 1e-12, 1e-13, what="training mean")
    ex_dev = [int(np.flatnonzero(model.mv_order == c)[0]) for c in exogenous(model)]
    coef = linear_model_coefficients(n_train, mean, cross, ex_dev, tg_dev, P)
    lm = nm.cv_predict(reps, k, coef=coef, predictions=True)
    expected = mean_predictions(problems, 2000, "lm")
    mine = lm[4] / lm[5][:, None]
    print("benchmark predictions: max abs difference %.3e" % np.max(np.abs(mine - expected)))
    assert_close(mine, expected, 1e-7, 1e-7, what="benchmark predictions")
    for q, p in enumerate(problems):
        assert_close(lm[0][q], p["lm_sse"], 1e-7, what="benchmark sse"); assert_close(lm[1][q], p["lm_sae"], 1e-7, what="benchmark sae")
        assert_close(lm[2][q], p["sst"], RTOL, what="benchmark sst")
    m, _ = metrics(problems)
    total = rows.sum()
    assert_close(np.sqrt(sse.sum(axis=0) / total), m["rmse"], RTOL, what="rmse")
    assert_close(1 - lm[0].sum(axis=0) / lm[2].sum(axis=0), m["lm.q2_predict"], 1e-7, 1e-9, what="lm q2")


def test_explicit_coefficients_are_applied_as_numpy_applies_them():
    rng = np.random.default_rng(5)
    X, blocks = orc.synth(1500, orc.chain_C(5), 4, seed=3)
    X = X * rng.uniform(0.5, 3.0, X.shape[1]) + rng.uniform(-5, 5, X.shape[1])
    model = orc.Model(blocks, orc.chain_C(5), "AAAAA", "path", True)
    nm = native_model(model, X)
    reps, k = 3, 6
    nm.cv(reps, k, seed=1)
    fold, order, offsets = nm.cv_fold_ids(reps, k)
    tg = nm.cv_targets()
    P, T = X.shape[1], len(tg)
    coef = rng.standard_normal((reps * k, T, P + 1))
    coef[4] = np.nan; coef[7, 2, 5] = np.nan                    # matrices with a NaN cover nothing
    sse, sae, sst, rows, psum, pcnt = nm.cv_predict(reps, k, coef=coef, predictions=True)
    Xd = X[:, model.mv_order]
    total, count = np.zeros((1500, T)), np.zeros(1500, dtype=np.int64)
    for q in range(reps * k):
        r, f = divmod(q, k)
        held = np.flatnonzero(fold[r] == f)
        if q in (4, 7):
            assert rows[q] == 0 and not sse[q].any() and not sae[q].any() and not sst[q].any()
            continue
        pred = np.column_stack((np.ones(len(held)), Xd[held])) @ coef[q].T
        e = Xd[held][:, tg] - pred
        assert rows[q] == len(held)
        assert_close(sse[q], (e ** 2).sum(axis=0), 1e-12, what="sse"); assert_close(sae[q], np.abs(e).sum(axis=0), 1e-12, what="sae")
        total[held] += pred; count[held] += 1
    assert np.array_equal(pcnt, count)
    assert_close(psum, total, 1e-12, 1e-11, what="prediction sums")


def test_chain_model_earliest_differs_from_direct_and_star_model_does_not():
    X, blocks = orc.synth(1200, orc.chain_C(6), 3, seed=9)
    model = orc.Model(blocks, orc.chain_C(6), "AAAAAA", "factorial", False)
    nm = native_model(model, X)
    nm.cv(1, 3, seed=2)
    folds = nm.cv_fold_ids(1, 3)[0]
    da, _ = check_predictions(nm, X, model, folds, 3, "direct")
    ea, _ = check_predictions(nm, X, model, folds, 3, "earliest")
    assert np.max(np.abs(da[0]["pred"] - ea[0]["pred"])) > 1e-3
    # every endogenous LV has only exogenous predecessors: the two techniques are one
    C = np.array([[0, 0, 0, 0], [0, 0, 0, 0], [1, 1, 0, 0], [1, 1, 0, 0]])
    X, blocks = orc.synth(900, C, 3, seed=4)
    model = orc.Model(blocks, C, "AAAA", "path", True)
    nm = native_model(model, X)
    nm.cv(2, 3, seed=2)
    a = nm.cv_predict(2, 3, 0, predictions=True)
    b = nm.cv_predict(2, 3, 1, predictions=True)
    for x, y in zip(a[:4], b[:4]):
        assert np.array_equal(x, y)
    assert_close(a[4], b[4], 1e-13, 1e-13, what="DA = EA")
    check_predictions(nm, X, model, nm.cv_fold_ids(2, 3)[0], 3, "earliest")


def test_a_flipped_score_predicts_like_the_helper():
    """The sign-rule construction of the golden case g5: the fit flips a score (the record's weights are not sign-corrected, its loadings and
    paths are) -- confirmed on the CPU with the restatement before the device is asked."""
    g5 = load("g5_sign_rule")
    X = g5["X"]
    model = orc.Model([np.arange(0, 2), np.arange(2, 7), np.arange(7, 11)], g5["C"], "AAA", "centroid", True)
    k = 4
    folds = host_folds(21, 2, X.shape[0], k)
    problems = cross_validate(X, model, folds, k, "direct")
    assert any(p["sign"] is not None and (p["sign"] < 0).any() for p in problems), "no training fit of this case flips a score"
    nm = native_model(model, X)
    nm.cv(2, k, seed=21)
    assert np.array_equal(nm.cv_fold_ids(2, k)[0], folds)
    check_predictions(nm, X, model, folds, k, "direct")
    check_predictions(nm, X, model, folds, k, "earliest")


def test_problems_that_do_not_converge_are_left_out():
    X, _ = sat_model("centroid", True, "BBBBBB")
    reps, k = 3, 5
    folds = host_folds(5, reps, X.shape[0], k)
    # the iteration limit: chosen on the CPU so that at least one training fit fails and fewer than half do
    full = orc.Model(satisfaction_oracle_inputs()[1], orc.satisfaction_C(), "BBBBBB", "centroid", True)
    its = sorted(p["iterations"] for p in cross_validate(X, full, folds, k))
    limit = its[-1] - 1
    failing = sum(i > limit for i in its)
    assert 1 <= failing < len(its) / 2, its
    model = orc.Model(full.blocks, full.C, full.modes, "centroid", True, max_iter=limit)
    nm = native_model(model, X)
    nm.cv(reps, k, fold=folds)
    status = nm.fetch(0, reps * k)[1]
    assert int((status == 1).sum()) == failing and int((status == 0).sum()) == reps * k - failing
    problems, (sse, sae, sst, rows) = check_predictions(nm, X, model, folds, k, "direct")
    assert int((rows == 0).sum()) == failing
    _, (used, covered) = metrics(problems)
    assert used == reps * k - failing and covered == rows.sum()


def test_bootstrap_rows_are_unchanged_by_a_prediction_call():
    X, blocks = orc.synth(10000, orc.satisfaction_C(), 10, seed=0)
    model = orc.Model(blocks, orc.satisfaction_C(), "AAAAAA", "path", True)
    nm = native_model(model, X)
    before = nm.bootstrap(64, seed=3)
    nm.cv(2, 10, seed=1)
    first = nm.cv_predict(2, 10)
    after = nm.bootstrap(64, seed=3)
    for x, y in zip(before, after):
        assert np.array_equal(x, y)
    from plspm import _native
    with pytest.raises(_native.NativeBackendError, match="replaced"):
        nm.cv_predict(2, 10)                                   # the bootstrap took the records
    nm.cv(2, 10, seed=1)
    for x, y in zip(first[:4], nm.cv_predict(2, 10)[:4]):
        assert np.array_equal(x, y)


def test_handles_outside_the_scope_are_refused():
    from plspm import _native
    X, blocks = orc.synth(500, orc.satisfaction_C(), 4, seed=3)
    model = orc.Model(blocks, orc.satisfaction_C(), "AAAAAA", "path", True)
    boff = np.concatenate(([0], np.cumsum([len(b) for b in model.blocks]))).astype(np.int32)
    nm = _native.NativeModel(boff, model.C.astype(np.uint8), np.zeros(6, dtype=np.int32), 2, True, 100, 1e-6, 0, nonmetric=True)
    nm.upload(X)
    with pytest.raises(_native.NativeBackendError, match="plain metric"):
        nm.cv(2, 5, 1)
    ind = np.full(24, -1, dtype=np.int32); ind[3] = 24
    nm1 = _native.NativeModel(boff, model.C.astype(np.uint8), np.zeros(6, dtype=np.int32), 2, True, 100, 1e-6, 0, missing=ind)
    nm1.upload(np.column_stack((X, np.zeros(500))))
    with pytest.raises(_native.NativeBackendError, match="plain metric"):
        nm1.cv(2, 5, 1)
    # a two-stage (higher-order construct) pair: neither handle takes a cross-validation
    from test_gpu_hoc import handles
    first, second, *_ = handles("path_B")
    first.attach_second_stage(second, [0, 1, 2, 4, 5, 6])
    with pytest.raises(_native.NativeBackendError, match="two-stage pair"):
        first.cv(2, 5, 1)
    with pytest.raises(_native.NativeBackendError):
        second.cv(2, 5, 1)                                     # (holds no data of its own)
    nm2 = native_model(model, X)
    for reps, k in ((0, 5), (2, 1), (2, 257)):
        with pytest.raises(_native.NativeBackendError, match="bad arguments"):
            nm2.cv(reps, k, 1)
    with pytest.raises(_native.NativeBackendError, match="four rows"):
        native_model(model, X[:5]).cv(1, 3, 1)
    bad = np.zeros((1, 500), dtype=np.uint8); bad[0, :100] = 5
    with pytest.raises(_native.NativeBackendError, match="not below k"):
        nm2.cv(1, 5, fold=bad)
    bad[0, :100] = 2
    with pytest.raises(_native.NativeBackendError, match="empty"):
        nm2.cv(1, 5, fold=bad)
    with pytest.raises(_native.NativeBackendError, match="no cross-validation"):
        nm2.cv_predict(1, 5)


# ------------------------------------------------------------------ the API
def _sat_config(scaled=False, mode=None):
    import plspm.config as c
    from plspm.mode import Mode
    mode = mode or Mode.A
    sat = satisfaction_frame()
    s = c.Structure()
    s.add_path(["IMAG"], ["EXPE", "SAT", "LOY"]); s.add_path(["EXPE"], ["QUAL", "VAL", "SAT"])
    s.add_path(["QUAL"], ["VAL", "SAT"]); s.add_path(["VAL"], ["SAT"]); s.add_path(["SAT"], ["LOY"])
    cfg = c.Config(s.path(), scaled=scaled)
    for lv in SAT_ADD_ORDER:
        cfg.add_lv_with_columns_named(lv, mode, sat, SAT_PREFIX[lv])
    return sat, cfg


@pytest.mark.parametrize("technique", ["direct", "earliest"])
def test_plspredict_frames_equal_the_helper(technique):
    from plspm.predict import PLSpredict
    from plspm.scheme import Scheme
    sat, cfg = _sat_config()
    res = PLSpredict(sat, cfg, Scheme.PATH, folds=5, repetitions=3, technique=technique, seed=17)
    X, model = sat_model("path", False)
    folds = res.folds()
    assert res.seed() == 17 and np.array_equal(folds, host_folds(17, 3, X.shape[0], 5))
    problems = cross_validate(X, model, folds, 5, technique)
    m, used = metrics(problems)
    assert res.used() == used == (15, 3 * X.shape[0])
    frame = res.metrics()
    assert list(frame.columns) == ["rmse", "mae", "q2_predict", "lm.rmse", "lm.mae", "lm.q2_predict"]
    # the frame's rows are the targets in device column order: the blocks of EXPE, QUAL, VAL, SAT, LOY
    cols = satisfaction_oracle_inputs()[2]
    names = [cols[p] for p in targets(model)]
    assert list(frame.index) == names and list(res.predictions().columns) == names
    for col in frame.columns:
        print("%s: max rel difference %.3e" % (col, np.max(np.abs(frame[col].values / m[col] - 1))))
        assert_close(frame[col].values, m[col], 1e-7, 1e-9, what=col)
    assert_close(res.predictions().values, mean_predictions(problems, X.shape[0]), 1e-7, 1e-7, what="predictions")
    assert_close(res.residuals().values, sat[names].values - res.predictions().values, 1e-13, 1e-13, what="residuals")
    rows, status, iters = res.records()
    assert rows.shape[0] == 15 and np.all(status == 0)
    assert np.all(frame["q2_predict"] < 1) and np.all(frame["rmse"] > 0)


@pytest.mark.parametrize("technique", ["direct", "earliest"])
def test_plspredict_leaves_out_the_problems_that_do_not_converge(technique, monkeypatch):
    """PLSpredict itself with training fits that fail: `used()`, every column of `metrics()` (the benchmark's are pooled over the same used
    problems) and `predictions()` (a row's average runs over the repetitions whose problem for it was used) equal the restatement's with
    those problems excluded.  The iteration limit is chosen on the CPU with the oracle: at least one training fit fails and fewer than half do,
    and the whole-sample fit that PLSpredict starts with still converges."""
    import plspm.predict as predict
    from plspm.mode import Mode
    from plspm.scheme import Scheme
    X, _ = sat_model("centroid", True, "BBBBBB")
    n, reps, k, seed = X.shape[0], 3, 5, 5
    folds = host_folds(seed, reps, n, k)
    blocks = satisfaction_oracle_inputs()[1]
    free = orc.Model(blocks, orc.satisfaction_C(), "BBBBBB", "centroid", True)
    its = sorted(p["iterations"] for p in cross_validate(X, free, folds, k))
    limit = its[-1] - 1
    failing = sum(i > limit for i in its)
    assert 1 <= failing < len(its) / 2, its
    assert orc.fit(X, free, orc.correction(n))["iterations"] <= limit
    model = orc.Model(blocks, orc.satisfaction_C(), "BBBBBB", "centroid", True, max_iter=limit)
    problems = cross_validate(X, model, folds, k, technique)
    m, used = metrics(problems)
    assert used[0] == reps * k - failing
    monkeypatch.setattr(predict, "MIN_ITERATIONS", 1)
    sat, cfg = _sat_config(scaled=True, mode=Mode.B)
    res = predict.PLSpredict(sat, cfg, Scheme.CENTROID, iterations=limit, folds=k, repetitions=reps, technique=technique, seed=seed)
    assert np.array_equal(res.folds(), folds)
    status = res.records()[1]
    assert [q for q in range(reps * k) if status[q] != 0] == [q for q, p in enumerate(problems) if p["pred"] is None]
    print("used", res.used(), "expected", used)
    assert res.used() == used
    frame = res.metrics()
    for col in ("rmse", "mae", "q2_predict", "lm.rmse", "lm.mae", "lm.q2_predict"):
        print("%s: max rel difference %.3e" % (col, np.max(np.abs(frame[col].values / m[col] - 1))))
        assert_close(frame[col].values, m[col], 1e-7, 1e-9, what=col)
    # the benchmark's columns are NOT those of all fifteen problems
    everything, _ = metrics(cross_validate(X, free, folds, k, technique))
    assert np.max(np.abs(everything["lm.rmse"] / m["lm.rmse"] - 1)) > 1e-6
    expected = mean_predictions(problems, n)
    assert not np.isnan(expected).any()                        # every row is still covered by another repetition
    print("predictions: max abs difference %.3e" % np.max(np.abs(res.predictions().values - expected)))
    assert_close(res.predictions().values, expected, 1e-7, 1e-7, what="predictions")
    # the rows of a failed problem are averaged over fewer repetitions than the others
    count = np.zeros(n, dtype=np.int64)
    for p in problems:
        if p["pred"] is not None:
            count[p["rows"]] += 1
    assert np.array_equal(res.raw["pred_cnt"], count) and count.min() < reps and count.max() == reps
