"""GPU: the prediction kernels (plspm_cv.hip, kernels_cv.h) at the shapes where they take another branch, make another loop trip or leave lanes idle.

  A1  cv_apply_kernel with row groups of 16, 8 and 4 (the expected value asserted from the restated selection rule, tests/helpers_predict.py), folds of one
      row, of less than a tile and of no whole number of tiles, and the PLSPM_E_LIMIT refusal above the LDS bound;
  A2  PLS predictions of Mode-A models with 65 and 96 indicators: the quad solver's records, cv_compose_kernel's lane loops with two trips;
  A3  cv_fold_moments_kernel / cv_train_moments_kernel directly against extended precision, for every residue of C1 % 4, one sweep and several, folds of
      1, 2, 3 and 5 rows, columns whose mean is 1e3 .. 1e4 times their spread;
  A4  cv_threshold_kernel's tie branch (kk < eq), with the keys in LDS and drawn again per pass;
  A5  cv_counts_kernel beyond one 65,536-row count window.

A3's bar.  Unit: n_train sd_p sd_q (sd: the training rows' population sd in extended precision) -- not relative to the element, since covariances near zero are
structurally small.  A plain fp64 NumPy two-pass computation (mean, then the product of the centred rows) of the same quantity on the same inputs is off by
MOMENT_TWO_PASS = 1.41e-15 of that unit at most against np.longdouble over the seven cases below (6.8e-16 at C1 = 4 to 1.41e-15 at C1 = 65: a few ulps of a
diagonal element, which is one unit itself), measured on the CPU and printed again by the test; the bar is ten times that, 1.41e-14, the margin
tests/test_gpu_ci.py gives its measured bar.

A4's search ranges (NumPy Philox only, seed 5, tests/helpers_predict.py _find_cv_tie): at N = 12,288 -- the most rows whose keys stay in LDS -- the first repetition
with two equal keys either side of a fold boundary is 110 (k = 229, rows 5,910 and 8,847), found in 0.13 s inside range(4000); at N = 200,000 repetition 0 has one
(k = 203, rows 87,995 and 128,891), inside range(64)."""
import numpy as np
import pytest

import plspm_oracle as orc
from helpers import assert_close
from helpers_mga import oracle_record
from helpers_predict import (RANK_CACHE_ROWS, CV_MAX_LDS, _find_cv_tie, cv_apply_lds, cv_apply_row_groups, cv_folds, synth_sized,
                             training_moments_longdouble, training_moments_two_pass)
from test_gpu_predict import check_predictions, host_folds, native_model

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-8, 1e-11
MOMENT_TWO_PASS = 1.41e-15         # measured on the CPU (module docstring)
MOMENT_BAR = 10 * MOMENT_TWO_PASS
TWO_LVS = np.array([[0, 0], [1, 0]])
QUAD = 5                           # get_option("last_solver"): solver_quad_kernel


def spread_columns(X, rng):
    """Every column at a scale and an offset of its own, as test_explicit_coefficients_are_applied_as_numpy_applies_them has them."""
    return X * rng.uniform(0.5, 3.0, X.shape[1]) + rng.uniform(-5, 5, X.shape[1])


# ------------------------------------------------------------------ A1: the apply kernel's row groups
def edge_folds(n, nrg, seed):
    """[2, n] fold ids, k = 4.  Repetition 0: fold 0 a single row, fold 1 three rows short of one tile (4 nrg rows), fold 2 two tiles and five rows, fold 3 the
    rest, scattered over the rows; repetition 1: the balanced folds of the host mirror."""
    tile = 4 * nrg
    sizes = [1, tile - 3, 2 * tile + 5]
    assert sum(sizes) + 4 <= n
    ids = np.full(n, 3, dtype=np.uint8)
    ids[:sum(sizes)] = np.repeat(np.arange(3, dtype=np.uint8), sizes)
    first = np.random.default_rng(seed).permutation(ids)
    return np.stack((first, cv_folds(seed, 1, n, 4))), sizes


def apply_case(sizes, nrg, n, reps, k):
    """(X, blocks, folds, coef) of an apply-kernel case.  A fold of one row has error sums of one term each, and an error that happens to be tiny next to the
    P + 1 products behind it is not known to 1e-12 in ANY fp64 evaluation; so the inputs are drawn again (seed + 1000) until the rounding bound of every expected
    sum -- eps sum |c_p x_p| per prediction, carried into the sums -- is below a fifth of the 1e-12 bar.  That is a property of the inputs alone."""
    P, T = sum(sizes), sizes[1]
    folds, fold_sizes = edge_folds(n, nrg, seed=T)
    assert fold_sizes[0] == 1 and fold_sizes[1] < 4 * nrg and fold_sizes[2] % (4 * nrg) != 0
    eps = np.finfo(np.float64).eps / 2
    for seed in range(100 + T, 100 + T + 8000, 1000):
        rng = np.random.default_rng(seed)
        X, blocks = synth_sized(n, TWO_LVS, sizes, seed=T)
        X = spread_columns(X, rng)
        coef = rng.standard_normal((reps * k, T, P + 1))
        bound = 0.0
        for q in range(reps * k):
            r, f = divmod(q, k)
            A = np.column_stack((np.ones(int((folds[r] == f).sum())), X[folds[r] == f]))
            e = X[folds[r] == f][:, sizes[0]:] - A @ coef[q].T
            mag = eps * (np.abs(A) @ np.abs(coef[q]).T)
            bound = max(bound, np.max((2 * np.abs(e) * mag).sum(axis=0) / (e ** 2).sum(axis=0)), np.max(mag.sum(axis=0) / np.abs(e).sum(axis=0)))
        if bound < 2e-13:
            coef[5] = np.nan                                    # a matrix with a NaN covers nothing
            return X, blocks, folds, coef
    raise AssertionError("no well-conditioned inputs for %r" % (sizes,))


@pytest.mark.parametrize("sizes,nrg", [((2, 63), 16), ((2, 64), 16), ((2, 65), 8), ((2, 124), 8), ((136, 64), 8), ((2, 125), 4), ((2, 128), 4), ((2, 129), 4)])
def test_explicit_coefficients_at_every_row_group_size(sizes, nrg):
    """cv_apply_kernel alone against np.column_stack((1, X)) @ coef.T with nrg = 16, 8 and 4: the thread -> (row group, target group) map, cv_group_sum over
    16, 8 and 4 lanes and the tile pitch 4 nrg + 2.  T = 64 | 65 is the switch 16 -> 8 by the thread count; the switch 8 -> 4 comes from the LDS bound before T
    reaches 128 (T = 124 | 125 with two exogenous indicators), so T = 128 | 129 both run with 4; 64 targets of 200 columns run with 8 for the LDS alone.  T = 63,
    65, 125, 129: not divisible by four."""
    P, T = sum(sizes), sizes[1]
    assert cv_apply_row_groups(P, T) == nrg, (P, T, cv_apply_row_groups(P, T))            # the branch this case is here for
    n, reps, k = 300, 2, 4
    X, blocks, folds, coef = apply_case(sizes, nrg, n, reps, k)
    model = orc.Model(blocks, TWO_LVS, "AA", "path", True)
    nm = native_model(model, X)
    nm.cv(reps, k, fold=folds)
    fold, order, offsets = nm.cv_fold_ids(reps, k)
    assert np.array_equal(fold, folds)
    tg = nm.cv_targets()
    assert len(tg) == T and X.shape[1] == P
    sse, sae, sst, rows, psum, pcnt = nm.cv_predict(reps, k, coef=coef, predictions=True)
    Xd = X[:, model.mv_order]
    total, count = np.zeros((n, T)), np.zeros(n, dtype=np.int64)
    worst = 0.0
    for q in range(reps * k):
        r, f = divmod(q, k)
        held = np.flatnonzero(folds[r] == f)
        if q == 5:
            assert rows[q] == 0 and not sse[q].any() and not sae[q].any() and not sst[q].any()
            continue
        pred = np.column_stack((np.ones(len(held)), Xd[held])) @ coef[q].T
        e = Xd[held][:, tg] - pred
        d = Xd[held][:, tg] - np.delete(Xd, held, axis=0)[:, tg].mean(axis=0)
        assert rows[q] == len(held)
        worst = max(worst, np.max(np.abs(sse[q] / (e ** 2).sum(axis=0) - 1)), np.max(np.abs(sae[q] / np.abs(e).sum(axis=0) - 1)))
        assert_close(sse[q], (e ** 2).sum(axis=0), 1e-12, what="sse of problem %d" % q)
        assert_close(sae[q], np.abs(e).sum(axis=0), 1e-12, what="sae of problem %d" % q)
        assert_close(sst[q], (d ** 2).sum(axis=0), RTOL, what="sst of problem %d" % q)
        total[held] += pred; count[held] += 1
    print("P %d T %d nrg %d: max rel sse / sae %.3e, max abs prediction sum %.3e" % (P, T, nrg, worst, np.max(np.abs(psum - total))))
    assert np.array_equal(pcnt, count)
    assert_close(psum, total, 1e-12, 1e-11, what="prediction sums")


def test_a_coefficient_matrix_above_the_lds_bound_is_refused():
    """133 targets of 135 columns: 169,104 bytes with row groups of four, above the 160 KiB -- PLSPM_E_LIMIT, and the handle goes on answering."""
    from plspm import _native
    sizes = (2, 133)
    P, T = sum(sizes), sizes[1]
    assert cv_apply_row_groups(P, T) == 0 and cv_apply_lds(P, T, 4) == 169104 > CV_MAX_LDS
    assert cv_apply_row_groups(131, 129) == 4 and cv_apply_lds(131, 129, 4) == 159904          # (the last size that fits, run above)
    n, reps, k = 300, 1, 3
    X, blocks = synth_sized(n, TWO_LVS, sizes, seed=7)
    X = spread_columns(X, np.random.default_rng(7))
    model = orc.Model(blocks, TWO_LVS, "AA", "path", True)
    nm = native_model(model, X)
    folds = host_folds(3, reps, n, k)
    nm.cv(reps, k, seed=3)
    before = nm.fetch(0, reps * k)
    coef = np.zeros((reps * k, T, P + 1))
    for kw in (dict(coef=coef), dict(technique=0)):
        with pytest.raises(_native.NativeBackendError, match=r"failed \(102\).*133 targets"):      # PLSPM_E_LIMIT
            nm.cv_predict(reps, k, **kw)
    # the call's state is intact: folds, moments and records answer, and a second cross-validation gives the first one's records
    assert np.array_equal(nm.cv_fold_ids(reps, k)[0], folds)
    n_train, mean, _ = nm.cv_moments(reps, k, cross=False)
    Xd = X[:, model.mv_order]
    for f in range(k):
        assert n_train[f] == (folds[0] != f).sum()
        assert_close(mean[f], Xd[folds[0] != f].mean(axis=0), 1e-12, 1e-13, what="training mean")
    assert np.all(before[1] == 0)
    nm.cv(reps, k, seed=3)
    for a, b in zip(before, nm.fetch(0, reps * k)):
        assert np.array_equal(a, b)


# ------------------------------------------------------------------ A2: PLS predictions with 65 .. 128 indicators
@pytest.mark.parametrize("L,per_lv,scaled,nrg", [(8, 12, True, 8), (8, 12, False, 8), (5, 13, True, 16)])
def test_wide_mode_a_models_predict_like_the_helper(L, per_lv, scaled, nrg):
    """96 indicators in 8 LVs (84 targets: nrg = 8) and 65 in 5 (the first size past one lane stride): solver_quad_kernel's records on the training rows, and
    cv_compose_kernel with two trips of every `p = lane; p < P; p += 64` loop (mean, sd0, g, the scaled sum of squares, the intercept's partial sums)."""
    C = orc.chain_C(L)
    n, reps, k = 600, 1, 3
    X, blocks = orc.synth(n, C, per_lv, seed=40 + L)
    X = spread_columns(X, np.random.default_rng(L))
    model = orc.Model(blocks, C, "A" * L, "path", scaled)
    P, T = L * per_lv, (L - 1) * per_lv
    assert 64 < P <= 128 and cv_apply_row_groups(P, T) == nrg
    nm = native_model(model, X)
    nm.cv(reps, k, seed=6)
    assert nm.get_option("last_gram_path") == 2 and nm.get_option("last_solver") == QUAD
    folds = nm.cv_fold_ids(reps, k)[0]
    assert np.array_equal(folds, host_folds(6, reps, n, k)) and len(nm.cv_targets()) == T
    rows, status, iters = nm.fetch(0, reps * k)
    for f in range(k):
        mine, its = oracle_record(X, model, folds[0] != f)
        assert status[f] == 0 and iters[f] == its, (f, status[f], iters[f], its)
        assert_close(rows[f], mine, RTOL, ATOL, what="training fit of problem %d" % f)
    da, _ = check_predictions(nm, X, model, folds, k, "direct")
    ea, _ = check_predictions(nm, X, model, folds, k, "earliest")
    assert np.max(np.abs(da[0]["pred"] - ea[0]["pred"])) > 1e-3        # (a chain: the two techniques are not one)


# ------------------------------------------------------------------ A3: the training moments
MOMENT_SIZES = [(1, 2), (2, 2), (2, 3), (3, 3), (19, 20), (31, 31), (32, 32)]      # C1 = P + 1 = 4, 5, 6, 7, 40, 63, 65
SMALL_FOLDS = (1, 2, 3, 5)


def moment_case(sizes):
    """(X, model, folds [2, n], k): columns whose mean is 1e3 .. 1e4 times their standard deviation, each with a ratio, a sign and a scale of its own; repetition 0
    has folds of 1, 2, 3 and 5 rows (and two large ones), repetition 1 the host mirror's balanced folds."""
    n, k = 200, 6
    P = sum(sizes)
    rng = np.random.default_rng(1000 + P)
    X, blocks = synth_sized(n, TWO_LVS, sizes, seed=P)
    sd = rng.uniform(0.5, 3.0, P)
    ratio = rng.uniform(1e3, 1e4, P) * rng.choice([-1.0, 1.0], P)
    X = (X - X.mean(axis=0)) / X.std(axis=0) * sd + ratio * sd
    ids = np.full(n, 5, dtype=np.uint8)
    ids[:sum(SMALL_FOLDS)] = np.repeat(np.arange(4, dtype=np.uint8), SMALL_FOLDS)
    ids[sum(SMALL_FOLDS):100] = 4
    folds = np.stack((rng.permutation(ids), cv_folds(9, 1, n, k)))
    return X, orc.Model(blocks, TWO_LVS, "AA", "path", True), folds, k


def moment_errors(Xd, train, mean, cross):
    """Largest error of `cross` [P, P] in units of n_train sd_p sd_q against extended precision, and the reference mean."""
    ref_mean, ref_cross, sd = training_moments_longdouble(Xd, train)
    unit = train.sum() * np.outer(sd, sd)
    return float(np.max(np.abs(cross - ref_cross) / unit)), ref_mean


@pytest.mark.parametrize("sizes", MOMENT_SIZES)
def test_training_moments_against_extended_precision(sizes):
    """cv_fold_moments_kernel + cv_train_moments_kernel + plspm_cv_moments: partial 4 x 4 tiles for C1 % 4 = 0, 1, 2, 3, ntile <= 64 (C1 <= 40: one sweep) and
    two or three sweeps (C1 = 63, 65), folds of one, two and three rows (waves without a row) and five, and training = total - fold where the columns' means dwarf
    their spread."""
    P, C1 = sum(sizes), sum(sizes) + 1
    TP = (C1 + 3) // 4
    ntile = TP * (TP + 1) // 2
    assert (ntile <= 64) == (C1 <= 40)
    X, model, folds, k = moment_case(sizes)
    reps, n = folds.shape
    assert sorted(np.bincount(folds[0]))[:4] == list(SMALL_FOLDS)
    nm = native_model(model, X)
    nm.cv(reps, k, fold=folds)
    n_train, mean, cross = nm.cv_moments(reps, k)
    Xd = X[:, model.mv_order]
    iu = np.triu_indices(P)
    worst = worst_numpy = 0.0
    for q in range(reps * k):
        r, f = divmod(q, k)
        train = folds[r] != f
        assert n_train[q] == train.sum()
        full = np.zeros((P, P)); full[iu] = cross[q]
        full = np.triu(full) + np.triu(full, 1).T
        err, ref_mean = moment_errors(Xd, train, mean[q], full)
        assert_close(mean[q], ref_mean, 1e-12, 1e-13, what="training mean of problem %d" % q)
        worst = max(worst, err)
        worst_numpy = max(worst_numpy, moment_errors(Xd, train, *training_moments_two_pass(Xd, train))[0])
    print("C1 %d (%d tiles): cross-products off by %.3e n sd sd at most; NumPy two-pass %.3e; bar %.3e" % (C1, ntile, worst, worst_numpy, MOMENT_BAR))
    assert worst <= MOMENT_BAR


# ------------------------------------------------------------------ A4: key ties at a fold boundary
@pytest.mark.parametrize("n,search,cached", [(12288, 4000, True), (200000, 64, False)])
def test_device_folds_with_key_ties_at_a_fold_boundary(n, search, cached):
    """cv_threshold_kernel's branch kk < eq: two rows share the key of a fold boundary and the row index decides -- with the keys in LDS (N = RANK_CACHE_ROWS) and
    drawn again in every pass."""
    from plspm import _native
    assert (n <= RANK_CACHE_ROWS) == cached
    seed = 5
    found = _find_cv_tie(seed, n, range(search))
    assert found is not None
    rep, k, a, b = found
    C = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0]])
    X, blocks = orc.synth(n, C, 3, seed=8)
    model = orc.Model(blocks, C, "AAA", "path", True)
    nm = native_model(model, X)
    nm.cv(1, k, seed=seed, rep_offset=rep)
    fold = nm.cv_fold_ids(1, k)[0][0]
    mirror = _native.cv_folds(seed, rep, n, k)
    assert a < b and mirror[a] + 1 == mirror[b]
    assert fold[a] + 1 == fold[b]
    assert np.array_equal(fold, mirror) and np.array_equal(mirror, cv_folds(seed, rep, n, k))


# ------------------------------------------------------------------ A5: two count windows
def test_cross_validation_beyond_one_count_window():
    """N = 70,000 > 65,536: the 0/1 counts of cv_counts_kernel span two windows of the fragment layout."""
    C = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0]])
    n, reps, k = 70000, 1, 4
    X, blocks = orc.synth(n, C, 4, seed=11)
    model = orc.Model(blocks, C, "ABA", "path", True)
    nm = native_model(model, X)
    nm.cv(reps, k, seed=99)
    assert nm.get_option("last_gram_path") == 2
    folds = nm.cv_fold_ids(reps, k)[0]
    assert np.array_equal(folds, host_folds(99, reps, n, k))
    for f in range(k):
        assert (folds[0] == f)[:65536].any() and (folds[0] == f)[65536:].any()        # every problem leaves rows out in both windows
    rows, status, iters = nm.fetch(0, reps * k)
    for f in range(k):
        mine, its = oracle_record(X, model, folds[0] != f)
        assert status[f] == 0 and iters[f] == its, (f, status[f], iters[f], its)
        assert_close(rows[f], mine, RTOL, ATOL, what="training fit of problem %d" % f)
    check_predictions(nm, X, model, folds, k, "direct")
