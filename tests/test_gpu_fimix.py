"""GPU: FIMIX-PLS (plspm_fimix_*) against its NumPy mirror (plspm.fimix._fimix) on the same scores and the same initial assignments.

Scores: single-item LVs on standardised columns, so the fit's scores are the columns (up to sign); the mirror reads the scores the device returns.  Cases, the
smallest shapes at which the kernel takes another path:
    chain          2 LVs, N = 40, K in {1, 2}: threads without a row, one regression of one predictor
    planted257     the planted design (helpers_fimix.planted), N = 257 (one thread with a second row), K = 1..4, three starts each: 9 moment entries, one sweep per
                   iteration for K <= 2 (16 entries a sweep), two for K = 3, 4 (8 a sweep)
    planted1000    the same, N = 1,000
    fan_in_11      ten predecessors, beyond the regressions solved in registers; N = 300, K = 2
    dense_7        dense 7-LV DAG, 28 moment entries, N = 300, K = 4: 4 sweeps per iteration (K x entries = 112 accumulators, a chunk holds 32)
    collinear      two identical predecessor columns, K = 2: the minimum-norm route, against the mirror solving by numpy.linalg.pinv
    many           300 problems of `chain` in one call (more workgroups than CUs), K mixed 1 and 2 with kmax = 2, so that NaN slots appear
    satisfaction   the real satisfaction model through ``Fimix``

The bar (the project's rule for derived quantities): ten times the largest difference, on the same inputs, between the fp64 mirror and the mirror in np.longdouble,
and at least 1e-12 max(1, |value|).  Measured on the CPU (tools/fimix_floor.py, the mirrors on the generators' columns), largest |fp64 - longdouble| over a case's problems
at max_iter = 1 / 2 / 5 / 25:
    chain         7.2e-15 / 2.2e-15 / 2.2e-15 / 1.2e-14        planted257     8.6e-14 / 2.2e-13 / 2.5e-13 / 3.5e-13
    planted1000   4.8e-13 / 1.1e-12 / 1.8e-12 / 2.2e-11        fan_in_11      5.7e-15 / 1.1e-13 / 1.7e-13 / 3.3e-14
    dense_7       1.5e-13 / 1.2e-13 / 1.1e-13 / 9.6e-14        collinear      3.3e-14 / 5.2e-15 / 8.7e-14 / 5.4e-14
    many          4.2e-15 / 2.0e-14 / 9.7e-15 / 1.8e-14
(the largest entries are lnL's and H's, sums of N terms, and at t = 25 the parameters of a start that is still far from its optimum.)  On the device the
largest |device - fp64 mirror| of the fixed-iteration runs was 0.91 of its bar.

Converged parity: the stop rule compares |lnL^t - lnL^(t-1)| with tol, so the margin the test demands of the mirror's stopping iteration is ten times the bar OF THAT
DIFFERENCE -- ten times the largest |fp64 - longdouble| of the last two differences, at least 1e-12 max(1, |difference|) -- not of lnL itself: lnL's own floor,
1e-12 |lnL| = 7e-10 (N = 257) or 2.5e-9 (N = 1,000), taken tenfold is of the size of tol = 1e-8, and with the EM's linear rate of about 0.48 on this design no
stopping iteration could clear it.  The starts below stop with |dlnL_T| = 8.3e-9, |dlnL_(T-1)| = 1.7e-8 (N = 257, T = 42) and 7.4e-9, 1.4e-8 (N = 1,000, T = 41).
"""
import functools

import numpy as np
import pytest

import helpers_fimix as hf
from plspm.fimix import STATUS_NOT_CONVERGED, Fimix, _criteria, _fimix, record_width

pytestmark = pytest.mark.gpu
STATUS_SINGULAR = 2
E_ARG, E_STATE, E_LIMIT = 100, 101, 102


def native_model(Y, C):
    """A model of single-item Mode-A blocks on the columns Y (centroid scheme: the fit itself regresses nothing), fitted with scores.  Returns (handle, scores)."""
    from plspm import _native
    L = C.shape[0]
    nm = _native.NativeModel(np.arange(L + 1, dtype=np.int32), C.astype(np.uint8), np.zeros(L, dtype=np.int32), 0, True, 100, 1e-6, 0)
    nm.upload(np.ascontiguousarray(Y))
    fit = nm.fit(want_scores=True)
    return nm, np.array(fit["scores"], dtype=np.float64)


def problems_of(name):
    """(Y, C, [(K, init)], solve) of a case."""
    if name == "chain":
        Y, C, _ = hf.two_segment(hf.tri(2), 40, 2)
        return Y, C, [(1, hf.random_init(40, 1, 0)), (2, hf.random_init(40, 2, 1))], None
    if name in ("planted257", "planted1000"):
        N = int(name[7:])
        Y, C, _ = hf.planted(N)
        return Y, C, [(K, hf.random_init(N, K, 10 * K + s)) for K in (1, 2, 3, 4) for s in range(3)], None
    if name == "fan_in_11":
        Y, C, _ = hf.two_segment(hf.fan_in(11), 300, 5)
        return Y, C, [(2, hf.random_init(300, 2, 7))], None
    if name == "dense_7":
        Y, C, _ = hf.two_segment(hf.dense(7), 300, 3)
        return Y, C, [(4, hf.random_init(300, 4, 8))], None
    if name == "collinear":
        Y, C, _ = hf.collinear(300)
        return Y, C, [(2, hf.random_init(300, 2, 3))], hf.pinv_solve
    if name == "many":          # ten distinct starts per K, cycled over 300 problems
        Y, C, _ = hf.two_segment(hf.tri(2), 40, 2)
        distinct = [(1 + (q % 2), hf.random_init(40, 1 + (q % 2), 100 + q)) for q in range(20)]
        return Y, C, [distinct[q % 20] for q in range(300)], None
    raise KeyError(name)


CASES = ["chain", "planted257", "planted1000", "fan_in_11", "dense_7", "collinear", "many"]


@functools.lru_cache(maxsize=None)
def case(name):
    """The case on the device and its mirrors, computed once: (handle, scores, C, problems, mirrors) -- mirrors[q] = (fp64, longdouble) of problem q, run for 25
    iterations at tol = 0 with the states of iterations 1, 2 and 5 kept."""
    Y, C, problems, solve = problems_of(name)
    nm, scores = native_model(Y, C)
    done, mirrors = {}, []
    for K, init in problems:
        key = (K, init.tobytes())
        if key not in done:
            done[key] = hf.mirror_pair(scores, C, K, init, 25, 0.0, solve=solve, snapshots=(1, 2, 5))
        mirrors.append(done[key])
    return nm, scores, C, problems, mirrors


def run(nm, problems, max_iter, tol, kmax=None):
    k_of = np.array([K for K, _ in problems], dtype=np.int32)
    nm.fimix(k_of, kmax=kmax, init=np.stack([init for _, init in problems]), max_iter=max_iter, tol=tol)
    return nm.fimix_fetch()


@pytest.mark.parametrize("max_iter", hf.ITERATIONS)
@pytest.mark.parametrize("name", CASES)
def test_fixed_iteration_parity(name, max_iter):
    nm, _, _, problems, mirrors = case(name)
    kmax = max(K for K, _ in problems)
    rows, status, iters = run(nm, problems, max_iter, 0.0)
    assert rows.shape == (len(problems), nm.fimix_width(kmax))
    for q, (m64, mld) in enumerate(mirrors):
        want, wld = hf.at(m64, max_iter), hf.at(mld, max_iter)
        if problems[q][0] == 1 and max_iter >= 2:           # one segment: lnL repeats exactly, so even tol = 0 stops at iteration 2 with status 0
            assert want["status"] == wld["status"] == 0 and want["iterations"] == wld["iterations"] == 2
        else:
            assert want["status"] == wld["status"] == STATUS_NOT_CONVERGED and want["iterations"] == wld["iterations"] == max_iter
        assert status[q] == want["status"] and iters[q] == want["iterations"], (q, status[q], iters[q])
        if name == "many" and q >= 20:
            assert np.array_equal(rows[q], rows[q % 20], equal_nan=True)        # the same problem in another workgroup: the same bits
            continue
        r64, rld = hf.records(want, wld, kmax)
        hf.assert_inside(rows[q], r64, rld, "%s problem %d at %d" % (name, q, max_iter))
    if name == "many":
        assert np.isnan(rows[0, 3]) and not np.isnan(rows[1, 3])               # rho of segment 2: a NaN slot where K = 1


@pytest.mark.parametrize("name,seed,expect", [("planted257", 0, 42), ("planted1000", 0, 41)])
def test_converged_parity(name, seed, expect):
    nm, scores, C, _, _ = case(name)
    N, tol = scores.shape[0], 1e-8
    init = hf.random_init(N, 2, seed)
    m64, mld = hf.mirror_pair(scores, C, 2, init, 5000, tol)
    T = m64["iterations"]
    assert m64["status"] == mld["status"] == 0 and mld["iterations"] == T
    # the mirror alone: its stopping iteration is clear of tol by ten times the bar of the difference that is compared with tol (module docstring)
    d64 = np.abs(np.diff(np.array(m64["trace"], dtype=np.float64)))[-2:]
    dld = np.abs(np.diff(np.array(mld["trace"], dtype=np.longdouble)))[-2:]
    dbar = max(10.0 * float(np.max(np.abs(d64 - dld))), hf.FLOOR * max(1.0, float(d64.max())))
    print("T %d, |dlnL_T| %.3g, |dlnL_(T-1)| %.3g, bar of the difference %.3g" % (T, d64[1], d64[0], dbar))
    assert d64[1] <= tol - 10.0 * dbar and d64[0] >= tol + 10.0 * dbar, "mis-specified: the stopping iteration is not clear of tol"
    rows, status, iters = run(nm, [(2, init)], 5000, tol)
    assert status[0] == 0 and iters[0] == T
    r64, rld = hf.records(m64, mld, 2)
    hf.assert_inside(rows[0], r64, rld, "%s converged at %d" % (name, T))
    print("iterations", T, "expected by the docstring", expect)


def test_collapse_gives_singular_and_nan_records():
    nm, scores, C, _, _ = case("planted257")
    N = scores.shape[0]
    empty = np.zeros(N, dtype=np.uint8)                       # valid segments below K = 2 that leave segment 1 empty
    m = _fimix(scores, C, 2, empty, 25, 0.0)
    assert m["status"] == STATUS_SINGULAR and m["iterations"] == 1
    rows, status, iters = run(nm, [(2, empty)], 25, 0.0)
    assert status[0] == STATUS_SINGULAR and iters[0] == 1 and np.all(np.isnan(rows[0]))
    # a column that is an exact linear function of its predecessors: psi is rounding residue
    Y, Ce = hf.exact_function(300)
    ne, se = native_model(Y, Ce)
    init = hf.random_init(300, 2, 3)
    m = _fimix(se, Ce, 2, init, 25, 0.0)
    assert m["status"] == STATUS_SINGULAR
    rows, status, iters = run(ne, [(2, init)], 25, 0.0)
    assert status[0] == STATUS_SINGULAR and iters[0] == m["iterations"] and np.all(np.isnan(rows[0]))


def test_the_same_call_twice_gives_the_same_bits():
    nm, _, _, problems, _ = case("planted1000")
    a = run(nm, problems, 25, 0.0)
    b = run(nm, problems, 25, 0.0)
    assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))
    nm, _, _, problems, _ = case("dense_7")
    a = run(nm, problems, 5, 0.0)
    b = run(nm, problems, 5, 0.0)
    assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))


def test_drawn_starts_equal_the_host_mirror_of_the_draw():
    from plspm import _native
    nm, scores, _, _, _ = case("planted257")
    N = scores.shape[0]
    k_of = np.array([1, 2, 3, 4, 2, 3], dtype=np.int32)
    nm.fimix(k_of, kmax=4, seed=11, start_offset=5, init=None, max_iter=10, tol=0.0)
    drawn = nm.fimix_fetch()
    init = np.stack([_native.fimix_starts(11, 5 + q, N, int(K)) for q, K in enumerate(k_of)])
    nm.fimix(k_of, kmax=4, init=init, max_iter=10, tol=0.0)
    given = nm.fimix_fetch()
    assert np.all(drawn[1][1:] == STATUS_NOT_CONVERGED) and drawn[1][0] == 0
    assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(drawn, given))


def test_posteriors():
    nm, scores, C, problems, mirrors = case("planted257")
    rows, status, _ = run(nm, problems, 25, 0.0)
    for q in (0, 4, 7, 11):                                   # K = 1, 2, 3, 4
        K = problems[q][0]
        m64, mld = mirrors[q]
        P = nm.fimix_posteriors(q)
        assert P.shape == (scores.shape[0], K)
        assert np.all(np.abs(P.sum(axis=1) - 1.0) <= K * 2.0 ** -52)
        pbar = max(10.0 * float(np.max(np.abs(m64["posteriors"] - mld["posteriors"]))), hf.FLOOR)
        gap = float(np.max(np.abs(P - m64["posteriors"])))
        print("K %d: posteriors gap %.3g, bar %.3g" % (K, gap, pbar))
        assert gap <= pbar
        # H and lnL again from the posteriors (lse_i = a_ik - ln P_ik at the row's largest posterior, a from the record's parameters)
        r64, rld = hf.records(m64, mld, 4)
        b = hf.bar(r64, rld)
        with np.errstate(divide="ignore", invalid="ignore"):
            h = -np.where(P > 0, P * np.log(P), 0.0).sum()
        assert abs(h - rows[q, 1]) <= b[1]
        n_dir, n_endo = len(m64["paths"]), len(m64["endo"])
        rho, beta = rows[q, 2:2 + K], rows[q, 6:6 + K * n_dir].reshape(K, n_dir)
        psi = rows[q, 2 + 4 * (1 + n_dir):2 + 4 * (1 + n_dir) + K * n_endo].reshape(K, n_endo)
        a = np.empty_like(P)
        for k in range(K):
            a[:, k] = np.log(rho[k]) - 0.5 * np.log(2 * np.pi * psi[k]).sum()
            for je, j in enumerate(m64["endo"]):
                r = scores[:, j] - sum(beta[k, d] * scores[:, f] for d, (f, t) in enumerate(m64["paths"]) if t == j)
                a[:, k] -= r * r / (2 * psi[k, je])
        top = np.argmax(P, axis=1)
        lnl = (a[np.arange(len(top)), top] - np.log(P[np.arange(len(top)), top])).sum()
        assert abs(lnl - rows[q, 0]) <= b[0]
        # the segments: the mirror's argmax except on rows whose two largest posteriors differ by less than the bar
        if K > 1:
            srt = np.sort(m64["posteriors"], axis=1)
            clear = srt[:, -1] - srt[:, -2] >= pbar
            assert np.array_equal(top[clear], np.argmax(m64["posteriors"], axis=1)[clear])


def test_state_and_arguments():
    from plspm import _native
    lib = _native.load()
    Y, C, _ = hf.planted(257)
    L = C.shape[0]
    nm = _native.NativeModel(np.arange(L + 1, dtype=np.int32), C.astype(np.uint8), np.zeros(L, dtype=np.int32), 0, True, 100, 1e-6, 0)
    nm.upload(np.ascontiguousarray(Y))
    init = hf.random_init(257, 2, 0)[None, :]

    def code(call):
        with pytest.raises(_native.NativeBackendError) as err:
            call()
        return int(str(err.value).split("(")[1].split(")")[0])
    assert code(lambda: nm.fimix([2], init=init)) == E_STATE                       # no fit yet
    assert code(lambda: nm.fimix_fetch()) == E_STATE and code(lambda: nm.fimix_posteriors(0)) == E_STATE
    nm.fit(want_scores=False)
    assert code(lambda: nm.fimix([2], init=init)) == E_STATE                       # a fit without scores leaves none
    nm.fit(want_scores=True)
    assert code(lambda: nm.fimix([0], kmax=1, init=init)) == E_ARG and code(lambda: nm.fimix([17], kmax=17, init=init)) == E_ARG
    assert code(lambda: nm.fimix([3], kmax=2, init=init)) == E_ARG                 # kmax below the largest K
    bad = init.copy(); bad[0, 5] = 2
    assert code(lambda: nm.fimix([2], init=bad)) == E_ARG                          # an initial segment that is not below K
    assert code(lambda: nm.fimix([2], init=init, max_iter=0)) == E_ARG
    nm.fimix([2], init=init, max_iter=3, tol=0.0)
    rows, status, iters = nm.fimix_fetch()
    assert status[0] == STATUS_NOT_CONVERGED and iters[0] == 3
    assert lib.plspm_fimix_fetch(nm._h, 1, 1, None, None, None) == E_ARG           # past the call's problems
    nm.upload(np.ascontiguousarray(Y))                                             # a fresh upload voids the scores and the records
    assert code(lambda: nm.fimix([2], init=init)) == E_STATE
    assert code(lambda: nm.fimix_fetch()) == E_STATE and code(lambda: nm.fimix_posteriors(0)) == E_STATE
    # the route's refusal: 16 segments' moments of 36 latent variables are 16 x 36 x 36 doubles = 162 KiB
    big = hf.tri(36)
    nb = _native.NativeModel(np.arange(37, dtype=np.int32), big.astype(np.uint8), np.zeros(36, dtype=np.int32), 0, True, 100, 1e-6, 0)
    nb.upload(np.ascontiguousarray(hf.two_segment(big, 60, 1)[0]))
    nb.fit(want_scores=True)
    assert code(lambda: nb.fimix([2], kmax=16, init=hf.random_init(60, 2, 0)[None, :])) == E_LIMIT
    nb.fimix([2], kmax=2, init=hf.random_init(60, 2, 0)[None, :], max_iter=2, tol=0.0)
    assert nb.fimix_fetch()[1][0] == STATUS_NOT_CONVERGED


def test_fimix_on_the_satisfaction_model():
    from test_fimix import sat_config
    from plspm.plspm import Plspm
    from plspm.scheme import Scheme
    sat, cfg = sat_config()
    fm = Fimix(sat, cfg, Scheme.PATH, segments=range(1, 4), starts=4, em_iterations=500, em_tolerance=1e-8, seed=7)
    records, status, iters = fm.records()
    assert records.shape == (12, record_width(3, 10, 5)) and fm.seed() == 7
    crit = fm.criteria()
    assert list(crit.columns) == ["lnl", "aic", "aic3", "aic4", "bic", "caic", "hq", "mdl5", "en", "start", "used"] and list(crit.index) == [1, 2, 3]
    # K = 1: no-intercept least squares on the scores
    scores = Plspm(sat, cfg, Scheme.PATH).scores()
    lvs = list(scores.columns)
    N = len(scores)
    assert crit.loc[1, "used"] == 4 and np.all(status[:4] == 0) and np.all(iters[:4] == 2)
    coef, psi, lnl = fm.path_coefficients(1), fm.residual_variances(1), 0.0
    for lv in psi.index:
        preds = [label.split(" -> ")[0] for label in coef.index if label.endswith(" -> " + lv)]
        beta, res = np.linalg.lstsq(scores[preds].values, scores[lv].values, rcond=None)[:2]
        np.testing.assert_allclose([coef.loc["%s -> %s" % (p, lv), "segment.1"] for p in preds], beta, rtol=1e-7, atol=1e-9)
        np.testing.assert_allclose(psi.loc[lv, "segment.1"], res[0] / N, rtol=1e-7)
        lnl += -N / 2 * (np.log(2 * np.pi * res[0] / N) + 1)
    np.testing.assert_allclose(crit.loc[1, "lnl"], lnl, rtol=1e-8)
    assert set(psi.index) <= set(lvs) and np.isnan(crit.loc[1, "en"])
    # the criteria are the formulas on the records
    for ki, K in enumerate((1, 2, 3)):
        assert len(fm.starts(K)) == 4
        if crit.loc[K, "start"] < 0:
            continue
        rec = records[ki * 4 + int(crit.loc[K, "start"])]
        want = _criteria(rec[0], rec[1], N, K, 10, 5)
        for name, value in want.items():
            np.testing.assert_allclose(crit.loc[K, name], value, rtol=1e-14, equal_nan=True)
        ok = status[ki * 4:(ki + 1) * 4] == 0
        assert rec[0] == records[ki * 4:(ki + 1) * 4, 0][ok].max() and crit.loc[K, "used"] == ok.sum() == fm.used()[K]
        sizes = fm.sizes(K)
        assert abs(sizes.sum() - 1.0) <= 1e-12 and np.all(np.diff(sizes.values) <= 0)
        post = fm.posteriors(K)
        assert post.shape == (N, K) and list(post.index) == list(sat.index)
        assert np.array_equal(fm.segments(K).values, np.argmax(post.values, axis=1) + 1)
        np.testing.assert_allclose(post.mean(axis=0).values, sizes.values, atol=1e-3)      # rho^(t+1) against rho^t of a converged run
