"""Shared by the FIMIX-PLS tests (tests/test_fimix.py, tests/test_gpu_fimix.py) and the floor measurement (tools/fimix_floor.py): the generators of the cases, the
NumPy mirror (plspm.fimix._fimix) of one problem in fp64 and in np.longdouble on the same fp64 inputs, and the bar of the comparison."""
import numpy as np

from plspm.fimix import _fimix, _record

FLOOR = 1e-12           # relative to max(1, |value|): lnL and H are sums of N terms
ITERATIONS = (1, 2, 5, 25)
PLANTED_C = np.array([[0, 0, 0, 0], [1, 0, 0, 0], [1, 1, 0, 0], [0, 1, 1, 0]], dtype=np.int64)
PLANTED_BETA = (dict(b01=.7, b02=.1, b12=.6, b13=.2, b23=.6), dict(b01=.1, b02=.6, b12=-.3, b13=.7, b23=-.1))     # 40 % and 60 % of the rows


def tri(L):
    C = np.zeros((L, L), dtype=np.int64)
    for j in range(1, L):
        C[j, j - 1] = 1
    return C


def fan_in(L):
    C = np.zeros((L, L), dtype=np.int64)
    C[L - 1, :L - 1] = 1
    return C


def dense(L):
    return np.tril(np.ones((L, L), dtype=np.int64), -1)


def standardise(X):
    return (X - X.mean(axis=0)) / X.std(axis=0)


def planted(N, seed=1):
    """The planted design: 4 LVs, paths 0->1, 0->2, 1->2, 1->3, 2->3, two segments (the first 40 % of the rows and the rest) with their own coefficients,
    residual sd 0.25, columns standardised.  Returns (Y [N, 4], C, segment [N])."""
    rng = np.random.default_rng(seed)
    n_a = int(round(0.4 * N))
    seg = (np.arange(N) >= n_a).astype(np.int64)
    Y = np.empty((N, 4))
    Y[:, 0] = rng.normal(size=N)
    e = 0.25 * rng.normal(size=(N, 3))
    for s, b in enumerate(PLANTED_BETA):
        r = seg == s
        Y[r, 1] = b["b01"] * Y[r, 0] + e[r, 0]
        Y[r, 2] = b["b02"] * Y[r, 0] + b["b12"] * Y[r, 1] + e[r, 1]
        Y[r, 3] = b["b13"] * Y[r, 1] + b["b23"] * Y[r, 2] + e[r, 2]
    return standardise(Y), PLANTED_C.copy(), seg


def two_segment(C, N, seed, sd=0.5):
    """Any DAG: two segments (40 % / 60 %) with coefficient sets drawn uniformly from (-0.6, 0.6), residual sd `sd`, columns standardised."""
    C = np.asarray(C)
    L = C.shape[0]
    rng = np.random.default_rng(seed)
    n_a = int(round(0.4 * N))
    seg = (np.arange(N) >= n_a).astype(np.int64)
    B = [np.where(C != 0, rng.uniform(-0.6, 0.6, (L, L)), 0.0) for _ in range(2)]
    Y = np.zeros((N, L))
    noise = rng.normal(size=(N, L))
    for j in range(L):
        if not C[j].any():
            Y[:, j] = noise[:, j]
        else:
            for s in range(2):
                r = seg == s
                Y[r, j] = Y[r] @ B[s][j] + sd * noise[r, j]
    return standardise(Y), C.copy(), seg


def collinear(N, seed=4):
    """Three LVs, 0 -> 2 and 1 -> 2, with column 1 a copy of column 0: the regressions of LV 2 take the minimum-norm route."""
    Y, C, seg = two_segment(np.array([[0, 0, 0], [0, 0, 0], [1, 1, 0]]), N, seed)
    Y[:, 1] = Y[:, 0]
    return Y, C, seg


def exact_function(N, seed=6):
    """Three LVs, 0 -> 2 and 1 -> 2, with column 2 an exact linear function of its predecessors: psi is rounding residue and every segment collapses."""
    rng = np.random.default_rng(seed)
    Y = standardise(rng.normal(size=(N, 3)))
    Y[:, 2] = 0.5 * Y[:, 0] - 0.25 * Y[:, 1]
    return Y, np.array([[0, 0, 0], [0, 0, 0], [1, 1, 0]], dtype=np.int64)


def random_init(N, K, seed):
    """A random hard assignment with no empty segment."""
    rng = np.random.default_rng(seed)
    init = rng.integers(0, K, N)
    init[:K] = np.arange(K)
    return init.astype(np.uint8)


def pinv_solve(A, b):
    """numpy.linalg.pinv on the normal equations (fp64 whatever the dtype of A: numpy has no long-double SVD)."""
    return np.linalg.pinv(np.asarray(A, dtype=np.float64), rcond=1e-12, hermitian=True) @ np.asarray(b, dtype=np.float64)


def mirror_pair(Y, C, K, init, max_iter, tol, solve=None, snapshots=()):
    """(fp64 mirror, longdouble mirror) of one problem on the same fp64 scores."""
    Y = np.asarray(Y, dtype=np.float64)
    return (_fimix(Y, C, K, init, max_iter, tol, solve=solve, snapshots=snapshots),
            _fimix(Y.astype(np.longdouble), C, K, init, max_iter, np.longdouble(tol), solve=solve, snapshots=snapshots))


def difference(r64, rld):
    """The largest |fp64 - longdouble| over two records (NaN where both are NaN counts as zero)."""
    d = np.abs(np.asarray(r64, dtype=np.longdouble) - np.asarray(rld, dtype=np.longdouble))
    both_nan = np.isnan(np.asarray(r64, dtype=np.float64)) & np.isnan(np.asarray(rld, dtype=np.float64))
    d = np.where(both_nan, 0, d)
    return float(d.max()) if d.size else 0.0


def bar(r64, rld):
    """Per value: ten times the largest difference between the two mirrors' records, at least FLOOR max(1, |value|)."""
    r64 = np.asarray(r64, dtype=np.float64)
    return np.maximum(10.0 * difference(r64, rld), FLOOR * np.maximum(1.0, np.abs(np.nan_to_num(r64))))


def assert_inside(device, r64, rld, what=""):
    """device record == fp64 mirror's inside the bar; NaN exactly where the mirror has NaN.  Prints the figures first."""
    device, r64 = np.asarray(device, dtype=np.float64), np.asarray(r64, dtype=np.float64)
    b = bar(r64, rld)
    nan = np.isnan(r64)
    gap = np.where(nan, 0.0, np.abs(device - r64))
    print("%s mirror difference %.3g, device gap %.3g, bar %.3g" % (what, difference(r64, rld), float(np.nanmax(gap)) if gap.size else 0.0, float(b.min())))
    assert np.array_equal(np.isnan(device), nan), what
    assert np.all(gap <= b), (what, float(np.nanmax(gap / b)))


def records(m64, mld, kmax):
    return _record(m64, kmax).astype(np.float64), _record(mld, kmax)


def at(mirror, t):
    """What a run of max_iter = t returns, from a longer run of the same problem that kept the state of iteration t (``snapshots``)."""
    return mirror if t >= mirror["iterations"] else mirror["snapshots"][t]
