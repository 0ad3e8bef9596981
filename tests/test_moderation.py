"""CPU: the host surface of the moderation analysis -- the NumPy mirror of the kernels (plspm.moderation._moderation) against a closed form, the portable part
of the kernels (csrc/moderation_core.h: the terms' lists, the plan, the second stage) as a stand-alone host program under AddressSanitizer and
UndefinedBehaviorSanitizer, the bootstrap's draws restated in NumPy, the declarations of the new C-ABI symbols, and the host errors that need no device.

The closed form: three single-item blocks, x_j = 0.4 y_a + 0.3 y_b + 0.25 y_a y_b with y the standardised x_a, x_b.  The score y_j is x_j standardised, so the
stage-2 regression is exact: on the standardised regressors direct2 = (0.4, 0.3) / sd(x_j), interaction = 0.25 sd(z) / sd(x_j), the slopes their sum and
difference and R2 = 1.  (With R2 = 1 the f2 divides by zero up to rounding: it is not compared, and the status may be 3.)"""
import fnmatch
import os
import re
import subprocess

import numpy as np
import pytest

from helpers_moderation import SAT_TERMS, core_inputs, fan_in, needed_lvs, philox_draws, planted, sum_list
from plspm import _native
from plspm.moderation import MAX_TERMS, _check_terms, _moderation

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tests", "moderation_host")
NEW_SYMBOLS = ("plspm_moderation_enable", "plspm_moderation_width", "plspm_moderation_fit", "plspm_moderation_fetch", "plspm_moderation_summary",
               "plspm_moderation_intervals")
SAT_C = np.array([[0, 0, 0, 0, 0, 0], [1, 0, 0, 0, 0, 0], [0, 1, 0, 0, 0, 0], [0, 1, 1, 0, 0, 0], [1, 1, 1, 1, 0, 0], [1, 0, 0, 0, 1, 0]])


def singles(L):
    return [np.array([l]) for l in range(L)]


def closed_form_data(dtype, n=200, seed=3):
    rng = np.random.default_rng(seed)
    xa, xb = rng.standard_normal(n), rng.standard_normal(n) + 0.3 * rng.standard_normal(n)
    xa, xb = xa.astype(dtype), (xb + 0.5 * xa).astype(dtype)
    std = lambda x: (x - x.mean()) / np.sqrt(((x - x.mean()) ** 2).mean())
    ya, yb = std(xa), std(xb)
    dt = np.dtype(dtype).type
    z = ya * yb
    xj = dt(4) / dt(10) * ya + dt(3) / dt(10) * yb + dt(25) / dt(100) * z
    return np.column_stack((3 * xa + 1, xb - 2, xj)), z, xj


@pytest.mark.parametrize("dtype", [np.float64, np.longdouble])
def test_closed_form(dtype):
    dt = np.dtype(dtype).type
    X, z, xj = closed_form_data(dtype)
    out = _moderation(X, None, np.ones(3), np.ones(3), singles(3), "AAA", fan_in(3), [(0, 1, 2)], dtype)
    assert out["record"].dtype == np.dtype(dtype) and out["pivots_pass"] and out["status"] in (0, 3)
    assert out["paths"] == [(0, 2), (1, 2)] and out["terms"] == [(0, 1, 2)]
    sd = lambda x: np.sqrt(((x - x.mean()) ** 2).mean())
    np.testing.assert_allclose(out["direct2"], [dt(4) / dt(10) / sd(xj), dt(3) / dt(10) / sd(xj)], rtol=1e-12)
    np.testing.assert_allclose(out["interaction"], [dt(25) / dt(100) * sd(z) / sd(xj)], rtol=1e-12)
    np.testing.assert_allclose(out["product_sd"], [sd(z)], rtol=1e-12)
    np.testing.assert_allclose(out["slope_low"], out["direct2"][0] - out["interaction"], rtol=1e-12)
    np.testing.assert_allclose(out["slope_high"], out["direct2"][0] + out["interaction"], rtol=1e-12)
    np.testing.assert_allclose(out["r2"], [0, 0, 1], atol=1e-12)
    assert out["record"].shape == (2 + 4 + 3,)
    # row multiplicities are rows: a data set with every row twice, and the same rows with count 2
    twice = _moderation(np.vstack((X, X)), None, np.ones(3), np.ones(3), singles(3), "AAA", fan_in(3), [(0, 1, 2)], dtype)
    counted = _moderation(X, np.full(X.shape[0], 2.0), np.ones(3), np.ones(3), singles(3), "AAA", fan_in(3), [(0, 1, 2)], dtype)
    np.testing.assert_allclose(counted["record"][:2], twice["record"][:2], rtol=1e-12)
    np.testing.assert_allclose(counted["interaction"], out["interaction"], rtol=1e-12)


def test_a_constant_product_is_status_3():
    """y_a = +-1 (two values, half the rows each) and y_b = y_a: the product is 1 in every row."""
    xa = np.tile([1.0, 2.0], 50)
    rng = np.random.default_rng(1)
    X = np.column_stack((xa, 5 * xa - 1, rng.standard_normal(100)))
    out = _moderation(X, None, np.ones(3), np.ones(3), singles(3), "AAA", fan_in(3), [(0, 1, 2)])
    assert out["product_sd"][0] == 0.0 and out["status"] == 3
    assert np.all(np.isnan(out["interaction"])) and np.all(np.isnan(out["f2"]))


def test_identical_predecessors_take_the_minimum_norm_route():
    rng = np.random.default_rng(2)
    x0, x2 = rng.standard_normal(150), rng.standard_normal(150)
    target = 0.5 * x0 + 0.3 * x2 + 0.2 * x0 * x2 + 0.5 * rng.standard_normal(150)
    X = np.column_stack((x0, x0, x2, target))
    out = _moderation(X, None, np.ones(4), np.ones(4), singles(4), "AAAA", fan_in(4), [(0, 2, 3)])
    assert not out["pivots_pass"] and out["status"] == 0 and np.all(np.isfinite(out["record"]))
    np.testing.assert_allclose(out["direct2"][0], out["direct2"][1], rtol=1e-9)      # the twins share their coefficient


# ------------------------------------------------------------------ the portable part of the kernels as a host program under sanitizers
def build_host():
    subprocess.check_call(["make", "-s", "-C", HOST, "moderation_host"])
    return os.path.join(HOST, "moderation_host")


def run_host(text, tmp_path, tag, stdin=False, expect=0):
    program = build_host()
    if stdin:
        run = subprocess.run([program], input=text, capture_output=True, text=True, timeout=120)
    else:
        path = tmp_path / (tag + ".txt")
        path.write_text(text)
        run = subprocess.run([program, str(path)], capture_output=True, text=True, timeout=120)
    assert run.returncode == expect, run.stderr
    assert "ERROR: " not in run.stderr and "runtime error" not in run.stderr, run.stderr
    return run


def header(mode, C, terms, items):
    return "\n".join([mode + " %d" % C.shape[0], " ".join(str(int(x)) for x in np.asarray(C).ravel()), "%d" % len(terms)] +
                     ["%d %d %d" % tuple(t) for t in terms] + [" ".join(str(int(k)) for k in items)])


def host_record(tmp_path, C, terms, mirror, counts, direct, r2, tag, stdin=False):
    """The record csrc/moderation_core.h computes from the mirror's scores: the needed LVs' correlations and the row sums, written as text."""
    numbers = lambda a: " ".join(repr(float(x)) for x in np.asarray(a, dtype=np.float64).ravel())
    n, rc, sums = core_inputs(mirror, C, terms, counts)
    assert rc.shape[0] == len(needed_lvs(C, terms)) and sums.shape[0] == len(sum_list(C, terms))
    text = "\n".join([header("record", C, terms, [1] * C.shape[0]), repr(float(n)), numbers(rc), numbers(sums), numbers(direct), numbers(r2)]) + "\n"
    values = np.array([float(x) for x in run_host(text, tmp_path, tag, stdin).stdout.split()])
    assert values.shape == (mirror["record"].shape[0] + 2,)
    return values


def single_item_case(n, C, terms, seed):
    """Single-item data with planted interactions, weights and loadings 1; the record's direct and r2 entries are made-up numbers the copies are known by."""
    from plspm.plsc import _effect_pairs
    L = C.shape[0]
    X, _ = planted(n, C, [1] * L, terms, seed)
    X = X + 0.3 * np.random.default_rng(seed + 100).standard_normal(X.shape)
    ne = len(_effect_pairs(C))
    direct, r2 = np.linspace(0.11, 0.19, ne), np.linspace(0.21, 0.29, L)
    return X, direct, r2


@pytest.mark.parametrize("stdin", [False, True])
def test_host_program_under_sanitizers_on_the_closed_form(tmp_path, stdin):
    X, _, _ = closed_form_data(np.float64)
    X[:, 2] += 0.2 * np.random.default_rng(9).standard_normal(X.shape[0])      # (off the exact fit: a finite f2)
    direct, r2 = np.array([0.4, 0.3]), np.array([0.0, 0.0, 0.9])
    out = _moderation(X, None, np.ones(3), np.ones(3), singles(3), "AAA", fan_in(3), [(0, 1, 2)], record_direct=direct, record_r2=r2)
    values = host_record(tmp_path, fan_in(3), [(0, 1, 2)], out, None, direct, r2, "closed_form", stdin=stdin)
    assert out["status"] == 0 and values[-2] == 0.0 and values[-1] == 7.0
    np.testing.assert_allclose(values[:-2], out["record"], rtol=1e-10, atol=1e-12)
    assert values[6] == 0.0 and values[7] == 0.0               # r2 of the LVs without terms: the record's own


@pytest.mark.parametrize("name", ["three_terms", "eight_terms", "ten_regressors"])
def test_host_program_against_the_mirror(tmp_path, name):
    """Three terms of which two share a target (a cross sum; the targets without terms copy the record); eight terms on one target (36 regression slots'
    worth of sums, 28 cross sums); nine predecessors and a term: ten regressors, beyond the eight-in-registers solve (solver_core.h spd_solve)."""
    if name == "three_terms":
        C, terms, n = SAT_C, SAT_TERMS, 400
    elif name == "eight_terms":
        C, terms, n = fan_in(6), [(a, b, 5) for a in range(5) for b in range(a + 1, 5)][:8], 500
    else:
        C, terms, n = fan_in(10), [(0, 1, 9)], 500
    L = C.shape[0]
    X, direct, r2 = single_item_case(n, C, terms, 11)
    rng = np.random.default_rng(5)
    counts = np.bincount(rng.integers(0, n, n), minlength=n).astype(np.float64)
    out = _moderation(X, counts, np.ones(L), np.ones(L), singles(L), "A" * L, C, terms, record_direct=direct, record_r2=r2)
    assert out["status"] == 0 and out["pivots_pass"]
    values = host_record(tmp_path, C, terms, out, counts, direct, r2, name)
    assert values[-2] == 0.0
    np.testing.assert_allclose(values[:-2], out["record"], rtol=1e-10, atol=1e-12)
    if name == "three_terms":                                   # EXPE, QUAL and VAL have no terms: their paths and R2 are the record's, bit for bit
        paths = out["paths"]
        for d, (f, t) in enumerate(paths):
            if t in (1, 2, 3):
                assert values[d] in direct
        assert np.array_equal(values[len(paths) + 12:len(paths) + 12 + 4][1:], r2[1:4])
    # slope_high - slope_low = 2 interaction
    n_dir, T = len(out["paths"]), len(terms)
    inter, low, high = (values[n_dir + k * T:n_dir + (k + 1) * T] for k in (0, 2, 3))
    np.testing.assert_allclose(high - low, 2 * inter, rtol=0, atol=1e-14)


def test_host_program_reports_a_constant_product(tmp_path):
    xa = np.tile([1.0, 2.0], 50)
    X = np.column_stack((xa, 5 * xa - 1, np.random.default_rng(1).standard_normal(100)))
    direct, r2 = np.array([0.1, 0.2]), np.array([0.0, 0.0, 0.5])
    out = _moderation(X, None, np.ones(3), np.ones(3), singles(3), "AAA", fan_in(3), [(0, 1, 2)], record_direct=direct, record_r2=r2)
    values = host_record(tmp_path, fan_in(3), [(0, 1, 2)], out, None, direct, r2, "constant_product")
    assert values[-2] == 3.0 and np.all(np.isnan(values[:6])) and values[6] == 0.0 and values[7] == 0.0 and np.isnan(values[8])      # (2 paths + 4, then r2 [3])


def test_host_program_refuses_bad_terms(tmp_path):
    for terms, word in (([(0, 0, 2)], "different"), ([(0, 1, 2), (1, 0, 2)], "same pair"), ([(0, 2, 1)], "add the path")):
        C = np.array([[0, 0, 0], [0, 0, 0], [1, 1, 0]])
        run = run_host(header("plan", C, terms, [1, 1, 1]) + "\n100\n", tmp_path, "bad", expect=3)
        assert word in run.stderr


# ------------------------------------------------------------------ the plan
def plan(tmp_path, C, terms, items, N):
    run = run_host(header("plan", C, terms, items) + "\n%d\n" % N, tmp_path, "plan")
    out = {}
    for line in run.stdout.splitlines():
        key, value = line.split(" ", 1)
        out[key] = value if key == "need" else int(value)
    return out


def test_the_plan(tmp_path):
    # the headline model (six LVs of ten items) with one and with three terms
    one = plan(tmp_path, SAT_C, SAT_TERMS[:1], [10] * 6, 10000)
    assert one["width"] == 10 + 4 + 6 and one["nsums"] == 2 + 4 + 1 and one["nacc"] == 16 and one["nl"] == 5 and one["ncoef"] == 50 and one["KM"] == 5
    assert one["row_block"] == 256 and one["row_blocks"] == 40 and one["table_in_lds"] == 1 and one["refused"] == 0 and one["njobs"] == 2
    assert one["rows_lds"] == ((50 + 5) * 64 + 4 * (1 + 5 + 1) * 64) * 8
    three = plan(tmp_path, SAT_C, SAT_TERMS, [10] * 6, 10000)
    assert three["width"] == 10 + 12 + 6 and three["nsums"] == 7 + 7 + 5 + 1 and three["nacc"] == 32 and three["nl"] == 6 and three["ncoef"] == 60
    assert three["ntgt"] == 2 and three["njobs"] == 3 + 2 and three["KM"] == 6
    # the first table that does not fit LDS beside four waves' values: (ncoef + 3) x 512 + 4 x 5 x 512 bytes > 160 KiB from 298 coefficients on
    fits, beyond = plan(tmp_path, fan_in(3), [(0, 1, 2)], [99, 99, 99], 400), plan(tmp_path, fan_in(3), [(0, 1, 2)], [100, 99, 99], 400)
    assert fits["table_in_lds"] == 1 and fits["rows_lds"] == 160 * 1024 and beyond["table_in_lds"] == 0 and beyond["rows_lds"] == 4 * 5 * 512 and beyond["refused"] == 0
    # the first shape refused: eight terms on a target of ten predecessors need 8 x 13 + 28 = 132 row sums; nine predecessors: 124
    eight = lambda L: [(a, b, L - 1) for a in range(5) for b in range(a + 1, 5)][:8]
    most = plan(tmp_path, fan_in(10), eight(10), [1] * 10, 400)
    assert most["nsums"] == 124 and most["nacc"] == 128 and most["refused"] == 0 and most["KM"] == 17
    over = plan(tmp_path, fan_in(11), eight(11), [1] * 11, 400)
    assert over["nsums"] == 132 and over["refused"] != 0 and "128 row sums" in over["need"]
    # the rows: one LDS histogram of 16-bit counters
    assert plan(tmp_path, fan_in(3), [(0, 1, 2)], [1, 1, 1], 65535)["refused"] == 0
    last = plan(tmp_path, fan_in(3), [(0, 1, 2)], [1, 1, 1], 65535)
    assert last["row_block"] == 1024 and last["row_blocks"] == 64 and last["counts_lds"] == 131072
    big = plan(tmp_path, fan_in(3), [(0, 1, 2)], [1, 1, 1], 65536)
    assert big["refused"] != 0 and "65535 rows" in big["need"]


# ------------------------------------------------------------------ the draws
def test_the_draws_restated_in_numpy():
    for seed, rep, n in ((3, 0, 70), (2 ** 40 + 5, 7, 1001), (17, 2 ** 33, 64)):
        mine = philox_draws(seed, rep, n)
        assert np.array_equal(mine, _native.bootstrap_indices(seed, rep, n)), (seed, rep, n)
        assert mine.min() >= 0 and mine.max() < n


# ------------------------------------------------------------------ the C-ABI's declarations and the errors that need no device
def test_new_symbols_are_declared_everywhere():
    header_text = open(os.path.join(ROOT, "include", "plspm_hip.h")).read()
    declared = set(re.findall(r"\b(plspm_[a-z_]+)\s*\(", header_text))
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
    one = np.zeros(1, dtype=np.int32)
    assert lib.plspm_moderation_enable(None, 1, one.ctypes.data, one.ctypes.data, one.ctypes.data) == 100         # PLSPM_E_ARG
    assert lib.plspm_moderation_enable(None, 0, None, None, None) == 100
    assert lib.plspm_moderation_width(None) == 0
    assert lib.plspm_moderation_fit(None, out.ctypes.data, None) == 100
    assert lib.plspm_moderation_fetch(None, 0, 1, out.ctypes.data, None) == 100
    assert lib.plspm_moderation_summary(None, 10, out.ctypes.data, out.ctypes.data, None) == 100
    assert lib.plspm_moderation_intervals(None, 10, out.ctypes.data, 0, 0.95, out.ctypes.data, None) == 100


def test_value_errors_of_the_terms():
    names = ["IMAG", "EXPE", "QUAL", "VAL", "SAT", "LOY"]
    assert _check_terms(SAT_C, [("IMAG", "EXPE", "SAT")], names) == [(0, 1, 4)]
    with pytest.raises(ValueError, match="add the path"):
        _check_terms(SAT_C, [("QUAL", "IMAG", "LOY")], names)      # QUAL -> LOY is no path of the model
    with pytest.raises(ValueError, match="listed twice"):
        _check_terms(SAT_C, [("IMAG", "EXPE", "SAT"), ("EXPE", "IMAG", "SAT")], names)
    with pytest.raises(ValueError, match="different"):
        _check_terms(SAT_C, [("IMAG", "IMAG", "SAT")], names)
    with pytest.raises(ValueError, match="unknown"):
        _check_terms(SAT_C, [("IMAG", "PRICE", "SAT")], names)
    nine = [(a, b, 5) for a in range(5) for b in range(a + 1, 5)][:MAX_TERMS + 1]
    with pytest.raises(ValueError, match="at most 8"):
        _check_terms(fan_in(6), nine)
    with pytest.raises(ValueError, match="at least one"):
        _check_terms(SAT_C, [])


def test_host_errors_that_need_no_device():
    from plspm.moderation import Moderation
    blank = Moderation.__new__(Moderation)
    with pytest.raises(NotImplementedError, match="no bca"):
        blank.intervals("interaction", "bca")
    with pytest.raises(ValueError):
        blank.intervals("interaction", "student")
    blank._paths, blank._terms, blank._lvs = [(0, 1)], [(0, 1, 2)], ["A", "B", "C"]
    with pytest.raises(ValueError, match="what must be one of"):
        blank._slice("vif")
