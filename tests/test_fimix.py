"""CPU: the host surface of FIMIX-PLS -- the NumPy mirror of the kernel (plspm.fimix._fimix) against least squares and the EM's monotonicity, the criteria
against their formulas, the portable part of the kernel (csrc/fimix_core.h) as a stand-alone host program under AddressSanitizer and
UndefinedBehaviorSanitizer, the plan of a call (csrc/fimix_route.h) against values worked out by hand, the declarations of the new C-ABI symbols, and the
host errors that need no device.

The plan table (test_the_plan_of_a_call), by hand.  One problem's LDS in doubles: kmax L^2 (the segments' moments) + 16 (n_dir + 2 n_endo + 3) (the parameter
tables, pitch 16) + 8 + waves (acc + 18) (the staging of the sums) + nslots (2 p^2 + p) (regression slots, p the most predecessors of one LV); a workgroup has 256
threads and 32 accumulators a thread whatever N; a problem of K segments (padded to KP = 1, 2, 4, 8, 16) sweeps 32 / KP moment entries at a time; nslots = min(64, kmax n_endo), halved while the LDS exceeds 160 KiB = 20,480 doubles.
    planted, N = 257, kmax = 4    L = 4, n_dir = 5, n_endo = 3, p = 2, 9 entries: width 2 + 4 (1 + 5 + 3) = 38; 64 + 224 + 8 + 4 x 50 + 12 x 10 = 616 doubles = 4,928 B;
                                  8 entries a sweep: 2 sweeps.  N = 10,000 the same.  kmax = 16: 2 entries a sweep, 5 sweeps; 256 + 224 + 8 + 200 + 48 x 10 = 1,168 doubles
    chunk edges                   kmax = 4: 7 and 8 entries 1 sweep, 9 entries 2; kmax = 1 (L = 9, n_dir = 8, n_endo = 1, p = 8: 81 + 208 + 8 + 200 + 136 = 633 doubles = 5,064 B): 32 entries
                                  1 sweep, 33 entries 2
    LDS edge, kmax = 16           a chain of L LVs (n_dir = n_endo = L - 1, p = 1, 2 L - 1 entries), 256 threads: 16 L^2 + 48 L + 208 + 3 nslots doubles.  L = 34:
                                  20,336 + 3 nslots fits with 32 slots (20,432 doubles = 163,456 B), not with 64; 2 entries a sweep: 34 sweeps.  L = 35: 21,488 + 3 with
                                  one slot = 171,928 B: refused."""
import os
import re
import subprocess

import numpy as np
import pandas as pd
import pytest

import plspm.config as c
import helpers_fimix as hf
from helpers import SAT_ADD_ORDER, SAT_PREFIX, satisfaction_frame
from plspm import _native
from plspm.fimix import Fimix, _criteria, _direct_paths, _fimix, _record, record_width
from plspm.mode import Mode
from plspm.scale import Scale
from plspm.scheme import Scheme

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tests", "fimix_host")
NEW_SYMBOLS = ("plspm_fimix_device", "plspm_fimix_width", "plspm_fimix_fetch", "plspm_fimix_posteriors", "plspm_fimix_starts")


def cases():
    return {"chain": hf.two_segment(hf.tri(2), 40, 2)[:2], "planted257": hf.planted(257)[:2], "planted1000": hf.planted(1000)[:2],
            "fan_in_11": hf.two_segment(hf.fan_in(11), 300, 5)[:2], "dense_7": hf.two_segment(hf.dense(7), 300, 3)[:2]}


# ------------------------------------------------------------------ the mirror
@pytest.mark.parametrize("dtype", [np.float64, np.longdouble])
@pytest.mark.parametrize("name", ["chain", "planted257", "dense_7"])
def test_mirror_with_one_segment_is_least_squares(name, dtype):
    Y, C = cases()[name]
    N = Y.shape[0]
    out = _fimix(Y.astype(dtype), C, 1, np.zeros(N, dtype=np.uint8), 50, 1e-10)
    assert out["status"] == 0 and out["iterations"] == 2 and out["beta"].dtype == np.dtype(dtype)
    lnl = 0.0
    for je, j in enumerate(out["endo"]):
        S = np.flatnonzero(C[j])
        beta, res = np.linalg.lstsq(Y[:, S], Y[:, j], rcond=None)[:2]
        np.testing.assert_allclose([out["beta"][0, out["paths"].index((int(p), j))] for p in S], beta, rtol=1e-10, atol=1e-12)
        np.testing.assert_allclose(float(out["psi"][0, je]), res[0] / N, rtol=1e-10)
        lnl += -N / 2 * (np.log(2 * np.pi * res[0] / N) + 1)
    np.testing.assert_allclose(float(out["lnl"]), lnl, rtol=1e-11)
    assert out["rho"][0] == 1 and out["h"] == 0 and np.all(out["posteriors"] == 1)


@pytest.mark.parametrize("name", ["chain", "planted257", "planted1000", "fan_in_11", "dense_7", "collinear"])
def test_mirror_never_loses_likelihood(name):
    """lnL^t >= lnL^(t-1) - bar for every t, the bar of lnL: ten times the largest difference between the two mirrors' traces, at least 1e-12 max(1, |lnL|)."""
    Y, C = hf.collinear(300)[:2] if name == "collinear" else cases()[name]
    solve = hf.pinv_solve if name == "collinear" else None
    for K in (2, 3):
        m64, mld = hf.mirror_pair(Y, C, K, hf.random_init(Y.shape[0], K, K), 40, 0.0, solve=solve)
        assert m64["status"] == mld["status"] == 1 and m64["iterations"] == 40
        t64, tld = np.array(m64["trace"], dtype=np.float64), np.array(mld["trace"], dtype=np.longdouble)
        bar = max(10.0 * float(np.max(np.abs(t64 - tld))), hf.FLOOR * max(1.0, float(np.max(np.abs(t64)))))
        assert np.all(np.diff(t64) >= -bar), (name, K, float(np.diff(t64).min()), bar)


def test_snapshots_are_the_runs_of_fewer_iterations():
    Y, C = cases()["planted257"]
    init = hf.random_init(257, 3, 1)
    whole = _fimix(Y, C, 3, init, 25, 0.0, snapshots=(1, 2, 5))
    for t in (1, 2, 5):
        short = _fimix(Y, C, 3, init, t, 0.0)
        assert short["status"] == 1 and short["iterations"] == t
        assert np.array_equal(_record(short, 4), _record(hf.at(whole, t), 4), equal_nan=True)
    rec = _record(whole, 4)
    assert rec.shape == (record_width(4, 5, 3),) and np.all(np.isnan(rec[5:6])) and not np.any(np.isnan(rec[:5]))       # rho of the slot k = 3 >= K
    assert _direct_paths(C) == [(0, 1), (0, 2), (1, 2), (1, 3), (2, 3)]


def test_mirror_collapses():
    Y, C = cases()["planted257"]
    out = _fimix(Y, C, 2, np.zeros(257, dtype=np.uint8), 25, 0.0)
    assert out["status"] == 2 and out["iterations"] == 1 and np.all(np.isnan(_record(out, 2)))
    Ye, Ce = hf.exact_function(300)
    out = _fimix(Ye, Ce, 2, hf.random_init(300, 2, 3), 25, 0.0)
    assert out["status"] == 2 and np.all(np.isnan(_record(out, 2)))


def test_criteria_against_their_formulas():
    lnl, h, N, K, n_dir, n_endo = -1234.5, 37.25, 500, 3, 5, 3
    nk = 2 + 3 * 8
    got = _criteria(lnl, h, N, K, n_dir, n_endo)
    want = dict(lnl=lnl, aic=2469.0 + 2 * nk, aic3=2469.0 + 3 * nk, aic4=2469.0 + 4 * nk, bic=2469.0 + np.log(500) * nk, caic=2469.0 + (np.log(500) + 1) * nk,
                hq=2469.0 + 2 * np.log(np.log(500)) * nk, mdl5=2469.0 + 5 * np.log(500) * nk, en=1 - 37.25 / (500 * np.log(3)))
    assert set(got) == set(want)
    for name in want:
        np.testing.assert_allclose(got[name], want[name], rtol=1e-14)
    assert np.isnan(_criteria(lnl, 0.0, N, 1, n_dir, n_endo)["en"]) and _criteria(lnl, 0.0, N, 1, n_dir, n_endo)["aic"] == 2469.0 + 2 * 8


# ------------------------------------------------------------------ the portable part of the kernel as a host program under sanitizers
def build_host():
    subprocess.check_call(["make", "-s", "-C", HOST, "fimix_host"])
    return os.path.join(HOST, "fimix_host")


def host_record(tmp_path, Y, C, K, kmax, init, max_iter, tol, tag, stdin=False):
    program = build_host()
    N, L = Y.shape
    text = "\n".join(["%d %d %d %d %d %r" % (N, L, K, kmax, max_iter, float(tol)), " ".join(str(int(x)) for x in np.asarray(C).ravel()),
                      " ".join(repr(float(x)) for x in Y.ravel()), " ".join(str(int(x)) for x in init)]) + "\n"
    if stdin:
        run = subprocess.run([program], input=text, capture_output=True, text=True, timeout=300)
    else:
        path = tmp_path / (tag + ".txt")
        path.write_text(text)
        run = subprocess.run([program, str(path)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr
    assert "ERROR" not in run.stderr and "runtime error" not in run.stderr, run.stderr
    values = np.array([float(x) for x in run.stdout.split()])
    assert values.shape == (record_width(kmax, int(np.count_nonzero(C)), int(np.count_nonzero(np.asarray(C).any(axis=1)))) + 2,)
    return values


@pytest.mark.parametrize("name,K", [("chain", 1), ("chain", 2), ("planted257", 2), ("planted257", 3), ("planted257", 4), ("planted1000", 4), ("fan_in_11", 2), ("dense_7", 4),
                                    ("collinear", 2)])
def test_host_program_under_sanitizers_agrees_with_the_mirror(tmp_path, name, K):
    Y, C = hf.collinear(300)[:2] if name == "collinear" else cases()[name]
    solve = hf.pinv_solve if name == "collinear" else None
    init = hf.random_init(Y.shape[0], K, 7)
    m64, mld = hf.mirror_pair(Y, C, K, init, 25, 0.0, solve=solve, snapshots=(1, 2, 5))
    for t in (2, 25):
        values = host_record(tmp_path, Y, C, K, 4, init, t, 0.0, "%s_%d_%d" % (name, K, t), stdin=(t == 2))
        want = hf.at(m64, t)          # (one segment: lnL repeats exactly, status 0 at iteration 2 whatever tol)
        assert want["status"] == (0 if K == 1 else 1) and want["iterations"] == (2 if K == 1 else t) and hf.at(mld, t)["iterations"] == want["iterations"]
        assert values[-2] == want["status"] and values[-1] == want["iterations"]
        hf.assert_inside(values[:-2], *hf.records(want, hf.at(mld, t), 4), what="%s K %d at %d" % (name, K, t))


def test_host_program_stops_and_collapses_like_the_mirror(tmp_path):
    Y, C = cases()["planted257"]
    init = hf.random_init(257, 2, 0)
    m64, mld = hf.mirror_pair(Y, C, 2, init, 5000, 1e-6)
    assert m64["status"] == 0 and mld["iterations"] == m64["iterations"]
    values = host_record(tmp_path, Y, C, 2, 2, init, 5000, 1e-6, "converged")
    assert values[-2] == 0.0 and values[-1] == m64["iterations"]
    hf.assert_inside(values[:-2], *hf.records(m64, mld, 2), what="converged")
    values = host_record(tmp_path, Y, C, 2, 2, np.zeros(257, dtype=np.uint8), 25, 0.0, "empty")
    assert values[-2] == 2.0 and values[-1] == 1.0 and np.all(np.isnan(values[:-2]))
    Ye, Ce = hf.exact_function(300)
    values = host_record(tmp_path, Ye, Ce, 2, 2, hf.random_init(300, 2, 3), 25, 0.0, "exact")
    assert values[-2] == 2.0 and np.all(np.isnan(values[:-2]))


def test_the_plan_of_a_call():
    """width threads acc nslots lds_bytes fits sweeps, against the values of the module docstring."""
    program = build_host()
    table = [("257 4 5 3 2 9 4", "38 256 32 12 4928 1 2"), ("10000 4 5 3 2 9 4", "38 256 32 12 4928 1 2"), ("257 4 5 3 2 9 16", "146 256 32 48 9344 1 5"),
             ("300 4 5 3 2 7 4", "38 256 32 12 4928 1 1"), ("300 4 5 3 2 8 4", "38 256 32 12 4928 1 1"), ("300 4 5 3 2 9 4", "38 256 32 12 4928 1 2"),
             ("300 9 8 1 8 32 1", "12 256 32 1 5064 1 1"), ("300 9 8 1 8 33 1", "12 256 32 1 5064 1 2"),
             ("60 34 33 33 1 67 16", "1074 256 32 32 163456 1 34"), ("60 35 34 34 1 69 16", "1106 256 32 1 171928 0 35")]
    run = subprocess.run([program, "plan"], input="\n".join(shape for shape, _ in table) + "\n", capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stderr == "", run.stderr
    assert run.stdout.splitlines() == [plan for _, plan in table]


# ------------------------------------------------------------------ the surface
def test_new_symbols_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "plspm_hip.h")).read() + open(os.path.join(ROOT, "include", "plspm_hip_test.h")).read()
    declared = set(re.findall(r"\b(plspm_[a-z_]+)\s*\(", header))
    for name in NEW_SYMBOLS:
        assert name in declared and name in _native.EXPORTS
    assert "plspm_fimix_starts" in open(os.path.join(ROOT, "include", "plspm_hip_test.h")).read()
    lib = _native.load()
    assert all(hasattr(lib, name) for name in NEW_SYMBOLS) and lib.plspm_abi_version() == 4


def test_null_handle_calls_return_the_argument_error():
    lib = _native.load()
    k_of = np.array([2], dtype=np.int32)
    assert lib.plspm_fimix_device(None, 1, _native._ptr(k_of), 2, 0, 0, None, 10, 0.0, None, None, None) == 100
    assert lib.plspm_fimix_fetch(None, 0, 1, None, None, None) == 100
    assert lib.plspm_fimix_posteriors(None, 0, None) == 100
    assert lib.plspm_fimix_width(None, 2) == 0
    seg = np.zeros(8, dtype=np.uint8)
    assert lib.plspm_fimix_starts(1, 0, 8, 0, _native._ptr(seg)) == 100 and lib.plspm_fimix_starts(1, 0, 8, 17, _native._ptr(seg)) == 100
    assert lib.plspm_fimix_starts(1, 0, 8, 2, None) == 100


def test_starts_are_deterministic_and_uniform():
    a, b = _native.fimix_starts(5, 3, 10_000, 4), _native.fimix_starts(5, 3, 10_000, 4)
    assert a.dtype == np.uint8 and np.array_equal(a, b) and a.max() == 3
    assert not np.array_equal(a, _native.fimix_starts(5, 4, 10_000, 4)) and not np.array_equal(a, _native.fimix_starts(6, 3, 10_000, 4))
    assert np.array_equal(a[:100], _native.fimix_starts(5, 3, 100, 4))                 # counter-based: row i whatever N
    sd = np.sqrt(10_000 * 0.25 * 0.75)
    for start in range(5):
        counts = np.bincount(_native.fimix_starts(5, start, 10_000, 4), minlength=4)
        assert np.all(np.abs(counts - 2_500) <= 5 * sd), counts
    assert np.all(_native.fimix_starts(9, 0, 50, 1) == 0)


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
    for segments in ([0, 1], [17], [], [2, 2]):
        with pytest.raises(ValueError, match="segments"):
            Fimix(sat, cfg, Scheme.PATH, segments=segments)
    with pytest.raises(ValueError, match="starts"):
        Fimix(sat, cfg, Scheme.PATH, starts=0)
    sat, numeric = sat_config(Scale.NUM)
    with pytest.raises(NotImplementedError, match="non-metric"):
        Fimix(sat, numeric, Scheme.PATH)
    sat, cfg = sat_config()
    holes = sat.copy()
    holes.iloc[3, 2] = np.nan
    with pytest.raises(NotImplementedError, match="missing cells"):
        Fimix(holes, cfg, Scheme.PATH)
    mobi = pd.read_csv(os.path.join(ROOT, "tests", "golden", "ref_data", "mobi.csv"), index_col=0).astype(float)
    structure = c.Structure()
    structure.add_path(["Expectation", "Quality"], ["Satisfaction"])
    structure.add_path(["Satisfaction"], ["Complaints", "Loyalty"])
    hoc = c.Config(structure.path())
    hoc.add_higher_order("Satisfaction", Mode.A, ["Image", "Value"])
    for lv, prefix in (("Expectation", "CUEX"), ("Quality", "PERQ"), ("Loyalty", "CUSL"), ("Image", "IMAG"), ("Complaints", "CUSCO"), ("Value", "PERV")):
        hoc.add_lv_with_columns_named(lv, Mode.A, mobi, prefix)
    with pytest.raises(NotImplementedError, match="higher-order"):
        Fimix(mobi, hoc, Scheme.PATH)
    lvs = ["IMAG", "EXPE"]
    alone = c.Config(pd.DataFrame(0, index=lvs, columns=lvs), scaled=True)
    for lv in lvs:
        alone.add_lv_with_columns_named(lv, Mode.A, sat, SAT_PREFIX[lv])
    with pytest.raises(ValueError, match="no path"):
        Fimix(sat, alone, Scheme.PATH)
