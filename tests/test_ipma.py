"""CPU: the host surface of the importance-performance map analysis -- the NumPy mirror (plspm.ipma._ipma) against the same quantities computed another way
from the raw rows, its invariance under affine maps of the columns, the portable part of the kernel (csrc/ipma_core.h: lists, plan, ipma_record) as a
stand-alone host program under AddressSanitizer and UndefinedBehaviorSanitizer, the edges of the launch plan, the declarations of the new C-ABI symbols, the
refusals and the host errors that need no device.

The bar of every comparison with the mirror is the project's mirror_bar rule per field (tests/helpers_ipma.py): ten times |fp64 mirror - longdouble mirror| on
the same rows, never below 1e-12 times the field's scale (100 for perf, mvperf and sd, 1 for the rest).  The comparisons with quantities computed another way
(least squares, column means of the rescaled scores) carry the other route's own rounding: 1e-9 on the 0-100 scale, 1e-11 on the effects."""
import fnmatch
import os
import re
import subprocess

import numpy as np
import pandas as pd
import pytest

import plspm.config as c
import plspm_oracle as orc
from helpers import SAT_ADD_ORDER, SAT_PREFIX, satisfaction_frame
from helpers_ipma import (FLOOR, case, check_record, dev_blocks, field_bars, host_input, mirror_pair, observed_bounds, oracle_record, pick, tri, wider_bounds)
from plspm import _native
from plspm.ipma import FIELDS, WHAT, Ipma, _bounds, _ipma, _layout
from plspm.mode import Mode
from plspm.scale import Scale
from plspm.scheme import Scheme

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tests", "ipma_host")
NEW_SYMBOLS = ("plspm_ipma_enable", "plspm_ipma_width", "plspm_ipma_targets", "plspm_ipma_fit", "plspm_ipma_fetch", "plspm_ipma_summary", "plspm_ipma_intervals")


# ------------------------------------------------------------------ the portable part of the kernel as a host program under sanitizers
def build_host():
    subprocess.check_call(["make", "-s", "-C", HOST, "ipma_host"])
    return os.path.join(HOST, "ipma_host")


def run_host(text, tmp_path=None, tag=None):
    program = build_host()
    if tmp_path is None:
        run = subprocess.run([program, "record"], input=text, capture_output=True, text=True, timeout=120)
    else:
        path = tmp_path / (tag + ".txt")
        path.write_text(text)
        run = subprocess.run([program, "record", str(path)], capture_output=True, text=True, timeout=120)
    assert "ERROR" not in run.stderr and "runtime error" not in run.stderr, run.stderr
    return run


def host_record(X, sizes, pairs, record, lo, hi, mask=None, tmp_path=None, tag=None):
    """The record csrc/ipma_core.h computes: (targets, values [W], status, iterations)."""
    run = run_host(host_input(X, sizes, pairs, record, lo, hi, mask), tmp_path, tag)
    assert run.returncode == 0, (run.stdout, run.stderr)
    out = run.stdout.split("\n")
    head = [int(v) for v in out[0].split()]
    W = int(out[1])
    values = np.array([float(v) for v in out[2:2 + W + 2]])
    assert head[0] == len(head) - 1
    return head[1:], values[:W], values[W], values[W + 1]


def sized_case(sizes, seed, modes=None, n=200):
    """n rows of a chain model with blocks of `sizes`: (rows in device order, model, the oracle's record of all rows, its effect pairs)."""
    L = len(sizes)
    X, _ = orc.synth(n, tri(L), max(sizes), seed=seed)
    model = orc.Model(pick(max(sizes), sizes), tri(L), modes or "A" * L, "centroid", True)
    rec, pairs = oracle_record(X, model)
    return X[:, model.mv_order], model, rec, pairs


def check_host_against_mirror(Xd, model, rec, pairs, lo, hi, tag, targets=None, tmp_path=None, status=0):
    sizes = [len(b) for b in model.blocks]
    mask = None if targets is None else [1 if l in targets else 0 for l in range(model.L)]
    got_targets, values, st, iterations = host_record(Xd, sizes, pairs, rec, lo, hi, mask, tmp_path, tag)
    m64, mld = mirror_pair(Xd, model, rec, pairs, lo, hi, targets)
    assert got_targets == m64["targets"] and iterations == 7.0
    worst = check_record(values, m64, mld, tag)
    print("%s: max |host program - mirror| per field %s" % (tag, {k: "%.1e" % v for k, v in worst.items()}))
    assert st == m64["status"] == mld["status"] == status, (tag, st, m64["status"], mld["status"])
    return values, m64


@pytest.mark.parametrize("sizes,tag", [([1, 4], "single_item"), ([3, 4], "k4"), ([65, 5], "k65"), ([66, 5], "k66")])
def test_host_program_on_block_sizes(tmp_path, sizes, tag):
    """A single-item block (weight_r exactly 1, its performance the item's); four items; 65 and 66 items: lane p of phase 2 takes a second item of the same block,
    and the batches of eight rows end on a full batch and on one of two."""
    Xd, model, rec, pairs = sized_case(sizes, seed=31 + len(tag))
    Xd = Xd * 1.7 + 0.3
    lo, hi = Xd.min(axis=0), Xd.max(axis=0)
    values, m64 = check_host_against_mirror(Xd, model, rec, pairs, lo, hi, tag, tmp_path=tmp_path if tag == "k4" else None)
    at, _ = _layout(sum(sizes), 2, len(pairs), 1)
    weights = values[at["weight_r"]]
    for blk in dev_blocks(model):
        assert abs(weights[blk].sum() - 1.0) <= 1e-14
    if sizes[0] == 1:
        assert weights[0] == 1.0 and values[at["perf"]][0] == values[at["mvperf"]][0]
    assert np.all(values[at["mvimp"]][sizes[0]:] == 0.0) and np.all(values[at["mvimp"]][:sizes[0]] != 0.0)      # the target's own block: 0


def test_host_program_on_120_mvs_and_a_target_mask():
    X, model, _, _, _ = case("quad_120x12")
    rec, pairs = oracle_record(X, model)
    Xd = X[:, model.mv_order]
    lo, hi = wider_bounds(X, model)
    values, m64 = check_host_against_mirror(Xd, model, rec, pairs, lo, hi, "quad_120x12")
    assert m64["targets"] == list(range(1, 12)) and values.shape == (2 * 12 + 2 * len(pairs) + 2 * 120 + 11 * 120,)
    masked, one = check_host_against_mirror(Xd, model, rec, pairs, lo, hi, "quad_120x12 masked", targets=[3, 11])
    at, _ = _layout(120, 12, len(pairs), 11)
    at2, _ = _layout(120, 12, len(pairs), 2)
    full = values[at["mvimp"]].reshape(11, 120)
    assert np.array_equal(masked[at2["mvimp"]].reshape(2, 120), full[[2, 10]]) and np.array_equal(masked[:at2["mvimp"].start], values[:at["mvimp"].start])


def test_host_program_on_a_constant_column():
    """Status 3, the values standing: the whole block of the constant column is not finite (0 * inf), and with it what reads its A; the rest is the mirror's."""
    Xd, model, rec, pairs = sized_case([4, 4, 4], seed=8)
    Xd = Xd.copy()
    lo, hi = Xd.min(axis=0) - 0.5, Xd.max(axis=0) + 0.5
    Xd[:, 1] = 1.25
    lo[1], hi[1] = 0.0, 2.0
    rec = rec.copy()
    rec[1] = 0.0                                             # the solver gives a constant item weight 0
    values, m64 = check_host_against_mirror(Xd, model, rec, pairs, lo, hi, "constant", status=3)
    at, _ = _layout(12, 3, len(pairs), 2)
    assert not np.any(np.isfinite(values[at["weight_r"]][:4])) and np.all(np.isfinite(values[at["weight_r"]][4:]))
    assert np.all(np.isfinite(values[at["mvperf"]])) and values[at["mvperf"]][1] == 62.5
    assert not np.isfinite(values[at["perf"]][0]) and np.all(np.isfinite(values[at["perf"]][1:]))


def test_host_program_on_a_negative_mode_b_weight():
    """Status 4, the values standing: a Mode-B block whose second weight is negative has a negative rescaled weight."""
    Xd, model, rec, pairs = sized_case([4, 4, 4], seed=9, modes="ABA")
    rec = rec.copy()
    rec[5] = -0.4 * abs(rec[5])
    lo, hi = Xd.min(axis=0), Xd.max(axis=0)
    values, m64 = check_host_against_mirror(Xd, model, rec, pairs, lo, hi, "mode_b", status=4)
    at, _ = _layout(12, 3, len(pairs), 2)
    assert np.all(np.isfinite(values)) and values[at["weight_r"]][5] < 0 and m64["min_abs_weight"] > 1e-3
    # a non-finite value wins over inadmissibility
    Xc = Xd.copy()
    Xc[:, 9] = 2.0
    lo2, hi2 = lo.copy(), hi.copy()
    lo2[9], hi2[9] = 1.0, 3.0
    check_host_against_mirror(Xc, model, rec, pairs, lo2, hi2, "mode_b constant", status=3)


def test_host_program_refusals():
    Xd, model, rec, pairs = sized_case([3, 4, 2], seed=5, n=40)
    sizes = [3, 4, 2]
    lo, hi = Xd.min(axis=0), Xd.max(axis=0)

    def refused(lo, hi, mask):
        run = run_host(host_input(Xd, sizes, pairs, rec, lo, hi, mask))
        assert run.returncode == 3, (run.stdout, run.stderr)
        return run.stdout
    bad = hi.copy(); bad[4] = lo[4]
    assert refused(lo, bad, None).startswith("refused arg MV 4: the bounds must be finite with lo < hi")
    bad = lo.copy(); bad[7] = -np.inf
    assert refused(bad, hi, None).startswith("refused arg MV 7:")
    bad = hi.copy(); bad[0] = np.nan
    assert refused(lo, bad, None).startswith("refused arg MV 0:")
    assert refused(lo, hi, [0, 0, 0]).startswith("refused arg the mask names no LV")
    assert refused(lo, hi, [1, 1, 0]).startswith("refused arg LV 0 has no predecessor")
    targets, _, status, _ = host_record(Xd, sizes, pairs, rec, lo, hi, [0, 0, 1])
    assert targets == [2] and status == 0.0


# ------------------------------------------------------------------ the plan's edges, derived from ipma_wave_doubles' own formula
def test_plan_edges():
    """One wave's slice is 7 P + 2 L + n_eff + 2 doubles; 4, 2 or 1 waves per workgroup, the largest count whose slices fit 160 KiB; refused when one does not."""
    program = build_host()
    L, ne, nt, cap, tail = 12, 66, 11, 160 * 1024 // 8, 2
    doubles = lambda P: 7 * P + 2 * L + ne + tail
    last = {w: (cap // w - 2 * L - ne - tail) // 7 for w in (4, 2, 1)}          # the largest P with w waves
    probes = [1, last[4], last[4] + 1, last[2], last[2] + 1, last[1], last[1] + 1]
    run = subprocess.run([program, "plan", str(L), str(ne), str(nt)] + [str(p) for p in probes], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "ERROR" not in run.stderr and "runtime error" not in run.stderr, run.stderr
    rows = [[int(v) for v in line.split()] for line in run.stdout.strip().split("\n")]
    print("plan edges at L = %d, n_eff = %d: four waves up to P = %d, two up to %d, one up to %d" % (L, ne, last[4], last[2], last[1]))
    for (P, waves, wd, lds, grid, refused, stride), probe, want in zip(rows, probes, [4, 4, 2, 2, 1, 1, None]):
        assert P == probe and wd == doubles(P) and stride == 2 * L + 2 * ne + 2 * P + nt * P + 2
        if want is None:
            assert refused == 1
            continue
        assert refused == 0 and waves == want and lds == waves * wd * 8 and lds <= 160 * 1024 and grid == -(-1000 // waves)
        assert waves == 4 or 2 * waves * wd * 8 > 160 * 1024          # the largest count that fits


# ------------------------------------------------------------------ the mirror against quantities computed another way from the raw rows
@pytest.mark.parametrize("name", ["wave_60x6", "mode_b", "packed_40"])
@pytest.mark.parametrize("bounds", ["observed", "wider"])
def test_mirror_against_the_rescaled_scores(name, bounds):
    X, model, _, _, _ = case(name)
    rec, pairs = oracle_record(X, model)
    Xd = X[:, model.mv_order]
    lo, hi = observed_bounds(X, model) if bounds == "observed" else wider_bounds(X, model)
    m = _ipma(Xd, dev_blocks(model), rec, pairs, lo, hi)
    assert m["status"] == 0 and m["record"].shape == (_layout(model.P, model.L, len(pairs), len(m["targets"]))[1],)
    blocks, L = dev_blocks(model), model.L
    Y = np.column_stack([(100.0 * (Xd[:, b] - lo[b]) / (hi[b] - lo[b])) @ m["weight_r"][b] for b in blocks])
    for b in blocks:
        assert abs(m["weight_r"][b].sum() - 1.0) <= 1e-14
    assert np.max(np.abs(Y.mean(axis=0) - m["perf"])) <= 1e-9 and np.max(np.abs(Y.std(axis=0) - np.abs(m["sd"]))) <= 1e-9
    np.testing.assert_allclose(m["mvperf"], (100.0 * (Xd - lo) / (hi - lo)).mean(axis=0), rtol=0, atol=1e-9)
    # direct_u: the least-squares slopes (with intercept) of Y_j on the Y of j's predecessors;  total_u: the sum of the powers of that path matrix
    Bu = np.zeros((L, L))
    for j in range(L):
        pred = np.flatnonzero(model.C[j])
        if pred.size:
            D = np.column_stack((np.ones(Y.shape[0]), Y[:, pred]))
            Bu[j, pred] = np.linalg.lstsq(D, Y[:, j], rcond=None)[0][1:]
    total, power = np.zeros((L, L)), Bu.copy()
    for _ in range(L):
        total += power
        power = power @ Bu
    for e, (f, t) in enumerate(pairs):
        assert abs(m["direct_u"][e] - Bu[t, f]) <= 1e-11 and abs(m["total_u"][e] - total[t, f]) <= 1e-11, (f, t)
    # mvimp: the product of its two factors; 0 without an effect pair and on the target's own block
    lvof = np.repeat(np.arange(L), [len(b) for b in blocks])
    for k, target in enumerate(m["targets"]):
        want = np.array([m["weight_r"][p] * total[target, lvof[p]] for p in range(model.P)])
        np.testing.assert_allclose(m["mvimp"][k], want, rtol=0, atol=1e-11)
        assert np.all(m["mvimp"][k][lvof == target] == 0.0)


@pytest.mark.parametrize("name", ["k3_4_13", "mode_b"])
def test_mirror_is_invariant_under_affine_maps_of_the_columns(name):
    """x_p -> c_p x_p + d_p (c_p > 0) with the bounds mapped along: the standardised columns of a scaled model do not move, so the fit is the same one -- its
    record's weights, which multiply the columns as uploaded (v_p = w_p s_p), become w_p / c_p, everything else stays -- and the IPMA record is unchanged
    within the bar."""
    X, model, _, _, _ = case(name)
    rec, pairs = oracle_record(X, model)
    Xd = X[:, model.mv_order]
    lo, hi = wider_bounds(X, model)
    rng = np.random.default_rng(5)
    cc, dd = rng.uniform(0.25, 8.0, model.P), rng.uniform(-50.0, 50.0, model.P)
    m64, mld = mirror_pair(Xd, model, rec, pairs, lo, hi)
    rec_moved = rec.copy()
    rec_moved[:model.P] /= cc
    moved = _ipma(Xd * cc + dd, dev_blocks(model), rec_moved, pairs, lo * cc + dd, hi * cc + dd)
    # the moved data carry their own rounding: the bar is taken on both sides
    m64b, mldb = mirror_pair(Xd * cc + dd, model, rec_moved, pairs, lo * cc + dd, hi * cc + dd)
    bars, bars_b = field_bars(m64, mld), field_bars(m64b, mldb)
    for name_ in FIELDS:
        diff = float(np.max(np.abs(moved[name_] - m64[name_])))
        assert diff <= bars[name_] + bars_b[name_], (name_, diff)
    assert moved["status"] == m64["status"] == 0


def test_mirror_in_longdouble_and_its_layout():
    X, model, _, _, _ = case("k4")
    rec, pairs = oracle_record(X, model)
    lo, hi = observed_bounds(X, model)
    m64, mld = mirror_pair(X[:, model.mv_order], model, rec, pairs, lo, hi)
    assert mld["record"].dtype == np.longdouble and m64["record"].dtype == np.float64
    at, width = _layout(7, 2, 1, 1)
    assert width == 2 * 2 + 2 * 1 + 2 * 7 + 7 and [at[f].start for f in FIELDS] == [0, 2, 4, 5, 6, 13, 20]
    assert all(v >= FLOOR * (100.0 if f in ("perf", "sd", "mvperf") else 1.0) for f, v in field_bars(m64, mld).items())
    assert np.array_equal(m64["record"][at["mvimp"]], m64["mvimp"].ravel()) and len(WHAT) == len(FIELDS)


# ------------------------------------------------------------------ ipma_mv_stats is kernels_moments.h mv_stats
def test_ipma_mv_stats_repeats_mv_stats_operation_for_operation():
    """The portable copy (csrc/ipma_core.h) and the device's (csrc/kernels_moments.h) are the same three statements once the moment accessor is named alike
    and the device's extra `varies` member is dropped: the threshold for a constant column cannot change in one of them alone."""
    csrc = os.path.join(ROOT, "plspm-python_amd", "csrc")

    def body(path, name):
        text = open(os.path.join(csrc, path)).read()
        found = re.search(r"%s\([^)]*\) \{\n(.*?)\n\}" % name, text, re.S)
        assert found, (path, name)
        return [" ".join(line.split()) for line in found.group(1).split("\n")]
    device = [line.replace("assess_moment<DENSE>(M, ld, ", "mom(").replace(", varies};", "};") for line in body("kernels_moments.h", "mv_stats")]
    portable = body("ipma_core.h", "ipma_mv_stats")
    assert len(device) == 3 and device == portable, (device, portable)
    assert "var > 1e-9 * m2" in portable[1] and "fma(-m, m, m2)" in portable[0]


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
    assert lib.plspm_ipma_enable(None, 1, None, out.ctypes.data, out.ctypes.data) == 100         # PLSPM_E_ARG
    assert lib.plspm_ipma_width(None) == 0
    assert lib.plspm_ipma_targets(None, None, None) == 100
    assert lib.plspm_ipma_fit(None, out.ctypes.data, None) == 100
    assert lib.plspm_ipma_fetch(None, 0, 1, out.ctypes.data, None) == 100
    assert lib.plspm_ipma_summary(None, 10, out.ctypes.data, out.ctypes.data, None) == 100
    assert lib.plspm_ipma_intervals(None, 10, out.ctypes.data, 2, 0.95, out.ctypes.data, None) == 100


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


def test_bounds():
    values = np.array([[1.0, 2.0, 5.0], [3.0, 2.5, 7.0], [2.0, 4.0, 6.0]])
    names = ["a", "b", "c"]
    lo, hi = _bounds(values, names, None)
    assert lo.tolist() == [1.0, 2.0, 5.0] and hi.tolist() == [3.0, 4.0, 7.0]
    lo, hi = _bounds(values, names, (0, 10))
    assert lo.tolist() == [0.0] * 3 and hi.tolist() == [10.0] * 3
    lo, hi = _bounds(values, names, {"b": (1, 5)})
    assert lo.tolist() == [1.0, 1.0, 5.0] and hi.tolist() == [3.0, 5.0, 7.0]
    for bad, match in (((1, 6), "c has data outside"), ((5, 5), "lo < hi"), ((7, 1), "lo < hi"), ({"z": (0, 1)}, "unknown"), ({"a": (0, np.inf)}, "finite"), (3, "scale must be"), ((1, "x"), "scale must be"), ({"a": 5}, "scale of a must be a pair"),
                       ({"a": (1, 2, 3)}, "scale of a must be a pair")):
        with pytest.raises(ValueError, match=match):
            _bounds(values, names, bad)
    values[:, 1] = 2.0
    with pytest.raises(ValueError, match="constant column.*b"):
        _bounds(values, names, (0, 10))


def test_host_errors_that_need_no_device():
    sat, cfg = sat_config()
    with pytest.raises(NotImplementedError, match="one GPU"):
        Ipma(sat, cfg, Scheme.PATH, iterations=100, processes=2)
    _, cfg_nm = sat_config(scale=Scale.NUM)
    with pytest.raises(NotImplementedError, match="non-metric"):
        Ipma(sat, cfg_nm, Scheme.PATH, iterations=100)
    holes = sat.copy()
    holes.iloc[3, holes.columns.get_loc(cfg.filter(sat).columns[0])] = np.nan
    with pytest.raises(NotImplementedError, match="missing"):
        Ipma(holes, cfg, Scheme.PATH, iterations=100)
    first = cfg.filter(sat).columns[0]
    for bad in (dict(targets=["NOPE"]), dict(targets=[]), dict(targets=["IMAG"]), dict(scale=(5, 5)), dict(scale=(4, 6)), dict(scale={"nope": (0, 1)}),
                dict(scale={first: (2, 1)})):
        with pytest.raises(ValueError):
            Ipma(sat, cfg, Scheme.PATH, iterations=100, **bad)
    flat = sat.copy()
    flat[first] = 3.0
    with pytest.raises(ValueError, match="constant column"):
        Ipma(flat, cfg, Scheme.PATH, iterations=100)
    # bca and unknown methods are refused before anything is read
    blank = Ipma.__new__(Ipma)
    with pytest.raises(NotImplementedError, match="no bca"):
        blank.intervals("performance", "bca")
    with pytest.raises(ValueError):
        blank.intervals("performance", "student")
