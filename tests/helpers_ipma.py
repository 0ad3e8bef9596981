"""Shared by the IPMA tests (tests/test_ipma.py, tests/test_gpu_ipma.py) and the tools (tools/ipma_floor.py, tools/ipma_bench.py): the cases, the NumPy mirror
(plspm.ipma._ipma) of one data set in fp64 and in np.longdouble, and the bar of the comparison.  The generators are copied from tests/helpers_tetrad.py, not
imported."""
import numpy as np

import plspm_oracle as orc
from plspm.ipma import FIELDS, _ipma, _layout

SCHEME_ID = {"centroid": 0, "factorial": 1, "path": 2}
# The bar (the project's mirror_bar rule), per field: ten times the largest |fp64 mirror - longdouble mirror| of the field on the same rows, never below
# 1e-12 times the field's scale -- 100 for the performances and the sd of the rescaled score, which live on the 0-100 scale, 1 for the rest.
FLOOR = 1e-12
SCALE = {"perf": 100.0, "sd": 100.0, "mvperf": 100.0, "total_u": 1.0, "direct_u": 1.0, "weight_r": 1.0, "mvimp": 1.0}


def native_model(model, X=None, **options):
    from plspm import _native
    boff = np.concatenate(([0], np.cumsum([len(b) for b in model.blocks]))).astype(np.int32)
    modes = np.array([0 if m == "A" else 1 for m in model.modes], dtype=np.int32)
    nm = _native.NativeModel(boff, model.C.astype(np.uint8), modes, SCHEME_ID[model.scheme], model.scaled, model.max_iter, model.tol, 0)
    for key, value in options.items():
        nm.set_option(key, value)
    if X is not None:
        nm.upload(X, model.mv_order.astype(np.int32))
    return nm


def tri(L):
    """Every LV is driven by the one before it."""
    C = np.zeros((L, L), dtype=np.int64)
    for j in range(1, L):
        C[j, j - 1] = 1
    return C


def pick(width, sizes):
    """Blocks of the given sizes out of a synthetic data set of `width` columns per LV: the first columns of every LV's block."""
    return [np.arange(l * width, l * width + k) for l, k in enumerate(sizes)]


# name -> (X, model, handle options, expected last_solver (None: do not check), expected last_gram_path)
def case(name):
    if name == "k4":
        X, _ = orc.synth(300, tri(2), 4, seed=21)
        return X, orc.Model(pick(4, [3, 4]), tri(2), "AA", "centroid", True), {}, None, 2
    if name == "k3_4_13":
        X, _ = orc.synth(300, tri(3), 13, seed=22)
        return X, orc.Model(pick(13, [3, 4, 13]), tri(3), "AAA", "centroid", True), {}, None, 2
    if name == "lds_65_5":                                   # a block of 65 items: the lanes of phase 2 go round twice, one item in the second round; tile-packed layout, LDS solver
        X, _ = orc.synth(300, tri(2), 65, seed=4)
        X = np.ascontiguousarray(X[:, :70])
        return X, orc.Model([np.arange(65), np.arange(65, 70)], tri(2), "AA", "factorial", True), {}, 1, 2
    if name == "window_66":
        X, _ = orc.synth(300, tri(2), 66, seed=25)
        X = np.ascontiguousarray(X[:, :71])
        return X, orc.Model([np.arange(66), np.arange(66, 71)], tri(2), "AA", "factorial", True), {}, None, None
    if name == "wave_60x6":                                  # dense layout, wave solver: the headline's shape
        X, blocks = orc.synth(400, orc.satisfaction_C(), 10, seed=2)
        return X, orc.Model(blocks, orc.satisfaction_C(), "AAAAAA", "path", True), {}, 7, 2
    if name == "quad_120x12":                                # dense layout, MVs on a second round of the lanes, quad solver
        X, blocks = orc.synth(400, orc.chain_C(12), 10, seed=3)
        return X, orc.Model(blocks, orc.chain_C(12), "A" * 12, "centroid", True), {}, 5, 2
    if name == "packed_40":                                  # the tile-packed layout with every dense solver switched off
        X, blocks = orc.synth(300, tri(4), 10, seed=5)
        return X, orc.Model(blocks, tri(4), "AAAA", "path", False), dict(solver_wave=0, solver_rows=0, solver_quad=0), 1, 2
    if name == "fp64_gram":
        X, blocks = orc.synth(300, tri(3), 4, seed=6)
        return X, orc.Model(blocks, tri(3), "AAA", "centroid", True), dict(gram_path=1), 1, 1
    if name == "mode_b":
        X, blocks = orc.synth(300, tri(3), 4, seed=7)
        return X, orc.Model(blocks, tri(3), "ABA", "path", True), {}, None, 2
    if name == "two_waves":                                  # 16 blocks of 24: 384 MVs, six rounds of the lanes over the MVs, sixteen LV lanes
        X, blocks = orc.synth(500, tri(16), 24, seed=24)
        return X, orc.Model(blocks, tri(16), "A" * 16, "centroid", True), {}, None, None
    raise KeyError(name)


CASES = ["k4", "k3_4_13", "lds_65_5", "window_66", "wave_60x6", "quad_120x12", "packed_40", "fp64_gram", "mode_b", "two_waves"]


def resamples(X, B=9, seed=17):
    return np.random.default_rng(seed).integers(0, X.shape[0], (B, X.shape[0])).astype(np.int32)


def dev_blocks(model):
    """The LV blocks in device column order (MVs grouped by LV, path order): consecutive ranges."""
    off = np.concatenate(([0], np.cumsum([len(b) for b in model.blocks])))
    return [np.arange(off[l], off[l + 1]) for l in range(model.L)]


def observed_bounds(X, model):
    Xd = X[:, model.mv_order]
    return Xd.min(axis=0), Xd.max(axis=0)


def wider_bounds(X, model):
    """Fixed bounds wider than the data: the integers around every column's range, one further out."""
    lo, hi = observed_bounds(X, model)
    return np.floor(lo) - 1.0, np.ceil(hi) + 1.0


def oracle_record(X, model, idx=None):
    """(the bootstrap record of the oracle's fit of the rows idx of X, in device order; its effect pairs).  corr: the full sample's, as the bootstrap has it."""
    rows = X if idx is None else X[np.asarray(idx)]
    r = orc.fit(rows, model, orc.correction(X.shape[0]))
    rec = np.concatenate((r["weights"][model.mv_order], r["r2"], r["total"], r["direct"], r["loadings"][model.mv_order]))
    return rec, [tuple(int(v) for v in p) for p in r["effect_pairs"]]


def mirror_pair(Xr, model, record, pairs, lo, hi, targets=None):
    """(fp64 mirror, longdouble mirror) -- plspm.ipma._ipma's dicts -- of the rows Xr [n, P] in device column order with that data set's bootstrap record."""
    blocks = dev_blocks(model)
    return (_ipma(Xr, blocks, record, pairs, lo, hi, targets, np.float64),
            _ipma(Xr, blocks, np.asarray(record, dtype=np.longdouble), pairs, np.asarray(lo, dtype=np.longdouble), np.asarray(hi, dtype=np.longdouble), targets, np.longdouble))


def field_difference(m64, mld):
    """Per field the largest |fp64 mirror - longdouble mirror| over the entries both have finite (0 for an empty field)."""
    out = {}
    for name in FIELDS:
        a, b = m64[name].ravel().astype(np.longdouble), mld[name].ravel()
        ok = np.isfinite(a) & np.isfinite(b)
        out[name] = float(np.max(np.abs(a[ok] - b[ok]))) if ok.any() else 0.0
    return out


def field_bars(m64, mld):
    """Per field: ten times the mirror difference, at least FLOOR times the field's scale (absolute)."""
    diff = field_difference(m64, mld)
    return {name: max(10.0 * diff[name], FLOOR * SCALE[name]) for name in FIELDS}


def check_record(values, m64, mld, tag):
    """A record [W] against the fp64 mirror, field by field; the same entries finite.  Returns {field: largest difference}."""
    P, L = m64["weight_r"].shape[0], m64["perf"].shape[0]
    at, width = _layout(P, L, m64["total_u"].shape[0], m64["mvimp"].shape[0])
    assert values.shape == (width,), (tag, values.shape, width)
    bars, worst = field_bars(m64, mld), {}
    for name in FIELDS:
        got, want = values[at[name]], m64[name].ravel()
        assert np.array_equal(np.isfinite(got), np.isfinite(want)), "%s %s: other entries finite than in the mirror" % (tag, name)
        ok = np.isfinite(want)
        worst[name] = float(np.max(np.abs(got[ok] - want[ok]))) if ok.any() else 0.0
        assert worst[name] <= bars[name], "%s %s: max |record - mirror| %.3e above the bar %.3e" % (tag, name, worst[name], bars[name])
    return worst


def status_is_decided(m64, mld):
    """The mirror's status is the record's wherever its smallest |weight_r_p| exceeds the bar of the weights (a weight nearer to zero may take either sign)."""
    return not np.isfinite(m64["min_abs_weight"]) or m64["min_abs_weight"] > field_bars(m64, mld)["weight_r"]


def host_input(X, sizes, pairs, record, lo, hi, mask=None):
    """The text tests/ipma_host reads: the rows X [n, P] in device order, blocks of `sizes`, the effect pairs, the bootstrap record, the bounds."""
    boff = np.concatenate(([0], np.cumsum(sizes)))
    fmt = lambda row: " ".join(repr(float(v)) for v in row)
    lines = ["%d %d" % (len(sizes), len(pairs)), " ".join(str(int(v)) for v in boff),
             " ".join(str(int(f)) for f, _ in pairs), " ".join(str(int(t)) for _, t in pairs),
             "0" if mask is None else "1 " + " ".join(str(int(v)) for v in mask), fmt(lo), fmt(hi), fmt(record), "%d" % X.shape[0]]
    lines += [fmt(row) for row in X]
    return "\n".join(lines) + "\n"
