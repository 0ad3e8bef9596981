"""Shared by the PLSc tests (tests/test_gpu_plsc.py) and the floor measurement (tools/plsc_floor.py): the cases, the inputs of the NumPy mirror
(plspm.plsc._plsc) for one resample in fp64 and in np.longdouble, and the bar of the comparison.  The first seven cases are built like those of
tests/test_gpu_quality.py (the generators are copied, not imported from the test file)."""
import numpy as np

import plspm_oracle as orc
from plspm.plsc import _plsc

SCHEME_ID = {"centroid": 0, "factorial": 1, "path": 2}
ANY_SOLVER, ANY_DENSE = "any", None
# The absolute floor of the bar: the largest |fp64 mirror - longdouble mirror| over every case's nine resamples and full sample, measured on the CPU with the
# oracle's weights and loadings (tools/plsc_floor.py: 3.7e-15, the nine-predecessor case), and never below 1e-12.
FLOOR = 1e-12


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


def fan_in(L):
    """The last LV is driven by all the others."""
    C = np.zeros((L, L), dtype=np.int64)
    C[L - 1, :L - 1] = 1
    return C


CASES = ["single_items", "wave_60x6", "quad_120x12", "lds_65_5", "packed_40", "fp64_gram", "mode_b", "nine_predecessors", "lv_33", "mixed_mask"]


def case(name):
    """(X, model, handle options, expected last_solver (ANY_DENSE: any dense one, ANY_SOLVER: not checked), expected last_gram_path, factor mask or None)."""
    if name == "single_items":
        X, blocks = orc.synth(300, tri(2), 1, seed=1)
        return X, orc.Model(blocks, tri(2), "AA", "centroid", True), {}, ANY_DENSE, 2, None
    if name in ("wave_60x6", "mixed_mask"):
        X, blocks = orc.synth(400, orc.satisfaction_C(), 10, seed=2)
        return X, orc.Model(blocks, orc.satisfaction_C(), "AAAAAA", "path", True), {}, 7, 2, ([1, 0, 1, 1, 0, 1] if name == "mixed_mask" else None)
    if name == "quad_120x12":
        X, blocks = orc.synth(400, orc.chain_C(12), 10, seed=3)
        return X, orc.Model(blocks, orc.chain_C(12), "A" * 12, "centroid", True), {}, 5, 2, None
    if name == "lds_65_5":
        X, _ = orc.synth(300, tri(2), 65, seed=4)
        X = np.ascontiguousarray(X[:, :70])
        return X, orc.Model([np.arange(65), np.arange(65, 70)], tri(2), "AA", "factorial", True), {}, 1, 2, None
    if name == "packed_40":
        X, blocks = orc.synth(300, tri(4), 10, seed=5)
        return X, orc.Model(blocks, tri(4), "AAAA", "path", False), dict(solver_wave=0, solver_rows=0, solver_quad=0), 1, 2, None
    if name == "fp64_gram":
        X, blocks = orc.synth(300, tri(3), 4, seed=6)
        return X, orc.Model(blocks, tri(3), "AAA", "centroid", True), dict(gram_path=1), 1, 1, None
    if name == "mode_b":
        X, blocks = orc.synth(300, tri(3), 4, seed=7)
        return X, orc.Model(blocks, tri(3), "ABA", "path", True), {}, ANY_DENSE, 2, None
    if name == "nine_predecessors":
        X, blocks = orc.synth(1000, fan_in(10), 2, seed=8)      # (two-item blocks under the path scheme: at 400 rows a resample can give an exogenous block weights of opposite signs and a negative rho_A)
        return X, orc.Model(blocks, fan_in(10), "A" * 10, "path", True), {}, ANY_SOLVER, 2, None
    if name == "lv_33":
        X, blocks = orc.synth(400, tri(33), 2, seed=9)
        return X, orc.Model(blocks, tri(33), "A" * 33, "centroid", True), {}, ANY_SOLVER, 2, None
    raise KeyError(name)


def resamples(X, B=9, seed=17):
    return np.random.default_rng(seed).integers(0, X.shape[0], (B, X.shape[0])).astype(np.int32)


def dev_blocks(model):
    """The LV blocks in device column order (MVs grouped by LV, path order): consecutive ranges."""
    off = np.concatenate(([0], np.cumsum([len(b) for b in model.blocks])))
    return [np.arange(off[l], off[l + 1]) for l in range(model.L)]


def mirror_pair(Xr, model, w, lam, factor):
    """(fp64 mirror, longdouble mirror) -- plspm.plsc._plsc's dicts -- on the rows Xr (device column order) with the weights w and loadings lam: the fp64 one is
    fed NumPy's correlation matrix and standard deviations of Xr, the longdouble one the same quantities accumulated in np.longdouble."""
    blocks = dev_blocks(model)
    P = Xr.shape[1]
    m64 = _plsc(np.corrcoef(Xr, rowvar=False).reshape(P, P), w, lam, blocks, model.modes, model.C, factor, sd=Xr.std(axis=0))
    XL = Xr.astype(np.longdouble)
    XL = XL - XL.mean(axis=0)
    CL = XL.T @ XL / np.longdouble(Xr.shape[0])
    sdL = np.sqrt(np.diag(CL))
    RL = CL / np.outer(sdL, sdL)
    mld = _plsc(RL, np.asarray(w, dtype=np.longdouble), np.asarray(lam, dtype=np.longdouble), blocks, model.modes, model.C, factor, sd=sdL)
    return m64, mld


def mirror_difference(m64, mld):
    return float(np.max(np.abs(m64["record"].astype(np.longdouble) - mld["record"])))


def mirror_bar(m64, mld, floor=FLOOR):
    """Ten times the largest difference between the fp64 and the longdouble mirror on the same inputs, at least `floor` (absolute)."""
    return max(10.0 * mirror_difference(m64, mld), floor)


def negative_pair_model(n=300, seed=18):
    """Two LVs; the first block's two items correlate at about -0.1 with each other and positively with the second block's four items: its rho_A is negative."""
    rng = np.random.default_rng(seed)
    eta = rng.standard_normal(n)
    z = rng.standard_normal((n, 2))
    e0, e1 = z[:, 0], -0.28 * z[:, 0] + np.sqrt(1.0 - 0.28 ** 2) * z[:, 1]
    X = np.empty((n, 6))
    X[:, 0], X[:, 1] = 0.4 * eta + e0, 0.4 * eta + e1
    X[:, 2:] = eta[:, None] * np.linspace(0.6, 0.9, 4)[None, :] + 0.6 * rng.standard_normal((n, 4))
    return X, orc.Model([np.arange(2), np.arange(2, 6)], tri(2), "AA", "centroid", True)
