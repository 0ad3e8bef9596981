"""Shared by the tetrad tests (tests/test_tetrad.py, tests/test_gpu_tetrad.py) and the bench (tools/tetrad_bench.py): the cases, the NumPy mirror
(plspm.tetrad._tetrads) of one data set in fp64 and in np.longdouble, and the bar of the comparison.  The generators are copied from
tests/test_gpu_quality.py and tests/helpers_structural.py, not imported."""
import numpy as np

import plspm_oracle as orc
from plspm.tetrad import _tetrads

SCHEME_ID = {"centroid": 0, "factorial": 1, "path": 2}
# The absolute floor of the bar (the project's mirror_bar rule): ten times the largest |fp64 mirror - longdouble mirror| on the same case, never below 1e-12.
FLOOR = 1e-12
MATRICES = ("correlation", "covariance")


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


# name -> (X, model, handle options, tetrad set, expected last_solver (None: do not check), expected last_gram_path)
def case(name):
    if name == "k4":                                         # the only testable block has four items
        X, _ = orc.synth(300, tri(2), 4, seed=21)
        return X, orc.Model(pick(4, [3, 4]), tri(2), "AA", "centroid", True), {}, "basis", None, 2
    if name == "k3_4_13":                                    # the block of 3 is skipped; 2 + 65 basis tetrads: a wave goes round twice
        X, _ = orc.synth(300, tri(3), 13, seed=22)
        return X, orc.Model(pick(13, [3, 4, 13]), tri(3), "AAA", "centroid", True), {}, "basis", None, 2
    if name == "all_7":                                      # 70 tetrads of one block
        X, _ = orc.synth(300, tri(2), 7, seed=23)
        return X, orc.Model(pick(7, [2, 7]), tri(2), "AA", "centroid", True), {}, "all", None, 2
    if name == "lds_65_5":                                   # one block of 65 items: its 64 staged columns fill one window, every lane busy; tile-packed layout with an odd tile count, LDS solver
        X, _ = orc.synth(300, tri(2), 65, seed=4)
        X = np.ascontiguousarray(X[:, :70])
        return X, orc.Model([np.arange(65), np.arange(65, 70)], tri(2), "AA", "factorial", True), {}, "basis", 1, 2
    if name == "window_66":                                  # 66 items: 65 staged columns, the last one in a second trip of the window loop (64 + 2: the first such size)
        X, _ = orc.synth(300, tri(2), 66, seed=25)
        X = np.ascontiguousarray(X[:, :71])
        return X, orc.Model([np.arange(66), np.arange(66, 71)], tri(2), "AA", "factorial", True), {}, "basis", None, None
    if name == "wave_60x6":                                  # dense layout, wave solver: the headline's shape
        X, blocks = orc.synth(400, orc.satisfaction_C(), 10, seed=2)
        return X, orc.Model(blocks, orc.satisfaction_C(), "AAAAAA", "path", True), {}, "basis", 7, 2
    if name == "quad_120x12":                                # dense layout, MVs on a second window, quad solver
        X, blocks = orc.synth(400, orc.chain_C(12), 10, seed=3)
        return X, orc.Model(blocks, orc.chain_C(12), "A" * 12, "centroid", True), {}, "basis", 5, 2
    if name == "packed_40":                                  # the tile-packed layout with every dense solver switched off
        X, blocks = orc.synth(300, tri(4), 10, seed=5)
        return X, orc.Model(blocks, tri(4), "AAAA", "path", False), dict(solver_wave=0, solver_rows=0, solver_quad=0), "basis", 1, 2
    if name == "fp64_gram":
        X, blocks = orc.synth(300, tri(3), 4, seed=6)
        return X, orc.Model(blocks, tri(3), "AAA", "centroid", True), dict(gram_path=1), "basis", 1, 1
    if name == "mode_b":
        X, blocks = orc.synth(300, tri(3), 4, seed=7)
        return X, orc.Model(blocks, tri(3), "ABA", "path", True), {}, "basis", None, 2
    if name == "two_waves":                                  # 16 blocks of 24: 2 P + T_tri + 1 = 5,185 doubles a wave, four of them exceed 160 KiB
        X, blocks = orc.synth(500, tri(16), 24, seed=24)
        return X, orc.Model(blocks, tri(16), "A" * 16, "centroid", True), {}, "basis", None, None
    raise KeyError(name)


CASES = ["k4", "k3_4_13", "all_7", "lds_65_5", "window_66", "wave_60x6", "quad_120x12", "packed_40", "fp64_gram", "mode_b", "two_waves"]


def resamples(X, B=9, seed=17):
    return np.random.default_rng(seed).integers(0, X.shape[0], (B, X.shape[0])).astype(np.int32)


def dev_blocks(model):
    """The LV blocks in device column order (MVs grouped by LV, path order): consecutive ranges."""
    off = np.concatenate(([0], np.cumsum([len(b) for b in model.blocks])))
    return [np.arange(off[l], off[l + 1]) for l in range(model.L)]


def mirror_pair(Xr, model, tetrads, matrix):
    """(fp64 mirror, longdouble mirror) -- plspm.tetrad._tetrads' dicts -- of the rows Xr [n, P] in device column order."""
    blocks = dev_blocks(model)
    return _tetrads(Xr, blocks, tetrads, matrix, np.float64), _tetrads(Xr, blocks, tetrads, matrix, np.longdouble)


def mirror_difference(m64, mld):
    return float(np.max(np.abs(m64["tetrads"].astype(np.longdouble) - mld["tetrads"]))) if m64["tetrads"].size else 0.0


def mirror_bar(m64, mld, floor=FLOOR):
    """Ten times the largest difference between the fp64 and the longdouble mirror on the same rows, at least `floor` (absolute)."""
    return max(10.0 * mirror_difference(m64, mld), floor)


def one_factor(n, k, seed):
    """n rows of k items of ONE common factor: loadings linspace(0.5, 0.9, k), unit-variance noise scaled by 0.6 -- every tetrad vanishes in the population."""
    rng = np.random.default_rng(seed)
    eta = rng.standard_normal(n)
    return eta[:, None] * np.linspace(0.5, 0.9, k)[None, :] + 0.6 * rng.standard_normal((n, k))


def two_clusters(n, k, seed, rho=0.2):
    """n rows of k items that are causes of two different things: the first half loads on one factor, the rest on another, the factors correlated `rho`.
    tau(1, 2, i, j) with i, j in the second half is r_12 r_ij - r_1i r_2j, far from zero: not tetrad-consistent."""
    rng = np.random.default_rng(seed)
    f = rng.standard_normal((n, 2))
    f[:, 1] = rho * f[:, 0] + np.sqrt(1.0 - rho * rho) * f[:, 1]
    which = (np.arange(k) >= k // 2).astype(int)
    return f[:, which] * 0.8 + 0.6 * rng.standard_normal((n, k))
