"""Shared by the structural tests (tests/test_gpu_structural.py) and the floor measurement (tools/structural_floor.py): the cases, the NumPy mirror
(plspm.structural._structural) of one replicate in fp64 and in np.longdouble, the bar of the comparison, the same statistics from the oracle's scores by
least squares, and the figure behind the bar of that cross-check.  The generators are copied from tests/helpers_plsc.py, not imported."""
import numpy as np

import plspm_oracle as orc
from plspm.plsc import _effect_pairs
from plspm.quality import _quality
from plspm.structural import _structural

SCHEME_ID = {"centroid": 0, "factorial": 1, "path": 2}
# The absolute floor of the bar: the largest |fp64 mirror - longdouble mirror| over every case's nine resamples and full sample, measured on the CPU with the
# oracle's construct correlations and direct effects in place of the device's (tools/structural_floor.py: 2.2e-15, the dense 7-LV case), and never
# below 1e-12.
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


def dense(L):
    """Every LV is driven by all the LVs before it."""
    return np.tril(np.ones((L, L), dtype=np.int64), -1)


CASES = ["single_items", "satisfaction", "fan_in_10", "fan_in_11", "fan_in_20", "tri_33", "dense_7", "mode_b"]


def case(name):
    """(X, model) of a case.  Every one of the nine resamples (``resamples``) and the full sample of every case has status 0 and finite values by the oracle
    alone (tools/structural_floor.py asserts it)."""
    if name == "single_items":
        X, blocks = orc.synth(300, tri(2), 1, seed=1)
        return X, orc.Model(blocks, tri(2), "AA", "centroid", True)
    if name == "satisfaction":
        X, blocks = orc.synth(400, orc.satisfaction_C(), 10, seed=2)
        return X, orc.Model(blocks, orc.satisfaction_C(), "AAAAAA", "path", True)
    if name == "fan_in_10":
        X, blocks = orc.synth(1000, fan_in(10), 2, seed=8)
        return X, orc.Model(blocks, fan_in(10), "A" * 10, "path", True)
    if name == "fan_in_11":
        X, blocks = orc.synth(1000, fan_in(11), 2, seed=10)
        return X, orc.Model(blocks, fan_in(11), "A" * 11, "path", True)
    if name == "fan_in_20":                                  # (centroid scheme: the solver's own iteration has no 19-predecessor regressions, its inner model has one)
        X, blocks = orc.synth(1000, fan_in(20), 2, seed=12)
        return X, orc.Model(blocks, fan_in(20), "A" * 20, "centroid", True)
    if name == "tri_33":
        X, blocks = orc.synth(400, tri(33), 2, seed=9)
        return X, orc.Model(blocks, tri(33), "A" * 33, "centroid", True)
    if name == "dense_7":
        X, blocks = orc.synth(400, dense(7), 4, seed=11)
        return X, orc.Model(blocks, dense(7), "A" * 7, "centroid", True)
    if name == "mode_b":
        X, blocks = orc.synth(300, tri(3), 4, seed=7)
        return X, orc.Model(blocks, tri(3), "ABA", "path", True)
    raise KeyError(name)


def resamples(X, B=9, seed=17):
    return np.random.default_rng(seed).integers(0, X.shape[0], (B, X.shape[0])).astype(np.int32)


def dev_blocks(model):
    """The LV blocks in device column order (MVs grouped by LV, path order): consecutive ranges."""
    off = np.concatenate(([0], np.cumsum([len(b) for b in model.blocks])))
    return [np.arange(off[l], off[l + 1]) for l in range(model.L)]


def square(lv_cor, L):
    """The assessment record's lv_cor [npairs] (i < j, i-major) as the L x L matrix rc, diagonal 1."""
    rc = np.eye(L, dtype=np.asarray(lv_cor).dtype)
    rc[np.triu_indices(L, 1)] = lv_cor
    return rc + np.triu(rc, 1).T


def record_direct(model, record):
    """The direct entries [n_eff] of a bootstrap record (weights | r2 | total | direct | loadings)."""
    ne = len(_effect_pairs(model.C))
    start = model.P + model.L + ne
    return record[start:start + ne]


def mirror_pair(model, lv_cor, direct):
    """(fp64 mirror, longdouble mirror) -- plspm.structural._structural's dicts -- on one replicate's construct correlations lv_cor [npairs] and direct
    effects [n_eff]: the same fp64 numbers, taken to np.longdouble for the second."""
    m64 = _structural(square(np.asarray(lv_cor, dtype=np.float64), model.L), model.C, np.asarray(direct, dtype=np.float64))
    mld = _structural(square(np.asarray(lv_cor, dtype=np.longdouble), model.L), model.C, np.asarray(direct, dtype=np.longdouble))
    return m64, mld


def mirror_difference(m64, mld):
    return float(np.max(np.abs(m64["record"].astype(np.longdouble) - mld["record"]))) if m64["record"].size else 0.0


def mirror_bar(m64, mld, floor=FLOOR):
    """Ten times the largest difference between the fp64 and the longdouble mirror on the same inputs, at least `floor` (absolute)."""
    return max(10.0 * mirror_difference(m64, mld), floor)


def oracle_lv_cor(Xr, model, w, lam):
    """The construct correlations [npairs] of the rows Xr (device column order) under the weights w and loadings lam: plspm.quality._quality's."""
    P = Xr.shape[1]
    return _quality(np.corrcoef(Xr, rowvar=False).reshape(P, P), w, lam, dev_blocks(model), model.modes, sd=Xr.std(axis=0))["lv_cor"]


def oracle_fit_record(X, model, rows, n_all):
    """(the oracle's fit of X[rows], its record in the device layout)."""
    f = orc.fit(X[rows], model, orc.correction(n_all))
    return f, np.concatenate((f["weights"][model.mv_order], f["r2"], f["total"], f["direct"], f["loadings"][model.mv_order]))


def lstsq_statistics(model, scores, path_coef):
    """The structural record from LV scores [n, L] by numpy.linalg.lstsq, with and without the predictor, and the path coefficients path_coef [L, L]: nothing
    of the mirror's regression, of rc, or of the device's order of operations."""
    from plspm.structural import _chains
    Y = scores - scores.mean(axis=0)

    def r2(col, S):
        if len(S) == 0:
            return 0.0
        beta = np.linalg.lstsq(Y[:, S], Y[:, col], rcond=None)[0]
        resid = Y[:, col] - Y[:, S] @ beta
        return 1.0 - (resid @ resid) / (Y[:, col] @ Y[:, col])
    f2, vif = [], []
    for i, j in [(f, t) for f, t in _effect_pairs(model.C) if model.C[t, f]]:
        pred = np.flatnonzero(model.C[j]).tolist()
        S = [k for k in pred if k != i]
        full = r2(j, pred)
        f2.append((full - r2(j, S)) / (1.0 - full))
        vif.append(1.0 / (1.0 - r2(i, S)))
    spec = []
    for chain in _chains(model.C):
        value = path_coef[chain[1], chain[0]]
        for a, b in zip(chain[1:-1], chain[2:]):
            value = value * path_coef[b, a]
        spec.append(value)
    return np.array(f2 + vif + spec, dtype=np.float64)


def perturbation_figure(X, model, idx, draws=20, rtol=1e-8, atol=1e-11, seed=0):
    """How far the structural statistics move when the oracle's records move inside the record bar (|d| <= atol + rtol |x|, uniform draws): the largest
    absolute change of any statistic over the resamples and draws (helpers_quality.perturbation_figure's method).  The statistics are the mirror's on the
    construct correlations of the record's weights and loadings and on the record's direct effects."""
    rng = np.random.default_rng(seed)
    P, worst = model.P, 0.0
    for r in range(idx.shape[0]):
        Xr = X[idx[r]][:, model.mv_order]
        _, rec = oracle_fit_record(X, model, idx[r], X.shape[0])
        base = _structural(square(oracle_lv_cor(Xr, model, rec[:P], rec[-P:]), model.L), model.C, record_direct(model, rec))["record"]
        for _ in range(draws):
            moved = rec + rng.uniform(-1.0, 1.0, rec.shape[0]) * (atol + rtol * np.abs(rec))
            stat = _structural(square(oracle_lv_cor(Xr, model, moved[:P], moved[-P:]), model.L), model.C, record_direct(model, moved))["record"]
            worst = max(worst, float(np.max(np.abs(stat - base))))
    return worst
