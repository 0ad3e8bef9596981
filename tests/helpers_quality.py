"""Shared by the assessment tests (tests/test_gpu_quality.py): the inputs of the NumPy mirror (plspm.quality._quality) for one resample, in fp64
and in np.longdouble, and the figure behind the bar of the comparison with the oracle's fits."""
import numpy as np

import plspm_oracle as orc
from plspm.quality import _quality, _record


def dev_blocks(model):
    """The LV blocks in device column order (MVs grouped by LV, path order): consecutive ranges."""
    off = np.concatenate(([0], np.cumsum([len(b) for b in model.blocks])))
    return [np.arange(off[l], off[l + 1]) for l in range(model.L)]


def mirror_pair(Xr, model, w, lam):
    """(fp64 record, longdouble record) of the mirror on the rows Xr (device column order) with the weights w and loadings lam: the fp64 one is fed NumPy's
    correlation matrix and standard deviations of Xr, the longdouble one the same quantities accumulated in np.longdouble."""
    blocks = dev_blocks(model)
    m64 = _record(_quality(np.corrcoef(Xr, rowvar=False).reshape(Xr.shape[1], Xr.shape[1]), w, lam, blocks, model.modes, sd=Xr.std(axis=0)))
    XL = Xr.astype(np.longdouble)
    XL = XL - XL.mean(axis=0)
    CL = XL.T @ XL / np.longdouble(Xr.shape[0])
    sdL = np.sqrt(np.diag(CL))
    RL = CL / np.outer(sdL, sdL)
    mld = _record(_quality(RL, np.asarray(w, dtype=np.longdouble), np.asarray(lam, dtype=np.longdouble), blocks, model.modes, sd=sdL))
    return m64, mld


def mirror_bar(m64, mld, floor=1e-12):
    """Ten times the largest difference between the fp64 and the longdouble mirror on the same inputs, at least `floor` (absolute)."""
    return max(10.0 * float(np.max(np.abs(m64.astype(np.longdouble) - mld))), floor)


def oracle_records(X, model, idx):
    """The oracle's fits of X[idx[r]] in the device record layout (tests/helpers_mga.oracle_record's), their iteration counts."""
    rows, iters = [], []
    for r in range(idx.shape[0]):
        f = orc.fit(X[idx[r]], model, orc.correction(X.shape[0]))
        rows.append(np.concatenate((f["weights"][model.mv_order], f["r2"], f["total"], f["direct"], f["loadings"][model.mv_order])))
        iters.append(f["iterations"])
    return np.array(rows), np.array(iters)


def perturbation_figure(X, model, idx, records, draws=20, rtol=1e-8, atol=1e-11, seed=0):
    """How far the criteria move when the oracle's records move inside the record bar (|d| <= atol + rtol |x|, uniform draws): the largest absolute
    change of any criterion over the resamples and draws (DESIGN.md 5l's method)."""
    rng = np.random.default_rng(seed)
    P, worst = model.P, 0.0
    for r in range(idx.shape[0]):
        Xr = X[idx[r]][:, model.mv_order]
        R, sd = np.corrcoef(Xr, rowvar=False), Xr.std(axis=0)
        blocks = dev_blocks(model)
        base = _record(_quality(R, records[r, :P], records[r, -P:], blocks, model.modes, sd=sd))
        for _ in range(draws):
            rec = records[r] + rng.uniform(-1.0, 1.0, records.shape[1]) * (atol + rtol * np.abs(records[r]))
            moved = _record(_quality(R, rec[:P], rec[-P:], blocks, model.modes, sd=sd))
            worst = max(worst, float(np.max(np.abs(moved - base))))
    return worst
