"""Shared by the model-fit tests (tests/test_modelfit.py, tests/test_gpu_modelfit.py) and the CPU measurements behind their bars (tools/modelfit_floor.py):
the closed-form population, the NumPy mirror (plspm.modelfit._model_fit on plspm.plsc._plsc) of one data set in fp64 and in np.longdouble, and the bars.
The shapes are tests/helpers_plsc.py's."""
import numpy as np

import plspm_oracle as orc
from helpers_plsc import dev_blocks
from plspm.modelfit import _model_fit
from plspm.plsc import _default_mask, _plsc

# The absolute floor of the kernel-against-mirror bar: the largest |fp64 mirror - longdouble mirror| over every case's nine resamples and full sample, measured
# on the CPU with the oracle's weights and loadings (tools/modelfit_floor.py: 5.0e-14, lds_65_5), and never below 1e-12.
FLOOR = 1e-12

# the closed-form population of tests/test_plsc.py: true loadings (blocks of 2, 3 and 5 items) and path coefficients of a three-LV model
LAMBDA = [np.array([0.8, 0.6]), np.array([0.9, 0.7, 0.5]), np.array([0.85, 0.75, 0.65, 0.55, 0.45])]
B21, B31, B32 = 0.5, 0.3, 0.4                     # LV 0 -> 1, 0 -> 2, 1 -> 2
PATH = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0]])
PATH_WITHOUT_02 = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]])
POP_BLOCKS = [np.arange(0, 2), np.arange(2, 5), np.arange(5, 10)]


def population(dtype):
    """(R, blocks, w, lam, phi) of the population in `dtype`: R = Lambda Phi Lambda' with a unit diagonal, w the population Mode-A weights (proportional to
    lambda), lam the loadings R v of the standardised composites."""
    dt = np.dtype(dtype).type
    lams = [l.astype(dtype) for l in LAMBDA]
    b21, b31, b32 = dt(B21), dt(B31), dt(B32)
    phi = np.eye(3, dtype=dtype)
    phi[0, 1] = phi[1, 0] = b21
    phi[0, 2] = phi[2, 0] = b31 + b32 * b21
    phi[1, 2] = phi[2, 1] = b31 * b21 + b32
    Lam = np.zeros((10, 3), dtype=dtype)
    for l, blk in enumerate(POP_BLOCKS):
        Lam[blk, l] = lams[l]
    R = Lam @ phi @ Lam.T
    R[np.diag_indices(10)] = dt(1)
    w = np.concatenate(lams)
    lam = np.empty(10, dtype=dtype)
    for blk in POP_BLOCKS:
        v = w[blk] / np.sqrt(w[blk] @ R[np.ix_(blk, blk)] @ w[blk])
        lam[blk] = R[np.ix_(blk, blk)] @ v
    return R, POP_BLOCKS, w, lam, phi


def population_sample(n, seed):
    """n Gaussian rows whose population correlation matrix is population()'s R."""
    R = population(np.float64)[0]
    return np.random.default_rng(seed).standard_normal((n, 10)) @ np.linalg.cholesky(R).T


def population_model(C):
    return orc.Model(POP_BLOCKS, C, "AAA", "path", True)


def mask_of(model, factor):
    """The 0 / 1 mask in LV order (None: PLSc's default, every Mode-A block of two items or more)."""
    return _default_mask(dev_blocks(model), model.modes) if factor is None else np.asarray(factor).astype(bool)


def correlations(Xr, dtype):
    """(R, sd) of the rows Xr: NumPy's own in fp64, the same quantities accumulated in np.longdouble otherwise."""
    P = Xr.shape[1]
    if np.dtype(dtype) == np.float64:
        return np.corrcoef(Xr, rowvar=False).reshape(P, P), Xr.std(axis=0)
    XL = Xr.astype(dtype)
    XL = XL - XL.mean(axis=0)
    CL = XL.T @ XL / np.dtype(dtype).type(Xr.shape[0])
    sd = np.sqrt(np.diag(CL))
    return CL / np.outer(sd, sd), sd


def mirror_fit(Xr, model, w, lam, factor, dtype=np.float64):
    """plspm.modelfit._model_fit's dict on the rows Xr (device column order) with the weights w and loadings lam; beside it the _plsc dict it was built on."""
    blocks, mask = dev_blocks(model), mask_of(model, factor)
    R, sd = correlations(Xr, dtype)
    plsc = _plsc(R, np.asarray(w, dtype=dtype), np.asarray(lam, dtype=dtype), blocks, model.modes, model.C, mask, sd=sd)
    return _model_fit(R, plsc, blocks, model.C, mask), plsc


def mirror_fit_pair(Xr, model, w, lam, factor):
    """(fp64 mirror, longdouble mirror) on the same inputs."""
    return mirror_fit(Xr, model, w, lam, factor)[0], mirror_fit(Xr, model, w, lam, factor, np.longdouble)[0]


def mirror_difference(m64, mld):
    return float(np.max(np.abs(m64["record"].astype(np.longdouble) - mld["record"])))


def mirror_bar(m64, mld, floor=FLOOR):
    """Ten times the largest difference between the fp64 and the longdouble mirror on the same inputs, at least `floor` (absolute)."""
    return max(10.0 * mirror_difference(m64, mld), floor)


def oracle_fit(Xr, model):
    """The oracle's fit of the rows Xr (data column order): (weights, loadings) in device column order, and the oracle's record."""
    f = orc.fit(Xr, model, orc.correction(Xr.shape[0]))
    return f["weights"][model.mv_order], f["loadings"][model.mv_order], f


def oracle_model_fit(Xr, model, factor, dtype=np.float64):
    """The mirror on the oracle's fit of the rows Xr (data column order)."""
    w, lam, _ = oracle_fit(Xr, model)
    return mirror_fit(Xr[:, model.mv_order], model, w, lam, factor, dtype)[0]


def perturbation_bar(Xr, model, w, lam, factor, draws=20, seed=5, rtol=1e-8, atol=1e-11):
    """Ten times the largest movement of a statistic when the weights and loadings are perturbed inside the project's record bar (rtol, atol): `draws` draws."""
    rng = np.random.default_rng(seed)
    base = mirror_fit(Xr, model, w, lam, factor)[0]["record"]
    worst = 0.0
    for _ in range(draws):
        wp = w + rng.uniform(-1, 1, w.shape) * (atol + rtol * np.abs(w))
        lp = lam + rng.uniform(-1, 1, lam.shape) * (atol + rtol * np.abs(lam))
        worst = max(worst, float(np.max(np.abs(mirror_fit(Xr, model, wp, lp, factor)[0]["record"] - base))))
    return 10.0 * worst
