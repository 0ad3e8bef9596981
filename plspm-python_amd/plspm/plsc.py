"""Consistent PLS (PLSc; Dijkstra and Henseler 2015) with bootstrap inference on the GPU (not in the reference): path coefficients, R squared,
effects, loadings and construct correlations corrected for attenuation, for the latent variables that are common factors.

Plain PLS is inconsistent for reflective common factors: construct correlations and path coefficients are attenuated and loadings inflated,
however many observations there are.  PLSc divides the construct correlations by the composites' reliabilities rho_A and estimates the inner
model on the corrected correlations.  Every replicate's record is computed on the device, behind the assessment kernel whose rho_a and
construct correlations it reads (include/plspm_hip.h ``plspm_plsc_*``).  This project's definitions, from the quantities of
``plspm.quality`` (v normalised per block so that v_l' R_ll v_l = 1, the fit's sign sigma_l, rho_a, lv_cor):

    factor mask   which LVs are common factors; default: every Mode-A block of two items or more (a Mode-B or single-item LV cannot be one)
    Q_l           rho_a[l] for a factor, 1 otherwise
    rc_ij         lv_cor_ij / sqrt(Q_i Q_j) for i != j, rc_ii = 1
    inner model   the solver's own on rc in place of the score covariance: per endogenous LV the normal equations on its predecessors (solved if
                  the Cholesky pivots pass PLSPM_PIVOT_RTOL, otherwise by the pseudo-inverse of the eigenvalues above PLSPM_EIG_RTOL lambda_max),
                  R2_j = beta' rc_pj, indirect effects B^2 + B^3 + ..., total = direct + indirect
    loadings      factor l: sigma_l v_p sqrt(Q_l) / (v_l' v_l); any other LV: the fit's.  Weights: the fit's.
    record        weights[P] | r2[L] | total[n_eff] | direct[n_eff] | loadings[P] | lv_cor_c[npairs]   (n_eff: the pairs f != t with a path f -> ... -> t,
                  from-major; npairs = L (L - 1) / 2, i < j, i-major)
    inadmissible  (status 4, NaN everywhere, not used) a factor's rho_a is not finite or <= 0, or some |rc_ij| is not below 1

With an all-zero mask the record is the bootstrap's up to rounding.  ``_plsc`` below is the same statistic in NumPy: the checker of the kernel.
Scope: metric data without missing cells and without higher-order constructs, one GPU; no bca intervals (the jackknife writes no PLSc records).
"""
import os

import numpy as np
import pandas as pd

import plspm.config as c
import plspm.weights as pw
from plspm import _native
from plspm.bootstrap import INTERVAL_COLUMNS, INTERVAL_METHODS, SUMMARY_COLUMNS
from plspm.estimator import Estimator
from plspm.quality import MIN_ITERATIONS, _quality, _unsupported
from plspm.scheme import Scheme

PIVOT_RTOL = 1e-13              # csrc/solver_core.h PLSPM_PIVOT_RTOL
EIG_RTOL = 1e-12                # csrc/solver_core.h PLSPM_EIG_RTOL
STATUS_OK, STATUS_SINGULAR, STATUS_NONFINITE, STATUS_INADMISSIBLE = 0, 2, 3, 4


def _effect_pairs(C):
    """The (from, to) pairs of the device's effect rows: f != t with a path f -> ... -> t, from-major (C[i, j] = 1 iff LV j -> LV i)."""
    L = C.shape[0]
    reach = (np.asarray(C) != 0)
    for k in range(L):
        reach = reach | (reach[:, [k]] & reach[[k], :])
    return [(f, t) for f in range(L) for t in range(L) if f != t and reach[t, f]]


def _default_mask(blocks, modes):
    return np.array([len(b) >= 2 and modes[l] in ("A", 0) for l, b in enumerate(blocks)], dtype=bool)


def _regress(A, b):
    """The device's rule for A x = b: solve if every Cholesky pivot d_j > PIVOT_RTOL a_jj, otherwise the pseudo-inverse of the eigenvalues above
    EIG_RTOL lambda_max.  Returns (x, ok, solved): ok False where the device reports a failed regression (a single predecessor without a pivot, or
    no positive eigenvalue); solved True where the pivots passed."""
    dt = A.dtype.type
    k = A.shape[0]
    U = np.zeros_like(A)
    ok = True
    for j in range(k):
        d = A[j, j] - (U[:j, j] ** 2).sum()
        if not d > dt(PIVOT_RTOL) * A[j, j]:
            ok = False
            break
        U[j, j] = np.sqrt(d)
        for col in range(j + 1, k):
            U[j, col] = (A[j, col] - (U[:j, j] * U[:j, col]).sum()) / U[j, j]
    if ok:
        z = np.zeros(k, dtype=A.dtype)
        for i in range(k):
            z[i] = (b[i] - (U[:i, i] * z[:i]).sum()) / U[i, i]
        x = np.zeros(k, dtype=A.dtype)
        for i in range(k - 1, -1, -1):
            x[i] = (z[i] - (U[i, i + 1:] * x[i + 1:]).sum()) / U[i, i]
        return x, True, True
    if k == 1:
        return np.zeros(1, dtype=A.dtype), False, False
    lam, V = np.linalg.eigh(A.astype(np.float64))
    lam, V = lam.astype(A.dtype), V.astype(A.dtype)
    keep = lam > dt(EIG_RTOL) * lam.max()
    if not keep.any():
        return np.zeros(k, dtype=A.dtype), False, False
    return (V[:, keep] / lam[keep]) @ (V[:, keep].T @ b), True, False


def _plsc(R, w, lam, blocks, modes, C, factor, sd=None):
    """The PLSc estimates of one data set: R [P, P] its indicator correlation matrix, w [P] the outer weights, lam [P] the loadings, blocks the column
    indices of every LV, modes "A" / "B" (or 0 / 1) per LV, C [L, L] the path matrix (C[i, j] = 1 iff LV j -> LV i), factor [L] the mask (None: the
    default), sd [P] the columns' standard deviations (None: w are weights of the standardised columns).  Returns a dict in the dtype of R --
    np.longdouble works: status, weights [P], loadings [P], reliabilities Q [L], lv_cor [L, L] (corrected), path [L, L], r2 [L], indirect [L, L],
    total [L, L], pairs, and record (the device's layout); beside them quality (``_quality``'s dict), side (sigma | v'Rv | v'v per LV of the weights as
    given: what the assessment kernel hands to the PLSc kernel) and pivots_pass (every regression was solved, none went to the pseudo-inverse).
    Inadmissible inputs: status 4 and NaN in the record."""
    R = np.asarray(R)
    dt = R.dtype.type
    w, lam = np.asarray(w, dtype=R.dtype), np.asarray(lam, dtype=R.dtype)
    blocks = [np.asarray(b, dtype=np.int64) for b in blocks]
    C = np.asarray(C)
    L, P = len(blocks), R.shape[0]
    allowed = _default_mask(blocks, modes)
    factor = allowed.copy() if factor is None else np.asarray(factor).astype(bool)
    if factor.shape != (L,) or np.any(factor & ~allowed):
        raise ValueError("a Mode-B or single-item latent variable cannot be a common factor")
    q = _quality(R, w, lam, blocks, modes, sd=sd)
    v = w if sd is None else w * np.asarray(sd, dtype=R.dtype)
    pairs = _effect_pairs(C)
    npairs, ne = L * (L - 1) // 2, len(pairs)
    out = {"status": STATUS_OK, "weights": w.copy(), "pairs": pairs}
    one = dt(1)
    Q = np.ones(L, dtype=R.dtype)
    loadings = lam.copy()
    side = np.ones(3 * L, dtype=R.dtype)         # sigma | v'Rv | v'v of the weights as given: what the assessment kernel hands to the PLSc kernel
    out["side"], out["quality"] = side, q
    with np.errstate(divide="ignore", invalid="ignore"):
        for l, blk in enumerate(blocks):
            Rb = R[np.ix_(blk, blk)]
            side[L + l], side[2 * L + l] = v[blk] @ Rb @ v[blk], v[blk] @ v[blk]
            vb = v[blk] / np.sqrt(side[L + l])
            sigma = side[l] = -one if ((Rb @ vb) * lam[blk]).sum() < 0 else one
            if factor[l]:
                Q[l] = q["rho_a"][l]
                loadings[blk] = sigma * vb * np.sqrt(Q[l]) / (vb @ vb)
        rc = np.eye(L, dtype=R.dtype)
        e = 0
        for i in range(L):
            for j in range(i + 1, L):
                rc[i, j] = rc[j, i] = q["lv_cor"][e] / np.sqrt(Q[i] * Q[j])
                e += 1
    out["reliabilities"], out["lv_cor"], out["loadings"] = Q, rc, loadings
    off = rc[np.triu_indices(L, 1)]
    if not (np.all(np.isfinite(Q[factor])) and np.all(Q[factor] > 0) and np.all(np.abs(off) < 1)):
        out["status"] = STATUS_INADMISSIBLE
        nan = np.full((L, L), np.nan, dtype=R.dtype)
        out.update(path=nan, indirect=nan, total=nan, r2=np.full(L, np.nan, dtype=R.dtype), pivots_pass=False,
                   record=np.full(2 * P + L + 2 * ne + npairs, np.nan, dtype=R.dtype))
        return out
    B = np.zeros((L, L), dtype=R.dtype)
    r2 = np.zeros(L, dtype=R.dtype)
    pivots_pass = True
    for i in range(L):
        f = np.flatnonzero(C[i])
        if f.size:
            x, ok, solved = _regress(rc[np.ix_(f, f)], rc[f, i])
            pivots_pass = pivots_pass and solved
            if not ok:
                out["status"] = STATUS_SINGULAR
            B[i, f] = x
            r2[i] = x @ rc[f, i]
    indirect = np.zeros((L, L), dtype=R.dtype)
    power = B.copy()
    for _ in range(1, L):
        power = power @ B
        indirect += power
    total = B + indirect
    if out["status"] == STATUS_OK and not np.all(np.isfinite(r2)):
        out["status"] = STATUS_NONFINITE
    out.update(path=B, indirect=indirect, total=total, r2=r2, pivots_pass=pivots_pass)
    out["record"] = np.concatenate((w, r2, np.array([total[t, f] for f, t in pairs], dtype=R.dtype), np.array([B[t, f] for f, t in pairs], dtype=R.dtype),
                                    loadings, off))
    return out


class _Frames:
    """The six frames of a [W, len(columns)] table in the PLSc record layout."""

    def __init__(self, cm, native, table, columns):
        P, L, ne = cm.P, cm.L, native.n_eff
        cols = cm.used_data_cols()
        inv = cm.inv_index[cm.inv_index >= 0]
        eff_index = ["%s -> %s" % (cm.lvs[f], cm.lvs[t]) for f, t in zip(native.eff_from.tolist(), native.eff_to.tolist())]
        pair_index = ["%s <-> %s" % (cm.lvs[i], cm.lvs[j]) for i in range(L) for j in range(i + 1, L)]
        R = 2 * P + L + 2 * ne

        def frame(block, index):
            return pd.DataFrame(block, index=index, columns=columns)
        self._frames = {
            "weights": frame(table[:P][inv], cols),
            "r_squared": frame(table[P:P + L], cm.lvs).loc[cm.endogenous(), :],
            "total_effects": frame(table[P + L:P + L + ne], eff_index),
            "paths": frame(table[P + L + ne:P + L + 2 * ne], eff_index),
            "loading": frame(table[P + L + 2 * ne:R][inv], cols),
            "lv_correlations": frame(table[R:], pair_index),
        }

    def weights(self) -> pd.DataFrame:
        return self._frames["weights"]

    def r_squared(self) -> pd.DataFrame:
        return self._frames["r_squared"]

    def total_effects(self) -> pd.DataFrame:
        return self._frames["total_effects"]

    def paths(self) -> pd.DataFrame:
        """Direct effects; the indirect-only pairs (no path of their own: exactly zero in every replicate) are hidden, as ``Bootstrap.paths()`` hides them."""
        return self._frames["paths"][~self._hidden]

    def loading(self) -> pd.DataFrame:
        return self._frames["loading"]

    def lv_correlations(self) -> pd.DataFrame:
        return self._frames["lv_correlations"]


class PLScIntervals(_Frames):
    """Confidence intervals of a :class:`PLScBootstrap`: its six accessors with ``INTERVAL_COLUMNS``."""

    def __init__(self, cm, native, table, hidden, used, method, level):
        super().__init__(cm, native, table, INTERVAL_COLUMNS)
        self._hidden, self._used, self._method, self._level = hidden, used, method, level

    def method(self):
        return self._method

    def level(self):
        return self._level

    def used(self) -> int:
        return self._used


class PLScBootstrap(_Frames):
    """Bootstrap summaries of the PLSc estimates: ``weights()``, ``r_squared()``, ``total_effects()``, ``paths()``, ``loading()`` and ``lv_correlations()``
    with ``SUMMARY_COLUMNS``; ``intervals(method, level)`` gives the same six with ``INTERVAL_COLUMNS``."""

    def __init__(self, owner, table, used):
        super().__init__(owner._cm, owner._native, table, SUMMARY_COLUMNS)
        self._owner, self._used = owner, used
        cm, native = owner._cm, owner._native
        self._hidden = np.array([cm.path[t, f] == 0 for f, t in zip(native.eff_from.tolist(), native.eff_to.tolist())], dtype=bool)
        self._interval_cache = {}

    def intervals(self, method="percentile", level=0.95) -> PLScIntervals:
        if method not in INTERVAL_METHODS:
            raise ValueError("method must be one of %s" % ", ".join(INTERVAL_METHODS))
        if method == "bca":
            raise NotImplementedError("no bca intervals for the PLSc estimates: the jackknife writes no PLSc records")
        if not 0.0 < float(level) < 1.0:
            raise ValueError("level must lie strictly between 0 and 1")
        key = (method, float(level))
        if key not in self._interval_cache:
            o = self._owner
            table, used = o._native.plsc_intervals(o._iterations, o._original, method, float(level))
            self._interval_cache[key] = PLScIntervals(o._cm, o._native, np.column_stack((o._original, table)), self._hidden, used, method, float(level))
        return self._interval_cache[key]

    def used(self) -> int:
        return self._used


def _factor_mask(cm, factors):
    """factors (LV names, None: the default) -> the 0 / 1 mask in LV order; ValueError for a name that is no LV, or an LV that cannot be a factor."""
    sizes = np.diff(cm.block_offset)
    allowed = (np.asarray(cm.modes) == 0) & (sizes >= 2)
    if factors is None:
        return allowed.astype(np.uint8)
    mask = np.zeros(cm.L, dtype=np.uint8)
    for name in factors:
        if name not in cm.lvs:
            raise ValueError("factors: %r is not a latent variable of this model" % (name,))
        l = cm.lvs.index(name)
        if not allowed[l]:
            raise ValueError("factors: %s cannot be a common factor (Mode B, or a single item)" % name)
        mask[l] = 1
    return mask


class PLSc:
    """``PLSc(data, config, scheme=Scheme.CENTROID, iterations=5000, seed=None, factors=None, fit_iterations=100, tolerance=1e-6, device_id=0,
    processes=1)`` -- ``iterations`` bootstrap replicates; ``factors``: the names of the LVs that are common factors (None: every Mode-A block of two
    items or more).  Also ``Plspm(..., bootstrap=True, consistent=True, factors=None).plsc()``.

    Full-sample frames: ``path_coefficients()`` (L x L), ``r_squared()``, ``effects()`` (from, to, direct, indirect, total), ``loadings()``, ``weights()``,
    ``reliabilities()`` (the Q used), ``lv_correlations()`` (corrected, L x L).  Inference: ``bootstrap()``; ``used()``, ``inadmissible()``, ``seed()``,
    ``replicates()``."""

    def __init__(self, data: pd.DataFrame, config: c.Config, scheme: Scheme = Scheme.CENTROID, iterations: int = 5000, seed: int = None, factors=None,
                 fit_iterations: int = 100, tolerance: float = 0.000001, device_id: int = 0, processes: int = 1):
        assert tolerance > 0
        assert scheme in Scheme
        if processes > 1:
            raise NotImplementedError("PLSc runs on one GPU (processes = 1)")
        observations = config.filter(data)
        why = _unsupported(config, observations)
        if why is not None:
            raise NotImplementedError("PLSc covers metric data without missing cells and without higher-order constructs: this model has " + why)
        _check_factor_names(config, factors)
        n = observations.shape[0]
        if n < 10:
            raise Exception("Bootstrapping could not be performed, at least 10 observations are required.")
        if iterations < 10:
            iterations = 100
        calculator = pw.WeightsCalculatorFactory(config, max(fit_iterations, MIN_ITERATIONS), tolerance, np.sqrt(n / (n - 1)), scheme, device_id)
        whole = Estimator(config).run(calculator, observations, want_scores=False)
        native = whole.native
        mask = _factor_mask(whole.compiled, factors)
        native.plsc_enable(True, mask)
        if seed is None:
            seed = int.from_bytes(os.urandom(8), "little")
        native.bootstrap_device(iterations, seed, 0)
        self._init(native, whole.compiled, iterations, mask)
        self._seed = seed

    @classmethod
    def of_bootstrap(cls, native, compiled, iterations, mask):
        """The PLSc estimates of a bootstrap that already ran on ``native`` with ``plsc_enable(True, mask)`` (``Plspm(bootstrap=True, consistent=True)``)."""
        self = cls.__new__(cls)
        self._init(native, compiled, iterations, mask)
        self._seed = None
        return self

    def _init(self, native, cm, iterations, mask):
        self._native, self._cm, self._iterations, self._mask = native, cm, iterations, np.asarray(mask, dtype=bool)
        try:
            self._original, self._status = native.plsc_fit()
            self._assess, _ = native.assess_fit()
            self._table, self._used = native.plsc_summary(iterations, self._original)
        except _native.NativeBackendError as err:
            raise NotImplementedError("no PLSc on this handle: " + str(err))
        self._bootstrap = None
        self._records = None

    # ---- the full sample
    def _square(self, values, diagonal, pairs):
        L = self._cm.L
        out = np.full((L, L), diagonal, dtype=np.float64)
        for (i, j), value in zip(pairs, values):
            out[i, j] = value
        return out

    def status(self) -> int:
        """Status of the full-sample record (0: fine; 4: inadmissible, every estimate NaN)."""
        return self._status

    def path_coefficients(self) -> pd.DataFrame:
        cm, nv = self._cm, self._native
        P, L, ne = cm.P, cm.L, nv.n_eff
        direct = self._original[P + L + ne:P + L + 2 * ne]
        B = self._square(direct, 0.0, [(t, f) for f, t in zip(nv.eff_from.tolist(), nv.eff_to.tolist())])
        B[cm.path == 0] = 0.0 if self._status != STATUS_INADMISSIBLE else np.nan
        return pd.DataFrame(B, index=cm.lvs, columns=cm.lvs)

    def r_squared(self) -> pd.Series:
        cm = self._cm
        return pd.Series(self._original[cm.P:cm.P + cm.L], index=cm.lvs, name="r_squared")

    def effects(self) -> pd.DataFrame:
        cm, nv = self._cm, self._native
        P, L, ne = cm.P, cm.L, nv.n_eff
        total, direct = self._original[P + L:P + L + ne], self._original[P + L + ne:P + L + 2 * ne]
        frm, to = [cm.lvs[f] for f in nv.eff_from.tolist()], [cm.lvs[t] for t in nv.eff_to.tolist()]
        return pd.DataFrame({"from": frm, "to": to, "direct": direct, "indirect": total - direct, "total": total},
                            index=["%s -> %s" % ft for ft in zip(frm, to)], columns=["from", "to", "direct", "indirect", "total"])

    def _mv_series(self, block, name):
        cm = self._cm
        return pd.Series(block[cm.inv_index[cm.inv_index >= 0]], index=cm.used_data_cols(), name=name)

    def loadings(self) -> pd.Series:
        cm, R = self._cm, self._native.row_width
        return self._mv_series(self._original[R - cm.P:R], "loading")

    def weights(self) -> pd.Series:
        return self._mv_series(self._original[:self._cm.P], "weight")

    def factors(self) -> list:
        """The LVs corrected as common factors."""
        return [lv for lv, f in zip(self._cm.lvs, self._mask) if f]

    def reliabilities(self) -> pd.Series:
        """The Q used: rho_A for a factor, 1 for any other LV."""
        L = self._cm.L
        rho_a = self._assess[L:2 * L]
        return pd.Series(np.where(self._mask, rho_a, 1.0), index=self._cm.lvs, name="reliability")

    def lv_correlations(self) -> pd.DataFrame:
        cm, L = self._cm, self._cm.L
        pairs = [(i, j) for i in range(L) for j in range(i + 1, L)]
        out = self._square(self._original[self._native.row_width:], 1.0, pairs)
        out = np.where(np.triu(np.ones((L, L), dtype=bool), 1), out, out.T)
        return pd.DataFrame(out, index=cm.lvs, columns=cm.lvs)

    # ---- inference
    def bootstrap(self) -> PLScBootstrap:
        if self._bootstrap is None:
            self._bootstrap = PLScBootstrap(self, self._table, self._used)
        return self._bootstrap

    def _fetch(self):
        if self._records is None:
            self._records = self._native.plsc_fetch(0, self._iterations)
        return self._records

    def used(self) -> int:
        """Number of replicates that entered the summaries."""
        return self._used

    def inadmissible(self) -> int:
        """Number of replicates with status 4: a factor's rho_A not positive and finite, or a corrected construct correlation not below 1 in magnitude."""
        return int(np.count_nonzero(self._fetch()[1] == STATUS_INADMISSIBLE))

    def seed(self):
        return self._seed

    def replicates(self):
        """The used replicates' PLSc records [n_used, W] (weights | r2 | total | direct | loadings | lv_cor_c), fetched from HBM."""
        records, status = self._fetch()
        return records[status == 0]


def _check_factor_names(config, factors):
    """ValueError for a ``factors`` entry that needs no device to be refused: not a list of LV names of this model's path."""
    if factors is None:
        return
    if isinstance(factors, str):
        raise ValueError("factors must be a list of latent variable names")
    lvs = list(config.path())
    for name in factors:
        if name not in lvs:
            raise ValueError("factors: %r is not a latent variable of this model" % (name,))
        if config.mode(name).value.code != 0 or len(list(config.mvs(name))) < 2:
            raise ValueError("factors: %s cannot be a common factor (Mode B, or a single item)" % name)
