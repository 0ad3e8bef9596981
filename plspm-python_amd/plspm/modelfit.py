"""Model fit with a bootstrap-based test of exact overall fit on the GPU (not in the reference): SRMR and d_ULS of the saturated and of the
estimated model, and the Bollen-Stine bootstrap of Dijkstra and Henseler (2015) with its HI95 / HI99 critical values.

Does the model reproduce the correlations of its indicators?  Every replicate's record is computed on the device, behind the PLSc kernel whose
loadings, construct correlations and path coefficients it reads (include/plspm_hip.h ``plspm_modelfit_*``).  This project's
definitions, from the quantities of ``plspm.plsc`` (lambda* the PLSc loadings: a factor's corrected, any other LV's the fit's; rc the PLSc construct
correlations; beta the PLSc path coefficients; the factor mask):

    Phi (saturated)   rc
    Phi (estimated)   LVs in path order.  Phi_jj = 1; j, k both without predecessors: rc_jk; j with predecessors, every k < j:
                      sum_{m in pred(j)} beta_jm Phi_mk, in ascending j -- the structural residual of j is uncorrelated with everything before it;
                      j without predecessors and an earlier k with: sum_{m in pred(k)} beta_km Phi_jm, in ascending k
    Sigma(Phi)        diagonal 1; p, q in blocks i != j: lambda*_p Phi_ij lambda*_q; p != q in one block: lambda*_p lambda*_q for a factor, r_pq
                      itself for a composite (Mode A outside the mask, every Mode-B block: a composite reproduces its own block)
    d_uls             sum_{p<q} (r_pq - sigma_pq)^2 = 1/2 ||R - Sigma||_F^2            srmr    sqrt(2 d_uls / (P (P + 1)))
    record            srmr_sat | d_uls_sat | srmr_est | d_uls_est
    inadmissible      (status 4, NaN everywhere, not used) the PLSc record is, a column is constant, or a value is not finite
    d_g               (``geodesic=True``; include/plspm_hip.h ``plspm_geodesic_*``) 1/2 sum_k (ln phi_k)^2 over the eigenvalues phi_k of
                      R^-1 Sigma: the geodesic discrepancy, which weighs a residual by how well the data determine it and so need not agree with the
                      other two.  Record d_g_sat | d_g_est; inadmissible where the model-fit record is, where R is singular (a Cholesky pivot not above
                      1e-12), where Sigma is not positive definite (some phi_k <= 0), or where a value is not finite

The test: the data are transformed once so that their correlation matrix is the implied one of the model under test (X~ = Z R^-1/2 Sigma^1/2), and
the ordinary bootstrap runs on X~ with the model-fit kernel on; the observed discrepancy is held against the replicates'.  ``_model_fit`` below is
the same statistic in NumPy: the checker of the kernel.  Scope: metric data without missing cells and without higher-order constructs, one GPU.
"""
import os

import numpy as np
import pandas as pd

import plspm.config as c
import plspm.weights as pw
from plspm import _native
from plspm.estimator import Estimator
from plspm.plsc import STATUS_INADMISSIBLE, STATUS_OK, _check_factor_names, _factor_mask
from plspm.quality import MIN_ITERATIONS, _unsupported
from plspm.scheme import Scheme
from plspm.weights import NumericalConditionError

STATISTICS = ["srmr", "d_uls"]
GEODESIC = "d_g"
GEODESIC_PIVOT_MIN = 1e-12      # a Cholesky pivot of R (unit diagonal) that is not above this: R is singular, d_G is inadmissible
FIT_COLUMNS = ["saturated", "estimated", "hi95", "hi99", "p.value"]
MODELS = ("saturated", "estimated")
CONDITION_RTOL = 1e-10          # a correlation matrix whose smallest eigenvalue is not above this share of its largest has no Bollen-Stine transformation


def _implied_phi(rc, B, C):
    """The estimated model's construct correlations from rc [L, L], the path coefficients B [L, L] (B[j, m]: m -> j) and the path matrix C, LVs in path order."""
    L = rc.shape[0]
    preds = [np.flatnonzero(np.asarray(C)[j]) for j in range(L)]
    if any(p.size and p.max() >= j for j, p in enumerate(preds)):
        raise ValueError("the latent variables must be in path order: every predecessor before its successor")
    phi = np.eye(L, dtype=rc.dtype)
    for j in range(L):
        for k in range(j):
            if preds[j].size:
                value = sum(B[j, m] * phi[m, k] for m in preds[j])
            elif preds[k].size:
                value = sum(B[k, m] * phi[j, m] for m in preds[k])
            else:
                value = rc[j, k]
            phi[j, k] = phi[k, j] = value
    return phi


def _implied_sigma(R, lam, phi, blocks, factor):
    P = R.shape[0]
    lvof = np.empty(P, dtype=np.int64)
    for l, blk in enumerate(blocks):
        lvof[blk] = l
    S = np.outer(lam, lam) * phi[np.ix_(lvof, lvof)]
    for l, blk in enumerate(blocks):
        S[np.ix_(blk, blk)] = np.outer(lam[blk], lam[blk]) if factor[l] else R[np.ix_(blk, blk)]
    S[np.diag_indices(P)] = R.dtype.type(1)
    return S


def _model_fit(R, plsc_out, blocks, C, factor):
    """The model fit of one data set: R [P, P] its indicator correlation matrix, plsc_out the dict of ``plspm.plsc._plsc`` on it (loadings, lv_cor, path,
    status), blocks the column indices of every LV, C [L, L] the path matrix (C[i, j] = 1 iff LV j -> LV i), factor [L] the mask plsc_out was computed
    with.  Returns a dict in the dtype of R -- np.longdouble works: status, phi (the estimated model's construct correlations), implied {"saturated",
    "estimated"} [P, P], srmr_sat, d_uls_sat, srmr_est, d_uls_est and record (the device's layout).  Inadmissible: status 4 and NaN in the record."""
    R = np.asarray(R)
    dt = R.dtype.type
    P, L = R.shape[0], len(blocks)
    blocks = [np.asarray(b, dtype=np.int64) for b in blocks]
    factor = np.asarray(factor).astype(bool)
    out = {"status": plsc_out["status"]}
    nan_record = np.full(4, np.nan, dtype=R.dtype)
    if plsc_out["status"] == STATUS_INADMISSIBLE or not np.all(np.isfinite(R)):
        out.update(status=STATUS_INADMISSIBLE, phi=None, implied=None, record=nan_record)
    else:
        lam, rc = np.asarray(plsc_out["loadings"], dtype=R.dtype), np.asarray(plsc_out["lv_cor"], dtype=R.dtype)
        phi = _implied_phi(rc, np.asarray(plsc_out["path"], dtype=R.dtype), C)
        implied = {"saturated": _implied_sigma(R, lam, rc, blocks, factor), "estimated": _implied_sigma(R, lam, phi, blocks, factor)}
        upper = np.triu_indices(P, 1)
        d = [((R - implied[model])[upper] ** 2).sum() for model in MODELS]
        scale = dt(2) / dt(P * (P + 1))
        record = np.array([np.sqrt(scale * d[0]), d[0], np.sqrt(scale * d[1]), d[1]], dtype=R.dtype)
        out.update(phi=phi, implied=implied, record=record)
        if not np.all(np.isfinite(record)):
            out.update(status=STATUS_INADMISSIBLE, record=nan_record)
    out["srmr_sat"], out["d_uls_sat"], out["srmr_est"], out["d_uls_est"] = out["record"]
    return out


def _geodesic(R, implied):
    """The eigenvalues behind d_G of one implied matrix, the mirror of csrc/geodesic_core.h in NumPy: (status, phi) with phi the eigenvalues of R^-1 implied
    in ascending order, computed as those of the symmetric G^-1 implied G^-T with R = G G' (cholesky, two triangular solves, eigvalsh).  Status 4 (inadmissible)
    where a Cholesky pivot of R is not above GEODESIC_PIVOT_MIN (phi is None then), where some phi_k is not positive, and where something is not finite."""
    R, implied = np.asarray(R, dtype=np.float64), np.asarray(implied, dtype=np.float64)
    if not (np.all(np.isfinite(R)) and np.all(np.isfinite(implied))):
        return STATUS_INADMISSIBLE, None
    try:
        G = np.linalg.cholesky(R)
    except np.linalg.LinAlgError:
        return STATUS_INADMISSIBLE, None
    if not np.all(np.diag(G) ** 2 > GEODESIC_PIVOT_MIN):
        return STATUS_INADMISSIBLE, None
    half = np.linalg.solve(G, implied)                       # G^-1 Sigma
    C = np.linalg.solve(G, half.T)                           # G^-1 (G^-1 Sigma)' = G^-1 Sigma G^-T
    phi = np.linalg.eigvalsh(0.5 * (C + C.T))
    admissible = np.all(np.isfinite(phi)) and np.all(phi > 0) and np.isfinite(_d_g(phi))
    return (STATUS_OK if admissible else STATUS_INADMISSIBLE), phi


def _d_g(phi):
    """1/2 sum (ln phi_k)^2."""
    with np.errstate(invalid="ignore", divide="ignore"):
        return 0.5 * float(np.sum(np.log(phi) ** 2))


def _geodesic_fit(R, fit):
    """The geodesic record of one data set from ``_model_fit``'s dict on it: {"status", "record" [d_g_sat, d_g_est], "phi": {model: eigenvalues}}.  Status: the
    model fit's, or 4 with NaN in both values by ``_geodesic``'s rules for either model."""
    out = {"status": fit["status"], "record": np.full(2, np.nan), "phi": {}}
    if fit["status"] == STATUS_INADMISSIBLE:
        return out
    values = []
    for model in MODELS:
        status, phi = _geodesic(R, fit["implied"][model])
        out["phi"][model] = phi
        if status != STATUS_OK:
            out["status"] = STATUS_INADMISSIBLE
        values.append(np.nan if phi is None else _d_g(phi))
    if out["status"] != STATUS_INADMISSIBLE:
        out["record"] = np.array(values)
    return out


def _sqrt_pair(M, what):
    """(M^1/2, M^-1/2) of a correlation matrix by its eigendecomposition; NumericalConditionError unless its smallest eigenvalue is above CONDITION_RTOL of
    its largest."""
    lam, V = np.linalg.eigh(M)
    if not np.all(np.isfinite(lam)) or not lam[0] > CONDITION_RTOL * lam[-1]:
        raise NumericalConditionError("no Bollen-Stine transformation: %s is not positive definite (smallest eigenvalue %.3e, largest %.3e)" % (what, lam[0], lam[-1]))
    root = np.sqrt(lam)
    return (V * root) @ V.T, (V / root) @ V.T


def _bollen_stine(X, sigma):
    """X [n, P] -> X~ = Z R^-1/2 sigma^1/2 on the standardised Z (divisor n), R = Z'Z / n: centred columns of unit variance whose correlation matrix is sigma."""
    X = np.asarray(X, dtype=np.float64)
    mean, sd = X.mean(axis=0), X.std(axis=0)
    if not np.all(sd > 0):
        raise NumericalConditionError("no Bollen-Stine transformation: a column is constant")
    Z = (X - mean) / sd
    _, r_inv_root = _sqrt_pair(Z.T @ Z / X.shape[0], "the data's correlation matrix (collinear columns?)")
    s_root, _ = _sqrt_pair(np.asarray(sigma, dtype=np.float64), "the model-implied correlation matrix")
    return Z @ r_inv_root @ s_root


def _plsc_out_of_record(record, status, native, cm):
    """The part of ``_plsc``'s dict that ``_model_fit`` reads, from a device PLSc record."""
    P, L, ne, R = cm.P, cm.L, native.n_eff, native.row_width
    rc = np.eye(L)
    rc[np.triu_indices(L, 1)] = record[R:]
    rc = np.where(np.triu(np.ones((L, L), dtype=bool), 1), rc, rc.T)
    B = np.zeros((L, L))
    for e, (f, t) in enumerate(zip(native.eff_from.tolist(), native.eff_to.tolist())):
        B[t, f] = record[P + L + ne + e]
    return {"status": status, "loadings": record[R - P:R], "lv_cor": rc, "path": B}


class ModelFit:
    """``ModelFit(data, config, scheme=Scheme.CENTROID, iterations=5000, seed=None, factors=(), null="estimated", fit_iterations=100, tolerance=1e-6,
    device_id=0, processes=1, geodesic=False)`` -- ``iterations`` Bollen-Stine bootstrap replicates (0: the values without inference); ``factors``: the names of the LVs
    that are common factors (``()``: none, the composite model plain ``Plspm`` estimates; None: every Mode-A block of two items or more, PLSc's default);
    ``null``: the model whose exact fit is tested, "estimated" or "saturated".

    ``fit()``: index srmr, d_uls; columns saturated, estimated (the observed values), hi95, hi99 (the 95 % and 99 % quantiles of the ``null`` model's
    statistic under exact fit) and p.value ((1 + #{d* >= d_obs}) / (1 + used): never zero).  ``implied(model)``: the P x P implied correlations.
    ``records()``, ``used()``, ``inadmissible()``, ``seed()``, ``replicates()``, ``status()``.

    ``geodesic=True`` adds the geodesic discrepancy: a third row ``d_g`` of ``fit()`` with the same five columns, from records of its own --
    ``records(measure="d_g")`` [iterations, 2] d_g_sat | d_g_est, ``used(measure="d_g")``, ``inadmissible(measure="d_g")``: a replicate whose implied matrix
    is not positive definite counts for srmr and d_uls and not for d_g.  A full sample that is inadmissible for d_g alone raises NumericalConditionError
    when replicates are asked for (there is nothing to hold them against); with ``iterations=0`` its row is NaN."""

    def __init__(self, data: pd.DataFrame, config: c.Config, scheme: Scheme = Scheme.CENTROID, iterations: int = 5000, seed: int = None, factors=(),
                 null: str = "estimated", fit_iterations: int = 100, tolerance: float = 0.000001, device_id: int = 0, processes: int = 1, geodesic: bool = False):
        assert tolerance > 0
        assert scheme in Scheme
        if processes > 1:
            raise NotImplementedError("model fit runs on one GPU (processes = 1)")
        if null not in MODELS:
            raise ValueError("null must be one of %s" % ", ".join(MODELS))
        if iterations < 0:
            raise ValueError("iterations must not be negative")
        observations = config.filter(data)
        why = _unsupported(config, observations)
        if why is not None:
            raise NotImplementedError("model fit covers metric data without missing cells and without higher-order constructs: this model has " + why)
        _check_factor_names(config, factors)
        n = observations.shape[0]
        if n < 10:
            raise Exception("Bootstrapping could not be performed, at least 10 observations are required.")
        calculator = pw.WeightsCalculatorFactory(config, max(fit_iterations, MIN_ITERATIONS), tolerance, np.sqrt(n / (n - 1)), scheme, device_id)
        whole = Estimator(config).run(calculator, observations, want_scores=False)
        native, cm = whole.native, whole.compiled
        self._cm, self._null, self._iterations = cm, null, int(iterations)
        self._mask = _factor_mask(cm, factors)
        self._geodesic = bool(geodesic)
        self._g_observed, self._g_status, self._g_records, self._g_used = np.full(2, np.nan), STATUS_OK, None, 0
        self._g_critical = np.full((2, 2), np.nan)
        enable = native.geodesic_enable if self._geodesic else native.modelfit_enable
        enable(True, self._mask)
        try:
            self._observed, self._status = native.modelfit_fit()
            plsc_record, plsc_status = native.plsc_fit()
            if self._geodesic:
                self._g_observed, self._g_status = native.geodesic_fit()
        except _native.NativeBackendError as err:
            raise NotImplementedError("no model fit on this handle: " + str(err))
        X = observations.values[:, cm.col_index].astype(np.float64)
        blocks = [np.arange(cm.block_offset[l], cm.block_offset[l + 1]) for l in range(cm.L)]
        self._mirror = _model_fit(np.corrcoef(X, rowvar=False).reshape(cm.P, cm.P), _plsc_out_of_record(plsc_record, plsc_status, native, cm), blocks, cm.path, self._mask)
        self._seed, self._records, self._used = seed, None, 0
        self._critical = np.full((4, 2), np.nan)
        self._transformed = None
        if self._iterations == 0:
            return
        if self._status == STATUS_INADMISSIBLE or self._mirror["status"] == STATUS_INADMISSIBLE:
            raise NumericalConditionError("the full-sample model fit is inadmissible (status 4): there is no implied correlation matrix to test against")
        if self._geodesic and self._g_status == STATUS_INADMISSIBLE:
            raise NumericalConditionError("the full-sample geodesic discrepancy d_g is inadmissible (status 4): the indicator correlation matrix is singular or "
                                          "an implied correlation matrix is not positive definite; srmr and d_uls are available with geodesic=False")
        tilde = observations.copy().astype(np.float64)
        tilde.iloc[:, cm.col_index] = _bollen_stine(X, self._mirror["implied"][null])
        self._transformed = Estimator(config).run(calculator, tilde, want_scores=False)
        second = self._transformed.native
        (second.geodesic_enable if self._geodesic else second.modelfit_enable)(True, self._mask)
        if seed is None:
            self._seed = int.from_bytes(os.urandom(8), "little")
        second.bootstrap_device(self._iterations, self._seed, 0)
        self._records = second.modelfit_fetch(0, self._iterations)
        original = np.where(np.isfinite(self._observed), self._observed, 0.0)
        for column, level in enumerate((0.90, 0.98)):
            table, self._used = second.modelfit_intervals(self._iterations, original, "percentile", level)
            self._critical[:, column] = table[:, 1]
        if self._geodesic:
            self._g_records = second.geodesic_fetch(0, self._iterations)
            for column, level in enumerate((0.90, 0.98)):
                table, self._g_used = second.geodesic_intervals(self._iterations, self._g_observed, "percentile", level)
                self._g_critical[:, column] = table[:, 1]

    def status(self) -> int:
        """Status of the full-sample record (0: fine; 4: inadmissible, every value NaN)."""
        return self._status

    def null(self) -> str:
        return self._null

    def fit(self) -> pd.DataFrame:
        obs = self._observed
        table = np.full((2, 5), np.nan)
        table[:, 0], table[:, 1] = obs[:2], obs[2:]
        if self._records is not None:
            first = 2 * MODELS.index(self._null)
            ok = self.replicates()
            table[:, 2:4] = self._critical[first:first + 2]
            table[:, 4] = (1.0 + np.count_nonzero(ok[:, first:first + 2] >= obs[first:first + 2], axis=0)) / (1.0 + ok.shape[0])
        if self._geodesic:
            row = np.full((1, 5), np.nan)
            row[0, :2] = self._g_observed
            if self._g_records is not None:
                which = MODELS.index(self._null)
                records, status = self._g_records
                ok = records[status == STATUS_OK]
                row[0, 2:4] = self._g_critical[which]
                row[0, 4] = (1.0 + np.count_nonzero(ok[:, which] >= self._g_observed[which])) / (1.0 + ok.shape[0])
            return pd.DataFrame(np.vstack([table, row]), index=STATISTICS + [GEODESIC], columns=FIT_COLUMNS)
        return pd.DataFrame(table, index=STATISTICS, columns=FIT_COLUMNS)

    def implied(self, model="estimated") -> pd.DataFrame:
        """The model-implied indicator correlations of the full sample, P x P, for "saturated" or "estimated"."""
        if model not in MODELS:
            raise ValueError("model must be one of %s" % ", ".join(MODELS))
        if self._mirror["implied"] is None:
            raise NumericalConditionError("the full-sample model fit is inadmissible (status 4)")
        cm = self._cm
        inv = cm.inv_index[cm.inv_index >= 0]
        cols = cm.used_data_cols()
        return pd.DataFrame(self._mirror["implied"][model][np.ix_(inv, inv)], index=cols, columns=cols)

    def factors(self) -> list:
        """The LVs taken as common factors."""
        return [lv for lv, f in zip(self._cm.lvs, self._mask) if f]

    def _is_geodesic(self, measure) -> bool:
        if measure is not None and measure not in STATISTICS + [GEODESIC]:
            raise ValueError("measure must be one of %s" % ", ".join(STATISTICS + [GEODESIC]))
        if measure == GEODESIC and not self._geodesic:
            raise ValueError("no d_g on this ModelFit: call it with geodesic=True")
        return measure == GEODESIC

    def records(self, measure=None):
        """(records [iterations, 4], status [iterations]) of the Bollen-Stine replicates: srmr_sat | d_uls_sat | srmr_est | d_uls_est;
        ``measure="d_g"``: the geodesic records [iterations, 2] d_g_sat | d_g_est and their status."""
        records = self._g_records if self._is_geodesic(measure) else self._records
        if records is None:
            raise Exception("No replicates: ModelFit was called with iterations=0")
        return records

    def replicates(self):
        """The used replicates' records [n_used, 4]."""
        records, status = self.records()
        return records[status == STATUS_OK]

    def used(self, measure=None) -> int:
        """Number of replicates behind hi95, hi99 and p.value (of srmr and d_uls; ``measure="d_g"``: of d_g)."""
        return self._g_used if self._is_geodesic(measure) else self._used

    def inadmissible(self, measure=None) -> int:
        """Number of replicates with status 4 (``measure="d_g"``: in the geodesic records)."""
        return int(np.count_nonzero(self.records(measure)[1] == STATUS_INADMISSIBLE))

    def seed(self):
        return self._seed
