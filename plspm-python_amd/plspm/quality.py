"""Measurement-model assessment with bootstrap inference on the GPU (not in the reference): Cronbach's alpha, rho_A, composite reliability
rho_C and AVE per latent variable; HTMT, HTMT2 and the construct correlations (for Fornell-Larcker) per pair of latent variables.

Every replicate's criteria are computed on the device, behind the solver, from the replicate's moment matrix and its record's weights and
loadings (include/plspm_hip.h ``plspm_assess_*``) -- HTMT, rho_A and the construct correlations need the replicate's indicator
correlations, which no record holds.  The summaries and intervals are the bootstrap's own kernels on the assessment records.  This project's
definitions, with R the indicator correlation matrix of the data set at hand, w the outer weights and lambda the loadings of its fit:

    v_p = w_p s_p (s_p the column's standard deviation), normalised per block so that v_b' R_bb v_b = 1
    u_p = sum_{q in block(p)} r_pq v_q;  sigma_l = sign(sum_{p in l} u_p lambda_p), +1 for 0  (u: the loading before the sign rule, lambda: behind it)
    per LV of k items (k = 1: all four are 1)
      alpha   max(0, k / (k - 1) * 2 sum_{i>j} r_ij / sum_ij r_ij)
      rho_a   Mode A: (v'v)^2 v'(R_bb - I)v / ((v'v)^2 - sum v_p^4)  (Dijkstra-Henseler);  Mode B: 1
      rho_c   (sum lambda)^2 / ((sum lambda)^2 + sum (1 - lambda^2))
      ave     sum lambda^2 / k
    per LV pair (i, j), i < j in LV order, i-major
      htmt    mean_{p in i, q in j} |r_pq| / sqrt(m_i m_j),  m_l the mean of |r_pq| over p < q in block l (1 for a single item)
      htmt2   the same with geometric means (exp of the mean log; a zero correlation gives 0)
      lv_cor  sigma_i sigma_j v_i' R_ij v_j

``_quality`` below is the same statistic in NumPy: the checker of the kernel.  Scope: metric data without missing cells and without
higher-order constructs, one GPU; no bca intervals (the jackknife writes no assessment records).
"""
import os

import numpy as np
import pandas as pd

import plspm.config as c
import plspm.weights as pw
from plspm import _native
from plspm.bootstrap import INTERVAL_COLUMNS, INTERVAL_METHODS, SUMMARY_COLUMNS
from plspm.estimator import Estimator
from plspm.scheme import Scheme

LV_CRITERIA = ("alpha", "rho_a", "rho_c", "ave")
PAIR_CRITERIA = ("htmt", "htmt2", "lv_cor")
CRITERIA = LV_CRITERIA + PAIR_CRITERIA
MIN_ITERATIONS = 100            # as Plspm: "default and minimum 100"


def _quality(R, w, lam, blocks, modes, sd=None):
    """The criteria of one data set: R [P, P] its indicator correlation matrix, w [P] the outer weights, lam [P] the loadings, blocks the
    column indices of every LV, modes "A" / "B" (or 0 / 1) per LV, sd [P] the columns' standard deviations (None: w are weights of the
    standardised columns).  Returns a dict of the seven arrays (``CRITERIA``) in the dtype of R -- np.longdouble works."""
    R = np.asarray(R)
    dt = R.dtype.type
    w, lam = np.asarray(w, dtype=R.dtype), np.asarray(lam, dtype=R.dtype)
    v = w if sd is None else w * np.asarray(sd, dtype=R.dtype)
    blocks = [np.asarray(b, dtype=np.int64) for b in blocks]
    L = len(blocks)
    one, zero = dt(1), dt(0)
    out = {name: np.ones(L, dtype=R.dtype) for name in LV_CRITERIA}
    vn, sigma, m_abs, m_geo = [], np.ones(L, dtype=R.dtype), np.ones(L, dtype=R.dtype), np.ones(L, dtype=R.dtype)
    for l, blk in enumerate(blocks):
        k = len(blk)
        Rb = R[np.ix_(blk, blk)]
        vb = v[blk] / np.sqrt(v[blk] @ Rb @ v[blk])
        vn.append(vb)
        u = Rb @ vb
        sigma[l] = -one if (u * lam[blk]).sum() < 0 else one
        if k == 1:
            continue
        upper = Rb[np.triu_indices(k, 1)]
        off = dt(2) * upper.sum()
        with np.errstate(divide="ignore", invalid="ignore"):
            out["alpha"][l] = max(zero, dt(k) / dt(k - 1) * off / (dt(k) + off))
            if modes[l] in ("A", 0):
                vv = vb @ vb
                out["rho_a"][l] = vv * vv * (vb @ (Rb - np.eye(k, dtype=R.dtype)) @ vb) / (vv * vv - (vb ** 4).sum())
            sl = lam[blk].sum()
            out["rho_c"][l] = sl * sl / (sl * sl + (one - lam[blk] ** 2).sum())
            out["ave"][l] = (lam[blk] ** 2).sum() / dt(k)
            m_abs[l] = np.abs(upper).mean()
            m_geo[l] = np.exp(np.log(np.abs(upper)).mean())
    npairs = L * (L - 1) // 2
    for name in PAIR_CRITERIA:
        out[name] = np.empty(npairs, dtype=R.dtype)
    e = 0
    for i in range(L):
        for j in range(i + 1, L):
            Rij = R[np.ix_(blocks[i], blocks[j])]
            with np.errstate(divide="ignore", invalid="ignore"):
                out["htmt"][e] = np.abs(Rij).mean() / np.sqrt(m_abs[i] * m_abs[j])
                out["htmt2"][e] = np.exp(np.log(np.abs(Rij)).mean()) / np.sqrt(m_geo[i] * m_geo[j])
            out["lv_cor"][e] = sigma[i] * sigma[j] * (vn[i] @ Rij @ vn[j])
            e += 1
    return out


def _record(q):
    """The assessment record of ``_quality``'s dict: alpha | rho_a | rho_c | ave | htmt | htmt2 | lv_cor."""
    return np.concatenate([q[name] for name in CRITERIA])


def _unsupported(config, observations):
    """What keeps the assessment away from this model (None: nothing) -- the handle kinds plspm_assess_enable refuses."""
    if not config.metric():
        return "non-metric scales"
    if config.hoc():
        return "higher-order constructs"
    if config.nan_columns(observations).any():
        return "missing cells"
    return None


class Quality:
    """``Quality(data, config, scheme=Scheme.CENTROID, iterations=5000, seed=None, fit_iterations=100, tolerance=1e-6, device_id=0, processes=1)``
    -- ``iterations`` bootstrap replicates.  Also ``Plspm(..., bootstrap=True, quality=True).quality()``.

    ``reliability()``: LVs x (alpha, rho_a, rho_c, ave); ``htmt()``, ``htmt2()``, ``lv_correlations()``, ``fornell_larcker()``: L x L frames of the
    full-sample values; ``summary(criterion)`` / ``intervals(criterion, method, level)``: the bootstrap's summary / interval columns, one row per LV
    (reliability criteria) or per pair "A <-> B" (pair criteria); ``used()``; ``replicates()``."""

    def __init__(self, data: pd.DataFrame, config: c.Config, scheme: Scheme = Scheme.CENTROID, iterations: int = 5000, seed: int = None,
                 fit_iterations: int = 100, tolerance: float = 0.000001, device_id: int = 0, processes: int = 1):
        assert tolerance > 0
        assert scheme in Scheme
        if processes > 1:
            raise NotImplementedError("the assessment runs on one GPU (processes = 1)")
        observations = config.filter(data)
        why = _unsupported(config, observations)
        if why is not None:
            raise NotImplementedError("the assessment covers metric data without missing cells and without higher-order constructs: this model has " + why)
        n = observations.shape[0]
        if n < 10:
            raise Exception("Bootstrapping could not be performed, at least 10 observations are required.")
        if iterations < 10:
            iterations = 100
        calculator = pw.WeightsCalculatorFactory(config, max(fit_iterations, MIN_ITERATIONS), tolerance, np.sqrt(n / (n - 1)), scheme, device_id)
        whole = Estimator(config).run(calculator, observations, want_scores=False)
        native = whole.native
        native.assess_enable(True)
        if seed is None:
            seed = int.from_bytes(os.urandom(8), "little")
        native.bootstrap_device(iterations, seed, 0)
        self._init(native, whole.compiled, iterations)
        self._seed = seed

    @classmethod
    def of_bootstrap(cls, native, compiled, iterations):
        """The assessment of a bootstrap that already ran on ``native`` with ``assess_enable`` on (``Plspm(bootstrap=True, quality=True)``)."""
        self = cls.__new__(cls)
        self._init(native, compiled, iterations)
        self._seed = None
        return self

    def _init(self, native, cm, iterations):
        self._native, self._cm, self._iterations = native, cm, iterations
        self._lvs = list(cm.lvs)
        L = len(self._lvs)
        self._pairs = [(i, j) for i in range(L) for j in range(i + 1, L)]
        self._pair_labels = ["%s <-> %s" % (self._lvs[i], self._lvs[j]) for i, j in self._pairs]
        try:
            self._original, _ = native.assess_fit()
            self._table, self._used = native.assess_summary(iterations, self._original)
        except _native.NativeBackendError as err:
            raise NotImplementedError("no assessment on this handle: " + str(err))
        self._interval_cache = {}

    def _slice(self, criterion):
        if criterion not in CRITERIA:
            raise ValueError("criterion must be one of %s" % ", ".join(CRITERIA))
        L, npairs = len(self._lvs), len(self._pairs)
        if criterion in LV_CRITERIA:
            k = LV_CRITERIA.index(criterion)
            return slice(k * L, (k + 1) * L), self._lvs
        k = PAIR_CRITERIA.index(criterion)
        return slice(4 * L + k * npairs, 4 * L + (k + 1) * npairs), self._pair_labels

    def _square(self, criterion, diagonal):
        sl, _ = self._slice(criterion)
        L = len(self._lvs)
        out = np.full((L, L), np.nan)
        np.fill_diagonal(out, diagonal)
        for (i, j), value in zip(self._pairs, self._original[sl]):
            out[i, j] = out[j, i] = value
        return pd.DataFrame(out, index=self._lvs, columns=self._lvs)

    def reliability(self) -> pd.DataFrame:
        L = len(self._lvs)
        return pd.DataFrame(self._original[:4 * L].reshape(4, L).T, index=self._lvs, columns=list(LV_CRITERIA))

    def htmt(self) -> pd.DataFrame:
        return self._square("htmt", 1.0)

    def htmt2(self) -> pd.DataFrame:
        return self._square("htmt2", 1.0)

    def lv_correlations(self) -> pd.DataFrame:
        return self._square("lv_cor", 1.0)

    def fornell_larcker(self) -> pd.DataFrame:
        """sqrt(ave) on the diagonal, the construct correlations below it (NaN above)."""
        L = len(self._lvs)
        frame = self._square("lv_cor", np.sqrt(self._original[3 * L:4 * L]))
        frame.values[np.triu_indices(L, 1)] = np.nan
        return frame

    def summary(self, criterion) -> pd.DataFrame:
        sl, index = self._slice(criterion)
        return pd.DataFrame(self._table[sl], index=index, columns=SUMMARY_COLUMNS)

    def intervals(self, criterion, method="percentile", level=0.95) -> pd.DataFrame:
        if method not in INTERVAL_METHODS:
            raise ValueError("method must be one of %s" % ", ".join(INTERVAL_METHODS))
        if method == "bca":
            raise NotImplementedError("no bca intervals for the assessment criteria: the jackknife writes no assessment records")
        if not 0.0 < float(level) < 1.0:
            raise ValueError("level must lie strictly between 0 and 1")
        sl, index = self._slice(criterion)
        key = (method, float(level))
        if key not in self._interval_cache:
            table, _ = self._native.assess_intervals(self._iterations, self._original, method, float(level))
            self._interval_cache[key] = np.column_stack((self._original, table))
        return pd.DataFrame(self._interval_cache[key][sl], index=index, columns=INTERVAL_COLUMNS)

    def used(self) -> int:
        """Number of replicates that entered the summaries."""
        return self._used

    def seed(self):
        return self._seed

    def replicates(self):
        """The OK replicates' assessment records [n_used, A] (alpha | rho_a | rho_c | ave | htmt | htmt2 | lv_cor), fetched from HBM."""
        records, status = self._native.assess_fetch(0, self._iterations)
        return records[status == 0]
