"""FIMIX-PLS on the GPU (not in the reference): latent-class segmentation of the inner model, the search for groups nobody recorded (Hahn, Johnson,
Herrmann and Huber 2002; Sarstedt, Becker, Ringle and Schwaiger 2011).

A finite mixture of inner-model regressions is fitted to the latent variable scores of one fit, by EM, from many random starts and for several numbers
of segments; all ``len(segments) x starts`` problems run in one device call, one persistent workgroup each (include/plspm_hip.h ``plspm_fimix_*``;
DESIGN.md 5s).  This project's definitions (equality with SmartPLS's numbers is not claimed), with Y [N, L] the scores, E the LVs that have
predecessors, pred(j) the predecessors of j, n_dir direct paths and n_endo = |E|:

    model          segment k: y_ij = sum_{p in pred(j)} beta_kjp y_ip + e, e ~ N(0, psi_kj); no intercept; the model is recursive (Jacobian 1)
    problem        (K, an initial hard assignment of the rows to K segments); P^0 its one-hot matrix
    M-step on P    n_k = sum_i P_ik, rho_k = n_k / N, m_k[a, b] = sum_i P_ik y_ia y_ib; beta_kj solves m_k[pred, pred] beta = m_k[pred, j] by the project's
                   regression (Cholesky if every pivot passes PLSPM_PIVOT_RTOL, otherwise the minimum-norm answer); psi_kj = (m_k[j, j] - beta_kj . m_k[pred, j]) / n_k
    collapse       status 2 (singular) at that iteration when an n_k < 1, a psi_kj <= 1e-10 m_k[j, j] / n_k or a regression has no answer: the record is NaN
    E-step         a_ik = ln rho_k + sum_j [-1/2 ln(2 pi psi_kj) - r_ikj^2 / (2 psi_kj)]; lse_i the log-sum-exp over k (row maximum subtracted);
                   lnL = sum_i lse_i; P_ik = exp(a_ik - lse_i); H = -sum_ik P_ik ln P_ik (0 ln 0 = 0); status 3 when lnL is not finite
    stop           status 0 when t >= 2 and |lnL^t - lnL^(t-1)| <= tol (an absolute change); status 1 at t = max_iter with the complete record of that t
    record         lnL | H | rho[Kmax] | beta[Kmax][n_dir] | psi[Kmax][n_endo]; beta from-major ("A -> B" by A, then B), psi in LV order, NaN in slots k >= K
    criteria       N_K = (K - 1) + K (n_dir + n_endo); -2 lnL + penalty: AIC 2 N_K, AIC3 3 N_K, AIC4 4 N_K, BIC ln N N_K, CAIC (ln N + 1) N_K,
                   HQ 2 ln(ln N) N_K, MDL5 5 ln N N_K; EN = 1 - H / (N ln K), NaN for K = 1
    solution       of a K: the start of status 0 with the largest lnL, ties to the lowest start

``_fimix`` below is the same iteration in NumPy (fp64 or np.longdouble): the checker of the kernel.  Scope: metric data without missing cells and without
higher-order constructs, one GPU; no intercepts, no re-estimation of the outer model per segment (``GroupComparison`` / ``Micom`` on ``segments(2)`` do that).
"""
import os

import numpy as np
import pandas as pd

import plspm.config as c
import plspm.weights as pw
from plspm.estimator import Estimator
from plspm.plsc import STATUS_NONFINITE, STATUS_OK, STATUS_SINGULAR, _regress
from plspm.quality import _unsupported
from plspm.scheme import Scheme

STATUS_NOT_CONVERGED = 1
MAX_SEGMENTS = 16
COLLAPSE_RTOL = 1e-10
CRITERIA = ("lnl", "aic", "aic3", "aic4", "bic", "caic", "hq", "mdl5", "en", "start", "used")


def _direct_paths(C):
    """The direct paths (from, to) of the path matrix C (C[i, j] = 1 iff LV j -> LV i), from-major: the order of the record's beta."""
    C = np.asarray(C) != 0
    L = C.shape[0]
    return [(f, t) for f in range(L) for t in range(L) if C[t, f]]


def _endogenous(C):
    C = np.asarray(C) != 0
    return [j for j in range(C.shape[0]) if C[j].any()]


def record_width(kmax, n_dir, n_endo):
    return 2 + kmax * (1 + n_dir + n_endo)


def _fimix(Y, path, K, init, max_iter, tol, solve=None, snapshots=()):
    """One EM problem in NumPy, in the dtype of Y (np.longdouble works): Y [N, L] scores, path [L, L] (path[i, j] = 1 iff LV j -> LV i), init [N] segments
    below K.  ``solve(A, b)``: another regression in place of the project's rule (a test passes numpy.linalg.pinv).  Returns a dict: status, iterations,
    lnl, h, rho [K], beta [K, n_dir], psi [K, n_endo] (NaN unless the status is 0 or 1), posteriors [N, K] of the last E-step, trace (lnL of every
    iteration), paths, endo.  ``snapshots``: iteration numbers whose complete state is kept as well, out["snapshots"][t] -- what a run of max_iter = t returns while t is below
    the iteration this run stops at.  (tol = 0 stops where lnL repeats exactly: a problem of one segment at t = 2.)"""
    Y = np.asarray(Y)
    dt = Y.dtype.type
    C = np.asarray(path) != 0
    N, L = Y.shape
    paths, endo = _direct_paths(C), _endogenous(C)
    preds = [np.flatnonzero(C[j]) for j in endo]
    n_dir, n_endo = len(paths), len(endo)
    init = np.asarray(init)
    P = np.zeros((N, K), dtype=Y.dtype)
    P[np.arange(N), init] = dt(1)
    two_pi = dt(8) * np.arctan(dt(1))
    nan = dt(np.nan)
    out = dict(status=None, iterations=0, lnl=nan, h=nan, rho=np.full(K, nan), beta=np.full((K, n_dir), nan), psi=np.full((K, n_endo), nan), posteriors=None, trace=[],
               paths=paths, endo=endo, snapshots={})

    def state(status, t, lnl, h, rho, beta, psi, P):
        flat = np.zeros((K, n_dir), dtype=Y.dtype)
        for k in range(K):
            for je, j in enumerate(endo):
                for r, p in enumerate(preds[je]):
                    flat[k, paths.index((int(p), j))] = beta[k][je][r]
        return dict(status=status, iterations=t, lnl=lnl, h=h, rho=rho, beta=flat, psi=psi.copy(), posteriors=P)
    before = None
    t = 0
    while True:
        t += 1
        out["iterations"] = t
        nk = P.sum(axis=0)
        collapse = bool(np.any(~(nk >= 1)))
        beta = [[None] * n_endo for _ in range(K)]
        psi = np.zeros((K, n_endo), dtype=Y.dtype)
        with np.errstate(divide="ignore", invalid="ignore"):
            for k in range(K):
                w = P[:, k]
                for je, j in enumerate(endo):
                    S = preds[je]
                    WY = Y[:, S] * w[:, None]
                    A, b, mjj = WY.T @ Y[:, S], WY.T @ Y[:, j], (w * Y[:, j] * Y[:, j]).sum()
                    if solve is None:
                        x, ok, _ = _regress(A, b)
                    else:
                        x, ok = np.asarray(solve(A, b), dtype=Y.dtype), True
                    beta[k][je] = x
                    psi[k, je] = (mjj - x @ b) / nk[k]
                    if not ok or not psi[k, je] > dt(COLLAPSE_RTOL) * mjj / nk[k]:
                        collapse = True
        if collapse:
            out["status"] = STATUS_SINGULAR
            return out
        rho = nk / dt(N)
        a = np.empty((N, K), dtype=Y.dtype)
        for k in range(K):
            acc = np.full(N, np.log(rho[k]) - np.log(two_pi * psi[k]).sum() / dt(2), dtype=Y.dtype)
            for je, j in enumerate(endo):
                r = Y[:, j] - Y[:, preds[je]] @ beta[k][je]
                acc = acc - r * r * (dt(1) / (dt(2) * psi[k, je]))
            a[:, k] = acc
        mx = a.max(axis=1)
        lse = mx + np.log(np.exp(a - mx[:, None]).sum(axis=1))
        lnl = lse.sum()
        lp = a - lse[:, None]
        P = np.exp(lp)
        h = -np.where(P > 0, P * lp, dt(0)).sum()
        out["trace"].append(lnl)
        if not np.isfinite(lnl):
            out["status"] = STATUS_NONFINITE
            return out
        done = STATUS_OK if (t >= 2 and abs(lnl - before) <= tol) else (STATUS_NOT_CONVERGED if t >= max_iter else None)
        if t in snapshots:
            out["snapshots"][t] = state(STATUS_NOT_CONVERGED if done is None else done, t, lnl, h, rho, beta, psi, P)
        if done is not None:
            out.update(state(done, t, lnl, h, rho, beta, psi, P))
            return out
        before = lnl


def _record(out, kmax):
    """The device's record of a ``_fimix`` result, width 2 + kmax (1 + n_dir + n_endo)."""
    K, n_dir = out["beta"].shape
    n_endo = out["psi"].shape[1]
    rec = np.full(record_width(kmax, n_dir, n_endo), np.nan, dtype=out["beta"].dtype)
    if out["status"] in (STATUS_OK, STATUS_NOT_CONVERGED):
        rec[0], rec[1] = out["lnl"], out["h"]
        rec[2:2 + K] = out["rho"]
        rec[2 + kmax:2 + kmax + K * n_dir] = out["beta"].ravel()
        rec[2 + kmax * (1 + n_dir):2 + kmax * (1 + n_dir) + K * n_endo] = out["psi"].ravel()
    return rec


def _criteria(lnl, h, N, K, n_dir, n_endo):
    """The information criteria and the normed entropy of one solution."""
    nk = (K - 1) + K * (n_dir + n_endo)
    ln_n = np.log(N)
    with np.errstate(divide="ignore", invalid="ignore"):
        en = np.float64(1.0) - np.float64(h) / (N * np.log(np.float64(K))) if K > 1 else np.nan
    return dict(lnl=lnl, aic=-2 * lnl + 2 * nk, aic3=-2 * lnl + 3 * nk, aic4=-2 * lnl + 4 * nk, bic=-2 * lnl + ln_n * nk, caic=-2 * lnl + (ln_n + 1) * nk,
                hq=-2 * lnl + 2 * np.log(ln_n) * nk, mdl5=-2 * lnl + 5 * ln_n * nk, en=en)


class Fimix:
    """``Fimix(data, config, scheme=Scheme.PATH, segments=range(1, 6), starts=10, em_iterations=5000, em_tolerance=1e-10, iterations=100, tolerance=1e-6,
    seed=None, device_id=0)`` -- the model is fitted once, then ``starts`` random starts for every K of ``segments`` run as one device call.

    ``criteria()``: K x (lnl, aic, aic3, aic4, bic, caic, hq, mdl5, en, start, used); ``sizes(K)``, ``path_coefficients(K)`` (paths "A -> B" x segment.1..K),
    ``residual_variances(K)``: the solution of K, segments by size, largest first; ``posteriors(K)``: rows x segments; ``segments(K)``: 1..K by largest
    posterior -- a ``group`` column for ``GroupComparison`` / ``Micom`` when K = 2; ``starts(K)``: lnl, status, iterations of every start; ``records()``;
    ``used()``; ``seed()``."""

    def __init__(self, data: pd.DataFrame, config: c.Config, scheme: Scheme = Scheme.PATH, segments=range(1, 6), starts: int = 10, em_iterations: int = 5000,
                 em_tolerance: float = 1e-10, iterations: int = 100, tolerance: float = 0.000001, seed: int = None, device_id: int = 0):
        assert tolerance > 0
        assert scheme in Scheme
        ks = [int(k) for k in segments]
        if not ks or min(ks) < 1 or max(ks) > MAX_SEGMENTS or len(set(ks)) != len(ks):
            raise ValueError("segments: distinct numbers of segments between 1 and %d" % MAX_SEGMENTS)
        if int(starts) < 1:
            raise ValueError("starts must be at least 1")
        if int(em_iterations) < 1 or not float(em_tolerance) >= 0:
            raise ValueError("em_iterations must be at least 1 and em_tolerance at least 0")
        if not np.asarray(config.path().values).any():
            raise ValueError("FIMIX-PLS needs an inner model: this model has no path")
        observations = config.filter(data)
        why = _unsupported(config, observations)
        if why is not None:
            raise NotImplementedError("FIMIX-PLS covers metric data without missing cells and without higher-order constructs: this model has " + why)
        n = observations.shape[0]
        calculator = pw.WeightsCalculatorFactory(config, iterations, tolerance, np.sqrt(n / (n - 1)), scheme, device_id)
        whole = Estimator(config).run(calculator, observations, want_scores=True)
        native, cm = whole.native, whole.compiled
        if seed is None:
            seed = int.from_bytes(os.urandom(8), "little")
        self._seed, self._ks, self._starts, self._n = seed, ks, int(starts), n
        self._native, self._index, self._lvs = native, whole.index, list(cm.lvs)
        C = np.asarray(cm.path)
        self._paths, self._endo = _direct_paths(C), _endogenous(C)
        self._kmax = max(ks)
        # problem ki * starts + s: start s of the ki-th K; its rows are drawn on the device from (seed, ki * starts + s)
        native.fimix(np.repeat(ks, self._starts), kmax=self._kmax, seed=seed, start_offset=0, init=None, max_iter=int(em_iterations), tol=float(em_tolerance))
        self._records, self._status, self._iters = native.fimix_fetch()
        self._best = {}
        for ki, K in enumerate(ks):
            sl = slice(ki * self._starts, (ki + 1) * self._starts)
            ok = self._status[sl] == STATUS_OK
            self._best[K] = int(np.argmax(np.where(ok, self._records[sl, 0], -np.inf))) if ok.any() else -1

    def _k(self, K):
        if K not in self._ks:
            raise ValueError("K must be one of %s" % ", ".join(str(k) for k in self._ks))
        return self._ks.index(K)

    def _solution(self, K):
        """(problem, rho, beta [K, n_dir], psi [K, n_endo], order) of the solution of K, the segments by rho descending (ties: the EM's order)."""
        ki = self._k(K)
        if self._best[K] < 0:
            raise ValueError("no start of K = %d converged without collapsing: see starts(%d)" % (K, K))
        problem = ki * self._starts + self._best[K]
        rec, kmax, n_dir, n_endo = self._records[problem], self._kmax, len(self._paths), len(self._endo)
        rho = rec[2:2 + K]
        beta = rec[2 + kmax:2 + kmax + K * n_dir].reshape(K, n_dir)
        psi = rec[2 + kmax * (1 + n_dir):2 + kmax * (1 + n_dir) + K * n_endo].reshape(K, n_endo)
        order = np.argsort(-rho, kind="stable")
        return problem, rho[order], beta[order], psi[order], order

    @staticmethod
    def _names(K):
        return ["segment.%d" % (k + 1) for k in range(K)]

    def criteria(self) -> pd.DataFrame:
        rows = []
        for ki, K in enumerate(self._ks):
            sl = slice(ki * self._starts, (ki + 1) * self._starts)
            used = int((self._status[sl] == STATUS_OK).sum())
            if self._best[K] < 0:
                rows.append([np.nan] * 9 + [-1, used])
                continue
            rec = self._records[ki * self._starts + self._best[K]]
            crit = _criteria(rec[0], rec[1], self._n, K, len(self._paths), len(self._endo))
            rows.append([crit[name] for name in CRITERIA[:9]] + [self._best[K], used])
        return pd.DataFrame(rows, index=pd.Index(self._ks, name="K"), columns=list(CRITERIA))

    def sizes(self, K) -> pd.Series:
        return pd.Series(self._solution(K)[1], index=self._names(K), name="size")

    def path_coefficients(self, K) -> pd.DataFrame:
        labels = ["%s -> %s" % (self._lvs[f], self._lvs[t]) for f, t in self._paths]
        return pd.DataFrame(self._solution(K)[2].T, index=labels, columns=self._names(K))

    def residual_variances(self, K) -> pd.DataFrame:
        return pd.DataFrame(self._solution(K)[3].T, index=[self._lvs[j] for j in self._endo], columns=self._names(K))

    def posteriors(self, K) -> pd.DataFrame:
        problem, _, _, _, order = self._solution(K)
        return pd.DataFrame(self._native.fimix_posteriors(problem)[:, order], index=self._index, columns=self._names(K))

    def segments(self, K) -> pd.Series:
        return pd.Series(np.argmax(self.posteriors(K).values, axis=1) + 1, index=self._index, name="segment")

    def starts(self, K) -> pd.DataFrame:
        ki = self._k(K)
        sl = slice(ki * self._starts, (ki + 1) * self._starts)
        return pd.DataFrame({"lnl": self._records[sl, 0], "status": self._status[sl], "iterations": self._iters[sl]}, index=pd.Index(range(self._starts), name="start"),
                            columns=["lnl", "status", "iterations"])

    def records(self):
        """(records [len(segments) * starts, width], status, iterations): problem ki * starts + s is start s of the ki-th K."""
        return self._records, self._status, self._iters

    def used(self) -> pd.Series:
        """Per K the number of starts of status 0."""
        return pd.Series([int((self._status[ki * self._starts:(ki + 1) * self._starts] == STATUS_OK).sum()) for ki in range(len(self._ks))],
                         index=pd.Index(self._ks, name="K"), name="used")

    def seed(self):
        return self._seed
