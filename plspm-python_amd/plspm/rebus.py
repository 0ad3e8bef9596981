"""REBUS-PLS on the GPU (not in the reference): response-based unit segmentation, the search for classes of rows that differ in their outer AND inner model
(Esposito Vinzi, Trinchera, Squillacciotti and Tenenhaus 2008; ``rebus.pls`` / ``it.reb`` of the R package plspm).  ``Fimix`` finds classes from the inner model
alone; REBUS re-estimates the whole model in every class and moves each row to the class whose local model leaves it the smallest measurement and structural
residuals (include/plspm_hip.h ``plspm_rebus_*``).  This project's definitions (equality with R's numbers is not claimed).  Inputs: the N rows, K
classes (1..16), labels c^0 [N] below K.  Iteration t = 1, 2, ...:

    local models   problem k = the model on the rows with c^(t-1) = k, estimated like a bootstrap replicate (its own n_k, treatment and ``scaled`` scalar);
                   mean_pk, sd_pk the population mean and standard deviation of column p over the class's rows
    residuals      of every row i under every class k: y_ilk the score ``Plspm.scores()`` would give row i under class k's fit (the rule of out-of-sample
                   prediction: class means, the class's ``scaled`` scalar, the fit's weights and sign); z_ipk = (x_ip - mean_pk) / sd_pk;
                   e_ipk = z_ipk - lambda_pk y_i,lv(p),k; f_ijk = y_ijk - sum_{q in pred(j)} beta_kjq y_iqk for every LV j with predecessors;
                   A_ik = sum_p e_ipk^2 / lambda_pk^2;  B_ik = sum_j f_ijk^2 / R^2_jk
    closeness      CM_ik = sqrt( A_ik / (sum_i A_ik / (N - 2)) * B_ik / (sum_i B_ik / (N - 2)) ), both sums over all N rows
    assignment     c^t_i = argmin_k CM_ik (ties: the lowest k; a NaN never wins; a row whose every CM is NaN keeps its class); changed_t = #{i: c^t_i != c^(t-1)_i}
    stop           status 0 when changed_t / N < stop_crit; status 1 at t = max_iter (max_iter = 0: no iteration); status 2 at iteration t when a class has fewer
                   than min_size rows, a local fit does not converge, an sd_pk is 0, or a lambda_pk^2 or an R^2_jk is not above 1e-10 (``fimix.COLLAPSE_RTOL`` on
                   quantities in [0, 1]): the labels stay c^(t-1)
    final pass     local models, residuals and closeness once more on c^t without reassigning (the same checks: status 2 there as well): the reported local
                   models and CM, and per class the within-class sums sum_{i in k} e_ipk^2 [P] and sum_{i in k} f_ijk^2 [n_endo].  Skipped at status 2: labels and
                   history stay, everything else is NaN
    GQI            sqrt( sum_k (n_k / N) mean_p(1 - sum_{i in k} e_ipk^2 / n_k) * sum_k (n_k / N) mean_j(1 - sum_{i in k} f_ijk^2 / n_k) ), the means over all P
                   indicators and all n_endo endogenous LVs

``_rebus`` below is the same iteration in NumPy (fp64 or np.longdouble): the checker of the kernels.  Scope: metric data without missing cells and without
higher-order constructs, every block Mode A, a model with at least one path, one GPU; the Ward start runs on the host (start-up work, as ``hclust`` is in R).
"""
import numpy as np
import pandas as pd

import plspm.config as c
import plspm.weights as pw
from plspm.estimator import Estimator
from plspm.fimix import COLLAPSE_RTOL, MAX_SEGMENTS, Fimix, _direct_paths, _endogenous
from plspm.mga import MIN_GROUP_ROWS
from plspm.mode import Mode
from plspm.quality import _unsupported
from plspm.scheme import Scheme

STATUS_OK, STATUS_NOT_CONVERGED, STATUS_SINGULAR = 0, 1, 2
MAX_CLASSES = MAX_SEGMENTS
WARD_MAX_BYTES = 2 << 30        # of the condensed distance matrix, N (N - 1) / 2 doubles


def _unpack(row, P, L, eff_from, eff_to):
    """A device record [weights | r2 | total | direct | loadings] as the dict ``_rebus`` takes for a local model."""
    n_eff = len(eff_from)
    B = np.zeros((L, L))
    B[np.asarray(eff_to, dtype=np.int64), np.asarray(eff_from, dtype=np.int64)] = row[P + L + n_eff:P + L + 2 * n_eff]
    return dict(weights=row[:P], r2=row[P:P + L], path_coef=B, loadings=row[P + L + 2 * n_eff:])


def _class_residuals(X, blocks, C, scaled, rows, rec, dt):
    """e [N, P], f [N, n_endo] of every row of X under the local model ``rec`` of the rows ``rows``, in the dtype of X; None when the class is not valid."""
    if rec is None:
        return None
    Xk = X[rows]
    n = dt(Xk.shape[0])
    one = dt(1)
    mean = Xk.sum(axis=0) / n
    sd = np.sqrt(((Xk - mean) ** 2).sum(axis=0) / n)
    w, lam = np.asarray(rec["weights"], dtype=X.dtype), np.asarray(rec["loadings"], dtype=X.dtype)
    r2, Bk = np.asarray(rec["r2"], dtype=X.dtype), np.asarray(rec["path_coef"], dtype=X.dtype)
    endo = _endogenous(C)
    if not (sd > 0).all() or not (lam * lam > dt(COLLAPSE_RTOL)).all() or not (r2[endo] > dt(COLLAPSE_RTOL)).all():
        return None
    g = one
    if scaled:
        grand = Xk.sum() / (n * dt(X.shape[1]))
        g = np.sqrt(((Xk - grand) ** 2).sum() / (n * dt(X.shape[1]) - one)) * np.sqrt((n - one) / n)
    Y = np.empty((X.shape[0], len(blocks)), dtype=X.dtype)
    for l, b in enumerate(blocks):
        sign = -one if (w[b] * lam[b] * sd[b]).sum() < 0 else one
        Y[:, l] = sign * (((X[:, b] - mean[b]) / g) @ w[b])
    E = np.empty_like(X)
    for l, b in enumerate(blocks):
        E[:, b] = (X[:, b] - mean[b]) / sd[b] - lam[b] * Y[:, [l]]
    F = np.empty((X.shape[0], len(endo)), dtype=X.dtype)
    for jj, j in enumerate(endo):
        hat = np.zeros(X.shape[0], dtype=X.dtype)
        for q in np.flatnonzero(np.asarray(C)[j]):
            hat = hat + Bk[j, q] * Y[:, q]
        F[:, jj] = Y[:, j] - hat
    return E, F, lam, r2[endo]


def _closeness(X, blocks, C, scaled, labels, K, recs, dt):
    """One pass: (CM [N, K], E, F per class) on ``labels``, or None when a class is not valid."""
    N = X.shape[0]
    A, B, res = np.empty((N, K), dtype=X.dtype), np.empty((N, K), dtype=X.dtype), []
    for k in range(K):
        r = _class_residuals(X, blocks, C, scaled, labels == k, recs[k], dt)
        if r is None:
            return None
        E, F, lam, r2 = r
        A[:, k] = (E * E / (lam * lam)).sum(axis=1)
        B[:, k] = (F * F / r2).sum(axis=1)
        res.append((E, F))
    d = dt(N - 2)
    return np.sqrt((A / (A.sum(axis=0) / d)) * (B / (B.sum(axis=0) / d))), res


def _argmin(cm, old):
    """Row-wise argmin: ties to the lowest k, a NaN never wins, an all-NaN row keeps ``old``."""
    nan = np.isnan(cm)
    best = np.argmin(np.where(nan, np.inf, cm), axis=1)
    return np.where(nan.all(axis=1), old, best)


def _gqi(within_e, within_f, sizes):
    """The group quality index and its parts per class: (gqi, communality [K], r_squared [K])."""
    sizes = np.asarray(sizes)
    n = sizes.astype(within_e.dtype)
    com = (1 - within_e / n[:, None]).mean(axis=1)
    r2 = (1 - within_f / n[:, None]).mean(axis=1)
    share = n / n.sum()
    return np.sqrt((share * com).sum() * (share * r2).sum()), com, r2


def _rebus(X, model, K, start, max_iter=100, stop_crit=0.005, min_size=MIN_GROUP_ROWS, fit=None, records=None, dtype=np.float64):
    """The iteration in NumPy, in ``dtype`` (np.longdouble works).  X [N, P]; ``model`` has ``blocks`` (column indices of every LV), ``C`` (C[i, j] = 1 iff LV j -> LV i)
    and ``scaled``.  The local estimator is an argument: ``fit(Xk)`` returns dict(weights [P], loadings [P], path_coef [L, L], r2 [L]) of the fp64 rows Xk, or None
    where it does not converge; or ``records[s]`` gives the K dicts of pass s = 0, 1, ... (the iterations, then the final pass), so one step can be checked on given
    local models.  Returns a dict: status, iterations, labels, cm [N, K], records (of the final pass), sizes, within_e [K, P], within_f [K, n_endo], gqi, changed
    and hist_sizes per iteration, cm_trace (the CM of every iteration)."""
    dt = np.dtype(dtype).type
    X64 = np.asarray(X, dtype=np.float64)
    Xd = X64.astype(dtype)
    blocks, C, scaled = [np.asarray(b, dtype=np.int64) for b in model.blocks], np.asarray(model.C), bool(model.scaled)
    N, P = Xd.shape
    n_endo = len(_endogenous(C))
    labels = np.asarray(start, dtype=np.int64).copy()
    nan = dt(np.nan)
    out = dict(status=None, iterations=0, labels=labels, cm=np.full((N, K), nan), records=None, sizes=np.bincount(labels, minlength=K), within_e=np.full((K, P), nan),
               within_f=np.full((K, n_endo), nan), gqi=nan, changed=[], hist_sizes=[], cm_trace=[])
    passes = [0]

    def local(labels):
        s = passes[0]
        passes[0] += 1
        if records is not None:
            return list(records[s])
        return [fit(X64[labels == k]) for k in range(K)]

    t = 0
    while out["status"] is None:
        if t == max_iter:
            out["status"], out["iterations"] = STATUS_NOT_CONVERGED, t
            break
        sizes = np.bincount(labels, minlength=K)
        r = None if (sizes < min_size).any() else _closeness(Xd, blocks, C, scaled, labels, K, local(labels), dt)
        if r is None:
            out["status"], out["iterations"] = STATUS_SINGULAR, t + 1
            break
        cm = r[0]
        new = _argmin(cm, labels)
        changed = int((new != labels).sum())
        labels = new
        t += 1
        out["changed"].append(changed)
        out["hist_sizes"].append(np.bincount(labels, minlength=K))
        out["cm_trace"].append(cm)
        if dt(changed) / dt(N) < dt(stop_crit):
            out["status"], out["iterations"] = STATUS_OK, t
    out["labels"], out["sizes"] = labels, np.bincount(labels, minlength=K)
    if out["status"] != STATUS_SINGULAR:
        recs = None if (out["sizes"] < min_size).any() else local(labels)
        r = None if recs is None else _closeness(Xd, blocks, C, scaled, labels, K, recs, dt)
        if r is None:
            out["status"] = STATUS_SINGULAR
        else:
            out["cm"], out["records"] = r[0], recs
            for k, (E, F) in enumerate(r[1]):
                out["within_e"][k] = (E[labels == k] ** 2).sum(axis=0)
                out["within_f"][k] = (F[labels == k] ** 2).sum(axis=0)
            out["gqi"] = _gqi(out["within_e"], out["within_f"], out["sizes"])[0]
    return out


def _ward_check(n):
    if n * (n - 1) // 2 * 8 > WARD_MAX_BYTES:
        raise ValueError('start="ward" clusters on the host and needs the condensed distance matrix of N (N - 1) / 2 doubles: %.1f GiB for N = %d, more than 2 GiB.  '
                         "Give start= a column of data (or an aligned pd.Series / array of labels), or a Fimix object" % (n * (n - 1) / 2 * 8 / 2 ** 30, n))


def _start_labels(data, start, classes):
    """The labels 0 .. classes - 1 of a column of ``data``, an aligned pd.Series or an array: the sorted distinct values in order."""
    if isinstance(start, pd.Series):
        if not start.index.equals(data.index):
            raise ValueError("start: a pd.Series must be aligned on data.index (same labels in the same order)")
        values = start
    elif isinstance(start, (np.ndarray, list, tuple)):
        if len(start) != len(data):
            raise ValueError("start: an array of labels needs one label per row of data")
        values = pd.Series(np.asarray(start), index=data.index)
    else:
        try:
            present = start in data.columns
        except TypeError:
            present = False
        if not present:
            raise ValueError('start must be "ward", a Fimix object, a column label of data, or a pd.Series / array of labels aligned on data.index')
        values = data[start]
    if values.isnull().any():
        raise ValueError("start: %d row(s) have no label (NaN / None)" % int(values.isnull().sum()))
    levels = sorted(values.unique())
    if len(levels) != classes:
        raise ValueError("start has %d distinct labels, classes = %d" % (len(levels), classes))
    return values.map({lv: k for k, lv in enumerate(levels)}).values.astype(np.int64)


class Rebus:
    """``Rebus(data, config, scheme=Scheme.PATH, classes=2, start="ward", stop_crit=0.005, max_iter=100, min_size=10, iterations=100, tolerance=1e-6, device_id=0)``

    ``classes``: K, or a list of them (the runs go one after another on the same handle; every accessor then takes ``K``).  ``start``: "ward" (Ward's clustering of
    the one-class model's residuals, cut into K clusters, on the host), a ``Fimix`` object (its ``segments(K)``), a column of ``data``, or an aligned ``pd.Series`` /
    array of labels.  ``stop_crit`` and ``max_iter`` are R's defaults, ``min_size`` is ``mga.MIN_GROUP_ROWS``.

    Classes are numbered 1..K, largest first.  ``segments()``: a ``group`` column for ``GroupComparison`` / ``Micom``; ``sizes()``; ``path_coefficients()`` (paths
    "A -> B" x class.1..K), ``loadings()``, ``weights()`` (indicators x classes), ``r_squared()`` (endogenous LVs x classes): the local models; ``closeness()``: CM,
    rows x classes; ``history()``: per iteration ``changed`` and the sizes; ``status()``: status (0 converged, 1 ``max_iter`` reached, 2 a class collapsed) and
    iterations; ``residuals()``: e and f of every row under the one-class model; ``quality()``: per class its size, mean communality, mean R^2 and their root,
    then the row ``gqi`` (the size-weighted means and the group quality index) and the row ``one.class`` (the same for the model on all rows)."""

    def __init__(self, data: pd.DataFrame, config: c.Config, scheme: Scheme = Scheme.PATH, classes=2, start="ward", stop_crit: float = 0.005, max_iter: int = 100,
                 min_size: int = MIN_GROUP_ROWS, iterations: int = 100, tolerance: float = 0.000001, device_id: int = 0):
        assert tolerance > 0
        assert scheme in Scheme
        ks = [int(k) for k in classes] if isinstance(classes, (list, tuple, range, np.ndarray)) else [int(classes)]
        if not ks or min(ks) < 1 or max(ks) > MAX_CLASSES or len(set(ks)) != len(ks):
            raise ValueError("classes: a number of classes between 1 and %d, or a list of distinct ones" % MAX_CLASSES)
        if int(max_iter) < 0 or not float(stop_crit) >= 0 or int(min_size) < 1:
            raise ValueError("max_iter must be at least 0, stop_crit at least 0 and min_size at least 1")
        if not np.asarray(config.path().values).any():
            raise ValueError("REBUS-PLS needs an inner model: this model has no path")
        observations = config.filter(data)
        why = _unsupported(config, observations)
        if why is not None:
            raise NotImplementedError("REBUS-PLS covers metric data without missing cells and without higher-order constructs: this model has " + why)
        not_a = [lv for lv in config.path().index if config.mode(lv) != Mode.A]
        if not_a:
            raise NotImplementedError("REBUS-PLS covers Mode A blocks only: %s" % ", ".join(map(str, not_a)))
        n = observations.shape[0]
        by_ward, by_fimix = isinstance(start, str) and start == "ward", isinstance(start, Fimix)
        if by_ward:
            _ward_check(n)
        given = None if by_ward or by_fimix else {K: _start_labels(data, start, K) for K in ks}      # (no missing cells: the filter dropped no row)
        calculator = pw.WeightsCalculatorFactory(config, iterations, tolerance, np.sqrt(n / (n - 1)), scheme, device_id)
        whole = Estimator(config).run(calculator, observations, want_scores=False)
        native, cm = whole.native, whole.compiled
        self._native, self._index, self._lvs, self._mvs, self._ks, self._n = native, whole.index, list(cm.lvs), list(cm.dev_mvs), ks, n
        C = np.asarray(cm.path)
        self._paths, self._endo = _direct_paths(C), _endogenous(C)
        self._e, self._f = native.rebus_residuals()
        ward = None
        self._runs = {}
        for K in ks:
            if by_ward:
                from scipy.cluster import hierarchy
                if ward is None:
                    ward = hierarchy.linkage(np.column_stack((self._e, self._f)), method="ward")
                labels = hierarchy.fcluster(ward, K, criterion="maxclust").astype(np.int64) - 1
                if len(np.unique(labels)) != K:
                    raise ValueError("Ward's clustering of the residuals gives fewer than %d clusters" % K)
            elif by_fimix:
                seg = start.segments(K)
                if not seg.index.equals(whole.index):
                    raise ValueError("start: the Fimix object was fitted on other rows")
                labels = seg.values.astype(np.int64) - 1
            else:
                labels = given[K]
            run = native.rebus(K, labels, max_iter=int(max_iter), stop_crit=float(stop_crit), min_size=int(min_size))
            order = np.argsort(-run["sizes"], kind="stable")                # classes by size, largest first (ties: the device's order)
            rank = np.empty(K, dtype=np.int64)
            rank[order] = np.arange(K)
            run["order"], run["rank"] = order, rank
            self._runs[K] = run

    def _run(self, K):
        if K is None:
            if len(self._ks) != 1:
                raise ValueError("K must be one of %s" % ", ".join(str(k) for k in self._ks))
            K = self._ks[0]
        if K not in self._runs:
            raise ValueError("K must be one of %s" % ", ".join(str(k) for k in self._ks))
        return K, self._runs[K]

    @staticmethod
    def _names(K):
        return ["class.%d" % (k + 1) for k in range(K)]

    def _local(self, K):
        """The K local models in the reported order: a list of ``_unpack`` dicts."""
        K, run = self._run(K)
        nm = self._native
        return K, [_unpack(run["records"][k], nm.P, nm.L, nm.eff_from, nm.eff_to) for k in run["order"]]

    def status(self, K=None) -> pd.Series:
        K, run = self._run(K)
        return pd.Series({"status": run["status"], "iterations": run["iterations"]}, name="rebus")

    def sizes(self, K=None) -> pd.Series:
        K, run = self._run(K)
        return pd.Series(run["sizes"][run["order"]], index=self._names(K), name="size")

    def segments(self, K=None) -> pd.Series:
        K, run = self._run(K)
        return pd.Series(run["rank"][run["labels"]] + 1, index=self._index, name="group")

    def path_coefficients(self, K=None) -> pd.DataFrame:
        K, local = self._local(K)
        labels = ["%s -> %s" % (self._lvs[f], self._lvs[t]) for f, t in self._paths]
        return pd.DataFrame(np.column_stack([[m["path_coef"][t, f] for f, t in self._paths] for m in local]), index=labels, columns=self._names(K))

    def loadings(self, K=None) -> pd.DataFrame:
        K, local = self._local(K)
        return pd.DataFrame(np.column_stack([m["loadings"] for m in local]), index=self._mvs, columns=self._names(K))

    def weights(self, K=None) -> pd.DataFrame:
        K, local = self._local(K)
        return pd.DataFrame(np.column_stack([m["weights"] for m in local]), index=self._mvs, columns=self._names(K))

    def r_squared(self, K=None) -> pd.DataFrame:
        K, local = self._local(K)
        return pd.DataFrame(np.column_stack([m["r2"][self._endo] for m in local]), index=[self._lvs[j] for j in self._endo], columns=self._names(K))

    def closeness(self, K=None) -> pd.DataFrame:
        K, run = self._run(K)
        return pd.DataFrame(run["cm"][:, run["order"]], index=self._index, columns=self._names(K))

    def history(self, K=None) -> pd.DataFrame:
        K, run = self._run(K)
        frame = pd.DataFrame(run["hist_sizes"][:, run["order"]], index=pd.Index(range(1, len(run["changed"]) + 1), name="iteration"), columns=self._names(K))
        frame.insert(0, "changed", run["changed"])
        return frame

    def residuals(self) -> pd.DataFrame:
        return pd.DataFrame(np.column_stack((self._e, self._f)), index=self._index, columns=self._mvs + [self._lvs[j] for j in self._endo])

    def quality(self, K=None) -> pd.DataFrame:
        K, run = self._run(K)
        order = run["order"]
        sizes = run["sizes"][order]
        with np.errstate(divide="ignore", invalid="ignore"):
            gqi, com, r2 = _gqi(run["within_e"][order], run["within_f"][order], sizes)
            one, com1, r21 = _gqi((self._e ** 2).sum(axis=0)[None, :], (self._f ** 2).sum(axis=0)[None, :], np.array([self._n]))
            share = sizes / sizes.sum()
            rows = [[sizes[k], com[k], r2[k], np.sqrt(com[k] * r2[k])] for k in range(K)]
            rows.append([self._n, (share * com).sum(), (share * r2).sum(), gqi])
            rows.append([self._n, com1[0], r21[0], one])
        return pd.DataFrame(rows, index=self._names(K) + ["gqi", "one.class"], columns=["size", "communality", "r_squared", "root"])

    def gqi(self, K=None) -> float:
        return float(self.quality(K).loc["gqi", "root"])
