"""Moderation analysis with bootstrap inference on the GPU (not in the reference): does the effect of a predictor on a target depend on a moderator?
Interaction terms by the two-stage approach (Chin et al. 2003; Henseler and Chin 2010; Becker et al. 2018).

Stage 1 is the main-effects model as it stands.  Stage 2 regresses every target that has terms on the stage-1 scores of its predecessors and on the products
of the standardised scores.  Every replicate's products are formed on the device from that replicate's own weights, in a pass over the rows behind the
solver (include/plspm_hip.h ``plspm_moderation_*``) -- no record and no moment matrix holds sum_i c_i y_a y_b y_l.  This project's definitions,
for one data set (the full sample, or one replicate with row multiplicities c_i, sum c_i = n):

    term           (predictor a, moderator b, target j): three different LVs, a -> j and b -> j paths of the model; at most 8; no two with the same {a, b} and j
    y_l            the stage-1 score by ``plspm.quality``'s conventions on the data set's own weighted means mu_p, population sds s_p and indicator
                   correlations R: v_p = w_p s_p normalised per block so that v_l' R_ll v_l = 1, sigma_l the sign rule, y_il = sigma_l sum_p v_p (x_ip - mu_p) / s_p
                   (mean 0, variance 1; an item without variance contributes 0)
    z_t            y_a y_b, neither centred nor rescaled; its standard deviation counts as zero unless its variance exceeds 1e-9 of its second moment
    correlations   of the L scores and the T products: weighted, over the rows
    stage 2        per target j that has terms: j on pred(j) in LV order, then on its terms in term order, on that correlation matrix by the project's own
                   regression (``plspm.plsc._regress``); R2 = beta' r.  A target without terms keeps its stage-1 values (the bootstrap record's)
    f2_t           (R2_j - R2_j without term t) / (1 - R2_j)
    slopes         slope_low_t = direct2[a -> j] - interaction_t, slope_high_t = direct2[a -> j] + interaction_t: the simple slope of a one SD below / above
                   the moderator's mean
    record         direct2[n_dir] | interaction[T] | f2[T] | slope_low[T] | slope_high[T] | r2[L], then status and iterations; direct paths in the order of
                   the effect pairs (from-major) restricted to direct paths
    status         the bootstrap record's if that failed (NaN everywhere); 2 (singular) when a regression reports failure, 3 (non-finite) when a value is
                   not finite (a product without variance, an R2 of 1) -- the values stand

``_moderation`` below is the same statistic in NumPy at the level of the data: the checker of the kernels.  Scope: metric data without missing cells and
without higher-order constructs, one GPU, at most 65,535 rows; no bca intervals (the jackknife writes no moderation records); the products are those of the
composites' scores, not PLSc-corrected; no quadratic terms (a = b) and no three-way interactions.
"""
import os

import numpy as np
import pandas as pd

import plspm.config as c
import plspm.weights as pw
from plspm import _native
from plspm.bootstrap import INTERVAL_COLUMNS, INTERVAL_METHODS, SUMMARY_COLUMNS
from plspm.estimator import Estimator
from plspm.plsc import STATUS_NONFINITE, STATUS_OK, STATUS_SINGULAR, _effect_pairs, _regress
from plspm.quality import MIN_ITERATIONS, _unsupported
from plspm.scheme import Scheme

MAX_TERMS = 8
MAX_ROWS = 65535
WHAT = ("direct", "interaction", "f2", "slope_low", "slope_high", "r2")
VARIANCE_RTOL = 1e-9            # csrc/kernels_moments.h mv_stats, csrc/moderation_core.h: a variance below this share of the second moment counts as zero


def _check_terms(C, terms, names=None):
    """The terms as a list of (a, b, j) LV indices, checked against the path matrix C (C[i, j] = 1 iff LV j -> LV i).  ``terms``: triples of indices, or of
    names when ``names`` lists the LVs.  ValueError for a term the definitions do not cover."""
    C = np.asarray(C)
    L = C.shape[0]
    out = []
    label = (lambda l: names[l]) if names is not None else str
    for term in terms:
        if len(term) != 3:
            raise ValueError("an interaction is (predictor, moderator, target)")
        if names is not None:
            unknown = [x for x in term if x not in names]
            if unknown:
                raise ValueError("unknown latent variable in an interaction: " + ", ".join(map(str, unknown)))
            term = tuple(names.index(x) for x in term)
        a, b, j = (int(x) for x in term)
        if not all(0 <= x < L for x in (a, b, j)):
            raise ValueError("latent variable out of range in an interaction")
        if len({a, b, j}) != 3:
            raise ValueError("predictor, moderator and target of an interaction must be three different latent variables")
        for x in (a, b):
            if not C[j, x]:
                raise ValueError("the interaction %s x %s -> %s needs the path %s -> %s in the model: add the path" % (label(a), label(b), label(j), label(x), label(j)))
        if any(j == j2 and {a, b} == {a2, b2} for a2, b2, j2 in out):
            raise ValueError("the interaction %s x %s -> %s is listed twice" % (label(a), label(b), label(j)))
        out.append((a, b, j))
    if not out:
        raise ValueError("at least one interaction")
    if len(out) > MAX_TERMS:
        raise ValueError("at most %d interactions (%d given)" % (MAX_TERMS, len(out)))
    return out


def _direct_paths(C):
    return [(f, t) for f, t in _effect_pairs(C) if C[t, f]]


def _weighted_correlation(F, counts, n, product):
    """The weighted correlation matrix of the columns of F [N, k]; ``product`` [k] marks the columns whose standard deviation takes the zero rule."""
    dt = F.dtype.type
    mean = (counts[:, None] * F).sum(axis=0) / n
    D = F - mean
    cov = (D * counts[:, None]).T @ D / n
    var = np.diag(cov).copy()
    second = (counts[:, None] * F * F).sum(axis=0) / n
    sd = np.sqrt(np.where(var > 0, var, dt(0)))
    sd = np.where(product & ~(var > dt(VARIANCE_RTOL) * second), dt(0), sd)
    with np.errstate(divide="ignore", invalid="ignore"):
        E = cov / np.outer(sd, sd)
    E[np.diag_indices_from(E)] = dt(1)
    return E, sd


def _moderation(X, counts, w, lam, blocks, modes, C, terms, dtype=np.float64, record_direct=None, record_r2=None):
    """The moderation record of one data set at the level of the data: X [N, P] its rows (any shift), counts [N] the row multiplicities (None: all 1), w [P]
    the outer weights of the columns as they are, lam [P] the loadings, blocks the column indices of every LV, modes per LV (unused: the weights are given), C
    the path matrix (C[i, j] = 1 iff LV j -> LV i), terms the (a, b, j) triples.  record_direct [n_eff] / record_r2 [L]: the bootstrap record's entries a target
    without terms keeps (None: the stage-1 regression on the scores' correlations).  Everything in ``dtype`` -- np.longdouble works.  Returns a dict: status,
    direct2, interaction, f2, slope_low, slope_high, r2, record, paths, terms, scores [N, L], products [N, T], product_sd [T] and pivots_pass (every
    regression was solved, none went to the pseudo-inverse)."""
    dt = np.dtype(dtype).type
    X = np.asarray(X, dtype=dtype)
    N, P = X.shape
    counts = np.ones(N, dtype=dtype) if counts is None else np.asarray(counts, dtype=dtype)
    w, lam = np.asarray(w, dtype=dtype), np.asarray(lam, dtype=dtype)
    blocks = [np.asarray(b, dtype=np.int64) for b in blocks]
    C = np.asarray(C)
    L = len(blocks)
    terms = _check_terms(C, terms)
    T = len(terms)
    n = counts.sum()
    one, zero = dt(1), dt(0)
    mu = (counts[:, None] * X).sum(axis=0) / n
    D = X - mu
    var = (counts[:, None] * D * D).sum(axis=0) / n
    second = (counts[:, None] * X * X).sum(axis=0) / n
    varies = var > dt(VARIANCE_RTOL) * second
    s = np.where(varies, np.sqrt(np.where(varies, var, one)), zero)
    Xs = np.where(varies, D / np.where(varies, s, one), zero)
    R = (Xs * counts[:, None]).T @ Xs / n
    v = w * s
    Y = np.empty((N, L), dtype=dtype)
    for l, blk in enumerate(blocks):
        Rb = R[np.ix_(blk, blk)].copy()
        Rb[np.diag_indices_from(Rb)] = one
        vb = v[blk] / np.sqrt(v[blk] @ Rb @ v[blk])
        sigma = -one if ((Rb @ vb) * lam[blk]).sum() < 0 else one
        Y[:, l] = sigma * (Xs[:, blk] @ vb)
    Z = np.column_stack([Y[:, a] * Y[:, b] for a, b, _ in terms])
    pairs = _effect_pairs(C)
    paths = [(f, t) for f, t in pairs if C[t, f]]
    n_dir = len(paths)
    direct2 = np.empty(n_dir, dtype=dtype)
    r2 = np.zeros(L, dtype=dtype)
    inter, f2 = np.empty(T, dtype=dtype), np.empty(T, dtype=dtype)
    status, pivots_pass = STATUS_OK, True
    product_sd = np.full(T, np.nan, dtype=dtype)
    for j in range(L):
        pred = np.flatnonzero(C[j]).tolist()
        mine = [t for t, term in enumerate(terms) if term[2] == j]
        k, m = len(pred), len(mine)
        if not mine:
            if record_r2 is not None:
                r2[j] = record_r2[j]
            for f in pred:
                d = paths.index((f, j))
                if record_direct is not None:
                    direct2[d] = record_direct[pairs.index((f, j))]
            if record_direct is None and pred:
                E, _ = _weighted_correlation(Y[:, pred + [j]], counts, n, np.zeros(k + 1, dtype=bool))
                x, ok, solved = _regress(E[:k, :k], E[:k, k])
                pivots_pass = pivots_pass and solved
                if not ok:
                    status = STATUS_SINGULAR
                for pos, f in enumerate(pred):
                    direct2[paths.index((f, j))] = x[pos]
                if record_r2 is None:
                    r2[j] = x @ E[:k, k]
            continue
        F = np.column_stack([Y[:, pred], Z[:, mine], Y[:, [j]]])
        E, sd = _weighted_correlation(F, counts, n, np.array([False] * k + [True] * m + [False]))
        product_sd[mine] = sd[k:k + m]
        if not np.all(np.isfinite(E.astype(np.float64))):      # a product without variance: nothing regressed on its correlations is a number
            r2[j] = np.nan
            for f in pred:
                direct2[paths.index((f, j))] = np.nan
            inter[mine], f2[mine] = np.nan, np.nan
            continue
        with np.errstate(divide="ignore", invalid="ignore"):
            x, ok, solved = _regress(E[:k + m, :k + m], E[:k + m, k + m])
            pivots_pass = pivots_pass and solved
            if not ok:
                status = STATUS_SINGULAR
            full = x @ E[:k + m, k + m]
            r2[j] = full
            for pos, f in enumerate(pred):
                direct2[paths.index((f, j))] = x[pos]
            for q, t in enumerate(mine):
                inter[t] = x[k + q]
                keep = [r for r in range(k + m) if r != k + q]
                xd, ok, solved = _regress(E[np.ix_(keep, keep)], E[keep, k + m])
                pivots_pass = pivots_pass and solved
                if not ok:
                    status = STATUS_SINGULAR
                f2[t] = (full - xd @ E[keep, k + m]) / (one - full)
    main = np.array([direct2[paths.index((a, j))] for a, _, j in terms], dtype=dtype)
    low, high = main - inter, main + inter
    record = np.concatenate((direct2, inter, f2, low, high, r2))
    if status == STATUS_OK and not np.all(np.isfinite(record.astype(np.float64))):
        status = STATUS_NONFINITE
    return dict(status=status, direct2=direct2, interaction=inter, f2=f2, slope_low=low, slope_high=high, r2=r2, record=record, paths=paths, terms=terms, scores=Y,
                products=Z, product_sd=product_sd, pivots_pass=pivots_pass)


def _term_names(config, interactions):
    """The (a, b, j) LV indices of the named interactions, checked against the model's path matrix."""
    path = config.path()
    return _check_terms(path.values, list(interactions), list(path))


class Moderation:
    """``Moderation(data, config, scheme=Scheme.CENTROID, interactions=[("IMAG", "EXPE", "SAT")], iterations=5000, seed=None, fit_iterations=100,
    tolerance=1e-6, device_id=0, processes=1)`` -- ``interactions``: (predictor, moderator, target) names; ``iterations`` bootstrap replicates.  Also
    ``Plspm(..., bootstrap=True, interactions=[...]).moderation()``.

    ``effects()``: terms "A x M -> B" x (predictor, moderator, target, interaction, f2, slope.low, slope.high) of the full sample; ``path_coefficients()``:
    paths "A -> B" x (main, moderated); ``r_squared()``: LVs x (main, moderated); ``simple_slopes(at)``: the slope of the predictor at moderator values in
    SDs; ``summary(what)`` / ``intervals(what, method, level)`` for what in ("direct", "interaction", "f2", "slope_low", "slope_high", "r2"); ``used()``;
    ``seed()``; ``status()``; ``replicates()``."""

    def __init__(self, data: pd.DataFrame, config: c.Config, scheme: Scheme = Scheme.CENTROID, interactions=None, iterations: int = 5000, seed: int = None,
                 fit_iterations: int = 100, tolerance: float = 0.000001, device_id: int = 0, processes: int = 1):
        assert tolerance > 0
        assert scheme in Scheme
        if processes > 1:
            raise NotImplementedError("the moderation analysis runs on one GPU (processes = 1)")
        observations = config.filter(data)
        why = _unsupported(config, observations)
        if why is not None:
            raise NotImplementedError("the moderation analysis covers metric data without missing cells and without higher-order constructs: this model has " + why)
        terms = _term_names(config, interactions or [])
        n = observations.shape[0]
        if n > MAX_ROWS:
            raise NotImplementedError("the moderation analysis covers at most %d rows: this data set has %d" % (MAX_ROWS, n))
        if n < 10:
            raise Exception("Bootstrapping could not be performed, at least 10 observations are required.")
        if iterations < 10:
            iterations = 100
        calculator = pw.WeightsCalculatorFactory(config, max(fit_iterations, MIN_ITERATIONS), tolerance, np.sqrt(n / (n - 1)), scheme, device_id)
        whole = Estimator(config).run(calculator, observations, want_scores=False)
        native = whole.native
        native.moderation_enable(terms)
        if seed is None:
            seed = int.from_bytes(os.urandom(8), "little")
        native.bootstrap_device(iterations, seed, 0)
        self._init(native, whole.compiled, iterations, terms)
        self._seed = seed

    @classmethod
    def of_bootstrap(cls, native, compiled, iterations, terms):
        """The analysis of a bootstrap that already ran on ``native`` with ``moderation_enable(terms)`` (``Plspm(bootstrap=True, interactions=[...])``)."""
        self = cls.__new__(cls)
        self._init(native, compiled, iterations, terms)
        self._seed = None
        return self

    def _init(self, native, cm, iterations, terms):
        self._native, self._cm, self._iterations, self._terms = native, cm, iterations, list(terms)
        lvs = self._lvs = list(cm.lvs)
        try:
            self._original, self._status = native.moderation_fit()
            self._table, self._used = native.moderation_summary(iterations, self._original)
        except _native.NativeBackendError as err:
            raise NotImplementedError("no moderation analysis on this handle: " + str(err))
        self._paths = _direct_paths(np.asarray(cm.path))
        self._path_labels = ["%s -> %s" % (lvs[f], lvs[t]) for f, t in self._paths]
        self._term_labels = ["%s x %s -> %s" % (lvs[a], lvs[b], lvs[j]) for a, b, j in self._terms]
        self._interval_cache = {}

    def _slice(self, what):
        if what not in WHAT:
            raise ValueError("what must be one of %s" % ", ".join(WHAT))
        n_dir, T, L = len(self._paths), len(self._terms), len(self._lvs)
        if what == "direct":
            return slice(0, n_dir), self._path_labels
        if what == "r2":
            return slice(n_dir + 4 * T, n_dir + 4 * T + L), self._lvs
        k = WHAT.index(what) - 1
        return slice(n_dir + k * T, n_dir + (k + 1) * T), self._term_labels

    def status(self) -> int:
        """Status of the full-sample record (0: fine)."""
        return self._status

    def effects(self) -> pd.DataFrame:
        lvs = self._lvs
        part = lambda what: self._original[self._slice(what)[0]]
        return pd.DataFrame({"predictor": [lvs[a] for a, _, _ in self._terms], "moderator": [lvs[b] for _, b, _ in self._terms],
                             "target": [lvs[j] for _, _, j in self._terms], "interaction": part("interaction"), "f2": part("f2"), "slope.low": part("slope_low"),
                             "slope.high": part("slope_high")}, index=self._term_labels,
                            columns=["predictor", "moderator", "target", "interaction", "f2", "slope.low", "slope.high"])

    def _stage1(self):
        nv = self._native
        fit = nv.fit(want_scores=False)
        direct_of = {(f, t): float(v) for f, t, v in zip(nv.eff_from.tolist(), nv.eff_to.tolist(), np.asarray(fit["direct"]).ravel())}
        return np.array([direct_of[p] for p in self._paths]), np.asarray(fit["r2"], dtype=np.float64).ravel()

    def path_coefficients(self) -> pd.DataFrame:
        """Per direct path "A -> B": the stage-1 coefficient (``main``) and the stage-2 coefficient (``moderated``)."""
        main, _ = self._stage1()
        return pd.DataFrame({"main": main, "moderated": self._original[self._slice("direct")[0]]}, index=self._path_labels, columns=["main", "moderated"])

    def r_squared(self) -> pd.DataFrame:
        _, main = self._stage1()
        return pd.DataFrame({"main": main, "moderated": self._original[self._slice("r2")[0]]}, index=self._lvs, columns=["main", "moderated"])

    def simple_slopes(self, at=(-1, 0, 1)) -> pd.DataFrame:
        """Per term: the slope of the predictor on the target where the moderator is ``at`` standard deviations from its mean, direct2 + at x interaction,
        from the full-sample record."""
        direct = self._original[self._slice("direct")[0]]
        inter = self._original[self._slice("interaction")[0]]
        main = np.array([direct[self._paths.index((a, j))] for a, _, j in self._terms])
        return pd.DataFrame({"at %g" % x: main + float(x) * inter for x in at}, index=self._term_labels, columns=["at %g" % x for x in at])

    def summary(self, what) -> pd.DataFrame:
        sl, index = self._slice(what)
        return pd.DataFrame(self._table[sl], index=index, columns=SUMMARY_COLUMNS)

    def intervals(self, what, method="percentile", level=0.95) -> pd.DataFrame:
        if method not in INTERVAL_METHODS:
            raise ValueError("method must be one of %s" % ", ".join(INTERVAL_METHODS))
        if method == "bca":
            raise NotImplementedError("no bca intervals for the moderation analysis: the jackknife writes no moderation records")
        if not 0.0 < float(level) < 1.0:
            raise ValueError("level must lie strictly between 0 and 1")
        sl, index = self._slice(what)
        key = (method, float(level))
        if key not in self._interval_cache:
            table, _ = self._native.moderation_intervals(self._iterations, self._original, method, float(level))
            self._interval_cache[key] = np.column_stack((self._original, table))
        return pd.DataFrame(self._interval_cache[key][sl], index=index, columns=INTERVAL_COLUMNS)

    def used(self) -> int:
        """Number of replicates that entered the summaries."""
        return self._used

    def seed(self):
        return self._seed

    def replicates(self):
        """The OK replicates' moderation records [n_used, W], fetched from HBM."""
        records, status = self._native.moderation_fetch(0, self._iterations)
        return records[status == 0]
