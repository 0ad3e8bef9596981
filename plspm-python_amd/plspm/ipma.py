"""Importance-performance map analysis (IPMA) with bootstrap inference on the GPU (not in the reference): for a target construct, which antecedent
constructs and indicators matter most, and how well do they perform today on a 0-100 scale?

The importance of a construct is its UNSTANDARDISED total effect on the target, on the 0-100 scale of the rescaled indicators; its performance is the
mean of its rescaled score.  Neither can be read off a fit's standardised outputs, and for inference both are recomputed per bootstrap replicate from that
replicate's own column means, standard deviations and block correlations: on the device, from the replicate's indicator moment matrix, behind the solver
of its batch (include/plspm_hip.h ``plspm_ipma_*``).  The definitions are THIS PROJECT'S, after Ringle & Sarstedt (2016), written down here
and in csrc/ipma_core.h; the numbers are not claimed to equal those of SmartPLS or of any other program.  For one data set (the full sample or one
replicate) of n rows, with fixed bounds lo_p < hi_p per indicator (range_p = hi_p - lo_p; the same for every replicate) and the data set's record
weights w | r2 | total | direct | loadings lambda:

    m_p, s_p, r_pq   the mean, the population standard deviation (divisor n) and the correlations of the columns; s_p is exactly 0 for a column that is
                     constant in the data set (on the device by the threshold of the solver and of the assessment)
    v_p              w_p s_p, normalised per block so that v_b' R_bb v_b = 1;   u_p = sum_{q in block(p)} r_pq v_q
    sigma_l          sign(sum_{p in l} u_p lambda_p), +1 for 0: ``plspm.quality``'s v and sign rule
    y_l              sigma_l sum_p v_p (x_p - m_p) / s_p, the standardised score
    x~_p             100 (x_p - lo_p) / range_p, the rescaled indicator
    a_p, A_l         a_p = sigma_l v_p range_p / (100 s_p), the coefficient of x~_p in y_l;   A_l = sum_{p in l} a_p
    weight_r_p       a_p / A_l: the rescaled weights, 1 in sum per block (1 for a single item)
    mvperf_p         100 (m_p - lo_p) / range_p: the indicator's performance
    perf_l           sum_{p in l} weight_r_p mvperf_p: the construct's performance, the mean of Y_l = sum weight_r_p x~_p
    sd_l             1 / A_l: Y_l - perf_l = y_l / A_l and y_l has population variance 1
    total_u, direct_u   per effect pair e = (i -> j): total[e] A_i / A_j and direct[e] A_i / A_j -- the rescaling is a diagonal similarity of the path
                     matrix, so it carries through to the total effects
    mvimp[t][p]      weight_r_p total_u(l -> t) for the indicator p of LV l != t: the indicator's importance for target t; 0 where the model has no effect
                     l -> t and for the target's own block
    record           perf [L] | sd [L] | total_u [n_eff] | direct_u [n_eff] | weight_r [P] | mvperf [P] | mvimp [n_t x P], then status and iterations;
                     MVs in device order (the order of the blocks' columns in the configuration), targets in ascending LV order
    status           the bootstrap record's if that failed (NaN everywhere); 3 (non-finite) when a value is not finite (a column that is constant in the
                     resample); otherwise 4 (inadmissible) when some weight_r_p < 0 -- an importance-performance map needs non-negative rescaled weights,
                     or a performance can leave [0, 100].  The values stand under both; such a replicate is counted and not used, as in PLSc.

``_ipma`` below is the same statistic in NumPy: the checker of the kernel.  It centres exactly, so it sees s_p = 0 for an exactly constant column and
no other.  Scope: metric data without missing cells and without higher-order constructs, one GPU; no bca intervals (the jackknife writes no IPMA
records); no PLSc-corrected importances; no re-coding of indicators to repair negative weights.
"""
import os

import numpy as np
import pandas as pd

import plspm.config as c
import plspm.weights as pw
from plspm import _native
from plspm._compile import compile_model
from plspm.bootstrap import INTERVAL_COLUMNS, INTERVAL_METHODS, SUMMARY_COLUMNS
from plspm.estimator import Estimator
from plspm.quality import MIN_ITERATIONS, _unsupported
from plspm.scheme import Scheme

STATUS_OK, STATUS_NONFINITE, STATUS_INADMISSIBLE = 0, 3, 4
FIELDS = ("perf", "sd", "total_u", "direct_u", "weight_r", "mvperf", "mvimp")
WHAT = ("performance", "sd", "total", "direct", "weights", "indicator_performance", "importance")


def _layout(P, L, n_eff, n_t):
    """{field: slice} of the record, and its width."""
    sizes = (L, L, n_eff, n_eff, P, P, n_t * P)
    out, at = {}, 0
    for name, size in zip(FIELDS, sizes):
        out[name] = slice(at, at + size)
        at += size
    return out, at


def _default_targets(effect_pairs):
    return sorted({int(t) for _, t in effect_pairs})


def _ipma(Xr, blocks, record, effect_pairs, lo, hi, targets=None, dtype=np.float64):
    """The IPMA record of one data set: Xr [n, P] its rows in device column order, blocks the column indices of every LV, record that data set's bootstrap
    record (weights [P] | r2 [L] | total [n_eff] | direct [n_eff] | loadings [P]), effect_pairs the (from, to) pairs of the record's effect rows, lo / hi [P]
    the bounds, targets the target LV indices (None: every LV with a predecessor).  Returns a dict in ``dtype`` -- np.longdouble works: the seven fields
    (``FIELDS``; mvimp as [n_t, P]), record (the device's layout), status, A [L], sigma [L], targets and min_abs_weight (the smallest |weight_r_p|)."""
    dt = np.dtype(dtype).type
    X = np.asarray(Xr, dtype=dtype)
    n, P, L = dt(X.shape[0]), X.shape[1], len(blocks)
    blocks = [np.asarray(b, dtype=np.int64) for b in blocks]
    pairs = [(int(f), int(t)) for f, t in effect_pairs]
    ne = len(pairs)
    rec = np.asarray(record, dtype=dtype)
    w, total, direct, lam = rec[:P], rec[P + L:P + L + ne], rec[P + L + ne:P + L + 2 * ne], rec[P + L + 2 * ne:P + L + 2 * ne + P]
    lo, hi = np.asarray(lo, dtype=dtype), np.asarray(hi, dtype=dtype)
    span = hi - lo
    targets = _default_targets(pairs) if targets is None else [int(t) for t in targets]
    hundred, one = dt(100), dt(1)
    shift = X.sum(axis=0) / n
    Xc = X - shift
    mu = Xc.sum(axis=0) / n
    lvof = np.zeros(P, dtype=np.int64)
    a, A, sigma = np.zeros(P, dtype=dtype), np.zeros(L, dtype=dtype), np.ones(L, dtype=dtype)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        mvperf = hundred * ((shift + mu) - lo) / span
        for l, blk in enumerate(blocks):
            lvof[blk] = l
            cov = (Xc[:, blk].T @ Xc[:, blk]) / n - np.outer(mu[blk], mu[blk])
            var = np.diag(cov)
            sd = np.where(var > 0, np.sqrt(np.where(var > 0, var, 1)), 0).astype(dtype)          # (a constant column: every centred entry is exactly 0)
            isd = one / sd
            R = cov * np.outer(isd, isd)
            np.fill_diagonal(R, one)
            v = w[blk] * sd
            t = R @ v
            f = one / np.sqrt(v @ t)
            sigma[l] = -one if (t * lam[blk]).sum() < 0 else one
            a[blk] = ((sigma[l] * (v * f)) * (span[blk] * isd)) / hundred
            A[l] = a[blk].sum()
        weight_r = a / A[lvof]
        perf = np.array([(weight_r[blk] * mvperf[blk]).sum() for blk in blocks], dtype=dtype)
        sd_l = one / A
        total_u = np.array([total[e] * A[i] / A[j] for e, (i, j) in enumerate(pairs)], dtype=dtype).reshape(ne)
        direct_u = np.array([direct[e] * A[i] / A[j] for e, (i, j) in enumerate(pairs)], dtype=dtype).reshape(ne)
        eff_of = {pair: e for e, pair in enumerate(pairs)}
        mvimp = np.zeros((len(targets), P), dtype=dtype)
        for k, target in enumerate(targets):
            for l, blk in enumerate(blocks):
                if (l, target) in eff_of:
                    mvimp[k, blk] = weight_r[blk] * total_u[eff_of[(l, target)]]
    out = dict(perf=perf, sd=sd_l, total_u=total_u, direct_u=direct_u, weight_r=weight_r, mvperf=mvperf, mvimp=mvimp)
    out["record"] = np.concatenate([out[name].ravel() for name in FIELDS])
    finite = bool(np.all(np.isfinite(out["record"])))
    out["status"] = STATUS_NONFINITE if not finite else STATUS_INADMISSIBLE if bool(np.any(weight_r < 0)) else STATUS_OK
    out["A"], out["sigma"], out["targets"] = A, sigma, targets
    out["min_abs_weight"] = float(np.min(np.abs(weight_r))) if np.all(np.isfinite(weight_r)) else float("nan")
    return out


def _bounds(values, names, scale):
    """(lo [P], hi [P]) of the columns ``values`` [n, P] named ``names``.  scale None: every column's observed minimum and maximum; (lo, hi): the same bounds
    for all columns; {name: (lo, hi)}: the columns it does not name use their observed bounds.  ValueError for a constant column, an unknown name, bounds
    that are not finite, lo >= hi, and data outside its bounds."""
    values = np.asarray(values, dtype=np.float64)
    names = list(names)
    low, high = values.min(axis=0), values.max(axis=0)
    constant = [name for name, x, y in zip(names, low, high) if not x < y]
    if constant:
        raise ValueError("constant column(s) %s: an indicator without variation has no place in the map" % ", ".join(map(str, constant)))
    lo, hi = low.copy(), high.copy()
    if isinstance(scale, dict):
        unknown = [name for name in scale if name not in names]
        if unknown:
            raise ValueError("scale names unknown indicator(s) %s" % ", ".join(map(str, unknown)))
        for name, pair in scale.items():
            try:
                x, y = pair
                lo[names.index(name)], hi[names.index(name)] = float(x), float(y)
            except (TypeError, ValueError):
                raise ValueError("the scale of %s must be a pair (lo, hi): got %r" % (name, pair))
    elif scale is not None:
        try:
            x, y = scale
            lo[:], hi[:] = float(x), float(y)
        except (TypeError, ValueError):
            raise ValueError("scale must be None, a pair (lo, hi) or a dict {indicator: (lo, hi)}")
    for name, x, y, x0, y0 in zip(names, lo, hi, low, high):
        if not (np.isfinite(x) and np.isfinite(y) and x < y):
            raise ValueError("the bounds of %s must be finite with lo < hi: got (%r, %r)" % (name, x, y))
        if x0 < x or y0 > y:
            raise ValueError("%s has data outside its bounds: observed [%r, %r], bounds [%r, %r]" % (name, x0, y0, x, y))
    return lo, hi


def _target_mask(cm, targets):
    """uint8 [L] for the LV names ``targets`` (None: None -- every LV with a predecessor); ValueError for an unknown name, an LV without predecessors, none."""
    path = np.asarray(cm.path)
    if not (path.sum(axis=1) > 0).any():
        raise ValueError("no latent variable has a predecessor: there is no target")
    if targets is None:
        return None
    if isinstance(targets, str):
        targets = [targets]
    mask = np.zeros(cm.L, dtype=np.uint8)
    for name in targets:
        if name not in cm.lvs:
            raise ValueError("unknown latent variable %r in targets" % (name,))
        l = cm.lvs.index(name)
        if not path[l].sum() > 0:
            raise ValueError("target %s has no predecessor: nothing has an effect on it" % name)
        mask[l] = 1
    if not mask.any():
        raise ValueError("targets names no latent variable")
    return mask


def _options(cm, observations, targets=None, scale=None):
    """(mask, lo, hi) for ``native.ipma_enable``: the refusals that need no device.  observations: the filtered frame."""
    mask = _target_mask(cm, targets)
    values = observations.values[:, cm.col_index].astype(np.float64)
    lo, hi = _bounds(values, cm.dev_mvs, scale)
    return mask, lo, hi


class Ipma:
    """``Ipma(data, config, scheme=Scheme.CENTROID, targets=None, scale=None, iterations=5000, seed=None, fit_iterations=100, tolerance=1e-6, device_id=0,
    processes=1)`` -- ``targets``: the names of the target LVs (None: every LV with a predecessor); ``scale``: None (every column's observed minimum and
    maximum), ``(lo, hi)`` for all columns, or ``{mv: (lo, hi)}`` (the others: observed); ``iterations`` bootstrap replicates.  Also
    ``Plspm(..., bootstrap=True, ipma=True | dict(targets=..., scale=...)).ipma()``.

    ``constructs(target)``: the LVs with an effect on the target x (importance, performance); ``indicators(target)``: their MVs x (block, importance,
    performance); ``performance()``: LVs x (performance, sd); ``weights()``: MVs x (block, weight, performance) with the rescaled weights;
    ``total_effects()`` / ``path_coefficients()``: the unstandardised ones, "A -> B" rows; ``scores()``: the rescaled scores Y_l;
    ``summary(what, target=None)`` / ``intervals(what, method="bc", level=0.95, target=None)`` for what in ``WHAT`` ("importance" takes the target);
    ``used()``, ``inadmissible()``, ``status()``, ``records()``, ``seed()``."""

    def __init__(self, data: pd.DataFrame, config: c.Config, scheme: Scheme = Scheme.CENTROID, targets=None, scale=None, iterations: int = 5000,
                 seed: int = None, fit_iterations: int = 100, tolerance: float = 0.000001, device_id: int = 0, processes: int = 1):
        assert tolerance > 0
        assert scheme in Scheme
        if processes > 1:
            raise NotImplementedError("the importance-performance map runs on one GPU (processes = 1)")
        observations = config.filter(data)
        why = _unsupported(config, observations)
        if why is not None:
            raise NotImplementedError("the importance-performance map covers metric data without missing cells and without higher-order constructs: this model has " + why)
        n = observations.shape[0]
        if n < 10:
            raise Exception("Bootstrapping could not be performed, at least 10 observations are required.")
        if iterations < 10:
            iterations = 100
        _options(compile_model(config, config.path(), observations.columns), observations, targets, scale)      # (the refusals that need no device come first)
        calculator = pw.WeightsCalculatorFactory(config, max(fit_iterations, MIN_ITERATIONS), tolerance, np.sqrt(n / (n - 1)), scheme, device_id)
        whole = Estimator(config).run(calculator, observations, want_scores=True)
        native = whole.native
        mask, lo, hi = _options(whole.compiled, observations, targets, scale)
        native.ipma_enable(True, mask, lo, hi)
        if seed is None:
            seed = int.from_bytes(os.urandom(8), "little")
        native.bootstrap_device(iterations, seed, 0)
        self._init(native, whole.compiled, iterations, lo, hi, whole.scores)
        self._seed = seed

    @classmethod
    def of_bootstrap(cls, native, compiled, iterations, lo, hi, scores):
        """The analysis of a bootstrap that already ran on ``native`` with ``ipma_enable`` on (``Plspm(bootstrap=True, ipma=True)``); scores: a callable
        that returns the fit's LV scores [N x L] as a frame."""
        self = cls.__new__(cls)
        self._init(native, compiled, iterations, lo, hi, scores)
        self._seed = None
        return self

    def _init(self, native, cm, iterations, lo, hi, scores):
        self._native, self._cm, self._iterations, self._fit_scores = native, cm, iterations, scores
        self._lo, self._hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
        try:
            self._targets = [int(t) for t in native.ipma_targets()]
            self._original, self._status = native.ipma_fit()
        except _native.NativeBackendError as err:
            raise NotImplementedError("no importance-performance map on this handle: " + str(err))
        lvs, mvs = list(cm.lvs), list(cm.dev_mvs)
        self._pairs = list(zip(native.eff_from.tolist(), native.eff_to.tolist()))
        self._at, width = _layout(cm.P, cm.L, len(self._pairs), len(self._targets))
        assert width == native.ipma_width
        self._lvof = np.repeat(np.arange(cm.L), np.diff(cm.block_offset))
        if self._status == STATUS_INADMISSIBLE:
            weight = self._original[self._at["weight_r"]]
            bad = ["%s (%s)" % (lvs[l], ", ".join(mvs[p] for p in np.flatnonzero((self._lvof == l) & (weight < 0)))) for l in range(cm.L)
                   if np.any(weight[self._lvof == l] < 0)]
            raise ValueError("the full sample is inadmissible for an importance-performance map: negative rescaled weights in " + "; ".join(bad))
        if self._status != STATUS_OK:
            raise ValueError("the full sample has no importance-performance map: status %d of its record" % self._status)
        try:
            self._table, self._used = native.ipma_summary(iterations, self._original)
        except _native.NativeBackendError as err:
            raise NotImplementedError("no importance-performance map on this handle: " + str(err))
        self._pair_labels = ["%s -> %s" % (lvs[f], lvs[t]) for f, t in self._pairs]
        self._interval_cache = {}

    # ---- the record's parts
    def _target(self, target):
        lvs = self._cm.lvs
        if target is None:
            if len(self._targets) != 1:
                raise ValueError("name the target: this map has the targets %s" % ", ".join(lvs[t] for t in self._targets))
            return 0
        if target not in lvs or lvs.index(target) not in self._targets:
            raise ValueError("%r is not a target of this map (targets: %s)" % (target, ", ".join(lvs[t] for t in self._targets)))
        return self._targets.index(lvs.index(target))

    def _slice(self, what, target=None):
        if what not in WHAT:
            raise ValueError("what must be one of %s" % ", ".join(WHAT))
        cm = self._cm
        if what == "importance":
            k, P = self._target(target), cm.P
            start = self._at["mvimp"].start + k * P
            return slice(start, start + P), list(cm.dev_mvs)
        field = FIELDS[WHAT.index(what)]
        index = list(cm.lvs) if what in ("performance", "sd") else self._pair_labels if what in ("total", "direct") else list(cm.dev_mvs)
        return self._at[field], index

    def _part(self, what, target=None):
        return self._original[self._slice(what, target)[0]]

    def _antecedents(self, target):
        t = self._targets[self._target(target)]
        return t, [(e, f) for e, (f, to) in enumerate(self._pairs) if to == t]

    def status(self) -> int:
        """Status of the full-sample record (0: fine)."""
        return self._status

    def constructs(self, target=None) -> pd.DataFrame:
        _, ante = self._antecedents(target)
        total, perf = self._part("total"), self._part("performance")
        return pd.DataFrame({"importance": [total[e] for e, _ in ante], "performance": [perf[f] for _, f in ante]},
                            index=[self._cm.lvs[f] for _, f in ante], columns=["importance", "performance"])

    def indicators(self, target=None) -> pd.DataFrame:
        _, ante = self._antecedents(target)
        keep = np.flatnonzero(np.isin(self._lvof, [f for _, f in ante]))
        imp, perf = self._part("importance", target), self._part("indicator_performance")
        return pd.DataFrame({"block": [self._cm.lvs[self._lvof[p]] for p in keep], "importance": imp[keep], "performance": perf[keep]},
                            index=[self._cm.dev_mvs[p] for p in keep], columns=["block", "importance", "performance"])

    def performance(self) -> pd.DataFrame:
        return pd.DataFrame({"performance": self._part("performance"), "sd": self._part("sd")}, index=list(self._cm.lvs), columns=["performance", "sd"])

    def weights(self) -> pd.DataFrame:
        return pd.DataFrame({"block": [self._cm.lvs[l] for l in self._lvof], "weight": self._part("weights"), "performance": self._part("indicator_performance")},
                            index=list(self._cm.dev_mvs), columns=["block", "weight", "performance"])

    def total_effects(self) -> pd.DataFrame:
        """The unstandardised total effects, one row per effect pair "A -> B"."""
        return pd.DataFrame({"from": [self._cm.lvs[f] for f, _ in self._pairs], "to": [self._cm.lvs[t] for _, t in self._pairs], "total": self._part("total")},
                            index=self._pair_labels, columns=["from", "to", "total"])

    def path_coefficients(self) -> pd.DataFrame:
        """The unstandardised path coefficients, one row per direct path "A -> B"."""
        path = np.asarray(self._cm.path)
        keep = [e for e, (f, t) in enumerate(self._pairs) if path[t, f]]
        direct = self._part("direct")
        return pd.DataFrame({"from": [self._cm.lvs[self._pairs[e][0]] for e in keep], "to": [self._cm.lvs[self._pairs[e][1]] for e in keep], "direct": direct[keep]},
                            index=[self._pair_labels[e] for e in keep], columns=["from", "to", "direct"])

    def scores(self) -> pd.DataFrame:
        """The rescaled scores Y_l = perf_l + (score_l - mean) / (sd_pop(score_l) A_l): an affine map of the scores the fit already fetched."""
        scores = self._fit_scores()
        values = scores.values.astype(np.float64)
        centred = values - values.mean(axis=0)
        sd = np.sqrt((centred * centred).mean(axis=0))
        return pd.DataFrame(self._part("performance") + centred / sd * self._part("sd"), index=scores.index, columns=scores.columns)

    def summary(self, what, target=None) -> pd.DataFrame:
        sl, index = self._slice(what, target)
        return pd.DataFrame(self._table[sl], index=index, columns=SUMMARY_COLUMNS)

    def intervals(self, what, method="bc", level=0.95, target=None) -> pd.DataFrame:
        if method not in INTERVAL_METHODS:
            raise ValueError("method must be one of %s" % ", ".join(INTERVAL_METHODS))
        if method == "bca":
            raise NotImplementedError("no bca intervals for the importance-performance map: the jackknife writes no IPMA records")
        if not 0.0 < float(level) < 1.0:
            raise ValueError("level must lie strictly between 0 and 1")
        sl, index = self._slice(what, target)
        key = (method, float(level))
        if key not in self._interval_cache:
            table, _ = self._native.ipma_intervals(self._iterations, self._original, method, float(level))
            self._interval_cache[key] = np.column_stack((self._original, table))
        return pd.DataFrame(self._interval_cache[key][sl], index=index, columns=INTERVAL_COLUMNS)

    def used(self) -> int:
        """Number of replicates that entered the summaries."""
        return self._used

    def inadmissible(self) -> int:
        """Number of replicates with a negative rescaled weight: counted, not used."""
        _, status = self._native.ipma_fetch(0, self._iterations)
        return int(np.count_nonzero(status == STATUS_INADMISSIBLE))

    def seed(self):
        return self._seed

    def records(self):
        """The OK replicates' IPMA records [n_used, W], fetched from HBM."""
        records, status = self._native.ipma_fetch(0, self._iterations)
        return records[status == 0]
