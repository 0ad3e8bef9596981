"""Structural-model assessment with bootstrap inference on the GPU (not in the reference): the f2 effect size and the inner VIF of every
path, and the specific indirect effects for mediation analysis.

Every replicate's record is computed on the device, behind the assessment kernel whose construct correlations it reads (include/plspm_hip.h
``plspm_structural_*``) -- the construct correlations of a replicate are in no bootstrap record.  This project's definitions, for
one data set (the full sample or one replicate):

    rc [L x L]     its construct correlation matrix: the assessment record's signed lv_cor (``plspm.quality``), diagonal 1
    pred(j)        the predecessors of LV j in the path matrix
    R2(j | S)      the R squared of regressing j on the LVs in S, on rc, by the project's own regression: the normal equations rc_SS beta = rc_Sj,
                   solved if the Cholesky pivots pass PLSPM_PIVOT_RTOL, otherwise by the pseudo-inverse of the eigenvalues above PLSPM_EIG_RTOL
                   lambda_max; R2 = beta' rc_Sj; exactly 0 for an empty S
    per direct path i -> j (C[j, i] = 1), in the order of the effect pairs (from-major) restricted to direct paths, with S = pred(j) without i
      f2           (R2(j | pred(j)) - R2(j | S)) / (1 - R2(j | pred(j)))
      vif          1 / (1 - R2(i | S))                      (exactly 1 for an empty S)
    per specific indirect effect: a directed chain i -> m_1 -> ... -> j with at least one mediator
      specific     the product of the record's own ``direct`` entries along the chain, multiplied left to right -- the bootstrap record's path
                   coefficients, not re-estimated ones
      order        by effect pair (the pair order), then lexicographically by node sequence
    record         f2[n_dir] | vif[n_dir] | specific[n_spec], then status and iterations
    status         the bootstrap record's if that failed (NaN everywhere); 2 (singular) when a regression reports failure, 3 (non-finite) when an f2 or
                   vif is not finite (an R2 of 1) -- the values stand
    limit          at most 4,096 chains (counted before they are enumerated)

``_structural`` below is the same statistic in NumPy, with a chain enumerator of its own: the checker of the kernel and of the host's enumeration.
Scope: metric data without missing cells and without higher-order constructs, one GPU; no bca intervals (the jackknife writes no structural
records); f2 on the composites' correlations, not on PLSc-corrected ones.
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

MAX_CHAINS = 4096
WHAT = ("f2", "vif", "specific")


def _chain_count(C):
    """The number of specific indirect effects of the path matrix C (C[i, j] = 1 iff LV j -> LV i, strictly lower triangular), by dynamic programming
    over the DAG: nothing is enumerated.  A Python int: no overflow."""
    C = np.asarray(C) != 0
    L = C.shape[0]
    total = 0
    for f in range(L):
        paths = [0] * L                             # directed paths f -> ... -> t
        for t in range(f + 1, L):
            paths[t] = sum(1 if k == f else paths[k] for k in np.flatnonzero(C[t]).tolist())
            total += paths[t] - int(C[t, f])
    return total


def _check_chain_count(C):
    n = _chain_count(C)
    if n > MAX_CHAINS:
        raise ValueError("the path model has %d specific indirect effects, more than the %d a structural record holds" % (n, MAX_CHAINS))
    return n


def _chains(C):
    """Every chain of at least three LVs, as tuples of LV indices: by effect pair (from-major), then lexicographically.  ValueError beyond MAX_CHAINS."""
    _check_chain_count(C)
    C = np.asarray(C) != 0
    L = C.shape[0]
    succ = [np.flatnonzero(C[:, i]).tolist() for i in range(L)]
    found = {}

    def extend(walk):
        for s in succ[walk[-1]]:
            nxt = walk + (s,)
            if len(nxt) >= 3:
                found.setdefault((nxt[0], s), []).append(nxt)
            extend(nxt)
    for f in range(L):
        extend((f,))
    return [chain for pair in _effect_pairs(C) for chain in sorted(found.get(pair, []))]


def _r2(rc, S, col):
    """(R2(col | S), ok, solved) on rc by the device's regression rule."""
    if len(S) == 0:
        return rc.dtype.type(0), True, True
    x, ok, solved = _regress(rc[np.ix_(S, S)], rc[S, col])
    return x @ rc[S, col], ok, solved


def _structural(rc, C, direct):
    """The structural record of one data set: rc [L, L] its construct correlation matrix, C [L, L] the path matrix (C[i, j] = 1 iff LV j -> LV i),
    direct the path coefficients -- [L, L] (direct[t, f]) or the record's [n_eff] in effect-pair order.  Returns a dict in the dtype of rc --
    np.longdouble works: status, f2 [n_dir], vif [n_dir], specific [n_spec], record, paths (the (from, to) of every direct path), chains (tuples of LV
    indices), r2 [L] and pivots_pass (every regression was solved, none went to the pseudo-inverse)."""
    rc = np.asarray(rc)
    dt = rc.dtype.type
    C = np.asarray(C)
    L = C.shape[0]
    pairs = _effect_pairs(C)
    direct = np.asarray(direct, dtype=rc.dtype)
    if direct.ndim == 1:
        B = np.zeros((L, L), dtype=rc.dtype)
        for (f, t), value in zip(pairs, direct):
            B[t, f] = value
    else:
        B = direct
    chains = _chains(C)
    paths = [(f, t) for f, t in pairs if C[t, f]]
    status, pivots_pass = STATUS_OK, True
    r2 = np.zeros(L, dtype=rc.dtype)
    for j in range(L):
        r2[j], ok, solved = _r2(rc, np.flatnonzero(C[j]), j)
        pivots_pass = pivots_pass and solved
        if not ok:
            status = STATUS_SINGULAR
    f2, vif = np.empty(len(paths), dtype=rc.dtype), np.empty(len(paths), dtype=rc.dtype)
    one = dt(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        for d, (i, j) in enumerate(paths):
            S = np.array([k for k in np.flatnonzero(C[j]) if k != i], dtype=np.int64)
            r2_j, ok_j, solved_j = _r2(rc, S, j)
            r2_i, ok_i, solved_i = _r2(rc, S, i)
            pivots_pass = pivots_pass and solved_j and solved_i
            if not (ok_j and ok_i):
                status = STATUS_SINGULAR
            f2[d] = (r2[j] - r2_j) / (one - r2[j])
            vif[d] = one / (one - r2_i)
    specific = np.empty(len(chains), dtype=rc.dtype)
    for s, chain in enumerate(chains):
        value = B[chain[1], chain[0]]
        for a, b in zip(chain[1:-1], chain[2:]):
            value = value * B[b, a]
        specific[s] = value
    if status == STATUS_OK and not (np.all(np.isfinite(f2)) and np.all(np.isfinite(vif))):
        status = STATUS_NONFINITE
    return dict(status=status, f2=f2, vif=vif, specific=specific, record=np.concatenate((f2, vif, specific)), paths=paths, chains=chains, r2=r2,
                pivots_pass=pivots_pass)


class Structural:
    """``Structural(data, config, scheme=Scheme.CENTROID, iterations=5000, seed=None, fit_iterations=100, tolerance=1e-6, device_id=0, processes=1)``
    -- ``iterations`` bootstrap replicates.  Also ``Plspm(..., bootstrap=True, structural=True).structural()``.

    ``effect_sizes()``: paths "A -> B" x (f2, vif) of the full sample; ``specific_effects()``: chains "A -> M -> B" x (from, to, through, effect);
    ``mediation()``: per effect pair that has chains its direct, indirect and total effect and the share of each chain; ``summary(what)`` /
    ``intervals(what, method, level)`` for what in ("f2", "vif", "specific"): the bootstrap's summary / interval columns; ``used()``; ``seed()``;
    ``replicates()``."""

    def __init__(self, data: pd.DataFrame, config: c.Config, scheme: Scheme = Scheme.CENTROID, iterations: int = 5000, seed: int = None,
                 fit_iterations: int = 100, tolerance: float = 0.000001, device_id: int = 0, processes: int = 1):
        assert tolerance > 0
        assert scheme in Scheme
        if processes > 1:
            raise NotImplementedError("the structural assessment runs on one GPU (processes = 1)")
        observations = config.filter(data)
        why = _unsupported(config, observations)
        if why is not None:
            raise NotImplementedError("the structural assessment covers metric data without missing cells and without higher-order constructs: this model has " + why)
        _check_chain_count(config.path().values)
        n = observations.shape[0]
        if n < 10:
            raise Exception("Bootstrapping could not be performed, at least 10 observations are required.")
        if iterations < 10:
            iterations = 100
        calculator = pw.WeightsCalculatorFactory(config, max(fit_iterations, MIN_ITERATIONS), tolerance, np.sqrt(n / (n - 1)), scheme, device_id)
        whole = Estimator(config).run(calculator, observations, want_scores=False)
        native = whole.native
        native.structural_enable(True)
        if seed is None:
            seed = int.from_bytes(os.urandom(8), "little")
        native.bootstrap_device(iterations, seed, 0)
        self._init(native, whole.compiled, iterations)
        self._seed = seed

    @classmethod
    def of_bootstrap(cls, native, compiled, iterations):
        """The assessment of a bootstrap that already ran on ``native`` with ``structural_enable`` on (``Plspm(bootstrap=True, structural=True)``)."""
        self = cls.__new__(cls)
        self._init(native, compiled, iterations)
        self._seed = None
        return self

    def _init(self, native, cm, iterations):
        self._native, self._cm, self._iterations = native, cm, iterations
        lvs = self._lvs = list(cm.lvs)
        try:
            dir_from, dir_to, chain_off, chain_nodes = native.structural_paths()
            self._original, self._status = native.structural_fit()
            self._table, self._used = native.structural_summary(iterations, self._original)
        except _native.NativeBackendError as err:
            raise NotImplementedError("no structural assessment on this handle: " + str(err))
        self._paths = list(zip(dir_from.tolist(), dir_to.tolist()))
        self._chains = [tuple(chain_nodes[chain_off[s]:chain_off[s + 1]].tolist()) for s in range(len(chain_off) - 1)]
        self._path_labels = ["%s -> %s" % (lvs[f], lvs[t]) for f, t in self._paths]
        self._chain_labels = [" -> ".join(lvs[l] for l in chain) for chain in self._chains]
        self._interval_cache = {}

    def _slice(self, what):
        if what not in WHAT:
            raise ValueError("what must be one of %s" % ", ".join(WHAT))
        n_dir, n_spec = len(self._paths), len(self._chains)
        if what == "f2":
            return slice(0, n_dir), self._path_labels
        if what == "vif":
            return slice(n_dir, 2 * n_dir), self._path_labels
        return slice(2 * n_dir, 2 * n_dir + n_spec), self._chain_labels

    def status(self) -> int:
        """Status of the full-sample record (0: fine)."""
        return self._status

    def effect_sizes(self) -> pd.DataFrame:
        n_dir = len(self._paths)
        return pd.DataFrame({"f2": self._original[:n_dir], "vif": self._original[n_dir:2 * n_dir]}, index=self._path_labels, columns=["f2", "vif"])

    def specific_effects(self) -> pd.DataFrame:
        lvs = self._lvs
        return pd.DataFrame({"from": [lvs[ch[0]] for ch in self._chains], "to": [lvs[ch[-1]] for ch in self._chains],
                             "through": [" -> ".join(lvs[l] for l in ch[1:-1]) for ch in self._chains], "effect": self._original[2 * len(self._paths):]},
                            index=self._chain_labels, columns=["from", "to", "through", "effect"])

    def mediation(self) -> pd.DataFrame:
        """Per effect pair that has chains: the full sample's direct effect, indirect effect (the sum of the pair's chains) and total effect, and per
        chain its share of the indirect effect -- one row per chain, index "A -> M -> B"; the pair's three figures repeat on its rows."""
        spec = self._original[2 * len(self._paths):]
        lvs, nv = self._lvs, self._native
        fit = nv.fit(want_scores=False)
        direct_of = {(f, t): float(v) for f, t, v in zip(nv.eff_from.tolist(), nv.eff_to.tolist(), np.asarray(fit["direct"]).ravel())}
        indirect_of = {}
        for chain, value in zip(self._chains, spec):
            indirect_of[(chain[0], chain[-1])] = indirect_of.get((chain[0], chain[-1]), 0.0) + float(value)
        rows = []
        with np.errstate(divide="ignore", invalid="ignore"):
            for chain, value in zip(self._chains, spec):
                pair = (chain[0], chain[-1])
                direct, indirect = direct_of[pair], indirect_of[pair]
                rows.append((lvs[pair[0]], lvs[pair[1]], direct, indirect, direct + indirect, float(value), float(np.float64(value) / np.float64(indirect))))
        return pd.DataFrame(rows, index=self._chain_labels, columns=["from", "to", "direct", "indirect", "total", "effect", "share"])

    def summary(self, what) -> pd.DataFrame:
        sl, index = self._slice(what)
        return pd.DataFrame(self._table[sl], index=index, columns=SUMMARY_COLUMNS)

    def intervals(self, what, method="percentile", level=0.95) -> pd.DataFrame:
        if method not in INTERVAL_METHODS:
            raise ValueError("method must be one of %s" % ", ".join(INTERVAL_METHODS))
        if method == "bca":
            raise NotImplementedError("no bca intervals for the structural assessment: the jackknife writes no structural records")
        if not 0.0 < float(level) < 1.0:
            raise ValueError("level must lie strictly between 0 and 1")
        sl, index = self._slice(what)
        key = (method, float(level))
        if key not in self._interval_cache:
            table, _ = self._native.structural_intervals(self._iterations, self._original, method, float(level))
            self._interval_cache[key] = np.column_stack((self._original, table))
        return pd.DataFrame(self._interval_cache[key][sl], index=index, columns=INTERVAL_COLUMNS)

    def used(self) -> int:
        """Number of replicates that entered the summaries."""
        return self._used

    def seed(self):
        return self._seed

    def replicates(self):
        """The OK replicates' structural records [n_used, S] (f2 | vif | specific), fetched from HBM."""
        records, status = self._native.structural_fetch(0, self._iterations)
        return records[status == 0]
