"""Confirmatory tetrad analysis (CTA-PLS) with bootstrap inference on the GPU (not in the reference): is a block reflective at all?

Under a one-factor reflective model every tetrad of four items of a block vanishes; CTA-PLS (Gudergan, Ringle, Wende & Will 2008, after Bollen & Ting)
bootstraps a non-redundant set of tetrads per block and rejects the reflective specification when a Bonferroni-adjusted bias-corrected interval
excludes zero.  Every replicate's tetrads are computed on the device from the replicate's indicator moment matrix, behind the solver of its batch
(include/plspm_hip.h ``plspm_tetrad_*``).  The definitions are THIS PROJECT'S, written down here and in csrc/tetrad_core.h; the numbers
are not claimed to equal those of SmartPLS or of any other program.  For one data set (the full sample or one replicate) of n rows:

    mu_p, c_pq     the mean of item p and the covariance c_pq = sum x_p x_q / n - mu_p mu_q (divisor n)
    s_p, r_pq      s_p = sqrt(c_pp), exactly 0 for a column that is constant in the data set; r_pq = c_pq / (s_p s_q).  On the device "constant" is a
                   threshold: c_pp <= 1e-9 of the column's second moment about the full sample's mean (the rounding residue of a constant column, the
                   rule of the solver and of the assessment).  The mirror centres exactly, so it sees c_pp = 0 for an exactly constant column and no
                   other; a column that varies by less than the threshold is constant to the device and not to the mirror
    x_pq           r_pq for matrix = "correlation" (the default: scale-free, the entries the assessment uses), c_pq for matrix = "covariance"
    tau(a,b,c,d)   x_ab x_cd - x_ac x_bd of four items of one block: two rounded products and one subtraction (no fused multiply-add)
    testable       a block of at least four items, numbered 1 .. k in device order (the order of the block's columns in the configuration)
    "basis"        k (k - 3) / 2 tetrads per block: for i = 4 .. k tau(1,3,i,2), tau(1,2,i,3); then for 4 <= i < j <= k, i-major, tau(1,2,i,j).  Its
                   Jacobian at a generic one-factor point has rank k (k - 3) / 2 and the other tetrads add nothing to it (tests/test_tetrad.py, k = 4 .. 10):
                   a non-redundant set of the model-implied vanishing tetrads
    "all"          2 C(k, 4) per block: per quadruple a < b < c < d in lexicographic order tau(a,b,c,d), tau(a,c,d,b); the third tetrad of the
                   quadruple is minus their sum
    record         the tetrads by block and then as above, then status and iterations
    status         the bootstrap record's if that failed (NaN everywhere); 3 (non-finite) when a tetrad is not finite (a column that is constant in the
                   resample, under "correlation") -- the values stand
    limit          at most 4,096 tetrads (counted before anything is enumerated)
    decision       per block of m tetrads the bias-corrected ("bc") interval of every tetrad at level 1 - alpha / m (Bonferroni); the reflective
                   specification is "rejected" when at least one interval excludes zero

``_tetrad_list`` and ``_tetrads`` below are the same statistic in NumPy: the checker of the kernel and of the host's lists.
Scope: metric data without missing cells and without higher-order constructs, one GPU; no bca intervals (the jackknife writes no tetrad records); no
tetrads across blocks; no redundancy sweep of Bollen & Ting for anything other than one-factor blocks.
"""
import os
from math import comb

import numpy as np
import pandas as pd

import plspm.config as c
import plspm.weights as pw
from plspm import _native
from plspm._compile import compile_model
from plspm.bootstrap import INTERVAL_COLUMNS, INTERVAL_METHODS, SUMMARY_COLUMNS, _intervals
from plspm.estimator import Estimator
from plspm.quality import MIN_ITERATIONS, _unsupported
from plspm.scheme import Scheme

MAX_TETRADS = 4096
SETS = ("basis", "all")
MATRICES = ("correlation", "covariance")
STATUS_OK, STATUS_NONFINITE = 0, 3


def _tetrad_count(k, tetrads="basis"):
    """Tetrads of a block of k items (0 below four).  A Python int: no overflow."""
    if tetrads not in SETS:
        raise ValueError("tetrads must be one of %s" % ", ".join(SETS))
    if k < 4:
        return 0
    return k * (k - 3) // 2 if tetrads == "basis" else 2 * comb(k, 4)


def _check_tetrad_count(sizes, tetrads="basis"):
    """The tetrads of the tested blocks of these sizes; ValueError beyond MAX_TETRADS -- from the count alone, nothing is enumerated."""
    n = sum(_tetrad_count(int(k), tetrads) for k in sizes)
    if n > MAX_TETRADS:
        raise ValueError("the tested blocks have %d tetrads, more than the %d a tetrad record holds" % (n, MAX_TETRADS))
    return n


def _tetrad_list(k, tetrads="basis"):
    """The ordered quadruples (a, b, c, d) of a block of k items, items numbered from 0 (the module docstring numbers them from 1)."""
    n = _tetrad_count(k, tetrads)
    if n > MAX_TETRADS:
        raise ValueError("a block of %d items has %d tetrads, more than the %d a tetrad record holds" % (k, n, MAX_TETRADS))
    out = []
    if k < 4:
        return out
    if tetrads == "basis":
        for i in range(3, k):
            out += [(0, 2, i, 1), (0, 1, i, 2)]
        for i in range(3, k):
            for j in range(i + 1, k):
                out.append((0, 1, i, j))
        return out
    for a in range(k):
        for b in range(a + 1, k):
            for cc in range(b + 1, k):
                for d in range(cc + 1, k):
                    out += [(a, b, cc, d), (a, cc, d, b)]
    return out


def _tetrad_values(x, quads):
    """tau of every quadruple [m, 4] (indices into x) on the symmetric matrix x: two products, one subtraction, in the dtype of x."""
    q = np.asarray(quads, dtype=np.int64).reshape(-1, 4)
    a, b, cc, d = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    first, second = x[a, b] * x[cc, d], x[a, cc] * x[b, d]
    return first - second


def _moments(X_rows, matrix="correlation", dtype=np.float64):
    """x [P, P] of the rows X_rows [n, P] (the module docstring's definitions) in ``dtype`` -- np.longdouble works."""
    if matrix not in MATRICES:
        raise ValueError("matrix must be one of %s" % ", ".join(MATRICES))
    X = np.asarray(X_rows, dtype=dtype)
    n = dtype(X.shape[0])
    Xc = X - X.sum(axis=0) / n
    m = Xc.sum(axis=0) / n
    cov = (Xc.T @ Xc) / n - np.outer(m, m)
    if matrix == "covariance":
        return cov
    var = np.diag(cov)
    sd = np.where(var > 0, np.sqrt(np.where(var > 0, var, 1)), 0).astype(dtype)          # (a constant column: every centred entry is exactly 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        isd = dtype(1) / sd
        return cov * np.outer(isd, isd)


def _tetrads(X_rows, blocks, tetrads="basis", matrix="correlation", dtype=np.float64):
    """The tetrad record of one data set: X_rows [n, P] its rows in device column order, blocks the tested blocks as arrays of column indices (a block of
    fewer than four columns is skipped, as the library skips it without a mask).  Returns a dict: tetrads [n_tet] in ``dtype``, status, list (per tetrad
    (position of the block in ``blocks``, a, b, c, d) with the items as column indices), per_block (the tetrad count of every block)."""
    sizes = [len(b) for b in blocks]
    _check_tetrad_count(sizes, tetrads)
    X_rows = np.asarray(X_rows)
    values, listed, per_block = [], [], []
    for l, block in enumerate(blocks):
        block = np.asarray(block, dtype=np.int64)
        quads = np.asarray(_tetrad_list(len(block), tetrads), dtype=np.int64).reshape(-1, 4)
        per_block.append(quads.shape[0])
        if not quads.shape[0]:
            continue
        x = _moments(X_rows[:, block], matrix, dtype)          # (the tetrads of a block read its own diagonal block only)
        with np.errstate(invalid="ignore", over="ignore"):
            values.append(_tetrad_values(x, quads))
        listed += [(l,) + tuple(int(v) for v in row) for row in block[quads]]
    tet = np.concatenate(values) if values else np.zeros(0, dtype=dtype)
    status = STATUS_OK if np.all(np.isfinite(tet)) else STATUS_NONFINITE
    return dict(tetrads=tet, status=status, list=listed, per_block=per_block)


def _excludes_zero(lower, upper):
    return (lower > 0.0) | (upper < 0.0)


def _decision_table(original, ok_records, block_of, alpha=0.05, interval=None):
    """Per tested block (ascending block id): (block id, tetrads m, level 1 - alpha / m, adjusted intervals that exclude zero), and the interval table
    [n_tet, 7] (level | lower, upper, z0, accel, level.lower, level.upper).  ``interval(level)`` returns the [n_tet, 6] table of one level; by default the
    NumPy restatement of the device's intervals on ok_records [n_used, n_tet]."""
    block_of = np.asarray(block_of)
    if interval is None:
        def interval(level):
            return _intervals(ok_records, original, None, "bc", level)
    ids = sorted(set(block_of.tolist()))
    count = {l: int(np.count_nonzero(block_of == l)) for l in ids}
    table = np.full((block_of.shape[0], 7), np.nan)
    cache = {}
    for l in ids:
        level = 1.0 - alpha / count[l]
        if level not in cache:
            cache[level] = interval(level)
        sel = block_of == l
        table[sel, 0] = level
        table[sel, 1:] = cache[level][sel]
    rows = [(l, count[l], 1.0 - alpha / count[l], int(np.count_nonzero(_excludes_zero(table[block_of == l, 1], table[block_of == l, 2])))) for l in ids]
    return rows, table


def _block_mask(cm, blocks):
    """uint8 [L] for the LV names ``blocks`` (None: every block of at least four items); ValueError for an unknown name or a block of fewer than four."""
    sizes = np.diff(cm.block_offset)
    if blocks is None:
        mask = (sizes >= 4).astype(np.uint8)
        if not mask.any():
            raise ValueError("no block has four items: there is nothing to test")
        return mask
    mask = np.zeros(cm.L, dtype=np.uint8)
    for name in blocks:
        if name not in cm.lvs:
            raise ValueError("unknown latent variable %r in blocks" % (name,))
        l = cm.lvs.index(name)
        if sizes[l] < 4:
            raise ValueError("block %s has %d items: a block is testable with at least four" % (name, sizes[l]))
        mask[l] = 1
    if not mask.any():
        raise ValueError("blocks names no block")
    return mask


def _options(cm, blocks, tetrads, matrix, alpha):
    if tetrads not in SETS:
        raise ValueError("tetrads must be one of %s" % ", ".join(SETS))
    if matrix not in MATRICES:
        raise ValueError("matrix must be one of %s" % ", ".join(MATRICES))
    if not 0.0 < float(alpha) < 1.0:
        raise ValueError("alpha must lie strictly between 0 and 1")
    mask = _block_mask(cm, blocks)
    _check_tetrad_count(np.diff(cm.block_offset)[mask != 0], tetrads)
    return mask


class TetradAnalysis:
    """``TetradAnalysis(data, config, scheme=Scheme.CENTROID, iterations=5000, seed=None, blocks=None, tetrads="basis", matrix="correlation", alpha=0.05,
    fit_iterations=100, tolerance=1e-6, device_id=0, processes=1)`` -- ``iterations`` bootstrap replicates; ``blocks``: the names of the tested LVs (None:
    every block of at least four items).  Also ``Plspm(..., bootstrap=True, tetrads=True).tetrads()``.

    ``tetrads()``: index "LV: a,b,c,d" x (block, a, b, c, d, tetrad) of the full sample; ``summary()``; ``intervals(method="bc", level=None)`` -- level None:
    the Bonferroni-adjusted level 1 - alpha / m of the tetrad's block, in a column ``level``; ``decision()``: per block its items, tetrads, level,
    nonvanishing (adjusted intervals that exclude zero) and reflective ("rejected" / "not rejected"); ``used()``; ``status()``; ``records()``; ``seed()``."""

    def __init__(self, data: pd.DataFrame, config: c.Config, scheme: Scheme = Scheme.CENTROID, iterations: int = 5000, seed: int = None, blocks=None,
                 tetrads: str = "basis", matrix: str = "correlation", alpha: float = 0.05, fit_iterations: int = 100, tolerance: float = 0.000001,
                 device_id: int = 0, processes: int = 1):
        assert tolerance > 0
        assert scheme in Scheme
        if processes > 1:
            raise NotImplementedError("the tetrad analysis runs on one GPU (processes = 1)")
        observations = config.filter(data)
        why = _unsupported(config, observations)
        if why is not None:
            raise NotImplementedError("the tetrad analysis covers metric data without missing cells and without higher-order constructs: this model has " + why)
        n = observations.shape[0]
        if n < 10:
            raise Exception("Bootstrapping could not be performed, at least 10 observations are required.")
        if iterations < 10:
            iterations = 100
        _options(compile_model(config, config.path(), observations.columns), blocks, tetrads, matrix, alpha)      # (the refusals that need no device come first)
        calculator = pw.WeightsCalculatorFactory(config, max(fit_iterations, MIN_ITERATIONS), tolerance, np.sqrt(n / (n - 1)), scheme, device_id)
        whole = Estimator(config).run(calculator, observations, want_scores=False)
        native = whole.native
        native.tetrad_enable(True, _options(whole.compiled, blocks, tetrads, matrix, alpha), tetrads, matrix)
        if seed is None:
            seed = int.from_bytes(os.urandom(8), "little")
        native.bootstrap_device(iterations, seed, 0)
        self._init(native, whole.compiled, iterations, alpha)
        self._seed = seed

    @classmethod
    def of_bootstrap(cls, native, compiled, iterations, alpha=0.05):
        """The analysis of a bootstrap that already ran on ``native`` with ``tetrad_enable`` on (``Plspm(bootstrap=True, tetrads=True)``)."""
        self = cls.__new__(cls)
        self._init(native, compiled, iterations, alpha)
        self._seed = None
        return self

    def _init(self, native, cm, iterations, alpha):
        self._native, self._cm, self._iterations, self._alpha = native, cm, iterations, float(alpha)
        try:
            block, a, b, cc, d = native.tetrad_list()
            self._original, self._status = native.tetrad_fit()
            self._table, self._used = native.tetrad_summary(iterations, self._original)
        except _native.NativeBackendError as err:
            raise NotImplementedError("no tetrad analysis on this handle: " + str(err))
        self._block = block
        self._items = np.stack((a, b, cc, d), axis=1)
        mvs, lvs = cm.dev_mvs, cm.lvs
        self._labels = ["%s: %s" % (lvs[l], ",".join(mvs[p] for p in row)) for l, row in zip(block.tolist(), self._items.tolist())]
        self._interval_cache = {}

    def status(self) -> int:
        """Status of the full-sample record (0: fine)."""
        return self._status

    def tetrads(self) -> pd.DataFrame:
        mvs, lvs = self._cm.dev_mvs, self._cm.lvs
        frame = {"block": [lvs[l] for l in self._block.tolist()]}
        for u, name in enumerate("abcd"):
            frame[name] = [mvs[p] for p in self._items[:, u].tolist()]
        frame["tetrad"] = self._original
        return pd.DataFrame(frame, index=self._labels, columns=["block", "a", "b", "c", "d", "tetrad"])

    def summary(self) -> pd.DataFrame:
        return pd.DataFrame(self._table, index=self._labels, columns=SUMMARY_COLUMNS)

    def _interval_table(self, method, level):
        key = (method, float(level))
        if key not in self._interval_cache:
            self._interval_cache[key], _ = self._native.tetrad_intervals(self._iterations, self._original, method, float(level))
        return self._interval_cache[key]

    def _adjusted(self, method="bc"):
        return _decision_table(self._original, None, self._block, self._alpha, lambda level: self._interval_table(method, level))

    def intervals(self, method="bc", level=None) -> pd.DataFrame:
        if method not in INTERVAL_METHODS:
            raise ValueError("method must be one of %s" % ", ".join(INTERVAL_METHODS))
        if method == "bca":
            raise NotImplementedError("no bca intervals for the tetrad analysis: the jackknife writes no tetrad records")
        if level is None:
            _, table = self._adjusted(method)
            frame = pd.DataFrame(np.column_stack((self._original, table[:, 1:])), index=self._labels, columns=INTERVAL_COLUMNS)
            frame["level"] = table[:, 0]
            return frame
        if not 0.0 < float(level) < 1.0:
            raise ValueError("level must lie strictly between 0 and 1")
        return pd.DataFrame(np.column_stack((self._original, self._interval_table(method, level))), index=self._labels, columns=INTERVAL_COLUMNS)

    def decision(self) -> pd.DataFrame:
        rows, _ = self._adjusted("bc")
        sizes = np.diff(self._cm.block_offset)
        out = [(int(sizes[l]), m, level, bad, "rejected" if bad > 0 else "not rejected") for l, m, level, bad in rows]
        return pd.DataFrame(out, index=[self._cm.lvs[l] for l, _, _, _ in rows], columns=["items", "tetrads", "level", "nonvanishing", "reflective"])

    def used(self) -> int:
        """Number of replicates that entered the summaries."""
        return self._used

    def seed(self):
        return self._seed

    def records(self):
        """The OK replicates' tetrad records [n_used, n_tet], fetched from HBM."""
        records, status = self._native.tetrad_fetch(0, self._iterations)
        return records[status == 0]
