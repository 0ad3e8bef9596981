"""Two-group comparison (multi-group analysis) by permutation -- what R's ``plspm.groups(..., method = "permutation")`` offers, on the GPU.

Is a path coefficient, weight, loading, R^2 or total effect different between two groups of respondents?  ``GroupComparison`` fits the model
on all rows (``global``) and on each group (``group.<a>``, ``group.<b>``: ordinary fits, equal to ``Plspm`` on the subsets), then re-splits
the rows at random ``permutations`` times into groups of the observed sizes and estimates both halves of every split on the full-data handle
(include/plspm_hip.h ``plspm_permutation_device``: 2 x permutations problems through the bootstrap's int8 Gram and solver, at least seven digit
planes).  The statistic of a result column j is the difference d_j = est_a(j) - est_b(j); the device counts the valid permutations (both
halves converged) with |d_rj| >= |d_obs,j| on the records in HBM (``plspm_permutation_counts``), and

    p_j = (1 + #{valid r : |d_rj| >= |d_obs,j|}) / (1 + n_used)          (never zero; NaN where d_obs,j is NaN)

is this project's p-value.  Group a is the first of the two sorted labels.  Scope: metric data without missing cells and without
higher-order constructs (``NotImplementedError`` otherwise).
"""
import os

import numpy as np
import pandas as pd

import plspm.config as c
import plspm.inner_model as im
import plspm.weights as w
from plspm.estimator import Estimator
from plspm.scheme import Scheme

MIN_GROUP_ROWS = 10


def _labels(data: pd.DataFrame, group) -> pd.Series:
    """The group label of every row of ``data``: a column of ``data`` or a Series on the same index."""
    if isinstance(group, pd.Series):
        if not group.index.equals(data.index):
            raise ValueError("group: a pd.Series must be aligned on data.index (same labels in the same order)")
        labels = group
    else:
        try:
            present = group in data.columns
        except TypeError:
            present = False
        if not present:
            raise ValueError("group must be a column label of data or a pd.Series aligned on data.index")
        labels = data[group]
    if labels.isnull().any():
        raise ValueError("group: %d row(s) have no label (NaN / None)" % int(labels.isnull().sum()))
    levels = sorted(labels.unique())
    if len(levels) != 2:
        raise ValueError("group must have exactly two distinct labels, found %d" % len(levels))
    counts = labels.value_counts()
    small = [lv for lv in levels if counts[lv] < MIN_GROUP_ROWS]
    if small:
        raise ValueError("every group needs at least %d rows: %s" % (MIN_GROUP_ROWS, ", ".join("%s has %d" % (lv, counts[lv]) for lv in small)))
    return labels


def _record(result) -> np.ndarray:
    """A fit's estimates in the device record layout: weights | r2 | total | direct | loadings (device column order)."""
    raw = result.raw
    return np.concatenate((raw["weights"], raw["r2"], raw["total"], raw["direct"], raw["loadings"])).astype(np.float64)


class GroupComparison:
    """``GroupComparison(data, config, group, scheme=Scheme.PATH, iterations=100, tolerance=1e-6, permutations=1000, seed=None, device_id=0)``

    ``group``: a column label of ``data`` or a ``pd.Series`` aligned on ``data.index``, with exactly two distinct labels and at least 10 rows
    each (``ValueError`` otherwise, before anything runs on the device).  Frames (``paths()``, ``weights()``, ``loading()``, ``r_squared()``,
    ``total_effects()``) carry the columns ``global``, ``group.<a>``, ``group.<b>``, ``diff.abs``, ``p.value``, ``sig.05`` and the index of the
    corresponding ``Bootstrap`` frame (``paths()``: the structural paths of the model).
    """

    def __init__(self, data: pd.DataFrame, config: c.Config, group, scheme: Scheme = Scheme.PATH, iterations: int = 100, tolerance: float = 0.000001,
                 permutations: int = 1000, seed: int = None, device_id: int = 0):
        assert tolerance > 0
        assert scheme in Scheme
        iterations = max(iterations, 100)                   # as Plspm: "default and minimum 100"
        if int(permutations) < 1:
            raise ValueError("permutations must be at least 1")
        labels = _labels(data, group)
        if not config.metric():
            raise NotImplementedError("the permutation test covers metric data only (no Scale.NUM / RAW / ORD / NOM)")
        if config.hoc():
            raise NotImplementedError("the permutation test does not cover higher-order constructs")
        observations = config.filter(data)
        if config.nan_columns(observations).any():
            raise NotImplementedError("the permutation test needs complete data (no missing cells in the model's columns)")
        a, b = sorted(labels.unique())
        in_a = (labels.loc[observations.index] == a).values
        self._labels = (a, b)
        self._permutations = int(permutations)
        self._seed = int.from_bytes(os.urandom(8), "little") if seed is None else int(seed)

        def fit(rows):
            n = rows.shape[0]
            calculator = w.WeightsCalculatorFactory(config, iterations, tolerance, np.sqrt(n / (n - 1)), scheme, device_id)
            return Estimator(config).run(calculator, rows, want_scores=False)

        whole = fit(observations)
        fits = []
        for part in (observations[in_a], observations[~in_a]):
            result = fit(part)
            fits.append(_record(result))
            result.native.close()
        observed = _record(whole)
        diff = fits[0] - fits[1]
        native = whole.native
        # the permutations on the full-data handle: its rows are already in HBM
        native.permutation(self._permutations, int(in_a.sum()), self._seed)
        exceed, used = native.permutation_counts(self._permutations, diff)
        with np.errstate(invalid="ignore"):
            p = (1.0 + exceed) / (1.0 + used)
        p[np.isnan(diff)] = np.nan
        self._native, self._used = native, used
        # device record layout (weights | r2 | total | direct | loadings, device column order)
        self.raw = {"global": observed, "group_a": fits[0], "group_b": fits[1], "observed_diff": diff, "exceed": exceed, "n_used": used, "p_value": p}
        self._frames = self._build_frames(whole, config.path(), observed, fits, diff, p)

    def _build_frames(self, whole, path, observed, fits, diff, p):
        cm, native = whole.compiled, whole.native
        P, L, ne = cm.P, cm.L, native.n_eff
        inner = im.InnerModel.from_device(path, whole)
        eff_index = list(inner.effects().index)
        inv = cm.inv_index[cm.inv_index >= 0]
        cols = cm.used_data_cols()
        a, b = self._labels
        columns = ["global", "group.%s" % a, "group.%s" % b, "diff.abs", "p.value", "sig.05"]

        def frame(sl, index, order=None):
            parts = [observed[sl], fits[0][sl], fits[1][sl], np.abs(diff[sl]), p[sl]]
            if order is not None:
                parts = [v[order] for v in parts]
            with np.errstate(invalid="ignore"):
                sig = np.where(parts[4] < 0.05, "yes", "no")
            return pd.DataFrame(dict(zip(columns, parts + [sig])), index=index, columns=columns)
        paths = frame(slice(P + L + ne, P + L + 2 * ne), eff_index)
        structural = [path.loc[lv_to, lv_from] == 1 for lv_from, lv_to in zip(inner.effects()["from"], inner.effects()["to"])]
        return {
            "weights": frame(slice(0, P), cols, inv),                                                   # data-column order (as Bootstrap)
            "r_squared": frame(slice(P, P + L), cm.lvs).loc[inner.endogenous(), :],
            "total_effects": frame(slice(P + L, P + L + ne), eff_index),
            "paths": paths[np.asarray(structural, dtype=bool)],
            "loading": frame(slice(P + L + 2 * ne, P + L + 2 * ne + P), cols, inv),
        }

    def paths(self) -> pd.DataFrame:
        """Path coefficients of the structural paths (index "from -> to")."""
        return self._frames["paths"]

    def weights(self) -> pd.DataFrame:
        return self._frames["weights"]

    def loading(self) -> pd.DataFrame:
        return self._frames["loading"]

    def r_squared(self) -> pd.DataFrame:
        """R squared of the endogenous latent variables."""
        return self._frames["r_squared"]

    def total_effects(self) -> pd.DataFrame:
        return self._frames["total_effects"]

    def used(self) -> int:
        """Permutations whose two estimates both converged (the others are dropped, as failed bootstrap replicates are)."""
        return self._used

    def seed(self) -> int:
        return self._seed

    def groups(self):
        """The two labels (a, b): a is the first in sorted order; differences are a - b."""
        return self._labels

    def permutation_records(self):
        """The 2 x permutations records, fetched from HBM: (rows [2B, R] in the device layout, status [2B], iterations [2B]); record 2r is
        group a of permutation r, 2r + 1 its group b."""
        return self._native.fetch(0, 2 * self._permutations)
