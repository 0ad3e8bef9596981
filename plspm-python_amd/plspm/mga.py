"""Two-group comparison (multi-group analysis) by permutation or by bootstrap -- what R's ``plspm.groups(..., method = "permutation" | "bootstrap")`` offers, on the GPU.

Is a path coefficient, weight, loading, R^2 or total effect different between two groups of respondents?  ``GroupComparison`` fits the model
on all rows (``global``) and on each group (``group.<a>``, ``group.<b>``: ordinary fits, equal to ``Plspm`` on the subsets), then re-splits
the rows at random ``permutations`` times into groups of the observed sizes and estimates both halves of every split on the full-data handle
(include/plspm_hip.h ``plspm_permutation_device``: 2 x permutations problems through the bootstrap's int8 Gram and solver, at least seven digit
planes).  The statistic of a result column j is the difference d_j = est_a(j) - est_b(j); the device counts the valid permutations (both
halves converged) with |d_rj| >= |d_obs,j| on the records in HBM (``plspm_permutation_counts``), and

    p_j = (1 + #{valid r : |d_rj| >= |d_obs,j|}) / (1 + n_used)          (never zero; NaN where d_obs,j is NaN)

is this project's p-value.  Group a is the first of the two sorted labels.  Scope: metric data without missing cells and without
higher-order constructs (``NotImplementedError`` otherwise).

``method="bootstrap"`` -- R's default method of ``plspm.groups`` -- bootstraps each group on its own instead: ``resamples`` times, n_a draws
from group a's rows and n_b draws from group b's (include/plspm_hip.h ``plspm_stratified_bootstrap_device``: 2 x resamples problems through
the same int8 Gram and solver, at least seven digit planes).  d = est_a - est_b of the ordinary group fits; se_a, se_b, and the bootstrap
means m_a, m_b are the device summaries of each group's records.  Three tests on the same records, this project's definitions (the exact
one- / two-sided conventions of R's and SmartPLS's implementations are not claimed):

    "parametric" (Keil et al. 2000):  s_p = sqrt((n_a-1)^2/(n_a+n_b-2) se_a^2 + (n_b-1)^2/(n_a+n_b-2) se_b^2),
                                      t = |d| / (s_p sqrt(1/n_a + 1/n_b)),  df = n_a + n_b - 2
    "welch":                          v = (n_a-1)/n_a se_a^2 + (n_b-1)/n_b se_b^2,  t = |d| / sqrt(v),
                                      df = v^2 / ((n_a-1)/n_a^2 se_a^4 + (n_b-1)/n_b^2 se_b^4) - 2
        both: p = 2 t.sf(t, df) (two-sided)
    "henseler" (PLS-MGA):             p_one = 1 - #{(i, k) : 2 m_a - x_a,i > 2 m_b - x_b,k} / (used_a used_b)  (H1: theta_a > theta_b;
                                      the counts over all pairs of valid records, on the device: ``plspm_stratified_pair_counts``)
                                      p = 2 min(p_one, 1 - p_one)

p is NaN where d, a standard error or a mean is NaN; a 0 / 0 t statistic gives NaN.
"""
import os

import numpy as np
import pandas as pd
from scipy import stats

import plspm.config as c
import plspm.inner_model as im
import plspm.weights as w
from plspm.estimator import Estimator
from plspm.scheme import Scheme

MIN_GROUP_ROWS = 10
METHODS = ("permutation", "bootstrap")
TESTS = ("parametric", "welch", "henseler")


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


def _observations(data: pd.DataFrame, config: c.Config, what: str) -> pd.DataFrame:
    """The model's columns of ``data`` once the scope of the two-group procedures holds: metric scales, no higher-order constructs, no missing cells."""
    if not config.metric():
        raise NotImplementedError(what + " covers metric data only (no Scale.NUM / RAW / ORD / NOM)")
    if config.hoc():
        raise NotImplementedError(what + " does not cover higher-order constructs")
    observations = config.filter(data)
    if config.nan_columns(observations).any():
        raise NotImplementedError(what + " needs complete data (no missing cells in the model's columns)")
    return observations


def bootstrap_tests(diff, se_a, se_b, mean_a, mean_b, n_a, n_b, above, used_a, used_b) -> dict:
    """The three tests of ``method="bootstrap"`` per result column (see the module docstring): {"parametric": (t, df, p), "welch": (t, df, p),
    "henseler": p}.  ``above``: Henseler's pair counts; ``used_a`` / ``used_b``: the valid records of each group."""
    diff, se_a, se_b, mean_a, mean_b = (np.asarray(v, dtype=np.float64) for v in (diff, se_a, se_b, mean_a, mean_b))
    na, nb = float(n_a), float(n_b)
    nan = np.isnan(diff) | np.isnan(se_a) | np.isnan(se_b) | np.isnan(mean_a) | np.isnan(mean_b)
    out = {}
    with np.errstate(divide="ignore", invalid="ignore"):
        sp = np.sqrt((na - 1) ** 2 / (na + nb - 2) * se_a ** 2 + (nb - 1) ** 2 / (na + nb - 2) * se_b ** 2)
        t = np.abs(diff) / (sp * np.sqrt(1.0 / na + 1.0 / nb))
        df = np.full(diff.shape, na + nb - 2)
        out["parametric"] = (t, df)
        v = (na - 1) / na * se_a ** 2 + (nb - 1) / nb * se_b ** 2
        t = np.abs(diff) / np.sqrt(v)
        df = v ** 2 / ((na - 1) / na ** 2 * se_a ** 4 + (nb - 1) / nb ** 2 * se_b ** 4) - 2
        out["welch"] = (t, df)
        for k, (t, df) in list(out.items()):
            p = 2.0 * stats.t.sf(t, df)
            p[nan | np.isnan(t) | np.isnan(df)] = np.nan
            out[k] = (t, df, p)
        pairs = float(used_a) * float(used_b)
        p_one = 1.0 - np.asarray(above, dtype=np.float64) / pairs if pairs > 0 else np.full(diff.shape, np.nan)
        p = 2.0 * np.minimum(p_one, 1.0 - p_one)
        p[nan] = np.nan
        out["henseler"] = p
    return out


def _record(result) -> np.ndarray:
    """A fit's estimates in the device record layout: weights | r2 | total | direct | loadings (device column order)."""
    raw = result.raw
    return np.concatenate((raw["weights"], raw["r2"], raw["total"], raw["direct"], raw["loadings"])).astype(np.float64)


class GroupComparison:
    """``GroupComparison(data, config, group, scheme=Scheme.PATH, iterations=100, tolerance=1e-6, permutations=1000, seed=None, device_id=0,
    method="permutation", resamples=1000, test="parametric")``

    ``group``: a column label of ``data`` or a ``pd.Series`` aligned on ``data.index``, with exactly two distinct labels and at least 10 rows
    each (``ValueError`` otherwise, before anything runs on the device).  Frames (``paths()``, ``weights()``, ``loading()``, ``r_squared()``,
    ``total_effects()``) carry the columns ``global``, ``group.<a>``, ``group.<b>``, ``diff.abs``, ``p.value``, ``sig.05`` and the index of the
    corresponding ``Bootstrap`` frame (``paths()``: the structural paths of the model).

    ``method="bootstrap"``: ``resamples`` bootstrap resamples of each group and the test ``test`` ("parametric", "welch" or "henseler"); the
    t-tests' frames carry ``t.stat`` and ``deg.fr`` after ``diff.abs``.  Every frame accessor takes ``test=`` to read another of the three
    tests of the same run (``ValueError`` with ``method="permutation"``).
    """

    def __init__(self, data: pd.DataFrame, config: c.Config, group, scheme: Scheme = Scheme.PATH, iterations: int = 100, tolerance: float = 0.000001,
                 permutations: int = 1000, seed: int = None, device_id: int = 0, method: str = "permutation", resamples: int = 1000,
                 test: str = "parametric"):
        assert tolerance > 0
        assert scheme in Scheme
        iterations = max(iterations, 100)                   # as Plspm: "default and minimum 100"
        if method not in METHODS:
            raise ValueError("method must be one of %s" % ", ".join(METHODS))
        if test not in TESTS:
            raise ValueError("test must be one of %s" % ", ".join(TESTS))
        if method == "permutation" and int(permutations) < 1:
            raise ValueError("permutations must be at least 1")
        if method == "bootstrap" and int(resamples) < 1:
            raise ValueError("resamples must be at least 1")
        labels = _labels(data, group)
        observations = _observations(data, config, "the %s test" % method)
        a, b = sorted(labels.unique())
        in_a = (labels.loc[observations.index] == a).values
        self._labels = (a, b)
        self._method, self._test = method, test
        self._permutations = int(permutations)
        self._resamples = int(resamples)
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
        self._native = native
        if method == "bootstrap":
            self._run_bootstrap(whole, config.path(), observed, fits, diff, in_a)
            return
        # the permutations on the full-data handle: its rows are already in HBM
        native.permutation(self._permutations, int(in_a.sum()), self._seed)
        exceed, used = native.permutation_counts(self._permutations, diff)
        with np.errstate(invalid="ignore"):
            p = (1.0 + exceed) / (1.0 + used)
        p[np.isnan(diff)] = np.nan
        self._used = used
        # device record layout (weights | r2 | total | direct | loadings, device column order)
        self.raw = {"global": observed, "group_a": fits[0], "group_b": fits[1], "observed_diff": diff, "exceed": exceed, "n_used": used, "p_value": p}
        self._frames = self._build_frames(whole, config.path(), observed, fits, diff, p)

    def _run_bootstrap(self, whole, path, observed, fits, diff, in_a):
        """Both groups' resamples on the full-data handle, the per-group device summaries, Henseler's pair counts and the three tests."""
        native, B = whole.native, self._resamples
        d_out, _, _ = native.stratified_bootstrap(B, in_a, self._seed)
        RS = native.row_stride
        summ_a, _ = native.summary(B, fits[0], d_rows=d_out, stride=2 * RS)
        summ_b, _ = native.summary(B, fits[1], d_rows=d_out + RS * 8, stride=2 * RS)
        mean_a, se_a, mean_b, se_b = summ_a[:, 1], summ_a[:, 2], summ_b[:, 1], summ_b[:, 2]
        above, used_a, used_b = native.stratified_pair_counts(B, mean_a, mean_b)
        n_a = int(in_a.sum())
        tests = bootstrap_tests(diff, se_a, se_b, mean_a, mean_b, n_a, in_a.size - n_a, above, used_a, used_b)
        self._used = (used_a, used_b)
        self.raw = {"global": observed, "group_a": fits[0], "group_b": fits[1], "observed_diff": diff, "n_a": n_a, "n_b": in_a.size - n_a,
                    "se_a": se_a, "se_b": se_b, "mean_a": mean_a, "mean_b": mean_b, "above": above, "used_a": used_a, "used_b": used_b,
                    "t_parametric": tests["parametric"][0], "df_parametric": tests["parametric"][1], "p_parametric": tests["parametric"][2],
                    "t_welch": tests["welch"][0], "df_welch": tests["welch"][1], "p_welch": tests["welch"][2], "p_henseler": tests["henseler"]}
        self._frames_by_test = {}
        for name in TESTS:
            if name == "henseler":
                self._frames_by_test[name] = self._build_frames(whole, path, observed, fits, diff, tests[name])
            else:
                t, df, p = tests[name]
                self._frames_by_test[name] = self._build_frames(whole, path, observed, fits, diff, p, t, df)
        self._frames = self._frames_by_test[self._test]

    def _build_frames(self, whole, path, observed, fits, diff, p, t=None, df=None):
        cm, native = whole.compiled, whole.native
        P, L, ne = cm.P, cm.L, native.n_eff
        inner = im.InnerModel.from_device(path, whole)
        eff_index = list(inner.effects().index)
        inv = cm.inv_index[cm.inv_index >= 0]
        cols = cm.used_data_cols()
        a, b = self._labels
        columns = ["global", "group.%s" % a, "group.%s" % b, "diff.abs"] + (["t.stat", "deg.fr"] if t is not None else []) + ["p.value", "sig.05"]

        def frame(sl, index, order=None):
            parts = [observed[sl], fits[0][sl], fits[1][sl], np.abs(diff[sl])] + ([t[sl], df[sl]] if t is not None else []) + [p[sl]]
            if order is not None:
                parts = [v[order] for v in parts]
            with np.errstate(invalid="ignore"):
                sig = np.where(parts[-1] < 0.05, "yes", "no")
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

    def _frame(self, name, test):
        if test is None:
            return self._frames[name]
        if self._method != "bootstrap":
            raise ValueError("test= selects one of the bootstrap tests: it needs method=\"bootstrap\"")
        if test not in TESTS:
            raise ValueError("test must be one of %s" % ", ".join(TESTS))
        return self._frames_by_test[test][name]

    def paths(self, test: str = None) -> pd.DataFrame:
        """Path coefficients of the structural paths (index "from -> to")."""
        return self._frame("paths", test)

    def weights(self, test: str = None) -> pd.DataFrame:
        return self._frame("weights", test)

    def loading(self, test: str = None) -> pd.DataFrame:
        return self._frame("loading", test)

    def r_squared(self, test: str = None) -> pd.DataFrame:
        """R squared of the endogenous latent variables."""
        return self._frame("r_squared", test)

    def total_effects(self, test: str = None) -> pd.DataFrame:
        return self._frame("total_effects", test)

    def used(self):
        """Permutations whose two estimates both converged (the others are dropped, as failed bootstrap replicates are); with
        method="bootstrap" the pair (used_a, used_b) of valid resamples of each group."""
        return self._used

    def seed(self) -> int:
        return self._seed

    def groups(self):
        """The two labels (a, b): a is the first in sorted order; differences are a - b."""
        return self._labels

    def permutation_records(self):
        """The 2 x permutations records, fetched from HBM: (rows [2B, R] in the device layout, status [2B], iterations [2B]); record 2r is
        group a of permutation r, 2r + 1 its group b."""
        if self._method != "permutation":
            raise ValueError("permutation_records needs method=\"permutation\"")
        return self._native.fetch(0, 2 * self._permutations)

    def bootstrap_records(self):
        """The 2 x resamples records of method="bootstrap", fetched from HBM: (rows [2B, R], status [2B], iterations [2B]); record 2r is
        group a's resample r, 2r + 1 group b's."""
        if self._method != "bootstrap":
            raise ValueError("bootstrap_records needs method=\"bootstrap\"")
        return self._native.fetch(0, 2 * self._resamples)
