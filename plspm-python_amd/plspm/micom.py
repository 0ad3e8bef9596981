"""MICOM -- the measurement invariance of composite models (Henseler, Ringle and Sarstedt 2016) by permutation, on the GPU: the check that comes before
any two-group comparison (``plspm.mga.GroupComparison``), whose differences mean nothing unless the composites measure the same thing in both groups.

Step 1, configural invariance (the same indicators, the same data treatment, the same algorithm settings in both groups), is the user's to establish: one
``Config`` for all rows is what this class takes.  Steps 2 and 3 are computed for the observed split and for ``permutations`` random re-splits of the rows
into groups of the observed sizes -- the splits of ``GroupComparison``, each half estimated on the full-data handle (include/plspm_hip.h
``plspm_permutation_device``), with one more kernel behind the solver that writes the MICOM record of every permutation (``plspm_micom_*``).

This project's definitions (SmartPLS's and cSEM's exact conventions are not claimed).  For one split into groups a and b, with each group's record weights
w_g and, from its own rows, the means mu_g, covariances C_g (divided by n_g) and standard deviations s_g = sqrt(diag C_g) (zero below the solver's 1e-9
threshold): v_g = w_g s_g.  From all rows, fixed for the run: the standard deviations s_0, the correlation matrix R_0, the weights w_0 of the fit on all
rows, v_0 = w_0 s_0 normalised per block so that v_0' R_0,ll v_0 = 1, and u = v_0 / s_0.  Per latent variable l:

    step 2   c_l       = v_a' R_0,ll v_b / sqrt((v_a' R_0,ll v_a) (v_b' R_0,ll v_b))
             the correlation, over all rows, of the two composites built from pooled-standardised indicators with each group's standardised weights
             (``Config(scaled=)``'s scalar and any per-group constant cancel; the weights are not sign-corrected, so c carries a genuine sign)
    step 3   dmean_l   = sum_{p in l} u_p (mu_a,p - mu_b,p)                                      mean of the pooled composite, a - b
             dlogvar_l = log(n_a / (n_a - 1) u' C_a,ll u) - log(n_b / (n_b - 1) u' C_b,ll u)     log ratio of its variances (ddof = 1)

A permutation counts when both its halves converged (``used``).  With alpha = 0.05 by default:

    c         quantile = the alpha quantile of the permutation distribution (the ``lower`` of the percentile interval at level 1 - 2 alpha);
              p = (1 + #{c_r <= c_obs}) / (1 + used);  compositional invariance holds when c_obs >= quantile
    dmean,    lower, upper = the percentile interval at level 1 - alpha;  p = (1 + #{|d_r| >= |d_obs|}) / (1 + used);
    dlogvar   the two are equal when lower <= d_obs <= upper

NaN never counts; p is NaN where the observed value is NaN.  Group a is the first of the two sorted labels.  Scope: metric data without missing cells and
without higher-order constructs, exactly two groups.
"""
import os

import numpy as np
import pandas as pd

import plspm.config as c
import plspm.weights as w
from plspm.estimator import Estimator
from plspm.mga import _labels, _observations
from plspm.scheme import Scheme


def _micom(X, member, w_a, w_b, w_0, blocks, dtype=np.float64) -> np.ndarray:
    """NumPy mirror of one MICOM record, c[L] | dmean[L] | dlogvar[L], computed from the data (no moment matrices) in ``dtype``: ``X`` [N, P] in device column
    order, ``member`` [N] bools (True = group a), the weights of the two groups' records and of the fit on all rows, ``blocks`` = the columns of every LV.
    Population standard deviations (ddof = 0), R_0 from all rows, ddof = 1 variances in step 3."""
    X = np.asarray(X, dtype=dtype)
    member = np.asarray(member, dtype=bool)
    w_a, w_b, w_0 = (np.asarray(v, dtype=dtype) for v in (w_a, w_b, w_0))
    Xa, Xb = X[member], X[~member]
    s_0, s_a, s_b = X.std(axis=0), Xa.std(axis=0), Xb.std(axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        Z = (X - X.mean(axis=0)) / s_0
        L = len(blocks)
        out = np.empty(3 * L, dtype=dtype)
        for l, cols in enumerate(blocks):
            cols = np.asarray(cols, dtype=np.int64)
            Zl = Z[:, cols]
            ya, yb = Zl @ (w_a[cols] * s_a[cols]), Zl @ (w_b[cols] * s_b[cols])
            out[l] = (ya * yb).mean() / np.sqrt((ya * ya).mean() * (yb * yb).mean())
            y0 = Zl @ (w_0[cols] * s_0[cols])
            y0 = y0 / np.sqrt((y0 * y0).mean())
            out[L + l] = y0[member].mean() - y0[~member].mean()
            out[2 * L + l] = np.log(y0[member].var(ddof=1)) - np.log(y0[~member].var(ddof=1))
    return out


def _p_values(observed, below, exceed, used, L) -> np.ndarray:
    """p of every record column: one-sided (lower tail) for c, two-sided for dmean and dlogvar; NaN where the observed value is NaN."""
    count = np.concatenate((below[:L], exceed[L:])).astype(np.float64)
    p = (1.0 + count) / (1.0 + used)
    p[np.isnan(observed)] = np.nan
    return p


class Micom:
    """``Micom(data, config, group, scheme=Scheme.PATH, iterations=100, tolerance=1e-6, permutations=1000, seed=None, device_id=0, alpha=0.05)``

    ``group``: a column label of ``data`` or a ``pd.Series`` aligned on ``data.index``, with exactly two distinct labels and at least 10 rows each
    (``ValueError`` otherwise, before anything runs on the device).  Configural invariance (step 1) is the user's to establish; ``compositional()`` is step 2,
    ``means()`` and ``variances()`` are step 3, ``summary()`` puts them together per latent variable: "partial" when step 2 holds, "full" when steps 2 and 3
    all hold, "none" otherwise.
    """

    def __init__(self, data: pd.DataFrame, config: c.Config, group, scheme: Scheme = Scheme.PATH, iterations: int = 100, tolerance: float = 0.000001,
                 permutations: int = 1000, seed: int = None, device_id: int = 0, alpha: float = 0.05):
        assert tolerance > 0
        assert scheme in Scheme
        iterations = max(iterations, 100)                   # as Plspm: "default and minimum 100"
        if int(permutations) < 1:
            raise ValueError("permutations must be at least 1")
        if not 0.0 < float(alpha) < 0.5:
            raise ValueError("alpha must lie strictly between 0 and 0.5")
        labels = _labels(data, group)
        observations = _observations(data, config, "MICOM")
        a, b = sorted(labels.unique())
        in_a = (labels.loc[observations.index] == a).values
        self._labels = (a, b)
        self._permutations = B = int(permutations)
        self._alpha = float(alpha)
        self._seed = int.from_bytes(os.urandom(8), "little") if seed is None else int(seed)
        n = observations.shape[0]
        calculator = w.WeightsCalculatorFactory(config, iterations, tolerance, np.sqrt(n / (n - 1)), scheme, device_id)
        whole = Estimator(config).run(calculator, observations, want_scores=False)
        native = self._native = whole.native
        lvs, L = list(whole.compiled.lvs), whole.compiled.L
        n1 = int(in_a.sum())
        native.micom_enable(True)
        # the observed split: the same kernel's record of a one-permutation call with explicit memberships
        native.permutation(1, n1, member=in_a[None, :])
        observed, observed_status = native.micom_fetch(0, 1)
        observed = observed[0]
        # the permutations on the full-data handle: its rows are already in HBM
        native.permutation(B, n1, self._seed)
        below, exceed, used = native.micom_counts(B, observed)
        one_sided, _ = native.micom_intervals(B, observed, "percentile", round(1.0 - 2.0 * self._alpha, 12))
        two_sided, _ = native.micom_intervals(B, observed, "percentile", round(1.0 - self._alpha, 12))
        p = _p_values(observed, below, exceed, used, L)
        self._used = used
        # device record layout: c[L] | dmean[L] | dlogvar[L]
        self.raw = {"observed": observed, "observed_status": int(observed_status[0]), "below": below, "exceed": exceed, "n_used": used, "p_value": p,
                    "quantile": one_sided[:L, 0], "lower": two_sided[:, 0], "upper": two_sided[:, 1], "n_a": n1, "n_b": n - n1}
        self._frames = _frames(lvs, observed, p, one_sided[:L, 0], two_sided[:, 0], two_sided[:, 1])

    def compositional(self) -> pd.DataFrame:
        """Step 2 per latent variable: ``c``, the alpha ``quantile`` of its permutation distribution, ``p.value``, ``invariant`` (c >= quantile)."""
        return self._frames["compositional"]

    def means(self) -> pd.DataFrame:
        """Step 3, means of the pooled composite: ``diff`` (a - b), ``lower`` / ``upper`` of the permutation distribution, ``p.value``, ``equal``."""
        return self._frames["means"]

    def variances(self) -> pd.DataFrame:
        """Step 3, log ratio of the pooled composite's variances: ``diff``, ``lower``, ``upper``, ``p.value``, ``equal``."""
        return self._frames["variances"]

    def summary(self) -> pd.DataFrame:
        """One row per latent variable: ``compositional``, ``equal.means``, ``equal.variances`` and ``invariance`` ("none", "partial": step 2 holds, "full":
        steps 2 and 3 all hold).  Configural invariance is assumed."""
        return self._frames["summary"]

    def used(self) -> int:
        """Permutations whose two estimates both converged (the others are dropped)."""
        return self._used

    def seed(self) -> int:
        return self._seed

    def groups(self):
        """The two labels (a, b): a is the first in sorted order; differences are a - b."""
        return self._labels

    def records(self):
        """The MICOM records of the permutations, fetched from HBM: (records [permutations, 3 L] as c | dmean | dlogvar, status [permutations])."""
        return self._native.micom_fetch(0, self._permutations)


def _frames(lvs, observed, p, quantile, lower, upper) -> dict:
    """The frames of ``Micom`` from the observed record, the p-values and the quantiles of the permutation distribution."""
    L = len(lvs)
    with np.errstate(invalid="ignore"):
        invariant = observed[:L] >= quantile
        inside = (lower <= observed) & (observed <= upper)
    compositional = pd.DataFrame({"c": observed[:L], "quantile": quantile, "p.value": p[:L], "invariant": invariant}, index=lvs,
                                 columns=["c", "quantile", "p.value", "invariant"])
    step3 = {}
    for name, sl in (("means", slice(L, 2 * L)), ("variances", slice(2 * L, 3 * L))):
        step3[name] = pd.DataFrame({"diff": observed[sl], "lower": lower[sl], "upper": upper[sl], "p.value": p[sl], "equal": inside[sl]}, index=lvs,
                                   columns=["diff", "lower", "upper", "p.value", "equal"])
    eq_m, eq_v = step3["means"]["equal"].values, step3["variances"]["equal"].values
    level = np.where(invariant & eq_m & eq_v, "full", np.where(invariant, "partial", "none"))
    summary = pd.DataFrame({"compositional": invariant, "equal.means": eq_m, "equal.variances": eq_v, "invariance": level}, index=lvs,
                           columns=["compositional", "equal.means", "equal.variances", "invariance"])
    return {"compositional": compositional, "means": step3["means"], "variances": step3["variances"], "summary": summary}
