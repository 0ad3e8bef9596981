"""Out-of-sample prediction by repeated k-fold cross-validation -- PLSpredict (Shmueli et al. 2016, 2019; SEMinR's ``predict_pls``), on the GPU.

How well does the model predict the indicators of rows it was not fitted on?  ``PLSpredict`` cuts the rows into ``folds`` folds, ``repetitions``
times over, estimates the model on the rows outside each fold (include/plspm_hip.h ``plspm_cv_device``: folds x repetitions problems through the
bootstrap's int8 Gram and solver, at least seven digit planes) and predicts the held-out rows of every fold from that fit, on the device
(``plspm_cv_predict``).  The targets are the indicators of every latent variable that has a predecessor.  For a held-out row the scores of the
latent variables are the ones ``Plspm.scores()`` would give it under the training fit (training means, the training ``scaled`` scalar, the
normalised weights); the predicted score of an endogenous latent variable is the path-weighted sum of its direct predecessors' scores
(``technique="direct"``, SEMinR's ``predict_DA``) or the same recursion with predicted scores for predecessors that are endogenous themselves
(``technique="earliest"``, ``predict_EA``); an indicator is predicted as its training mean + (the ordinary least squares slope of the indicator
on its latent variable's score in the training rows = loading x sd(indicator) / sd(score)) x the predicted score.

The linear-model benchmark (columns ``lm.*``) regresses every target on an intercept and all indicators of the latent variables without a
predecessor, on the same training rows (normal equations from the device's training moments, ``numpy.linalg.lstsq`` on the host: minimum norm),
and is scored by the same kernel on the same held-out rows.

This project's metric definitions, per target indicator, pooled over all used (repetition, fold) problems:

    rmse = sqrt(sum SSE / sum rows),   mae = sum SAE / sum rows,   q2_predict = 1 - sum SSE / sum SST

with SSE / SAE the sums of the squared / absolute prediction errors of a problem's held-out rows and SST their squared distances from that
problem's *training* mean.  SEMinR averages a row's predictions over the repetitions first and scores the averages; equality with its numbers
is not claimed.

Used problems: a problem whose estimate did not converge is left out (as a failed bootstrap replicate is), from the PLS and the benchmark
columns alike; ``used()`` returns how many problems were used and how many rows x repetitions they cover.  Scope: metric data without missing
cells and without higher-order constructs (``NotImplementedError`` otherwise).
"""
import os

import numpy as np
import pandas as pd

import plspm.config as c
import plspm.weights as w
from plspm.estimator import Estimator
from plspm.scheme import Scheme

TECHNIQUES = ("direct", "earliest")
MIN_TRAINING_ROWS = 4
MIN_ITERATIONS = 100            # as Plspm: "default and minimum 100" (the tests lower it to see training fits fail)


def linear_model_coefficients(n_train, mean, cross, exogenous, targets, P):
    """The benchmark's affine maps [problems, T, P + 1] from the training moments of ``NativeModel.cv_moments``: per problem the regression of
    every target column on an intercept and the ``exogenous`` columns (minimum-norm least squares on the centred normal equations)."""
    nprob = mean.shape[0]
    iu = np.triu_indices(P)
    coef = np.zeros((nprob, len(targets), P + 1))
    S = np.empty((P, P))
    for q in range(nprob):
        S[iu] = cross[q]
        S.T[iu] = cross[q]
        b = np.linalg.lstsq(S[np.ix_(exogenous, exogenous)], S[np.ix_(exogenous, targets)], rcond=None)[0]       # [exogenous, T]
        coef[q][:, 1 + np.asarray(exogenous)] = b.T
        coef[q][:, 0] = mean[q, targets] - b.T @ mean[q, exogenous]
    return coef


class PLSpredict:
    """``PLSpredict(data, config, scheme=Scheme.PATH, iterations=100, tolerance=1e-6, folds=10, repetitions=10, technique="direct", seed=None,
    device_id=0, benchmark=True)``

    ``metrics()``: one row per target indicator, columns ``rmse``, ``mae``, ``q2_predict`` and (``benchmark=True``) ``lm.rmse``, ``lm.mae``,
    ``lm.q2_predict``.  ``predictions()``: the out-of-sample prediction of every row [N x T], averaged over the repetitions whose problem for
    that row was used; ``residuals()``: data - predictions.  See the module docstring for the definitions."""

    def __init__(self, data: pd.DataFrame, config: c.Config, scheme: Scheme = Scheme.PATH, iterations: int = 100, tolerance: float = 0.000001,
                 folds: int = 10, repetitions: int = 10, technique: str = "direct", seed: int = None, device_id: int = 0, benchmark: bool = True):
        assert tolerance > 0
        assert scheme in Scheme
        iterations = max(iterations, MIN_ITERATIONS)
        if technique not in TECHNIQUES:
            raise ValueError("technique must be one of %s" % ", ".join(TECHNIQUES))
        if not 2 <= int(folds) <= 256:
            raise ValueError("folds must be between 2 and 256")
        if int(repetitions) < 1:
            raise ValueError("repetitions must be at least 1")
        what = "out-of-sample prediction"
        if not config.metric():
            raise NotImplementedError(what + " covers metric data only (no Scale.NUM / RAW / ORD / NOM)")
        if config.hoc():
            raise NotImplementedError(what + " does not cover higher-order constructs")
        observations = config.filter(data)
        if config.nan_columns(observations).any():
            raise NotImplementedError(what + " needs complete data (no missing cells in the model's columns)")
        folds, repetitions = int(folds), int(repetitions)
        n = observations.shape[0]
        if n - (n + folds - 1) // folds < MIN_TRAINING_ROWS:
            raise ValueError("every training set needs at least %d rows: %d rows in %d folds leave %d" % (MIN_TRAINING_ROWS, n, folds, n - (n + folds - 1) // folds))
        self._folds, self._repetitions, self._technique = folds, repetitions, technique
        self._seed = int.from_bytes(os.urandom(8), "little") if seed is None else int(seed)
        calculator = w.WeightsCalculatorFactory(config, iterations, tolerance, np.sqrt(n / (n - 1)), scheme, device_id)
        whole = Estimator(config).run(calculator, observations, want_scores=False)
        native, cm = whole.native, whole.compiled
        self._native = native
        native.cv(repetitions, folds, self._seed)
        sse, sae, sst, rows, pred_sum, pred_cnt = native.cv_predict(repetitions, folds, TECHNIQUES.index(technique), predictions=True)
        targets = native.cv_targets()
        names = [cm.dev_mvs[p] for p in targets]
        used = rows > 0
        self._used = (int(used.sum()), int(rows.sum()))

        def pooled(sse, sae, sst, rows, prefix=""):
            total = float(rows.sum())
            with np.errstate(divide="ignore", invalid="ignore"):
                return {prefix + "rmse": np.sqrt(sse.sum(axis=0) / total), prefix + "mae": sae.sum(axis=0) / total,
                        prefix + "q2_predict": 1.0 - sse.sum(axis=0) / sst.sum(axis=0)}
        columns = pooled(sse, sae, sst, rows)
        self.raw = {"targets": targets, "sse": sse, "sae": sae, "sst": sst, "rows": rows, "pred_sum": pred_sum, "pred_cnt": pred_cnt}
        if benchmark:
            exogenous = [p for l in range(cm.L) if cm.path[l].sum() == 0 for p in range(cm.block_offset[l], cm.block_offset[l + 1])]
            n_train, mean, cross = native.cv_moments(repetitions, folds)
            coef = linear_model_coefficients(n_train, mean, cross, exogenous, targets, cm.P)
            coef[~used] = np.nan                             # the benchmark is scored on the problems the PLS prediction used
            lm = native.cv_predict(repetitions, folds, coef=coef)
            columns.update(pooled(lm[0], lm[1], lm[2], lm[3], "lm."))
            self.raw.update({"lm_sse": lm[0], "lm_sae": lm[1], "lm_sst": lm[2], "lm_rows": lm[3], "lm_coef": coef})
        self._metrics = pd.DataFrame(columns, index=names)
        with np.errstate(divide="ignore", invalid="ignore"):
            mean_pred = np.where(pred_cnt[:, None] > 0, pred_sum / pred_cnt[:, None], np.nan)
        self._predictions = pd.DataFrame(mean_pred, index=observations.index, columns=names)
        self._residuals = observations[names].astype(np.float64) - self._predictions

    def metrics(self) -> pd.DataFrame:
        return self._metrics

    def predictions(self) -> pd.DataFrame:
        return self._predictions

    def residuals(self) -> pd.DataFrame:
        return self._residuals

    def folds(self) -> np.ndarray:
        """[repetitions, N] the fold every row was held out in, per repetition (rows in the order of ``predictions()``)."""
        return self._native.cv_fold_ids(self._repetitions, self._folds)[0]

    def used(self):
        """(problems whose estimate converged and was used, rows x repetitions they cover)."""
        return self._used

    def seed(self) -> int:
        return self._seed

    def records(self):
        """The folds x repetitions training fits, fetched from HBM: (rows [repetitions * folds, R] in the device layout, status, iterations); record
        r * folds + f is the fit on the rows outside fold f of repetition r."""
        return self._native.fetch(0, self._repetitions * self._folds)
