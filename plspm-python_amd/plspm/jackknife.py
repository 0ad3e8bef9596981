"""The jackknife -- delete-one or delete-a-group -- of a PLS path model on the GPU (not in the reference).

Problem g of ``groups`` (default: the number of rows, the ordinary leave-one-out jackknife) is the model estimated on the rows i with
i % groups != g; a smaller ``groups`` is the delete-a-group jackknife for data sets where N problems of N rows are too many.  Every problem is one
more 0/1 count row of the bootstrap's int8 Gram and batch solver (include/plspm_hip.h ``plspm_jackknife_device``, at least seven digit
planes), and the reduction runs on the records in HBM (``plspm_jackknife_stats``).  This project's definitions, per estimate, over the n
problems whose fit converged, with theta the full-sample estimate and d_g = mean - theta_(g):

    mean = sum theta_(g) / n      bias = (n - 1) (mean - theta)      std.error = sqrt((n - 1) / n  sum d_g^2)
    accel = sum d_g^3 / (6 (sum d_g^2)^1.5)   (NaN where sum d_g^2 = 0: constant columns such as absent paths)

``accel`` is the acceleration of the BCa bootstrap interval (``Bootstrap.intervals("bca")`` runs this jackknife on its own handle).  With
unequal groups (N % groups != 0) the formulas are still the equal-group ones.  Scope: metric data without missing cells and without
higher-order constructs (``NotImplementedError`` otherwise); one GPU.
"""
import numpy as np
import pandas as pd

import plspm.config as c
import plspm.inner_model as im
import plspm.weights as w
from plspm.bootstrap import Bootstrap, _result_frames
from plspm.estimator import Estimator
from plspm.scheme import Scheme

JACKKNIFE_COLUMNS = ["original", "mean", "bias", "std.error", "accel"]
MIN_TRAINING_ROWS = 4
MIN_ITERATIONS = 100            # as Plspm: "default and minimum 100"


class Jackknife:
    """``Jackknife(data, config, scheme=Scheme.CENTROID, groups=None, iterations=100, tolerance=1e-6, device_id=0)``

    ``weights()``, ``r_squared()``, ``total_effects()``, ``paths()`` and ``loading()``: the frames of ``Bootstrap`` (same index and order)
    with the columns ``original``, ``mean``, ``bias``, ``std.error``, ``accel``.  ``estimates()``: the problems' records; ``used()``: how many
    of them converged and entered the statistics."""

    def __init__(self, data: pd.DataFrame, config: c.Config, scheme: Scheme = Scheme.CENTROID, groups: int = None, iterations: int = 100,
                 tolerance: float = 0.000001, device_id: int = 0):
        assert tolerance > 0
        assert scheme in Scheme
        iterations = max(iterations, MIN_ITERATIONS)
        what = "the jackknife"
        if not config.metric():
            raise NotImplementedError(what + " covers metric data only (no Scale.NUM / RAW / ORD / NOM)")
        if config.hoc():
            raise NotImplementedError(what + " does not cover higher-order constructs")
        observations = config.filter(data)
        if config.nan_columns(observations).any():
            raise NotImplementedError(what + " needs complete data (no missing cells in the model's columns)")
        n = observations.shape[0]
        groups = n if groups is None else int(groups)
        if not 2 <= groups <= n:
            raise ValueError("groups must lie between 2 and the number of rows")
        if n - (n + groups - 1) // groups < MIN_TRAINING_ROWS:
            raise ValueError("every problem needs at least %d rows: %d rows in %d groups leave %d" % (MIN_TRAINING_ROWS, n, groups, n - (n + groups - 1) // groups))
        self._groups = groups
        calculator = w.WeightsCalculatorFactory(config, iterations, tolerance, np.sqrt(n / (n - 1)), scheme, device_id)
        estimator = Estimator(config)
        whole = estimator.run(calculator, observations, want_scores=False)
        native, cm = whole.native, whole.compiled
        self._native = native
        inner_model = im.InnerModel.from_device(estimator.config().path(), whole)
        original = Bootstrap._original(whole, inner_model, None)
        native.jackknife(groups)
        mean, se, accel, used = native.jackknife_stats(groups)
        self._used = used
        table = np.column_stack((original, mean, (used - 1) * (mean - original), se, accel))
        self._frames = _result_frames(cm, native.n_eff, inner_model, table, JACKKNIFE_COLUMNS)
        self._hidden = (self._frames["paths"]["mean"] == 0).values        # indirect-only pairs, as Bootstrap.paths() hides them

    def weights(self) -> pd.DataFrame:
        return self._frames["weights"]

    def r_squared(self) -> pd.DataFrame:
        return self._frames["r_squared"]

    def total_effects(self) -> pd.DataFrame:
        return self._frames["total_effects"]

    def paths(self) -> pd.DataFrame:
        return self._frames["paths"][~self._hidden]

    def loading(self) -> pd.DataFrame:
        return self._frames["loading"]

    def groups(self) -> int:
        return self._groups

    def used(self) -> int:
        """Number of problems whose fit converged and entered the statistics."""
        return self._used

    def estimates(self):
        """The problems' records, fetched from HBM: (rows [groups, R] in the device layout weights | r2 | total | direct | loadings, status,
        iterations); record g is the fit without the rows i with i % groups == g."""
        return self._native.jackknife_fetch(0, self._groups)
