"""SciPy / NumPy restatement of the bootstrap confidence intervals and the jackknife statistics (include/plspm_hip.h plspm_bootstrap_intervals,
plspm_jackknife_stats; plspm.bootstrap._intervals / _jackknife_stats) for the tests: written directly from the definitions, sharing no code with
the package's mirrors."""
import numpy as np
from scipy.stats import norm


def levels(level):
    """alpha and 1 - alpha, rounded to twelve decimals."""
    return round((1.0 - level) / 2.0, 12), round((1.0 + level) / 2.0, 12)


def interval(x, theta, method, level, accel=None):
    """(lower, upper, z0, accel, level.lower, level.upper) of one column: x the used replicates, theta the estimate."""
    x = np.asarray(x, dtype=np.float64)
    m = x.size
    nan = np.nan
    if m == 0 or np.isnan(theta):
        return (nan,) * 6
    a_lo, a_hi = levels(level)
    below = int((x < theta).sum())
    z0 = norm.ppf(below / m)
    if method in ("percentile", "basic"):
        p, a = (a_lo, a_hi), nan
    else:
        a = 0.0 if method == "bc" else float(accel)
        if below in (0, m) or np.isnan(a):
            return nan, nan, z0, a, nan, nan
        with np.errstate(divide="ignore", invalid="ignore"):
            p = tuple(float(norm.cdf(z0 + (z0 + z) / (1.0 - a * (z0 + z)))) for z in (norm.ppf(a_lo), norm.ppf(a_hi)))
        if np.isnan(p[0]) or np.isnan(p[1]):
            return nan, nan, z0, a, p[0], p[1]
    s = np.sort(x)

    def q(p_):
        pos = p_ * (m - 1)
        lo = int(np.floor(pos))
        hi = min(lo + 1, m - 1)
        return s[lo] + (s[hi] - s[lo]) * (pos - lo)
    lo, hi = q(p[0]), q(p[1])
    if method == "basic":
        lo, hi = 2.0 * theta - q(p[1]), 2.0 * theta - q(p[0])
    return lo, hi, z0, a, p[0], p[1]


def intervals(samples, original, method, level, accel=None):
    samples = np.asarray(samples, dtype=np.float64)
    return np.array([interval(samples[:, c], original[c], method, level, None if accel is None else accel[c]) for c in range(samples.shape[1])])


def jackknife_stats(records):
    """(mean, std_error, accel) per column with Python-float accumulation in math.fsum (correctly rounded sums)."""
    import math
    v = np.asarray(records, dtype=np.float64)
    n, R = v.shape
    mean, se, acc = np.full(R, np.nan), np.full(R, np.nan), np.full(R, np.nan)
    for c in range(R if n else 0):
        mu = math.fsum(v[:, c]) / n
        d = mu - v[:, c]
        s2, s3 = math.fsum(d * d), math.fsum(d * d * d)
        mean[c], se[c] = mu, math.sqrt((n - 1) / n * s2) if s2 == s2 else np.nan
        if s2 > 0:
            acc[c] = s3 / (6.0 * s2 ** 1.5)
    return mean, se, acc


def synthetic_records(rng, B, R, stride):
    """[B, stride] records of R columns, status 0, iterations 5: columns of different scale and location."""
    rec = np.zeros((B, stride))
    rec[:, :R] = rng.standard_normal((B, R)) * rng.uniform(0.01, 5.0, R) + rng.uniform(-3.0, 3.0, R)
    rec[:, R + 1] = 5.0
    return rec
