"""GPU: the jackknife's statistics kernel (kernels_jack.h jack_stats_kernel) with more problems than threads and with some problems failed.

  B1  G = 257, 512, 600: thread t takes the problems t, t + 256, ... -- two and three trips of the `g += 256` loops, a second trip of one thread only
      (257), whole trips (512) and a ragged last one (600: leave-one-out);
  B2  some problems fail and most do not: the statistics run over the OK records alone;
  B3  N = 37: the count rows (jack_counts_kernel on count_rows.h) with a tail piece and a ragged last group of problems, against a cross-validation
      handed the same kept rows.

The bars are those of tests/test_gpu_ci.py (mean, std.error rtol 1e-12; accel atol 1e-12), against the package's mirror and against math.fsum
(tests/helpers_ci.py).  They still hold at n = 600: a fixed-order fp64 sum of n cubes is off by n eps of sum |d|^3 <= (sum d^2)^1.5 at most, so the
acceleration by n eps / 6 = 1.1e-14; the sum of squares by n eps = 6.7e-14 relative; and a mean that is off by its own n eps / 2 |theta| moves every
d_g alike, which the sum of squares does not see to first order (sum d = 0) and the acceleration sees as delta / (2 sqrt(sum d^2)) -- below 1e-12 while
the estimates' jackknife spread is above 2e-2 of their size, as it is here."""
import numpy as np
import pytest

import plspm_oracle as orc
from helpers import assert_close
from helpers_ci import jackknife_stats as fsum_jackknife_stats
from helpers_mga import oracle_record
from test_gpu_ci import check_stats, native_model

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-8, 1e-11
C3 = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0]])
JACK_NT = 256                      # threads of a jack_stats_kernel workgroup


def check_stats_fsum(stats, rows, ok):
    """The device's (mean, se, accel) against correctly rounded sums over the OK records."""
    m_ref, se_ref, a_ref = fsum_jackknife_stats(rows[ok])
    mean, se, accel = stats
    for mine, ref in ((mean, m_ref), (se, se_ref), (accel, a_ref)):
        assert np.array_equal(np.isnan(mine), np.isnan(ref))
    with np.errstate(invalid="ignore", divide="ignore"):
        print("against fsum: max rel mean %.3e se %.3e, max abs accel %.3e" % (
            np.nanmax(np.abs(mean / m_ref - 1)), np.nanmax(np.abs(se / se_ref - 1)), np.nanmax(np.abs(accel - a_ref))))
    np.testing.assert_allclose(mean, m_ref, rtol=1e-12, atol=0)
    np.testing.assert_allclose(se, se_ref, rtol=1e-12, atol=1e-300)
    np.testing.assert_allclose(accel, a_ref, rtol=0, atol=1e-12)


@pytest.mark.parametrize("G", [600, 257, 512])
def test_more_problems_than_threads(G):
    """600 rows, 3 LVs: G > 256 problems, so the loops over the problems make more than one trip.  Records against the oracle either side of every
    256-problem boundary, and the first and the last."""
    n = 600
    assert G > JACK_NT
    X, blocks = orc.synth(n, C3, 3, seed=12)
    model = orc.Model(blocks, C3, "ABA", "path", True)
    nm = native_model(model, X)
    nm.jackknife(G)
    assert nm.get_option("last_gram_path") == 2
    rows, status, iters = nm.jackknife_fetch(0, G)
    assert np.all(status == 0)
    sample = sorted({g for g in (0, 255, 256, 511, 512, G - 1) if g < G})
    assert sample[0] == 0 and sample[-1] == G - 1 and any(g >= JACK_NT for g in sample)
    for g in sample:
        mine, its = oracle_record(X, model, np.arange(n) % G != g)
        assert iters[g] == its, (g, iters[g], its)
        assert_close(rows[g], mine, RTOL, ATOL, what="jackknife problem %d of %d" % (g, G))
    stats = check_stats(nm, G, rows, status)
    check_stats_fsum(stats, rows, status == 0)
    # every problem counts: the statistics of the first 256 alone are others
    from plspm.bootstrap import _jackknife_stats
    first_trip = _jackknife_stats(rows[:JACK_NT])
    with np.errstate(invalid="ignore", divide="ignore"):
        assert np.nanmax(np.abs(first_trip[0] / stats[0] - 1)) > 1e-9 and np.nanmax(np.abs(first_trip[1] / stats[1] - 1)) > 1e-3


@pytest.mark.parametrize("G", [37, 5])
def test_count_rows_with_a_tail_piece(G):
    """N = 37: two whole 16-row pieces and a tail of five rows (kernels_jack.h jack_counts_kernel on count_rows.h); G = 37 (leave-one-out: five groups of eight
    problems, the last ragged) and G = 5 (29 or 30 rows kept).  The records are bit for bit those of a cross-validation handed the folds i % G -- the same kept
    rows as explicit bytes --, and the first and the last problem are the oracle's fits."""
    n = 37
    X, blocks = orc.synth(n, C3, 2, seed=14)
    model = orc.Model(blocks, C3, "AAA", "path", True)
    nm = native_model(model, X)
    assert n - -(-n // G) >= 4
    nm.jackknife(G)
    assert nm.get_option("last_gram_path") == 2
    rows, status, iters = nm.jackknife_fetch(0, G)
    nm.cv(1, G, fold=(np.arange(n) % G).astype(np.uint8)[None, :])
    rows2, status2, iters2 = nm.fetch(0, G)
    assert np.array_equal(status, status2) and np.array_equal(iters, iters2) and np.array_equal(rows, rows2, equal_nan=True)
    for g in (0, G - 1):
        mine, its = oracle_record(X, model, np.arange(n) % G != g)
        assert status[g] == 0 and iters[g] == its, (g, status[g], iters[g], its)
        assert_close(rows[g], mine, RTOL, ATOL, what="jackknife problem %d of %d" % (g, G))


def test_some_problems_fail_and_the_rest_are_used():
    """Leave-one-out of 120 rows, Mode B: the iteration limit -- chosen on the CPU with the oracle -- fails at least one problem and fewer than half.  The
    device's statuses are the oracle's pattern, `used` is the OK count, and mean, std.error and acceleration are those of the OK records alone, which are
    not those of all records."""
    from plspm.bootstrap import _jackknife_stats
    n = G = 120
    X, blocks = orc.synth(n, C3, 3, seed=3)
    free = orc.Model(blocks, C3, "BBB", "centroid", True)
    its = np.array([oracle_record(X, free, np.arange(n) % G != g)[1] for g in range(G)])
    limit = int(its.max()) - 1
    failing = its > limit
    print("iterations %s, limit %d, failing %d of %d" % (np.bincount(its).tolist(), limit, failing.sum(), G))
    assert 1 <= failing.sum() < G / 2
    model = orc.Model(blocks, C3, "BBB", "centroid", True, max_iter=limit)
    nm = native_model(model, X)
    nm.jackknife(G)
    rows, status, iters = nm.jackknife_fetch(0, G)
    assert np.array_equal(status != 0, failing), (np.flatnonzero(status != 0), np.flatnonzero(failing))
    assert np.array_equal(iters[~failing], its[~failing])
    for g in (int(np.flatnonzero(~failing)[0]), int(np.flatnonzero(~failing)[-1])):
        assert_close(rows[g], oracle_record(X, model, np.arange(n) % G != g)[0], RTOL, ATOL, what="jackknife problem %d" % g)
    mean, se, accel = check_stats(nm, G, rows, status)                                # (asserts used == the OK count)
    assert nm.jackknife_stats(G)[3] == G - failing.sum()
    check_stats_fsum((mean, se, accel), rows, ~failing)
    # the failed problems would have mattered
    everything = _jackknife_stats(rows)
    with np.errstate(invalid="ignore"):
        assert not np.allclose(everything[0], mean, rtol=1e-9, atol=0) and not np.allclose(everything[1], se, rtol=1e-9, atol=0)
