"""The single fit (csrc/plspm_fit.hip plspm_fit) at the edges of its plan (csrc/fit_route.h; the plan itself: tests/test_fit_route.py), through NativeModel.fit: every
tile count of the dense Gram with its launch options, every instantiation of the scores kernel at tile sizes that do not divide N, the 8 MiB edge of the scores' way
to the host, a staging block that grows between calls, a model without effect pairs.  References: oracle/plspm_oracle.py and NumPy, at the tolerances
tests/test_gpu_parity.py applies to the same quantities (covariance 1e-10 / 1e-13, means 1e-12 / 1e-13, scores 1e-7 / 1e-9, weights 1e-8)."""
import functools

import numpy as np
import pytest

import plspm_oracle as orc
from fuzz_cases import _ragged
from helpers import assert_close
from helpers_batch_route import tiles_for
from test_gpu_parity import RTOL, native_model

pytestmark = pytest.mark.gpu
CHAIN2 = np.array([[0, 0], [1, 0]])
# MVs whose columns + the ones column fill T 16-column tiles (csrc/plspm_hip.hip tiles_for): even counts everywhere, the odd ones 5 .. 15 that metric models run
P_OF_T = {2: 4, 4: 40, 5: 70, 6: 90, 7: 100, 8: 116, 9: 130, 10: 150, 11: 166, 12: 180, 13: 200, 14: 216, 15: 230, 16: 250, 18: 260, 20: 300}
GRAM = ([(T, None, 0) for T in sorted(P_OF_T)] + [(13, "wide_ring", v) for v in (0, 4, 6)] + [(14, "wide_nw", v) for v in (4, 8, 16)] +
        [(T, "fit_chunks", v) for T in (4, 13) for v in (1, 3)])


def two_blocks(N, P, seed):
    """N rows of P MVs under two LVs, the second regressed on the first, all Mode A."""
    X, blocks = _ragged(N, CHAIN2, [P // 2, P - P // 2], seed=seed)
    return X, orc.Model(blocks, CHAIN2, "AA", "centroid", True)


def fit(X, model, options=(), **kw):
    nm = native_model(model)
    for key, value in options:
        nm.set_option(key, value)
    nm.upload(np.ascontiguousarray(X), model.mv_order.astype(np.int32))
    return nm.fit(**kw)


@functools.lru_cache(maxsize=None)
def gram_reference(T):
    X, model = two_blocks(133, P_OF_T[T], seed=T)
    Xo = X[:, model.mv_order]
    Xt = orc.treat_metric(Xo, True)
    return X, model, Xt.T @ Xt / X.shape[0], Xo.mean(axis=0)


@pytest.mark.parametrize("T,option,value", GRAM, ids=["T%d%s" % (T, "" if o is None else "-%s%d" % (o, v)) for T, o, v in GRAM])
def test_dense_gram_of_every_tile_count(T, option, value):
    """133 rows -- no multiple of the four rows of a k-group -- through gram_rows_kernel (T 2, 4), gram_wide_kernel (5 .. 16; T 13 on the ring of 4 and 6 row buffers and
    on the ping-pong, T 14 with 4, 8 and 16 virtual waves) and gram_block_kernel (18, 20), in one row chunk, in three and in the automatic count."""
    X, model, cov, mean = gram_reference(T)
    assert tiles_for(X.shape[1], False) == T
    g = fit(X, model, [(option, value)] if option else [], want_scores=False, want_cov=True)
    assert_close(g["cov"], cov, 1e-10, 1e-13, what="treated covariance")
    assert_close(g["mean"], mean, 1e-12, 1e-13, what="means")


@functools.lru_cache(maxsize=None)
def scores_reference(P, N):
    X, model = two_blocks(N, P, seed=P + N)
    return X, model, orc.fit(X, model)


def check_scores(g, r, model, tag):
    inv = np.empty(len(model.mv_order), dtype=np.int64); inv[model.mv_order] = np.arange(len(inv))
    assert g["status"] == 0, tag
    assert_close(g["weights"][inv], r["weights"], RTOL, what=tag + " weights")
    assert_close(g["scores"], r["scores"], 1e-7, 1e-9, what=tag + " scores")


# the five chunk classes of scores_kernel (PA 32, 80, 144, 208, 288) under both tile sizes and the automatic choice, which takes 32 rows up to P = 255 and 16 from 256
SCORES = [(P, tile) for P in (4, 64, 128, 192, 256) for tile in (0, 16, 32)] + [(255, 0)]


@pytest.mark.parametrize("N", [67, 32])
@pytest.mark.parametrize("P,tile", SCORES)
def test_scores_of_every_instantiation(P, tile, N):
    """67 rows: neither tile size divides them, the last tile is partial; 32 rows: exactly one tile of 32."""
    X, model, r = scores_reference(P, N)
    g = fit(X, model, [("scores_tile", tile)], want_scores=True)
    check_scores(g, r, model, "P=%d N=%d scores_tile=%d" % (P, N, tile))


@functools.lru_cache(maxsize=None)
def staging_rows():
    return two_blocks(524289, 4, seed=9)


@pytest.mark.parametrize("N", [524288, 524289])
def test_scores_at_the_edge_of_the_pinned_block(N):
    """Two LVs: 524,288 rows of scores are exactly 8 MiB and ride the pinned block behind the results; one row more goes straight into the caller's array."""
    Xall, model = staging_rows()
    X = np.ascontiguousarray(Xall[:N])
    g = fit(X, model, want_scores=True)
    assert g["scores"].shape == (N, 2) and g["scores"].nbytes == 8 * N * 2
    check_scores(g, orc.fit(X, model), model, "N=%d" % N)


def test_one_handle_three_calls_share_every_bit():
    """No scores, then scores (the staging block grows by them), then scores and the covariance matrix (the download takes the whole block): what the calls share is
    bit-identical."""
    C = orc.satisfaction_C()
    X, blocks = orc.synth(1000, C, 10, seed=5)
    model = orc.Model(blocks, C, "AAAAAA", "path", True)
    nm = native_model(model)
    nm.upload(X, model.mv_order.astype(np.int32))
    a = nm.fit(want_scores=False)
    b = nm.fit(want_scores=True)
    c = nm.fit(want_cov=True)
    assert a["scores"] is None and a["cov"] is None and b["cov"] is None and c["cov"].shape == (60, 60) and a["status"] == 0
    shared = [k for k in a if k not in ("scores", "cov")]
    assert len(shared) == 13
    for k in shared:
        assert np.array_equal(a[k], b[k]) and np.array_equal(a[k], c[k]), k
    assert np.array_equal(b["scores"], c["scores"])
    r = orc.fit(X, model)
    assert_close(c["scores"], r["scores"], 1e-7, 1e-9, what="scores")
    Xt = orc.treat_metric(X[:, model.mv_order], True)
    assert_close(c["cov"], Xt.T @ Xt / X.shape[0], 1e-10, 1e-13, what="treated covariance")


def test_two_unconnected_lvs_have_no_effects():
    """No path at all: n_eff = 0, the indirect effects keep a slot of one double in the result block and nothing of it reaches the caller.  The call returns with a
    status of its own (an inner estimate of zero has no weights to normalise); the per-LV and per-MV results keep their shapes."""
    none = np.zeros((2, 2), dtype=np.int64)
    X, blocks = _ragged(200, none, [2, 2], seed=3)
    model = orc.Model(blocks, none, "AA", "centroid", True)
    nm = native_model(model)
    assert nm.n_eff == 0
    nm.upload(X, model.mv_order.astype(np.int32))
    g = nm.fit()
    with pytest.raises(Exception, match="converge"):      # (the oracle's own verdict on an inner estimate of zero)
        orc.fit(X, model)
    assert g["status"] in (1, 2, 3) and 0 <= g["iterations"] <= model.max_iter + 1
    assert g["total"].size == 0 and g["direct"].size == 0 and g["indirect"].size == 0
    assert g["scores"].shape == (200, 2) and g["weights"].shape == (4,) and g["path_coef"].shape == (2, 2)
