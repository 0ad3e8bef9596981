"""CPU check of the single fit's plan (csrc/fit_route.h fit_plan, csrc/solver_route.h solver_lds) through the emulation build in tests/hostemu/: an explicit table with a
row for every decision plspm_fit used to make inline -- the layout of the result block, the row chunks of the dense Gram, the scores launch, whether the scores ride
the pinned block, where the solver keeps its workspace -- and their edges.  The expected values are worked out by hand from the formulas plspm_fit, dense_moments and
launch_solver carried before the plan had a function of its own:

    block, sizes in doubles: weights P | loadings P | crossloadings P L | path L^2 | r2 L | lv_cov L^2 | record 2P + L + 2 n_eff + 2 | indirect max(n_eff, 1) | score_w P |
                       score_c L | mean P | cov P^2;  tail = 64 + L + 16 bytes (iterations int 0, status int 1, signs from int 4);  total / direct at record + Po + L (+ n_eff)
    chunks = ceil(ceil(N / 4) / (16 waves' k-groups x 4 waves at T <= 4, x 1 above)), 1 .. 512 at T <= 4, 1 .. 256 above
    scores LDS (tr rows) = (tr (PA + 1) + P + L + tr L) 8 + (L + 2) 4;  32 rows while that is <= 72 KiB;  class = ceil(PA / 32) -> 2 / 4 / 6 / 8, 0 beyond 8
    per_cu = 160 KiB / LDS, 1 .. 8;  grid = min(256 per_cu, ceil(N / tr));  staged: 0 < 8 N L <= 8 MiB
    solver: descriptors + small workspace + S against 160 KiB (one problem) / 64 KiB (a batch)
"""
import ctypes

import numpy as np
import pytest

import plspm_oracle as orc
from helpers_batch_route import tiles_for
from helpers_gram_route import load_emu
from test_solver_route import dag, shape as route_shape

OUT = ("o_w", "o_ld", "o_cl", "o_pc", "o_r2", "o_lc", "o_row", "o_ind", "o_sw", "o_sc", "o_mean", "o_cov", "o_end", "h_total", "h_direct", "tail_bytes", "fit_bytes", "block_bytes", "nchunks",
       "tile_rows", "cls", "lds", "ntl", "per_cu", "grid", "score_bytes", "stage_scores", "stage_need", "s_in_lds", "small_in_lds", "solver_lds", "batch_s_in_lds", "batch_small_in_lds",
       "batch_solver_lds", "int_iters", "int_status", "int_sign")
MiB = 1 << 20


@pytest.fixture(scope="module")
def emu():
    return load_emu()


def fit_shape(N, sizes, C, modes=None, Pm=None):
    """A handle of N rows as plspm_model_create and the upload derive it (csrc/host_internal.h fit_shape); Pm: the logical MVs of a categorical handle whose
    sum(sizes) device columns are aug columns."""
    P, L, kmax, n_chol, n_eff, nedge, _ = route_shape(sizes, modes or "A" * len(sizes), C)
    T = tiles_for(P, Pm is not None)
    return dict(N=N, P=P, Po=P if Pm is None else Pm, L=L, n_eff=n_eff, PA=16 * T, T=T, kmax=kmax, n_chol=n_chol, nedge=nedge, categorical=int(Pm is not None))


def plan(lib, s, want_scores=0, want_cov=0, fit_chunks=0, scores_tile=0):
    sh = np.array([s[k] for k in ("N", "P", "Po", "L", "n_eff", "PA", "T", "kmax", "n_chol", "nedge", "categorical")], dtype=np.int64)
    cl = np.array([want_scores, want_cov, fit_chunks, scores_tile], dtype=np.int64)
    out = np.zeros(len(OUT), dtype=np.int64)
    lib.hostemu_fit_plan(*[a.ctypes.data_as(ctypes.c_void_p) for a in (sh, cl, out)])
    return dict(zip(OUT, (int(v) for v in out)))


SAT = orc.satisfaction_C()
NONE2 = np.zeros((2, 2), dtype=np.int64)


def head(N=10000):
    """bench.py's model: 60 MVs under 6 LVs (15 effect pairs, 10 edges, at most 4 predecessors)."""
    return fit_shape(N, [10] * 6, SAT)


def wide(N=1000000):
    return fit_shape(N, [10] * 20, dag(20, 1))      # 200 MVs under a chain of 20 LVs: 13 tiles


def one_block(P, N=67, L=2):
    """P MVs under L LVs in a chain, the first block taking the rest."""
    return fit_shape(N, [P - (L - 1)] + [1] * (L - 1), dag(L, 1))


def two(N, C=None):
    return fit_shape(N, [2, 2], orc.chain_C(2) if C is None else C)


# (id, shape, call, expected)
PLANS = [
    ("headline 10,000 x 60 x 6", head(), dict(want_scores=1),
     dict(nchunks=40, tile_rows=32, cls=2, lds=18736, ntl=313, per_cu=8, grid=313, score_bytes=480000, stage_scores=1, o_w=0, o_ld=60, o_cl=120, o_pc=480, o_r2=516, o_lc=522, o_row=558,
          o_ind=716, o_sw=731, o_sc=791, o_mean=797, o_cov=857, o_end=4457, h_total=624, h_direct=639, tail_bytes=86, fit_bytes=35742, block_bytes=6856, stage_need=515742,
          int_iters=0, int_status=1, int_sign=4, s_in_lds=1, small_in_lds=1, solver_lds=1152 + 10656 + 29768, batch_s_in_lds=1, batch_solver_lds=41576)),
    ("headline without scores: the block alone", head(), {}, dict(score_bytes=0, stage_scores=0, stage_need=35742, block_bytes=6856)),
    ("headline with the covariance matrix", head(), dict(want_cov=1), dict(block_bytes=35656, fit_bytes=35742, stage_need=35742)),
    ("1,000,000 x 200 x 20", wide(), dict(want_scores=1),
     dict(nchunks=256, tile_rows=32, cls=8, lds=60472, ntl=31250, per_cu=2, grid=512, score_bytes=160000000, stage_scores=0, stage_need=8 * (400 + 4000 + 400 + 20 + 400 + 802 + 190 + 200 + 20 + 200 + 40000) + 100,
          # 5,128 bytes of descriptors + 70,112 of small workspace fit one CU, the 323,208 of S do not; a batch's 64 KiB take neither
          s_in_lds=0, small_in_lds=1, solver_lds=75240, batch_s_in_lds=0, batch_small_in_lds=0, batch_solver_lds=5128)),
    ("100 MVs x 4 LVs: S (81,608 bytes) in LDS for one problem, not in a batch", fit_shape(500, [25] * 4, dag(4, 1)), {},
     dict(s_in_lds=1, small_in_lds=1, solver_lds=1484 + 10240 + 81608, batch_s_in_lds=0, batch_small_in_lds=1, batch_solver_lds=11724)),
    # ---- the row chunks
    ("N 2: one chunk", two(2), {}, dict(nchunks=1)),
    ("N 1", two(1), {}, dict(nchunks=1)),
    ("N 3", two(3), {}, dict(nchunks=1)),
    ("N 257, T 2: 65 k-groups, two chunks", two(257), {}, dict(nchunks=2)),
    ("T <= 4: 511 chunks", head(130816), {}, dict(nchunks=511)),
    ("T <= 4: 512 exactly", head(131072), {}, dict(nchunks=512)),
    ("T <= 4: the cap", head(131073), {}, dict(nchunks=512)),
    ("T > 4: 255 chunks", wide(16320), {}, dict(nchunks=255)),
    ("T > 4: 256 exactly", wide(16384), {}, dict(nchunks=256)),
    ("T > 4: the cap", wide(16385), {}, dict(nchunks=256)),
    ("fit_chunks below the automatic count", head(), dict(fit_chunks=3), dict(nchunks=3)),
    ("fit_chunks above the cap at T <= 4", head(), dict(fit_chunks=1000), dict(nchunks=1000)),
    ("fit_chunks at T > 4", wide(), dict(fit_chunks=3), dict(nchunks=3)),
    ("fit_chunks above the cap at T > 4", wide(), dict(fit_chunks=300), dict(nchunks=300)),
    # ---- the scores kernel's chunk class
    ("P + 1 = 64: PA 64", one_block(63), dict(want_scores=1), dict(cls=2, tile_rows=32)),
    ("P + 1 = 65: PA 80", one_block(64), dict(want_scores=1), dict(cls=4, tile_rows=32)),
    ("P + 1 = 128: PA 128", one_block(127), dict(want_scores=1), dict(cls=4, tile_rows=32)),
    ("P + 1 = 129: PA 144", one_block(128), dict(want_scores=1), dict(cls=6, tile_rows=32)),
    ("P + 1 = 192: PA 192", one_block(191), dict(want_scores=1), dict(cls=6, tile_rows=32)),
    ("P + 1 = 193: PA 208", one_block(192), dict(want_scores=1), dict(cls=8, tile_rows=32)),
    ("P + 1 = 256: PA 256, 32 rows take 68,376 bytes", one_block(255), dict(want_scores=1), dict(cls=8, tile_rows=32, lds=68376, per_cu=2, ntl=3, grid=3)),
    ("P + 1 = 257: PA 288, 32 rows would take 76,576: 16", one_block(256), dict(want_scores=1), dict(cls=0, tile_rows=16, lds=39328, per_cu=4, ntl=5, grid=5)),
    ("scores_tile 32 forces the tall tile", one_block(256), dict(want_scores=1, scores_tile=32), dict(cls=0, tile_rows=32, lds=76576, per_cu=2, ntl=3)),
    ("scores_tile 16 forces the short one", one_block(255), dict(want_scores=1, scores_tile=16), dict(cls=8, tile_rows=16, lds=35224, per_cu=4, ntl=5)),
    ("scores_tile 16 on the headline", head(), dict(want_scores=1, scores_tile=16), dict(tile_rows=16, lds=(16 * 65 + 66 + 96) * 8 + 32, per_cu=8, ntl=625, grid=625)),
    ("more tiles than resident workgroups", head(100000), dict(want_scores=1), dict(tile_rows=32, per_cu=8, ntl=3125, grid=2048)),
    # ---- scores on the pinned block
    ("scores of exactly 8 MiB ride the pinned block", two(524288), dict(want_scores=1), dict(score_bytes=8 * MiB, stage_scores=1, fit_bytes=618, stage_need=618 + 8 * MiB)),
    ("one row more: straight to the caller", two(524289), dict(want_scores=1), dict(score_bytes=8 * MiB + 16, stage_scores=0, fit_bytes=618, stage_need=618)),
    # ---- the layout
    ("4 MVs x 2 LVs, one effect pair", two(100), {},
     dict(o_w=0, o_ld=4, o_cl=8, o_pc=16, o_r2=20, o_lc=22, o_row=26, o_ind=40, o_sw=41, o_sc=45, o_mean=47, o_cov=51, o_end=67, h_total=32, h_direct=33, tail_bytes=82, fit_bytes=618, block_bytes=408)),
    ("... with the covariance matrix", two(100), dict(want_cov=1), dict(block_bytes=536, fit_bytes=618)),
    ("no effect pairs: the indirect slot keeps one double", two(100, NONE2), {},
     dict(o_row=26, o_ind=38, o_sw=39, o_sc=43, o_mean=45, o_cov=49, o_end=65, h_total=32, h_direct=32, fit_bytes=8 * 65 + 82, block_bytes=8 * 49)),
    ("categorical, 12 aug columns of 4 logical MVs: total / direct behind Pm + L", fit_shape(100, [6, 6], orc.chain_C(2), Pm=4), {},
     dict(o_ld=12, o_cl=24, o_pc=48, o_r2=52, o_lc=54, o_row=58, o_ind=88, o_sw=89, o_sc=101, o_mean=103, o_cov=115, o_end=259, h_total=64, h_direct=65)),
]


@pytest.mark.parametrize("s,cl,expected", [c[1:] for c in PLANS], ids=[c[0] for c in PLANS])
def test_fit_plan(emu, s, cl, expected):
    got = plan(emu, s, **cl)
    assert {k: got[k] for k in expected} == expected
    # what holds for every call: the parts follow one another without a gap, the byte counts agree with the chain, the tail's ints and signs fit it
    P, L, ne = s["P"], s["L"], s["n_eff"]
    sizes = (P, P, P * L, L * L, L, L * L, 2 * P + L + 2 * ne + 2, max(ne, 1), P, L, P, P * P)
    offs = [got[k] for k in OUT[:13]]
    assert offs[0] == 0 and [b - a for a, b in zip(offs, offs[1:])] == list(sizes)
    assert got["fit_bytes"] == 8 * got["o_end"] + got["tail_bytes"] and got["tail_bytes"] >= 4 * got["int_sign"] + L
    assert got["block_bytes"] == 8 * (got["o_end"] if cl.get("want_cov") else got["o_cov"])
    assert got["h_direct"] + ne <= got["o_ind"] and got["h_total"] == got["o_row"] + s["Po"] + L
    assert got["stage_need"] == got["fit_bytes"] + (got["score_bytes"] if got["stage_scores"] else 0)
    assert got["grid"] >= 1 and got["grid"] <= got["ntl"] and got["lds"] <= 160 * 1024
    assert not got["s_in_lds"] or got["small_in_lds"]
    assert not got["batch_small_in_lds"] or got["small_in_lds"]


def test_shapes_of_the_table():
    assert (head()["T"], head()["PA"], head()["n_eff"], head()["nedge"], head()["kmax"]) == (4, 64, 15, 10, 4)
    assert (wide()["T"], wide()["PA"], wide()["n_eff"], wide()["nedge"], wide()["kmax"]) == (13, 208, 190, 19, 1)
    assert [one_block(P)["PA"] for P in (63, 64, 127, 128, 191, 192, 255, 256)] == [64, 80, 128, 144, 192, 208, 256, 288]
    assert (two(2)["T"], two(2)["n_eff"], two(2, NONE2)["n_eff"]) == (2, 1, 0)
    cat = fit_shape(100, [6, 6], orc.chain_C(2), Pm=4)
    assert (cat["P"], cat["Po"], cat["PA"], cat["categorical"]) == (12, 4, 32, 1)


def test_every_class_and_tile_has_a_row():
    assert {(c[3]["tile_rows"], c[3]["cls"]) for c in PLANS if "cls" in c[3]} >= {(32, 2), (32, 4), (32, 6), (32, 8), (32, 0), (16, 0), (16, 8)}
