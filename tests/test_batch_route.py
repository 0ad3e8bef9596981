"""CPU check of the batch driver's plan (csrc/batch_route.h batch_plan / batch_chunk: Gram route, solver arrangement, scratch buffers and strides, problems per pass)
through the emulation build in tests/hostemu/: an explicit table with a row for every decision and the edges of the pass budgets, the histogram window and the int8
route.  The expected values are what the driver's prelude computed before the plan had a function of its own, worked out by hand from its formulas:

    ent_stride = (N + 3 & ~3) + 4 int2 entries; kpad = 64 bytes x 2 ceil(N / 128) k-blocks; psize = T (T + 1) / 2 x 256 doubles; a dense matrix (Pg + 1) x ((Pg + 1) | 1)
    10,000 x 60: 80,032 bytes of list, 10,112 of counts, 4 tiles -> 20,480 bytes packed, 61 x 61 doubles = 29,768 dense
    per_rep = lists + max(packed, dense) + global histogram + uint16 histogram + counts + verification;  chunk = min(B, budget / per_rep), whole 256s on the int8 route
"""
import numpy as np
import pytest

import plspm_oracle as orc
import test_nm_route as nmr
from helpers_batch_route import (BUDGETED, CROSS_VALIDATION, GiB, JACKKNIFE, PERMUTATION, PLAIN, SOLVE_HOC, SOLVE_METRIC, SOLVE_MOMENTS, SOLVE_NM_WAVE, SOLVE_NONMETRIC, STRATIFIED, call, chunk,
                                 load_emu, metric_shape, nonmetric_shape, plan, tiles_for)
from test_solver_route import LDS, WAVE16_8


@pytest.fixture(scope="module")
def emu():
    return load_emu()


SAT = orc.satisfaction_C()


def head(N=10000, **kw):
    """bench.py's model: 60 MVs under 6 LVs, all Mode A."""
    return metric_shape([10] * 6, "A" * 6, SAT, N, **kw)


def narrow(N):
    return metric_shape([2, 2], "AA", orc.chain_C(2), N)


NUM = nonmetric_shape(nmr.num_shape([10] * 6, 10000))                  # tools/nonmetric_bench.py
CAT = nonmetric_shape(nmr.cat_shape([[5] * 10] * 6, 10000))            # tools/categorical_bench.py: 300 indicator columns
HOC = nonmetric_shape(nmr.cat_shape([[5] * 4] * 4, 3000), nm2=nmr.cat_shape([[5] * 4, [1] * 3], 3000, attached=1, P1=80, kb=60))
ATTACHED = nonmetric_shape(nmr.cat_shape([[5] * 4, [1] * 3], 3000, attached=1, P1=80, kb=60))
WIDE = metric_shape([200] * 12, "A" * 12, orc.chain_C(12), 1000)      # 2,400 MVs: 180,226 pair groups
NUM_VERIFY = 102 * 67 * 8 + 4 * (133 + 8) * 8                          # (max_iter + 2) score maps of P + L + 1 doubles + four slots of a table row + 64 bytes
CAT_VERIFY = 102 * 307 * 8 + 8 * (6 * 2 * 7 * 2 * 64 + 64)             # ... + eight slots of digit planes + 64 bytes
# (id, shape, call, options, expected)
PLANS = [
    ("headline: int8 route, no lists, dense solver, one pass", head(), call(5000), {},
     dict(gpath=2, plane_floor=0, lds_hist=1, need_lists=0, need_ghist=0, rows_solver=1, dense=1, route=WAVE16_8, nm_wave=0, want16=0, micom=0, raises=0, sub_batches=1, ent_stride=10004, psize=2560,
          kpad=10112, ent_bytes=0, gram_budget_bytes=29768, gram_bytes=29768, counts_bytes=10112, per_rep=39880, budget=2 * GiB, chunk=5000, passes=1, closed=0, counts_route_open=1)),
    ("headline, B 100,000: the 2 GiB budget cuts at 53,848 -> 210 tiles of 256", head(), call(100000), {}, dict(per_rep=39880, chunk=53760, passes=2)),
    ("headline, B 53,848: the last batch in one pass", head(), call(53848), {}, dict(chunk=53848, passes=1)),
    ("headline, B 53,849", head(), call(53849), {}, dict(chunk=53760, passes=2)),
    ("boot_pass 256 against B 600", head(), call(600), dict(boot_pass=256), dict(chunk=256, passes=3)),
    ("boot_pass above the batch changes nothing", head(), call(600), dict(boot_pass=1024), dict(chunk=600, passes=1)),
    ("boot_pass caps the fp64 route too", head(), call(600), dict(boot_pass=256, gram_path=1), dict(gpath=1, chunk=256, passes=3)),
    ("gram_path 1: fp64 route on lists", head(), call(5000), dict(gram_path=1),
     dict(gpath=1, need_lists=1, need_ghist=0, rows_solver=0, dense=0, route=WAVE16_8, ent_bytes=80032, nent_bytes=4, gram_budget_bytes=29768, gram_bytes=20480, counts_bytes=0, per_rep=109800, chunk=5000)),
    ("fp64 route: the cut is not rounded to tiles", head(), call(100000), dict(gram_path=1), dict(chunk=(2 * GiB) // 109800, passes=6)),
    ("B below i8_min_batch", head(), call(999), dict(i8_min_batch=1000), dict(gpath=1, need_lists=1)),
    ("B at i8_min_batch", head(), call(1000), dict(i8_min_batch=1000), dict(gpath=2, need_lists=0)),
    ("gram_path 2 whatever i8_min_batch says", head(), call(10), dict(i8_min_batch=1000, gram_path=2), dict(gpath=2)),
    ("explicit indices on the int8 route: lists for the fallback", head(), call(5000, explicit_idx=1), {},
     dict(gpath=2, need_lists=1, rows_solver=1, raises=1, sub_batches=0, ent_bytes=80032, gram_bytes=29768, counts_bytes=10112, per_rep=119912)),
    ("solver_rows 0: packed matrices", head(), call(5000), dict(solver_rows=0), dict(gpath=2, route=LDS, rows_solver=0, dense=0, gram_budget_bytes=29768, gram_bytes=20480, per_rep=39880)),
    # ---- the histogram window
    ("N 65,535, fp64 route: the LDS histogram", head(65535), call(600), dict(gram_path=1), dict(lds_hist=1, need_lists=1, need_ghist=0, ent_stride=65540, ghist_bytes=0)),
    ("N 65,536, fp64 route: a global histogram per replicate", head(65536), call(600), dict(gram_path=1), dict(lds_hist=0, need_lists=1, need_ghist=1, ent_stride=65540, ghist_bytes=262144, per_rep=524320 + 29768 + 262144)),
    ("N 65,536, int8 route on Philox draws: no lists, no histogram", head(65536), call(600), {}, dict(gpath=2, lds_hist=0, need_lists=0, need_ghist=0)),
    ("N 65,536, explicit indices: lists from the global histogram", head(65536), call(600, explicit_idx=1), {}, dict(gpath=2, need_lists=1, need_ghist=1)),
    ("Scale.NUM, N 65,535 without counts8: open, uint16 histograms", nonmetric_shape(nmr.num_shape([10] * 6, 65535)), call(600), dict(nm_counts8=0), dict(gpath=2, closed=0, counts8_plan=0, want_dcnt=1, need_lists=1, need_ghist=0)),
    ("Scale.NUM, N 65,536 without counts8: closed", nonmetric_shape(nmr.num_shape([10] * 6, 65536)), call(600), dict(nm_counts8=0), dict(gpath=1, closed=1, counts_route_open=0, want_dcnt=0, need_lists=1, need_ghist=1)),
    ("Scale.NUM, N 65,536 with counts8: open", nonmetric_shape(nmr.num_shape([10] * 6, 65536)), call(600), {}, dict(gpath=2, closed=0, counts8_plan=1, want_dcnt=0, need_lists=0, nm_wave=1)),
    ("Scale.NUM, N 65,536, explicit indices: the int8 counts are the only dense multiplicities", nonmetric_shape(nmr.num_shape([10] * 6, 65536)), call(600, explicit_idx=1), {}, dict(gpath=2, counts8_plan=1, need_lists=1, need_ghist=1, want_dcnt=0)),
    ("Scale.NUM, N 10,000, explicit indices: lists and uint16 histograms", NUM, call(600, explicit_idx=1), {}, dict(gpath=2, counts8_plan=0, want_dcnt=1, need_lists=1, nm_wave=0)),
    # ---- the int8 route closed
    ("N 2^24 - 1, 4 MVs: 14 planes' digit blocks x 262,150 k-blocks within 24 GiB", narrow((1 << 24) - 1), call(600), {}, dict(gpath=2, closed=0, counts_route_open=1)),
    ("N 2^24: int32 accumulators", narrow(1 << 24), call(600), dict(gram_path=2), dict(gpath=1, closed=1, counts_route_open=0)),
    ("N 2^24 - 1, 60 MVs: 840 digit blocks per k-block beyond 24 GiB", head((1 << 24) - 1), call(600), dict(gram_path=2), dict(gpath=1, closed=1, counts_route_open=0)),
    ("an attached second stage", ATTACHED, call(600), dict(gram_path=2), dict(gpath=1, closed=1, counts_route_open=0)),
    ("2,400 MVs x 700 rows: 18 k-blocks of planes within 24 GiB", dict(WIDE, N=700), call(600), {}, dict(gpath=2, closed=0, counts_route_open=1)),
    ("2,400 MVs x 1,000 rows: 22 k-blocks x 1,261,582 KiB beyond", WIDE, call(600), {}, dict(gpath=1, closed=1, counts_route_open=0)),
    ("2,400 MVs x 1,000 rows at five planes: open for the bootstrap, not for a call that brings counts", WIDE, call(600), dict(i8_slices=5), dict(gpath=2, closed=0, counts_route_open=0)),
    # ---- the kinds that bring their own counts
    ("permutation: int8 whatever gram_path says, seven planes, no MICOM unless enabled", head(), call(600, PERMUTATION), dict(gram_path=1), dict(gpath=2, plane_floor=7, need_lists=0, micom=0, raises=0)),
    ("permutation with MICOM", head(micom_on=1), call(600, PERMUTATION), {}, dict(gpath=2, micom=1, micom_stride=20)),
    ("... not into a caller's records", head(micom_on=1), call(600, PERMUTATION, rows_out=1), {}, dict(micom=0)),
    ("... not on a handle with missing values", head(micom_on=1, n_ind=2), call(600, PERMUTATION), {}, dict(micom=0, rows_solver=0)),
    ("... not for a stratified call", head(micom_on=1), call(600, STRATIFIED), {}, dict(gpath=2, plane_floor=7, micom=0, raises=1)),
    ("... not for a plain bootstrap", head(micom_on=1), call(600), {}, dict(micom=0, plane_floor=0)),
    ("cross-validation", head(), call(512, CROSS_VALIDATION), dict(gram_path=1, i8_min_batch=1000), dict(gpath=2, plane_floor=7, rows_solver=1)),
    ("jackknife into records of its own", head(), call(600, JACKKNIFE, rows_out=1), dict(gram_path=1), dict(gpath=2, plane_floor=7, rows_solver=1, micom=0)),
    ("fewer than 128 rows raise the error word", head(127), call(600), {}, dict(raises=1, sub_batches=0)),
    ("128 rows do not", head(128), call(600), {}, dict(raises=0, sub_batches=1)),
    ("the stream-K schedule does", head(), call(600), dict(i8_sched=1), dict(raises=1, sub_batches=0)),
    # ---- no dense solver
    ("moments seam: packed matrices, no solver", head(), call(600, moments=1), {}, dict(gpath=2, rows_solver=0, dense=0, gram_bytes=20480, gram_budget_bytes=29768)),
    ("moments seam, Scale.NUM: no one-launch form", NUM, call(600, moments=1), {}, dict(gpath=2, counts8_plan=1, nm_wave=0, dense=0, verify_bytes=0)),
    ("moments seam, categorical: no uint16 output", CAT, call(600, moments=1), {}, dict(gpath=2, want16=0, cat_one=1)),
    ("missing-value indicators: the impute pass reads packed matrices", head(n_ind=3), call(5000), {}, dict(gpath=2, rows_solver=0, dense=0, psize=2560, gram_budget_bytes=64 * 65 * 8, gram_bytes=20480)),
    # ---- non-metric
    ("Scale.NUM with the int8 counts: one launch + verification", NUM, call(5000), {},
     dict(gpath=2, counts8_plan=1, counts8_possible=1, want_dcnt=0, need_lists=0, nm_wave=1, dense=1, rows_solver=0, cat_one=0, want16=0, sub_batches=0, verify_bytes=NUM_VERIFY, gram_bytes=29768,
          per_rep=29768 + 10112 + 59184, chunk=5000, passes=1)),
    ("Scale.NUM, nm_counts8 0: lists and uint16 histograms", NUM, call(5000), dict(nm_counts8=0),
     dict(gpath=2, counts8_plan=0, counts8_possible=0, want_dcnt=1, need_lists=1, nm_wave=0, dense=0, dcnt_stride=10000, dcnt_bytes=20000, verify_bytes=0, gram_bytes=20480, per_rep=80032 + 29768 + 20000 + 10112)),
    ("Scale.NUM, draws on a second stream: no counts8", NUM, call(5000), dict(resample_aux=1), dict(counts8_plan=0, want_dcnt=1, need_lists=1)),
    ("Scale.NUM, a second stream left over from an earlier call", NUM, call(5000), dict(aux_stream=1), dict(counts8_plan=0, want_dcnt=1)),
    ("Scale.NUM, nm_wave16 0: counts8 without the one-launch form", NUM, call(5000), dict(nm_wave16=0), dict(counts8_plan=1, nm_wave=0, dense=0, verify_bytes=0, per_rep=29768 + 10112)),
    ("Scale.NUM, conv_pass 1: no dense stop-rule pass, no counts8", NUM, call(5000), dict(conv_pass=1), dict(counts8_plan=0, counts8_possible=0, need_lists=1, nm_wave=0)),
    ("Scale.NUM on the fp64 route", NUM, call(5000), dict(gram_path=1), dict(gpath=1, counts8_plan=0, want_dcnt=1, need_lists=1, nm_wave=0, counts_bytes=0)),
    ("incomplete rows: lists", nonmetric_shape(nmr.num_shape([10] * 6, 2000, nmx_K=37)), call(600), {}, dict(gpath=2, counts8_plan=0, want_dcnt=1, need_lists=1, nm_wave=0)),
    ("categorical headline: one launch, the 16 GiB budget, uint16 counts from the Gram", CAT, call(5000), {},
     dict(gpath=2, counts8_plan=1, cat_one=1, want16=1, nm_wave=0, dense=0, need_lists=0, psize=53760, gram_budget_bytes=724808, gram_bytes=430080, verify_bytes=CAT_VERIFY, gk16_stride=301 * 304,
          gk16_bytes=183008, per_rep=724808 + 10112 + 337040, budget=16 * GiB, chunk=5000, passes=1)),
    ("categorical headline, B 20,000: 16,026 fit -> 62 tiles of 256", CAT, call(20000), {}, dict(budget=16 * GiB, chunk=15872, passes=2)),
    ("categorical, nm_cat_one 0: the 2 GiB budget", CAT, call(20000), dict(nm_cat_one=0), dict(cat_one=0, want16=1, verify_bytes=0, per_rep=724808 + 10112, budget=2 * GiB, chunk=2816, passes=8)),
    ("categorical, nm_direct16 0", CAT, call(5000), dict(nm_direct16=0), dict(want16=0, gk16_bytes=0, cat_one=1)),
    ("a HOC pair: counts8 when both stages have a dense pass, no uint16 output", HOC, call(600), {}, dict(gpath=2, counts8_plan=1, counts8_possible=1, want16=0, nm_wave=0, need_lists=0)),
    ("a HOC pair whose second stage has no dense pass", dict(HOC, nm2=dict(HOC["nm2"], kb=200, P1=1500)), call(600), {}, dict(gpath=2, counts8_plan=0, counts8_possible=0, want_dcnt=1, need_lists=1)),
]

NB = 512
# (id, shape, call, options, pass, expected)
CHUNKS = [
    ("no fallback: the dense solver", head(), call(5000, explicit_idx=1), {}, dict(nb=NB), dict(f64_gram=0, counts8=0, build_lists=0, lists=1, dense_solver=1, route=WAVE16_8, solve=SOLVE_METRIC)),
    ("fallback with explicit indices: lists, fp64 Gram, the LDS solver", head(), call(5000, explicit_idx=1), {}, dict(nb=NB, fell_back=1), dict(f64_gram=1, build_lists=1, dense_solver=0, route=LDS, solve=SOLVE_METRIC)),
    ("Philox draws", head(), call(5000), {}, dict(nb=NB), dict(f64_gram=0, build_lists=0, lists=0, dense_solver=1, route=WAVE16_8, solve=SOLVE_METRIC, call=(0,) * 5)),
    ("fp64 route", head(), call(5000), dict(gram_path=1), dict(nb=NB), dict(f64_gram=1, build_lists=1, lists=1, dense_solver=0, route=LDS, solve=SOLVE_METRIC)),
    ("moments seam", head(), call(5000, moments=1), {}, dict(nb=NB), dict(f64_gram=0, dense_solver=0, solve=SOLVE_MOMENTS)),
    ("Scale.NUM with counts8: one launch", NUM, call(5000), {}, dict(nb=NB), dict(counts8=1, build_lists=0, lists=0, solve=SOLVE_NM_WAVE, call=(NB, 1, 0, 0, 1))),
    ("non-metric with counts8 off: lists + uint16 histograms", NUM, call(5000), dict(nm_counts8=0), dict(nb=NB), dict(f64_gram=0, counts8=0, build_lists=1, lists=1, solve=SOLVE_NONMETRIC, call=(NB, 0, 1, 0, 1))),
    ("Scale.NUM beyond one window, explicit indices fell back: lists without uint16 histograms", nonmetric_shape(nmr.num_shape([10] * 6, 65536)), call(600, explicit_idx=1), {}, dict(nb=NB, fell_back=1),
     dict(f64_gram=1, counts8=0, build_lists=1, lists=1, solve=SOLVE_NONMETRIC, call=(NB, 0, 0, 0, 1))),
    ("... and did not: the one launch", nonmetric_shape(nmr.num_shape([10] * 6, 65536)), call(600, explicit_idx=1), {}, dict(nb=NB), dict(f64_gram=0, counts8=1, build_lists=0, lists=0, solve=SOLVE_NM_WAVE)),
    ("wrote16: the Gram left uint16 counts", CAT, call(5000), {}, dict(nb=NB, wrote16=1), dict(counts8=1, build_lists=0, lists=0, solve=SOLVE_NONMETRIC, call=(NB, 1, 0, 1, 1))),
    ("categorical, planes that are not 0/1: fp64 slots", CAT, call(5000), {}, dict(nb=NB), dict(counts8=1, solve=SOLVE_NONMETRIC, call=(NB, 1, 0, 0, 1))),
    ("a HOC pair: stage 1 without records, stage 2 with", HOC, call(600), {}, dict(nb=NB), dict(counts8=1, lists=0, solve=SOLVE_HOC, call=(NB, 1, 0, 0, 0), call2=(NB, 1, 0, 0, 1))),
    ("a HOC pair on lists", HOC, call(600), dict(nm_counts8=0), dict(nb=NB), dict(counts8=0, build_lists=1, lists=1, solve=SOLVE_HOC, call=(NB, 0, 1, 0, 0), call2=(NB, 0, 1, 0, 1))),
]


@pytest.mark.parametrize("shape,cl,opts,expected", [c[1:] for c in PLANS], ids=[c[0] for c in PLANS])
def test_batch_plan(emu, shape, cl, opts, expected):
    got = plan(emu, shape, cl, **opts)
    assert {k: got[k] for k in expected} == expected
    # what holds for every call: the budget is the sum of its parts, the passes cover the batch, nothing is sized for a buffer nobody fills
    B = int(cl[0])
    assert got["per_rep"] == sum(got[k] for k in BUDGETED) and got["gram_bytes"] <= got["gram_budget_bytes"]
    assert got["chunk"] >= 1 and got["passes"] * got["chunk"] >= B and (got["passes"] - 1) * got["chunk"] < B
    rounded = max(256, got["budget"] // got["per_rep"] // 256 * 256)
    assert got["chunk"] <= B or got["chunk"] == rounded
    assert got["chunk"] == B or got["gpath"] == 1 or got["chunk"] % 256 == 0
    assert not got["need_ghist"] or got["need_lists"]
    assert not got["want_dcnt"] or (shape["nonmetric"] and got["lds_hist"])
    assert not got["nm_wave"] or (got["dense"] and got["counts8_plan"] and not got["rows_solver"] and shape["nonmetric"])
    assert got["sub_batches"] == (not shape["nonmetric"] and not got["raises"])


@pytest.mark.parametrize("shape,cl,opts,ps,expected", [c[1:] for c in CHUNKS], ids=[c[0] for c in CHUNKS])
def test_batch_chunk(emu, shape, cl, opts, ps, expected):
    got = chunk(emu, shape, cl, **ps, **opts)
    assert {k: got[k] for k in expected} == expected
    # lists are read only where they were reserved; a pass on the fp64 Gram has neither int8 counts nor a dense solver
    p = plan(emu, shape, cl, **opts)
    assert not got["lists"] or p["need_lists"]
    assert not got["build_lists"] or p["need_lists"]
    assert not got["f64_gram"] or not (got["counts8"] or got["dense_solver"])


def test_every_arrangement_has_a_row():
    assert {c[5]["solve"] for c in CHUNKS} == {SOLVE_MOMENTS, SOLVE_HOC, SOLVE_NM_WAVE, SOLVE_NONMETRIC, SOLVE_METRIC}


def test_shapes_of_the_table():
    assert (head()["T"], tiles_for(60, True), CAT["T"], CAT["P"], WIDE["P"]) == (4, 4, 20, 300, 2400)
    assert (HOC["has_stage2"], HOC["nm"]["has_stage2"], ATTACHED["has_stage1"]) == (1, 1, 1)
    assert tiles_for(200, False) == 13 and tiles_for(200, True) == 14      # (metric models may run an odd tile count)
