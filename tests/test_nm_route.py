"""CPU check of the non-metric route plan (csrc/nm_route.h nm_plan: stop-rule pass, step kernel, one-launch forms) through the emulation build in
tests/hostemu/: an explicit table of model shapes at the edges of every route.  The shape is derived from (categories per item, items per LV) as
plspm_model_set_categorical does (one indicator column per category); the expected flags are what the GPU tests observe through get_option("last_nm_*")
for the same shapes (test_gpu_categorical.py, test_gpu_nmwave.py, test_gpu_hoc.py, test_gpu_fuzz.py, test_gpu_parity.py)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from test_solver_hostemu import EMU

OUT = ("error", "dense", "dense_whole", "use_codes", "use_mfma", "flag_from_list", "k16", "wave_step", "bound_ok", "sub_pass", "one_launch", "lmax", "cmax", "cpl",
       "num_one", "direct16", "KS", "tpc", "nparts", "nsub", "cat_fast")
OPTS = ("conv_pass", "conv_gy", "nm_k16", "nm_wave", "nm_codes", "nm_mfma", "nm_subset", "nm_cat_one", "nm_cpl", "nm_c10", "nm_fast_lds", "nm_wave16", "nm_direct16")
DEFAULTS = dict(conv_pass=0, conv_gy=0, nm_k16=1, nm_wave=1, nm_codes=1, nm_mfma=1, nm_subset=4, nm_cat_one=1, nm_cpl=0, nm_c10=1, nm_fast_lds=1, nm_wave16=1,
                nm_direct16=1)


@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-s", "-C", EMU, "libplspm_hostemu.so"])
    return ctypes.CDLL(os.path.join(EMU, "libplspm_hostemu.so"))


def cat_shape(lvs, N, **kw):
    """An all-ORD / NOM chain model: lvs = per LV the category counts of its items."""
    L, cats = len(lvs), [c for lv in lvs for c in lv]
    P = sum(cats)
    d = dict(P=P, P1=P, Pm=len(cats), L=L, kmax=1, n_chol=0, n_eff=L * (L - 1) // 2, nedge=L - 1, cmax=max(cats), kmv=max(len(lv) for lv in lvs), kb=max(sum(lv) for lv in lvs),
             max_iter=100, N=N, nmx_K=0, nonmetric=1, categorical=1, cat_pure=1, src_cat_pure=1, all_mode_a=1, attached=0, has_stage2=0, has_ind=0, codes_tables=1)
    d.update(kw)
    return d


def num_shape(sizes, N, **kw):
    """A Scale.NUM chain model, all Mode A."""
    L, P = len(sizes), sum(sizes)
    d = dict(P=P, P1=P, Pm=0, L=L, kmax=1, n_chol=0, n_eff=L * (L - 1) // 2, nedge=L - 1, cmax=1, kmv=1, kb=max(sizes), max_iter=100, N=N, nmx_K=0, nonmetric=1, categorical=0,
             cat_pure=0, src_cat_pure=0, all_mode_a=1, attached=0, has_stage2=0, has_ind=0, codes_tables=0)
    d.update(kw)
    return d


SHAPE_KEYS = ("P", "P1", "Pm", "L", "kmax", "n_chol", "n_eff", "nedge", "cmax", "kmv", "kb", "max_iter", "N", "nmx_K", "nonmetric", "categorical", "cat_pure", "src_cat_pure",
              "all_mode_a", "attached", "has_stage2", "has_ind", "codes_tables")
BOOT = dict(nproblems=5000, counts8=1, lists_dcnt=0, counts16_ready=0, finish=1)      # a bootstrap batch on the int8 Gram with on-device draws
LISTS = dict(nproblems=5000, counts8=0, lists_dcnt=1, counts16_ready=0, finish=1)     # ... with explicit indices / on the fp64 Gram: (row,count) lists + uint16 histograms
FIT = dict(nproblems=1, counts8=0, lists_dcnt=0, counts16_ready=0, finish=1)


def plan(lib, shape, call, **opts):
    sh = np.array([shape[k] for k in SHAPE_KEYS], dtype=np.int64)
    cl = np.array([call[k] for k in ("nproblems", "counts8", "lists_dcnt", "counts16_ready", "finish")], dtype=np.int64)
    op = np.array([dict(DEFAULTS, **opts)[k] for k in OPTS], dtype=np.int32)
    out = np.zeros(len(OUT), dtype=np.int64)
    lib.hostemu_nm_plan(sh.ctypes.data_as(ctypes.c_void_p), cl.ctypes.data_as(ctypes.c_void_p), op.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p))
    return dict(zip(OUT, (int(v) for v in out)))


HEAD = cat_shape([[5] * 10] * 6, 10000)        # tools/categorical_bench.py: 10,000 rows x 60 five-point items x 6 LVs
ONE = dict(error=0, dense=1, use_codes=1, use_mfma=1, flag_from_list=1, wave_step=1, sub_pass=1, one_launch=1, num_one=0, direct16=1)
# (id, shape, call, options, expected)
CASES = [
    ("categorical headline", HEAD, BOOT, {}, dict(ONE, lmax=6, cmax=8, cpl=6, KS=1, nsub=4)),
    ("headline with the Gram's uint16 counts", HEAD, dict(BOOT, counts16_ready=1), {}, dict(ONE, error=0)),
    ("headline single fit: gathering pass, wave step", HEAD, FIT, {}, dict(error=0, dense=0, use_codes=0, use_mfma=0, flag_from_list=0, wave_step=1, sub_pass=0, one_launch=0, nparts=10, nsub=0)),
    ("headline on lists: dense pass on fp64 columns", HEAD, LISTS, {}, dict(dense=1, use_codes=0, use_mfma=0, wave_step=1, one_launch=0, sub_pass=0)),
    ("nm_wave 0", HEAD, BOOT, {"nm_wave": 0}, dict(wave_step=0, use_mfma=1, one_launch=0, sub_pass=0, direct16=0)),
    ("nm_wave 0 with uint16 counts is refused", HEAD, dict(BOOT, counts16_ready=1), {"nm_wave": 0}, dict(error=2)),
    ("nm_mfma 0", HEAD, BOOT, {"nm_mfma": 0}, dict(use_codes=1, use_mfma=0, wave_step=1, one_launch=0, sub_pass=0)),
    ("nm_codes 0", HEAD, BOOT, {"nm_codes": 0}, dict(dense=1, use_codes=0, use_mfma=0, wave_step=1, one_launch=0)),
    ("nm_subset 0", HEAD, BOOT, {"nm_subset": 0}, dict(use_mfma=1, wave_step=1, one_launch=0, sub_pass=0, nsub=0, direct16=1)),
    ("nm_subset 1", HEAD, BOOT, {"nm_subset": 1}, dict(one_launch=1, nsub=1)),
    ("nm_cat_one 0", HEAD, BOOT, {"nm_cat_one": 0}, dict(use_mfma=1, wave_step=1, one_launch=0, sub_pass=1, nsub=4)),
    ("nm_k16 0", HEAD, BOOT, {"nm_k16": 0}, dict(k16=0, wave_step=0, use_mfma=1, one_launch=0)),
    ("nm_direct16 0", HEAD, BOOT, {"nm_direct16": 0}, dict(direct16=0, wave_step=1, one_launch=1)),
    ("conv_pass 1: no dense pass for the int8 counts", HEAD, BOOT, {"conv_pass": 1}, dict(error=1, dense=0)),
    ("conv_pass 2: one LV block at a time", HEAD, LISTS, {"conv_pass": 2}, dict(dense=1, dense_whole=0)),
    ("a few hundred rows: one launch, else no row subsets", cat_shape([[5] * 6] * 6, 300), BOOT, {}, dict(one_launch=1, sub_pass=1)),
    ("a few hundred rows, nm_cat_one 0", cat_shape([[5] * 6] * 6, 300), BOOT, {"nm_cat_one": 0}, dict(one_launch=0, sub_pass=0, wave_step=1)),
    ("N 1023, nm_cat_one 0", cat_shape([[5] * 6] * 6, 1023), BOOT, {"nm_cat_one": 0}, dict(sub_pass=0)),
    ("N 1024, nm_cat_one 0", cat_shape([[5] * 6] * 6, 1024), BOOT, {"nm_cat_one": 0}, dict(sub_pass=1)),
    ("eight categories, 2 LVs", cat_shape([[8] * 6] * 2, 2500), BOOT, {}, dict(wave_step=1, lmax=2, cmax=8, cpl=6)),
    ("nine- and ten-category items", cat_shape([[10, 9, 10, 10]] * 2, 2500), BOOT, {}, dict(wave_step=1, lmax=2, cmax=10, cpl=6)),
    ("ten-category items, nm_c10 0", cat_shape([[10, 9, 10, 10]] * 2, 2500), BOOT, {"nm_c10": 0}, dict(wave_step=1, lmax=2, cmax=16, cpl=6)),
    ("ten-category items, nm_cpl 8", cat_shape([[10, 9, 10, 10]] * 2, 2500), BOOT, {"nm_cpl": 8}, dict(wave_step=1, cmax=16, cpl=8)),
    ("sixteen-category items", cat_shape([[16, 9, 16, 16]] * 2, 2500), BOOT, {}, dict(wave_step=1, lmax=2, cmax=16, cpl=8)),
    ("seventeen categories: no wave step", cat_shape([[17, 5, 5, 5]] * 2, 2500), BOOT, {}, dict(wave_step=0, one_launch=0, use_mfma=1)),
    ("6 LVs x 12 categories: six columns per lane", cat_shape([[12, 5, 5]] * 6, 3000), BOOT, {}, dict(wave_step=1, lmax=6, cmax=16, cpl=6)),
    ("7 LVs x 12 categories: eight columns per lane", cat_shape([[12, 5, 5]] * 7, 3000), BOOT, {}, dict(wave_step=1, lmax=8, cmax=16, cpl=8)),
    ("7 LVs x 12 categories, single fit", cat_shape([[12, 5, 5]] * 7, 3000), FIT, {}, dict(wave_step=1, lmax=8, cmax=16, cpl=8, one_launch=0)),
    ("7 LVs x 10 categories", cat_shape([[10, 5, 5]] * 7, 3000), BOOT, {}, dict(wave_step=1, lmax=8, cmax=10, cpl=6)),
    ("9 LVs: no wave step", cat_shape([[5] * 4] * 9, 3000), BOOT, {}, dict(wave_step=0, one_launch=0, use_mfma=1)),
    ("383 aug columns", cat_shape([[8] * 47 + [7]], 3000), BOOT, {}, dict(wave_step=1, cpl=6, use_mfma=0)),
    ("384 aug columns", cat_shape([[8] * 48], 3000), BOOT, {}, dict(wave_step=1, cpl=8)),
    ("511 aug columns", cat_shape([[8] * 63 + [7]], 3000), BOOT, {}, dict(wave_step=1)),
    ("512 aug columns", cat_shape([[8] * 64], 3000), BOOT, {}, dict(wave_step=0)),
    ("N 65535", cat_shape([[4] * 4] * 3, 65535), BOOT, {}, dict(k16=1, wave_step=1, use_codes=1, one_launch=1)),
    ("N 65536: no uint16 counts", cat_shape([[4] * 4] * 3, 65536), BOOT, {}, dict(k16=0, wave_step=0, use_codes=1, use_mfma=1, one_launch=0, direct16=0)),
    ("block of 64 columns", cat_shape([[4] * 16, [4] * 5], 3000), BOOT, {}, dict(use_mfma=1, KS=1, one_launch=1)),
    ("block of 65 columns", cat_shape([[4] * 15 + [5], [4] * 5], 3000), BOOT, {}, dict(use_mfma=1, KS=2, one_launch=1)),
    ("block of 128 columns", cat_shape([[4] * 32, [4] * 5], 3000), BOOT, {}, dict(use_codes=1, use_mfma=1, KS=2, wave_step=1, one_launch=1)),
    ("block of 129 columns: codes pass, launch by launch", cat_shape([[3] * 43, [3] * 5], 3000), BOOT, {}, dict(use_codes=1, use_mfma=0, wave_step=1, one_launch=0, sub_pass=0)),
    # (a block of 160 columns: neither the whole coefficient tile, 389 x 64 doubles, nor one block of it, (2 x 160 + 2) x 64 doubles = 164,864 bytes, fits the 163,840
    #  bytes of LDS -- no dense pass, so the bootstrap may not count on the Gram's int8 counts, nm_counts8_possible, and takes the gathering pass on lists)
    ("20 items of 8 categories under one LV: int8 counts refused", cat_shape([[8] * 20, [8] * 4], 3000), BOOT, {}, dict(error=1, dense=0, one_launch=0)),
    ("20 items of 8 categories under one LV: gathering pass", cat_shape([[8] * 20, [8] * 4], 3000), LISTS, {}, dict(error=0, dense=0, use_codes=0, wave_step=1, one_launch=0, nparts=3)),
    ("64 MVs", cat_shape([[3] * 32] * 2, 3000), BOOT, {}, dict(wave_step=1, one_launch=1)),
    ("65 MVs", cat_shape([[3] * 32, [3] * 33], 3000), BOOT, {}, dict(wave_step=0, one_launch=0, use_mfma=1)),
    ("a Mode-B block", cat_shape([[5] * 4] * 3, 3000, all_mode_a=0, n_chol=800), BOOT, {}, dict(wave_step=0, one_launch=0, use_mfma=1)),
    ("mixed ORD / NUM items", cat_shape([[5] * 4] * 3, 3000, cat_pure=0, src_cat_pure=0), BOOT, {}, dict(dense=1, use_codes=0, use_mfma=0, k16=0, wave_step=0, one_launch=0)),
    ("first stage of a HOC pair", cat_shape([[5] * 4] * 4, 3000, has_stage2=1), dict(BOOT, finish=0), {}, dict(use_mfma=1, wave_step=1, one_launch=1, direct16=0)),
    ("attached second stage", cat_shape([[5] * 4, [1] * 3], 3000, attached=1, P1=80, kb=60), BOOT, {}, dict(use_codes=1, use_mfma=1, flag_from_list=0, bound_ok=0, sub_pass=0, one_launch=0, direct16=0)),
    ("attached second stage, nm_mfma 0", cat_shape([[5] * 4, [1] * 3], 3000, attached=1, P1=80, kb=60), BOOT, {"nm_mfma": 0}, dict(use_codes=1, use_mfma=0, one_launch=0)),
    ("attached second stage, nm_codes 0", cat_shape([[5] * 4, [1] * 3], 3000, attached=1, P1=80, kb=60), BOOT, {"nm_codes": 0}, dict(dense=1, use_codes=0, use_mfma=0)),
    ("Scale.NUM with int8 counts: one launch + verification", num_shape([10] * 6, 10000), BOOT, {}, dict(error=0, dense=1, dense_whole=1, use_codes=0, wave_step=0, one_launch=0, num_one=1)),
    ("Scale.NUM on lists", num_shape([10] * 6, 10000), LISTS, {}, dict(dense=1, flag_from_list=1, num_one=0)),
    ("Scale.NUM, nm_wave16 0", num_shape([10] * 6, 10000), BOOT, {"nm_wave16": 0}, dict(dense=1, num_one=0)),
    ("Scale.NUM, 65 MVs", num_shape([8] * 7 + [9], 10000), BOOT, {}, dict(dense=1, num_one=0)),
    ("Scale.NUM, first stage of a pair", num_shape([10] * 6, 10000, has_stage2=1), BOOT, {}, dict(dense=1, num_one=0)),
    ("Scale.NUM single fit", num_shape([10] * 6, 10000), FIT, {}, dict(dense=0, nparts=10, num_one=0, wave_step=0)),
    ("missing values: lists, the launch-by-launch solver", num_shape([10] * 6, 2000, nmx_K=37), LISTS, {}, dict(error=0, dense=1, use_codes=0, wave_step=0, num_one=0, one_launch=0)),
    ("missing values, single fit", num_shape([10] * 6, 2000, nmx_K=37), FIT, {}, dict(dense=0, nparts=2, num_one=0)),
]


@pytest.mark.parametrize("shape,call,opts,expected", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_nm_plan(emu, shape, call, opts, expected):
    got = plan(emu, shape, call, **opts)
    assert {k: got[k] for k in expected} == expected


def test_shape_of_the_categorical_headline():
    assert (HEAD["P"], HEAD["Pm"], HEAD["L"], HEAD["cmax"], HEAD["kmv"], HEAD["kb"]) == (300, 60, 6, 5, 10, 50)
