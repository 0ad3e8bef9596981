"""Shared by the CPU table test of the batch driver's plan (tests/test_batch_route.py) and the GPU test that ties the plan to what runs (tests/test_gpu_passes.py):
the plan of a call and of a pass through the emulation build in tests/hostemu/ (hostemu_batch_plan, hostemu_batch_chunk), and the shape of a handle as
plspm_model_create and the upload derive it (csrc/host_internal.h batch_shape)."""
import ctypes

import numpy as np

import test_nm_route as nmr
from helpers_gram_route import load_emu  # noqa: F401  (the tests' fixture)
from test_solver_route import shape as route_shape

PLAIN, PERMUTATION, STRATIFIED, CROSS_VALIDATION, JACKKNIFE = range(5)
SOLVE_MOMENTS, SOLVE_HOC, SOLVE_NM_WAVE, SOLVE_NONMETRIC, SOLVE_METRIC = range(5)
GiB = 1 << 30
OUT = ("gpath", "plane_floor", "lds_hist", "counts8_plan", "want_dcnt", "route", "rows_solver", "nm_wave", "dense", "need_lists", "need_ghist", "cat_one", "want16", "micom", "raises",
       "ent_stride", "dcnt_stride", "psize", "gk16_stride", "micom_stride", "kpad", "ent_bytes", "gram_budget_bytes", "gram_bytes", "ghist_bytes", "dcnt_bytes", "counts_bytes",
       "verify_bytes", "nent_bytes", "gk16_bytes", "per_rep", "budget", "chunk", "passes", "closed", "counts_route_open", "counts8_possible", "sub_batches")
BUDGETED = ("ent_bytes", "gram_budget_bytes", "ghist_bytes", "dcnt_bytes", "counts_bytes", "verify_bytes")      # the parts of per_rep
CHUNK_OUT = ("f64_gram", "counts8", "build_lists", "lists", "dense_solver", "route", "solve", "call", "call2")
OPTS = ("gram_path", "i8_min_batch", "i8_slices", "nm_counts8", "resample_aux", "i8_shape", "i8_sched", "solver_wave", "solver_quad", "solver_rows", "boot_pass", "aux_stream")
DEFAULTS = dict(gram_path=0, i8_min_batch=1, i8_slices=0, nm_counts8=1, resample_aux=0, i8_shape=16, i8_sched=0, solver_wave=1, solver_quad=1, solver_rows=1, boot_pass=0, aux_stream=0)
SHAPE_KEYS = ("N", "P", "Pg", "T", "L", "R", "n_ind", "nonmetric", "has_stage1", "has_stage2", "micom_on", "plain_metric", "kmax", "n_chol", "n_eff", "nedge")


def tiles_for(cols, nonmetric):
    """16-column tiles of the resident matrix [columns | 1 | 0-pad] (csrc/plspm_hip.hip tiles_for)."""
    t16 = (cols + 1 + 15) // 16
    return t16 if not nonmetric and t16 % 2 and 5 <= t16 <= 15 else 2 * ((cols + 1 + 31) // 32)


def metric_shape(sizes, modes, C, N, n_ind=0, **kw):
    """A metric handle of N rows (n_ind missing-value indicator columns behind the data)."""
    P, L, kmax, n_chol, n_eff, nedge, boff = route_shape(sizes, modes, C)
    d = dict(N=N, P=P, Pg=P + n_ind, T=tiles_for(P + n_ind, False), L=L, R=0, n_ind=n_ind, nonmetric=0, has_stage1=0, has_stage2=0, micom_on=0, plain_metric=int(n_ind == 0),
             kmax=kmax, n_chol=n_chol, n_eff=n_eff, nedge=nedge, boff=boff, nm=None, nm2=None)
    d.update(kw)
    return d


def nonmetric_shape(nm, nm2=None, **kw):
    """A non-metric handle from its NmShape (test_nm_route.num_shape / cat_shape; all Mode A, a chain), nm2: the attached second stage of a HOC pair."""
    P, L = nm["P"], nm["L"]
    d = dict(N=nm["N"], P=P, Pg=P, T=tiles_for(P, True), L=L, R=0, n_ind=0, nonmetric=1, has_stage1=nm["attached"], has_stage2=int(nm2 is not None), micom_on=0, plain_metric=0,
             kmax=nm["kmax"], n_chol=nm["n_chol"], n_eff=nm["n_eff"], nedge=nm["nedge"], boff=np.zeros(L + 1, dtype=np.int32), nm=dict(nm, has_stage2=int(nm2 is not None)), nm2=nm2)
    d.update(kw)
    return d


def call(B, kind=PLAIN, explicit_idx=0, moments=0, rows_out=0):
    return np.array([B, kind != PLAIN, kind == PERMUTATION, kind == STRATIFIED, explicit_idx, moments, rows_out], dtype=np.int64)


def _inputs(shape, cl, opts):
    unknown = set(opts) - set(OPTS) - set(nmr.OPTS)
    assert not unknown, unknown
    blank = nmr.num_shape([1], 2)
    arrays = [np.array([shape[k] for k in SHAPE_KEYS], dtype=np.int64), np.ascontiguousarray(shape["boff"], dtype=np.int32),
              np.array([(shape["nm"] or blank)[k] for k in nmr.SHAPE_KEYS], dtype=np.int64), np.array([(shape["nm2"] or blank)[k] for k in nmr.SHAPE_KEYS], dtype=np.int64),
              np.array([dict(DEFAULTS, **opts)[k] for k in OPTS], dtype=np.int32)]
    nm_opts = np.array([dict(nmr.DEFAULTS, **opts)[k] for k in nmr.OPTS], dtype=np.int32)      # (both stages of a pair under the same options)
    return arrays + [nm_opts, nm_opts, cl]


def _run(fn, arrays, n_out):
    out = np.zeros(n_out, dtype=np.int64)
    fn(*[a.ctypes.data_as(ctypes.c_void_p) for a in arrays], out.ctypes.data_as(ctypes.c_void_p))
    return [int(v) for v in out]


def plan(lib, shape, cl, **opts):
    """batch_plan of the call `cl` (call(...)) on `shape` under the driver's and the non-metric options named in opts."""
    return dict(zip(OUT, _run(lib.hostemu_batch_plan, _inputs(shape, cl, opts), len(OUT))))


def chunk(lib, shape, cl, nb, fell_back=0, wrote16=0, **opts):
    """batch_chunk of a pass of nb problems of that call; call / call2: (nproblems, counts8, lists_dcnt, counts16_ready, finish)."""
    v = _run(lib.hostemu_batch_chunk, _inputs(shape, cl, opts) + [np.array([nb, fell_back, wrote16], dtype=np.int64)], 17)
    return dict(zip(CHUNK_OUT, v[:7] + [tuple(v[7:12]), tuple(v[12:17])]))
