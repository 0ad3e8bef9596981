"""Shared by the CPU table test of the int8 Gram's launch plan (tests/test_gram_route.py) and the GPU test that ties the plan to what is launched
(tests/test_gpu_gram_i8.py): the plan through the emulation build in tests/hostemu/ (hostemu_gram_i8_plan), and what prepare_zs fixes for a data set."""
import ctypes
import os
import subprocess

import numpy as np

from test_solver_hostemu import EMU

PLAIN, IND, WIDE20, PRIV, PERSIST, SK, NARROW, SHAPE32 = range(8)
HIST16, HIST8, HIST4 = 0, 1, 2
OUT = ("form", "waves", "variant", "dma_buffer", "rt_tall", "rt_short", "nty_tall", "nty_short", "nty", "ntx", "MT", "per_xcd", "grid", "block", "pp_wgs", "sk_grid", "hist", "hist_bytes", "hist_windows", "hist_threads", "cd_bytes", "to16", "priv_takes", "round_units")
OPTS = ("priv", "persist", "rt", "short_rows", "cus", "dma", "nibbles", "waves", "shape", "sched", "variant")
DEFAULTS = dict(priv=1, persist=0, rt=0, short_rows=-1, cus=0, dma=0, nibbles=1, waves=8, shape=16, sched=0, variant=-1)


def load_emu():
    subprocess.check_call(["make", "-s", "-C", EMU, "libplspm_hostemu.so"])
    return ctypes.CDLL(os.path.join(EMU, "libplspm_hostemu.so"))


def data(S, N, mvs, ind=False):
    """What prepare_zs fixes for N rows x mvs columns (+ the ones column) at S digit planes."""
    npair = (mvs + 1) * (mvs + 2) // 2
    npg = (npair + 31) // 32 * 2
    if ind:
        npg = (npg + 13) // 14 * 14
    return dict(S=S, KB=(N + 127) // 128 * 2, NT=npg * S, npg=npg, zs_ind=int(ind))


def plan(lib, d, nb, cu_count=256, explicit_idx=0, own_counts=0, want16=0, experiments=0, **opts):
    dv = np.array([d[k] for k in ("S", "KB", "NT", "npg", "zs_ind")], dtype=np.int32)
    op = np.array([dict(DEFAULTS, **opts)[k] for k in OPTS], dtype=np.int32)
    cl = np.array([nb, explicit_idx, own_counts, want16, cu_count, experiments], dtype=np.int64)
    out = np.zeros(len(OUT), dtype=np.int64)
    lib.hostemu_gram_i8_plan(dv.ctypes.data_as(ctypes.c_void_p), op.ctypes.data_as(ctypes.c_void_p), cl.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p))
    return dict(zip(OUT, (int(v) for v in out)))
