"""CPU check of the bootstrap solver routes (csrc/solver_route.h: metric_batch_route / nm_wave_route, the codes get_option("last_solver")
reports) through the emulation build in tests/hostemu/: an explicit table of model shapes at the edges of every solver's class.  The model's
shape is derived from (block sizes, modes, path) as plspm_model_create does (csrc/plspm_hip.hip); the expected codes are the ones the GPU
tests observe for the same shapes (test_gpu_solver_wave.py, test_gpu_solver_quad.py, test_gpu_nmwave.py)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import plspm_oracle as orc
from helpers import effect_pairs
from test_solver_hostemu import EMU

LDS, ROWS, WAVE, ROWS_SPLIT, QUAD, WAVE16_16, WAVE16_8, WAVE16_32 = 1, 2, 3, 4, 5, 6, 7, 8
NONE, NM_WAVE_8, NM_WAVE_16, NM_WAVE_32 = 0, 9, 10, 11


@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-s", "-C", EMU, "libplspm_hostemu.so"])
    return ctypes.CDLL(os.path.join(EMU, "libplspm_hostemu.so"))


def dag(L, fan):
    """Every LV's `fan` nearest predecessors (kmax = min(fan, L - 1))."""
    C = np.zeros((L, L), dtype=np.int64)
    for i in range(1, L):
        C[i, max(0, i - fan):i] = 1
    return C


def shape(sizes, modes, C):
    """(P, L, kmax, n_chol, n_eff, nedge, boff) as plspm_model_create derives them."""
    L = len(sizes)
    boff = np.concatenate(([0], np.cumsum(sizes))).astype(np.int32)
    npred = C.sum(axis=1)
    n_chol = sum(2 * k * k for k, m in zip(sizes, modes) if m == "B")
    reach = C.astype(bool)
    for k in range(L):
        reach = reach | (reach[:, k:k + 1] & reach[k:k + 1, :])
    return int(boff[-1]), L, int(npred.max()), n_chol, int(reach.sum() - np.trace(reach)), int(npred.sum()), boff


def route(lib, sizes, modes, C, solver_wave=1, solver_quad=1, solver_rows=1, nm=False):
    P, L, kmax, n_chol, n_eff, nedge, boff = shape(sizes, modes, C)
    return lib.hostemu_solver_route(P, L, kmax, n_chol, n_eff, nedge, boff.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), solver_wave, solver_quad,
                                    solver_rows, int(nm))


SAT = orc.satisfaction_C()
# (id, block sizes, modes, path, options, expected metric route)
METRIC = [
    ("headline", [10] * 6, "A" * 6, SAT, {}, WAVE16_8),
    ("headline wave 2", [10] * 6, "A" * 6, SAT, {"solver_wave": 2}, WAVE16_8),
    ("headline wave 3", [10] * 6, "A" * 6, SAT, {"solver_wave": 3}, WAVE),
    ("headline wave 0", [10] * 6, "A" * 6, SAT, {"solver_wave": 0}, ROWS),
    ("headline quad 0", [10] * 6, "A" * 6, SAT, {"solver_quad": 0}, WAVE16_8),
    ("headline rows 0", [10] * 6, "A" * 6, SAT, {"solver_rows": 0}, LDS),
    ("headline mode B", [10] * 6, "ABABAB", SAT, {}, WAVE16_8),
    ("headline mode B wave 3", [10] * 6, "ABABAB", SAT, {"solver_wave": 3}, WAVE),
    ("P 64", [8] * 8, "A" * 8, orc.chain_C(8), {}, WAVE16_8),
    ("P 65", [8] * 7 + [9], "A" * 8, orc.chain_C(8), {}, QUAD),
    ("P 65 quad 0", [8] * 7 + [9], "A" * 8, orc.chain_C(8), {"solver_quad": 0}, ROWS_SPLIT),
    ("P 65 wave 0", [8] * 7 + [9], "A" * 8, orc.chain_C(8), {"solver_wave": 0}, QUAD),
    ("P 65 rows 0", [8] * 7 + [9], "A" * 8, orc.chain_C(8), {"solver_rows": 0}, LDS),
    ("L 8", [3] * 8, "A" * 8, orc.chain_C(8), {}, WAVE16_8),
    ("L 9", [3] * 9, "A" * 9, orc.chain_C(9), {}, WAVE16_16),
    ("L 9 wave 0", [3] * 9, "A" * 9, orc.chain_C(9), {"solver_wave": 0}, ROWS),
    ("L 9 mode B", [3] * 9, "B" * 9, orc.chain_C(9), {}, WAVE16_16),
    ("L 16", [3] * 16, "A" * 16, orc.chain_C(16), {}, WAVE16_16),
    ("L 17", [3] * 17, "A" * 17, orc.chain_C(17), {}, WAVE16_32),
    ("L 17 mode B", [3] * 17, "A" * 16 + "B", orc.chain_C(17), {}, ROWS),
    ("L 32", [2] * 32, "A" * 32, orc.chain_C(32), {}, WAVE16_32),
    ("L 32 wave 0: rows workspace beyond kMaxLds / 4", [2] * 32, "A" * 32, orc.chain_C(32), {"solver_wave": 0}, LDS),
    ("L 33", [1] * 33, "A" * 33, orc.chain_C(33), {}, LDS),
    ("two Mode-B blocks of 30: inverses beyond the wave workspace", [30, 30], "BB", orc.chain_C(2), {}, ROWS),
    # the 20 KB workspace of solver_wave16_kernel<8>, crossed through the Mode-B factors ...
    ("Mode-B block of 31", [31] + [1] * 7, "B" + "A" * 7, orc.chain_C(8), {}, WAVE16_8),
    ("Mode-B block of 32", [32] + [1] * 7, "B" + "A" * 7, orc.chain_C(8), {}, WAVE),
    ("Mode-B block of 33", [33] + [1] * 7, "B" + "A" * 7, orc.chain_C(8), {}, ROWS),
    # ... and through kmax
    ("Mode-B block of 26, kmax 4", [26] + [1] * 7, "B" + "A" * 7, dag(8, 4), {}, WAVE16_8),
    ("Mode-B block of 26, kmax 5", [26] + [1] * 7, "B" + "A" * 7, dag(8, 5), {}, WAVE),
    # the 80 KB workspace of solver_quad_kernel<16> (kmax), and the split rows solver's kMaxLds / 2
    ("quad kmax 10", [5] * 16, "A" * 16, dag(16, 10), {}, QUAD),
    ("quad kmax 11", [5] * 16, "A" * 16, dag(16, 11), {}, LDS),
    ("split kmax 6", [5] * 16, "A" * 16, dag(16, 6), {"solver_quad": 0}, ROWS_SPLIT),
    ("split kmax 7", [5] * 16, "A" * 16, dag(16, 7), {"solver_quad": 0}, LDS),
    ("P 128", [8] * 16, "A" * 16, dag(16, 1), {}, QUAD),
    ("P 130", [13] * 10, "A" * 10, orc.chain_C(10), {}, LDS),
    ("P 120 x 12 LVs", [10] * 12, "A" * 12, orc.chain_C(12), {}, QUAD),
    ("P 90 mode B", [30, 20, 30], "ABA", orc.chain_C(3), {}, ROWS_SPLIT),
    ("P 85 x 17 LVs", [5] * 17, "A" * 17, orc.chain_C(17), {}, ROWS_SPLIT),
    ("P 70 no block boundary at or below 64", [66, 4], "AA", orc.chain_C(2), {}, LDS),
]

# (id, block sizes, modes, path, expected Scale.NUM / RAW route)
NM = [
    ("headline", [10] * 6, "A" * 6, SAT, NM_WAVE_8),
    ("headline mode B", [6] * 6, "ABABAB", SAT, NM_WAVE_8),
    ("L 2", [7, 7], "AA", orc.chain_C(2), NM_WAVE_8),
    ("L 10 mode B", [6] * 10, "ABBAABBAAB", orc.chain_C(10), NM_WAVE_16),
    ("L 12", [5] * 12, "A" * 12, orc.chain_C(12), NM_WAVE_16),
    ("L 17 mode B", [3] * 17, "A" * 16 + "B", orc.chain_C(17), NONE),
    ("L 20", [3] * 20, "A" * 20, orc.chain_C(20), NM_WAVE_32),
    ("L 32", [2] * 32, "A" * 32, orc.chain_C(32), NM_WAVE_32),
    ("L 33", [1] * 33, "A" * 33, orc.chain_C(33), NONE),
    ("P 65", [8] * 7 + [9], "A" * 8, orc.chain_C(8), NONE),
    ("two Mode-B blocks of 30", [30, 30], "BB", orc.chain_C(2), NONE),
    # (the non-metric form of <= 8 LVs takes 64 doubles more than the metric one: its 20 KB edge lies one block size lower)
    ("Mode-B block of 30", [30] + [1] * 7, "B" + "A" * 7, orc.chain_C(8), NM_WAVE_8),
    ("Mode-B block of 31", [31] + [1] * 7, "B" + "A" * 7, orc.chain_C(8), NONE),
    ("Mode-B block of 26, kmax 4", [26] + [1] * 7, "B" + "A" * 7, dag(8, 4), NM_WAVE_8),
    ("Mode-B block of 26, kmax 5", [26] + [1] * 7, "B" + "A" * 7, dag(8, 5), NONE),
]


@pytest.mark.parametrize("sizes,modes,C,opts,expected", [c[1:] for c in METRIC], ids=[c[0] for c in METRIC])
def test_metric_batch_route(emu, sizes, modes, C, opts, expected):
    assert route(emu, sizes, modes, C, **opts) == expected


@pytest.mark.parametrize("sizes,modes,C,expected", [c[1:] for c in NM], ids=[c[0] for c in NM])
def test_nm_wave_route(emu, sizes, modes, C, expected):
    assert route(emu, sizes, modes, C, nm=True) == expected


def test_shape_of_the_headline_model():
    P, L, kmax, n_chol, n_eff, nedge, boff = shape([10] * 6, "ABABAB", SAT)
    assert (P, L, kmax, n_chol, nedge) == (60, 6, SAT.sum(axis=1).max(), 3 * 2 * 10 * 10, SAT.sum())
    assert n_eff == len(effect_pairs(SAT)) and list(boff) == list(range(0, 61, 10))
