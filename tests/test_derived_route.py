"""CPU check of the plan of the derived records (csrc/derived_route.h: the stage table, derived_plan, derived_fit_layout) through the emulation build in tests/hostemu/:
an explicit table with a row for every decision plspm_derived.hip used to make inline -- which stages run, their record pitch, the waves and the LDS of their
workgroups, the structural stage's regression slots, the hand-over to PLSc, what the LDS refuses, the layout of the full-sample block -- and their edges.  The expected
values are worked out by hand from the formulas the unit and the kernels' workspace functions carried before the plan had a function of its own:

    stages, in launch order (bit):  assessment (1), structural (2), PLSc (4), model fit (8), geodesic (16);  PLSc and structural read the assessment, model fit reads
                                    PLSc, geodesic reads model fit and PLSc;  what runs = the switches and everything they read
    width:  4 L + 3 L (L - 1) / 2  |  2 n_dir + n_spec  |  R + L (L - 1) / 2  |  4  |  2;   stride = width + 2
    one wave's doubles:  4 P + 7 L + 192  |  L^2 + L + 8 + nslots slot  |  P + 4 L^2 + 3 L + 8 + L reg  |  3 P + 2 L^2 + 8  |  model fit's + P (P + 1) + 4 P
                         reg = 2 kmax^2 + kmax,  slot = reg + (kmax + 1) // 2
    waves:  4;  geodesic min(4, 20480 // doubles), at least 1, refused when one wave's doubles exceed 20480 (160 KiB);  structural 4, 2 or 1: the first w with
            fit = (20480 // w - (L^2 + L + 8)) // slot >= 1, nslots = min(fit, 64, max(L, n_dir)), refused when there is none
    lds = 8 waves doubles;  grid = ceil(nb / waves);  side = 24 L nb bytes where PLSc runs
    full-sample block, in doubles:  R + 2 | the running stages' strides in launch order | 3 L where PLSc runs | two ints
"""
import ctypes

import numpy as np
import pytest

from helpers_gram_route import load_emu

ASSESS, STRUCTURAL, PLSC, MODELFIT, GEODESIC = range(5)
NAMES = ("assess", "structural", "plsc", "modelfit", "geodesic")
FIELDS = ("stride", "waves", "wave_doubles", "lds", "grid")


@pytest.fixture(scope="module")
def emu():
    lib = load_emu()
    lib.hostemu_derived_word.restype = ctypes.c_char_p
    return lib


def shape(P, L, kmax, n_eff, n_dir=0, n_spec=0):
    return dict(P=P, L=L, kmax=kmax, R=2 * P + L + 2 * n_eff, n_dir=n_dir, n_spec=n_spec)


def plan(lib, s, enabled, nb, target=-1):
    sh = np.array([s[k] for k in ("P", "L", "kmax", "R", "n_dir", "n_spec")], dtype=np.int64)
    out = np.zeros(4 + 5 * 5 + 9, dtype=np.int64)
    lib.hostemu_derived_plan(sh.ctypes.data_as(ctypes.c_void_p), ctypes.c_long(enabled), ctypes.c_long(nb), ctypes.c_long(target), out.ctypes.data_as(ctypes.c_void_p))
    v = [int(x) for x in out]
    got = dict(runs=v[0], nslots=v[1], side_bytes=v[2], refused=v[3])
    for s_, name in enumerate(NAMES):
        got[name] = dict(zip(FIELDS, v[4 + 5 * s_:9 + 5 * s_]))
    if target >= 0:
        got["fit"] = dict(runs=v[29], o_stage=v[30:35], o_side=v[35], o_ints=v[36], bytes=v[37])
    return got


# bench.py's model: 60 MVs under 6 LVs, 15 effect pairs, at most 4 predecessors; its 10 direct paths and 24 specific indirect effects
HEAD = shape(60, 6, 4, 15, n_dir=10, n_spec=24)
NB = 5000
HEAD_STAGE = {
    "assess": dict(stride=71, waves=4, wave_doubles=474, lds=15168, grid=1250),
    "structural": dict(stride=46, waves=4, wave_doubles=50 + 10 * 38, lds=13760, grid=1250),
    "plsc": dict(stride=173, waves=4, wave_doubles=446, lds=14272, grid=1250),
    "modelfit": dict(stride=6, waves=4, wave_doubles=260, lds=8320, grid=1250),
    "geodesic": dict(stride=4, waves=4, wave_doubles=4160, lds=133120, grid=1250),
}
NOT_RUN = dict(stride=0, waves=0, wave_doubles=0, lds=0, grid=0)
# the running set of every combination of the five switches, by the switches' value 0 .. 31
RUNS = [0, 1, 3, 3, 5, 5, 7, 7, 13, 13, 15, 15, 13, 13, 15, 15, 29, 29, 31, 31, 29, 29, 31, 31, 29, 29, 31, 31, 29, 29, 31, 31]


@pytest.mark.parametrize("enabled", range(32))
def test_switch_combinations_on_the_headline(emu, enabled):
    got = plan(emu, HEAD, enabled, NB)
    runs = RUNS[enabled]
    assert got["runs"] == runs and got["refused"] == -1
    for s, name in enumerate(NAMES):
        assert got[name] == (HEAD_STAGE[name] if runs >> s & 1 else NOT_RUN), name
    assert got["side_bytes"] == (720000 if runs & 4 else 0)
    assert got["nslots"] == (10 if runs & 2 else 0)


def test_the_running_sets_named():
    assert RUNS[1 << STRUCTURAL] == 0b00011 and RUNS[1 << PLSC] == 0b00101 and RUNS[1 << MODELFIT] == 0b01101 and RUNS[1 << GEODESIC] == 0b11101
    assert RUNS[(1 << GEODESIC) | (1 << STRUCTURAL)] == 0b11111 and len(RUNS) == 32


def test_more_bits_than_stages_are_ignored(emu):
    assert plan(emu, HEAD, 32 | 1, NB)["runs"] == 1 and plan(emu, HEAD, 64, NB)["runs"] == 0


def two_lv(P):
    """P MVs under two LVs in a chain: one effect pair, one predecessor.  A geodesic wave takes 3 P + 16 + P (P + 1) + 4 P = (P + 4)^2 doubles."""
    return shape(P, 2, 1, 1)


# (id, P, waves, lds, grid of 10 problems, refused)
GEODESIC_EDGES = [
    ("P 67: 71^2 = 5,041 doubles, the largest with four waves", 67, 4, 4 * 5041 * 8, 3, -1),
    ("P 68: 72^2 = 5,184, three", 68, 3, 3 * 5184 * 8, 4, -1),
    ("P 78: 82^2 = 6,724, the largest with three", 78, 3, 3 * 6724 * 8, 4, -1),
    ("P 79: 83^2 = 6,889, two", 79, 2, 2 * 6889 * 8, 5, -1),
    ("P 97: 101^2 = 10,201, the largest with two", 97, 2, 2 * 10201 * 8, 5, -1),
    ("P 98: 102^2 = 10,404, one", 98, 1, 10404 * 8, 10, -1),
    ("P 139: 143^2 = 20,449, the largest that fits", 139, 1, 20449 * 8, 10, -1),
    ("P 140: 144^2 = 20,736 > 20,480: refused", 140, 1, 20736 * 8, 10, GEODESIC),
]


@pytest.mark.parametrize("P,waves,lds,grid,refused", [c[1:] for c in GEODESIC_EDGES], ids=[c[0] for c in GEODESIC_EDGES])
def test_geodesic_edges(emu, P, waves, lds, grid, refused):
    got = plan(emu, two_lv(P), 1 << GEODESIC, 10)
    assert got["runs"] == 0b11101 and got["refused"] == refused
    assert got["geodesic"] == dict(stride=4, waves=waves, wave_doubles=(P + 4) ** 2, lds=lds, grid=grid)
    assert (lds <= 160 * 1024) == (refused < 0)
    # the stages of fixed waves beside it: four waves whatever P is
    assert got["assess"] == dict(stride=4 * 2 + 3 + 2, waves=4, wave_doubles=4 * P + 14 + 192, lds=32 * (4 * P + 206), grid=3)
    assert got["plsc"] == dict(stride=2 * P + 4 + 1 + 2, waves=4, wave_doubles=P + 16 + 6 + 8 + 2 * 3, lds=32 * (P + 36), grid=3)
    assert got["modelfit"] == dict(stride=6, waves=4, wave_doubles=3 * P + 16, lds=32 * (3 * P + 16), grid=3)
    assert got["side_bytes"] == 10 * 6 * 8


def test_geodesic_refusal_needs_the_stage(emu):
    assert plan(emu, two_lv(140), 1 << MODELFIT, 10)["refused"] == -1


# (id, L, kmax, n_dir, waves, nslots, wave_doubles, refused): base = L^2 + L + 8, slot = 2 kmax^2 + kmax + (kmax + 1) // 2
STRUCTURAL_EDGES = [
    ("63 direct paths: 63 slots", 8, 2, 63, 4, 63, 80 + 63 * 11, -1),
    ("64 direct paths: 64 slots", 8, 2, 64, 4, 64, 80 + 64 * 11, -1),
    ("65 direct paths: still 64", 8, 2, 65, 4, 64, 80 + 64 * 11, -1),
    ("more LVs than direct paths: a slot per LV", 12, 1, 5, 4, 12, 164 + 12 * 4, -1),
    ("kmax 5, slot 58: (5,120 - 118) // 58 = 86, so 64 slots fit beside four waves", 10, 5, 70, 4, 64, 118 + 64 * 58, -1),
    ("kmax 6, slot 81: (5,120 - 118) // 81 = 61 slots", 10, 6, 70, 4, 61, 118 + 61 * 81, -1),
    ("L 60, kmax 30, slot 1,845: none beside four waves, (10,240 - 3,668) // 1,845 = 3 beside two", 60, 30, 59, 2, 3, 3668 + 3 * 1845, -1),
    ("L 60, kmax 50, slot 5,075: one slot beside two waves", 60, 50, 59, 2, 1, 3668 + 5075, -1),
    ("L 60, kmax 59, slot 7,051: (20,480 - 3,668) // 7,051 = 2 in a workgroup of one wave", 60, 59, 59, 1, 2, 3668 + 2 * 7051, -1),
    ("L 100, kmax 99, slot 19,751 beside rc's 10,108: one wave with one slot does not fit", 100, 99, 99, 1, 1, 10108 + 19751, STRUCTURAL),
    ("L 150: rc alone, 22,658 doubles, does not fit", 150, 1, 149, 1, 1, 22658 + 4, STRUCTURAL),
]


@pytest.mark.parametrize("L,kmax,n_dir,waves,nslots,doubles,refused", [c[1:] for c in STRUCTURAL_EDGES], ids=[c[0] for c in STRUCTURAL_EDGES])
def test_structural_edges(emu, L, kmax, n_dir, waves, nslots, doubles, refused):
    s = shape(2 * L, L, kmax, n_dir, n_dir=n_dir, n_spec=7)
    got = plan(emu, s, 1 << STRUCTURAL, 9)
    assert got["runs"] == 0b00011 and got["refused"] == refused and got["nslots"] == nslots and got["side_bytes"] == 0
    assert got["structural"] == dict(stride=2 * n_dir + 7 + 2, waves=waves, wave_doubles=doubles, lds=8 * waves * doubles, grid=-(-9 // waves))
    assert (got["structural"]["lds"] <= 160 * 1024) == (refused < 0)


def test_structural_lists_not_built(emu):
    """The width of the structural records before plspm_structural_enable has enumerated the paths: zero, and a slot per LV."""
    got = plan(emu, shape(60, 6, 4, 15), 1 << STRUCTURAL, 1)
    assert got["structural"] == dict(stride=2, waves=4, wave_doubles=50 + 6 * 38, lds=32 * 278, grid=1) and got["nslots"] == 6


# the headline's full-sample block per target stage: the solver's record takes 156 + 2 doubles
FIT_LAYOUT = [
    ("assessment", ASSESS, dict(runs=0b00001, o_stage=[158, -1, -1, -1, -1], o_side=229, o_ints=229, bytes=229 * 8 + 8)),
    ("structural", STRUCTURAL, dict(runs=0b00011, o_stage=[158, 229, -1, -1, -1], o_side=275, o_ints=275, bytes=275 * 8 + 8)),
    ("PLSc", PLSC, dict(runs=0b00101, o_stage=[158, -1, 229, -1, -1], o_side=402, o_ints=420, bytes=420 * 8 + 8)),
    ("model fit", MODELFIT, dict(runs=0b01101, o_stage=[158, -1, 229, 402, -1], o_side=408, o_ints=426, bytes=426 * 8 + 8)),
    ("geodesic", GEODESIC, dict(runs=0b11101, o_stage=[158, -1, 229, 402, 408], o_side=412, o_ints=430, bytes=430 * 8 + 8)),
]


@pytest.mark.parametrize("target,expected", [c[1:] for c in FIT_LAYOUT], ids=[c[0] for c in FIT_LAYOUT])
def test_full_sample_block(emu, target, expected):
    got = plan(emu, HEAD, 0, 1, target)
    assert got["fit"] == expected
    assert got["runs"] == 0      # (the plan of the switches, none here, beside the layout's own)


def test_stage_table(emu):
    """What each stage reads, its workgroup, whether its entry points are for plain metric handles only, the words of its messages, and the refusal of a stage sized by the LDS."""
    rows = []
    for s in range(5):
        out = np.zeros(4, dtype=np.int64)
        emu.hostemu_derived_stage(s, out.ctypes.data_as(ctypes.c_void_p))
        rows.append(tuple(int(v) for v in out) + tuple(emu.hostemu_derived_word(s, k).decode() for k in range(5)))
    assert rows == [
        (0, 4, 4, 0, "assess", "assessment", "assessed", "", ""),
        (1, 4, 1, 1, "structural", "structural", "structural", "structural assessment", "rc and one regression slot of one replicate need more than 160 KiB of LDS"),
        (1, 4, 4, 0, "plsc", "PLSc", "PLSc", "", ""),
        (4, 4, 4, 1, "modelfit", "model-fit", "model-fit", "", ""),
        (12, 4, 1, 1, "geodesic", "geodesic", "geodesic", "geodesic discrepancy", "the two P x P triangles of one replicate need more than 160 KiB of LDS"),
    ]
