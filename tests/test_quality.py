"""CPU: the host surface of the measurement-model assessment -- the NumPy mirror of the assessment kernel (plspm.quality._quality) against closed
forms and against Unidimensionality's Cronbach's alpha, the declarations of the new C-ABI symbols, and the argument errors that need no device."""
import fnmatch
import os
import re
import types

import numpy as np
import pytest

import plspm.config as c
import plspm_oracle as orc
from helpers import SAT_ADD_ORDER, SAT_PREFIX, satisfaction_frame
from plspm import _native
from plspm._compile import compile_model
from plspm.mode import Mode
from plspm.quality import CRITERIA, LV_CRITERIA, PAIR_CRITERIA, _quality, _record
from plspm.unidimensionality import Unidimensionality

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("plspm_assess_enable", "plspm_assess_width", "plspm_assess_fit", "plspm_assess_fetch", "plspm_assess_summary", "plspm_assess_intervals")


def equicorrelated(sizes, rho, tau):
    """Blocks of the given sizes: correlation rho inside a block, tau between blocks."""
    P = sum(sizes)
    lv = np.repeat(np.arange(len(sizes)), sizes)
    R = np.where(lv[:, None] == lv[None, :], rho, tau).astype(np.float64)
    np.fill_diagonal(R, 1.0)
    off = np.concatenate(([0], np.cumsum(sizes)))
    return R, [np.arange(off[l], off[l + 1]) for l in range(len(sizes))]


@pytest.mark.parametrize("dtype", [np.float64, np.longdouble])
@pytest.mark.parametrize("k,rho", [(2, 0.3), (4, 0.55), (9, 0.8)])
def test_equicorrelated_block_closed_forms(k, rho, dtype):
    R, blocks = equicorrelated([k], rho, 0.0)
    lam = np.full(k, np.sqrt(rho))
    q = _quality(R.astype(dtype), np.ones(k), lam, blocks, "A")
    assert q["alpha"].dtype == np.dtype(dtype)
    np.testing.assert_allclose(q["alpha"], [k * rho / (1 + (k - 1) * rho)], rtol=1e-14)
    # equal weights on an equicorrelated block: v'v = k c^2, v'(R - I)v = c^2 k (k - 1) rho, sum v^4 = k c^4  =>  rho_a = k rho / (1 + (k - 1) rho) as well
    np.testing.assert_allclose(q["rho_a"], [k * rho / (1 + (k - 1) * rho)], rtol=1e-13)
    np.testing.assert_allclose(q["ave"], [rho], rtol=1e-14)
    np.testing.assert_allclose(q["rho_c"], [k * k * rho / (k * k * rho + k * (1 - rho))], rtol=1e-14)
    assert q["htmt"].shape == (0,)


@pytest.mark.parametrize("tau", [0.24, -0.24])
def test_two_equicorrelated_blocks_htmt(tau):
    rho = 0.6
    R, blocks = equicorrelated([3, 5], rho, tau)
    q = _quality(R, np.ones(8), np.full(8, 0.7), blocks, "AB")
    np.testing.assert_allclose(q["htmt"], [abs(tau) / rho], rtol=1e-14)
    np.testing.assert_allclose(q["htmt2"], [abs(tau) / rho], rtol=1e-13)
    # v_b = 1 / sqrt(k (1 + (k - 1) rho)) on every item: v_i' R_ij v_j = tau k_i k_j v_i v_j
    expect = tau * 15 / np.sqrt(3 * (1 + 2 * rho) * 5 * (1 + 4 * rho))
    np.testing.assert_allclose(q["lv_cor"], [expect], rtol=1e-14)
    assert q["rho_a"][1] == 1.0                               # Mode B
    assert q["rho_a"][0] != 1.0


def test_the_sign_follows_the_loadings():
    R, blocks = equicorrelated([3, 3], 0.5, 0.2)
    lam = np.full(6, 0.7)
    plain = _quality(R, np.ones(6), lam, blocks, "AA")["lv_cor"][0]
    lam[:3] = -0.7                                            # the fit flipped LV 0
    assert _quality(R, np.ones(6), lam, blocks, "AA")["lv_cor"][0] == -plain
    # the weights' global scale and the columns' standard deviations cancel in the normalisation
    scaled = _quality(R, 3.0 * np.ones(6) / np.array([1, 2, 3, 4, 5, 6.0]), np.full(6, 0.7), blocks, "AA", sd=np.array([1, 2, 3, 4, 5, 6.0]))
    np.testing.assert_allclose(scaled["lv_cor"], [plain], rtol=1e-14)


def test_single_item_blocks_are_one():
    R, blocks = equicorrelated([1, 1, 3], 0.5, 0.3)
    q = _quality(R, np.ones(5), np.array([1.0, 1.0, 0.8, 0.8, 0.8]), blocks, "AAA")
    for name in LV_CRITERIA:
        assert q[name][0] == 1.0 and q[name][1] == 1.0, name
    np.testing.assert_allclose(q["htmt"][0], 0.3, rtol=1e-14)              # both m_l are 1
    np.testing.assert_allclose(q["htmt"][1], 0.3 / np.sqrt(0.5), rtol=1e-14)
    np.testing.assert_allclose(q["lv_cor"][0], 0.3, rtol=1e-14)
    assert _record(q).shape == (4 * 3 + 3 * 3,)
    assert CRITERIA == LV_CRITERIA + PAIR_CRITERIA


def test_a_zero_correlation_gives_htmt2_zero():
    R, blocks = equicorrelated([2, 2], 0.5, 0.2)
    R[0, 2] = R[2, 0] = 0.0
    q = _quality(R, np.ones(4), np.full(4, 0.7), blocks, "AA")
    assert q["htmt2"][0] == 0.0 and q["htmt"][0] > 0.0


def test_alpha_is_unidimensionality_cronbach_alpha_on_satisfaction():
    sat = satisfaction_frame()
    s = c.Structure()
    s.add_path(["IMAG"], ["EXPE", "SAT", "LOY"]); s.add_path(["EXPE"], ["QUAL", "VAL", "SAT"])
    s.add_path(["QUAL"], ["VAL", "SAT"]); s.add_path(["VAL"], ["SAT"]); s.add_path(["SAT"], ["LOY"])
    cfg = c.Config(s.path(), scaled=True)
    for lv in SAT_ADD_ORDER:
        cfg.add_lv_with_columns_named(lv, Mode.A, sat, SAT_PREFIX[lv])
    data = cfg.filter(sat)
    cm = compile_model(cfg, cfg.path(), list(data.columns))
    X = data.values[:, cm.col_index].astype(np.float64)      # device column order
    cov = np.cov(X, rowvar=False, bias=True)
    fake = types.SimpleNamespace(compiled=cm, raw={"cov": cov})
    uni = Unidimensionality(cfg, fake).summary()
    blocks = [np.arange(cm.block_offset[l], cm.block_offset[l + 1]) for l in range(cm.L)]
    q = _quality(np.corrcoef(X, rowvar=False), np.ones(cm.P), np.full(cm.P, 0.5), blocks, "A" * cm.L)
    assert list(uni.index) == orc.SAT_LVS
    np.testing.assert_allclose(q["alpha"], uni["cronbach_alpha"].values.astype(np.float64), rtol=0, atol=1e-12)


# ------------------------------------------------------------------ the C-ABI's declarations
def test_new_symbols_are_declared_everywhere():
    header = open(os.path.join(ROOT, "include", "plspm_hip.h")).read()
    declared = set(re.findall(r"\b(plspm_[a-z_]+)\s*\(", header))
    exports_map = open(os.path.join(ROOT, "plspm-python_amd", "csrc", "exports.map")).read()
    pattern = re.search(r"global:\s*([^;]+);", exports_map).group(1).strip()
    lib = _native.load()
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in _native.EXPORTS, name
        assert fnmatch.fnmatchcase(name, pattern), (name, pattern)
        assert hasattr(lib, name), name
    assert lib.plspm_abi_version() == 4 and _native.ABI_VERSION == 4
    assert int(re.search(r"#define PLSPM_ABI_VERSION (\d+)", header).group(1)) == 4
    assert _native.KERNELS["assess"] == int(re.search(r"PLSPM_K_ASSESS = (\d+)", header).group(1))


def test_argument_errors_without_a_handle():
    lib = _native.load()
    out = np.zeros(16)
    assert lib.plspm_assess_enable(None, 1) == 100            # PLSPM_E_ARG
    assert lib.plspm_assess_width(None) == 0
    assert lib.plspm_assess_fit(None, out.ctypes.data, None) == 100
    assert lib.plspm_assess_fetch(None, 0, 1, out.ctypes.data, None) == 100
    assert lib.plspm_assess_summary(None, 10, out.ctypes.data, out.ctypes.data, None) == 100
    assert lib.plspm_assess_intervals(None, 10, out.ctypes.data, 0, 0.95, out.ctypes.data, None) == 100
