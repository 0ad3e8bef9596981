"""CPU: the host surface of model fit -- the NumPy mirror of the model-fit kernel (plspm.modelfit._model_fit) against a closed form, the composite model,
the implied construct correlations against an independent route, the Bollen-Stine transformation, the portable part of the kernel (csrc/modelfit_core.h) as
a stand-alone host program under AddressSanitizer and UndefinedBehaviorSanitizer, the declarations of the new C-ABI symbols, and the host errors that need no
device.

The closed form is tests/test_plsc.py's population (R = Lambda Phi Lambda' + Theta, three LVs, every path).  With the population weights PLSc returns Lambda,
Phi and the path coefficients exactly, so the model reproduces R: all four statistics are zero.  Without the path 0 -> 2 in the model the regression of LV 2
is on LV 1 alone, beta_21 = phi_12, the implied phi_02 is phi_12 phi_01, and the only residuals are those between blocks 0 and 2:
d_uls_est = (sum lambda_0^2) (sum lambda_2^2) (phi_02 - phi_12 phi_01)^2 = 1.0 * 2.2125 * 0.225^2."""
import fnmatch
import os
import re
import subprocess

import numpy as np
import pandas as pd
import pytest

import plspm.config as c
import plspm_oracle as orc
from helpers import SAT_ADD_ORDER, SAT_PREFIX, satisfaction_frame, satisfaction_oracle_inputs
from helpers_modelfit import PATH, PATH_WITHOUT_02, oracle_model_fit, population
from plspm import _native
from plspm.mode import Mode
from plspm.modelfit import ModelFit, _bollen_stine, _implied_phi, _model_fit
from plspm.plsc import _effect_pairs, _plsc
from plspm.scale import Scale
from plspm.scheme import Scheme
from plspm.weights import NumericalConditionError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tests", "modelfit_host")
NEW_SYMBOLS = ("plspm_modelfit_enable", "plspm_modelfit_width", "plspm_modelfit_fit", "plspm_modelfit_fetch", "plspm_modelfit_summary", "plspm_modelfit_intervals")


def population_fit(dtype, C, factor=(1, 1, 1)):
    R, blocks, w, lam, _ = population(dtype)
    plsc = _plsc(R, w, lam, blocks, "AAA", C, list(factor))
    return R, blocks, plsc, _model_fit(R, plsc, blocks, C, factor)


# ------------------------------------------------------------------ 1. the closed form
@pytest.mark.parametrize("dtype", [np.float64, np.longdouble])
def test_closed_form(dtype):
    R, _, _, fit = population_fit(dtype, PATH)
    assert fit["status"] == 0 and fit["record"].dtype == np.dtype(dtype)
    np.testing.assert_allclose(fit["record"].astype(np.float64), 0.0, rtol=0, atol=1e-12)
    np.testing.assert_allclose(fit["implied"]["estimated"].astype(np.float64), R.astype(np.float64), rtol=0, atol=1e-12)
    # without the path 0 -> 2
    R, _, _, fit = population_fit(dtype, PATH_WITHOUT_02)
    assert fit["status"] == 0
    assert abs(float(fit["srmr_sat"])) <= 1e-12 and abs(float(fit["d_uls_sat"])) <= 1e-12
    expected = 1.0 * 2.2125 * 0.225 ** 2
    np.testing.assert_allclose(float(fit["d_uls_est"]), expected, rtol=1e-12)
    np.testing.assert_allclose(float(fit["srmr_est"]), np.sqrt(2.0 * expected / (10 * 11)), rtol=1e-12)
    np.testing.assert_allclose(float(fit["phi"][2, 0]), 0.55 * 0.5, rtol=1e-12)
    assert np.array_equal(fit["record"], [fit["srmr_sat"], fit["d_uls_sat"], fit["srmr_est"], fit["d_uls_est"]])


# ------------------------------------------------------------------ 2. the composite model
def random_problem(seed, sizes, C, n=200, modes=None):
    """R of random correlated data, unit weights, the composites' loadings."""
    rng = np.random.default_rng(seed)
    P = sum(sizes)
    off = np.concatenate(([0], np.cumsum(sizes)))
    blocks = [np.arange(off[l], off[l + 1]) for l in range(len(sizes))]
    common = rng.standard_normal((n, 1))
    X = np.empty((n, P))
    for blk in blocks:
        X[:, blk] = 0.6 * common + 0.7 * rng.standard_normal((n, 1)) + 0.8 * rng.standard_normal((n, len(blk)))
    R = np.corrcoef(X, rowvar=False).reshape(P, P)
    R = 0.5 * (R + R.T)                                      # (symmetric to the last bit, and a unit diagonal)
    np.fill_diagonal(R, 1.0)
    w = np.ones(P)
    lam = np.concatenate([R[np.ix_(b, b)] @ (w[b] / np.sqrt(w[b] @ R[np.ix_(b, b)] @ w[b])) for b in blocks])
    return R, blocks, w, lam, modes or "A" * len(sizes)


def test_composite_model():
    C = np.array([[0, 0, 0, 0], [1, 0, 0, 0], [1, 1, 0, 0], [0, 1, 1, 0]])
    R, blocks, w, lam, modes = random_problem(1, [3, 1, 4, 5], C)
    zero = np.zeros(4, dtype=int)
    plsc = _plsc(R, w, lam, blocks, modes, C, zero)
    fit = _model_fit(R, plsc, blocks, C, zero)
    assert fit["status"] == 0
    P = R.shape[0]
    for model in ("saturated", "estimated"):
        S = fit["implied"][model]
        assert np.array_equal(S, S.T) and np.all(np.diag(S) == 1.0)
        for blk in blocks:
            assert np.array_equal(S[np.ix_(blk, blk)], R[np.ix_(blk, blk)])      # a composite reproduces its own block: the residual is exactly 0
    S = fit["implied"]["saturated"]
    np.testing.assert_allclose(fit["d_uls_sat"], 0.5 * np.linalg.norm(R - S, "fro") ** 2, rtol=1e-13)
    np.testing.assert_allclose(fit["srmr_sat"], np.sqrt(np.linalg.norm(R - S, "fro") ** 2 / (P * (P + 1))), rtol=1e-13)
    # entry by entry, between blocks: lambda_p rc_ij lambda_q with the fit's own loadings
    for i, bi in enumerate(blocks):
        for j, bj in enumerate(blocks):
            if i != j:
                for p in bi:
                    for q in bj:
                        assert abs(S[p, q] - lam[p] * plsc["lv_cor"][i, j] * lam[q]) <= 1e-15
    assert fit["d_uls_sat"] > 0 and fit["d_uls_est"] != fit["d_uls_sat"]
    # a factor block is not reproduced: lambda lambda' off its diagonal
    one = np.array([1, 0, 1, 1])
    plsc1 = _plsc(R, w, lam, blocks, modes, C, one)
    S1 = _model_fit(R, plsc1, blocks, C, one)["implied"]["saturated"]
    b0 = blocks[0]
    expect = np.outer(plsc1["loadings"][b0], plsc1["loadings"][b0])
    np.fill_diagonal(expect, 1.0)
    assert np.array_equal(S1[np.ix_(b0, b0)], expect) and not np.array_equal(expect, R[np.ix_(b0, b0)])
    # a Mode-B block is a composite
    plscb = _plsc(R, w, lam, blocks, "AABA", C, [1, 0, 0, 1])
    Sb = _model_fit(R, plscb, blocks, C, [1, 0, 0, 1])["implied"]["estimated"]
    assert np.array_equal(Sb[np.ix_(blocks[2], blocks[2])], R[np.ix_(blocks[2], blocks[2])])


def test_inadmissible_inputs():
    R, blocks, w, lam, _ = population(np.float64)
    Rn = R.copy()
    Rn[0, 1] = Rn[1, 0] = -0.1                               # rho_A of LV 0 negative: the PLSc record is inadmissible
    plsc = _plsc(Rn, w, lam, blocks, "AAA", PATH, [1, 1, 1])
    fit = _model_fit(Rn, plsc, blocks, PATH, [1, 1, 1])
    assert plsc["status"] == 4 and fit["status"] == 4 and np.all(np.isnan(fit["record"])) and fit["implied"] is None
    plsc = _plsc(R, w, lam, blocks, "AAA", PATH, [1, 1, 1])
    Rc = R.copy()
    Rc[3, :] = Rc[:, 3] = np.nan                             # a constant column has no correlations
    fit = _model_fit(Rc, plsc, blocks, PATH, [1, 1, 1])
    assert fit["status"] == 4 and np.all(np.isnan(fit["record"]))
    with pytest.raises(ValueError, match="path order"):
        _implied_phi(np.eye(2), np.zeros((2, 2)), np.array([[0, 1], [0, 0]]))


# ------------------------------------------------------------------ 3. the implied construct correlations against an independent route
def covariance_route(rc, B, C):
    """eta = (I - B)^-1 zeta:  Phi = A Psi A' with A = (I - B)^-1, Psi = rc among the LVs without predecessors, and for an LV with predecessors a residual
    that is uncorrelated with every other entry of zeta and whose variance makes Phi_jj = 1."""
    L = rc.shape[0]
    A = np.linalg.inv(np.eye(L) - B)
    exo = np.flatnonzero(C.sum(axis=1) == 0)
    Psi = np.zeros((L, L))
    Psi[np.ix_(exo, exo)] = rc[np.ix_(exo, exo)]
    for j in range(L):
        if C[j].any():
            Psi[j, j] = 1.0 - A[j, :j] @ Psi[:j, :j] @ A[j, :j]
    return A @ Psi @ A.T


def dag_cases():
    cases = []
    for seed, L in ((1, 5), (2, 8), (3, 12), (4, 12)):
        rng = np.random.default_rng(seed)
        cases.append(("random_%d" % seed, np.tril(rng.random((L, L)) < 0.35, -1).astype(int)))
    C = np.zeros((12, 12), dtype=int)
    C[9, :9] = 1                                             # nine predecessors
    C[10, [0, 1]] = 1                                        # two LVs with predecessors and no link between them
    C[11, [2, 3]] = 1
    cases.append(("nine_and_unlinked", C))
    C = np.zeros((6, 6), dtype=int)                          # LVs without predecessors behind LVs with: 2 and 4
    C[1, 0] = C[3, 1] = C[3, 2] = C[5, 3] = C[5, 4] = 1
    cases.append(("exogenous_behind_endogenous", C))
    return cases


@pytest.mark.parametrize("name,C", dag_cases(), ids=[n for n, _ in dag_cases()])
def test_implied_construct_correlations_against_the_covariance_route(name, C):
    L = C.shape[0]
    rng = np.random.default_rng(L)
    F = rng.standard_normal((L, L))
    rc = F @ F.T + L * np.eye(L)
    rc = rc / np.sqrt(np.outer(np.diag(rc), np.diag(rc)))
    B = C * rng.uniform(-0.3, 0.3, (L, L))
    if name == "nine_and_unlinked":
        assert C[9].sum() == 9 and C[10].any() and C[11].any() and not C[11, 10]
    if name == "exogenous_behind_endogenous":
        assert not C[2].any() and C[1].any()
    phi = _implied_phi(rc, B, C)
    assert np.array_equal(phi, phi.T) and np.all(np.diag(phi) == 1.0)
    np.testing.assert_allclose(phi, covariance_route(rc, B, C), rtol=0, atol=1e-12)


# ------------------------------------------------------------------ 4. the Bollen-Stine transformation
def satisfaction_problem():
    X, blocks, _ = satisfaction_oracle_inputs()
    model = orc.Model(blocks, orc.satisfaction_C(), "AAAAAA", "path", True)
    return X, model


def test_transformation():
    X, model = satisfaction_problem()
    fit = oracle_model_fit(X, model, None)
    assert fit["status"] == 0
    Xd = X[:, model.mv_order]
    for sigma in (fit["implied"]["estimated"], fit["implied"]["saturated"]):
        Xt = _bollen_stine(Xd, sigma)
        assert float(np.max(np.abs(np.corrcoef(Xt, rowvar=False) - sigma))) <= 1e-10
        np.testing.assert_allclose(Xt.mean(axis=0), 0.0, rtol=0, atol=1e-10)
        np.testing.assert_allclose(Xt.std(axis=0), 1.0, rtol=1e-10)
    rng = np.random.default_rng(3)
    Y = rng.standard_normal((300, 10)) @ rng.standard_normal((10, 10)) + 5.0
    F = rng.standard_normal((10, 3))
    sigma = F @ F.T + np.diag(rng.uniform(0.5, 1.5, 10))
    sigma = sigma / np.sqrt(np.outer(np.diag(sigma), np.diag(sigma)))
    assert float(np.max(np.abs(np.corrcoef(_bollen_stine(Y, sigma), rowvar=False) - sigma))) <= 1e-10
    # collinear columns: R is singular
    Yc = Y.copy()
    Yc[:, 9] = Yc[:, 0] + Yc[:, 1]
    with pytest.raises(NumericalConditionError, match="data's correlation matrix"):
        _bollen_stine(Yc, sigma)
    # an implied matrix that is not positive definite
    bad = np.full((10, 10), -0.5)
    np.fill_diagonal(bad, 1.0)
    with pytest.raises(NumericalConditionError, match="model-implied"):
        _bollen_stine(Y, bad)
    const = Y.copy()
    const[:, 4] = 1.0
    with pytest.raises(NumericalConditionError):
        _bollen_stine(const, sigma)


# ------------------------------------------------------------------ 5. the portable part of the kernel as a host program under sanitizers
def host_values(tmp_path, R, plsc, blocks, C, factor, tag):
    """What csrc/modelfit_core.h computes from the mirror's PLSc estimates: written as text, run as a child process.  (record [6], Phi^ [L, L])"""
    subprocess.check_call(["make", "-s", "-C", HOST, "modelfit_host"])
    P, L = R.shape[0], len(blocks)
    pairs = _effect_pairs(C)
    boff = np.concatenate(([0], np.cumsum([len(b) for b in blocks])))
    numbers = lambda a: " ".join(repr(float(x)) for x in np.asarray(a, dtype=np.float64).ravel())      # noqa: E731
    text = "\n".join(["%d %d" % (P, L), " ".join(str(int(x)) for x in boff), " ".join(str(int(x)) for x in np.asarray(C).ravel()),
                      " ".join(str(int(x)) for x in factor), numbers(plsc["loadings"]), numbers(plsc["lv_cor"][np.triu_indices(L, 1)]),
                      numbers([plsc["path"][t, f] for f, t in pairs]), numbers(R), "%d 7" % plsc["status"]])
    path = tmp_path / (tag + ".txt")
    path.write_text(text + "\n")
    run = subprocess.run([os.path.join(HOST, "modelfit_host"), str(path)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    assert "ERROR" not in run.stderr and "runtime error" not in run.stderr, run.stderr
    values = np.array([float(x) for x in run.stdout.split()])
    assert values.shape == (6 + L * L,)
    return values[:6], values[6:].reshape(L, L)


def host_shapes():
    R, blocks, w, lam, _ = population(np.float64)
    yield "closed_form_without_02", R, blocks, w, lam, "AAA", PATH_WITHOUT_02, [1, 0, 1]
    C = np.zeros((10, 10), dtype=int)
    C[9, :9] = 1
    yield ("nine_predecessors",) + random_problem(2, [2] * 10, C) + (C, [1] * 10)
    C = dict(dag_cases())["exogenous_behind_endogenous"]
    yield ("exogenous_behind_endogenous",) + random_problem(3, [3, 1, 4, 2, 5, 3], C, modes="AAAABA") + (C, [1, 0, 0, 1, 0, 1])
    C = dict(dag_cases())["random_3"]
    yield ("twelve_composites",) + random_problem(4, [2] * 12, C) + (C, [0] * 12)


@pytest.mark.parametrize("shape", list(host_shapes()), ids=[s[0] for s in host_shapes()])
def test_host_program_under_sanitizers_against_the_mirror(tmp_path, shape):
    tag, R, blocks, w, lam, modes, C, factor = shape
    plsc = _plsc(R, w, lam, blocks, modes, C, factor)
    fit = _model_fit(R, plsc, blocks, C, factor)
    assert plsc["status"] == 0 and fit["status"] == 0 and fit["d_uls_est"] > 0
    record, phi = host_values(tmp_path, R, plsc, blocks, C, factor, tag)
    assert record[4] == 0.0 and record[5] == 7.0
    np.testing.assert_allclose(record[:4], fit["record"], rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(phi, fit["phi"], rtol=0, atol=1e-14)


def test_host_program_reports_a_value_that_is_not_finite(tmp_path):
    R, blocks, w, lam, _ = population(np.float64)
    plsc = _plsc(R, w, lam, blocks, "AAA", PATH, [1, 1, 1])
    Rn = R.copy()
    Rn[0, 5] = Rn[5, 0] = np.nan
    record, _ = host_values(tmp_path, Rn, plsc, blocks, PATH, [1, 1, 1], "not_finite")
    assert record[4] == 4.0 and record[5] == 7.0 and np.all(np.isnan(record[:4]))


# ------------------------------------------------------------------ 6. the surface
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


def test_argument_errors_without_a_handle():
    lib = _native.load()
    out = np.zeros(32)
    assert lib.plspm_modelfit_enable(None, 1, None) == 100   # PLSPM_E_ARG
    assert lib.plspm_modelfit_width(None) == 0
    assert lib.plspm_modelfit_fit(None, out.ctypes.data, None) == 100
    assert lib.plspm_modelfit_fetch(None, 0, 1, out.ctypes.data, None) == 100
    assert lib.plspm_modelfit_summary(None, 10, out.ctypes.data, out.ctypes.data, None) == 100
    assert lib.plspm_modelfit_intervals(None, 10, out.ctypes.data, 0, 0.95, out.ctypes.data, None) == 100


def sat_config(scale=None, mode_b=None):
    sat = satisfaction_frame()
    s = c.Structure()
    s.add_path(["IMAG"], ["EXPE", "SAT", "LOY"]); s.add_path(["EXPE"], ["QUAL", "VAL", "SAT"])
    s.add_path(["QUAL"], ["VAL", "SAT"]); s.add_path(["VAL"], ["SAT"]); s.add_path(["SAT"], ["LOY"])
    cfg = c.Config(s.path(), scaled=True) if scale is None else c.Config(s.path(), default_scale=scale)
    for lv in SAT_ADD_ORDER:
        cfg.add_lv_with_columns_named(lv, Mode.B if lv == mode_b else Mode.A, sat, SAT_PREFIX[lv])
    return sat, cfg


def test_host_errors_that_need_no_device():
    sat, cfg = sat_config()
    with pytest.raises(NotImplementedError, match="one GPU"):
        ModelFit(sat, cfg, Scheme.PATH, iterations=100, processes=2)
    with pytest.raises(ValueError, match="null"):
        ModelFit(sat, cfg, Scheme.PATH, iterations=100, null="independence")
    with pytest.raises(ValueError, match="negative"):
        ModelFit(sat, cfg, Scheme.PATH, iterations=-1)
    with pytest.raises(ValueError, match="not a latent variable"):
        ModelFit(sat, cfg, Scheme.PATH, iterations=100, factors=["IMAG", "NOPE"])
    with pytest.raises(ValueError, match="list"):
        ModelFit(sat, cfg, Scheme.PATH, iterations=100, factors="IMAG")
    _, cfg_b = sat_config(mode_b="VAL")
    with pytest.raises(ValueError, match="cannot be a common factor"):
        ModelFit(sat, cfg_b, Scheme.PATH, iterations=100, factors=["VAL"])
    _, cfg_nm = sat_config(scale=Scale.NUM)
    with pytest.raises(NotImplementedError, match="non-metric"):
        ModelFit(sat, cfg_nm, Scheme.PATH, iterations=100)
    holes = sat.copy()
    holes.iloc[3, holes.columns.get_loc(cfg.filter(sat).columns[0])] = np.nan
    with pytest.raises(NotImplementedError, match="missing"):
        ModelFit(holes, cfg, Scheme.PATH, iterations=100)
    mobi = pd.read_csv(os.path.join(ROOT, "tests", "golden", "ref_data", "mobi.csv"), index_col=0).astype(float)
    structure = c.Structure()
    structure.add_path(["Expectation", "Quality"], ["Satisfaction"])
    structure.add_path(["Satisfaction"], ["Complaints", "Loyalty"])
    hoc = c.Config(structure.path())
    hoc.add_higher_order("Satisfaction", Mode.A, ["Image", "Value"])
    for lv, prefix in (("Expectation", "CUEX"), ("Quality", "PERQ"), ("Loyalty", "CUSL"), ("Image", "IMAG"), ("Complaints", "CUSCO"), ("Value", "PERV")):
        hoc.add_lv_with_columns_named(lv, Mode.A, mobi, prefix)
    with pytest.raises(NotImplementedError, match="higher-order"):
        ModelFit(mobi, hoc, Scheme.PATH, iterations=100)
