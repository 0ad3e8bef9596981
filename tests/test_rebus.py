"""CPU: REBUS-PLS without a GPU -- the portable part of the kernels (csrc/rebus_core.h, csrc/rebus_route.h) as a host program under AddressSanitizer / UBSan against
the NumPy mirror plspm.rebus._rebus, the plan table, properties of the mirror itself, and the argument and scope errors of plspm.rebus.Rebus."""
import os
import subprocess

import numpy as np
import pandas as pd
import pytest

import plspm.config as c
import plspm_oracle as orc
from helpers_fimix import assert_inside
from helpers_rebus import TRI3, flipped, host_input, mirror_pair, oracle_fit, planted, random_start, sized
from plspm import _native
from plspm.mode import Mode
from plspm.rebus import WARD_MAX_BYTES, Rebus, _argmin, _rebus, _start_labels, _ward_check
from plspm.scale import Scale

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tests", "rebus_host")
NEW_SYMBOLS = ("plspm_rebus_device", "plspm_rebus_fetch", "plspm_rebus_residuals")
SAT = orc.satisfaction_C()


# ------------------------------------------------------------------ the portable part of the kernels as a host program under sanitizers
def run_host(args, text=None):
    subprocess.check_call(["make", "-s", "-C", HOST, "rebus_host"])
    run = subprocess.run([os.path.join(HOST, "rebus_host")] + args, input=text, capture_output=True, text=True, timeout=120)
    assert "ERROR" not in run.stderr and "runtime error" not in run.stderr, run.stderr
    assert run.returncode == 0, (run.stdout, run.stderr)
    return run.stdout.strip().split("\n")


def host_step(X, model, K, labels, fits):
    """(flags [K], labels [N], CM [N, K]) of one step of csrc/rebus_core.h."""
    out = run_host(["step"], host_input(X, model, K, labels, fits))
    flags = [int(v) for v in out[0].split()]
    rows = np.array([[float(v) for v in line.split()] for line in out[1:]])
    assert rows.shape == (X.shape[0], K + 1)
    return flags, rows[:, 0].astype(np.int64), rows[:, 1:]


@pytest.mark.parametrize("N,C,sizes,K", [(61, np.array([[0, 0], [1, 0]]), [3, 1], 2), (257, SAT, [3] * 6, 3)], ids=["n61_single_item", "n257_satisfaction"])
def test_the_host_program_agrees_with_the_mirror(N, C, sizes, K):
    X, model = sized(N, C, sizes, seed=1)
    start = random_start(N, K, seed=1)
    fit = oracle_fit(model)
    fits = [fit(X[start == k]) for k in range(K)]
    m64, mld = mirror_pair(X, model, K, start, max_iter=0, records=[fits])
    flags, labels, cm = host_step(X, model, K, start, fits)
    assert flags == [1] * K
    assert_inside(cm, m64["cm"], mld["cm"], "host program CM")
    assert np.array_equal(labels, _argmin(m64["cm"], start)) and np.array_equal(labels, np.argmin(cm, axis=1))


def test_the_host_program_flags_an_invalid_class_and_a_nan_never_wins():
    X, model = sized(61, TRI3, [2, 2, 2], seed=2)
    start = random_start(61, 2, seed=2)
    fit = oracle_fit(model)
    flags, labels, cm = host_step(X, model, 2, start, [None, fit(X[start == 1])])
    assert flags == [0, 1] and np.isnan(cm[:, 0]).all() and np.isfinite(cm[:, 1]).all() and np.all(labels == 1)
    # a squared loading below the collapse bound (9e-6 squared: 1e-5 squared rounds to just above 1e-10), an R^2 at it
    for key, index in (("loadings", 3), ("r2", 2)):
        bad = fit(X[start == 0])
        bad[key] = bad[key].copy()
        bad[key][index] = 9e-6 if key == "loadings" else 1e-10
        assert host_step(X, model, 2, start, [bad, fit(X[start == 1])])[0] == [0, 1], key
    Xc = X.copy()
    Xc[start == 0, 1] = 2.5                                # a constant column in class 0
    assert host_step(Xc, model, 2, start, [fit(X[start == 0]), fit(X[start == 1])])[0] == [0, 1]


def plan(P, L, n_endo, K, N, caps):
    keys = ("param_doubles", "xs", "classes_per_load", "loads", "rows", "tiles", "assign_grid", "slices", "slice_rows", "lds_bytes", "refused")
    out = run_host(["plan", str(P), str(L), str(n_endo), str(K), str(N)] + [str(cap) for cap in caps])
    return [dict(zip(keys, (int(v) for v in line.split()))) for line in out]


def test_the_plan_table():
    # the satisfaction model at K = 3: everything in one load; the test-only cap splits it
    for p, cpl in zip(plan(18, 6, 5, 3, 1000, [0, 1, 2, 16]), [3, 1, 2, 3]):
        assert p["param_doubles"] == 5 * 18 + 6 + 5 * 7 and p["xs"] == 19 and p["rows"] == 64 and p["tiles"] == 16 and p["assign_grid"] == 4
        assert (p["classes_per_load"], p["loads"], p["refused"]) == (cpl, -(-3 // cpl), 0)
        assert p["lds_bytes"] == (64 * 19 + 6 * 256 + cpl * p["param_doubles"]) * 8 <= 160 * 1024
        assert p["slices"] == 1 and p["slice_rows"] == 1000
    # the split the LDS itself forces: 16 classes of 859 doubles beside 12,224 fixed ones -- nine per load
    p = plan(150, 10, 9, 16, 10000, [0])[0]
    assert p["param_doubles"] == 859 and (p["classes_per_load"], p["loads"], p["refused"]) == (9, 2, 0)
    assert p["lds_bytes"] <= 160 * 1024 < p["lds_bytes"] + 859 * 8
    assert p["tiles"] == 157 and p["assign_grid"] == 40 and p["slices"] == 5 and p["slices"] * p["slice_rows"] >= 10000 and p["slice_rows"] % 4 == 0
    # the refusal: one class's parameters do not fit beside the tile
    p = plan(300, 30, 29, 2, 1000, [0])[0]
    assert (p["classes_per_load"], p["loads"], p["refused"]) == (0, 0, 1)
    # the slices stop at 64
    assert plan(18, 6, 5, 2, 1000000, [0])[0]["slices"] == 64


# ------------------------------------------------------------------ the mirror itself
def test_one_class_stops_at_the_first_iteration():
    X, model, _ = planted(200, seed=1)
    start = np.zeros(200, dtype=np.int64)
    out = _rebus(X, model, 1, start, fit=oracle_fit(model))
    assert (out["status"], out["iterations"], out["changed"]) == (0, 1, [0])
    # its GQI is the one-class value: from the residuals of the model on all rows
    once = _rebus(X, model, 1, start, max_iter=0, fit=oracle_fit(model))
    com = (1 - once["within_e"][0] / 200).mean()
    r2 = (1 - once["within_f"][0] / 200).mean()
    assert out["gqi"] == once["gqi"] and abs(out["gqi"] - np.sqrt(com * r2)) <= 1e-15
    # communality and R^2 as the fit reports them: mean e^2 = 1 - loading^2, mean f^2 = 1 - R^2
    fit = oracle_fit(model)(X)
    np.testing.assert_allclose(1 - once["within_e"][0] / 200, fit["loadings"] ** 2, rtol=0, atol=1e-12)
    np.testing.assert_allclose(1 - once["within_f"][0] / 200, fit["r2"][1:], rtol=0, atol=1e-12)


@pytest.mark.parametrize("seed", [1, 2])
def test_planted_classes_beat_the_one_class_model(seed):
    X, model, cls = planted(400, seed=seed)
    fit = oracle_fit(model)
    one = _rebus(X, model, 1, np.zeros(400, dtype=np.int64), fit=fit)
    two = _rebus(X, model, 2, flipped(cls, 0.25, seed=3), fit=fit)
    print("GQI: one class %.4f, two classes %.4f after %d iterations" % (one["gqi"], two["gqi"], two["iterations"]))
    assert two["status"] == 0 and two["gqi"] > one["gqi"]


def test_a_permuted_start_gives_the_permuted_result():
    X, model, cls = planted(257, seed=1)
    start = random_start(257, 3, seed=5)
    perm = np.array([2, 0, 1])
    fit = oracle_fit(model)
    a = _rebus(X, model, 3, start, max_iter=30, fit=fit)
    b = _rebus(X, model, 3, perm[start], max_iter=30, fit=fit)
    assert (a["status"], a["iterations"], a["changed"]) == (b["status"], b["iterations"], b["changed"])
    assert np.array_equal(perm[a["labels"]], b["labels"]) and np.array_equal(a["sizes"], b["sizes"][perm])
    assert np.array_equal(a["cm"], b["cm"][:, perm]) and np.array_equal(a["within_e"], b["within_e"][perm])


def test_statuses_of_the_mirror():
    X, model, cls = planted(257, seed=1)
    fit = oracle_fit(model)
    start = flipped(cls, 0.25, seed=3)
    capped = _rebus(X, model, 2, start, max_iter=2, fit=fit)
    assert (capped["status"], capped["iterations"], len(capped["changed"])) == (1, 2, 2) and np.isfinite(capped["cm"]).all()
    none = _rebus(X, model, 2, start, max_iter=0, fit=fit)
    assert (none["status"], none["iterations"]) == (1, 0) and np.array_equal(none["labels"], start)
    small = start.copy()
    small[:] = 0
    small[:5] = 1
    out = _rebus(X, model, 2, small, fit=fit)
    assert (out["status"], out["iterations"], out["changed"]) == (2, 1, []) and np.array_equal(out["labels"], small) and np.isnan(out["cm"]).all() and np.isnan(out["gqi"])


# ------------------------------------------------------------------ the library and the package
def test_the_library_exports_the_entry_points():
    lib = _native.load()
    assert all(name in _native.EXPORTS and hasattr(lib, name) for name in NEW_SYMBOLS)


def frame_and_config(n=120, mode_b=False, scale=None):
    X, model, cls = planted(n, seed=1)
    lvs = ["A", "B", "C"]
    frame = pd.DataFrame(X, columns=["%s%d" % (lvs[l].lower(), i + 1) for l in range(3) for i in range(3)])
    structure = c.Structure()
    structure.add_path(["A"], ["B", "C"])
    structure.add_path(["B"], ["C"])
    config = c.Config(structure.path(), scaled=True) if scale is None else c.Config(structure.path(), default_scale=scale)
    for l, lv in enumerate(lvs):
        config.add_lv(lv, Mode.B if (mode_b and l == 1) else Mode.A, *[c.MV("%s%d" % (lv.lower(), i + 1)) for i in range(3)])
    return frame, config, cls


def test_argument_and_scope_errors_come_before_the_device():
    frame, config, cls = frame_and_config()
    for bad in (0, 17, [2, 2], []):
        with pytest.raises(ValueError, match="classes"):
            Rebus(frame, config, classes=bad, start=cls)
    with pytest.raises(ValueError, match="max_iter"):
        Rebus(frame, config, start=cls, max_iter=-1)
    with pytest.raises(ValueError, match="max_iter"):
        Rebus(frame, config, start=cls, stop_crit=float("nan"))
    with pytest.raises(ValueError, match="3 distinct labels, classes = 2"):
        Rebus(frame, config, classes=2, start=np.arange(120) % 3)
    with pytest.raises(ValueError, match="one label per row"):
        Rebus(frame, config, classes=2, start=cls[:50])
    with pytest.raises(ValueError, match="aligned on data.index"):
        Rebus(frame, config, classes=2, start=pd.Series(cls, index=np.arange(120) + 1))
    with pytest.raises(ValueError, match='start must be "ward", a Fimix object'):
        Rebus(frame, config, classes=2, start="no_such_column")
    with pytest.raises(NotImplementedError, match="Mode A blocks only: B"):
        Rebus(*frame_and_config(mode_b=True)[:2], start=cls)
    with pytest.raises(NotImplementedError, match="metric data"):
        Rebus(*frame_and_config(scale=Scale.NUM)[:2], start=cls)
    holes = frame.copy()
    holes.iloc[3, 2] = np.nan
    with pytest.raises(NotImplementedError, match="metric data without missing cells"):
        Rebus(holes, config, start=cls)
    lvs = ["A", "B", "C"]
    alone = c.Config(pd.DataFrame(0, index=lvs, columns=lvs), scaled=True)
    for lv in lvs:
        alone.add_lv(lv, Mode.A, *[c.MV("%s%d" % (lv.lower(), i + 1)) for i in range(3)])
    with pytest.raises(ValueError, match="no path"):
        Rebus(frame, alone, start=cls)


def test_start_labels_and_the_ward_refusal():
    frame, config, cls = frame_and_config()
    frame["who"] = np.where(cls == 0, "b", "a")
    assert np.array_equal(_start_labels(frame, "who", 2), 1 - cls)              # the sorted distinct values in order
    assert np.array_equal(_start_labels(frame, pd.Series(cls * 5, index=frame.index), 2), cls)
    n = 1
    while n * (n - 1) // 2 * 8 <= WARD_MAX_BYTES:
        n *= 2
    lo, hi = n // 2, n                                     # the largest N the host clustering takes, by bisection
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if mid * (mid - 1) // 2 * 8 <= WARD_MAX_BYTES else (lo, mid)
    _ward_check(lo)
    with pytest.raises(ValueError, match=r"more than 2 GiB.*a column of data.*Fimix object"):
        _ward_check(hi)
    big = pd.DataFrame(np.zeros((hi, 9)), columns=[col for col in frame.columns if col != "who"])
    with pytest.raises(ValueError, match="more than 2 GiB"):
        Rebus(big, config, classes=2)                      # start="ward" is the default: refused before anything is uploaded
