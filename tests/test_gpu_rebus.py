"""GPU: REBUS-PLS (include/plspm_hip.h plspm_rebus_*; plspm.rebus) against the NumPy mirror plspm.rebus._rebus.

One-step parity isolates the new kernels: the mirror runs in fp64 and in np.longdouble on the device's own local records, and CM and the within-class sums must
lie inside the project's existing bar (helpers_fimix.bar: ten times the difference of the two mirrors, floor 1e-12 max(1, |v|)); labels are equal.  A run with
max_iter = 0 is the final pass on the start labels: its records are the local models of iteration 1, its CM the CM iteration 1 assigns by (the same kernels, the
same bits).  Whole-loop parity takes the oracle as the mirror's local estimator and demands equal status, iterations, history and labels -- after asserting that
every row's gap between its best and second-best CM is at least 1,000 times that CM's bar at every iteration, which makes exact labels a fair demand."""
import numpy as np
import pandas as pd
import pytest

import plspm.config as c
import plspm_oracle as orc
from helpers_fimix import assert_inside, bar
from helpers_rebus import ONE_PATH, TRI3, device_records, flipped, mirror_pair, native_model, oracle_fit, planted, random_start, sized
from plspm.mode import Mode
from plspm.scheme import Scheme

pytestmark = pytest.mark.gpu
E_ARG, E_STATE = 100, 101

SAT = orc.satisfaction_C()
#         id            N     C         sizes       K   min_size
SHAPES = [("n61_k1", 61, ONE_PATH, [3, 1], 1, 10),                 # below one row tile; one path; one single-item block
          ("n61_k2", 61, ONE_PATH, [3, 1], 2, 10),
          ("n257_k2", 257, SAT, [3] * 6, 2, 10),                   # one row past a tile; satisfaction-shaped model
          ("n257_k3", 257, SAT, [3] * 6, 3, 10),
          ("n257_k16", 257, ONE_PATH, [2, 2], 16, 4),              # every class the kernels take
          ("n1000_k3", 1000, SAT, [4] * 6, 3, 10)]
FLOAT_KEYS = ("cm", "within_e", "within_f", "records")


def check_step(run, m64, mld, what):
    """A device run against the mirror pair on the same local records."""
    assert run["status"] == m64["status"] == mld["status"] and run["iterations"] == m64["iterations"], what
    assert np.array_equal(run["labels"], m64["labels"]) and np.array_equal(m64["labels"], mld["labels"]), what
    assert np.array_equal(run["sizes"], m64["sizes"]) and list(run["changed"]) == m64["changed"], what
    if m64["status"] == 2:
        assert all(np.isnan(run[key]).all() for key in FLOAT_KEYS), what
        return
    assert_inside(run["cm"], m64["cm"], mld["cm"], what + " CM")
    assert_inside(run["within_e"], m64["within_e"], mld["within_e"], what + " within e")
    assert_inside(run["within_f"], m64["within_f"], mld["within_f"], what + " within f")


def one_step(nm, X, model, K, start, min_size):
    """max_iter = 0 (the final pass on the start labels), then max_iter = 1, each against the mirror pair on the device's own records.  Returns both runs."""
    run0 = nm.rebus(K, start, max_iter=0, min_size=min_size)
    assert run0["status"] == 1 and run0["iterations"] == 0 and np.array_equal(run0["labels"], start) and len(run0["changed"]) == 0
    rec0 = device_records(nm, run0)
    check_step(run0, *mirror_pair(X, model, K, start, max_iter=0, min_size=min_size, records=[rec0]), "final pass on the start")
    run1 = nm.rebus(K, start, max_iter=1, stop_crit=0.005, min_size=min_size)
    rec1 = device_records(nm, run1) if run1["status"] != 2 else [None] * K
    m64, mld = mirror_pair(X, model, K, start, max_iter=1, stop_crit=0.005, min_size=min_size, records=[rec0, rec1])
    # the labels of iteration 1 are the argmin of the CM the first call reported
    assert np.array_equal(run1["labels"], np.argmin(run0["cm"], axis=1))
    check_step(run1, m64, mld, "one iteration")
    return run0, run1


@pytest.mark.parametrize("name,N,C,sizes,K,min_size", SHAPES, ids=[s[0] for s in SHAPES])
def test_one_step_parity(name, N, C, sizes, K, min_size):
    X, model = sized(N, C, sizes, seed=1)
    start = random_start(N, K, seed=1)
    nm = native_model(X, model)
    run0, run1 = one_step(nm, X, model, K, start, min_size)
    assert run1["status"] != 2, "the case is meant to stay valid through one iteration"
    assert nm.get_option("last_rebus_loads") == 1
    if name == "n1000_k3":
        # once more with one class per LDS load: three loads per tile, every output bit-equal
        capped = native_model(X, model, rebus_classes=1)
        for run, want in ((capped.rebus(K, start, max_iter=0, min_size=min_size), run0), (capped.rebus(K, start, max_iter=1, min_size=min_size), run1)):
            assert capped.get_option("last_rebus_loads") == 3
            for key in FLOAT_KEYS + ("labels", "sizes", "changed", "hist_sizes", "rec_status", "rec_iters"):
                assert np.array_equal(run[key], want[key], equal_nan=key in FLOAT_KEYS), key
        capped.close()
    nm.close()


@pytest.mark.parametrize("seed,K", [(1, 2), (2, 3)])
def test_whole_loop_parity_with_the_oracle_as_local_estimator(seed, K):
    X, model, cls = planted(257, seed=seed)
    start = flipped(cls, 0.25, seed=3) if K == 2 else random_start(257, K, seed=seed)
    kw = dict(max_iter=30, stop_crit=0.005, min_size=10)
    m64, mld = mirror_pair(X, model, K, start, fit=oracle_fit(model), **kw)
    # the condition that makes exact labels a fair demand, on the checker alone
    assert m64["status"] == mld["status"] == 0 and m64["changed"] == mld["changed"]
    for t, (c64, cld) in enumerate(zip(m64["cm_trace"] + [m64["cm"]], mld["cm_trace"] + [mld["cm"]])):
        order = np.sort(c64, axis=1)
        gap, best = order[:, 1] - order[:, 0], np.argmin(c64, axis=1)
        b = bar(c64, cld)[np.arange(len(best)), best]
        print("iteration %d: smallest gap %.3g, largest bar %.3g" % (t + 1, gap.min(), b.max()))
        assert np.all(gap >= 1000 * b), t
    nm = native_model(X, model)
    run = nm.rebus(K, start, **kw)
    assert (run["status"], run["iterations"]) == (m64["status"], m64["iterations"])
    assert list(run["changed"]) == m64["changed"] and np.array_equal(run["hist_sizes"], np.array(m64["hist_sizes"]))
    assert np.array_equal(run["labels"], m64["labels"]) and np.array_equal(run["sizes"], m64["sizes"])
    assert np.all(run["rec_status"] == 0)
    for k, (dev, ref) in enumerate(zip(device_records(nm, run), m64["records"])):          # the tolerances smoke() uses for a fit
        assert run["rec_iters"][k] == ref["iterations"]
        np.testing.assert_allclose(dev["weights"], ref["weights"], rtol=1e-8)
        np.testing.assert_allclose(dev["path_coef"], ref["path_coef"], rtol=1e-8, atol=1e-11)
        np.testing.assert_allclose(dev["loadings"], ref["loadings"], rtol=1e-8, atol=1e-11)
        np.testing.assert_allclose(dev["r2"], ref["r2"], rtol=1e-8, atol=1e-11)
    nm.close()


def test_status_two_keeps_labels_and_history():
    X, model = sized(257, TRI3, [3, 3, 3], seed=2)
    nm = native_model(X, model)
    # a start with a class below min_size: iteration 1 ends the run, nothing ran
    start = np.zeros(257, dtype=np.int64)
    start[:5] = 1
    run = nm.rebus(2, start, max_iter=5, min_size=10)
    assert (run["status"], run["iterations"]) == (2, 1) and np.array_equal(run["labels"], start) and len(run["changed"]) == 0
    assert list(run["sizes"]) == [252, 5] and np.all(run["rec_status"] == -1)
    assert all(np.isnan(run[key]).all() for key in FLOAT_KEYS)
    nm.close()
    # a class with a constant column: the local model has no estimate for it
    Xc = X.copy()
    start = random_start(257, 2, seed=4)
    Xc[start == 1, 4] = 3.25
    nm = native_model(Xc, model)
    run = nm.rebus(2, start, max_iter=5, min_size=10)
    assert (run["status"], run["iterations"]) == (2, 1) and np.array_equal(run["labels"], start) and len(run["changed"]) == 0
    assert all(np.isnan(run[key]).all() for key in FLOAT_KEYS)
    # ... and met in the final pass (no iteration: nothing to keep but the labels)
    last = nm.rebus(2, start, max_iter=0, min_size=10)
    assert (last["status"], last["iterations"]) == (2, 0) and np.array_equal(last["labels"], start)
    nm.close()


def test_a_repeated_call_gives_the_same_bits_and_a_bootstrap_keeps_its_records():
    X, model, cls = planted(257, seed=1)
    start = flipped(cls, 0.25, seed=3)
    nm = native_model(X, model)
    rows, status, iters = (a.copy() for a in nm.bootstrap(64, seed=3))
    first = nm.rebus(2, start, max_iter=30)
    again = nm.rebus(2, start, max_iter=30)
    for key in FLOAT_KEYS + ("labels", "sizes", "changed", "hist_sizes", "rec_status", "rec_iters"):
        assert np.array_equal(first[key], again[key], equal_nan=key in FLOAT_KEYS), key
    assert (first["status"], first["iterations"]) == (again["status"], again["iterations"])
    e, f = nm.rebus_residuals()
    e2, f2 = nm.rebus_residuals()
    assert np.array_equal(e, e2) and np.array_equal(f, f2)
    kept = nm.fetch(0, 64)
    assert np.array_equal(kept[0], rows) and np.array_equal(kept[1], status) and np.array_equal(kept[2], iters)
    nm.close()


def test_one_class_residuals_against_the_mirror():
    """plspm_rebus_residuals: e and f of the one-class model, against the mirror on the device's own record (K = 1, max_iter = 0)."""
    from plspm.rebus import _class_residuals
    X, model = sized(257, SAT, [3] * 6, seed=3)
    nm = native_model(X, model)
    e, f = nm.rebus_residuals()
    run = nm.rebus(1, np.zeros(257, dtype=np.int64), max_iter=0)
    rec = device_records(nm, run)[0]
    rows = np.ones(257, dtype=bool)
    E64, F64 = _class_residuals(X, model.blocks, model.C, True, rows, rec, np.float64)[:2]
    Eld, Fld = _class_residuals(X.astype(np.longdouble), model.blocks, model.C, True, rows, rec, np.longdouble)[:2]
    assert_inside(e, E64, Eld, "e")
    assert_inside(f, F64, Fld, "f")
    assert_inside(run["within_e"][0], (E64 ** 2).sum(axis=0), (Eld ** 2).sum(axis=0), "sum e^2")
    nm.close()


def test_handle_state_and_argument_errors():
    from plspm import _native
    X, model = sized(61, ONE_PATH, [3, 2], seed=1)
    start = random_start(61, 2, seed=1)
    nm = native_model(X, model)
    with pytest.raises(_native.NativeBackendError, match=r"\(%d\)" % E_STATE):
        nm.rebus_fetch()
    nm.rebus(2, start, max_iter=1)
    nm.upload(X)                                            # an upload voids the state
    with pytest.raises(_native.NativeBackendError, match=r"\(%d\)" % E_STATE):
        nm.rebus_fetch()
    for K in (0, 17):
        with pytest.raises(_native.NativeBackendError, match=r"\(%d\)" % E_ARG):
            nm.rebus(K, start)
    bad = start.copy()
    bad[7] = 2
    with pytest.raises(_native.NativeBackendError, match=r"\(%d\)" % E_ARG):
        nm.rebus(2, bad)
    nm.close()
    mode_b = orc.Model(model.blocks, model.C, "AB", "path", True)
    nb = native_model(X, mode_b)
    with pytest.raises(_native.NativeBackendError, match=r"\(%d\).*Mode A" % E_ARG):
        nb.rebus(2, start)
    with pytest.raises(_native.NativeBackendError, match=r"\(%d\).*Mode A" % E_ARG):
        nb.rebus_residuals()
    nb.close()
    fresh = _native.NativeModel(np.array([0, 3, 5], dtype=np.int32), ONE_PATH.astype(np.uint8), np.zeros(2, dtype=np.int32), 2, True, 100, 1e-6, 0)
    with pytest.raises(_native.NativeBackendError, match=r"\(%d\)" % E_STATE):
        fresh._check(fresh._lib.plspm_rebus_residuals(fresh._h, np.empty(1).ctypes.data), "plspm_rebus_residuals")
    fresh.close()


def planted_frame(n, seed):
    X, model, cls = planted(n, seed=seed)
    lvs = ["A", "B", "C"]
    frame = pd.DataFrame(X, columns=["%s%d" % (lvs[l].lower(), i + 1) for l in range(3) for i in range(3)])
    structure = c.Structure()
    structure.add_path(["A"], ["B", "C"])
    structure.add_path(["B"], ["C"])
    config = c.Config(structure.path(), scaled=True)
    for l, lv in enumerate(lvs):
        config.add_lv(lv, Mode.A, *[c.MV("%s%d" % (lv.lower(), i + 1)) for i in range(3)])
    return frame, config, cls


def test_the_api_on_planted_data():
    from plspm.fimix import Fimix
    from plspm.mga import GroupComparison
    from plspm.rebus import Rebus
    frame, config, cls = planted_frame(400, seed=1)
    frame["start"] = np.where(flipped(cls, 0.2, seed=3) == 0, "x", "y")
    rb = Rebus(frame, config, classes=2, start="start")
    names, mvs = ["class.1", "class.2"], [col for col in frame.columns if col != "start"]
    assert rb.status()["status"] == 0 and 1 <= rb.status()["iterations"] <= 100
    sizes = rb.sizes()
    assert list(sizes.index) == names and sizes.sum() == 400 and sizes.iloc[0] >= sizes.iloc[1]
    seg = rb.segments()
    assert seg.name == "group" and seg.index.equals(frame.index) and sorted(seg.unique()) == [1, 2] and (seg == 1).sum() == sizes.iloc[0]
    assert list(rb.path_coefficients().index) == ["A -> B", "A -> C", "B -> C"] and list(rb.path_coefficients().columns) == names
    assert list(rb.loadings().index) == mvs and list(rb.weights().index) == mvs and list(rb.loadings().columns) == names
    assert list(rb.r_squared().index) == ["B", "C"] and list(rb.r_squared().columns) == names
    cm = rb.closeness()
    assert cm.shape == (400, 2) and cm.index.equals(frame.index) and np.isfinite(cm.values).all()
    hist = rb.history()
    assert list(hist.columns) == ["changed"] + names and len(hist) == rb.status()["iterations"] and hist.index.name == "iteration"
    assert list(hist.iloc[-1][names]) == list(sizes)
    assert rb.residuals().shape == (400, 11) and list(rb.residuals().columns) == mvs + ["B", "C"]
    q = rb.quality()
    assert list(q.index) == names + ["gqi", "one.class"] and list(q.columns) == ["size", "communality", "r_squared", "root"]
    assert q.loc["gqi", "root"] > q.loc["one.class", "root"] and rb.gqi() == q.loc["gqi", "root"]
    # segments() is a group column
    data = frame.drop(columns="start")
    GroupComparison(data, config, seg, permutations=64, seed=1).paths()
    # the other two forms of start
    ward = Rebus(data, config, classes=[2, 3], start="ward", max_iter=20)
    assert ward.sizes(2).sum() == 400 and ward.sizes(3).sum() == 400 and ward.status(3)["status"] in (0, 1, 2)
    with pytest.raises(ValueError, match="K must be one of"):
        ward.sizes()
    fm = Fimix(data, config, segments=[2], starts=2, seed=1)
    assert Rebus(data, config, classes=2, start=fm, max_iter=20).sizes().sum() == 400
