"""GPU: the handle's host side in plspm_hip.hip -- options through the table of csrc/options.h on a live handle (against tests/golden/option_table.json, the
fixture of tests/test_options.py), what a changed option voids, and the ownership of device blocks (plspm_model::Buf): every handle kind created, used and
destroyed twice over with the allocator's cache emptied in between.  No test here asserts on numbers of its own: the kinds' results are checked where the kinds
are tested; here two rounds must agree bit for bit."""
import ctypes
import json
import os

import numpy as np
import pytest

import plspm_oracle as orc
from helpers import GOLDEN

pytestmark = pytest.mark.gpu
E_ARG = 100
TRI3 = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0]], dtype=np.int64)


def plain(n=64, mvs=2, seed=4):
    """n x (3 mvs) synthetic data on a three-LV model, uploaded."""
    from plspm import _native
    X, blocks = orc.synth(n, TRI3, mvs, seed=seed)
    boff = np.concatenate(([0], np.cumsum([len(b) for b in blocks]))).astype(np.int32)
    nm = _native.NativeModel(boff, TRI3.astype(np.uint8), np.zeros(3, dtype=np.int32), 0, True, 100, 1e-6, 0)
    nm.upload(X)
    return nm


@pytest.fixture(scope="module")
def table():
    with open(os.path.join(GOLDEN, "option_table.json")) as fh:
        return json.load(fh)


def test_options_on_a_live_handle_follow_the_recorded_table(table):
    """One handle with no data, no kernel: every probe of every option is accepted or refused as the fixture records for the build that is loaded, a refusal
    with its text and the value left alone; the read-only names answer 0 on a fresh handle (boot_round_units: 64, no digit planes yet) and cannot be set."""
    from plspm import _native
    nm = _native.NativeModel(np.array([0, 2, 4, 6], dtype=np.int32), TRI3.astype(np.uint8), np.zeros(3, dtype=np.int32), 0, True, 100, 1e-6, 0)
    lib, h = nm._lib, nm._h
    error = lambda: lib.plspm_last_error(h).decode()
    experiments = nm.get_option("build_experiments")
    assert experiments in (0, 1)
    for name in table["read_only"]:
        if name != "build_experiments":
            assert nm.get_option(name) == (64 if name == "boot_round_units" else 0), name
        assert lib.plspm_model_set_option(h, name.encode(), 0) == E_ARG and error() == "plspm_model_set_option: unknown option '%s'" % name
    for name, o in table["options"].items():
        accepted, wider = o["accepted"]["experiments" if experiments else "release"], o["accepted"]["experiments"]
        assert nm.get_option(name) == o["default"], name
        held = o["default"]
        for value in table["probes"]:
            rc = lib.plspm_model_set_option(h, name.encode(), value)
            if value in accepted:
                assert rc == 0, (name, value, error())
                held = value
            else:
                assert rc == E_ARG, (name, value)
                if value in wider:
                    assert error() == "plspm_model_set_option: this value of '%s' names a variant of the experiments build (make experiments; PLSPM_HIP_LIB)" % name
                else:
                    assert error() == "plspm_model_set_option: value out of range for '%s'" % name
            assert nm.get_option(name) == held, (name, value)
        nm.set_option(name, o["default"])
    v = ctypes.c_int32(0)
    assert lib.plspm_model_get_option(h, b"no_such_option", ctypes.byref(v)) == E_ARG
    assert lib.plspm_model_set_option(h, b"no_such_option", 0) == E_ARG and error() == "plspm_model_set_option: unknown option 'no_such_option'"
    nm.close()


@pytest.mark.parametrize("fixed", [6, 0], ids=["six_planes", "automatic_count"])
@pytest.mark.parametrize("name,other", [("i8_slices", 7), ("i8_ind", 0)])
def test_a_changed_plane_option_voids_the_digit_planes_and_the_same_value_does_not(name, other, fixed):
    """64 x 6.  With a fixed plane count plspm_bootstrap_prepare cuts the planes itself; with the automatic count it only enqueues the column statistics, and the
    first bootstrap call cuts them."""
    nm = plain()
    nm.set_option("i8_slices", fixed)
    nm.prepare_bootstrap()
    if not fixed:
        assert nm.get_option("last_i8_slices") == 0
        nm.bootstrap(16, seed=1)
    planes = nm.get_option("last_i8_slices")
    assert planes == fixed if fixed else planes > 0
    nm.set_option(name, nm.get_option(name))
    assert nm.get_option("last_i8_slices") == planes
    assert other != nm.get_option(name)
    nm.set_option(name, other)
    assert nm.get_option("last_i8_slices") == 0
    nm.close()


# ---- ownership: create, upload, one call, destroy -- twice, the second time on blocks the first round gave back; then the cache goes back to the runtime
def round_plain():
    nm = plain()
    out = nm.bootstrap(32, seed=2)
    nm.close()
    return out


def round_missing():
    from test_gpu_missing import gpu_model
    X, blocks = orc.synth(60, TRI3, 4, seed=6)
    X[[3, 17, 40], 2] = np.nan
    X[[5, 17], 9] = np.nan
    nm, _ = gpu_model(X, orc.Model(blocks, TRI3, "AAA", "centroid", True))
    out = nm.bootstrap(32, seed=2)
    nm.close()
    return out


def round_categorical():
    from test_gpu_categorical import gpu_fit_cat
    from test_oracle_golden import RUSSA_C, RUSSA_CAT_BLOCKS, RUSSA_CAT_SCALES, russa_cat_inputs
    nm, fit = gpu_fit_cat(russa_cat_inputs(), orc.Model(RUSSA_CAT_BLOCKS, RUSSA_C, "AAA", "centroid", True, tol=1e-7, scales=RUSSA_CAT_SCALES))
    out = (fit["weights"], fit["scores"]) + tuple(nm.bootstrap(16, seed=2))
    nm.close()
    return out


def round_hoc(first_goes_first):
    from test_gpu_hoc import handles
    first, second, *_ = handles("path_B")
    first.attach_second_stage(second, [0, 1, 2, 4, 5, 6])
    out = first.bootstrap(16, seed=2)
    for handle in ((first, second) if first_goes_first else (second, first)):
        handle.close()
    return out


def round_group():
    """Two handles on one device as the two ranks of a group; one handle is destroyed while the group still holds it."""
    from plspm import _native
    models = [plain(), plain()]
    comm = _native.NativeComm([0, 0])
    group = _native.NativeGroup(comm, models)
    group.bootstrap(33, seed=2)
    out = group.rows()
    models[1].close()
    group.close(); comm.close()
    models[0].close()
    return out


@pytest.mark.parametrize("one_round", [round_plain, round_missing, round_categorical, lambda: round_hoc(True), lambda: round_hoc(False), round_group],
                         ids=["plain", "missing", "categorical", "hoc_first_stage_first", "hoc_second_stage_first", "group"])
def test_a_handle_kind_lives_twice_on_the_same_blocks(one_round):
    from plspm import _native
    once = one_round()
    again = one_round()
    assert len(once) == len(again) and all(np.array_equal(a, b, equal_nan=True) for a, b in zip(once, again))
    assert _native.load().plspm_release_cached_memory() == 0
