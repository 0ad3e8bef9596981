"""CPU: the option table of a handle (csrc/options.h: option_set / option_get over a bare Tune, through the emulation build in tests/hostemu/) against
tests/golden/option_table.json -- per option its default, the probe values each of the two builds accepts and what a change of it voids, recorded from the two
hand-written if-chains the table replaced; the probes are the fixture's "probes" list."""
import ctypes
import json
import os

import pytest

from helpers import GOLDEN
from helpers_gram_route import load_emu

OK, OUT_OF_RANGE, EXPERIMENTS_ONLY, UNKNOWN = range(4)
VOIDS = {"nothing": 0, "planes": 1, "planes_and_stats": 3}
KEEP = -2 ** 31           # hostemu_option_set: start from the default


@pytest.fixture(scope="module")
def emu():
    return load_emu()


@pytest.fixture(scope="module")
def table():
    with open(os.path.join(GOLDEN, "option_table.json")) as fh:
        return json.load(fh)


def option_set(lib, name, value, experiments, start=KEEP):
    """(result, effect bits, fields of Tune that changed, the option's value afterwards)"""
    out = (ctypes.c_int * 4)()
    lib.hostemu_option_set(name.encode(), start, value, int(experiments), out)
    return tuple(out)


def option_get(lib, name):
    v = ctypes.c_int(0)
    return v.value if lib.hostemu_option_get(name.encode(), ctypes.byref(v)) else None


def test_the_table_holds_the_fixtures_options_and_no_other(emu, table):
    emu.hostemu_option_name.restype = ctypes.c_char_p
    names = [emu.hostemu_option_name(i).decode() for i in range(emu.hostemu_option_count())]
    assert len(names) == 52 and sorted(names) == sorted(table["options"])
    for name, o in table["options"].items():
        assert option_get(emu, name) == o["default"], name
    for name in table["read_only"] + ["no_such_option", ""]:          # the read-outs need a handle: not in this table
        assert option_get(emu, name) is None, name
        assert option_set(emu, name, 0, True) == (UNKNOWN, 0, 0, KEEP), name


@pytest.mark.parametrize("experiments", [False, True])
def test_every_probe_is_accepted_or_refused_as_recorded(emu, table, experiments):
    for name, o in table["options"].items():
        accepted, wider = o["accepted"]["experiments" if experiments else "release"], o["accepted"]["experiments"]
        for value in table["probes"]:
            got = option_set(emu, name, value, experiments)
            if value in accepted:
                changed = value != o["default"]
                assert got == (OK, VOIDS[o["voids"]] if changed else 0, int(changed), value), (name, value, got)
            else:               # refused: Tune untouched; a value the experiments build alone takes says so
                assert got == (EXPERIMENTS_ONLY if value in wider else OUT_OF_RANGE, 0, 0, o["default"]), (name, value, got)


def test_the_effect_is_of_a_change_from_the_value_held_not_from_the_default(emu, table):
    for name, o in table["options"].items():
        for held in o["accepted"]["experiments"]:
            assert option_set(emu, name, held, True, start=held) == (OK, 0, 0, held), (name, held)
            back = option_set(emu, name, o["default"], True, start=held)
            assert back == (OK, VOIDS[o["voids"]] if held != o["default"] else 0, int(held != o["default"]), o["default"]), (name, held, back)
