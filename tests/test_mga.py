"""CPU: the two-group permutation test's host surface -- the split of a permutation (plspm_permutation_members, the host mirror of the
device's splits) against the NumPy restatement of its definition (tests/helpers_mga.py), the new C-ABI symbols, and the argument checks of
plspm.mga.GroupComparison, which all happen before anything runs on a device."""
import numpy as np
import pandas as pd
import pytest

import plspm.config as c
from plspm import _native
from plspm.mga import GroupComparison
from plspm.mode import Mode
from plspm.scale import Scale
from plspm.scheme import Scheme

from helpers import SAT_ADD_ORDER, SAT_PREFIX, satisfaction_frame
from helpers_mga import find_tie, permutation_keys, permutation_members


@pytest.mark.parametrize("seed,perm,n,n1", [(0, 0, 250, 148), (7, 3, 250, 10), (7, 4, 250, 240), (0xC0FFEE, 12345, 10000, 5000),
                                            (2 ** 63 + 5, 2 ** 33 + 1, 10000, 2000), (11, 1, 70001, 10), (11, 2, 70001, 69991), (99, 5, 131075, 40000)])
def test_members_match_the_numpy_philox_restatement(seed, perm, n, n1):
    mine = _native.permutation_members(seed, perm, n, n1)
    assert mine.dtype == bool and mine.shape == (n,)
    assert int(mine.sum()) == n1
    assert np.array_equal(mine, permutation_members(seed, perm, n, n1))


def test_members_break_key_ties_by_row():
    """Where two rows share a key and the cut falls between them, the lower row index is the member."""
    found = find_tie(5, 200000, range(4))
    assert found is not None
    perm, n1 = found
    keys = permutation_keys(5, perm, 200000)
    mine = _native.permutation_members(5, perm, 200000, n1)
    assert np.array_equal(mine, permutation_members(5, perm, 200000, n1))
    thr = keys[mine].max()
    tied = np.flatnonzero(keys == thr)
    assert tied.size >= 2 and mine[tied[0]] and not mine[tied[-1]]


def test_permutation_stream_is_not_the_bootstrap_stream():
    """Counter word 1 = 1: the keys are not the words the bootstrap's draws of the same (seed, replicate) come from."""
    from helpers_mga import philox4x32_10
    q = np.arange(64, dtype=np.uint64)
    boot = np.stack(philox4x32_10(q, 0, 3, 0, 9, 0), axis=1).reshape(-1).astype(np.uint32)
    assert not np.array_equal(permutation_keys(9, 3, 256), boot)
    idx = _native.bootstrap_indices(9, 3, 256)                              # the bootstrap mirror maps exactly those words to rows
    assert np.array_equal(idx, ((boot.astype(np.uint64) * np.uint64(256)) >> np.uint64(32)).astype(np.int32))


def test_members_reject_bad_sizes():
    lib = _native.load()
    out = np.empty(10, dtype=np.uint8)
    for n, n1 in ((10, 0), (10, 10), (1, 1)):
        assert lib.plspm_permutation_members(1, 0, n, n1, out.ctypes.data) != 0


def test_new_symbols_are_exported_and_declared():
    lib = _native.load()
    for name in ("plspm_permutation_device", "plspm_permutation_counts", "plspm_permutation_members"):
        assert name in _native.EXPORTS
        assert hasattr(lib, name)
    assert lib.plspm_abi_version() == 4


# ------------------------------------------------------------------ GroupComparison: argument checks (no device needed)
def _sat():
    sat = satisfaction_frame()
    s = c.Structure()
    s.add_path(["IMAG"], ["EXPE", "SAT", "LOY"]); s.add_path(["EXPE"], ["QUAL", "VAL", "SAT"])
    s.add_path(["QUAL"], ["VAL", "SAT"]); s.add_path(["VAL"], ["SAT"]); s.add_path(["SAT"], ["LOY"])
    cfg = c.Config(s.path(), scaled=False)
    for lv in SAT_ADD_ORDER:
        cfg.add_lv_with_columns_named(lv, Mode.A, sat, SAT_PREFIX[lv])
    return sat, cfg


def test_group_needs_two_labels():
    sat, cfg = _sat()
    three = sat["gender"].where(sat.index % 3 != 0, "other")
    with pytest.raises(ValueError, match="two distinct"):
        GroupComparison(sat, cfg, three, Scheme.PATH, permutations=10, seed=1)
    with pytest.raises(ValueError, match="two distinct"):
        GroupComparison(sat, cfg, pd.Series("female", index=sat.index), Scheme.PATH, permutations=10, seed=1)


def test_group_needs_ten_rows_each():
    sat, cfg = _sat()
    lab = pd.Series(np.where(np.arange(len(sat)) < 9, "x", "y"), index=sat.index)
    with pytest.raises(ValueError, match="at least 10 rows"):
        GroupComparison(sat, cfg, lab, Scheme.PATH, permutations=10, seed=1)


def test_group_rejects_missing_labels():
    sat, cfg = _sat()
    lab = sat["gender"].copy()
    lab.iloc[17] = np.nan
    with pytest.raises(ValueError, match="no label"):
        GroupComparison(sat, cfg, lab, Scheme.PATH, permutations=10, seed=1)
    df = sat.copy()
    df.loc[df.index[3], "gender"] = None
    with pytest.raises(ValueError, match="no label"):
        GroupComparison(df, cfg, "gender", Scheme.PATH, permutations=10, seed=1)


def test_group_rejects_a_misaligned_series():
    sat, cfg = _sat()
    with pytest.raises(ValueError, match="aligned"):
        GroupComparison(sat, cfg, sat["gender"].iloc[::-1], Scheme.PATH, permutations=10, seed=1)
    with pytest.raises(ValueError, match="aligned"):
        GroupComparison(sat, cfg, sat["gender"].iloc[:-1], Scheme.PATH, permutations=10, seed=1)
    with pytest.raises(ValueError, match="column label"):
        GroupComparison(sat, cfg, "sex", Scheme.PATH, permutations=10, seed=1)


def test_models_outside_the_scope_raise_not_implemented():
    sat, cfg = _sat()
    # Scale.NUM
    s = cfg.path()
    num = c.Config(s, scaled=True, default_scale=Scale.NUM)
    for lv in SAT_ADD_ORDER:
        num.add_lv_with_columns_named(lv, Mode.A, sat, SAT_PREFIX[lv])
    with pytest.raises(NotImplementedError):
        GroupComparison(sat, num, "gender", Scheme.PATH, permutations=10, seed=1)
    # missing cells
    holes = sat.copy()
    holes.iloc[5, 2] = np.nan
    _, cfg2 = _sat()
    with pytest.raises(NotImplementedError):
        GroupComparison(holes, cfg2, "gender", Scheme.PATH, permutations=10, seed=1)
    # a higher-order construct
    st = c.Structure()
    st.add_path(["IMAG"], ["H"]); st.add_path(["H"], ["LOY"])
    hoc = c.Config(st.path(), default_scale=Scale.NUM)
    hoc.add_higher_order("H", Mode.A, ["SAT", "VAL"])
    for lv in ("IMAG", "SAT", "VAL", "LOY"):
        hoc.add_lv_with_columns_named(lv, Mode.A, sat, SAT_PREFIX[lv])
    with pytest.raises(NotImplementedError):
        GroupComparison(sat, hoc, "gender", Scheme.PATH, permutations=10, seed=1)
