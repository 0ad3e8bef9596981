"""Shared by the MICOM tests (tests/test_gpu_micom.py): the NumPy mirror (plspm.micom._micom) in fp64 and np.longdouble on one split, the restatement of the
counts and p-values on fetched records, and the figure behind the bar of the comparison with the oracle's fits."""
import numpy as np

from plspm.micom import _micom


def dev_blocks(model):
    """The LV blocks in device column order (MVs grouped by LV, path order): consecutive ranges."""
    off = np.concatenate(([0], np.cumsum([len(b) for b in model.blocks])))
    return [np.arange(off[l], off[l + 1]) for l in range(model.L)]


def mirror_pair(Xdev, member, w_a, w_b, w_0, blocks):
    """(fp64 record, longdouble record) of the mirror on the same inputs."""
    return _micom(Xdev, member, w_a, w_b, w_0, blocks, np.float64), _micom(Xdev, member, w_a, w_b, w_0, blocks, np.longdouble)


def mirror_bar(m64, mld, floor=1e-12):
    """Ten times the largest difference between the fp64 and the longdouble mirror on the same inputs, at least `floor` (absolute)."""
    return max(10.0 * float(np.max(np.abs(m64.astype(np.longdouble) - mld))), floor)


def counts(records, status, observed):
    """(below, exceed, used) on fetched MICOM records: #{valid r : x_r <= obs}, #{valid r : |x_r| >= |obs|} per column (NaN on either side: neither)."""
    x = records[status == 0]
    with np.errstate(invalid="ignore"):
        below = (x <= observed[None, :]).sum(axis=0).astype(np.int64)
        exceed = (np.abs(x) >= np.abs(observed)[None, :]).sum(axis=0).astype(np.int64)
    return below, exceed, int(x.shape[0])


def p_values(below, exceed, used, observed, L):
    p = (1.0 + np.concatenate((below[:L], exceed[L:]))) / (1.0 + used)
    p[np.isnan(observed)] = np.nan
    return p


def perturbation_figure(Xdev, member, w_a, w_b, w_0, blocks, draws=20, rtol=1e-8, atol=1e-11, seed=0):
    """How far the MICOM values move when the three weight vectors move inside the record bar (|d| <= atol + rtol |w|, uniform draws): the largest absolute
    change of any value over the draws."""
    rng = np.random.default_rng(seed)
    base = _micom(Xdev, member, w_a, w_b, w_0, blocks)
    worst = 0.0
    for _ in range(draws):
        moved = _micom(Xdev, member, *(v + rng.uniform(-1.0, 1.0, v.shape[0]) * (atol + rtol * np.abs(v)) for v in (w_a, w_b, w_0)), blocks)
        worst = max(worst, float(np.max(np.abs(moved - base))))
    return worst
