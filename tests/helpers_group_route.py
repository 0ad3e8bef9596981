"""Shared by the CPU table test of the group driver's plan (tests/test_group_route.py) and the GPU test that ties the plan to what a group runs (tests/test_gpu_dist.py):
the plan of a call through the emulation build in tests/hostemu/ (hostemu_group_plan: csrc/group_route.h group_plan, group_shard, group_segment)."""
import ctypes

import numpy as np

from helpers_gram_route import load_emu  # noqa: F401  (the tests' fixture)

CHUNKS_MAX = 8


def plan(lib, B, nranks, RS, chunks=0, ratio=50, align=0, units=64, nothing_to_hide=None):
    """group_plan of a call of B replicates on nranks ranks with records of RS doubles under the options chunks / ratio ("chunk_ratio") / align ("chunk_align"); units: the
    alignment the ranks agreed on; nothing_to_hide: one rank (the default), or ranks that share a device.  subs: (first, B, cap, off) per sub-batch; segments[k][rank]:
    (rec0, first, count) in the receive buffer; shards[k][rank]: (first within the sub-batch, count, full)."""
    nth = nranks == 1 if nothing_to_hide is None else nothing_to_hide
    arg = np.array([B, nranks, RS, chunks, ratio, align, units, nth], dtype=np.int64)
    out = np.full(6 + 4 * CHUNKS_MAX + 5 * CHUNKS_MAX * nranks, -1, dtype=np.int64)
    lib.hostemu_group_plan(arg.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p))
    v = [int(x) for x in out]
    K = v[0]
    assert v[5] == CHUNKS_MAX and 1 <= K <= CHUNKS_MAX
    per = [v[6 + 4 * K + 5 * i:6 + 4 * K + 5 * (i + 1)] for i in range(K * nranks)]
    return dict(K=K, cap=v[1], send_bytes=v[2], recv_bytes=v[3], consults_units=v[4], subs=[tuple(v[6 + 4 * k:10 + 4 * k]) for k in range(K)],
                segments=[[tuple(per[k * nranks + r][:3]) for r in range(nranks)] for k in range(K)],
                shards=[[(per[k * nranks + r][3], per[k * nranks + r][2], per[k * nranks + r][4]) for r in range(nranks)] for k in range(K)])
