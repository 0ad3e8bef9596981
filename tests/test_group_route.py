"""CPU check of the group driver's plan (csrc/group_route.h: chunk_plan, group_plan, group_shard, group_segment -- how many collectives every rank of a job issues and of
what sizes) through the emulation build in tests/hostemu/: an explicit table with a row for every rule, then the properties every plan has, on a grid.  The expected
values are what plspm_group_bootstrap computed before the plan had a function of its own, worked out by hand from its formulas:

    a call is cut per rank: ceil(B / nranks) replicates in n parts, n = "chunks" (0: one part below 2 MiB of records, else three), at most 8, and no more than
    (per_rank + align / 2) / max(512, align) of them; part k is per_rank q^k / (1 + q + .. + q^(n-1)) rounded to the nearest multiple of the alignment (one at least),
    the last part the remainder -- unless that remainder would fall below min(align, 64): then the cutting stops and the part before takes it
    a sub-batch is nranks times its part (the last one: what is left of B); cap = ceil(sub-batch / nranks) records per rank; off = the caps before it
    headline, 5,000 per rank at q = 0.5 in rounds of 1,280: 5000 / 1.75 = 2857.1 -> 2,560; 1428.6 -> 1,280; left 1,160.  Records of 140 doubles: 5.6 MB per rank
"""
import pytest

from helpers_group_route import CHUNKS_MAX, load_emu, plan


@pytest.fixture(scope="module")
def emu():
    return load_emu()


def subs(nranks, *parts, B=None):
    """The sub-batches of a call whose per-rank parts are `parts` (the last sub-batch: what is left of B)."""
    out, at, off = [], 0, 0
    for k, p in enumerate(parts):
        size = p * nranks if k < len(parts) - 1 or B is None else B - at
        cap = -(-size // nranks)
        out.append((at, size, cap, off))
        at += size; off += cap
    return out


RS = 140                                           # bench.py's model: 1,120 bytes per record, 2 MiB = 1,872.5 of them
# (id, arguments of plan(), expected)
PLANS = [
    ("B 1, one rank", dict(B=1, nranks=1, RS=RS), dict(K=1, cap=1, subs=[(0, 1, 1, 0)], send_bytes=1120, recv_bytes=1120, consults_units=0, shards=[[(0, 1, 1)]], segments=[[(0, 0, 1)]])),
    ("B 2 on three ranks: an empty shard, cap 1", dict(B=2, nranks=3, RS=RS), dict(K=1, cap=1, subs=[(0, 2, 1, 0)], recv_bytes=3 * 1120, shards=[[(0, 1, 1), (1, 1, 1), (2, 0, 0)]],
                                                                              segments=[[(0, 0, 1), (1, 1, 1), (2, 2, 0)]])),
    ("B 7 on three ranks: ragged, only the first shard is full", dict(B=7, nranks=3, RS=RS), dict(K=1, cap=3, subs=[(0, 7, 3, 0)], shards=[[(0, 3, 1), (3, 2, 0), (5, 2, 0)]],
                                                                                                segments=[[(0, 0, 3), (3, 3, 2), (6, 5, 2)]])),
    ("B a multiple of the ranks: every shard full", dict(B=6, nranks=3, RS=RS), dict(K=1, cap=2, shards=[[(0, 2, 1), (2, 2, 1), (4, 2, 1)]])),
    # ---- the remainder rule
    ("1,023 in two parts at q 0.1: 930 -> 960, the remainder 63 is no part", dict(B=1023, nranks=1, RS=RS, chunks=2, ratio=10, align=64), dict(K=1, subs=[(0, 1023, 1023, 0)])),
    ("1,024: the remainder 64 is one", dict(B=1024, nranks=1, RS=RS, chunks=2, ratio=10, align=64), dict(K=2, subs=subs(1, 960, 64))),
    ("1,600 in three at q 0.1: 1441 -> 1,472, 144 -> 128 would leave 0: the second part takes the rest", dict(B=1600, nranks=1, RS=RS, chunks=3, ratio=10, align=64), dict(K=2, subs=subs(1, 1472, 128))),
    ("the same per rank on four ranks, B not a multiple", dict(B=4 * 1600 - 3, nranks=4, RS=RS, chunks=3, ratio=10, align=64, nothing_to_hide=0),
     dict(K=2, cap=1600, subs=[(0, 4 * 1472, 1472, 0), (4 * 1472, 4 * 128 - 3, 128, 1472)])),
    # ---- the number of parts
    ("chunks 0, 1,872 records per rank: below 2 MiB, one part", dict(B=3744, nranks=2, RS=RS, align=64), dict(K=1, cap=1872, consults_units=0)),
    ("chunks 0, 1,873 per rank: three parts 1070 -> 1,088, 535 -> 512, 273", dict(B=3745, nranks=2, RS=RS, align=64), dict(K=3, cap=1873, subs=subs(2, 1088, 512, 273, B=3745))),
    ("chunks 0 without an alignment option consults the agreed units", dict(B=3745, nranks=2, RS=RS), dict(K=3, consults_units=1)),
    ("chunks 1: one part, no agreement needed", dict(B=40000, nranks=8, RS=RS, chunks=1), dict(K=1, cap=5000, consults_units=0, subs=[(0, 40000, 5000, 0)])),
    ("chunks 8 of 5,000 per rank: the seventh cut would leave 8", dict(B=40000, nranks=8, RS=RS, chunks=8, align=64), dict(K=7, cap=5000, subs=subs(8, 2496, 1280, 640, 320, 128, 64, 72))),
    ("chunks 8 of 50,000 per rank: eight parts", dict(B=400000, nranks=8, RS=RS, chunks=8, align=64), dict(K=8, cap=50000, subs=subs(8, 25088, 12544, 6272, 3136, 1600, 768, 384, 208))),
    ("no part below 512 units: 1,500 per rank gives two of the three asked for", dict(B=3000, nranks=2, RS=RS, chunks=3, align=64), dict(K=2, subs=subs(2, 1024, 476))),
    ("nor below one alignment unit: 5,000 per rank in rounds of 2,560 gives two of eight", dict(B=40000, nranks=8, RS=RS, chunks=8, units=2560), dict(K=2, subs=subs(8, 2560, 2440), consults_units=1)),
    # ---- nothing to hide
    ("ranks sharing a device, chunks 0: one sub-batch whatever the size, no agreement", dict(B=40000, nranks=8, RS=RS, nothing_to_hide=1), dict(K=1, cap=5000, consults_units=0)),
    ("one rank, chunks 0", dict(B=40000, nranks=1, RS=RS), dict(K=1, cap=40000, consults_units=0)),
    ("ranks sharing a device, chunks 3: cut as asked, in agreed units", dict(B=40000, nranks=8, RS=RS, chunks=3, units=1280, nothing_to_hide=1), dict(K=3, consults_units=1, subs=subs(8, 2560, 1280, 1160))),
    ("one rank, chunks 3, in count tiles", dict(B=5000, nranks=1, RS=RS, chunks=3, align=64), dict(K=3, consults_units=0, subs=subs(1, 2880, 1408, 712))),
    # ---- the headline shape: 5,000 per rank on 8 ranks
    ("headline in rounds of the device (1,280 agreed)", dict(B=40000, nranks=8, RS=RS, units=1280, nothing_to_hide=0),
     dict(K=3, cap=5000, consults_units=1, send_bytes=5600000, recv_bytes=44800000, subs=[(0, 20480, 2560, 0), (20480, 10240, 1280, 2560), (30720, 9280, 1160, 3840)])),
    ("headline, chunk_align 1280: the same cuts, nothing to agree on", dict(B=40000, nranks=8, RS=RS, align=1280, units=64, nothing_to_hide=0), dict(K=3, consults_units=0, subs=subs(8, 2560, 1280, 1160))),
    ("headline, chunk_align 64", dict(B=40000, nranks=8, RS=RS, align=64, nothing_to_hide=0), dict(K=3, cap=5000, subs=subs(8, 2880, 1408, 712))),
    ("headline, segment (1, 3) starts behind sub-batch 0's 8 x 2,560 records", dict(B=40000, nranks=8, RS=RS, align=1280, nothing_to_hide=0),
     dict(segments=[[(r * 2560, r * 2560, 2560) for r in range(8)], [(20480 + r * 1280, 20480 + r * 1280, 1280) for r in range(8)], [(30720 + r * 1160, 30720 + r * 1160, 1160) for r in range(8)]])),
]


@pytest.mark.parametrize("args,expected", [c[1:] for c in PLANS], ids=[c[0] for c in PLANS])
def test_group_plan(emu, args, expected):
    got = plan(emu, **args)
    assert {k: got[k] for k in expected} == expected
    check_properties(got, args["B"], args["nranks"], args["RS"])


def check_properties(p, B, nranks, RS):
    K, sub = p["K"], p["subs"]
    assert 1 <= K <= CHUNKS_MAX
    # the sub-batches tile [0, B) in order; the caps add up to the buffers
    assert sub[0][0] == 0 and sum(s[1] for s in sub) == B and all(s[1] >= 1 for s in sub) and all(sub[k][0] + sub[k][1] == sub[k + 1][0] for k in range(K - 1))
    assert all(s[2] == -(-s[1] // nranks) for s in sub) and [s[3] for s in sub] == [sum(t[2] for t in sub[:k]) for k in range(K)]
    assert p["cap"] == sum(s[2] for s in sub) and p["send_bytes"] == p["cap"] * RS * 8 and p["recv_bytes"] == p["send_bytes"] * nranks == sum(s[2] for s in sub) * nranks * RS * 8
    # the segments of all (k, rank): disjoint blocks of `cap` records in the order of the receive buffer, inside it; their replicates tile [0, B) in order
    rec_at, rep_at = 0, 0
    for k in range(K):
        for r in range(nranks):
            rec0, first, count = p["segments"][k][r]
            sfirst, scount, full = p["shards"][k][r]
            assert rec0 == rec_at and first == rep_at and 0 <= count <= sub[k][2] and first == sub[k][0] + sfirst and scount == count
            assert count >= sub[k][2] - 1 and full == (count == sub[k][2] and count > 0)
            rec_at += sub[k][2]; rep_at += count
        assert rep_at == sub[k][0] + sub[k][1]
    assert rec_at * RS * 8 == p["recv_bytes"] and rep_at == B


def test_properties_of_every_plan_on_a_grid(emu):
    """... and the plan is a function of rank-invariant inputs only: group_plan takes no rank (every rank's shards and segments above come from the one plan), and the one
    input that starts out rank-local -- the alignment a handle would choose for itself -- is read only where group_consults_units says the ranks agree on it first."""
    n = 0
    for B in (1, 2, 7, 63, 513, 1537, 2561, 4095, 5003, 40000, 40017, (1 << 20) + 5):
        for nranks in (1, 2, 3, 8, 16):
            for chunks in range(CHUNKS_MAX + 1):
                for ratio, align, rs in ((10, 0, 3), (50, 64, 140), (100, 1280, 27), (50, 0, 1000), (33, 100, 140)):
                    for nth in (0, 1):
                        if nranks == 1 and not nth:
                            continue
                        a, b = (plan(emu, B, nranks, rs, chunks, ratio, align, units, nth) for units in (64, 2560))
                        check_properties(a, B, nranks, rs); check_properties(b, B, nranks, rs)
                        assert a["consults_units"] == b["consults_units"] == int(not (nth and chunks == 0) and chunks != 1 and align == 0)
                        assert a["consults_units"] or a == b
                        assert all(s[1] % (nranks * (align or 64)) == 0 for s in a["subs"][:-1])
                        n += 1
    assert n == 12 * 9 * 5 * 9


def test_every_rule_has_a_row():
    ks = {(c[1].get("chunks", 0), c[2].get("K")) for c in PLANS}
    assert {(0, 1), (0, 3), (1, 1), (8, 7), (8, 8), (3, 2), (3, 3), (2, 1)} <= ks
    assert any(c[1].get("nothing_to_hide") == 1 and c[1].get("chunks", 0) == 0 for c in PLANS) and any(c[1].get("nothing_to_hide") == 1 and c[1].get("chunks") == 3 for c in PLANS)
    assert {64, 1280} <= {c[1].get("align") for c in PLANS}
