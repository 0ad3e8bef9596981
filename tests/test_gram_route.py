"""CPU check of the launch form of the int8 Gram (csrc/gram_route.h gram_i8_plan: kernel form, tile rows, grid, resample histogram, buffer sizes) through the
emulation build in tests/hostemu/: an explicit table with a row for every form and rows at the edges of the batch size, the plane count and the options.  The
expected values are what the launcher computed before the plan had a function of its own and what the GPU tests observe through get_option("last_i8_*") for the
same shapes (test_gpu_gram_i8.py, test_host_api.py)."""
import pytest

from helpers_gram_route import HIST4, HIST8, HIST16, IND, NARROW, PERSIST, PLAIN, PRIV, SHAPE32, SK, WIDE20, data, load_emu, plan


@pytest.fixture(scope="module")
def emu():
    return load_emu()


HEAD6, HEAD7 = data(6, 10000, 60), data(7, 10000, 60)      # bench.py's 10,000 x 60: 158 k-blocks, 60 pair tiles
SMALL6, SMALL7 = data(6, 777, 15), data(7, 777, 15)        # test_gpu_gram_i8.py's 777 x 15: 14 k-blocks, 5 pair tiles
TINY6, TINY7 = dict(S=6, KB=14, NT=24, npg=4, zs_ind=0), dict(S=7, KB=14, NT=28, npg=4, zs_ind=0)      # two pair tiles
IND1 = dict(S=1, KB=16, NT=28, npg=28, zs_ind=1)           # 0/1 data: one plane per pair group, two tiles of 2 x 7 groups
EXP = dict(experiments=1)
# (id, data, call, options, expected)
CASES = [
    # ---- one row per form
    ("private counts, six planes: 12 tall + 5 short rows on 256 CUs", HEAD6, dict(nb=5000), {},
     dict(form=PRIV, waves=4, variant=64, dma_buffer=0, rt_tall=20, rt_short=16, nty_tall=12, nty_short=5, nty=17, ntx=60, MT=320, per_xcd=128, grid=1024, block=256, pp_wgs=0, sk_grid=0,
          hist=HIST16, hist_bytes=20224, hist_windows=1, hist_threads=256, cd_bytes=53739520, to16=0, priv_takes=1)),
    ("persistent: one workgroup per CU", HEAD6, dict(nb=5000), dict(persist=1), dict(form=PERSIST, variant=64, nty_tall=12, nty_short=5, per_xcd=128, pp_wgs=32, grid=256, block=256)),
    ("round-3 kernel on the 320-replicate tile, rows of 256 mixed in", HEAD6, dict(nb=5000), dict(priv=0),
     dict(form=WIDE20, waves=8, variant=-1, dma_buffer=0, rt_tall=20, rt_short=16, nty_tall=12, nty_short=5, MT=320, grid=1024, block=512, priv_takes=0)),
    ("plain, seven planes: buffer form of the LDS-DMA", HEAD7, dict(nb=5000), dict(priv=0),
     dict(form=PLAIN, waves=8, variant=-1, dma_buffer=1, rt_tall=16, rt_short=0, nty_tall=20, nty_short=0, nty=20, MT=320, per_xcd=150, grid=1200, block=512)),
    ("plain, i8_dma 1: the flat form", HEAD7, dict(nb=5000), dict(priv=0, dma=1), dict(form=PLAIN, dma_buffer=0, grid=1200)),
    ("eight planes: plain whatever i8_priv says", dict(HEAD7, S=8, NT=960), dict(nb=5000), {}, dict(form=PLAIN, dma_buffer=1, rt_tall=16, MT=320, grid=1200, priv_takes=0, round_units=64)),
    ("five planes", dict(HEAD7, S=5, NT=600), dict(nb=300), {}, dict(form=PLAIN, dma_buffer=1, nty=2, MT=32, per_xcd=15, grid=120, cd_bytes=5373952)),
    ("indicator data", IND1, dict(nb=700), {}, dict(form=IND, waves=8, dma_buffer=1, rt_tall=16, nty=3, MT=48, ntx=2, per_xcd=1, grid=8, block=512, hist_bytes=2048, cd_bytes=1081344, to16=0, priv_takes=0)),
    ("indicator data, uint16 output", IND1, dict(nb=700, want16=1), {}, dict(form=IND, dma_buffer=1, ntx=2, to16=1)),
    ("indicator data, uint16 output, flat DMA", IND1, dict(nb=700, want16=1), dict(dma=1), dict(form=IND, dma_buffer=0, to16=1)),
    ("uint16 output asked of multi-plane data", HEAD6, dict(nb=700, want16=1), {}, dict(form=PRIV, to16=0)),
    ("stream-K (experiments)", HEAD6, dict(nb=5000, **EXP), dict(sched=1), dict(form=SK, waves=8, rt_tall=16, nty=20, MT=320, sk_grid=256, grid=256, block=512, dma_buffer=0, priv_takes=0)),
    ("stream-K, four waves (experiments)", HEAD6, dict(nb=5000, **EXP), dict(sched=1, waves=4), dict(form=SK, waves=4, grid=256, block=256)),
    ("narrow tile (experiments)", HEAD7, dict(nb=5000, **EXP), dict(rt=8, waves=4), dict(form=NARROW, waves=4, rt_tall=8, nty=40, MT=320, per_xcd=300, grid=2400, block=256, dma_buffer=0, priv_takes=0)),
    ("32x32x32 shape (experiments)", HEAD6, dict(nb=5000, **EXP), dict(shape=32), dict(form=SHAPE32, waves=4, rt_tall=16, MT=320, grid=1200, block=256, dma_buffer=0, priv_takes=0)),
    ("four waves (experiments): private counts all the same", HEAD7, dict(nb=5000, **EXP), dict(waves=4), dict(form=PRIV, waves=4, variant=64, nty_tall=17, nty_short=4, grid=1264, block=256)),
    ("four waves, plain (experiments)", HEAD7, dict(nb=5000, **EXP), dict(priv=0, waves=4), dict(form=PLAIN, waves=4, dma_buffer=1, grid=1200, block=256)),
    ("schedule variant of the seven-plane kernel (experiments)", HEAD7, dict(nb=5000, **EXP), dict(priv=0, variant=12), dict(form=PLAIN, variant=12, dma_buffer=0, grid=1200, block=512)),
    ("320-replicate tile on four waves: the buffer form (experiments)", HEAD6, dict(nb=5000, **EXP), dict(priv=0, rt=20, waves=4), dict(form=WIDE20, waves=4, dma_buffer=1, nty_tall=16, nty_short=0, grid=960, block=256)),
    ("schedule variant of the 320-replicate tile (experiments)", HEAD6, dict(nb=5000, **EXP), dict(priv=0, rt=20, variant=13), dict(form=WIDE20, variant=13, dma_buffer=0, nty_tall=16, grid=960, block=512)),
    ("variant of the private-count kernel (experiments)", HEAD6, dict(nb=5000, **EXP), dict(variant=77), dict(form=PRIV, variant=77, nty_tall=12, nty_short=5, grid=1024, priv_takes=1)),
    ("a variant names a round-3 kernel in the release build", HEAD7, dict(nb=5000), dict(variant=12), dict(form=PLAIN, priv_takes=0, round_units=64)),
    # ---- the batch size, six against seven planes (private counts: tile rows of 320 / 256 against 256 / 192 replicates)
    ("six planes, B 1", TINY6, dict(nb=1, cu_count=64), {}, dict(form=PRIV, rt_tall=20, rt_short=16, nty_tall=0, nty_short=1, MT=16, per_xcd=1, grid=8, cd_bytes=327680)),
    ("six planes, B 255", TINY6, dict(nb=255, cu_count=64), {}, dict(nty_tall=0, nty_short=1, MT=16)),
    ("six planes, B 256", TINY6, dict(nb=256, cu_count=64), {}, dict(nty_tall=0, nty_short=1, MT=16)),
    ("six planes, B 257", TINY6, dict(nb=257, cu_count=64), {}, dict(nty_tall=0, nty_short=2, MT=32, grid=8)),
    ("six planes, B 320", TINY6, dict(nb=320, cu_count=64), {}, dict(nty_tall=0, nty_short=2, MT=32)),
    ("six planes, B 321", TINY6, dict(nb=321, cu_count=64), {}, dict(nty_tall=0, nty_short=2, MT=32, cd_bytes=655360)),
    ("seven planes, B 1", TINY7, dict(nb=1, cu_count=64), {}, dict(form=PRIV, rt_tall=16, rt_short=12, nty_tall=0, nty_short=1, MT=12, grid=8, cd_bytes=245760)),
    ("seven planes, B 255", TINY7, dict(nb=255, cu_count=64), {}, dict(nty_tall=0, nty_short=2, MT=24)),
    ("seven planes, B 256", TINY7, dict(nb=256, cu_count=64), {}, dict(nty_tall=0, nty_short=2, MT=24)),
    ("seven planes, B 257", TINY7, dict(nb=257, cu_count=64), {}, dict(nty_tall=0, nty_short=2, MT=24)),
    ("seven planes, B 320", TINY7, dict(nb=320, cu_count=64), {}, dict(nty_tall=0, nty_short=2, MT=24)),
    ("seven planes, B 321", TINY7, dict(nb=321, cu_count=64), {}, dict(nty_tall=0, nty_short=2, MT=24, cd_bytes=491520)),
    ("seven planes, B 5000", HEAD7, dict(nb=5000), {}, dict(form=PRIV, rt_tall=16, rt_short=12, nty_tall=17, nty_short=4, nty=21, MT=320, per_xcd=158, grid=1264)),
    ("64 replicates: one tile row either way, the lower tile wins", HEAD6, dict(nb=64), {}, dict(form=PRIV, nty_tall=0, nty_short=1, MT=16, grid=64)),
    # ---- i8_rt 0 / 16 / 20
    ("six planes, i8_rt 16: the 256-replicate round-3 kernel", TINY6, dict(nb=321, cu_count=64), dict(rt=16), dict(form=PLAIN, dma_buffer=1, rt_tall=16, rt_short=0, nty=2, MT=32, block=512, priv_takes=0, round_units=64)),
    ("six planes, i8_rt 20: tall rows only", TINY6, dict(nb=321, cu_count=64), dict(rt=20), dict(form=PRIV, rt_tall=20, nty_tall=2, nty_short=0, MT=40, cd_bytes=819200, priv_takes=1)),
    ("six planes, i8_rt 20, round-3 kernel", TINY6, dict(nb=321, cu_count=64), dict(rt=20, priv=0), dict(form=WIDE20, dma_buffer=0, nty_tall=2, nty_short=0, MT=40, block=512)),
    ("seven planes, i8_rt 16: tall rows only", TINY7, dict(nb=321, cu_count=64), dict(rt=16), dict(form=PRIV, rt_tall=16, nty_tall=2, nty_short=0, MT=32, priv_takes=1)),
    ("seven planes, i8_rt 20 names the round-3 kernel", TINY7, dict(nb=321, cu_count=64), dict(rt=20), dict(form=PLAIN, dma_buffer=1, rt_tall=16, nty=2, MT=32, priv_takes=0, round_units=64)),
    ("4,096 replicates x 60 pair tiles: 960 tiles of 256 beat every cut of the round-3 kernel", HEAD6, dict(nb=4096), dict(priv=0), dict(form=PLAIN, dma_buffer=1, rt_tall=16, nty=16, MT=256, grid=960)),
    ("64 replicates, round-3 kernel: the lower tile wins", HEAD6, dict(nb=64), dict(priv=0), dict(form=PLAIN, rt_tall=16, nty=1, MT=16, grid=64)),
    # ---- i8_short_rows: capped by the rows there are
    ("two short rows behind two tall ones", TINY6, dict(nb=1100, cu_count=64), dict(rt=20, short_rows=2), dict(form=PRIV, nty_tall=2, nty_short=2, nty=4, MT=72, per_xcd=2, grid=16)),
    ("4,096 short rows asked for: five there are", TINY6, dict(nb=1100, cu_count=64), dict(rt=20, short_rows=4096), dict(form=PRIV, nty_tall=0, nty_short=5, MT=80)),
    ("... on the round-3 kernel", TINY6, dict(nb=1100, cu_count=64), dict(rt=20, short_rows=4096, priv=0), dict(form=WIDE20, nty_tall=0, nty_short=5, MT=80, block=512)),
    ("no short rows beside the buffer form of the round-3 kernel", TINY6, dict(nb=1100, cu_count=64), dict(rt=20, short_rows=3, priv=0, dma=2), dict(form=WIDE20, dma_buffer=0, nty_tall=4, nty_short=0, MT=80)),
    ("seven planes: six rows of 192", TINY7, dict(nb=1100, cu_count=64), dict(rt=16, short_rows=4096), dict(form=PRIV, nty_tall=0, nty_short=6, MT=72)),
    ("seven planes, i8_rt 0 with three short rows", TINY7, dict(nb=1100, cu_count=64), dict(short_rows=3), dict(form=PRIV, nty_tall=3, nty_short=3, MT=84, cd_bytes=1720320)),
    ("test_gpu_gram_i8's 777 x 15, B 1100, five short rows", SMALL6, dict(nb=1100), dict(rt=20, short_rows=5), dict(form=PRIV, nty_short=min(5, (1100 + 255) // 256), ntx=5)),
    # ---- i8_cus: a cut for fewer CUs than there are tiles
    ("cut for 64 CUs", HEAD6, dict(nb=5000), dict(cus=64), dict(form=PRIV, nty_tall=16, nty_short=0, MT=320, per_xcd=120, grid=960)),
    ("persistent on 8 CUs: one workgroup per XCD", HEAD6, dict(nb=5000), dict(cus=8, persist=1), dict(form=PERSIST, nty_tall=15, nty_short=1, MT=316, per_xcd=121, pp_wgs=1, grid=8, cd_bytes=53067776)),
    ("i8_cus above the device's count: the device's", HEAD6, dict(nb=5000), dict(cus=4096), dict(nty_tall=12, nty_short=5)),
    # ---- the resample histogram
    ("explicit indices: 16-bit counters whatever KB is", dict(TINY6, KB=3000), dict(nb=257, cu_count=64, explicit_idx=1), {}, dict(hist=HIST16, hist_bytes=131072, hist_windows=3, hist_threads=1024, cd_bytes=98500608)),
    ("one 16-bit window", dict(TINY6, KB=1024), dict(nb=257, cu_count=64), {}, dict(hist=HIST16, hist_bytes=131072, hist_windows=1, hist_threads=1024)),
    ("one k-block past it: 4-bit counters", dict(TINY6, KB=1025), dict(nb=257, cu_count=64), {}, dict(hist=HIST4, hist_bytes=32800, hist_windows=1, hist_threads=512)),
    ("one k-block past it, explicit indices: two windows", dict(TINY6, KB=1025), dict(nb=257, cu_count=64, explicit_idx=1), {}, dict(hist=HIST16, hist_windows=2)),
    ("100,000 rows, i8_nibbles 0: 8-bit counters", dict(TINY6, KB=1564), dict(nb=257, cu_count=64), dict(nibbles=0), dict(hist=HIST8, hist_bytes=100096, hist_windows=1, hist_threads=1024)),
    ("one 8-bit window", dict(TINY6, KB=2048), dict(nb=257, cu_count=64), dict(nibbles=0), dict(hist=HIST8, hist_bytes=131072, hist_windows=1)),
    ("one k-block past the 8-bit window", dict(TINY6, KB=2049), dict(nb=257, cu_count=64), dict(nibbles=0), dict(hist=HIST8, hist_bytes=131072, hist_windows=2)),
    ("100,000 rows: 4-bit counters, three workgroups per CU", dict(TINY6, KB=1564), dict(nb=257, cu_count=64), {}, dict(hist=HIST4, hist_bytes=50048, hist_windows=1, hist_threads=512)),
    ("one 4-bit window", dict(TINY6, KB=4096), dict(nb=257, cu_count=64), {}, dict(hist=HIST4, hist_bytes=131072, hist_windows=1, hist_threads=1024)),
    ("one k-block past the 4-bit window", dict(TINY6, KB=4097), dict(nb=257, cu_count=64), dict(nibbles=2), dict(hist=HIST4, hist_windows=2, cd_bytes=134447104)),
    ("32x32x32 shape: no 4-bit counters (experiments)", dict(TINY6, KB=1025), dict(nb=257, cu_count=64, **EXP), dict(shape=32), dict(form=SHAPE32, hist=HIST8)),
    # ---- the 4 GiB bound of the buffer DMA: (KB + 6 slack k-blocks) x 840 digit blocks x 1 KB
    ("last KB whose walk stays below 4 GiB", dict(HEAD7, KB=4987), dict(nb=5000), dict(priv=0), dict(form=PLAIN, dma_buffer=1)),
    ("one k-block more: the flat form", dict(HEAD7, KB=4988), dict(nb=5000), dict(priv=0), dict(form=PLAIN, dma_buffer=0)),
]


@pytest.mark.parametrize("d,call,opts,expected", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_gram_i8_plan(emu, d, call, opts, expected):
    got = plan(emu, d, **call, **opts)
    assert {k: got[k] for k in expected} == expected
    # what holds for every launch: the rows cover the batch, the grid follows from the rows
    assert got["nty"] == got["nty_tall"] + got["nty_short"] and got["MT"] == got["nty_tall"] * got["rt_tall"] + got["nty_short"] * got["rt_short"]
    assert 16 * got["MT"] >= call["nb"] and got["block"] == 64 * got["waves"]
    assert got["per_xcd"] == (got["ntx"] * got["nty_tall"] + 7) // 8 + (got["ntx"] * got["nty_short"] + 7) // 8
    assert got["grid"] == (8 * got["pp_wgs"] if got["form"] == PERSIST else got["sk_grid"] if got["form"] == SK else 8 * got["per_xcd"])
    assert got["cd_bytes"] == got["MT"] * 16 * (d["KB"] + 6) * 64


def test_every_form_has_a_row():
    assert {c[4]["form"] for c in CASES if "form" in c[4]} == set(range(8))


@pytest.mark.parametrize("d", [HEAD6, HEAD7, SMALL6, SMALL7, TINY6, TINY7], ids=["10000x60 S6", "10000x60 S7", "777x15 S6", "777x15 S7", "two tiles S6", "two tiles S7"])
@pytest.mark.parametrize("cus,i8_cus", [(256, 0), (304, 0), (64, 0), (8, 0), (256, 64), (256, 8), (64, 240)])
def test_round_units_are_whole_rounds_of_the_tall_tile_the_plan_reports(emu, d, cus, i8_cus):
    """The sub-batch plan's alignment (get_option("boot_round_units")) and the launcher read one predicate and one tile height."""
    got = plan(emu, d, 5000, cu_count=cus, cus=i8_cus)
    assert got["form"] == PRIV and got["priv_takes"] == 1 and got["rt_tall"] == (20 if d["S"] == 6 else 16)
    cut_for = max(8, min(i8_cus, cus) if i8_cus else cus)
    assert got["round_units"] == max(1, cut_for // got["ntx"]) * got["rt_tall"] * 16


def test_shapes_of_the_table():
    assert (HEAD6["KB"], HEAD6["npg"], HEAD6["NT"]) == (158, 120, 720) and (SMALL6["KB"], SMALL6["npg"]) == (14, 10) and data(1, 1000, 26, ind=True)["npg"] == 28
