"""GPU: the derived records at the edges of their plan (csrc/derived_route.h, csrc/plspm_derived.hip): every combination of the five switches, a call cut into
passes and into sub-batches, and the largest model the geodesic stage takes beside the first it refuses.

The model: three LVs with the paths 0 -> 1, 1 -> 2 and 0 -> 2 (three direct paths, one specific indirect effect), blocks of two MVs, 30 rows.  What a stage
writes for a replicate depends on the replicate alone, so everything here is compared bit for bit (the raw bytes, NaNs included): a stage's records under any
combination of switches against the run with that stage's switch alone, and a cut call against the whole one."""
import itertools

import numpy as np
import pytest

import plspm_oracle as orc
from helpers_plsc import native_model, tri

pytestmark = pytest.mark.gpu
E_STATE, E_LIMIT = 101, 102
INADMISSIBLE = 4
STAGES = ("assess", "structural", "plsc", "modelfit", "geodesic")            # in launch order
READS = {"assess": (), "structural": ("assess",), "plsc": ("assess",), "modelfit": ("plsc",), "geodesic": ("modelfit", "plsc")}
NOUN = {"assess": "assessment", "structural": "structural", "plsc": "PLSc", "modelfit": "model-fit", "geodesic": "geodesic"}
C3 = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0]])
N, B, SEED = 30, 5, 11                                       # B = 5: one full workgroup of four waves and one partial


def closure(on):
    """The stages that run: the switches and everything they read."""
    runs = set(on)
    while True:
        more = runs | {r for s in runs for r in READS[s]}
        if more == runs:
            return runs
        runs = more


def handle(on, **options):
    X, blocks = orc.synth(N, C3, 2, seed=21)
    nm = native_model(orc.Model(blocks, C3, "AAA", "path", True), X, **options)
    for s in STAGES:
        getattr(nm, s + "_enable")(s in on)
    return nm


def same_bytes(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def stage_records(nm, s, count):
    recs, status = getattr(nm, s + "_fetch")(0, count)
    return recs, status


@pytest.fixture(scope="module")
def alone():
    """Per stage, with its switch alone: its B records, their status, and its full-sample record."""
    out = {}
    for s in STAGES:
        nm = handle({s})
        rows = nm.bootstrap(B, seed=SEED)
        out[s] = stage_records(nm, s, B) + getattr(nm, s + "_fit")() + (rows,)
    return out


def test_the_closures_named():
    assert closure({"structural"}) == {"assess", "structural"} and closure({"geodesic"}) == {"assess", "plsc", "modelfit", "geodesic"}
    assert closure({"modelfit"}) == {"assess", "plsc", "modelfit"} and closure(set()) == set()


@pytest.mark.parametrize("on", [frozenset(s for s, bit in zip(STAGES, bits) if bit) for bits in itertools.product((0, 1), repeat=5)],
                         ids=lambda on: "+".join(s for s in STAGES if s in on) or "none")
def test_switch_combinations(alone, on):
    from plspm import _native
    nm = handle(on)
    rows = nm.bootstrap(B, seed=SEED)
    for a, b in zip(rows, alone["assess"][4]):
        assert same_bytes(a, b)                              # the bootstrap's own records do not depend on the switches
    runs = closure(on)
    for s in STAGES:
        if s in runs:
            recs, status = stage_records(nm, s, B)
            assert recs.shape == (B, getattr(nm, s + "_width")) and status.shape == (B,)
            assert same_bytes(recs, alone[s][0]) and same_bytes(status, alone[s][1]), s
        else:
            with pytest.raises(_native.NativeBackendError, match=r"plspm_%s_fetch failed \(%d\).*: no %s records on this handle" % (s, E_STATE, NOUN[s])):
                stage_records(nm, s, B)
        if s == "structural":
            nm.structural_paths()                            # (lists the paths where no switch did: the caller sizes the record by structural_width, 0 until then)
        full, status = getattr(nm, s + "_fit")()             # the full-sample record asks for no switch
        assert same_bytes(full, alone[s][2]) and status == alone[s][3], s


def test_passes_and_sub_batches():
    """All five stages on, 600 replicates through plspm_bootstrap(): one pass, three passes of 256 (the "boot_pass" test option), and three sub-batches whose
    records start behind the first one's in every stage's buffer."""
    count = 600

    def run(**options):
        nm = handle(set(STAGES), **options)
        rows = nm.bootstrap(count, seed=SEED)
        return nm, list(rows) + [a for s in STAGES for a in stage_records(nm, s, count)]
    nm, whole = run()
    assert nm.get_option("last_boot_passes") == 1
    nm, cut = run(boot_pass=256)
    assert nm.get_option("last_boot_passes") == 3
    _, parts = run(boot_chunks=3, boot_align=64)
    for a, b, c in zip(whole, cut, parts):
        assert same_bytes(a, b) and same_bytes(a, c)
    assert np.any(whole[1] == 0)                             # (some replicates converged: the records compared are not all void)


def two_blocks(P):
    """160 rows of P MVs under two LVs in a chain, the first block taking the odd one: a geodesic wave takes (P + 4)^2 doubles of the 20,480 a workgroup has."""
    rng = np.random.default_rng(7)
    eta = rng.standard_normal((160, 2))
    eta[:, 1] = 0.6 * eta[:, 0] + 0.8 * eta[:, 1]
    sizes = [P - P // 2, P // 2]
    blocks = [np.arange(0, sizes[0]), np.arange(sizes[0], P)]
    X = np.concatenate([0.7 * eta[:, [l]] + 0.7 * rng.standard_normal((160, sizes[l])) for l in range(2)], axis=1)
    return X, orc.Model(blocks, tri(2), "AA", "centroid", True)


def test_the_largest_geodesic_model_that_fits():
    """P = 139: 143^2 = 20,449 doubles, one wave per workgroup."""
    X, model = two_blocks(139)
    nm = native_model(model, X)
    nm.geodesic_enable(True)
    nm.bootstrap_device(2, 1, 0)
    recs, status = nm.geodesic_fetch(0, 2)
    assert recs.shape == (2, 2)
    for r in range(2):                                       # (a resample of 160 rows has fewer distinct rows than MVs: its correlation matrix is singular)
        assert (status[r] == 0 and np.all(np.isfinite(recs[r]))) or (status[r] == INADMISSIBLE and np.all(np.isnan(recs[r])))
    full, st = nm.geodesic_fit()
    assert st == 0 and np.all(np.isfinite(full)) and np.all(full >= 0.0)
    assert nm.modelfit_fetch(0, 2)[0].shape == (2, 4) and nm.plsc_fetch(0, 2)[0].shape[0] == 2 and nm.assess_fetch(0, 2)[0].shape[0] == 2


def test_the_first_geodesic_model_that_is_refused():
    """P = 140: 144^2 = 20,736 doubles.  The call is refused before it runs anything, behind the point where it voided the handle's records."""
    from plspm import _native
    X, model = two_blocks(140)
    nm = native_model(model, X)
    nm.modelfit_enable(True)
    nm.bootstrap_device(2, 1, 0)
    assert nm.modelfit_fetch(0, 2)[0].shape == (2, 4) and nm.fetch(0, 2)[0].shape[0] == 2
    nm.geodesic_enable(True)
    refusal = r"plspm_bootstrap_device failed \(%d\).*geodesic discrepancy: the two P x P triangles of one replicate need more than 160 KiB of LDS" % E_LIMIT
    with pytest.raises(_native.NativeBackendError, match=refusal):
        nm.bootstrap_device(2, 1, 0)
    for s in ("assess", "plsc", "modelfit", "geodesic"):
        with pytest.raises(_native.NativeBackendError, match=r"plspm_%s_fetch failed \(%d\).*: no %s records on this handle" % (s, E_STATE, NOUN[s])):
            stage_records(nm, s, 2)
    with pytest.raises(_native.NativeBackendError, match=r"plspm_bootstrap_fetch failed \(%d\)" % E_STATE):
        nm.fetch(0, 2)
    nm.geodesic_enable(False)                                # model fit alone still runs on it
    nm.bootstrap_device(2, 1, 0)
    assert nm.modelfit_fetch(0, 2)[0].shape == (2, 4)
