"""GPU: every kind of batch call one after the other on ONE handle (plspm_bootstrap.hip plspm_detail_bootstrap and its BatchCall).  The other tests pin each
kind on a handle of its own; state that a call left behind -- a spec, a destination, an offset, a voided or a forgotten record count -- shows only in a sequence.

On one handle with assessment, PLSc, model fit and MICOM enabled: plain bootstrap (host entry point, cut into sub-batches where the call allows it), permutation, jackknife,
cross-validation, stratified bootstrap, the moments seam, plain bootstrap again (device entry point), upload.  After every step

  * what the step wrote -- records, status, iteration counts, assessment / PLSc / model-fit / MICOM records, training moments, moment matrices -- is bit-identical to the same
    call on a fresh handle, and
  * every kind's records are there with the expected count, or gone (PLSPM_E_STATE), as the driver's rules say (EFFECT below).

At N = 300 and at N = 100 (below 128 rows the launches take the short-N forms that share the device error word: the other side of may_raise), in one pass
and with 256 problems per pass."""
import numpy as np
import pytest

import plspm_oracle as orc
from test_gpu_predict import native_model

pytestmark = pytest.mark.gpu
E_ARG, E_STATE = 100, 101
C3 = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0]])
B, SPLITS, REPS, K, MOMENTS = 300, 150, 3, 5, 8
KINDS = ("rows", "cv", "assess", "plsc", "modelfit", "micom", "jack")

# What a step does to each kind's records: a count (valid, that many), None (void) or absent (unchanged).  Read off plspm_detail_bootstrap: a call voids
# whatever went with the bootstrap records it replaces; the jackknife writes into buffers of its own.  The PLSc and model-fit records follow the assessment's
# in every step (model.h void_records).
EFFECT = {
    "plain": dict(rows=B, cv=None, assess=B, plsc=B, modelfit=B, micom=None),
    "permutation": dict(rows=2 * SPLITS, cv=None, assess=None, plsc=None, modelfit=None, micom=SPLITS),
    "jackknife": dict(jack="N"),
    "cv": dict(rows=REPS * K, cv=REPS * K, assess=None, plsc=None, modelfit=None, micom=None),
    "stratified": dict(rows=2 * SPLITS, cv=None, assess=None, plsc=None, modelfit=None, micom=None),
    "moments": dict(rows=None, cv=None, assess=None, plsc=None, modelfit=None, micom=None),
    "plain_device": dict(rows=B, cv=None, assess=B, plsc=B, modelfit=B, micom=None),
    "upload": dict(rows=None, cv=None, assess=None, plsc=None, modelfit=None, micom=None, jack=None),
}
SEQUENCE = ("plain", "permutation", "jackknife", "cv", "stratified", "moments", "plain_device", "upload")


def new_handle(X, model, cap):
    nm = native_model(model, X)
    nm.modelfit_enable()                     # (model fit reads the PLSc records, and those the assessment's: all three stages are on)
    nm.micom_enable()
    nm.set_option("boot_pass", cap)
    nm.set_option("boot_chunks", 2)          # plspm_bootstrap() as two sub-batches where the call may be cut (not below 128 rows)
    nm.set_option("boot_align", 64)
    return nm


def run_step(nm, step, X, model, member):
    """The step's call on `nm`; returns every array it wrote."""
    n = X.shape[0]
    if step == "plain":
        return nm.bootstrap(B, seed=11) + nm.fetch(0, B) + nm.assess_fetch(0, B) + nm.plsc_fetch(0, B) + nm.modelfit_fetch(0, B)
    if step == "permutation":
        nm.permutation(SPLITS, (2 * n) // 5, seed=12)
        return nm.fetch(0, 2 * SPLITS) + nm.micom_fetch(0, SPLITS)
    if step == "jackknife":
        nm.jackknife(n)
        return nm.jackknife_fetch(0, n)
    if step == "cv":
        nm.cv(REPS, K, seed=13)
        return nm.fetch(0, REPS * K) + nm.cv_moments(REPS, K)
    if step == "stratified":
        nm.stratified_bootstrap(SPLITS, member, seed=14)
        return nm.fetch(0, 2 * SPLITS)
    if step == "moments":
        return (nm.bootstrap_moments(MOMENTS, seed=15),)
    if step == "plain_device":
        nm.bootstrap_device(B, seed=16)
        return nm.fetch(0, B) + nm.assess_fetch(0, B) + nm.plsc_fetch(0, B) + nm.modelfit_fetch(0, B)
    assert step == "upload"
    nm.upload(X, model.mv_order.astype(np.int32))
    return ()


def check_records(nm, expected):
    """Every kind's fetch serves exactly expected[kind] records, or fails with PLSPM_E_STATE where that is None."""
    from plspm import _native
    fetch = dict(rows=("plspm_bootstrap_fetch", nm.fetch), assess=("plspm_assess_fetch", nm.assess_fetch), plsc=("plspm_plsc_fetch", nm.plsc_fetch),
                 modelfit=("plspm_modelfit_fetch", nm.modelfit_fetch), micom=("plspm_micom_fetch", nm.micom_fetch),
                 jack=("plspm_jackknife_fetch", nm.jackknife_fetch))
    for kind, (name, call) in fetch.items():
        count = expected[kind]
        if count is None:
            with pytest.raises(_native.NativeBackendError, match=r"%s failed \(%d\)" % (name, E_STATE)):
                call(0, 1)
        else:
            call(0, count)
            with pytest.raises(_native.NativeBackendError, match=r"%s failed \(%d\)" % (name, E_ARG)):      # one more than there are
                call(count, 1)
    if expected["cv"] is None:
        with pytest.raises(_native.NativeBackendError, match=r"plspm_cv_moments failed \(%d\)" % E_STATE):
            nm.cv_moments(REPS, K)
    else:
        nm.cv_moments(REPS, K)


@pytest.mark.parametrize("cap", [0, 256])
@pytest.mark.parametrize("n", [300, 100])
def test_every_kind_in_sequence_on_one_handle(n, cap):
    X, blocks = orc.synth(n, C3, 3, seed=21)
    model = orc.Model(blocks, C3, "ABA", "path", True)
    member = np.zeros(n, dtype=bool)
    member[np.random.default_rng(3).permutation(n)[:(2 * n) // 5]] = True
    nm = new_handle(X, model, cap)
    expected = dict.fromkeys(KINDS)
    check_records(nm, expected)
    for step in SEQUENCE:
        got = run_step(nm, step, X, model, member)
        want = run_step(new_handle(X, model, cap), step, X, model, member)
        assert len(got) == len(want)
        for i, (a, b) in enumerate(zip(got, want)):
            assert a.shape == b.shape and np.array_equal(a, b, equal_nan=True), (step, i)
        if step in ("plain_device", "permutation", "stratified", "jackknife"):      # (the host entry point's sub-batches are batches of their own)
            problems = {"plain_device": B, "jackknife": n}.get(step, 2 * SPLITS)
            assert nm.get_option("last_boot_passes") == (-(-problems // cap) if cap else 1), step
        if step not in ("moments", "upload"):
            print(step, "n", n, "cap", cap, "converged", int(np.sum(got[1] == 0)), "of", got[1].size)
            assert np.mean(got[1] == 0) > 0.5, step       # (the sequence compares estimates, not failure codes)
        expected.update({kind: (n if count == "N" else count) for kind, count in EFFECT[step].items()})
        check_records(nm, expected)
