"""GPU: the second and later passes of a batch (plspm_bootstrap.hip plspm_detail_bootstrap).  A batch is cut into passes of 2 GiB of scratch, which at test
sizes is always one pass; the test-only handle option "boot_pass" (include/plspm_hip_test.h) caps the problems per pass, so that the 0/1 count kernels of the
cross-validation, the jackknife, the permutation and the stratified bootstrap run with prob0 != 0, and the plain bootstrap's draws with a later replicate offset.

Every call runs uncapped (one pass, asserted) and with 256 problems per pass (two or three passes, asserted) on one handle and seed: records, status and
iteration counts are bit-identical -- the project's rule for any cut of a batch -- and two problems of the second pass and one of the last are the oracle's
at the record bar (rtol 1e-8, atol 1e-11, identical iteration counts)."""
import numpy as np
import pytest

import plspm_oracle as orc
from helpers import assert_close
from helpers_mga import oracle_record
from test_gpu_mga_bootstrap import oracle_rec
from test_gpu_predict import host_folds, native_model

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-8, 1e-11
CAP = 256
C3 = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0]])
N = 2000


def handle():
    X, blocks = orc.synth(N, C3, 3, seed=21)
    model = orc.Model(blocks, C3, "ABA", "path", True)
    return X, model, native_model(model, X)


def capped_and_not(nm, problems, call):
    """call() -> tuple of arrays, once uncapped and once with CAP problems per pass: the pass counts, and every array bit for bit."""
    nm.set_option("boot_pass", 0)
    whole = call()
    assert nm.get_option("last_boot_passes") == 1
    nm.set_option("boot_pass", CAP)
    assert nm.get_option("boot_pass") == CAP
    cut = call()
    passes = nm.get_option("last_boot_passes")
    assert passes == -(-problems // CAP) and passes > 1, passes
    nm.set_option("boot_pass", 0)
    for a, b in zip(whole, cut):
        assert a.shape == b.shape and np.array_equal(a, b, equal_nan=True)
    assert nm.get_option("last_gram_path") == 2
    return cut


def later_passes(problems):
    """Two problems of the second pass and the last problem of the last pass."""
    return CAP, CAP + 45, problems - 1


def check_oracle(X, model, records, q, rows):
    """rows: a mask of the problem's rows, or its draws as row numbers (with repeats: helpers_mga.oracle_record would count the non-zero row numbers as n)."""
    mine, its = oracle_record(X, model, rows) if rows.dtype == bool else oracle_rec(X, model, rows)
    assert records[1][q] == 0 and records[2][q] == its, (q, records[1][q], records[2][q], its)
    assert_close(records[0][q], mine, RTOL, ATOL, what="problem %d" % q)


def test_the_option_takes_multiples_of_256_only():
    from plspm import _native
    _, _, nm = handle()
    assert nm.get_option("boot_pass") == 0 and nm.get_option("last_boot_passes") == 0
    for bad in (-256, 1, 255, 257, 300):
        with pytest.raises(_native.NativeBackendError):
            nm.set_option("boot_pass", bad)
    nm.set_option("boot_pass", 512)
    assert nm.get_option("boot_pass") == 512
    nm.bootstrap_device(300, seed=1)                         # a cap above the batch changes nothing
    assert nm.get_option("last_boot_passes") == 1


def test_bootstrap_in_three_passes():
    from plspm import _native
    X, model, nm = handle()
    B, seed = 600, 17
    nm.set_option("gram_path", 2)

    def call():
        nm.bootstrap_device(B, seed=seed)
        return nm.fetch(0, B)
    records = capped_and_not(nm, B, call)
    for q in later_passes(B):
        idx = _native.bootstrap_indices(seed, q, N)
        mine, its = orc.bootstrap_replicate(X, model, idx, orc.correction(N))
        assert records[1][q] == 0 and records[2][q] == its, (q, records[2][q], its)
        assert_close(records[0][q], mine, RTOL, ATOL, what="replicate %d" % q)


def test_permutation_in_three_passes():
    """perm_counts_kernel with prob0 = 256 and 512 (permutations 128 .. and 256 ..)."""
    from plspm import _native
    X, model, nm = handle()
    B, n1, seed = 300, 800, 23

    def call():
        nm.permutation(B, n1, seed)
        return nm.fetch(0, 2 * B)
    records = capped_and_not(nm, 2 * B, call)
    for q in later_passes(2 * B):
        member = _native.permutation_members(seed, q // 2, N, n1)
        check_oracle(X, model, records, q, member if q % 2 == 0 else ~member)


def test_stratified_bootstrap_in_three_passes():
    """strat_counts_kernel with prob0 = 256 and 512."""
    from plspm import _native
    X, model, nm = handle()
    B, seed = 300, 29
    member = np.zeros(N, dtype=bool)
    member[np.random.default_rng(2).permutation(N)[:700]] = True

    def call():
        nm.stratified_bootstrap(B, member, seed)
        return nm.fetch(0, 2 * B)
    records = capped_and_not(nm, 2 * B, call)
    for q in later_passes(2 * B):
        d = _native.stratified_draws(seed, q // 2, member)
        check_oracle(X, model, records, q, d[:700] if q % 2 == 0 else d[700:])


def test_cross_validation_in_two_passes():
    """cv_counts_kernel with prob0 = 256: the second repetition's 256 folds.  The error sums, the predictions and the training moments behind the records are
    bit-identical too."""
    X, model, nm = handle()
    reps, k, seed = 2, 256, 31

    def call():
        nm.cv(reps, k, seed=seed)
        return nm.fetch(0, reps * k) + nm.cv_predict(reps, k, 0, predictions=True) + nm.cv_moments(reps, k)
    records = capped_and_not(nm, reps * k, call)
    folds = host_folds(seed, reps, N, k)
    assert np.array_equal(nm.cv_fold_ids(reps, k)[0], folds)
    for q in later_passes(reps * k):
        r, f = divmod(q, k)
        assert r == 1
        check_oracle(X, model, records, q, folds[r] != f)


def test_jackknife_in_three_passes():
    """jack_counts_kernel with prob0 = 256 and 512."""
    X, model, nm = handle()
    G = 600

    def call():
        nm.jackknife(G)
        return nm.jackknife_fetch(0, G) + nm.jackknife_stats(G)[:3]
    records = capped_and_not(nm, G, call)
    for q in later_passes(G):
        check_oracle(X, model, records, q, np.arange(N) % G != q)


def test_the_calls_that_bring_counts_refuse_alike():
    """plspm_bootstrap.hip counts_call_scope in front of all four: a handle without data is PLSPM_E_STATE (101), a non-metric one PLSPM_E_ARG (100) and says why."""
    from plspm import _native
    X, model, _ = handle()
    boff = np.concatenate(([0], np.cumsum([len(b) for b in model.blocks]))).astype(np.int32)
    modes = np.zeros(3, dtype=np.int32)
    member = np.arange(N) < 700

    def calls(nm):
        return (("plspm_permutation_device", lambda: nm.permutation(4, 800, 1)),
                ("plspm_stratified_bootstrap_device", lambda: nm.stratified_bootstrap(4, member[:nm.N], 1)),
                ("plspm_cv_device", lambda: nm.cv(2, 5, 1)),
                ("plspm_jackknife_device", lambda: nm.jackknife(10)))
    empty = _native.NativeModel(boff, model.C.astype(np.uint8), modes, 2, True, 100, 1e-6, 0)
    for who, call in calls(empty):
        with pytest.raises(_native.NativeBackendError, match=r"%s failed \(101\)" % who):
            call()
    nonmetric = _native.NativeModel(boff, model.C.astype(np.uint8), modes, 2, True, 100, 1e-6, 0, nonmetric=True)
    nonmetric.upload(X)
    for who, call in calls(nonmetric):
        with pytest.raises(_native.NativeBackendError, match=r"%s failed \(100\).*plain metric" % who):
            call()


def test_the_plan_is_what_runs():
    """csrc/batch_route.h through the emulation build (helpers_batch_route) against the handle's own report: the passes and the Gram route of this file's handle at
    B 600, uncapped and capped, on either Gram; and of a Scale.NUM handle of 300 rows."""
    import helpers_batch_route as hb
    import test_nm_route as nmr
    from test_gpu_nmwave import _handle
    emu = hb.load_emu()
    _, _, nm = handle()
    shape = hb.metric_shape([3, 3, 3], "ABA", C3, N)
    for gram_path in (0, 1):
        for cap in (0, CAP):
            nm.set_option("gram_path", gram_path)
            nm.set_option("boot_pass", cap)
            nm.bootstrap_device(600, seed=3)
            p = hb.plan(emu, shape, hb.call(600), gram_path=gram_path, boot_pass=cap)
            assert (p["passes"], p["gpath"]) == (nm.get_option("last_boot_passes"), nm.get_option("last_gram_path")) == (3 if cap else 1, 1 if gram_path else 2)
    Cn = orc.chain_C(2)
    X, blocks = orc.synth(300, Cn, 7, seed=21)
    num = _handle(X, blocks, Cn, "AA", "factorial")             # (Scale.NUM; sets gram_path 2)
    num.bootstrap_device(300, seed=3)
    p = hb.plan(emu, hb.nonmetric_shape(nmr.num_shape([7, 7], 300)), hb.call(300), gram_path=2)
    assert (p["passes"], p["gpath"]) == (num.get_option("last_boot_passes"), num.get_option("last_gram_path")) == (1, 2)
    assert p["nm_wave"] == num.get_option("last_nm_wave16") == 1
