"""Shared by the moderation tests (tests/test_moderation.py, tests/test_gpu_moderation.py) and the floor measurement (tools/moderation_floor.py): the cases
(data with a planted interaction), the NumPy mirror (plspm.moderation._moderation) of one data set in fp64 and in np.longdouble, the bar of the comparison,
the bootstrap's draws restated with tests/helpers_mga.philox4x32_10, the inputs of csrc/moderation_core.h (the needed LVs' correlations and the row sums in the
device's order) from the mirror's scores, and the figure behind the bar of the end-to-end check."""
import numpy as np

import plspm_oracle as orc
from helpers_mga import philox4x32_10
from plspm.moderation import _moderation
from plspm.plsc import _effect_pairs

SCHEME_ID = {"centroid": 0, "factorial": 1, "path": 2}
# The absolute floor of the bar (the project's rule for derived records): never below 1e-12; ten times the largest |fp64 mirror - longdouble mirror| where that
# is more (tools/moderation_floor.py; the figures: tests/test_gpu_moderation.py).
FLOOR = 1e-12


def native_model(model, X=None, **options):
    from plspm import _native
    boff = np.concatenate(([0], np.cumsum([len(b) for b in model.blocks]))).astype(np.int32)
    modes = np.array([0 if m == "A" else 1 for m in model.modes], dtype=np.int32)
    nm = _native.NativeModel(boff, model.C.astype(np.uint8), modes, SCHEME_ID[model.scheme], model.scaled, model.max_iter, model.tol, 0)
    for key, value in options.items():
        nm.set_option(key, value)
    if X is not None:
        nm.upload(X, model.mv_order.astype(np.int32))
    return nm


def fan_in(L):
    C = np.zeros((L, L), dtype=np.int64)
    C[L - 1, :L - 1] = 1
    return C


def planted(n, C, items, terms, seed, gamma=0.3):
    """Data with planted interactions: eta_j = sum_i 0.4 C[j, i] eta_i + gamma sum over the terms (a, b, j) of eta_a eta_b + noise; the indicators as
    oracle.synth makes them (loadings linspace(0.5, 0.9, k), noise 0.6).  items: per LV.  Returns (X [n, P], blocks)."""
    rng = np.random.default_rng(seed)
    L = C.shape[0]
    eps = rng.standard_normal((n, L))
    eta = np.zeros((n, L))
    for j in range(L):
        eta[:, j] = eps[:, j] + 0.4 * eta[:, C[j] == 1].sum(axis=1)
        for a, b, t in terms:
            if t == j:
                eta[:, j] += gamma * eta[:, a] * eta[:, b]
    cols, blocks, p = [], [], 0
    for j in range(L):
        k = items[j]
        lam = np.linspace(0.5, 0.9, k) if k > 1 else np.ones(1)
        noise = 0.6 * rng.standard_normal((n, k)) if k > 1 else np.zeros((n, 1))
        cols.append(eta[:, [j]] * lam[None, :] + noise)
        blocks.append(np.arange(p, p + k))
        p += k
    return np.hstack(cols), blocks


SAT_TERMS = [(0, 1, 4), (2, 3, 4), (0, 4, 5)]      # IMAG x EXPE -> SAT, QUAL x VAL -> SAT, IMAG x SAT -> LOY
CASES = ["one_term", "single_items", "mode_b", "satisfaction", "eight_terms", "fan_in_10", "wide_table", "n63", "n64", "n65", "n1100"]


def case(name):
    """(X, model, terms) of a case.  Every one of the nine resamples (``resamples``) and the full sample of every case has status 0 and passes every pivot
    test by the mirror alone on the oracle's records (tools/moderation_floor.py asserts it)."""
    def make(n, C, items, terms, seed, modes=None, scheme="centroid"):
        X, blocks = planted(n, C, items, terms, seed)
        return X, orc.Model(blocks, C, modes or "A" * C.shape[0], scheme, True), terms
    if name == "one_term":                                   # three LVs of three items, N = 70: ragged against every row block
        return make(70, fan_in(3), [3, 3, 3], [(0, 1, 2)], 1)
    if name == "single_items":                               # k = 1 blocks, the moderator included
        return make(300, fan_in(3), [1, 1, 1], [(0, 1, 2)], 2)
    if name == "mode_b":                                     # a Mode-B block as the moderator
        return make(300, fan_in(3), [4, 4, 4], [(0, 1, 2)], 3, modes="ABA", scheme="path")
    if name == "satisfaction":                               # 400 x 60: two terms on one target (a cross sum) and a third target
        return make(400, orc.satisfaction_C(), [10] * 6, SAT_TERMS, 4, scheme="path")
    if name == "eight_terms":                                # five LVs fanning into one target: eight of the ten pairs
        pairs = [(a, b, 5) for a in range(5) for b in range(a + 1, 5)][:8]
        return make(600, fan_in(6), [2] * 6, pairs, 5)
    if name == "fan_in_10":                                  # nine predecessors and a term: ten regressors, beyond the eight-in-registers solve
        return make(600, fan_in(10), [2] * 10, [(0, 1, 9)], 6)
    if name == "wide_table":                                 # 3 x 100 items: table and values together exceed the LDS, the lanes read the table from memory
        return make(400, fan_in(3), [100, 100, 100], [(0, 1, 2)], 7)
    if name in ("n63", "n64", "n65", "n1100"):               # part of a row block, one wave's 64 rows and one more, several row blocks with a ragged last one
        return make(int(name[1:]), fan_in(3), [2, 2, 2], [(0, 1, 2)], 8)
    raise KeyError(name)


def resamples(X, B=9, seed=17):
    return np.random.default_rng(seed).integers(0, X.shape[0], (B, X.shape[0])).astype(np.int32)


def counts_of(idx, n):
    return np.bincount(np.asarray(idx), minlength=n).astype(np.float64)


def philox_draws(seed, rep, n):
    """The bootstrap's draws of replicate `rep` (csrc/philox.h resample_quad, to_index): draw i is word i & 3 of Philox(counter = (i >> 2, 0, lo32(rep),
    hi32(rep)), key = (lo32(seed), hi32(seed))), mapped to [0, n) by the high word of the 32 x 32 product."""
    q = np.arange((n + 3) // 4, dtype=np.uint64)
    words = philox4x32_10(q, 0, rep & 0xFFFFFFFF, rep >> 32, seed & 0xFFFFFFFF, seed >> 32)
    u = np.stack(words, axis=1).reshape(-1)[:n].astype(np.uint64)
    return ((u * np.uint64(n)) >> np.uint64(32)).astype(np.int32)


def dev_blocks(model):
    off = np.concatenate(([0], np.cumsum([len(b) for b in model.blocks])))
    return [np.arange(off[l], off[l + 1]) for l in range(model.L)]


def record_parts(model, record):
    """(weights [P], r2 [L], direct [n_eff], loadings [P]) of a bootstrap record (weights | r2 | total | direct | loadings)."""
    ne = len(_effect_pairs(model.C))
    P, L = model.P, model.L
    return record[:P], record[P:P + L], record[P + L + ne:P + L + 2 * ne], record[P + L + 2 * ne:2 * P + L + 2 * ne]


def mirror_of(X, model, terms, counts, record, dtype):
    """plspm.moderation._moderation on the rows X (the model's column order is applied here) weighted by counts, fed the record's weights, loadings, direct and
    r2 entries."""
    w, r2, direct, lam = record_parts(model, np.asarray(record))
    return _moderation(np.asarray(X)[:, model.mv_order], counts, w, lam, dev_blocks(model), model.modes, model.C, terms, dtype, record_direct=direct, record_r2=r2)


def mirror_pair(X, model, terms, counts, record):
    return mirror_of(X, model, terms, counts, record, np.float64), mirror_of(X, model, terms, counts, record, np.longdouble)


def mirror_difference(m64, mld):
    return float(np.max(np.abs(m64["record"].astype(np.longdouble) - mld["record"])))


def mirror_bar(m64, mld, floor=FLOOR):
    """Ten times the largest difference between the fp64 and the longdouble mirror on the same inputs, at least `floor` (absolute)."""
    return max(10.0 * mirror_difference(m64, mld), floor)


def oracle_record(X, model, rows, n_all):
    """(the oracle's fit of X[rows], its record in the device layout)."""
    f = orc.fit(X[rows], model, orc.correction(n_all))
    return f, np.concatenate((f["weights"][model.mv_order], f["r2"], f["total"], f["direct"], f["loadings"][model.mv_order]))


# ---- the inputs of csrc/moderation_core.h, restated: the needed LVs and the order of the row sums
def needed_lvs(C, terms):
    need = set()
    for _, _, j in terms:
        need.add(j)
        need.update(np.flatnonzero(np.asarray(C)[j]).tolist())
    return sorted(need)


def sum_list(C, terms):
    """The row sums in the device's order, as (kind, ...) tuples: ("one", t), ("square", t), ("score", t, l) for l in pred(j) and then j -- per term --, then
    ("cross", t, u) for the terms t < u of one target."""
    out = []
    for t, (_, _, j) in enumerate(terms):
        out += [("one", t), ("square", t)] + [("score", t, int(l)) for l in np.flatnonzero(np.asarray(C)[j])] + [("score", t, j)]
    for t in range(len(terms)):
        for u in range(t + 1, len(terms)):
            if terms[t][2] == terms[u][2]:
                out.append(("cross", t, u))
    return out


def core_inputs(mirror, C, terms, counts):
    """(n, rc [nl, nl] of the needed LVs, sums) from the mirror's scores and products: what the prepare kernel and the row pass hand to the finish kernel."""
    Y, Z = mirror["scores"].astype(np.float64), mirror["products"].astype(np.float64)
    c = np.ones(Y.shape[0]) if counts is None else np.asarray(counts, dtype=np.float64)
    n = c.sum()
    need = needed_lvs(C, terms)
    Yn = Y[:, need]
    rc = (Yn * c[:, None]).T @ Yn / n
    rc = rc / np.sqrt(np.outer(np.diag(rc), np.diag(rc)))
    np.fill_diagonal(rc, 1.0)
    sums = []
    for s in sum_list(C, terms):
        if s[0] == "one":
            sums.append((c * Z[:, s[1]]).sum())
        elif s[0] == "square":
            sums.append((c * Z[:, s[1]] ** 2).sum())
        elif s[0] == "score":
            sums.append((c * Z[:, s[1]] * Y[:, s[2]]).sum())
        else:
            sums.append((c * Z[:, s[1]] * Z[:, s[2]]).sum())
    return n, rc, np.array(sums)


def perturbation_figure(X, model, terms, draws=20, rtol=1e-8, atol=1e-11, seed=0):
    """How far the moderated coefficients of the full sample move when the oracle's record moves inside the record bar (|d| <= atol + rtol |x|, uniform
    draws): the largest absolute change of direct2 and interaction over the draws (helpers_quality.perturbation_figure's method)."""
    rng = np.random.default_rng(seed)
    _, rec = oracle_record(X, model, np.arange(X.shape[0]), X.shape[0])
    pick = lambda m: np.concatenate((m["direct2"], m["interaction"]))
    base = pick(mirror_of(X, model, terms, None, rec, np.float64))
    worst = 0.0
    for _ in range(draws):
        moved = rec + rng.uniform(-1.0, 1.0, rec.shape[0]) * (atol + rtol * np.abs(rec))
        worst = max(worst, float(np.max(np.abs(pick(mirror_of(X, model, terms, None, moved, np.float64)) - base))))
    return worst
