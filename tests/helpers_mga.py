"""NumPy restatement of the two-group permutation test (include/plspm_hip.h plspm_permutation_device / plspm_permutation_counts; plspm.mga)
for the tests: the Philox splits, the two group estimates on the oracle, the exceedance counts and the p-values."""
import numpy as np

import plspm_oracle as orc

_MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on uint64 arrays holding 32-bit words (the 32 x 32 -> 64 products fit)."""
    c = [np.asarray(v, dtype=np.uint64) & _MASK for v in (c0, c1, c2, c3)]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = np.uint64(k0 & 0xFFFFFFFF), np.uint64(k1 & 0xFFFFFFFF)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & _MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & _MASK]
        k0 = (k0 + np.uint64(0x9E3779B9)) & _MASK
        k1 = (k1 + np.uint64(0xBB67AE85)) & _MASK
    return c


def permutation_keys(seed, perm, n):
    """key(i) = word i & 3 of Philox(counter = (i >> 2, 1, lo32(perm), hi32(perm)), key = (lo32(seed), hi32(seed)))."""
    q = np.arange((n + 3) // 4, dtype=np.uint64)
    words = philox4x32_10(q, 1, perm & 0xFFFFFFFF, perm >> 32, seed & 0xFFFFFFFF, seed >> 32)
    return np.stack(words, axis=1).reshape(-1)[:n].astype(np.uint32)


def permutation_members(seed, perm, n, n1):
    """Group a of permutation `perm`: the n1 rows with the smallest (key, row) pairs."""
    order = np.lexsort((np.arange(n), permutation_keys(seed, perm, n)))
    member = np.zeros(n, dtype=bool)
    member[order[:n1]] = True
    return member


def find_tie(seed, n, perms):
    """(perm, n1) such that two rows of permutation `perm` share a key and the cut of group a falls between them (the first is the last
    member, the second is not), or None."""
    for perm in perms:
        keys = permutation_keys(seed, perm, n)
        order = np.lexsort((np.arange(n), keys))
        ks = keys[order]
        same = np.flatnonzero(ks[1:] == ks[:-1])          # sorted positions j, j + 1 with one key: n1 = j + 1 cuts between them
        if same.size:
            return perm, int(same[0]) + 1
    return None


def oracle_record(X, model, rows):
    """The oracle's estimate on X[rows] in the device record layout (weights | r2 | total | direct | loadings, device = model.mv_order column
    order) and its iteration count -- the group's own n and correction."""
    r = orc.fit(X[rows], model, orc.correction(int(np.count_nonzero(rows))))
    row = np.concatenate((r["weights"][model.mv_order], r["r2"], r["total"], r["direct"], r["loadings"][model.mv_order]))
    return row, r["iterations"]


def exceedance(records, status, observed_diff):
    """#{valid p : |d_p| >= |d_obs|} per column (NaN on either side: not >=) and the number of valid permutations, from the 2B records."""
    a, b = records[0::2], records[1::2]
    valid = (status[0::2] == 0) & (status[1::2] == 0)
    with np.errstate(invalid="ignore"):
        ge = np.abs(a[valid] - b[valid]) >= np.abs(observed_diff)[None, :]
    return ge.sum(axis=0).astype(np.int64), int(valid.sum())


def p_values(exceed, n_used, observed_diff):
    p = (1.0 + exceed) / (1.0 + n_used)
    p[np.isnan(observed_diff)] = np.nan
    return p
