"""NumPy restatement of the k-fold out-of-sample prediction (include/plspm_hip.h plspm_cv_device / plspm_cv_predict; plspm.predict) for the
tests: the Philox folds, the oracle's fit on every training set, the held-out predictions of both techniques, the linear-model benchmark by
lstsq on the raw training rows, and the pooled metrics.  Never calls the library."""
import numpy as np

import plspm_oracle as orc
from helpers_mga import philox4x32_10


def cv_keys(seed, rep, n):
    """key(i) = word i & 3 of Philox(counter = (i >> 2, 3, lo32(rep), hi32(rep)), key = (lo32(seed), hi32(seed)))."""
    q = np.arange((n + 3) // 4, dtype=np.uint64)
    words = philox4x32_10(q, 3, rep & 0xFFFFFFFF, rep >> 32, seed & 0xFFFFFFFF, seed >> 32)
    return np.stack(words, axis=1).reshape(-1)[:n].astype(np.uint32)


def cv_folds(seed, rep, n, k):
    """Fold of every row in repetition `rep`: the rows ordered by (key, row), position j belongs to fold (j * k) // n."""
    order = np.lexsort((np.arange(n), cv_keys(seed, rep, n)))
    fold = np.empty(n, dtype=np.uint8)
    fold[order] = (np.arange(n, dtype=np.int64) * k) // n
    return fold


def _find_cv_tie(seed, n, reps):
    """(rep, k, row a, row b): in repetition `rep` the rows a < b share a key, sit at adjacent sorted positions, and with k folds a fold boundary
    falls between them."""
    for rep in reps:
        keys = cv_keys(seed, rep, n)
        order = np.lexsort((np.arange(n), keys))
        ks = keys[order]
        for j in np.flatnonzero(ks[1:] == ks[:-1]):
            for k in range(2, 257):
                if (int(j) * k) // n != ((int(j) + 1) * k) // n:
                    return rep, k, int(order[j]), int(order[j + 1])
    return None


def targets(model):
    """Data columns of the target indicators in device column order: the blocks of every LV that has a predecessor."""
    return np.concatenate([model.blocks[l] for l in range(model.L) if model.C[l].sum() > 0])


def exogenous(model):
    return np.concatenate([model.blocks[l] for l in range(model.L) if model.C[l].sum() == 0])


def pls_predict(X, model, train, technique="direct"):
    """Predictions [held-out rows, T] of X[~train] from the oracle's fit on X[train], or None where that fit does not converge.  Also returns
    the fit (its `sign` tells whether a score was flipped)."""
    Xtr, Xte = X[train], X[~train]
    n = Xtr.shape[0]
    try:
        r = orc.fit(Xtr, model, orc.correction(n))
    except orc.NotConverged:
        return None, None
    mean = Xtr.mean(axis=0)
    g = np.std(Xtr.reshape(-1), ddof=1) * np.sqrt((n - 1) / n) if model.scaled else 1.0
    W = np.zeros((X.shape[1], model.L))
    for l, b in enumerate(model.blocks):
        W[b, l] = r["weights"][b]
    Y = ((Xte - mean) / g) @ W * r["sign"]                     # the scores Plspm.scores() would give the unseen rows under the training fit
    B = r["path_coef"]
    Yhat = np.zeros_like(Y)
    for j in range(model.L):
        for i in np.flatnonzero(model.C[j]):
            chain = technique == "earliest" and model.C[i].sum() > 0
            Yhat[:, j] += B[j, i] * (Yhat[:, i] if chain else Y[:, i])
    sd_x = np.std(Xtr, axis=0, ddof=0)
    sd_y = np.std(r["scores"], axis=0, ddof=0)
    cols = []
    for l in range(model.L):
        if model.C[l].sum() > 0:
            for p in model.blocks[l]:
                cols.append(mean[p] + r["loadings"][p] * sd_x[p] / sd_y[l] * Yhat[:, l])
    return np.column_stack(cols), r


def lm_predict(X, model, train):
    """The benchmark: every target regressed on an intercept + all indicators of the LVs without a predecessor, on the raw training rows."""
    ex, tg = exogenous(model), targets(model)
    A = np.column_stack((np.ones(int(train.sum())), X[train][:, ex]))
    beta = np.linalg.lstsq(A, X[train][:, tg], rcond=None)[0]
    return np.column_stack((np.ones(int((~train).sum())), X[~train][:, ex])) @ beta


def cross_validate(X, model, folds, k, technique="direct"):
    """`folds` [reps, N] fold ids.  Per problem q = r k + f: dict(rows = held-out row numbers, pred, lm [rows, T] (pred None: not converged),
    sse / sae / sst [T] of both, sign)."""
    tg = targets(model)
    out = []
    for r in range(folds.shape[0]):
        for f in range(k):
            train = folds[r] != f
            pred, fit = pls_predict(X, model, train, technique)
            lm = lm_predict(X, model, train)
            actual = X[~train][:, tg]
            d = actual - X[train][:, tg].mean(axis=0)
            item = dict(rows=np.flatnonzero(~train), pred=pred, lm=lm, sst=(d ** 2).sum(axis=0), sign=None if fit is None else fit["sign"],
                        iterations=None if fit is None else fit["iterations"])
            for name, p in (("", pred), ("lm_", lm)):
                if p is not None:
                    e = actual - p
                    item[name + "sse"], item[name + "sae"] = (e ** 2).sum(axis=0), np.abs(e).sum(axis=0)
            out.append(item)
    return out


def metrics(problems):
    """Pooled over the used problems (those whose PLS fit converged): dict of [T] arrays rmse, mae, q2_predict, lm.rmse, lm.mae, lm.q2_predict,
    and (problems used, rows covered)."""
    used = [p for p in problems if p["pred"] is not None]
    rows = float(sum(len(p["rows"]) for p in used))
    sst = sum(p["sst"] for p in used)
    out = {}
    for name, pre in (("", ""), ("lm_", "lm.")):
        sse, sae = sum(p[name + "sse"] for p in used), sum(p[name + "sae"] for p in used)
        out[pre + "rmse"], out[pre + "mae"], out[pre + "q2_predict"] = np.sqrt(sse / rows), sae / rows, 1.0 - sse / sst
    return out, (len(used), int(rows))


def mean_predictions(problems, n, key="pred"):
    """[N, T] the predictions of every row averaged over the used problems that held it out (NaN where none did)."""
    T = next(p[key].shape[1] for p in problems if p[key] is not None)
    total, count = np.zeros((n, T)), np.zeros(n)
    for p in problems:
        if p["pred"] is not None:
            total[p["rows"]] += p[key]
            count[p["rows"]] += 1
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(count[:, None] > 0, total / count[:, None], np.nan)


# ------------------------------------------------------------------ launch geometry of the prediction kernels, restated (plspm_cv.hip, kernels_cv.h)
CV_NT = 256                     # threads of a cv_apply_kernel workgroup
CV_MAX_LDS = 160 * 1024         # LDS a workgroup may take
RANK_CACHE_ROWS = 12288         # up to this many rows rank_select.h (cv_threshold_kernel, perm_threshold_kernel) keeps the keys in LDS


def cv_apply_lds(P, T, nrg):
    """Bytes of LDS cv_apply_kernel takes for T targets of P columns with row groups of nrg x 4 rows: the transposed matrix [P + 1][TS], the row tile
    [P][4 nrg + 2], the targets' means [TS] (doubles), their columns [TS] and the tile's rows [4 nrg] (ints); TS = T rounded up to four."""
    TS, XS = (T + 3) & ~3, 4 * nrg + 2
    return ((P + 1) * TS + P * XS + TS) * 8 + (TS + 4 * nrg) * 4


def cv_apply_row_groups(P, T):
    """Row groups per workgroup plspm_cv_predict picks: the first of 16, 8, 4 with a thread per (row group, four targets) whose tile fits the LDS; 0: refused."""
    for nrg in (16, 8, 4):
        if (CV_NT // nrg) * 4 >= T and cv_apply_lds(P, T, nrg) <= CV_MAX_LDS:
            return nrg
    return 0


def synth_sized(n, C, sizes, seed):
    """orc.synth with a block of sizes[l] indicators for LV l: (X [n, sum(sizes)], blocks)."""
    full, _ = orc.synth(n, np.asarray(C), max(sizes), seed=seed)
    m = max(sizes)
    X = np.column_stack([full[:, l * m:l * m + s] for l, s in enumerate(sizes)])
    off = np.concatenate(([0], np.cumsum(sizes)))
    return X, [np.arange(off[l], off[l + 1]) for l in range(len(sizes))]


def training_moments_longdouble(Xd, train):
    """(mean [P], centred cross-products [P, P], population sd [P]) of Xd[train] in extended precision, rounded to fp64 at the end."""
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63, "np.longdouble is not an extended format on this machine"
    x = Xd[train].astype(np.longdouble)
    n = x.shape[0]
    mean = x.sum(axis=0) / n
    xc = x - mean
    cross = np.empty((x.shape[1], x.shape[1]), dtype=np.longdouble)
    for p in range(x.shape[1]):                                # (a longdouble matmul is not BLAS: column by column keeps the temporaries small)
        cross[p] = (xc[:, [p]] * xc).sum(axis=0)
    sd = np.sqrt(np.diag(cross) / n)
    return mean.astype(np.float64), cross.astype(np.float64), sd.astype(np.float64)


def training_moments_two_pass(Xd, train):
    """The same in plain fp64 NumPy: mean, then the product of the centred rows."""
    x = Xd[train]
    mean = x.mean(axis=0)
    xc = x - mean
    return mean, xc.T @ xc
