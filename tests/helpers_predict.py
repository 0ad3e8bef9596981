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
