"""Shared by the REBUS-PLS tests (tests/test_rebus.py, tests/test_gpu_rebus.py) and the timing tool (tools/rebus_time.py): the generators of the cases, the oracle
as the local estimator of the NumPy mirror (plspm.rebus._rebus), the mirror in fp64 and in np.longdouble on the same fp64 inputs, and the text the host program reads.
The bar of the comparisons is the project's existing one, helpers_fimix.bar."""
import numpy as np

import plspm_oracle as orc
from plspm.rebus import _rebus, _unpack

ONE_PATH = np.array([[0, 0], [1, 0]], dtype=np.int64)
TRI3 = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0]], dtype=np.int64)


def sized(n, C, sizes, seed):
    """orc.synth with a block of sizes[l] indicators for LV l, columns in device order: (X [n, sum(sizes)], model)."""
    C = np.asarray(C)
    full, _ = orc.synth(n, C, max(sizes), seed=seed)
    m = max(sizes)
    X = np.ascontiguousarray(np.column_stack([full[:, l * m:l * m + s] for l, s in enumerate(sizes)]))
    off = np.concatenate(([0], np.cumsum(sizes)))
    return X, orc.Model([np.arange(off[l], off[l + 1]) for l in range(len(sizes))], C, "A" * len(sizes), "path", True)


def planted(n, seed=1, share=0.4):
    """Two classes (the first ``share`` of the rows and the rest) that differ in their loadings (each class has its own weak indicator per block) and in their paths
    (0 -> 1 changes its sign): three LVs, paths 0 -> 1, 0 -> 2, 1 -> 2, three indicators each.  Returns (X [n, 9], model, classes [n])."""
    rng = np.random.default_rng(seed)
    n_a = int(round(share * n))
    cls = (np.arange(n) >= n_a).astype(np.int64)
    lam = (np.array([[.9, .85, .2], [.9, .2, .85], [.2, .9, .85]]), np.array([[.2, .85, .9], [.2, .9, .85], [.9, .85, .2]]))
    beta = (dict(b01=.8, b02=.6, b12=.2), dict(b01=-.8, b02=-.2, b12=.7))
    X = np.empty((n, 9))
    for s in range(2):
        r = np.flatnonzero(cls == s)
        eta = np.empty((len(r), 3))
        eta[:, 0] = rng.normal(size=len(r))
        eta[:, 1] = beta[s]["b01"] * eta[:, 0] + 0.4 * rng.normal(size=len(r))
        eta[:, 2] = beta[s]["b02"] * eta[:, 0] + beta[s]["b12"] * eta[:, 1] + 0.4 * rng.normal(size=len(r))
        eta = (eta - eta.mean(axis=0)) / eta.std(axis=0)
        for l in range(3):
            X[np.ix_(r, np.arange(3 * l, 3 * l + 3))] = eta[:, [l]] * lam[s][l] + np.sqrt(1 - lam[s][l] ** 2) * rng.normal(size=(len(r), 3))
    return X, orc.Model([np.arange(3 * l, 3 * l + 3) for l in range(3)], TRI3, "AAA", "path", True), cls


def flipped(cls, share, seed):
    """``cls`` with ``share`` of the labels flipped (two classes)."""
    rng = np.random.default_rng(seed)
    out = cls.copy()
    flip = rng.choice(len(cls), int(round(share * len(cls))), replace=False)
    out[flip] = 1 - out[flip]
    return out


def random_start(n, K, seed):
    """Random labels with classes of nearly equal size."""
    return np.random.default_rng(seed).permutation(np.arange(n) % K).astype(np.int64)


def oracle_fit(model):
    """The oracle as ``_rebus``'s local estimator: the fit of the rows Xk with their own n (as a bootstrap replicate has), None where it does not converge."""
    def fit(Xk):
        try:
            r = orc.fit(Xk, model)
        except orc.NotConverged:
            return None
        if not np.all(np.isfinite(r["weights"])):
            return None
        return dict(weights=r["weights"], loadings=r["loadings"], path_coef=r["path_coef"], r2=r["r2"], iterations=r["iterations"])
    return fit


def mirror_pair(X, model, K, start, **kw):
    """(fp64 mirror, longdouble mirror) of one run on the same fp64 rows and the same local models."""
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63, "np.longdouble is not an extended format on this machine"
    return _rebus(X, model, K, start, dtype=np.float64, **kw), _rebus(X, model, K, start, dtype=np.longdouble, **kw)


def native_model(X, model, **options):
    """A handle with the rows uploaded (device column order = the model's column order)."""
    from plspm import _native
    boff = np.concatenate(([0], np.cumsum([len(b) for b in model.blocks]))).astype(np.int32)
    modes = np.array([0 if mode == "A" else 1 for mode in model.modes], dtype=np.int32)
    nm = _native.NativeModel(boff, model.C.astype(np.uint8), modes, {"centroid": 0, "factorial": 1, "path": 2}[model.scheme], model.scaled, model.max_iter, model.tol, 0)
    for key, value in options.items():
        nm.set_option(key, value)
    nm.upload(X)
    return nm


def device_records(nm, run):
    """The local records of a device run as the dicts ``_rebus`` takes (None where the local fit is not OK)."""
    return [_unpack(run["records"][k], nm.P, nm.L, nm.eff_from, nm.eff_to) if run["rec_status"][k] == 0 else None for k in range(len(run["rec_status"]))]


def effect_pairs(C):
    return orc.effects(np.asarray(C, dtype=np.float64))[0]


def record_row(fit, C):
    """A fit dict as a device record [weights | r2 | total | direct | loadings]; total and direct carry the path coefficients of the effect pairs (total is not read)."""
    pairs = effect_pairs(C)
    direct = np.array([fit["path_coef"][t, f] for f, t in pairs])
    return np.concatenate((fit["weights"], fit["r2"], direct, direct, fit["loadings"]))


def host_input(X, model, K, labels, fits):
    """The text tests/rebus_host reads for one step on the local models ``fits`` (dicts, or None: status 1 and a record of zeros)."""
    pairs = effect_pairs(model.C)
    boff = np.concatenate(([0], np.cumsum([len(b) for b in model.blocks])))
    fmt = lambda row: " ".join(repr(float(v)) for v in row)
    R = 2 * model.P + model.L + 2 * len(pairs)
    lines = ["%d %d %d %d %d" % (model.L, len(pairs), int(model.scaled), K, X.shape[0]), " ".join(str(int(v)) for v in boff),
             " ".join(str(int(f)) for f, _ in pairs), " ".join(str(int(t)) for _, t in pairs), " ".join(str(int(v)) for v in model.C.ravel())]
    for fit in fits:
        lines.append("1 " + fmt(np.zeros(R)) if fit is None else "0 " + fmt(record_row(fit, model.C)))
    lines.append(" ".join(str(int(v)) for v in labels))
    lines += [fmt(row) for row in X]
    return "\n".join(lines) + "\n"
