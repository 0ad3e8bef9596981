"""One Fimix-sized call, timed: N rows of the bench model's six latent variables (the satisfaction path model on synthetic data), K = 1..8, `starts` random starts
each, in ONE plspm_fimix_device call.  GPU: warm, the median of `--reps` calls, host clock around call + sync (a call is hundreds of milliseconds).  `--mirror`: the
NumPy mirror's time on this CPU instead, per K from `--mirror-iterations` iterations of one problem, scaled to the iteration counts in `--iterations-json` (what
the GPU run printed).  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "plspm-python_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000)
    ap.add_argument("--starts", type=int, default=10)
    ap.add_argument("--kmax", type=int, default=8)
    ap.add_argument("--em-iterations", type=int, default=5000)
    ap.add_argument("--em-tolerance", type=float, default=1e-10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--mirror", action="store_true")
    ap.add_argument("--mirror-iterations", type=int, default=20)
    ap.add_argument("--iterations-json", default=None)
    args = ap.parse_args()
    import plspm_oracle as orc
    C = orc.satisfaction_C()
    X, blocks = orc.synth(args.rows, C, 10, seed=5)
    ks = list(range(1, args.kmax + 1))
    if args.mirror:
        from plspm.fimix import _fimix
        model = orc.Model(blocks, C, "AAAAAA", "path", True)
        scores = np.asarray(orc.fit(X, model)["scores"], dtype=np.float64)
        total = json.loads(args.iterations_json) if args.iterations_json else {str(K): args.starts * args.mirror_iterations for K in ks}
        per_iteration, seconds = {}, 0.0
        for K in ks:
            init = np.random.default_rng(K).integers(0, K, args.rows)
            t0 = time.perf_counter()
            out = _fimix(scores, C, K, init, args.mirror_iterations, 0.0)
            per_iteration[K] = (time.perf_counter() - t0) / out["iterations"]
            seconds += per_iteration[K] * total[str(K)]
        print(json.dumps({"what": "numpy mirror", "rows": args.rows, "seconds": seconds, "ms_per_iteration": {K: 1e3 * v for K, v in per_iteration.items()}}))
        return
    from plspm import _native
    boff = np.concatenate(([0], np.cumsum([len(b) for b in blocks]))).astype(np.int32)
    nm = _native.NativeModel(boff, C.astype(np.uint8), np.zeros(6, dtype=np.int32), 2, True, 100, 1e-6, 0)
    nm.upload(X)
    assert nm.fit(want_scores=True)["status"] == 0
    k_of = np.repeat(ks, args.starts)
    times = []
    for rep in range(args.reps + 1):
        nm.sync()
        t0 = time.perf_counter()
        nm.fimix(k_of, kmax=args.kmax, seed=args.seed, max_iter=args.em_iterations, tol=args.em_tolerance)
        nm.sync()
        times.append(time.perf_counter() - t0)
    rows, status, iters = nm.fimix_fetch()
    by_k = {int(K): int(iters[k_of == K].sum()) for K in ks}
    print(json.dumps({"what": "plspm_fimix_device", "rows": args.rows, "problems": len(k_of), "median_ms": 1e3 * float(np.median(times[1:])), "first_ms": 1e3 * times[0],
                      "all_ms": [round(1e3 * t, 3) for t in times[1:]], "iterations": by_k, "max_iterations": int(iters.max()),
                      "status_counts": {int(s): int((status == s).sum()) for s in np.unique(status)}, "lib": os.environ.get("PLSPM_HIP_LIB", "default")}))


if __name__ == "__main__":
    main()
