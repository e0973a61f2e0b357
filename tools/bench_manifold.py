"""Times the stages of phamers_amd.manifold on the device: PCA, neighbour graph, affinities, symmetrisation, and the
gradient iteration, for n = 4510 + {0, 1e4, 1e5} rows at d = 50 (synthetic blobs).  Prints one JSON line per size.

    python tools/bench_manifold.py [--sizes 4510,14510,104510] [--iters 50] [--cpu]

--cpu also times scikit-learn's TSNE (Barnes-Hut, reference parameters) on the host for the sizes below 20 000.
Kernel times: run under `rocprofv3 --kernel-trace --stats -- python tools/bench_manifold.py --sizes 104510`."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from phamers_amd import _lib, manifold   # noqa: E402


def blobs(n, d, seed=0):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, d)) + 4.0 * rng.standard_normal((20, d))[rng.integers(0, 20, n)]


def timed(fn):
    ctx = _lib.get_context()
    ctx.sync()
    t = time.perf_counter()
    out = fn()
    ctx.sync()
    return out, time.perf_counter() - t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4510,14510,104510")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--cpu", action="store_true")
    args = ap.parse_args()
    manifold.PCA(2).fit_transform(blobs(512, 8))   # warm-up: context, workspace
    for n in [int(s) for s in args.sizes.split(",")]:
        X256 = blobs(n, 256, 1)
        Z, t_pca = timed(lambda: manifold.PCA(50).fit_transform(X256))
        k = manifold.n_neighbors_for(n, 30.0)
        (idx, d2), t_nn = timed(lambda: manifold.neighbors(Z, k))
        (P, beta), t_aff = timed(lambda: manifold.conditional_affinities(d2, 30.0))
        csr, t_sym = timed(lambda: manifold.symmetrize(idx, P))
        Y0 = Z[:, :2] / np.std(Z[:, 0]) * 1e-4
        # per-iteration time from two descents of different length (uploads and the download cancel)
        _, t1 = timed(lambda: manifold.descend(Y0, csr, 10, learning_rate=2000.0))
        Y, t2 = timed(lambda: manifold.descend(Y0, csr, 10 + args.iters, learning_rate=2000.0))
        per_iter = (t2 - t1) / args.iters
        row = dict(n=n, k=k, pca_s=t_pca, neighbors_s=t_nn, affinities_s=t_aff, symmetrize_s=t_sym, iteration_ms=per_iter * 1e3,
                   pairs_per_s=n * (n - 1) / per_iter)
        if n <= 20000:
            t = manifold.TSNE(perplexity=30.0, early_exaggeration=1.0, random_state=10, init="pca", learning_rate=2000)
            _, row["fit_1000_iter_s"] = timed(lambda: t.fit_transform(Z))
            row["kl"] = t.kl_divergence_
            if args.cpu:
                from sklearn.manifold import TSNE
                t0 = time.perf_counter()
                TSNE(perplexity=30.0, early_exaggeration=1.0, random_state=10, init="pca", learning_rate=2000).fit_transform(Z)
                row["sklearn_barnes_hut_s"] = time.perf_counter() - t0
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
