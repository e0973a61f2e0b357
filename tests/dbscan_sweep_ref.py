"""NumPy restatement of learning.dbscan_sweep (test-only): tests/cluster_ref.dbscan once per cell of the grid, in the order
``for eps in eps_values: for m in min_samples_values``, and the summary numbers of every cell."""
import numpy as np

from tests import cluster_ref

SUMMARY = ("n_clusters", "n_core", "n_border", "n_noise", "largest")


def summarize(labels, core):
    """The summary numbers of one cell from its labels (-1 = noise) and its core mask."""
    labels = np.asarray(labels)
    core = np.asarray(core, dtype=bool)
    clustered = labels >= 0
    sizes = np.bincount(labels[clustered]) if clustered.any() else np.zeros(1, dtype=int)
    return {"n_clusters": int(len(set(labels[clustered].tolist()))), "n_core": int(core.sum()),
            "n_border": int((clustered & ~core).sum()), "n_noise": int((~clustered).sum()), "largest": int(sizes.max())}


def dbscan_sweep(X, eps_values, min_samples_values):
    """One record per cell: eps, min_samples, labels (int64), core_sample_indices and the summary numbers."""
    records = []
    for eps in eps_values:
        for m in min_samples_values:
            labels, core = cluster_ref.dbscan(X, float(eps), int(m))
            record = {"eps": float(eps), "min_samples": int(m), "labels": labels, "core_sample_indices": np.flatnonzero(core)}
            record.update(summarize(labels, core))
            records.append(record)
    return records


def same_records(got, want, keys=("eps", "min_samples", "labels", "core_sample_indices") + SUMMARY):
    """assert that two lists of records agree in every key of ``keys`` (arrays by array_equal)."""
    assert len(got) == len(want), (len(got), len(want))
    for i, (g, w) in enumerate(zip(got, want)):
        for key in keys:
            if isinstance(w[key], np.ndarray) or isinstance(g[key], np.ndarray):
                assert np.asarray(g[key]).dtype.kind == np.asarray(w[key]).dtype.kind, (i, key)
                assert np.array_equal(g[key], w[key]), (i, key, g["eps"], g["min_samples"])
            else:
                assert g[key] == w[key], (i, key, g[key], w[key])
