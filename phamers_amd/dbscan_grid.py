"""
dbscan_grid.py -- the table behind a choice of DBSCAN's ``eps`` and ``min_samples`` (the ``dbscan`` scoring method's
``scorer.eps`` / ``scorer.min_samples``, ``learning.dbscan``'s arguments): clusters, core, border and noise rows per cell of
an eps x min_samples grid, what scripts/cluster.py is to ``k_clusters``.

    grid(data, eps_values, min_samples_values)                  -> one batched device call (learning.dbscan_sweep)
    python -m phamers_amd.dbscan_grid -in FEATURES [-out FILE] --eps V [V ...] --min_samples M [M ...] [--silhouettes]
                                                                -> a CSV of eps, min_samples and the summary columns

The reference has no such study: its defaults (``eps = [1, 1]``) put every row of its normalised 4-mer data, whose rows lie
a few hundredths apart, into one cluster.  Plots are out of scope: the table is written as a CSV.
"""
import argparse
import os

import numpy as np

from . import fileIO, learning

COLUMNS = ("eps", "min_samples", "n_clusters", "n_core", "n_border", "n_noise", "largest", "silhouette")
_INT_COLUMNS = COLUMNS[1:7]


def grid(data, eps_values, min_samples_values, silhouettes=False):
    """The summary columns of ``learning.dbscan_sweep``'s records as a dict of arrays, one entry per cell in the sweep's
    order (eps outermost): ``eps`` and ``silhouette`` float64 (NaN where it was not asked for or is not defined), the others
    int64."""
    records = learning.dbscan_sweep(data, eps_values, min_samples_values, silhouettes=silhouettes)
    out = {"eps": np.array([r["eps"] for r in records], dtype=np.float64),
           "silhouette": np.array([r.get("silhouette", float("nan")) for r in records], dtype=np.float64)}
    for name in _INT_COLUMNS:
        out[name] = np.array([r[name] for r in records], dtype=np.int64)
    return out


def save_grid(filename, table, args=None):
    """One 'eps,min_samples,n_clusters,n_core,n_border,n_noise,largest,silhouette' row per cell (the floats as ``repr``
    prints them) under a '# ' comment header."""
    header = "DBSCAN parameter grid: " + ",".join(COLUMNS)
    if args is not None:
        header = fileIO.generate_summary(args, header=header).rstrip('\n')
    with open(filename, 'w') as f:
        f.write('# ' + header.replace('\n', '\n# ') + '\n')
        for i in range(len(table["eps"])):
            f.write('%r,%s,%r\n' % (float(table["eps"][i]), ','.join('%d' % int(table[name][i]) for name in _INT_COLUMNS),
                                    float(table["silhouette"][i])))


def read_grid(filename):
    """The dict of arrays of a file save_grid wrote."""
    rows = [line.strip().split(',') for line in open(filename) if not line.startswith('#') and line.strip()]
    out = {"eps": np.array([float(r[0]) for r in rows], dtype=np.float64),
           "silhouette": np.array([float(r[7]) for r in rows], dtype=np.float64)}
    for k, name in enumerate(_INT_COLUMNS):
        out[name] = np.array([int(r[1 + k]) for r in rows], dtype=np.int64)
    return out


def main(argv=None):
    parser = argparse.ArgumentParser(prog="python -m phamers_amd.dbscan_grid", description=__doc__.split('\n\n')[0])
    parser.add_argument("-in", "--features_file", required=True, help="Features file")
    parser.add_argument("-out", "--output_file", required=False, help="Filename for the output CSV")
    parser.add_argument("--eps", nargs='+', type=float, required=True, help="the eps values of the grid")
    parser.add_argument("--min_samples", nargs='+', type=int, required=True, help="the min_samples values of the grid")
    parser.add_argument("--silhouettes", action="store_true",
                        help="also the mean silhouette of the clustered rows of every cell (one more pass per cell)")
    args = parser.parse_args(argv)
    ids, data = fileIO.read_feature_file(args.features_file, normalize=True)
    table = grid(data, args.eps, args.min_samples, silhouettes=args.silhouettes)
    if args.output_file is None:
        filename = "%s_dbscan.csv" % os.path.splitext(os.path.basename(args.features_file))[0]
    else:
        filename = args.output_file
    save_grid(filename, table, args=args)
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
