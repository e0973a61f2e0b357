"""
mixture_grid.py -- the number of components of a multinomial mixture chosen from the data (this project's own; DESIGN.md
section 4.25): what svm_grid.py is to the svm method's parameters and bandwidth.py to the density method's.  Every fit of
the grid runs in lock step on the device (``mixture.sweep`` / ``mixture.cross_validate``).

    python -m phamers_amd.mixture_grid -pf FILE -nf FILE -K 8 32 86 256 -N FOLDS -out FILE
        one row per K: K,auc,accuracy,held_out_per_kmer_positive,held_out_per_kmer_negative,bic_positive,bic_negative,
        mean_iterations,dead -- the held-out scores l_+ - l_- under the fold's two fitted mixtures
    python -m phamers_amd.mixture_grid -in FEATURES|FASTA -K ... -N FOLDS -out FILE
        one row per K: K,held_out_per_kmer,bic,mean_iterations,dead

The integers are written as integers, the floats as ``repr`` prints them, under a '# ' comment header and the column line.
"""
import argparse

import numpy as np

from . import _lib, fileIO, mixture

TWO_CLASS_COLUMNS = ("K", "auc", "accuracy", "held_out_per_kmer_positive", "held_out_per_kmer_negative", "bic_positive",
                     "bic_negative", "mean_iterations", "dead")
ONE_FILE_COLUMNS = ("K", "held_out_per_kmer", "bic", "mean_iterations", "dead")
INTEGERS = ("K", "dead")


def two_class_table(result):
    """One dict of TWO_CLASS_COLUMNS per K from a ``mixture.cross_validate(..., bic=True)``."""
    return [dict(K=K, **{name: getattr(result, name)[b] for name in TWO_CLASS_COLUMNS[1:]})
            for b, K in enumerate(result.n_components)]


def save_grid(filename, columns, table, args=None):
    """One row per K under a '# ' comment header and the line of ``columns``."""
    header = "Mixture component grid"
    if args is not None:
        header = fileIO.generate_summary(args, header=header).rstrip('\n')
    with open(filename, 'w') as f:
        f.write('# ' + header.replace('\n', '\n# ') + '\n')
        f.write(",".join(columns) + '\n')
        for row in table:
            f.write(",".join("%d" % row[name] if name in INTEGERS else repr(float(row[name])) for name in columns) + '\n')


def read_grid(filename):
    """(columns, one dict per K) of a file ``save_grid`` wrote."""
    lines = [line.strip() for line in open(filename) if not line.startswith('#') and line.strip()]
    columns = tuple(lines[0].split(','))
    return columns, [{name: (int(v) if name in INTEGERS else float(v)) for name, v in zip(columns, line.split(','))}
                     for line in lines[1:]]


def _parser():
    ap = argparse.ArgumentParser(prog="python -m phamers_amd.mixture_grid", description=__doc__.split('\n\n')[0],
                                 formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    ap.add_argument('-pf', '--positive_features_file', help="Positive features (count) file")
    ap.add_argument('-nf', '--negative_features_file', help="Negative features (count) file")
    ap.add_argument('-in', '--input_file', help="One features (count) file, or FASTA file to count")
    ap.add_argument('-k', '--kmer_length', type=int, default=4, help="k-mer length when the input is a FASTA file")
    ap.add_argument('-K', '--components', type=int, nargs='+', required=True, help="The component counts of the grid")
    ap.add_argument('-N', '--N_fold', type=int, required=True, help="Folds of the validator's split")
    ap.add_argument('--seed', type=int, default=None, help="Seed of the fold assignment")
    ap.add_argument('--fit_seed', type=int, default=0, help="Seed of the first start of every fit")
    ap.add_argument('--n_init', type=int, default=1, help="Seeded starts per fit; the largest evidence is kept")
    ap.add_argument('--max_iter', type=int, default=100, help="Most M-steps of a start")
    ap.add_argument('--tol', type=float, default=1e-6, help="Relative gain of the evidence below which EM stops")
    ap.add_argument('--pseudocount', type=float, default=0.5, help="Pseudocount of the profiles")
    ap.add_argument('-out', '--output_file', required=True, help="CSV to write")
    return ap


def main(argv=None):
    ap = _parser()
    args = ap.parse_args(argv)
    two = bool(args.positive_features_file and args.negative_features_file)
    if two == bool(args.input_file) or (not two and (args.positive_features_file or args.negative_features_file)):
        ap.error("give both -pf FILE and -nf FILE, or -in FILE")
    if two:
        pos = fileIO.read_feature_file(args.positive_features_file, normalize=False)[1]
        neg = fileIO.read_feature_file(args.negative_features_file, normalize=False)[1]
        res = mixture.cross_validate(pos, neg, args.components, args.N_fold, args.seed, args.fit_seed, args.n_init,
                                     args.pseudocount, args.max_iter, args.tol, bic=True)
        save_grid(args.output_file, TWO_CLASS_COLUMNS, two_class_table(res), args)
        return 0
    fasta = batch = None
    try:
        if mixture._is_fasta(args.input_file):
            fasta = _lib.Fasta(args.input_file)
            data = batch = _lib.Batch.from_fasta(_lib.get_context(), fasta, args.kmer_length)
        else:
            data = fileIO.read_feature_file(args.input_file, normalize=False)[1]
        sw = mixture.sweep(data, args.components, args.N_fold, args.seed, args.fit_seed, args.n_init, args.pseudocount,
                           args.max_iter, args.tol)
    finally:
        if batch is not None:
            batch.close()
        if fasta is not None:
            fasta.close()
    save_grid(args.output_file, ONE_FILE_COLUMNS, sw.table(), args)
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
