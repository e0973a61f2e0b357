"""
cut_validator.py -- AUC against sequence cut length (PhaMers' scripts/cut_validator.py:32-114), and the producer of the
cut feature files it reads, which the reference does not ship (kmer.count_cuts: the cut rule is this project's own).

    t = tester(); t.cut_directory = 'cuts'; t.N_fold = 20
    t.make_cut_files('phage.fasta', 'bacteria.fasta', [1000, 5000, 10000])
    aucs = t.test_cut_response()          # {cut size: ROC AUC}

Every cut size is one N-fold cross validation on one resident GPU model (cross_validate.cross_validator) and one ROC
evaluation on the device (learning.predictor_performance).  The reference's plot is not drawn.
"""
import logging
import os
import re

import numpy as np

from . import cross_validate
from . import fileIO
from . import kmer
from . import learning
from . import phamer

logger = logging.getLogger(__name__)
logger.setLevel(logging.WARNING)


class tester(object):

    def __init__(self):
        self.cut_directory = None
        self.output_directory = None
        self.all_features_files = None
        self.N_fold = 20
        self.validator = None
        self.cut_sizes = []
        self.cut_file_map = None
        self.aucs = None

    def get_cut_file_map(self):
        """{cut size: [files of that cut size]} over the .csv files of ``cut_directory`` (scripts/cut_validator.py:44-58)."""
        self.all_features_files = [os.path.join(self.cut_directory, file) for file in sorted(os.listdir(self.cut_directory))
                                   if file.endswith(".csv")]
        cut_map = {}
        for file in self.all_features_files:
            cut_map.setdefault(get_cutsize_from_filename(file), []).append(file)
        return cut_map

    def make_cut_files(self, phage_fasta, bacteria_fasta, cut_sizes, k=4):
        """Writes ``phage_kmer_count_k<k>_c<cut>_s0.csv`` and ``bacteria_...`` into ``cut_directory`` for every cut size: the
        k-mer counts of kmer.count_cuts, one row per piece, in the legacy format ``test_cut_response`` reads (no id column, no
        header).  Returns the file names."""
        if not os.path.isdir(self.cut_directory):
            os.makedirs(self.cut_directory)
        written = []
        for cut_size in cut_sizes:
            for kind, fasta in (("phage", phage_fasta), ("bacteria", bacteria_fasta)):
                _, counts = kmer.count_cuts(fasta, k, cut_size)
                name = os.path.join(self.cut_directory, "%s_kmer_count_k%d_c%d_s0.csv" % (kind, k, cut_size))
                np.savetxt(name, counts, fmt='%d', delimiter=',')
                written.append(name)
        return written

    def test_cut_response(self):
        """{cut size: ROC AUC} of an ``N_fold`` cross validation of every cut size's phage / bacteria files
        (scripts/cut_validator.py:67-96)."""
        self.cut_file_map = self.get_cut_file_map()
        self.cut_sizes = sorted(self.cut_file_map.keys())
        self.aucs = np.zeros(len(self.cut_sizes))
        if self.validator is None:
            self.validator = cross_validate.cross_validator()
            self.validator.scoring_function = phamer.score_points
        self.validator.N = self.N_fold
        for i, cut_size in enumerate(self.cut_sizes):
            logger.info("Cross validating with cutsize: %d bp" % cut_size)
            files = self.cut_file_map[cut_size]
            phage_file = [file for file in files if os.path.basename(file).startswith("phage")][0]
            bacteria_file = [file for file in files if os.path.basename(file).startswith("bacteria")][0]
            self.validator.positive_data = fileIO.read_feature_file(phage_file, normalize=True, old=True)[1]
            self.validator.negative_data = fileIO.read_feature_file(bacteria_file, normalize=True, old=True)[1]
            phage_scores, bacteria_scores = self.validator.cross_validate()
            self.aucs[i] = learning.predictor_performance(phage_scores, bacteria_scores)[2]
        return dict(zip(self.cut_sizes, self.aucs))


def get_cutsize_from_filename(filename):
    """The cut size of a cut features file: 100000 for phage_kmer_count_k4_c100000_s0.csv, the example of
    scripts/cut_validator.py:99-114.  The reference takes the text between the FIRST "_c" and the next "_", which in its own
    example is the "ount" of "_count" (a ValueError); here it is the first "_c<digits>_" of the base name, which is the same
    field wherever the reference's rule finds a number.  ValueError for a name without one."""
    base = os.path.basename(filename)
    found = re.search(r"_c(\d+)_", base)
    if found is None:
        logger.error("Could not parse filename: %s" % base)
        raise ValueError("no _c<cut size>_ field in the file name %r" % base)
    return int(found.group(1))


def main(argv=None):
    import argparse
    parser = argparse.ArgumentParser("This script tests the cross validation performance impact of using cut sequences")
    parser.add_argument('-in', '--input_directory', required=True, help="Directory containing cuts")
    parser.add_argument('-out', '--output_directory', required=True, help="Directory to put output files in")
    parser.add_argument('-n', '--N_fold', default=20, type=int, help="N-fold cross validation")
    parser.add_argument('-v', '--verbose', action='store_true', help='Verbose output')
    parser.add_argument('--debug', action='store_true', help='Debug console')
    args = parser.parse_args(argv)
    logger.setLevel(logging.DEBUG if args.debug else logging.INFO if args.verbose else logging.WARNING)
    my_tester = tester()
    my_tester.N_fold = args.N_fold
    my_tester.cut_directory = args.input_directory
    my_tester.output_directory = args.output_directory
    for cut_size, auc in sorted(my_tester.test_cut_response().items()):
        print("%d\t%r" % (cut_size, float(auc)))
    return 0


if __name__ == '__main__':
    import sys
    sys.exit(main())
