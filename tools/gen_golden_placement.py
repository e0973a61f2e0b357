#!/usr/bin/env python3
"""
gen_golden_placement.py -- the parity fixture of the per-contig placement and taxonomy prediction,
tests/golden/placement.npz + placement.json, produced by running the REFERENCE's own code with the installed scikit-learn
and SciPy through tools/gen_golden.py's ``extract`` (no reference text is stored): learning.kmeans and
cluster_silhouettes (scripts/learning.py), taxonomy.find_enriched_classification (scripts/taxonomy.py) and
results_analyzer.get_taxonomy_prediction_dict (scripts/analysis.py:754-792) on an instance that carries only the attributes
that method reads.

Probe set: reference = the 2255 normalised phage rows of ref_features.npz (not stored again); 20 contigs = negative rows
0, 200, ..., 2200, six seeded uniform 5 kb contigs (stored), phage rows 0 and 1000 (exact duplicates of a reference row).
Per contig: the reference's assignments (int16) and cluster silhouettes; with a synthetic lineage table (six ranks per
phage, derived from the phage rows' own k-means clusters so that some clusters are enriched and some are not) the
prediction tuples and texts.  Plus small synthetic sets (D = 24 and 130, k = 2 and 7), stored whole.

Usage:  python tools/gen_golden_placement.py --ref <PhaMers checkout> [--out tests/golden]
"""
import argparse
import json
import logging
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tools'))
from gen_golden import extract  # noqa: E402

K_CLUSTERS = 86
NEG_ROWS = list(range(0, 2201, 200))
DUP_ROWS = [0, 1000]
N_UNIFORM = 6
SYNTH = (('s24', 300, 24, 2, 5), ('s130', 200, 130, 7, 5))   # name, rows, D, k, contigs


def load_reference(ref):
    import sklearn
    import scipy
    from scipy import stats
    from sklearn.cluster import DBSCAN, KMeans
    from sklearn.metrics import silhouette_samples, silhouette_score
    scripts = os.path.join(ref, 'scripts')
    quiet = logging.getLogger('reference')
    quiet.setLevel(logging.ERROR)
    kmer = extract(os.path.join(scripts, 'kmer.py'), ['normalize_counts'], {'np': np, 'xrange': range, 'logger': quiet})
    ns = {'np': np, 'xrange': range, 'logger': quiet, 'DBSCAN': DBSCAN, 'KMeans': KMeans,
          'silhouette_samples': silhouette_samples, 'silhouette_score': silhouette_score}
    learning = extract(os.path.join(scripts, 'learning.py'),
                       ['kmeans_seed', 'silhouettes', 'cluster_silhouettes', 'sort_assignment_by_size', 'kmeans'], ns)
    tax = extract(os.path.join(scripts, 'taxonomy.py'), ['find_enriched_classification'],
                  {'np': np, 'xrange': range, 'logger': quiet, 'stats': stats})
    analysis = extract(os.path.join(scripts, 'analysis.py'), ['results_analyzer'],
                       {'np': np, 'xrange': range, 'logger': quiet, 'learning': learning, 'tax': tax})
    return kmer, learning, tax, analysis, {'sklearn': sklearn.__version__, 'scipy': scipy.__version__, 'numpy': np.__version__}


def uniform_contigs(kmer):
    from oracle import oracle
    from phamers_amd import synth
    seqs = synth.synth_contigs(20260101, N_UNIFORM, 5000)
    return kmer.normalize_counts(np.asarray(oracle.count(seqs, 4)).astype(np.int64))


def lineage_table(km):
    """Six ranks per phage from its cluster c in the phage rows' own k-means: the family follows the cluster (enriched),
    the sub-family only in even clusters (scattered names elsewhere), the genus splits every cluster four ways."""
    rng = np.random.RandomState(7)
    out = []
    for i, c in enumerate(km.tolist()):
        sub = 'Subfamily%02d' % c if c % 2 == 0 else 'Scatter%02d' % rng.randint(0, 40)
        out.append(['Viruses', 'dsDNA viruses' if c % 7 else 'ssDNA viruses', 'Order%02d' % (c // 8), 'Family%02d' % (c // 3), sub,
                    'Genus%02d_%d' % (c, i % 4)])
    return out


def blobs(rows, D, k, contigs, seed):
    rng = np.random.RandomState(seed)
    centres = rng.uniform(-1, 1, (max(k, 3), D))
    X = centres[rng.randint(0, centres.shape[0], rows)] + 0.25 * rng.randn(rows, D)
    Z = centres[rng.randint(0, centres.shape[0], contigs)] + 0.25 * rng.randn(contigs, D)
    return X, Z


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ref', required=True, help='a checkout of the reference (jondeaton/PhaMers)')
    ap.add_argument('--out', default=os.path.join(REPO, 'tests', 'golden'))
    args = ap.parse_args()
    kmer, learning, tax, analysis, versions = load_reference(args.ref)
    with np.load(os.path.join(args.out, 'ref_features.npz')) as z:
        pos = kmer.normalize_counts(z['pos_counts'].astype(np.int64))
        neg = kmer.normalize_counts(z['neg_counts'].astype(np.int64))
    uni = uniform_contigs(kmer)
    contigs = np.vstack((neg[NEG_ROWS], uni, pos[DUP_ROWS]))
    ids = ['neg_%d' % r for r in NEG_ROWS] + ['uniform_%d' % i for i in range(N_UNIFORM)] + ['phage_%d' % r for r in DUP_ROWS]
    arrays = {'uniform_rows': uni, 'neg_rows': np.array(NEG_ROWS), 'dup_rows': np.array(DUP_ROWS), 'k_clusters': np.array([K_CLUSTERS])}

    km = np.asarray(learning.kmeans(pos, K_CLUSTERS))
    lineages = lineage_table(km)

    an = object.__new__(analysis.results_analyzer)
    an.phage_features, an.lineages, an.num_reference_phage = pos, lineages, pos.shape[0]
    an.contig_features, an.contig_ids = contigs, np.array(ids)
    an.k_clusters, an.ids_to_diagram = K_CLUSTERS, None
    an.phylogeny_names = ['Viruses', 'Baltimore', 'Order', 'Family', 'Sub-Family', 'Genus']
    an.get_virsorter_ids = lambda: ids
    # the method keeps the silhouettes and lineages but not the assignments: record those on their way through
    assignments = []
    ref_kmeans = learning.kmeans

    def recording_kmeans(data, k, **kw):
        a = np.asarray(ref_kmeans(data, k, **kw))
        assignments.append(a)
        return a
    learning.kmeans = recording_kmeans
    analysis.results_analyzer.get_taxonomy_prediction_dict.__globals__['learning'] = learning
    pred = an.get_taxonomy_prediction_dict()
    assert len(assignments) == len(ids)
    arrays['assignments'] = np.array(assignments).astype(np.int16)
    sil_len = np.array([len(an.cluster_silhouette_map[i]) for i in ids])
    arrays['sil_len'] = sil_len
    arrays['sil'] = np.concatenate([np.asarray(an.cluster_silhouette_map[i], dtype=np.float64) for i in ids])
    expected = {}
    for i in ids:
        if i in pred:
            (kind, res, ratio), text = pred[i]
            expected[i] = {'kind': kind, 'chi2': float(res[0]), 'p': float(res[1]), 'dof': int(res[2]),
                           'expected': np.asarray(res[3]).tolist(), 'ratio': float(ratio), 'text': text}
        else:
            expected[i] = None
        print(i, 'cluster', assignments[ids.index(i)][-1], 'members', sil_len[ids.index(i)] - 1, expected[i] and expected[i]['text'])

    # find_enriched_classification on every (probe cluster, depth), degenerate tables included
    enrich = []
    for i in ids:
        for depth in range(6):
            kind, res, ratio = tax.find_enriched_classification(an.cluster_lineage_map[i], lineages, depth)
            enrich.append({'id': i, 'depth': depth, 'kind': kind, 'ratio': ratio,
                           'chi2': None if res is None else float(res[0]), 'p': None if res is None else float(res[1]),
                           'dof': None if res is None else int(res[2]),
                           'expected': None if res is None else np.asarray(res[3]).tolist()})

    for name, rows, D, k, nc in SYNTH:
        X, Z = blobs(rows, D, k, nc, len(name) + D)
        arrays[name + '_X'], arrays[name + '_Z'], arrays[name + '_k'] = X, Z, np.array([k])
        labs, sils, lens = [], [], []
        for b in range(nc):
            app = np.vstack((X, Z[b:b + 1]))
            a = np.asarray(ref_kmeans(app, k))
            s = np.asarray(learning.cluster_silhouettes(app, a, a[-1]), dtype=np.float64)
            labs.append(a)
            sils.append(s)
            lens.append(len(s))
        arrays[name + '_assignments'] = np.array(labs).astype(np.int16)
        arrays[name + '_sil'] = np.concatenate(sils)
        arrays[name + '_sil_len'] = np.array(lens)

    path = os.path.join(args.out, 'placement.npz')
    np.savez_compressed(path, **arrays)
    with open(os.path.join(args.out, 'placement.json'), 'w') as f:
        json.dump({'versions': versions, 'ids': ids, 'lineages': lineages, 'predictions': expected, 'enrichment': enrich}, f,
                  indent=0, sort_keys=True)
    print('wrote %s (%d bytes) and placement.json (%d bytes)' % (path, os.path.getsize(path),
                                                                 os.path.getsize(os.path.join(args.out, 'placement.json'))))


if __name__ == '__main__':
    main()
