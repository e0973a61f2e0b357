"""
analysis.py -- the taxonomy prediction of PhaMers' scripts/analysis.py (results_analyzer.get_taxonomy_prediction_dict,
:754-792): for every candidate contig, k-means of the reference phage rows with the contig's row appended, the phage that
share the contig's cluster, and the deepest rank at which one taxon is enriched among them.  All contigs are placed by ONE
batched device call (learning.place_contigs).  VirSorter / IMG parsing, contig diagrams and plots are out of scope: the
contigs to predict are ``contig_ids`` (the reference takes VirSorter's), narrowed by ``ids_to_diagram`` when it is set.
"""
import numpy as np

from . import learning
from . import taxonomy as tax


class taxonomy_predictor(object):
    """Attribute names are the reference's (results_analyzer): ``phage_features`` (n, D), ``lineages`` (one list of ranks per
    phage row), ``contig_features`` (N, D), ``contig_ids`` (N,), ``k_clusters``, ``ids_to_diagram`` (None = all),
    ``phylogeny_names``."""

    def __init__(self, phage_features, lineages, contig_features, contig_ids):
        self.phage_features = np.asarray(phage_features, dtype=np.float64)
        self.lineages = lineages
        self.contig_features = np.asarray(contig_features, dtype=np.float64)
        self.contig_ids = np.asarray(contig_ids)
        self.num_reference_phage = self.phage_features.shape[0]
        self.phylogeny_names = ['Viruses', 'Baltimore', 'Order', 'Family', 'Sub-Family', 'Genus']
        self.k_clusters = 86
        self.ids_to_diagram = None
        self.taxonomy_prediction_dict = {}
        self.cluster_silhouette_map = {}
        self.cluster_lineage_map = {}
        self.placement_routes = {}

    def get_taxonomy_prediction_dict(self):
        """Fills ``taxonomy_prediction_dict`` {id: ((taxon, (chi2, p, dof, expected), ratio), text)},
        ``cluster_silhouette_map`` and ``cluster_lineage_map`` as scripts/analysis.py:754-792 does, and returns the first."""
        self.taxonomy_prediction_dict = {}
        self.cluster_silhouette_map = {}
        self.cluster_lineage_map = {}
        self.placement_routes = {}
        ids = [id for id in self.contig_ids.tolist() if self.ids_to_diagram is None or id in self.ids_to_diagram]
        rows = []
        for id in ids:
            match = self.contig_features[self.contig_ids == id]
            if match.shape[0] != 1:
                raise ValueError("contig id %r names %d rows of contig_features, expected one" % (id, match.shape[0]))
            rows.append(match[0])
        if not ids:
            return self.taxonomy_prediction_dict
        placed = learning.place_contigs(self.phage_features, np.array(rows), self.k_clusters)
        for id, rec in zip(ids, placed):
            cluster_phage = rec['members']
            self.cluster_lineage_map[id] = np.array([self.lineages[i] for i in cluster_phage])
            self.cluster_silhouette_map[id] = rec['silhouettes']
            self.placement_routes[id] = rec['route']
            cluster_size = len(cluster_phage)
            if cluster_size > 0:
                for lineage_depth in range(5, -1, -1):
                    tup = tax.find_enriched_classification(self.cluster_lineage_map[id], self.lineages, lineage_depth)
                    if tup[0] is not None:
                        sil = self.cluster_silhouette_map[id][-1]
                        mean_sil = np.mean(self.cluster_silhouette_map[id][:-1])
                        std_sil = np.std(self.cluster_silhouette_map[id][:-1])
                        if sil < max(0, mean_sil - std_sil):
                            continue
                        tax_text = "{pct} {kind} ({taxon}), sil:{sil} ({mean_sil} +/- {std_sil}), p={p}"
                        tax_text = tax_text.format(kind=tup[0], pct=100.0 * tup[2], sil=sil, mean_sil=mean_sil, std_sil=std_sil,
                                                   p=tup[1][1], taxon=self.phylogeny_names[min(4, lineage_depth)])
                        self.taxonomy_prediction_dict[id] = (tup, tax_text)
                        break
        return self.taxonomy_prediction_dict
