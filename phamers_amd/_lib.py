"""
ctypes binding of libphamers_hip.so (include/phamers_hip.h).

The library is the product: there is no CPU fallback.  If the shared object is
missing, or no gfx950 device can be opened, every operation raises.
"""
import ctypes
import os
import threading

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libphamers_hip.so")

PHK_OK = 0
PHK_ERR_ARG, PHK_ERR_HIP, PHK_ERR_NOMEM, PHK_ERR_UNSUPPORTED, PHK_ERR_NAN, PHK_ERR_IO = -1, -2, -3, -4, -5, -6
METHOD_KNN, METHOD_KMEANS, METHOD_COMBO, METHOD_DENSITY, METHOD_SVM = 1, 2, 3, 4, 5
METHODS = {"knn": METHOD_KNN, "kmeans": METHOD_KMEANS, "combo": METHOD_COMBO, "density": METHOD_DENSITY, "svm": METHOD_SVM}
MAX_K = 7
SORT_TILE, SORT_MAX_BLOCKS = 4096, 512   # PHK_SORT_TILE, PHK_SORT_MAX_BLOCKS
ABI_VERSION = 2

c_void_p, c_int, c_u32, c_u64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint64
c_char_p, c_double = ctypes.c_char_p, ctypes.c_double
P = ctypes.POINTER

# name -> (restype, argtypes); one entry per function declared in include/phamers_hip.h
SIGNATURES = {
    "phk_abi_version": (c_int, []),
    "phk_last_error": (c_char_p, []),
    "phk_device_count": (c_int, [P(c_int)]),
    "phk_create": (c_int, [c_int, c_void_p, P(c_void_p)]),
    "phk_destroy": (c_int, [c_void_p]),
    "phk_sync": (c_int, [c_void_p]),
    "phk_set_option": (c_int, [c_void_p, c_char_p, c_char_p]),
    "phk_malloc": (c_int, [c_void_p, c_u64, P(c_void_p)]),
    "phk_free": (c_int, [c_void_p, c_void_p]),
    "phk_memcpy_h2d": (c_int, [c_void_p, c_void_p, c_void_p, c_u64]),
    "phk_memcpy_d2h": (c_int, [c_void_p, c_void_p, c_void_p, c_u64]),
    "phk_count_ascii": (c_int, [c_void_p, c_void_p, c_void_p, c_u64, c_int, c_char_p, c_void_p]),
    "phk_normalize_i64": (c_int, [c_void_p, c_void_p, c_u64, c_u64, c_void_p]),
    "phk_normalize_f64": (c_int, [c_void_p, c_void_p, c_u64, c_u64, c_void_p]),
    "phk_permute_columns_i64": (c_int, [c_void_p, c_void_p, c_u64, c_u64, c_void_p, c_void_p]),
    "phk_fold_strands_i64": (c_int, [c_void_p, c_void_p, c_u64, c_u64, c_void_p]),
    "phk_fasta_read": (c_int, [c_char_p, c_int, P(c_void_p)]),
    "phk_fasta_index": (c_int, [c_char_p, c_int, P(c_void_p)]),
    "phk_fasta_read_range": (c_int, [c_char_p, c_u64, c_u64, c_int, P(c_void_p)]),
    "phk_fasta_read_part": (c_int, [c_char_p, c_u32, c_u32, c_int, P(c_void_p)]),
    "phk_fasta_shape": (c_int, [c_void_p, P(c_u64), P(c_u64), P(c_u64)]),
    "phk_fasta_data": (c_int, [c_void_p, P(c_void_p), P(c_void_p), P(c_void_p), P(c_void_p)]),
    "phk_fasta_free": (c_int, [c_void_p]),
    "phk_parse_id": (c_int, [c_char_p, c_u64, c_char_p, c_u64, P(c_u64), P(c_int)]),
    "phk_fasta_ids": (c_int, [c_void_p, P(c_void_p), P(c_void_p), P(c_void_p)]),
    "phk_fasta_ids_fixed": (c_int, [c_void_p, c_u64, c_void_p]),
    "phk_count_fasta": (c_int, [c_void_p, c_void_p, c_int, c_char_p, c_void_p]),
    "phk_batch_from_ascii": (c_int, [c_void_p, c_void_p, c_void_p, c_u64, c_int, c_char_p, P(c_void_p)]),
    "phk_batch_from_fasta": (c_int, [c_void_p, c_void_p, c_int, c_char_p, P(c_void_p)]),
    "phk_batch_from_counts": (c_int, [c_void_p, c_void_p, c_u64, c_u64, P(c_void_p)]),
    "phk_batch_windows_from_ascii": (c_int, [c_void_p, c_void_p, c_void_p, c_u64, c_int, c_char_p, c_u64, c_u64, c_u32, P(c_void_p)]),
    "phk_batch_windows_from_fasta": (c_int, [c_void_p, c_void_p, c_int, c_char_p, c_u64, c_u64, c_u32, P(c_void_p)]),
    "phk_windows_grid_pass": (c_int, [c_int, P(c_u64)]),
    "phk_batch_from_fasta_file": (c_int, [c_void_p, c_char_p, c_int, c_char_p, c_int, P(c_void_p), P(c_void_p)]),
    "phk_batch_from_fasta_part": (c_int, [c_void_p, c_char_p, c_u32, c_u32, c_int, c_char_p, c_int, P(c_void_p), P(c_void_p)]),
    "phk_batch_shape": (c_int, [c_void_p, P(c_u64), P(c_u64), P(c_u64), P(c_int)]),
    "phk_batch_device_ptrs": (c_int, [c_void_p, P(c_void_p), P(c_void_p)]),
    "phk_batch_counts_i64": (c_int, [c_void_p, c_void_p, c_void_p]),
    "phk_batch_counts_u32": (c_int, [c_void_p, c_void_p, c_void_p]),
    "phk_write_counts_csv": (c_int, [c_char_p, c_char_p, c_void_p, c_void_p, c_void_p, c_int, c_u64, c_u64]),
    "phk_write_scores_csv": (c_int, [c_char_p, c_char_p, c_void_p, c_void_p, c_void_p, c_u64]),
    "phk_write_counts_csv_ucs4": (c_int, [c_char_p, c_char_p, c_void_p, c_u64, c_void_p, c_int, c_u64, c_u64]),
    "phk_write_scores_csv_ucs4": (c_int, [c_char_p, c_char_p, c_void_p, c_u64, c_void_p, c_u64]),
    "phk_format_float": (c_int, [c_double, c_char_p, c_int]),
    "phk_features_open": (c_int, [c_char_p, P(c_void_p), P(c_u64), P(c_u64), P(c_u64)]),
    "phk_features_read": (c_int, [c_void_p, c_void_p, c_void_p, c_u64]),
    "phk_features_close": (c_int, [c_void_p]),
    "phk_batch_normalized": (c_int, [c_void_p, c_void_p, c_void_p]),
    "phk_batch_select": (c_int, [c_void_p, c_void_p, c_void_p, c_u64, P(c_void_p)]),
    "phk_batch_column_sums": (c_int, [c_void_p, c_void_p, c_void_p]),
    "phk_batch_gather_columns": (c_int, [c_void_p, c_void_p, c_void_p, P(c_void_p)]),
    "phk_batch_fold_strands": (c_int, [c_void_p, c_void_p]),
    "phk_batch_strands": (c_int, [c_void_p, P(c_int)]),
    "phk_fold_grid_pass": (c_int, [c_int, P(c_u64)]),
    "phk_batch_score": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    "phk_batch_free": (c_int, [c_void_p, c_void_p]),
    "phk_kmeans": (c_int, [c_void_p, c_void_p, c_u64, c_u64, c_u32, c_u64, c_int, c_void_p, c_void_p, P(c_int)]),
    "phk_kmeans_lloyd": (c_int, [c_void_p, c_void_p, c_u64, c_u64, c_u32, c_void_p, c_double, c_int, c_void_p, c_void_p, P(c_int),
                                 P(c_int), P(c_double)]),
    "phk_model_create": (c_int, [c_void_p, c_void_p, c_u64, c_void_p, c_u64, c_void_p, c_u64,
                                 c_void_p, c_u64, c_u64, c_int, P(c_void_p)]),
    "phk_model_destroy": (c_int, [c_void_p, c_void_p]),
    "phk_model_set_centroids": (c_int, [c_void_p, c_void_p, c_void_p, c_u64, c_void_p, c_u64]),
    "phk_model_set_column_mask": (c_int, [c_void_p, c_void_p, c_void_p]),
    "phk_model_set_bandwidths": (c_int, [c_void_p, c_void_p, c_double, c_double]),
    "phk_kde_log_density": (c_int, [c_void_p, c_void_p, c_u64, c_void_p, c_u64, c_u64, c_double, c_void_p]),
    "phk_kde_sweep": (c_int, [c_void_p, c_void_p, c_u64, c_void_p, c_u64, c_u64, c_void_p, c_u32, c_int, c_u64, c_void_p]),
    "phk_lik_table_create": (c_int, [c_void_p, c_void_p, c_u64, c_void_p, c_void_p, c_u64, c_void_p, c_u64, P(c_void_p)]),
    "phk_lik_table_destroy": (c_int, [c_void_p, c_void_p]),
    "phk_lik_score": (c_int, [c_void_p, c_void_p, c_void_p, c_u64, c_u64, c_void_p, c_u64, c_void_p, c_void_p, c_void_p]),
    "phk_batch_lik_score": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "phk_mix_table_create": (c_int, [c_void_p, c_void_p, c_void_p, c_u64, c_u64, P(c_void_p)]),
    "phk_mix_table_update": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_u64, c_u64]),
    "phk_mix_table_destroy": (c_int, [c_void_p, c_void_p]),
    "phk_mix_block_rows": (c_u64, []),
    "phk_mix_expect": (c_int, [c_void_p, c_void_p, c_void_p, c_u64, c_u64, c_u64, c_void_p, c_void_p, c_void_p, c_void_p,
                               c_void_p, c_void_p]),
    "phk_batch_mix_expect": (c_int, [c_void_p, c_void_p, c_void_p, c_u64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                     c_void_p]),
    "phk_mix_responsibilities": (c_int, [c_void_p, c_void_p, c_void_p, c_u64, c_u64, c_u64, c_void_p, c_void_p]),
    "phk_batch_mix_responsibilities": (c_int, [c_void_p, c_void_p, c_void_p, c_u64, c_void_p, c_void_p]),
    "phk_mix_sweep_create": (c_int, [c_void_p, c_void_p, c_u64, c_u64, c_void_p, c_void_p, c_u64, P(c_void_p)]),
    "phk_batch_mix_sweep_create": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_u64, P(c_void_p)]),
    "phk_mix_sweep_step": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_u64, c_void_p, c_void_p, c_int, c_int, c_u64,
                                   c_void_p]),
    "phk_mix_sweep_destroy": (c_int, [c_void_p, c_void_p]),
    "phk_host_table_create": (c_int, [c_void_p, c_void_p, c_u64, c_u64, c_void_p, P(c_void_p)]),
    "phk_host_table_destroy": (c_int, [c_void_p, c_void_p]),
    "phk_host_rank": (c_int, [c_void_p, c_void_p, c_void_p, c_u64, c_u64, c_void_p, c_int, c_u64, c_void_p, c_void_p]),
    "phk_batch_host_rank": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    "phk_host_null_fit": (c_int, [c_void_p, c_void_p, c_void_p, c_u64, c_u64, c_u64, c_void_p, c_void_p]),
    "phk_segment_decode": (c_int, [c_void_p, c_void_p, c_u64, c_void_p, c_u64, c_void_p, c_void_p, c_void_p, c_void_p,
                                   c_void_p, c_void_p, c_void_p, c_void_p]),
    "phk_segment_grid_pass": (c_u64, []),
    "phk_segment_expect": (c_int, [c_void_p, c_void_p, c_u64, c_void_p, c_u64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                   c_void_p]),
    "phk_segment_fit": (c_int, [c_void_p, c_void_p, c_u64, c_void_p, c_u64, c_void_p, c_int, c_void_p, ctypes.c_uint32,
                                ctypes.c_double, c_void_p, c_void_p, c_void_p, c_void_p]),
    "phk_chain_create": (c_int, [c_void_p, c_void_p, c_u64, c_u64, c_void_p, c_u64, ctypes.c_uint32, c_u64, P(c_void_p)]),
    "phk_batch_chain_create": (c_int, [c_void_p, c_void_p, c_void_p, c_u64, ctypes.c_uint32, c_u64, P(c_void_p)]),
    "phk_chain_create_from_emissions": (c_int, [c_void_p, c_void_p, c_u64, c_void_p, c_u64, ctypes.c_uint32, P(c_void_p)]),
    "phk_chain_set": (c_int, [c_void_p, c_void_p, c_void_p, c_u64, c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_double]),
    "phk_chain_emissions": (c_int, [c_void_p, c_void_p, c_void_p]),
    "phk_chain_expect": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "phk_chain_decode": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "phk_chain_grid_pass": (c_u64, []),
    "phk_chain_destroy": (c_int, [c_void_p, c_void_p]),
    "phk_chain_set_scan": (c_int, [c_void_p, c_void_p, c_u64]),
    "phk_chain_tile": (c_u64, []),
    "phk_chain_scan_grid_pass": (c_u64, []),
    "phk_chain_set_groups": (c_int, [c_void_p, c_void_p, c_void_p, c_u64]),
    "phk_chain_set_grouped": (c_int, [c_void_p, c_void_p, c_void_p, c_u64, c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_double,
                                      c_void_p]),
    "phk_chain_expect_grouped": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "phk_refine_boundaries_ascii": (c_int, [c_void_p, c_void_p, c_void_p, c_u64, c_int, c_char_p, c_void_p, c_u64, c_u64, c_void_p,
                                            c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_u64, c_void_p, c_void_p, c_void_p]),
    "phk_refine_boundaries_fasta": (c_int, [c_void_p, c_void_p, c_int, c_char_p, c_void_p, c_u64, c_u64, c_void_p, c_void_p, c_void_p,
                                            c_void_p, c_void_p, c_void_p, c_u64, c_void_p, c_void_p, c_void_p]),
    "phk_refine_grid_pass": (c_u64, []),
    "phk_refine_confidence_ascii": (c_int, [c_void_p, c_void_p, c_void_p, c_u64, c_int, c_char_p, c_void_p, c_u64, c_u64, c_void_p,
                                            c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_u64, ctypes.c_int64, c_void_p, c_void_p,
                                            c_void_p, c_void_p, c_void_p]),
    "phk_refine_confidence_fasta": (c_int, [c_void_p, c_void_p, c_int, c_char_p, c_void_p, c_u64, c_u64, c_void_p, c_void_p, c_void_p,
                                            c_void_p, c_void_p, c_void_p, c_u64, ctypes.c_int64, c_void_p, c_void_p, c_void_p, c_void_p,
                                            c_void_p]),
    "phk_neighbors": (c_int, [c_void_p, c_void_p, c_u64, c_void_p, c_u64, c_u64, c_int, c_u64, c_void_p, c_void_p]),
    "phk_model_neighbors": (c_int, [c_void_p, c_void_p, c_void_p, c_u64, c_int, c_void_p, c_void_p]),
    "phk_batch_neighbors": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    "phk_neighbors_stats": (c_int, [c_void_p, c_void_p]),
    "phk_neighbors_keep_details": (c_int, [c_void_p, c_int]),
    "phk_neighbors_details": (c_int, [c_void_p, c_u64, c_int, c_void_p, c_void_p, c_void_p]),
    "phk_model_fit_svm": (c_int, [c_void_p, c_void_p, c_double, c_double, c_double]),
    "phk_nusvc_fit": (c_int, [c_void_p, c_void_p, c_u64, c_u64, c_void_p, c_double, c_double, c_double, ctypes.c_int32,
                              c_void_p, c_void_p, P(c_double), P(ctypes.c_int32), P(ctypes.c_int32)]),
    "phk_nusvc_decision": (c_int, [c_void_p, c_void_p, c_u64, c_u64, c_void_p, c_double, c_double, c_void_p, c_u64,
                                   c_void_p]),
    "phk_nusvc_sweep": (c_int, [c_void_p, c_void_p, c_u64, c_u64, c_void_p, c_void_p, c_u32, c_void_p, c_u32, c_void_p, c_u32,
                                c_double, ctypes.c_int32, ctypes.c_int64, c_u32, c_u32, c_void_p, c_void_p, c_void_p, c_void_p,
                                c_void_p, c_void_p]),
    "phk_nusvc_sweep_lds_rows": (c_u32, []),
    "phk_score": (c_int, [c_void_p, c_void_p, c_void_p, c_u64, c_int, c_void_p]),
    "phk_distances": (c_int, [c_void_p, c_void_p, c_u64, c_void_p, c_u64, c_u64, c_void_p]),
    "phk_silhouettes": (c_int, [c_void_p, c_void_p, c_u64, c_u64, c_void_p, c_u32, c_void_p]),
    "phk_dbscan": (c_int, [c_void_p, c_void_p, c_u64, c_u64, c_double, c_u64, c_void_p, c_void_p, P(c_u64)]),
    "phk_dbscan_sweep_create": (c_int, [c_void_p, c_void_p, c_u64, c_u64, P(c_void_p)]),
    "phk_dbscan_sweep_destroy": (c_int, [c_void_p, c_void_p]),
    "phk_dbscan_sweep": (c_int, [c_void_p, c_void_p, c_u32, c_void_p, c_void_p, c_u64, c_void_p, c_void_p, c_void_p, c_void_p]),
    "phk_placement_create": (c_int, [c_void_p, c_void_p, c_u64, c_u64, P(c_void_p)]),
    "phk_placement_destroy": (c_int, [c_void_p, c_void_p]),
    "phk_placement_run": (c_int, [c_void_p, c_void_p, c_void_p, c_u64, c_u32, c_u32, c_void_p, c_double, c_int, c_u32, c_void_p,
                                  c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "phk_sweep_create": (c_int, [c_void_p, c_void_p, c_u64, c_u64, P(c_void_p)]),
    "phk_sweep_destroy": (c_int, [c_void_p, c_void_p]),
    "phk_sweep_run": (c_int, [c_void_p, c_void_p, c_u64, c_void_p, c_void_p, c_void_p, c_void_p, c_double, c_int, c_u32,
                              ctypes.c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "phk_combo_grid_create": (c_int, [c_void_p, c_void_p, c_u64, c_u64, c_void_p, c_void_p, c_u32, P(c_void_p)]),
    "phk_combo_grid_destroy": (c_int, [c_void_p, c_void_p]),
    "phk_combo_grid_fit": (c_int, [c_void_p, c_void_p, c_u64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                   c_int, c_u32, c_u64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "phk_combo_grid_get_centroids": (c_int, [c_void_p, c_void_p, c_u64, c_u64, c_void_p]),
    "phk_combo_grid_put_centroids": (c_int, [c_void_p, c_void_p, c_u64, c_u64, c_void_p]),
    "phk_combo_grid_score": (c_int, [c_void_p, c_void_p, c_u32, c_void_p, c_u32, c_void_p, c_u64, c_void_p, c_void_p]),
    "phk_pca_covariance": (c_int, [c_void_p, c_void_p, c_u64, c_u64, c_void_p, c_void_p]),
    "phk_pca_project": (c_int, [c_void_p, c_void_p, c_u64, c_u64, c_void_p, c_void_p, c_u64, c_void_p]),
    "phk_tsne_neighbors": (c_int, [c_void_p, c_void_p, c_u64, c_u64, c_u64, c_void_p, c_void_p]),
    "phk_tsne_affinities": (c_int, [c_void_p, c_void_p, c_u64, c_u64, c_double, c_void_p, c_void_p]),
    "phk_tsne_symmetrize": (c_int, [c_void_p, c_void_p, c_u64, c_u64, c_void_p, c_void_p, c_void_p, P(c_u64)]),
    "phk_tsne_gradient": (c_int, [c_void_p, c_void_p, c_u64, c_void_p, c_void_p, c_void_p, c_double, P(c_double), c_void_p]),
    "phk_tsne_descend": (c_int, [c_void_p, c_void_p, c_u64, c_void_p, c_void_p, c_void_p, c_double, c_double, c_double, c_double,
                                 c_u64, P(c_double)]),
    "phk_tsne_fit": (c_int, [c_void_p, c_void_p, c_u64, c_void_p, c_void_p, c_void_p, c_double, c_double, c_u64, c_u64, c_double,
                             P(c_double), P(c_u64)]),
    "phk_argsort_f64": (c_int, [c_void_p, c_void_p, c_u64, c_int, c_void_p]),
    "phk_argsort_f64_dev": (c_int, [c_void_p, c_void_p, c_u64, c_int, c_void_p]),
    "phk_roc_curve": (c_int, [c_void_p, c_void_p, c_void_p, c_u64, c_int, c_void_p, c_void_p, c_void_p, P(c_u64), P(c_u64)]),
    "phk_roc_curve_dev": (c_int, [c_void_p, c_void_p, c_void_p, c_u64, c_int, c_void_p, c_void_p, c_void_p, P(c_u64), P(c_u64)]),
    "phk_truth_counts": (c_int, [c_void_p, c_void_p, c_void_p, c_u64, c_double, c_void_p]),
    "phk_compare_create": (c_int, [c_void_p, c_void_p, c_u64, c_u64, c_u64, P(c_void_p)]),
    "phk_compare_destroy": (c_int, [c_void_p, c_void_p]),
    "phk_compare_placements": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p]),
    "phk_compare_grams": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "phk_compare_bootstrap": (c_int, [c_void_p, c_void_p, c_u64, c_u64, c_u64, c_u64, c_void_p]),
    "phk_pack_ascii_dev": (c_int, [c_void_p, c_void_p, c_u64, c_char_p, c_void_p, c_void_p, c_void_p]),
    "phk_count_dev": (c_int, [c_void_p, c_void_p, c_void_p, c_u64, c_void_p, c_u64, c_int,
                              c_void_p, c_void_p]),
    "phk_normalize_dev": (c_int, [c_void_p, c_void_p, c_u64, c_u64, c_void_p]),
    "phk_score_dev": (c_int, [c_void_p, c_void_p, c_void_p, c_u64, c_int, c_void_p, c_void_p]),
    "phk_score_counts_dev": (c_int, [c_void_p, c_void_p, c_void_p, c_u64, c_int, c_void_p, c_void_p]),
    "phk_count_score_dev": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_u64, c_void_p, c_u64,
                                    c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "phk_check_counts_dev": (c_int, [c_void_p, c_void_p, c_void_p, c_u64, c_u64, c_u64, c_void_p]),
    "phk_score_stats": (c_int, [c_void_p, P(c_u64), P(c_u64)]),
    "phk_score_stats_ex": (c_int, [c_void_p, c_void_p, c_int]),
    "phk_mfma_f16_probe": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_u64, c_u32, c_void_p]),
    "phk_synth_packed_dev": (c_int, [c_void_p, c_u64, c_u64, c_u64, c_u64, c_u32, c_void_p,
                                     c_void_p, c_void_p]),
    "phk_synth_ragged_dev": (c_int, [c_void_p, c_u64, c_u64, c_u64, c_void_p, c_u64, c_u32, c_u32, c_void_p, c_void_p]),
    "phk_profile_enable": (c_int, [c_void_p, c_int]),
    "phk_profile_reset": (c_int, [c_void_p]),
    "phk_profile_count": (c_int, [c_void_p, P(c_int)]),
    "phk_profile_get": (c_int, [c_void_p, c_int, c_char_p, c_int, P(c_double), P(c_u64)]),
}

_lib = None
_lock = threading.Lock()
_contexts = {}


class PhkError(RuntimeError):
    def __init__(self, code, message):
        RuntimeError.__init__(self, "libphamers_hip: %s (code %d)" % (message, code))
        self.code = code


def load():
    """dlopen the in-tree library and declare every signature; raises if it is absent."""
    global _lib
    if _lib is None:
        with _lock:
            if _lib is None:
                path = LIB_PATH
                # A/B timing runs on one box (tools/diag): another build of the library -- an earlier round's, a candidate's --
                # in place of the in-tree one.  Only together with PHK_ALLOW_DIAGNOSTIC_BUILD=1, never for results; entry points
                # such a build lacks stay unbound.
                other = os.environ.get("PHAMERS_AB_LIB") if os.environ.get("PHK_ALLOW_DIAGNOSTIC_BUILD") == "1" else None
                if other:
                    path = other
                if not os.path.exists(path):
                    raise ImportError(
                        "%s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                        "(or `make -C phamers_amd/csrc`). There is no CPU fallback." % path)
                lib = ctypes.CDLL(path)
                for name, (res, args) in SIGNATURES.items():
                    if other and not hasattr(lib, name):
                        continue
                    fn = getattr(lib, name)
                    fn.restype = res
                    fn.argtypes = args
                ver = lib.phk_abi_version()
                if other:
                    ver = ABI_VERSION
                if ver != ABI_VERSION and not (ver == (ABI_VERSION | 0x40000000)
                                               and os.environ.get("PHK_ALLOW_DIAGNOSTIC_BUILD") == "1"):
                    raise ImportError(
                        "%s reports ABI version %#x, this binding is for %d%s" % (
                            LIB_PATH, ver, ABI_VERSION,
                            " (a -DPHK_DIAGNOSTIC_BUILD library: timing only, never for results; tools/diag scripts "
                            "load it with PHK_ALLOW_DIAGNOSTIC_BUILD=1)" if ver & 0x40000000 else ""))
                _lib = lib
    return _lib


def check(rc):
    if rc != PHK_OK:
        raise PhkError(rc, load().phk_last_error().decode("utf-8", "replace"))


def last_error():
    """The message of the last failed call without its "phk_...: " prefix."""
    msg = load().phk_last_error().decode("utf-8", "replace")
    return msg.split(": ", 1)[1] if msg.startswith("phk_") and ": " in msg else msg


def check_value(rc, nan=True, arg=True):
    """``check`` for calls whose refusals are the caller's ValueError: PHK_ERR_NAN (``nan``) as scikit-learn words it for the
    reference, PHK_ERR_ARG (``arg``) with the library's message."""
    if nan and rc == PHK_ERR_NAN:
        raise ValueError("Input contains NaN.")
    if arg and rc == PHK_ERR_ARG:
        raise ValueError(last_error())
    check(rc)


def kmeans_trials(k):
    """Seeding trials per centre of a k-means problem (kb_trials, csrc/kmeans_batch.h)."""
    return 2 + int(np.log(k))


def _pack_draws(ks, draws):
    """The problems' draws one after the other, as the batched k-means entry points take them: (flat float64, offsets
    uint64).  ``draws[s]`` holds the (ks[s] - 1) * kmeans_trials(ks[s]) uniforms of problem s; an empty result is one zero."""
    flat, offs, at = [], np.zeros(len(ks), dtype=np.uint64), 0
    for s, k in enumerate(int(k) for k in ks):
        d = np.ascontiguousarray(draws[s], dtype=np.float64)
        if k >= 1 and d.size != (k - 1) * kmeans_trials(k):
            raise ValueError("draws of problem %d must be (%d, %d)" % (s, k - 1, kmeans_trials(k)))
        offs[s] = at
        at += d.size
        flat.append(d.ravel())
    flat = np.ascontiguousarray(np.concatenate(flat) if flat else np.zeros(0), dtype=np.float64)
    return (flat if flat.size else np.zeros(1, dtype=np.float64)), offs


class _Resident(object):
    """A handle the library keeps for a context (``self.ctx``, ``self.handle``); ``_destroy`` names the entry point
    ``(ctx handle, handle)`` that releases it.  Closing twice, or after the context, does nothing."""
    _destroy = None

    def _open(self):
        if not getattr(self, "handle", None):
            raise ValueError("this %s is closed" % type(self).__name__)

    def close(self):
        ctx = getattr(self, "ctx", None)
        if getattr(self, "handle", None) and getattr(ctx, "handle", None):
            getattr(ctx.lib, self._destroy)(ctx.handle, self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def default_device():
    for var in ("PHAMERS_HIP_DEVICE", "LOCAL_RANK"):
        v = os.environ.get(var)
        if v not in (None, ""):
            return int(v)
    return 0


def ptr(a):
    """void* of a C-contiguous NumPy array (or None)."""
    if a is None:
        return None
    assert a.flags["C_CONTIGUOUS"]
    return ctypes.c_void_p(a.ctypes.data)


class Context(object):
    """One per (process, GPU).  ``stream`` may be a raw hipStream_t integer
    (e.g. ``torch.cuda.current_stream().cuda_stream``)."""

    def __init__(self, device=None, stream=None):
        self.lib = load()
        self.device = default_device() if device is None else int(device)
        h = ctypes.c_void_p()
        check(self.lib.phk_create(self.device, ctypes.c_void_p(stream) if stream else None, ctypes.byref(h)))
        self.handle = h

    def close(self):
        if getattr(self, "handle", None):
            self.lib.phk_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync(self):
        check(self.lib.phk_sync(self.handle))

    def set_option(self, key, value):
        """Tuning / diagnostic knob (phk_set_option); knobs start from PHK_<KEY> in the environment at creation."""
        check(self.lib.phk_set_option(self.handle, key.encode(), str(value).encode()))

    def options(self, **kw):
        """Context manager: set knobs for a block, restore the given ``(value, restore)`` pairs afterwards:
        ``with ctx.options(force_exact=("1", "0")): ...``"""
        ctx = self

        class _Scope(object):
            def __enter__(self_):
                for k, (v, _) in kw.items():
                    ctx.set_option(k, v)

            def __exit__(self_, *exc):
                for k, (_, r) in kw.items():
                    ctx.set_option(k, r)
        return _Scope()

    def score_stats(self):
        """(queries sent to the float64 fallback, orderings decided by exact candidate distances)
        of the most recent scoring call."""
        a, b = ctypes.c_uint64(), ctypes.c_uint64()
        check(self.lib.phk_score_stats(self.handle, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    def score_stats_ex(self):
        """Diagnostics of the most recent scoring call (phk_score_stats_ex) as a dict."""
        out = np.zeros(9, dtype=np.uint64)
        check(self.lib.phk_score_stats_ex(self.handle, ptr(out), 9))
        names = ("brute_forced", "exact_distance_decisions", "second_chance", "window_wider_than_refined",
                 "window_past_lists", "refined_values_too_close", "centroid_leader_uncertified",
                 "reswept_three_digits", "swept_f16_beyond_int8")
        return {k: int(v) for k, v in zip(names, out)}

    def neighbors_stats(self):
        """(queries answered, queries that took the exact fallback) of the neighbour lookups since the last call."""
        out = np.zeros(2, dtype=np.uint64)
        check(self.lib.phk_neighbors_stats(self.handle, ptr(out)))
        return int(out[0]), int(out[1])

    # ---- timing ----
    def profile_enable(self, on=True):
        check(self.lib.phk_profile_enable(self.handle, 1 if on else 0))

    def profile_reset(self):
        check(self.lib.phk_profile_reset(self.handle))

    def profile(self):
        """{kernel name: (total_ms, launches)} since the last reset."""
        n = ctypes.c_int()
        check(self.lib.phk_profile_count(self.handle, ctypes.byref(n)))
        out = {}
        for i in range(n.value):
            name = ctypes.create_string_buffer(128)
            ms, cnt = ctypes.c_double(), ctypes.c_uint64()
            check(self.lib.phk_profile_get(self.handle, i, name, 128, ctypes.byref(ms), ctypes.byref(cnt)))
            out[name.value.decode()] = (ms.value, cnt.value)
        return out


class Model(_Resident):
    """Device-resident training side of phamer_scorer.score_points."""
    _destroy = "phk_model_destroy"

    def __init__(self, ctx, positive, negative, positive_centroids=None, negative_centroids=None,
                 k_neighbors=3):
        self.ctx = ctx
        pos = np.ascontiguousarray(positive, dtype=np.float64)
        neg = np.ascontiguousarray(negative, dtype=np.float64)
        if pos.ndim != 2 or neg.ndim != 2 or pos.shape[1] != neg.shape[1]:
            raise ValueError("positive / negative data must be 2-D with the same number of columns")
        cp = cn = None
        if positive_centroids is not None:
            cp = np.ascontiguousarray(positive_centroids, dtype=np.float64)
            cn = np.ascontiguousarray(negative_centroids, dtype=np.float64)
        # a zero-count reference row is NaN after normalisation; the reference's scikit-learn fit raises on it
        # (scripts/learning.py:127, 138), so no model is ever built from such data
        for a in (pos, neg, cp, cn):
            if a is not None and np.isnan(a).any():
                raise ValueError("Input contains NaN.")
        self.D = pos.shape[1]
        self._pos, self._neg, self._mask = pos, neg, None     # (the svm method's gamma='scale' reads the unmasked rows)
        h = ctypes.c_void_p()
        check(ctx.lib.phk_model_create(ctx.handle, ptr(pos), pos.shape[0], ptr(neg), neg.shape[0],
                                       ptr(cp), 0 if cp is None else cp.shape[0],
                                       ptr(cn), 0 if cn is None else cn.shape[0],
                                       self.D, int(k_neighbors), ctypes.byref(h)))
        self.handle = h

    def set_centroids(self, positive_centroids, negative_centroids):
        """Replace the centroid segments (same counts as at creation): a cross-validation fold's k-means result."""
        cp = np.ascontiguousarray(positive_centroids, dtype=np.float64)
        cn = np.ascontiguousarray(negative_centroids, dtype=np.float64)
        if np.isnan(cp).any() or np.isnan(cn).any():
            raise ValueError("Input contains NaN.")
        check(self.ctx.lib.phk_model_set_centroids(self.ctx.handle, self.handle, ptr(cp), cp.shape[0], ptr(cn), cn.shape[0]))

    def set_column_mask(self, mask):
        """Exclude train rows from the k-NN search (``mask``: bool over vstack(positive, negative); None lifts it)."""
        m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
        check(self.ctx.lib.phk_model_set_column_mask(self.ctx.handle, self.handle, ptr(m)))
        self._mask = None if m is None else m.astype(bool)

    def fit_svm(self, nu=0.5, gamma='scale', tol=1e-3):
        """Fits the svm method (phamer_scorer.svm_score_points: NuSVC().fit(train, labels), scripts/phamer.py:258-266) on
        the train rows the column mask leaves in; 'scale' / 'auto' are scikit-learn's, over those rows in vstack order.
        Returns gamma.  ValueError for an infeasible nu or a class without rows, as scikit-learn raises."""
        X = np.vstack((self._pos, self._neg))
        if self._mask is not None:
            X = X[~self._mask]
        g = svm_gamma(X, gamma)
        rc = self.ctx.lib.phk_model_fit_svm(self.ctx.handle, self.handle, float(nu), g, float(tol))
        check_value(rc, nan=False)
        return g

    def set_bandwidths(self, h_pos, h_neg):
        """Gaussian kernel widths of the density method per class (phamer_scorer.positive_bandwidth / negative_bandwidth;
        a model starts with the reference's 0.005 / 0.01).  ValueError unless both are finite and > 0."""
        h_pos, h_neg = float(h_pos), float(h_neg)
        if not (np.isfinite(h_pos) and np.isfinite(h_neg) and h_pos > 0 and h_neg > 0):
            raise ValueError("bandwidths must be finite and > 0, got %r, %r" % (h_pos, h_neg))
        check(self.ctx.lib.phk_model_set_bandwidths(self.ctx.handle, self.handle, h_pos, h_neg))

    def score(self, Q, method="combo"):
        Q = np.ascontiguousarray(Q, dtype=np.float64)
        if Q.ndim != 2 or Q.shape[1] != self.D:
            raise ValueError("query rows must be (N, %d)" % self.D)
        out = np.empty(Q.shape[0], dtype=np.float64)
        check(self.ctx.lib.phk_score(self.ctx.handle, self.handle, ptr(Q), Q.shape[0], METHODS[method], ptr(out)))
        return out

    def neighbors(self, rows, k):
        """(distances (N, k) float64, indices (N, k) int64 into vstack(positive, negative)) of the k nearest train rows the
        column mask leaves in, by (distance, index) (phk_model_neighbors)."""
        Q = np.ascontiguousarray(rows, dtype=np.float64)
        if Q.ndim != 2 or Q.shape[1] != self.D:
            raise ValueError("query rows must be (N, %d)" % self.D)
        idx, dist = _neighbor_outputs(Q.shape[0], k)
        return _neighbor_result(self.ctx.lib.phk_model_neighbors(self.ctx.handle, self.handle, ptr(Q), Q.shape[0], int(k),
                                                                 ptr(idx), ptr(dist)), idx, dist)


PLACEMENT_DUPLICATE, PLACEMENT_EMPTY = 1, 2
SWEEP_EMPTY = 2


class Placement(_Resident):
    """Device-resident reference rows of the batched per-contig placement (phk_placement): ``run`` solves, for every row
    of ``Z``, k-means of the reference rows with that row appended and the silhouettes of the row's cluster."""
    _destroy = "phk_placement_destroy"

    def __init__(self, ctx, reference):
        self.ctx = ctx
        X = np.ascontiguousarray(reference, dtype=np.float64)
        if X.ndim != 2 or X.shape[0] < 1 or X.shape[1] < 1:
            raise ValueError("reference rows must be a non-empty 2-D array")
        self.n, self.D = X.shape
        h = ctypes.c_void_p()
        check_value(ctx.lib.phk_placement_create(ctx.handle, ptr(X), self.n, self.D, ctypes.byref(h)), arg=False)
        self.handle = h

    def run(self, Z, k, first_seed, draws, tol=1e-4, max_iter=300, chunk=0):
        """dict of per-problem arrays: labels (B, n + 1) uint32, seeds (B, k), sil (B, n + 1) of which the first
        n_members[b] count, n_members, status (PLACEMENT_* bits), n_iter, min_gap, seed_margin."""
        self._open()
        Z = np.ascontiguousarray(Z, dtype=np.float64)
        if Z.ndim != 2 or Z.shape[1] != self.D:
            raise ValueError("contig rows must be (B, %d)" % self.D)
        B, n1, k = Z.shape[0], self.n + 1, int(k)
        draws = np.ascontiguousarray(draws, dtype=np.float64)
        if k >= 1 and draws.shape != (k - 1, kmeans_trials(k)):   # (k < 1 is the library's to refuse, as in Sweep.run)
            raise ValueError("draws must be (%d, %d)" % (k - 1, kmeans_trials(k)))
        out = {"labels": np.empty((B, n1), dtype=np.uint32), "seeds": np.empty((B, k), dtype=np.uint32),
               "sil": np.empty((B, n1), dtype=np.float64), "n_members": np.empty(B, dtype=np.uint32),
               "status": np.empty(B, dtype=np.uint32), "n_iter": np.empty(B, dtype=np.int32),
               "min_gap": np.empty(B, dtype=np.float64), "seed_margin": np.empty(B, dtype=np.float64)}
        rc = self.ctx.lib.phk_placement_run(self.ctx.handle, self.handle, ptr(Z), B, k, int(first_seed), ptr(draws), float(tol),
                                            int(max_iter), int(chunk), ptr(out["labels"]), ptr(out["seeds"]), ptr(out["sil"]),
                                            ptr(out["n_members"]), ptr(out["status"]), ptr(out["n_iter"]), ptr(out["min_gap"]),
                                            ptr(out["seed_margin"]))
        check_value(rc)
        return out


class Sweep(_Resident):
    """Device-resident rows of the k-means sweep (phk_sweep): ``run`` solves one k-means problem per entry of ``ks`` on the
    same rows, each with its own first centre and draws, and (optionally) the silhouettes of every row of every problem."""
    _destroy = "phk_sweep_destroy"

    def __init__(self, ctx, data):
        self.ctx = ctx
        X = np.ascontiguousarray(data, dtype=np.float64)
        if X.ndim != 2 or X.shape[0] < 1 or X.shape[1] < 1:
            raise ValueError("the rows must be a non-empty 2-D array")
        self.n, self.D = X.shape
        h = ctypes.c_void_p()
        check_value(ctx.lib.phk_sweep_create(ctx.handle, ptr(X), self.n, self.D, ctypes.byref(h)), arg=False)
        self.handle = h

    def run(self, ks, first_seeds, draws, silhouettes=True, tol=1e-4, max_iter=300, chunk=0, pair_budget=-1):
        """``draws[s]`` = the (ks[s] - 1, 2 + int(ln ks[s])) uniforms of problem s.  dict of per-problem results: labels
        (S, n) uint32, seeds (list of S arrays), sil (S, n) or None, status (SWEEP_EMPTY bit), n_iter, min_gap,
        seed_margin.  ``pair_budget``: bytes the stored pair distances may take (-1: a quarter of the free memory)."""
        self._open()
        ks = np.ascontiguousarray(ks, dtype=np.uint32)
        S, n = len(ks), self.n
        first = np.ascontiguousarray(first_seeds, dtype=np.uint32)
        if first.shape != (S,) or len(draws) != S:
            raise ValueError("one first seed and one set of draws per problem")
        flat, offs = _pack_draws(ks, draws)
        seeds = np.empty(int(ks.sum()), dtype=np.uint32)
        out = {"labels": np.empty((S, n), dtype=np.uint32), "sil": np.empty((S, n), dtype=np.float64) if silhouettes else None,
               "status": np.empty(S, dtype=np.uint32), "n_iter": np.empty(S, dtype=np.int32),
               "min_gap": np.empty(S, dtype=np.float64), "seed_margin": np.empty(S, dtype=np.float64)}
        rc = self.ctx.lib.phk_sweep_run(self.ctx.handle, self.handle, S, ptr(ks), ptr(first), ptr(flat), ptr(offs), float(tol),
                                        int(max_iter), int(chunk), int(pair_budget), ptr(out["labels"]), ptr(seeds),
                                        ptr(out["sil"]) if silhouettes else None, ptr(out["status"]), ptr(out["n_iter"]),
                                        ptr(out["min_gap"]), ptr(out["seed_margin"]))
        check_value(rc)
        out["seeds"] = np.split(seeds, np.cumsum(ks.astype(np.int64))[:-1]) if S else []
        return out


COMBO_GRID_EMPTY = 2
COMBO_GRID_MAX_NEIGHBORS = 64   # a row's neighbour classes are one 64-bit word
COMBO_GRID_MAX_ROWS = 1 << 22


class ComboGrid(_Resident):
    """Device-resident state of the k_neighbors x k_clusters grid (phk_combo_grid): the rows of ``vstack(positive,
    negative)`` with their held-out fold and class, the row lists of the train sets and the centroid bank.  Train set
    ``slot * folds + fold`` (slot 0: positive, 1: negative) holds that class's rows outside the fold, in row order."""
    _destroy = "phk_combo_grid_destroy"

    def __init__(self, ctx, X, fold_of, is_positive, folds):
        self.ctx = ctx
        X = np.ascontiguousarray(X, dtype=np.float64)
        if X.ndim != 2 or X.shape[0] < 1 or X.shape[1] < 1:
            raise ValueError("the rows must be a non-empty 2-D array")
        self.M, self.D = X.shape
        self.folds = int(folds)
        fold_of = np.ascontiguousarray(fold_of, dtype=np.uint32)
        cls = np.ascontiguousarray(np.asarray(is_positive) != 0, dtype=np.uint8)
        if fold_of.shape != (self.M,) or cls.shape != (self.M,):
            raise ValueError("one fold and one class per row")
        h = ctypes.c_void_p()
        check_value(ctx.lib.phk_combo_grid_create(ctx.handle, ptr(X), self.M, self.D, ptr(fold_of), ptr(cls), self.folds,
                                                  ctypes.byref(h)))
        self.handle = h
        self.bank_rows = 0

    def _call(self, rc):
        check_value(rc, nan=False)

    def fit(self, sets, ks, first_seeds, draws, set_mean, set_tol, bank_rows, bank_off, max_iter=300, chunk=0):
        """One k-means problem per entry (``draws[s]``: the (ks[s] - 1, 2 + int(ln ks[s])) uniforms); the centroids go to
        rows ``bank_off[s]`` .. of a bank of ``bank_rows`` rows.  dict of per-problem status (COMBO_GRID_EMPTY bit), n_iter,
        min_gap, seed_margin."""
        self._open()
        sets = np.ascontiguousarray(sets, dtype=np.uint32)
        ks = np.ascontiguousarray(ks, dtype=np.uint32)
        first = np.ascontiguousarray(first_seeds, dtype=np.uint32)
        bank_off = np.ascontiguousarray(bank_off, dtype=np.uint64)
        S = len(ks)
        if sets.shape != (S,) or first.shape != (S,) or bank_off.shape != (S,) or len(draws) != S:
            raise ValueError("one train set, first seed, bank offset and set of draws per problem")
        set_mean = np.ascontiguousarray(set_mean, dtype=np.float64)
        set_tol = np.ascontiguousarray(set_tol, dtype=np.float64)
        if set_mean.shape != (2 * self.folds, self.D) or set_tol.shape != (2 * self.folds,):
            raise ValueError("set_mean must be (%d, %d) and set_tol (%d,)" % (2 * self.folds, self.D, 2 * self.folds))
        flat, offs = _pack_draws(ks, draws)
        out = {"status": np.zeros(S, dtype=np.uint32), "n_iter": np.zeros(S, dtype=np.int32),
               "min_gap": np.zeros(S, dtype=np.float64), "seed_margin": np.zeros(S, dtype=np.float64)}
        self._call(self.ctx.lib.phk_combo_grid_fit(self.ctx.handle, self.handle, S, ptr(sets), ptr(ks), ptr(first), ptr(flat), ptr(offs),
                                                   ptr(set_mean), ptr(set_tol), int(max_iter), int(chunk), int(bank_rows), ptr(bank_off),
                                                   ptr(out["status"]), ptr(out["n_iter"]), ptr(out["min_gap"]),
                                                   ptr(out["seed_margin"])))
        self.bank_rows = int(bank_rows)
        return out

    def get_centroids(self, row0, rows):
        self._open()
        out = np.empty((int(rows), self.D), dtype=np.float64)
        self._call(self.ctx.lib.phk_combo_grid_get_centroids(self.ctx.handle, self.handle, int(row0), int(rows), ptr(out)))
        return out

    def put_centroids(self, row0, centroids):
        self._open()
        C = np.ascontiguousarray(centroids, dtype=np.float64)
        if C.ndim != 2 or C.shape[1] != self.D:
            raise ValueError("centroids must be (rows, %d)" % self.D)
        self._call(self.ctx.lib.phk_combo_grid_put_centroids(self.ctx.handle, self.handle, int(row0), C.shape[0], ptr(C)))

    def score(self, k_neighbors, k_clusters, rows_per_pass=0):
        """(knn (Kn, M) of +-1.0, kmeans (Ku, M)) for the bank laid out as include/phamers_hip.h describes."""
        self._open()
        kn = np.ascontiguousarray(k_neighbors, dtype=np.uint32).ravel()
        ku = np.ascontiguousarray(k_clusters, dtype=np.uint32).ravel()
        knn = np.empty((len(kn), self.M), dtype=np.float64)
        km = np.empty((len(ku), self.M), dtype=np.float64)
        self._call(self.ctx.lib.phk_combo_grid_score(self.ctx.handle, self.handle, len(kn), ptr(kn) if len(kn) else None, len(ku),
                                                     ptr(ku) if len(ku) else None, int(rows_per_pass),
                                                     ptr(knn) if len(kn) else None, ptr(km) if len(ku) else None))
        return knn, km


NEIGHBORS_MAX_K = 28


def _neighbor_outputs(n, k):
    k = int(k)
    if not 1 <= k <= NEIGHBORS_MAX_K:
        raise ValueError("k = %d is not in 1..%d" % (k, NEIGHBORS_MAX_K))
    return np.empty((n, k), dtype=np.int32), np.empty((n, k), dtype=np.float64)


def _neighbor_result(rc, idx, dist):
    check_value(rc)   # (NaN rows: as scoring does)
    return dist, idx.astype(np.int64)


def check_neighbor_arguments(Q, X, k):
    """The ValueErrors of a neighbour lookup that need no device: shapes, 1 <= k <= min(28, rows)."""
    if Q.ndim != 2 or X.ndim != 2:
        raise ValueError("query rows and data must be 2-D, got %dD and %dD" % (Q.ndim, X.ndim))
    if Q.shape[1] != X.shape[1] or X.shape[1] == 0:
        raise ValueError("query rows have %d columns, data %d" % (Q.shape[1], X.shape[1]))
    k = int(k)
    if not 1 <= k <= NEIGHBORS_MAX_K:
        raise ValueError("k = %d is not in 1..%d" % (k, NEIGHBORS_MAX_K))
    if k > X.shape[0]:
        raise ValueError("Expected n_neighbors <= n_samples_fit, but n_neighbors = %d, n_samples_fit = %d" % (k, X.shape[0]))


def neighbors(ctx, Q, X, k, batch_rows=0, details=None):
    """The k nearest rows of X for every row of Q by (distance, index) on the device (phk_neighbors): (distances (N, k)
    float64, indices (N, k) int64).  ``details``: a dict that receives fell_back (count), queries, E (N,), approx_d2 (N, k)
    and fell_back_rows (N,) bool."""
    Q = np.ascontiguousarray(Q, dtype=np.float64)
    X = np.ascontiguousarray(X, dtype=np.float64)
    check_neighbor_arguments(Q, X, k)
    if np.isnan(X).any():
        raise ValueError("Input contains NaN.")
    idx, dist = _neighbor_outputs(Q.shape[0], k)
    if details is not None:
        ctx.neighbors_stats()
        check(ctx.lib.phk_neighbors_keep_details(ctx.handle, 1))
    try:
        out = _neighbor_result(ctx.lib.phk_neighbors(ctx.handle, ptr(Q), Q.shape[0], ptr(X), X.shape[0], X.shape[1], int(k),
                                                     int(batch_rows), ptr(idx), ptr(dist)), idx, dist)
        if details is not None:
            n = Q.shape[0]
            E, a, fb = np.empty(n), np.empty((n, int(k))), np.zeros(n, dtype=np.uint8)
            if n:
                check(ctx.lib.phk_neighbors_details(ctx.handle, n, int(k), ptr(E), ptr(a), ptr(fb)))
            queries, fell = ctx.neighbors_stats()
            details.update(fell_back=fell, queries=queries, E=E, approx_d2=a, fell_back_rows=fb.astype(bool))
    finally:
        if details is not None:
            ctx.lib.phk_neighbors_keep_details(ctx.handle, 0)
    return out


def kde_log_density(ctx, Q, X, h):
    """KernelDensity(kernel='gaussian', bandwidth=h).fit(X).score_samples(Q) on the device (phk_kde_log_density): (N,) float64.
    ValueError for NaN input or a bandwidth that is not finite and > 0, as scikit-learn raises."""
    Q = np.ascontiguousarray(Q, dtype=np.float64)
    X = np.ascontiguousarray(X, dtype=np.float64)
    if Q.ndim != 2 or X.ndim != 2 or Q.shape[1] != X.shape[1]:
        raise ValueError("query rows and data must be 2-D with the same number of columns")
    if X.shape[0] == 0:
        raise ValueError("Found array with 0 sample(s) (shape=%s) while a minimum of 1 is required." % (X.shape,))
    h = float(h)
    if not (np.isfinite(h) and h > 0):
        raise ValueError("bandwidth must be finite and > 0, got %r" % (h,))
    if np.isnan(Q).any() or np.isnan(X).any():
        raise ValueError("Input contains NaN.")
    out = np.empty(Q.shape[0], dtype=np.float64)
    check(ctx.lib.phk_kde_log_density(ctx.handle, ptr(Q), Q.shape[0], ptr(X), X.shape[0], X.shape[1], h, ptr(out)))
    return out


KDE_SWEEP_PER_PASS = 8   # PHK_KDE_SWEEP_PER_PASS: bandwidths one device pass of phk_kde_sweep carries


def check_kde_sweep_arguments(Q, X, bandwidths, exclude_self):
    """(Q, X, h) as float64 C-contiguous arrays, or the ValueError of learning.density_sweep -- no library needed."""
    Q = np.ascontiguousarray(Q, dtype=np.float64)
    X = np.ascontiguousarray(X, dtype=np.float64)
    if Q.ndim != 2 or X.ndim != 2 or Q.shape[1] != X.shape[1]:
        raise ValueError("query rows and data must be 2-D with the same number of columns")
    if X.shape[0] == 0:
        raise ValueError("Found array with 0 sample(s) (shape=%s) while a minimum of 1 is required." % (X.shape,))
    h = np.ascontiguousarray(np.asarray(bandwidths, dtype=np.float64).ravel())
    if h.size == 0:
        raise ValueError("no bandwidths given")
    if not (np.isfinite(h) & (h > 0)).all():
        raise ValueError("bandwidth must be finite and > 0, got %r" % (h.tolist(),))
    if exclude_self:
        if Q.shape != X.shape:
            raise ValueError("exclude_self needs the data rows as queries: shapes %s and %s" % (Q.shape, X.shape))
        if X.shape[0] == 1:
            raise ValueError("exclude_self leaves no row of a one-row data set")
    if np.isnan(Q).any() or np.isnan(X).any():
        raise ValueError("Input contains NaN.")
    return Q, X, h


def kde_sweep(ctx, Q, X, h, exclude_self=False, per_pass=None, batch_rows=0):
    """kde_log_density at every bandwidth of ``h`` from one upload and one pass over the pairs per KDE_SWEEP_PER_PASS
    bandwidths (phk_kde_sweep): (B, N) float64, row b bit for bit kde_log_density(ctx, Q, X, h[b]).  ``Q``, ``X``, ``h`` as
    check_kde_sweep_arguments returns them.  ``per_pass`` (tests): at most that many bandwidths per call of the library."""
    per = len(h) if per_pass is None else int(per_pass)   # (None: one call, the library runs its passes on resident rows)
    out = np.empty((len(h), Q.shape[0]), dtype=np.float64)
    for b0 in range(0, len(h), per):
        hs, part = np.ascontiguousarray(h[b0:b0 + per]), out[b0:b0 + per]
        check(ctx.lib.phk_kde_sweep(ctx.handle, ptr(Q), Q.shape[0], ptr(X), X.shape[0], X.shape[1], ptr(hs), len(hs),
                                    1 if exclude_self else 0, int(batch_rows), ptr(part)))
    return out


def silhouettes(ctx, X, labels, n_labels):
    """scikit-learn silhouette_samples(X, labels) on the device (phk_silhouettes): ``labels`` already encoded
    0..n_labels-1; (n,) float64."""
    X = np.ascontiguousarray(X, dtype=np.float64)
    lab = np.ascontiguousarray(labels, dtype=np.uint32)
    if X.ndim != 2 or lab.shape != (X.shape[0],):
        raise ValueError("X must be 2-D with one label per row")
    out = np.empty(X.shape[0], dtype=np.float64)
    check(ctx.lib.phk_silhouettes(ctx.handle, ptr(X), X.shape[0], X.shape[1], ptr(lab), int(n_labels), ptr(out)))
    return out


def dbscan(ctx, X, eps, min_samples):
    """DBSCAN(eps, min_samples).fit(X) on the device (phk_dbscan): (labels int64 (-1 = noise), core mask bool, n_clusters)."""
    X = np.ascontiguousarray(X, dtype=np.float64)
    if X.ndim != 2:
        raise ValueError("X must be 2-D")
    labels = np.empty(X.shape[0], dtype=np.int64)
    core = np.empty(X.shape[0], dtype=np.uint8)
    k = c_u64()
    check(ctx.lib.phk_dbscan(ctx.handle, ptr(X), X.shape[0], X.shape[1], float(eps), int(min_samples), ptr(labels), ptr(core),
                             ctypes.byref(k)))
    return labels, core.astype(bool), int(k.value)


class DbscanRows(_Resident):
    """Rows resident on the device for the DBSCAN parameter sweep (phk_dbscan_sweep_create); ``run`` solves up to 64 cells."""
    _destroy = "phk_dbscan_sweep_destroy"

    def __init__(self, ctx, X):
        X = np.ascontiguousarray(X, dtype=np.float64)
        if X.ndim != 2:
            raise ValueError("X must be 2-D")
        self.ctx, self.n = ctx, X.shape[0]
        h = ctypes.c_void_p()
        check(ctx.lib.phk_dbscan_sweep_create(ctx.handle, ptr(X), X.shape[0], X.shape[1], ctypes.byref(h)))
        self.handle = h

    def run(self, eps, min_samples, tiles_per_launch=0):
        """The cells (eps[c], min_samples[c]): {labels (C, n) int32, coremask (n,) uint64, n_clusters (C,), launches (3,)}."""
        eps = np.ascontiguousarray(eps, dtype=np.float64)
        ms = np.ascontiguousarray(min_samples, dtype=np.uint64)
        C = eps.shape[0]
        if eps.ndim != 1 or ms.shape != eps.shape:
            raise ValueError("one eps and one min_samples per cell")
        out = {"labels": np.empty((C, self.n), dtype=np.int32), "coremask": np.empty(self.n, dtype=np.uint64),
               "n_clusters": np.empty(C, dtype=np.uint64), "launches": np.zeros(3, dtype=np.uint32)}
        check(self.ctx.lib.phk_dbscan_sweep(self.ctx.handle, self.handle, C, ptr(eps), ptr(ms), int(tiles_per_launch),
                                            ptr(out["labels"]), ptr(out["coremask"]), ptr(out["n_clusters"]), ptr(out["launches"])))
        return out


COMPARE_MAX_CELLS = 256            # PHK_COMPARE_MAX_CELLS
COMPARE_BOOT_MAX_ROWS = 65535      # PHK_COMPARE_BOOT_MAX_ROWS: a resample's weights live in LDS


def _check_compare(rc):
    """``check`` for the phk_compare_* calls: a refusal of the input is the caller's ValueError."""
    if rc == PHK_ERR_NAN:
        raise ValueError("Input contains NaN or infinity.")
    if rc in (PHK_ERR_ARG, PHK_ERR_UNSUPPORTED):
        raise ValueError(last_error())
    check(rc)


class Compare(_Resident):
    """C score vectors over the same rows, sorted on the device (phk_compare_create): placements, Gram matrices and the
    stratified bootstrap of phamers_amd/compare.py.  ``scores`` is (C, n) float64, the first ``n_pos`` columns positive."""
    _destroy = "phk_compare_destroy"

    def __init__(self, ctx, scores, n_pos):
        scores = np.ascontiguousarray(scores, dtype=np.float64)
        if scores.ndim != 2:
            raise ValueError("scores must be 2-D")
        self.ctx, self.C, self.n, self.n_pos = ctx, scores.shape[0], scores.shape[1], int(n_pos)
        h = ctypes.c_void_p()
        _check_compare(ctx.lib.phk_compare_create(ctx.handle, ptr(scores), self.C, self.n, self.n_pos, ctypes.byref(h)))
        self.handle = h

    def placements(self):
        """(t_pos (C, P) uint32, t_neg (C, N) uint32)."""
        self._open()
        t_pos = np.empty((self.C, self.n_pos), dtype=np.uint32)
        t_neg = np.empty((self.C, self.n - self.n_pos), dtype=np.uint32)
        _check_compare(self.ctx.lib.phk_compare_placements(self.ctx.handle, self.handle, ptr(t_pos), ptr(t_neg)))
        return t_pos, t_neg

    def grams(self):
        """(area2 (C,), G10 (C, C), G01 (C, C)), uint64."""
        self._open()
        area2 = np.empty(self.C, dtype=np.uint64)
        g10, g01 = np.empty((self.C, self.C), dtype=np.uint64), np.empty((self.C, self.C), dtype=np.uint64)
        _check_compare(self.ctx.lib.phk_compare_grams(self.ctx.handle, self.handle, ptr(area2), ptr(g10), ptr(g01)))
        return area2, g10, g01

    def bootstrap(self, seed, count, first=0, per_launch=0):
        """area2_boot (count, C) uint64 of the resamples first .. first + count - 1."""
        self._open()
        out = np.empty((int(count), self.C), dtype=np.uint64)
        _check_compare(self.ctx.lib.phk_compare_bootstrap(self.ctx.handle, self.handle, int(seed) & (2 ** 64 - 1), int(first),
                                                          int(count), int(per_launch), ptr(out)))
        return out


def svm_gamma(X, gamma):
    """scikit-learn's _gamma (sklearn/svm/_base.py): 'scale' = 1 / (D * X.var()) (1.0 when the variance is 0), 'auto' =
    1 / D, else the number itself."""
    if isinstance(gamma, str):
        if gamma == 'scale':
            X_var = X.var()
            return 1.0 / (X.shape[1] * X_var) if X_var != 0 else 1.0
        if gamma == 'auto':
            return 1.0 / X.shape[1]
        raise ValueError("gamma must be 'scale', 'auto' or a float, got %r" % (gamma,))
    g = float(gamma)
    if not (np.isfinite(g) and g > 0):
        raise ValueError("gamma must be finite and > 0, got %r" % (gamma,))
    return g


def nusvc_fit(ctx, X, labels, nu, gamma, tol, max_iter=-1):
    """phk_nusvc_fit: (support, libsvm dual coefficients, libsvm rho, n_iter) for labels in {0, 1} and gamma > 0.
    ValueError (libsvm's message) for an infeasible nu, a single class or other bad arguments."""
    X = np.ascontiguousarray(X, dtype=np.float64)
    y = np.ascontiguousarray(labels, dtype=np.float64)
    n = X.shape[0]
    support = np.empty(n, dtype=np.int32)
    coef = np.empty(n, dtype=np.float64)
    rho, n_sv, n_iter = c_double(), ctypes.c_int32(), ctypes.c_int32()
    rc = ctx.lib.phk_nusvc_fit(ctx.handle, ptr(X), n, X.shape[1], ptr(y), float(nu), float(gamma), float(tol), int(max_iter),
                               ptr(support), ptr(coef), ctypes.byref(rho), ctypes.byref(n_sv), ctypes.byref(n_iter))
    check_value(rc, nan=False)
    k = n_sv.value
    return support[:k].copy(), coef[:k].copy(), rho.value, n_iter.value


def nusvc_decision(ctx, SV, coef, rho, gamma, Q):
    """phk_nusvc_decision: libsvm's decision values (N,) float64 of the rows Q."""
    SV = np.ascontiguousarray(SV, dtype=np.float64)
    coef = np.ascontiguousarray(coef, dtype=np.float64)
    Q = np.ascontiguousarray(Q, dtype=np.float64)
    out = np.empty(Q.shape[0], dtype=np.float64)
    check(ctx.lib.phk_nusvc_decision(ctx.handle, ptr(SV), SV.shape[0], SV.shape[1], ptr(coef), float(rho), float(gamma),
                                     ptr(Q), Q.shape[0], ptr(out)))
    return out


SVM_OK, SVM_INFEASIBLE, SVM_NOT_FINITE = 0, 1, 2   # PHK_SVM_*: a sweep problem's status


def nusvc_sweep_lds_rows():
    """Rows whose solver state fits the LDS of one workgroup of phk_nusvc_sweep (no device needed)."""
    return int(load().phk_nusvc_sweep_lds_rows())


def check_nusvc_sweep_arguments(X, labels, nus, gammas, fold_of, folds, tol, max_iter):
    """(X, labels, nus, gammas, fold_of) as C-contiguous arrays of the library's types, or the ValueError of
    svm.nusvc_sweep -- no library needed.  ``gammas`` are numbers here; ``fold_of`` is None with ``folds`` = 0."""
    X = np.ascontiguousarray(X, dtype=np.float64)
    y = np.ascontiguousarray(labels, dtype=np.float64)
    if X.ndim != 2 or y.ndim != 1 or len(y) != len(X) or X.shape[0] == 0 or X.shape[1] == 0:
        raise ValueError("X must be 2-D and y 1-D with one label per row")
    if not np.isin(y, (0.0, 1.0)).all():
        raise ValueError("labels must be 0 or 1")
    nus = np.ascontiguousarray(np.asarray(nus, dtype=np.float64).ravel())
    gammas = np.ascontiguousarray(np.asarray(gammas, dtype=np.float64).ravel())
    if nus.size == 0 or gammas.size == 0:
        raise ValueError("an empty axis of the grid: %d nu value(s), %d gamma value(s)" % (nus.size, gammas.size))
    if not ((nus > 0) & (nus <= 1)).all():
        raise ValueError("nu <= 0 or nu > 1")
    if not (np.isfinite(gammas) & (gammas > 0)).all():
        raise ValueError("gamma must be finite and > 0, got %r" % (gammas.tolist(),))
    if not (np.isfinite(tol) and tol > 0):
        raise ValueError("tol must be finite and > 0, got %r" % (tol,))
    if not (max_iter == -1 or max_iter > 0):
        raise ValueError("max_iter must be -1 or > 0, got %r" % (max_iter,))
    folds = int(folds)
    if folds:
        fold_of = np.ascontiguousarray(fold_of, dtype=np.int32)
        if fold_of.shape != y.shape or ((fold_of < 0) | (fold_of >= folds)).any():
            raise ValueError("one fold id in [0, %d) per row" % folds)
    else:
        fold_of = None
    if np.isnan(X).any():
        raise ValueError("Input contains NaN.")
    return X, y, nus, gammas, fold_of


def nusvc_sweep(ctx, X, labels, nus, gammas, fold_of=None, folds=0, tol=1e-3, max_iter=-1, lds_rows=-1, gammas_per_pass=0,
                threads=0):
    """phk_nusvc_sweep on arguments as check_nusvc_sweep_arguments returns them: {status, n_iter, n_sv (Gm, V, folds + 1)
    int32, rho (Gm, V, folds + 1), coef (Gm, V, folds + 1, n): libsvm's values, subset 0 = the full fit; held_dec (Gm, V, n)
    or None without folds}."""
    n, Gm, V, S = X.shape[0], len(gammas), len(nus), folds + 1
    out = {"status": np.empty((Gm, V, S), dtype=np.int32), "n_iter": np.empty((Gm, V, S), dtype=np.int32),
           "n_sv": np.empty((Gm, V, S), dtype=np.int32), "rho": np.empty((Gm, V, S), dtype=np.float64),
           "coef": np.empty((Gm, V, S, n), dtype=np.float64),
           "held_dec": np.empty((Gm, V, n), dtype=np.float64) if folds else None}
    rc = ctx.lib.phk_nusvc_sweep(ctx.handle, ptr(X), n, X.shape[1], ptr(labels), ptr(gammas), Gm, ptr(nus), V, ptr(fold_of),
                                 folds, float(tol), int(max_iter), int(lds_rows), int(gammas_per_pass), int(threads),
                                 ptr(out["status"]), ptr(out["n_iter"]), ptr(out["n_sv"]), ptr(out["rho"]), ptr(out["coef"]),
                                 ptr(out["held_dec"]))
    check_value(rc, nan=False)
    return out


def _groups(groups, n, what):
    """int32 C-contiguous group ids (n,), or None."""
    if groups is None:
        return None
    g = np.ascontiguousarray(groups, dtype=np.int32)
    if g.shape != (n,):
        raise ValueError("%s: one group id per row (%d), got shape %r" % (what, n, g.shape))
    return g


class LikelihoodTable(_Resident):
    """The resident log table of the multinomial likelihood scorer (phk_lik_table): ``log_pos`` (M+, D) and ``log_neg``
    (M-, D, or None for a one-class table) float64 rows of log p_r[j], with optional group ids per row."""
    _destroy = "phk_lik_table_destroy"

    def __init__(self, ctx, log_pos, log_neg=None, groups_pos=None, groups_neg=None):
        lp = np.ascontiguousarray(log_pos, dtype=np.float64)
        ln = None if log_neg is None else np.ascontiguousarray(log_neg, dtype=np.float64)
        if lp.ndim != 2 or (ln is not None and (ln.ndim != 2 or ln.shape[1] != lp.shape[1])):
            raise ValueError("the log tables must be 2-D with the same number of columns")
        self.ctx, self.D, self.n_pos, self.n_neg = ctx, lp.shape[1], lp.shape[0], 0 if ln is None else ln.shape[0]
        gp = _groups(groups_pos, self.n_pos, "groups_pos")
        gn = None if ln is None else _groups(groups_neg, self.n_neg, "groups_neg")
        h = ctypes.c_void_p()
        rc = ctx.lib.phk_lik_table_create(ctx.handle, ptr(lp), self.n_pos, ptr(gp), ptr(ln), self.n_neg, ptr(gn), self.D,
                                          ctypes.byref(h))
        if rc == PHK_ERR_NAN:
            raise ValueError(last_error())
        check_value(rc, nan=False)
        self.handle = h

    def _score(self, call, n, details):
        lp, ln, sc = (np.empty(n, dtype=np.float64) for _ in range(3))
        check_value(call(lp, ln, sc), nan=False)
        if details is not None:
            details["l_pos"], details["l_neg"] = lp, ln
        return sc

    def score(self, counts, query_groups=None, batch_rows=0, details=None):
        """Scores (N,) float64 of the uint32 count rows ``counts`` (N, D) on the host (phk_lik_score).  ValueError when a
        query's group leaves a class without rows."""
        self._open()
        c = np.ascontiguousarray(counts, dtype=np.uint32)
        if c.ndim != 2 or c.shape[1] != self.D:
            raise ValueError("the counts must be (N, %d), got shape %r" % (self.D, c.shape))
        g = _groups(query_groups, c.shape[0], "query_groups")
        return self._score(lambda lp, ln, sc: self.ctx.lib.phk_lik_score(
            self.ctx.handle, self.handle, ptr(c), c.shape[0], self.D, ptr(g), int(batch_rows), ptr(lp), ptr(ln), ptr(sc)),
            c.shape[0], details)


MIX_MAX_COMPONENTS = 256   # one row chunk of the Gram tile (mixture.hip)


class MixtureTable(_Resident):
    """The resident table of the mixture E-step (phk_mix_table): ``log_profiles`` (K, D) float64 and ``log_weights`` (K,),
    both made on the host; a log weight of -inf switches its component off.  ValueError for a value the library refuses."""
    _destroy = "phk_mix_table_destroy"

    def __init__(self, ctx, log_profiles, log_weights):
        lp, lw = self._arrays(log_profiles, log_weights)
        self.ctx, self.K, self.D = ctx, lp.shape[0], lp.shape[1]
        h = ctypes.c_void_p()
        self._rc(ctx.lib.phk_mix_table_create(ctx.handle, ptr(lp), ptr(lw), self.K, self.D, ctypes.byref(h)))
        self.handle = h

    @staticmethod
    def _arrays(log_profiles, log_weights):
        lp = np.ascontiguousarray(log_profiles, dtype=np.float64)
        lw = np.ascontiguousarray(log_weights, dtype=np.float64)
        if lp.ndim != 2 or lw.shape != (lp.shape[0],):
            raise ValueError("log_profiles must be (K, D) and log_weights (K,)")
        return lp, lw

    @staticmethod
    def _rc(rc):
        if rc == PHK_ERR_NAN:
            raise ValueError(last_error())
        check_value(rc, nan=False)

    def update(self, log_profiles, log_weights):
        """New values for a table of the same shape (phk_mix_table_update)."""
        self._open()
        lp, lw = self._arrays(log_profiles, log_weights)
        self._rc(self.ctx.lib.phk_mix_table_update(self.ctx.handle, self.handle, ptr(lp), ptr(lw), lp.shape[0], lp.shape[1]))

    def _expect(self, call, n, rows):
        T, Nk, L = np.zeros((self.K, self.D)), np.zeros(self.K), np.zeros(1)
        ll = np.zeros(n) if rows else None
        am = np.zeros(n, dtype=np.int32) if rows else None
        mr = np.zeros(n) if rows else None
        check_value(call(ptr(T), ptr(Nk), ptr(L), ptr(ll), ptr(am), ptr(mr)), nan=False)
        return (T, Nk, float(L[0])) + ((ll, am, mr) if rows else ())

    def _counts(self, counts):
        self._open()
        c = np.ascontiguousarray(counts, dtype=np.uint32)
        if c.ndim != 2 or c.shape[1] != self.D:
            raise ValueError("the counts must be (N, %d), got shape %r" % (self.D, c.shape))
        return c

    def expect(self, counts, batch_rows=0, rows=False):
        """One E-step over the uint32 count rows ``counts`` (N, D) on the host (phk_mix_expect): (T (K, D), Nk (K,), L), and
        with ``rows`` also (row_ll (N,), argmax (N,) int32, max_resp (N,))."""
        c = self._counts(counts)
        return self._expect(lambda *o: self.ctx.lib.phk_mix_expect(
            self.ctx.handle, self.handle, ptr(c), c.shape[0], self.D, int(batch_rows), *o), c.shape[0], rows)

    def responsibilities(self, counts, batch_rows=0):
        """(r (N, K), row_ll (N,)) of host count rows (phk_mix_responsibilities): the one call that brings N x K back."""
        c = self._counts(counts)
        r, ll = np.zeros((c.shape[0], self.K)), np.zeros(c.shape[0])
        check_value(self.ctx.lib.phk_mix_responsibilities(self.ctx.handle, self.handle, ptr(c), c.shape[0], self.D,
                                                          int(batch_rows), ptr(r), ptr(ll)), nan=False)
        return r, ll


class MixtureSweep(_Resident):
    """Count rows and row sets resident for many mixture E-steps per call (phk_mix_sweep).
    ``counts_or_batch``: uint32 count rows (N, D) on the host, or a ``Batch`` (kept alive here, read where it lies);
    ``row_sets``: strictly ascending row indices per set, none empty.  ValueError for what the library refuses."""
    _destroy = "phk_mix_sweep_destroy"

    def __init__(self, ctx, counts_or_batch, row_sets):
        sets = [np.ascontiguousarray(s, dtype=np.int64).ravel() for s in row_sets]
        if isinstance(counts_or_batch, Batch):
            counts_or_batch._open()
            self.source, c, self.N, self.D = counts_or_batch, None, counts_or_batch.n, counts_or_batch.D
        else:
            c = np.ascontiguousarray(counts_or_batch, dtype=np.uint32)
            if c.ndim != 2:
                raise ValueError("the counts must be (N, D), got shape %r" % (c.shape,))
            self.source, (self.N, self.D) = None, c.shape
        for i, s in enumerate(sets):
            if s.size and (s.min() < 0 or s.max() >= self.N):
                raise ValueError("row set %d holds an index outside 0 .. %d" % (i, self.N - 1))
        self.ctx, self.sizes = ctx, [int(s.size) for s in sets]
        offsets = np.zeros(len(sets) + 1, dtype=np.uint64)
        offsets[1:] = np.cumsum(self.sizes, dtype=np.uint64)
        flat = np.ascontiguousarray(np.concatenate(sets) if sets else np.zeros(0), dtype=np.uint32)
        flat = flat if flat.size else np.zeros(1, dtype=np.uint32)
        h = ctypes.c_void_p()
        if c is None:
            rc = ctx.lib.phk_batch_mix_sweep_create(ctx.handle, self.source.handle, ptr(flat), ptr(offsets), len(sets),
                                                    ctypes.byref(h))
        else:
            rc = ctx.lib.phk_mix_sweep_create(ctx.handle, ptr(c), self.N, self.D, ptr(flat), ptr(offsets), len(sets),
                                              ctypes.byref(h))
        MixtureTable._rc(rc)
        self.handle = h

    def step(self, jobs, rows=False, _budget_bytes=0, expect=True):
        """One device call over ``jobs``, a list of (row set, log_profiles (K, D), log_weights (K,)): per job the tuple
        (T (K, D), Nk (K,), L, l) -- l (n_set,) the rows' log-likelihoods with ``rows``, else None; ``expect=False``
        (evaluation: needs ``rows``) leaves T, Nk and L None.  Every job's values are the bits of ``MixtureTable.expect`` on
        that job's rows alone.  ``_budget_bytes`` (device bytes per group of jobs) is for the tests: no result depends on it."""
        self._open()
        if not (expect or rows):
            raise ValueError("step: expect=False needs rows=True")
        jobs = [(int(s),) + MixtureTable._arrays(lp, lw) for s, lp, lw in jobs]
        if not jobs:
            return []
        for j, (s, lp, lw) in enumerate(jobs):
            if not 0 <= s < len(self.sizes):
                raise ValueError("job %d names row set %d of %d" % (j, s, len(self.sizes)))
            if lp.shape[1] != self.D or not 1 <= lp.shape[0] <= MIX_MAX_COMPONENTS:
                raise ValueError("job %d: log_profiles must be (1 to %d, %d), got %r" % (j, MIX_MAX_COMPONENTS, self.D, lp.shape))
        sets = np.array([j[0] for j in jobs], dtype=np.uint32)
        Ks = np.array([j[1].shape[0] for j in jobs], dtype=np.uint32)
        logp = np.ascontiguousarray(np.concatenate([j[1].ravel() for j in jobs]))
        logw = np.ascontiguousarray(np.concatenate([j[2] for j in jobs]))
        E = [int(k) * self.D + int(k) + 1 for k in Ks] if expect else [0] * len(jobs)
        n = [self.sizes[s] for s in sets] if rows else [0] * len(jobs)
        out = np.zeros(sum(E) + sum(n))
        MixtureTable._rc(self.ctx.lib.phk_mix_sweep_step(self.ctx.handle, self.handle, ptr(sets), ptr(Ks), len(jobs), ptr(logp),
                                                        ptr(logw), int(bool(expect)), int(bool(rows)), int(_budget_bytes),
                                                        ptr(out)))
        got, at, row_at = [], 0, sum(E)
        for j, K in enumerate(int(k) for k in Ks):
            T = Nk = L = l = None
            if expect:
                T, Nk, L = out[at:at + K * self.D].reshape(K, self.D), out[at + K * self.D:at + E[j] - 1], float(out[at + E[j] - 1])
                at += E[j]
            if rows:
                l = out[row_at:row_at + n[j]]
                row_at += n[j]
            got.append((T, Nk, L, l))
        return got


HOSTS_MAX_TOP = 16   # PHK_HOSTS_MAX_TOP


def check_hosts_top(top, rows):
    """``top`` as an int, or the ValueError of a ranking of ``rows`` reference rows -- no library needed."""
    top = int(top)
    if not 1 <= top <= HOSTS_MAX_TOP:
        raise ValueError("top = %d is not in 1..%d" % (top, HOSTS_MAX_TOP))
    if top > rows:
        raise ValueError("top = %d exceeds the %d reference rows" % (top, rows))
    return top


class HostTable(_Resident):
    """The resident log table of the likelihood-ranked lookup (phk_host_table): ``log_table`` (M, D) float64 -- multinomial
    log profiles or Markov log transitions, see hosts.py -- with optional group ids per row."""
    _destroy = "phk_host_table_destroy"

    def __init__(self, ctx, log_table, groups=None):
        lt = np.ascontiguousarray(log_table, dtype=np.float64)
        if lt.ndim != 2 or lt.shape[0] == 0 or lt.shape[1] == 0:
            raise ValueError("the log table must be 2-D with at least one row, got shape %r" % (lt.shape,))
        self.ctx, self.M, self.D = ctx, lt.shape[0], lt.shape[1]
        g = _groups(groups, self.M, "groups")
        h = ctypes.c_void_p()
        rc = ctx.lib.phk_host_table_create(ctx.handle, ptr(lt), self.M, self.D, ptr(g), ctypes.byref(h))
        if rc == PHK_ERR_NAN:
            raise ValueError(last_error())
        check_value(rc, nan=False)
        self.handle = h

    def _rank(self, call, n, top):
        idx, s = np.empty((n, top), dtype=np.int32), np.empty((n, top), dtype=np.float64)
        check_value(call(idx, s), nan=False)
        return idx.astype(np.int64), s

    def rank(self, counts, top, query_groups=None, batch_rows=0):
        """(indices (N, top) int64, S (N, top) float64) of the uint32 count rows ``counts`` (N, D) on the host
        (phk_host_rank).  ValueError when ``top`` exceeds the rows a query's group leaves it."""
        self._open()
        top = check_hosts_top(top, self.M)
        c = np.ascontiguousarray(counts, dtype=np.uint32)
        if c.ndim != 2 or c.shape[1] != self.D:
            raise ValueError("the counts must be (N, %d), got shape %r" % (self.D, c.shape))
        g = _groups(query_groups, c.shape[0], "query_groups")
        return self._rank(lambda idx, s: self.ctx.lib.phk_host_rank(
            self.ctx.handle, self.handle, ptr(c), c.shape[0], self.D, ptr(g), top, int(batch_rows), ptr(idx), ptr(s)),
            c.shape[0], top)

    def null_fit(self, counts, batch_rows=0):
        """(mu (M,), sigma (M,)) of S / n over the uint32 null count rows ``counts`` (P, D) (phk_host_null_fit)."""
        self._open()
        c = np.ascontiguousarray(counts, dtype=np.uint32)
        if c.ndim != 2 or c.shape[1] != self.D:
            raise ValueError("the null counts must be (P, %d), got shape %r" % (self.D, c.shape))
        mu, sigma = np.empty(self.M, dtype=np.float64), np.empty(self.M, dtype=np.float64)
        check_value(self.ctx.lib.phk_host_null_fit(self.ctx.handle, self.handle, ptr(c), c.shape[0], self.D, int(batch_rows),
                                                   ptr(mu), ptr(sigma)), nan=False)
        return mu, sigma


SEG_TILE, SEG_QUANT_BITS = 64, 16   # PHK_SEG_TILE, PHK_SEG_QUANT_BITS


def segment_decode(ctx, x, offsets, trans, init, qlog_trans, qlog_init):
    """(posterior (n,) float64, state (n,) uint8, log_odds (R,) float64, path_score (R,) int64) of the two-state decode
    of the flat evidence ``x`` (n,) cut into records by ``offsets`` (R + 1,) (phk_segment_decode; segment.py prepares the
    arguments).  ValueError for the library's PHK_ERR_ARG and for an x that is not finite."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    off = np.ascontiguousarray(offsets, dtype=np.uint64)
    if x.ndim != 1 or off.ndim != 1 or off.shape[0] < 1:
        raise ValueError("segment_decode: x must be (n,) and offsets (R + 1,)")
    n, R = x.shape[0], off.shape[0] - 1
    tr, pi = np.ascontiguousarray(trans, dtype=np.float64).ravel(), np.ascontiguousarray(init, dtype=np.float64).ravel()
    qt, qp = np.ascontiguousarray(qlog_trans, dtype=np.int64).ravel(), np.ascontiguousarray(qlog_init, dtype=np.int64).ravel()
    if tr.shape != (4,) or pi.shape != (2,) or qt.shape != (4,) or qp.shape != (2,):
        raise ValueError("segment_decode: 4 transition and 2 initial parameters")
    posterior, state = np.empty(n, dtype=np.float64), np.empty(n, dtype=np.uint8)
    log_odds, path_score = np.empty(R, dtype=np.float64), np.empty(R, dtype=np.int64)
    rc = ctx.lib.phk_segment_decode(ctx.handle, ptr(x), n, ptr(off), R, ptr(tr), ptr(pi), ptr(qt), ptr(qp), ptr(posterior),
                                    ptr(state), ptr(log_odds), ptr(path_score))
    if rc == PHK_ERR_NAN:
        raise ValueError(last_error())
    check_value(rc, nan=False)
    return posterior, state, log_odds, path_score


SEG_TRACE_COLS, SEG_FIT_MAX_ITER = 10, 100000                        # PHK_SEG_TRACE_COLS, PHK_SEG_FIT_MAX_ITER
SEG_START_FIXED, SEG_START_FREE, SEG_START_STATIONARY = 0, 1, 2       # PHK_SEG_START_*
SEG_FIT_CONVERGED, SEG_FIT_CLAMPED, SEG_FIT_NO_TRANSITIONS = 1, 2, 4  # PHK_SEG_FIT_*


def _segment_records(who, x, offsets):
    x = np.ascontiguousarray(x, dtype=np.float64)
    off = np.ascontiguousarray(offsets, dtype=np.uint64)
    if x.ndim != 1 or off.ndim != 1 or off.shape[0] < 1:
        raise ValueError("%s: x must be (n,) and offsets (R + 1,)" % who)
    return x, off


def _segment_rc(rc):
    if rc == PHK_ERR_NAN:
        raise ValueError(last_error())
    check_value(rc, nan=False)


def segment_expect(ctx, x, offsets, trans, init):
    """(counts_rec (R, 6), totals (6,), log_odds (R,), log_evidence) of one E-step of the chain at ``trans`` (4,) and
    ``init`` (2,) over the flat evidence ``x`` (n,) cut into records by ``offsets`` (R + 1,) (phk_segment_expect).  A row of
    counts_rec: xi(0->0), xi(0->1), xi(1->0), xi(1->1), gamma_0(0), gamma_0(1).  ValueError as ``segment_decode``."""
    x, off = _segment_records("segment_expect", x, offsets)
    n, R = x.shape[0], off.shape[0] - 1
    tr, pi = np.ascontiguousarray(trans, dtype=np.float64).ravel(), np.ascontiguousarray(init, dtype=np.float64).ravel()
    if tr.shape != (4,) or pi.shape != (2,):
        raise ValueError("segment_expect: 4 transition and 2 initial parameters")
    counts, totals = np.empty((R, 6), dtype=np.float64), np.empty(6, dtype=np.float64)
    log_odds, evidence = np.empty(R, dtype=np.float64), ctypes.c_double()
    _segment_rc(ctx.lib.phk_segment_expect(ctx.handle, ptr(x), n, ptr(off), R, ptr(tr), ptr(pi), ptr(counts), ptr(totals),
                                           ptr(log_odds), ctypes.byref(evidence)))
    return counts, totals, log_odds, evidence.value


def segment_fit(ctx, x, offsets, start, start_mode, prior_counts, max_iter, tol):
    """(trace (n_iter + 1, 10), n_iter, status, fitted (3,)) of the Baum-Welch loop from ``start`` = (a, b, p_start)
    (phk_segment_fit): a trace row is a, b, p_start, the six totals and the log evidence at those parameters; ``status`` is
    the sum of the SEG_FIT_* bits.  ValueError as ``segment_decode``."""
    x, off = _segment_records("segment_fit", x, offsets)
    st, pc = np.ascontiguousarray(start, dtype=np.float64).ravel(), np.ascontiguousarray(prior_counts, dtype=np.float64).ravel()
    if st.shape != (3,) or pc.shape != (4,):
        raise ValueError("segment_fit: 3 start parameters and 4 prior counts")
    if not 0 <= int(max_iter) <= SEG_FIT_MAX_ITER:
        raise ValueError("segment_fit: max_iter must lie in [0, %d], got %r" % (SEG_FIT_MAX_ITER, max_iter))
    trace = np.zeros((int(max_iter) + 1, SEG_TRACE_COLS), dtype=np.float64)
    n_iter, status, fitted = ctypes.c_uint32(), ctypes.c_uint32(), np.empty(3, dtype=np.float64)
    _segment_rc(ctx.lib.phk_segment_fit(ctx.handle, ptr(x), x.shape[0], ptr(off), off.shape[0] - 1, ptr(st), int(start_mode),
                                        ptr(pc), int(max_iter), float(tol), ptr(trace), ctypes.byref(n_iter),
                                        ctypes.byref(status), ptr(fitted)))
    return trace[:n_iter.value + 1].copy(), int(n_iter.value), int(status.value), fitted


CHAIN_MAX_STATES = 8   # PHK_CHAIN_MAX_STATES


class Chain(_Resident):
    """An S-state chain over window rows (phk_chain): ``rows`` is an integer count matrix (n, D)
    (uploaded once), a ``Batch`` (read where it lies; it must outlive the chain) or, with ``emissions=True``, float64
    emissions (n, S); ``offsets`` (R + 1,) cuts the rows into records.  ``set`` then ``expect`` / ``decode`` /
    ``emissions``.  ValueError for what the library refuses as an argument or as not finite."""
    _destroy = "phk_chain_destroy"

    def __init__(self, ctx, rows, offsets, n_states, batch_rows=0, emissions=False):
        self.ctx, self.S = ctx, int(n_states)
        off = np.ascontiguousarray(offsets, dtype=np.uint64)
        if off.ndim != 1 or off.shape[0] < 1:
            raise ValueError("offsets must be (R + 1,)")
        self.R = off.shape[0] - 1
        if not 0 <= self.S < 2 ** 32:
            raise ValueError("n_states = %r" % (n_states,))
        h = ctypes.c_void_p()
        if emissions:
            E = np.ascontiguousarray(rows, dtype=np.float64)
            if E.ndim != 2 or E.shape[1] != self.S:
                raise ValueError("the emissions must be (n, %d), got shape %r" % (self.S, E.shape))
            self.n, self.D, self.from_counts = E.shape[0], 0, False
            rc = ctx.lib.phk_chain_create_from_emissions(ctx.handle, ptr(E), self.n, ptr(off), self.R, self.S, ctypes.byref(h))
        elif isinstance(rows, Batch):
            rows._open()
            self.n, self.D, self.from_counts = rows.n, rows.D, True
            self._batch = rows
            rc = ctx.lib.phk_batch_chain_create(ctx.handle, rows.handle, ptr(off), self.R, self.S, int(batch_rows), ctypes.byref(h))
        else:
            c = np.ascontiguousarray(rows, dtype=np.uint32)
            if c.ndim != 2:
                raise ValueError("the counts must be (n, D)")
            self.n, self.D, self.from_counts = c.shape[0], c.shape[1], True
            rc = ctx.lib.phk_chain_create(ctx.handle, ptr(c), self.n, self.D, ptr(off), self.R, self.S, int(batch_rows),
                                          ctypes.byref(h))
        self._rc(rc)
        self.handle = h
        self.G = 0     # groups (set_groups); 0: one set of parameters for every record

    @staticmethod
    def _rc(rc):
        if rc == PHK_ERR_NAN:
            raise ValueError(last_error())
        check_value(rc, nan=False)

    def set(self, log_profiles, trans, init, qlog_trans, qlog_init, temper=1.0):
        """The parameters of the calls that follow (phk_chain_set); forms the emissions on the device.  ``log_profiles``
        (S, D), None for a chain made from emissions; ``qlog_*``: the quantised logarithms (segment.quantise)."""
        self._open()
        S = self.S
        lp = None if log_profiles is None else np.ascontiguousarray(log_profiles, dtype=np.float64)
        if lp is not None and (lp.ndim != 2 or lp.shape[0] != S):
            raise ValueError("log_profiles must be (%d, D)" % S)
        tr, pi = np.ascontiguousarray(trans, dtype=np.float64), np.ascontiguousarray(init, dtype=np.float64)
        qt, qp = np.ascontiguousarray(qlog_trans, dtype=np.int64), np.ascontiguousarray(qlog_init, dtype=np.int64)
        if tr.shape != (S, S) or pi.shape != (S,) or qt.shape != (S, S) or qp.shape != (S,):
            raise ValueError("trans must be (%d, %d) and init (%d,), with their quantised logarithms" % (S, S, S))
        self._rc(self.ctx.lib.phk_chain_set(self.ctx.handle, self.handle, ptr(lp), 0 if lp is None else lp.shape[1], ptr(tr),
                                            ptr(pi), ptr(qt), ptr(qp), float(temper)))

    def set_scan(self, scan_from):
        """Records of at least ``scan_from`` windows take the tile scan in every later ``expect`` and
        ``decode`` (phk_chain_set_scan); 0: none, the state after create.  Before or after ``set``."""
        self._open()
        scan_from = int(scan_from)
        if not 0 <= scan_from < 2 ** 64:
            raise ValueError("scan_from = %r" % (scan_from,))
        self._rc(self.ctx.lib.phk_chain_set_scan(self.ctx.handle, self.handle, scan_from))

    def set_groups(self, group_offsets):
        """Cuts the records into groups of consecutive records (phk_chain_set_groups):
        ``group_offsets`` (G + 1,) runs from 0 to R; every group then has parameters of its own (``set_grouped``,
        ``expect_grouped``; ``decode`` and ``emissions`` work as before).  None returns the chain to one set of parameters."""
        self._open()
        if group_offsets is None:
            self._rc(self.ctx.lib.phk_chain_set_groups(self.ctx.handle, self.handle, None, 0))
            self.G = 0
            return
        go = np.ascontiguousarray(group_offsets, dtype=np.uint64)
        if go.ndim != 1 or go.shape[0] < 2:
            raise ValueError("group_offsets must be (G + 1,) with G >= 1")
        self._rc(self.ctx.lib.phk_chain_set_groups(self.ctx.handle, self.handle, ptr(go), go.shape[0] - 1))
        self.G = go.shape[0] - 1

    def set_grouped(self, log_profiles, trans, init, qlog_trans, qlog_init, temper=1.0, active=None):
        """The parameters of every group (phk_chain_set_grouped): ``log_profiles`` (G, S, D), ``trans`` (G, S, S), ``init``
        (G, S) with their quantised logarithms; ``active`` (G,) bool or None for all.  An inactive group is passed over by
        every kernel, its parameters are not read and its outputs are zeros."""
        self._open()
        S, G = self.S, self.G
        lp = np.ascontiguousarray(log_profiles, dtype=np.float64)
        tr, pi = np.ascontiguousarray(trans, dtype=np.float64), np.ascontiguousarray(init, dtype=np.float64)
        qt, qp = np.ascontiguousarray(qlog_trans, dtype=np.int64), np.ascontiguousarray(qlog_init, dtype=np.int64)
        if G and (lp.ndim != 3 or lp.shape[:2] != (G, S) or tr.shape != (G, S, S) or pi.shape != (G, S)
                  or qt.shape != (G, S, S) or qp.shape != (G, S)):
            raise ValueError("log_profiles must be (%d, %d, D), trans (%d, %d, %d) and init (%d, %d), with their quantised "
                             "logarithms" % (G, S, G, S, S, G, S))
        act = None
        if active is not None:
            act = np.ascontiguousarray(np.asarray(active).astype(bool), dtype=np.uint8)
            if act.shape != (G,):
                raise ValueError("active must be (%d,)" % G)
        self._rc(self.ctx.lib.phk_chain_set_grouped(self.ctx.handle, self.handle, ptr(lp), lp.shape[-1], ptr(tr), ptr(pi), ptr(qt),
                                                    ptr(qp), float(temper), ptr(act)))

    def expect_grouped(self, records=False):
        """One E-step of every group (phk_chain_expect_grouped): (T (G, S, D), Ns (G, S), xi (G, S, S), gamma0 (G, S),
        log_evidence (G,)), and with ``records`` also the log evidence per record (R,)."""
        self._open()
        S, G = self.S, self.G
        T, Ns, xi = np.zeros((G, S, self.D)), np.zeros((G, S)), np.zeros((G, S, S))
        g0, L = np.zeros((G, S)), np.zeros(G)
        rec = np.zeros(self.R) if records else None
        self._rc(self.ctx.lib.phk_chain_expect_grouped(self.ctx.handle, self.handle, ptr(T), ptr(Ns), ptr(xi), ptr(g0), ptr(L),
                                                       ptr(rec)))
        return (T, Ns, xi, g0, L) + ((rec,) if records else ())

    def emissions(self):
        """E (n, S) float64 as the device holds it (phk_chain_emissions)."""
        self._open()
        E = np.zeros((self.n, self.S), dtype=np.float64)
        self._rc(self.ctx.lib.phk_chain_emissions(self.ctx.handle, self.handle, ptr(E)))
        return E

    def expect(self, records=False):
        """One E-step (phk_chain_expect): (T (S, D), Ns (S,), xi (S, S), gamma0 (S,), log_evidence), and with ``records`` also
        the log evidence per record (R,).  T and Ns are None for a chain made from emissions."""
        self._open()
        S = self.S
        want = self.from_counts
        T, Ns = (np.zeros((S, self.D)), np.zeros(S)) if want else (None, None)
        xi, g0, L = np.zeros((S, S)), np.zeros(S), np.zeros(1)
        rec = np.zeros(self.R) if records else None
        self._rc(self.ctx.lib.phk_chain_expect(self.ctx.handle, self.handle, ptr(T), ptr(Ns), ptr(xi), ptr(g0), ptr(L), ptr(rec)))
        return (T, Ns, xi, g0, float(L[0])) + ((rec,) if records else ())

    def decode(self, posterior=True):
        """(state (n,) uint8, posterior (n, S) or None, log_evidence (R,), path_score (R,) int64) (phk_chain_decode)."""
        self._open()
        state = np.zeros(self.n, dtype=np.uint8)
        post = np.zeros((self.n, self.S)) if posterior else None
        le, ps = np.zeros(self.R), np.zeros(self.R, dtype=np.int64)
        self._rc(self.ctx.lib.phk_chain_decode(self.ctx.handle, self.handle, ptr(state), ptr(post), ptr(le), ptr(ps)))
        return state, post, le, ps


class Batch(_Resident):
    """Device-resident contig batch (phk_batch): counts + row sums in HBM; see include/phamers_hip.h."""
    _destroy = "phk_batch_free"

    def __init__(self, ctx, handle):
        self.ctx = ctx
        self.handle = handle
        n, D, T, inv = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_int()
        check(ctx.lib.phk_batch_shape(handle, ctypes.byref(n), ctypes.byref(D), ctypes.byref(T), ctypes.byref(inv)))
        self.n, self.D, self.total_bases, self.any_invalid = n.value, D.value, T.value, bool(inv.value)

    @property
    def folded(self):
        """True once the rows hold both strands (``fold_strands``); a selection and a column gather inherit it."""
        f = ctypes.c_int()
        check(self.ctx.lib.phk_batch_strands(self.handle, ctypes.byref(f)))
        return bool(f.value)

    @classmethod
    def from_fasta(cls, ctx, fasta, kmer_length, symbols=b"ATGC"):
        h = ctypes.c_void_p()
        check(ctx.lib.phk_batch_from_fasta(ctx.handle, fasta.handle, int(kmer_length), symbols, ctypes.byref(h)))
        return cls(ctx, h)

    @classmethod
    def from_sequences(cls, ctx, sequences, kmer_length, symbols=b"ATGC"):
        raw = [s.encode("latin-1", "replace") for s in sequences]
        offsets = np.zeros(len(raw) + 1, dtype=np.uint64)
        if raw:
            offsets[1:] = np.cumsum([len(r) for r in raw], dtype=np.uint64)
        bases = np.frombuffer(b"".join(raw) or b"\0", dtype=np.uint8)
        h = ctypes.c_void_p()
        check(ctx.lib.phk_batch_from_ascii(ctx.handle, ptr(np.ascontiguousarray(bases)), ptr(offsets), len(raw),
                                           int(kmer_length), symbols, ctypes.byref(h)))
        return cls(ctx, h)

    @classmethod
    def windows_from_fasta(cls, ctx, fasta, kmer_length, window, step, symbols=b"ATGC", segment=0):
        """The sliding windows of a parsed file's records as rows (phk_batch_windows_from_fasta)."""
        h = ctypes.c_void_p()
        check(ctx.lib.phk_batch_windows_from_fasta(ctx.handle, fasta.handle, int(kmer_length), symbols, int(window), int(step),
                                                   int(segment), ctypes.byref(h)))
        return cls(ctx, h)

    @classmethod
    def windows_from_sequences(cls, ctx, sequences, kmer_length, window, step, symbols=b"ATGC", segment=0):
        """The sliding windows [j step, j step + window) of every sequence as rows (phk_batch_windows_from_ascii): every base
        goes up once whatever the overlap.  ``segment`` = windows per work unit, 0 = chosen by the launch."""
        raw = [s.encode("latin-1", "replace") for s in sequences]
        offsets = np.zeros(len(raw) + 1, dtype=np.uint64)
        if raw:
            offsets[1:] = np.cumsum([len(r) for r in raw], dtype=np.uint64)
        bases = np.frombuffer(b"".join(raw) or b"\0", dtype=np.uint8)
        h = ctypes.c_void_p()
        check(ctx.lib.phk_batch_windows_from_ascii(ctx.handle, ptr(np.ascontiguousarray(bases)), ptr(offsets), len(raw),
                                                   int(kmer_length), symbols, int(window), int(step), int(segment), ctypes.byref(h)))
        return cls(ctx, h)

    @classmethod
    def from_counts(cls, ctx, counts):
        """A batch from an integer count matrix (n, 4^k) on the host -- the features cache of an earlier run (phk_batch_from_counts).
        None when the matrix is not such a one (another width, negative entries, an entry or a row sum of 2^32 or more): the caller keeps the float rows."""
        c = np.ascontiguousarray(counts, dtype=np.int64)
        if c.ndim != 2:
            return None
        h = ctypes.c_void_p()
        rc = ctx.lib.phk_batch_from_counts(ctx.handle, ptr(c), c.shape[0], c.shape[1], ctypes.byref(h))
        if rc == PHK_ERR_UNSUPPORTED:
            return None
        check(rc)
        return cls(ctx, h)

    def counts(self):
        """int64 (n, 4^k) on the host: what kmer.count_file returns (one download, widened on the device)."""
        out = np.zeros((self.n, self.D), dtype=np.int64)
        check(self.ctx.lib.phk_batch_counts_i64(self.ctx.handle, self.handle, ptr(out)))
        return out

    def counts_u32(self):
        """uint32 (n, 4^k) on the host, as the device holds them (what the features-cache writer takes)."""
        out = np.zeros((self.n, self.D), dtype=np.uint32)
        check(self.ctx.lib.phk_batch_counts_u32(self.ctx.handle, self.handle, ptr(out)))
        return out

    def row_sums(self):
        """uint32 (n,): the counted k-mers of every row (0 = a row that normalises to NaN)."""
        out = np.zeros(self.n, dtype=np.uint32)
        if self.n:
            d = ctypes.c_void_p()
            check(self.ctx.lib.phk_batch_device_ptrs(self.handle, None, ctypes.byref(d)))
            check(self.ctx.lib.phk_memcpy_d2h(self.ctx.handle, ptr(out), d, out.nbytes))
        return out

    def normalized(self):
        out = np.empty((self.n, self.D), dtype=np.float64)
        check(self.ctx.lib.phk_batch_normalized(self.ctx.handle, self.handle, ptr(out)))
        return out

    def select(self, rows):
        rows = np.ascontiguousarray(rows, dtype=np.uint64)
        h = ctypes.c_void_p()
        check(self.ctx.lib.phk_batch_select(self.ctx.handle, self.handle, ptr(rows), rows.shape[0], ctypes.byref(h)))
        return Batch(self.ctx, h)

    def column_sums(self):
        """int64 (4^k,): the column sums over the batch's rows, reduced on the device (phk_batch_column_sums)."""
        out = np.zeros(self.D, dtype=np.int64)
        check(self.ctx.lib.phk_batch_column_sums(self.ctx.handle, self.handle, ptr(out)))
        return out

    def gather_columns(self, table):
        """A new resident batch whose column j is this batch's column table[j] (phk_batch_gather_columns).  A table that is
        not a permutation can lift a row's sum to 2^32 or more, which a batch cannot hold: PhkError with code
        PHK_ERR_UNSUPPORTED then, and no batch (transform the host matrix with transform_kmers.transform_kmers instead)."""
        table = np.ascontiguousarray(table, dtype=np.uint32)
        if table.shape != (self.D,):
            raise ValueError("gather_columns: the table must have %d entries" % self.D)
        h = ctypes.c_void_p()
        check(self.ctx.lib.phk_batch_gather_columns(self.ctx.handle, self.handle, ptr(table), ctypes.byref(h)))
        return Batch(self.ctx, h)

    def fold_strands(self):
        """Adds to every resident row its reverse-complement permutation, in place (phk_batch_fold_strands): the counts of
        the sequence and of its reverse complement together, row sums doubled.  Returns the batch.  PhkError with code
        PHK_ERR_ARG when the batch is folded already, PHK_ERR_UNSUPPORTED (batch untouched) when a row's sum is 2^31 or
        more."""
        check(self.ctx.lib.phk_batch_fold_strands(self.ctx.handle, self.handle))
        return self

    def score(self, model, method="combo"):
        out = np.empty(self.n, dtype=np.float64)
        rc = self.ctx.lib.phk_batch_score(self.ctx.handle, model.handle, self.handle, METHODS[method], ptr(out))
        check_value(rc, arg=False)
        return out

    def likelihood(self, table, details=None):
        """Multinomial likelihood scores (n,) float64 of the resident count rows under a ``LikelihoodTable``
        (phk_batch_lik_score); ``details``: a dict that receives 'l_pos' and 'l_neg'."""
        self._open()
        return table._score(lambda lp, ln, sc: self.ctx.lib.phk_batch_lik_score(
            self.ctx.handle, table.handle, self.handle, ptr(lp), ptr(ln), ptr(sc)), self.n, details)

    def mixture_expect(self, table, batch_rows=0, rows=False):
        """One E-step of a ``MixtureTable`` over the resident count rows (phk_batch_mix_expect): (T, Nk, L), and with ``rows``
        also (row_ll, argmax, max_resp); see ``MixtureTable.expect``."""
        self._open()
        table._open()
        return table._expect(lambda *o: self.ctx.lib.phk_batch_mix_expect(
            self.ctx.handle, table.handle, self.handle, int(batch_rows), *o), self.n, rows)

    def mixture_responsibilities(self, table, batch_rows=0):
        """(r (n, K), row_ll (n,)) of the resident count rows (phk_batch_mix_responsibilities)."""
        self._open()
        table._open()
        r, ll = np.zeros((self.n, table.K)), np.zeros(self.n)
        check_value(self.ctx.lib.phk_batch_mix_responsibilities(self.ctx.handle, table.handle, self.handle, int(batch_rows),
                                                                ptr(r), ptr(ll)), nan=False)
        return r, ll

    def hosts(self, table, top):
        """(indices (n, top) int64, S (n, top) float64): the ``top`` most likely rows of a ``HostTable`` for every resident
        count row, by (S descending, index ascending) (phk_batch_host_rank)."""
        self._open()
        table._open()
        top = check_hosts_top(top, table.M)
        return table._rank(lambda idx, s: self.ctx.lib.phk_batch_host_rank(
            self.ctx.handle, table.handle, self.handle, top, ptr(idx), ptr(s)), self.n, top)

    def neighbors(self, model, k):
        """(distances (n, k), indices (n, k) int64 into the model's vstack(positive, negative)) of the k nearest train rows of
        every resident row, normalised on the device (phk_batch_neighbors).  ValueError for a row without counts."""
        idx, dist = _neighbor_outputs(self.n, k)
        return _neighbor_result(self.ctx.lib.phk_batch_neighbors(self.ctx.handle, model.handle, self.handle, int(k), ptr(idx),
                                                                 ptr(dist)), idx, dist)


def refine_grid_pass():
    """Boundaries one launch of the refinement kernel covers in one pass of its grid (phk_refine_grid_pass)."""
    return int(load().phk_refine_grid_pass())


def refine_boundaries(ctx, source, kmer_length, symbols, qtable, seq, lo, x, hi, left_row, right_row):
    """(position (B,) int64, evidence (B, 3) int64, support (B,) uint32) of phk_refine_boundaries_fasta (``source`` a
    ``Fasta``) or phk_refine_boundaries_ascii (a list of strings).  The arrays are converted, not checked: the library
    refuses what it does not take (ValueError for its PHK_ERR_ARG)."""
    return _refine_call("refine_boundaries", ctx, source, kmer_length, symbols, qtable, seq, lo, x, hi, left_row, right_row, None)


def refine_confidence(ctx, source, kmer_length, symbols, qtable, seq, lo, x, hi, left_row, right_row, drop_q):
    """``refine_boundaries``' three arrays, then interval (B, 3) int64 = (lower, upper, n_within) and sums (B, 5) float64 =
    (Z, M, S1_left, S1_right, S2) of phk_refine_confidence_fasta / _ascii; ``drop_q`` an integer in units of 2^-16 nat."""
    drop_q = int(drop_q)
    if not -2 ** 63 <= drop_q < 2 ** 63:
        raise ValueError("refine_confidence: drop_q must fit an int64")
    return _refine_call("refine_confidence", ctx, source, kmer_length, symbols, qtable, seq, lo, x, hi, left_row, right_row, drop_q)


def _refine_call(name, ctx, source, kmer_length, symbols, qtable, seq, lo, x, hi, left_row, right_row, drop_q):
    """phk_refine_boundaries_* (``drop_q`` None) or phk_refine_confidence_*."""
    q = np.ascontiguousarray(qtable, dtype=np.int64)
    if q.ndim != 2:
        raise ValueError("%s: the table must be (n_rows, D)" % name)
    u64 = lambda v: np.ascontiguousarray(v, dtype=np.uint64).ravel()
    u32 = lambda v: np.ascontiguousarray(v, dtype=np.uint32).ravel()
    seq, lo, x, hi, left_row, right_row = u64(seq), u64(lo), u64(x), u64(hi), u32(left_row), u32(right_row)
    B = seq.shape[0]
    if not all(a.shape[0] == B for a in (lo, x, hi, left_row, right_row)):
        raise ValueError("%s: seq, lo, x, hi, left_row and right_row must have one entry per boundary" % name)
    position, evidence = np.zeros(B, dtype=np.int64), np.zeros((B, 3), dtype=np.int64)
    support = np.zeros(B, dtype=np.uint32)
    out = (position, evidence, support)
    tail = (ptr(q), q.shape[0], q.shape[1], ptr(seq), ptr(lo), ptr(x), ptr(hi), ptr(left_row), ptr(right_row), B)
    if drop_q is None:
        entry = "phk_refine_boundaries_"
    else:
        entry = "phk_refine_confidence_"
        out += (np.zeros((B, 3), dtype=np.int64), np.zeros((B, 5), dtype=np.float64))
        tail += (drop_q,)
    tail += tuple(ptr(a) for a in out)
    if isinstance(source, Fasta):
        rc = getattr(ctx.lib, entry + "fasta")(ctx.handle, source.handle, int(kmer_length), symbols, *tail)
    else:
        raw = [s.encode("latin-1", "replace") for s in source]
        offsets = np.zeros(len(raw) + 1, dtype=np.uint64)
        if raw:
            offsets[1:] = np.cumsum([len(r) for r in raw], dtype=np.uint64)
        bases = np.frombuffer(b"".join(raw) or b"\0", dtype=np.uint8)
        rc = getattr(ctx.lib, entry + "ascii")(ctx.handle, ptr(np.ascontiguousarray(bases)), ptr(offsets), len(raw),
                                               int(kmer_length), symbols, *tail)
    check_value(rc, nan=False)
    return out


class Fasta(object):
    """A FASTA file parsed by the native multi-threaded reader (phk_fasta_read)."""

    def __init__(self, path, threads=0, part=None, byte_range=None, index_only=False):
        """``part`` = (i, n): only the records that begin in the i-th of n equal byte ranges of the file (one rank's
        share, phk_fasta_read_part); ``byte_range`` = (lo, hi): those that begin in [lo, hi) (phk_fasta_read_range);
        ``index_only``: ids, titles and lengths without the sequences (phk_fasta_index)."""
        self.lib = load()
        h = ctypes.c_void_p()
        if index_only:
            rc = self.lib.phk_fasta_index(os.fsencode(path), int(threads), ctypes.byref(h))
        elif part is not None:
            rc = self.lib.phk_fasta_read_part(os.fsencode(path), int(part[0]), int(part[1]), int(threads), ctypes.byref(h))
        elif byte_range is not None:
            hi = 0xFFFFFFFFFFFFFFFF if byte_range[1] is None else int(byte_range[1])
            rc = self.lib.phk_fasta_read_range(os.fsencode(path), int(byte_range[0]), hi, int(threads), ctypes.byref(h))
        else:
            rc = self.lib.phk_fasta_read(os.fsencode(path), int(threads), ctypes.byref(h))
        if rc == PHK_ERR_IO:
            raise IOError(self.lib.phk_last_error().decode("utf-8", "replace"))
        check(rc)
        self._attach(h)

    def _attach(self, h):
        self.handle = h
        n, t, tb = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        check(self.lib.phk_fasta_shape(h, ctypes.byref(n), ctypes.byref(t), ctypes.byref(tb)))
        self.n_records, self.total_bases, self.title_bytes = n.value, t.value, tb.value
        b, o, ti, to = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        check(self.lib.phk_fasta_data(h, ctypes.byref(b), ctypes.byref(o), ctypes.byref(ti), ctypes.byref(to)))
        self._bases, self._offsets, self._titles, self._title_off = b.value, o.value, ti.value, to.value

    @classmethod
    def count_file(cls, ctx, path, kmer_length, symbols=b"ATGC", threads=0, part=None):
        """(index, batch) of a FASTA file in one call (phk_batch_from_fasta_file): the sequences are parsed straight into the
        upload's staging buffers -- no host copy of them exists; ``index`` is a Fasta as ``index_only=True`` gives it (titles,
        ids, lengths).  ``part`` = (i, n): the records that begin in the i-th of n equal byte ranges of the file only (one
        rank's share, phk_batch_from_fasta_part).  IOError when the file cannot be read."""
        self = cls.__new__(cls)
        self.lib = load()
        h, hb = ctypes.c_void_p(), ctypes.c_void_p()
        if part is not None:
            rc = self.lib.phk_batch_from_fasta_part(ctx.handle, os.fsencode(path), int(part[0]), int(part[1]), int(kmer_length),
                                                    symbols, int(threads), ctypes.byref(h), ctypes.byref(hb))
        else:
            rc = self.lib.phk_batch_from_fasta_file(ctx.handle, os.fsencode(path), int(kmer_length), symbols, int(threads),
                                                    ctypes.byref(h), ctypes.byref(hb))
        if rc == PHK_ERR_IO:
            raise IOError(self.lib.phk_last_error().decode("utf-8", "replace"))
        check(rc)
        self._attach(h)
        return self, Batch(ctx, hb)

    def offsets(self):
        return np.ctypeslib.as_array(ctypes.cast(self._offsets, ctypes.POINTER(ctypes.c_uint64)),
                                     shape=(self.n_records + 1,)).copy()

    def lengths(self):
        return np.diff(self.offsets().astype(np.int64))

    def titles(self):
        off = np.ctypeslib.as_array(ctypes.cast(self._title_off, ctypes.POINTER(ctypes.c_uint64)),
                                    shape=(self.n_records + 1,))
        raw = ctypes.string_at(self._titles, self.title_bytes) if self.title_bytes else b""
        return [raw[int(off[i]):int(off[i + 1])].decode("latin-1") for i in range(self.n_records)]

    def ids(self):
        """Bio.SeqIO record.id: the first white-space delimited word of each title."""
        return [(t.split(None, 1) or [""])[0] for t in self.titles()]

    def phamers_ids(self):
        """What fileIO.get_fasta_ids returns (scripts/fileIO.py:62-77): id_parser.get_id of every record.id,
        parsed by the native reader.  Raises IndexError where the reference does (a header that matches none of
        its three shapes); a header for which the reference returns None gives None (object array)."""
        n = self.n_records
        ids, off, st = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        check(self.lib.phk_fasta_ids(self.handle, ctypes.byref(ids), ctypes.byref(off), ctypes.byref(st)))
        if n == 0:
            return np.array([])
        status = np.ctypeslib.as_array(ctypes.cast(st.value, ctypes.POINTER(ctypes.c_uint8)), shape=(n,))
        if (status == 1).any():
            bad = int(np.argmax(status == 1))
            raise IndexError("list index out of range (FASTA header %r has none of the id shapes)" % self.titles_at(bad))
        offs = np.ctypeslib.as_array(ctypes.cast(off.value, ctypes.POINTER(ctypes.c_uint64)), shape=(n + 1,))
        width = max(int(np.diff(offs.astype(np.int64)).max()), 1)
        fixed = np.zeros(n, dtype="S%d" % width)
        check(self.lib.phk_fasta_ids_fixed(self.handle, width, ptr(fixed)))
        # latin-1 decode = code point identity: bytes -> uint32 -> 'U' view, without a Python loop over the ids
        out = np.ascontiguousarray(fixed.view(np.uint8).reshape(n, width).astype(np.uint32)).view("U%d" % width)[:, 0]
        if (status == 2).any():
            out = out.astype(object)
            out[status == 2] = None
        return out

    def titles_at(self, i):
        off = np.ctypeslib.as_array(ctypes.cast(self._title_off, ctypes.POINTER(ctypes.c_uint64)),
                                    shape=(self.n_records + 1,))
        return ctypes.string_at(self._titles + int(off[i]), int(off[i + 1] - off[i])).decode("latin-1")

    def sequences(self):
        off = self.offsets()
        if self.total_bases and not self._bases:
            raise ValueError("this Fasta was opened with index_only=True: it holds no sequences")
        raw = ctypes.string_at(self._bases, self.total_bases) if self.total_bases else b""
        return [raw[int(off[i]):int(off[i + 1])].decode("latin-1") for i in range(self.n_records)]

    def count(self, ctx, kmer_length, symbols=b"ATGC"):
        out = np.zeros((self.n_records, 4 ** int(kmer_length)), dtype=np.int64)
        check(self.lib.phk_count_fasta(ctx.handle, self.handle, int(kmer_length), symbols, ptr(out)))
        return out

    def close(self, wait=True):
        """Frees the parsed file.  ``wait=False``: on a helper thread -- unmapping the sequence buffer of a multi-GB file
        takes tenths of a second (0.23 s for 5 GB) that the caller need not stand in."""
        h, self.handle = getattr(self, "handle", None), None
        if not h:
            return
        if wait:
            self.lib.phk_fasta_free(h)
        else:
            threading.Thread(target=self.lib.phk_fasta_free, args=(h,), name="phamers-fasta-free").start()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def get_context(device=None):
    """Process-wide default context for ``device`` (created on first use)."""
    dev = default_device() if device is None else int(device)
    with _lock:
        ctx = _contexts.get(dev)
    if ctx is None:
        ctx = Context(dev)
        with _lock:
            _contexts.setdefault(dev, ctx)
            ctx = _contexts[dev]
    return ctx
