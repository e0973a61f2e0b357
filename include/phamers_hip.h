/*
 * phamers_hip.h -- C ABI of libphamers_hip.so, the MI355X (gfx950) k-mer count +
 * phage-score path behind PhaMers' Python hot-path functions.
 *
 * The reference (jondeaton/PhaMers, Python 2.7) has no FFI / plugin interface: its
 * boundary for this path is a set of Python call signatures.  Each entry point below
 * names the reference function (file:line, relative to the PhaMers tree) whose
 * arithmetic it replaces; phamers_amd/{kmer,learning,phamer}.py bind them with ctypes
 * and reproduce the Python-level names, defaults, return shapes and soft-failure
 * behaviour (INTEGRATION.md shows the stub a PhaMers maintainer would add).
 *
 * Conventions
 *   - plain C: pointers + sizes, no C++/torch types.  Every function returns
 *     PHK_OK (0) or a negative PHK_ERR_* code; phk_last_error() gives the text
 *     (thread-local).
 *   - the library never allocates caller-visible memory: outputs are caller-allocated.
 *   - "host API" functions take HOST pointers, are synchronous, and stage through a
 *     per-context device workspace.  "device API" functions (suffix _dev) take DEVICE
 *     pointers (hipMalloc / torch data_ptr), enqueue on the context's HIP stream and
 *     return without synchronising (phk_sync() to wait).
 *   - one context per (process, GPU); calls on one context are serialised on its
 *     stream; distinct contexts may be used from distinct threads.
 *
 * Packed base stream (the device-side sequence format; this library's own layout)
 *   All contigs of a batch are concatenated into ONE stream of T bases with no padding.
 *   offsets[n+1] (uint64, in bases, offsets[0] = 0, offsets[n] = T) delimits contig c as
 *   stream positions [offsets[c], offsets[c+1]).
 *   packed : uint32 words, ceil(T/16)+1 of them (one zero pad word).  Base g is the 2-bit
 *            field at bits [30-2*(g%16), 31-2*(g%16)] of word g/16 -- the FIRST base of a
 *            word sits in the MOST significant bits, so a k-mer read off the word is
 *            already the reference's bin index (first base = most significant base-4
 *            digit, scripts/kmer.py:50).  Codes follow the symbols string: for the
 *            default 'ATGC' A=0 T=1 G=2 C=3 (scripts/kmer.py:28).
 *   mask   : optional validity bits, uint32 words, ceil(T/32)+1 of them; bit 31-(g%32) of
 *            word g/32 is 1 when base g is one of the 4 symbols (case-sensitive) and 0
 *            otherwise (the reference's '-', scripts/kmer.py:190-191).  NULL = all valid.
 *   A window is counted iff all k of its bases lie inside one contig and are valid
 *   (scripts/kmer.py:47-50).
 */
#ifndef PHAMERS_HIP_H
#define PHAMERS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2 (round 5): phk_kmeans_lloyd reports the smallest assignment gap; phk_batch_from_fasta_part; knobs, see phk_set_option */
#define PHK_ABI_VERSION 2

#define PHK_OK 0
#define PHK_ERR_ARG (-1)         /* bad argument (null pointer, bad k, bad shape) */
#define PHK_ERR_HIP (-2)         /* HIP runtime error; text has hipGetErrorString */
#define PHK_ERR_NOMEM (-3)       /* device allocation failed */
#define PHK_ERR_UNSUPPORTED (-4) /* outside the implemented path (e.g. k > PHK_MAX_K) */
#define PHK_ERR_NAN (-5)         /* a query row contains NaN (zero-count contig), see phk_score_* */
#define PHK_ERR_IO (-6)          /* file cannot be opened / read (phk_fasta_read) */

#define PHK_MAX_K 7              /* 4^k uint32 bins must fit one wave's LDS histogram */

#define PHK_METHOD_KNN 1         /* scripts/phamer.py:268-273 */
#define PHK_METHOD_KMEANS 2      /* scripts/phamer.py:240-256 (centroids supplied) */
#define PHK_METHOD_COMBO 3       /* scripts/phamer.py:303-313 */
#define PHK_METHOD_DENSITY 4     /* scripts/phamer.py:275-287; exclusive: not to be OR-ed with the others */
#define PHK_METHOD_SVM 5         /* scripts/phamer.py:258-266; exclusive, needs phk_model_fit_svm first */

typedef struct phk_ctx phk_ctx;
typedef struct phk_model phk_model;
typedef struct phk_fasta phk_fasta;
typedef struct phk_batch phk_batch;

/* ---- library / context ------------------------------------------------------------- */
int phk_abi_version(void);
const char *phk_last_error(void);
int phk_device_count(int *count);
/* stream: a hipStream_t to enqueue on (e.g. torch.cuda.current_stream().cuda_stream), or
 * NULL to let the context create and own a stream. */
int phk_create(int device_id, void *stream, phk_ctx **out);
int phk_destroy(phk_ctx *ctx);
int phk_sync(phk_ctx *ctx);
/* Tuning / diagnostic knobs of a context.  Each knob takes its initial value from the environment variable
 * PHK_<KEY upper case> ONCE, when the context is created; afterwards it changes only through this call (no
 * launch path reads the environment).  Keys: "count_lanes" ("0" wave-per-contig count kernel only, "f" the slot
 * kernel whatever the batch looks like, "P" / "p" the two-windows-per-add kernel with 1024 / 512 threads where the
 * batch's statistics allow it, "Q" / "q" the same forced), "count_sort" ("0" = no
 * length-bucketed order for ragged batches), "force_exact" ("1" = float64 scoring path for every model), "proposal"
 * ("" default: high parts only at k = 4, the two-part int8 sweep at k = 5, 6 | "f16" split-query kernel | "hi" / "cxf" /
 * "i83": the general-D alternatives), "cx_cfg" ("24" | "28": workgroup shape of the k = 4 sweep), "rerank" ("w" | "g"),
 * "score_batch" (queries per scoring batch), "tail_aside" ("0" = a multi-batch call keeps every batch's queue tail on
 * the main stream), "gen_groups" / "gen_seq" / "i8_insert" (general-D sweep shapes), "ws_fail" (fault injection for
 * the tests: the n-th workspace request from now fails with PHK_ERR_NOMEM; not read from the environment).
 * Unknown key -> PHK_ERR_ARG.  The results of every entry point are the same under every setting; the parity tests
 * use the knobs to cross-check the paths.  (ABI 2 dropped "count_cfg", "slot_threads", "pipeline" and the proposal
 * values "f32" / "cx2" with the kernels behind them.) */
int phk_set_option(phk_ctx *ctx, const char *key, const char *value);

/* device buffers for hosts that do not bring their own allocator */
int phk_malloc(phk_ctx *ctx, uint64_t bytes, void **dptr);
int phk_free(phk_ctx *ctx, void *dptr);
int phk_memcpy_h2d(phk_ctx *ctx, void *dst_dev, const void *src_host, uint64_t bytes);
int phk_memcpy_d2h(phk_ctx *ctx, void *dst_host, const void *src_dev, uint64_t bytes);

/* ---- host API: counting ------------------------------------------------------------ */
/* kmer.count_string / kmer.count (scripts/kmer.py:32-50, 82-111): n sequences given as
 * concatenated ASCII `bases` + offsets[n+1]; counts[n][4^k] int64 (NumPy's default int, as
 * the reference returns).  symbols: the 4 characters that code 0..3 (the reference's
 * `symbols` argument when it has exactly 4 characters; "ATGC" by default). */
int phk_count_ascii(phk_ctx *ctx, const char *bases, const uint64_t *offsets, uint64_t n, int k,
                    const char *symbols4, int64_t *counts);

/* kmer.normalize_counts (scripts/kmer.py:209-221): out[r][j] = (double)counts[r][j] /
 * (double)sum_j counts[r][j]; a zero row gives NaN exactly as the reference does, and a row with entries that sums to
 * zero (negative entries) gives +-inf and NaN as NumPy's division does.  The row sum is formed in 64-bit integers and
 * converted once, where the reference converts every entry and sums in float64: the two are equal, and the result bit
 * for bit the reference's, while the entries' magnitudes sum to less than 2^53 (any count matrix); beyond that the
 * integer entry point is not exact -- pass such a matrix as float64 to phk_normalize_f64. */
int phk_normalize_i64(phk_ctx *ctx, const int64_t *counts, uint64_t n, uint64_t D, double *out);
/* same for an already-float matrix: the row sum in the order of NumPy's np.sum on a contiguous float64 row (pairwise in
 * pieces of 8 192 elements, the pieces' sums added in order), the quotient an IEEE division */
int phk_normalize_f64(phk_ctx *ctx, const double *rows, uint64_t n, uint64_t D, double *out);

/* transform_kmers.transform_kmers (scripts/transform_kmers.py:68-88): out[r][j] = rows[r][perm[j]]; the
 * reverse / complement / reverse-complement count vectors are column permutations (perm built by the
 * host facade). */
int phk_permute_columns_i64(phk_ctx *ctx, const int64_t *rows, uint64_t n, uint64_t D, const uint32_t *perm,
                            int64_t *out);
/* Strand-symmetric counts of a host matrix: out[r][c] = counts[r][c] + counts[r][rc(c)], rc(c) = the column of the
 * reverse-complement k-mer (the k base-4 digits of c reversed, bit 0 of each flipped: see phk_batch_fold_strands).  64-bit
 * sums: no limit on the entries.  PHK_ERR_UNSUPPORTED when D is not 4^k with 1 <= k <= PHK_MAX_K. */
int phk_fold_strands_i64(phk_ctx *ctx, const int64_t *counts, uint64_t n, uint64_t D, int64_t *out);

/* ---- host API: FASTA ingest --------------------------------------------------------- */
/* One multi-threaded pass over a FASTA file (plain, or gzip when the name ends in ".gz") replacing
 * the Biopython passes of kmer.count_file (scripts/kmer.py:124-140) and fileIO.read_fasta /
 * get_fasta_ids / get_fasta_sequences (scripts/fileIO.py:28-94).  Record semantics are Bio.SeqIO's:
 * title = '>' line minus '>' and trailing white space (record.id = its first word); sequence = the
 * following lines with trailing white space, ' ' and '\r' removed.  threads <= 0 = automatic.
 * Returns PHK_ERR_IO when the file cannot be read (count_file then returns (None, None),
 * scripts/kmer.py:126-128). */
int phk_fasta_read(const char *path, int threads, phk_fasta **out);
/* Titles, ids and sequence LENGTHS only (offsets as phk_fasta_read gives them; phk_fasta_data returns NULL for the bases
 * and the handle cannot be counted): what phamer_scorer.screen_by_length needs when the features came from the cache
 * (scripts/phamer.py:144-157 parses the whole file again for the lengths).  One pass over the file, no sequence buffer. */
int phk_fasta_index(const char *path, int threads, phk_fasta **out);
/* The same pass over ONE rank's share of the file (the multi-GPU form of kmer.count_file's loop, scripts/kmer.py:
 * 124-140 with fileIO.get_fasta_ids scripts/fileIO.py:62-77: records are independent, so the file is cut by bytes):
 * the records whose '>' line begins in bytes [byte_lo, byte_hi) of the file (of the decompressed stream for ".gz").
 * Ranges that tile [0, size) give every record to exactly one range wherever the cuts fall (inside a sequence line, a
 * title, at a '>' that does not begin a line); byte_hi past the end = to the end.  Only the range's own bytes are
 * read from a plain file.  phk_fasta_read_part: range `part` of `n_parts` equal byte ranges. */
int phk_fasta_read_range(const char *path, uint64_t byte_lo, uint64_t byte_hi, int threads, phk_fasta **out);
int phk_fasta_read_part(const char *path, uint32_t part, uint32_t n_parts, int threads, phk_fasta **out);
int phk_fasta_shape(const phk_fasta *f, uint64_t *n_records, uint64_t *total_bases, uint64_t *title_bytes);
/* borrowed pointers, valid until phk_fasta_free: concatenated sequence bytes + offsets[n+1] (exactly the
 * arguments of phk_count_ascii), concatenated titles + title_offsets[n+1] */
int phk_fasta_data(const phk_fasta *f, const char **bases, const uint64_t **offsets, const char **titles,
                   const uint64_t **title_offsets);
int phk_fasta_free(phk_fasta *f);

/* FASTA header -> PhaMers id (id_parser.get_id, scripts/id_parser.py:89-100, with get_contig_id :18-30,
 * get_phage_id :71-77, get_bacteria_id :57-68, is_genbank_id :80-86).  *status says what the reference does with
 * the header: PHK_ID_OK (the id is written to id_out, *id_len bytes, no terminator), PHK_ID_INDEX_ERROR (the
 * reference raises IndexError: a header that matches none of its three shapes), PHK_ID_NONE (it returns None). */
#define PHK_ID_OK 0
#define PHK_ID_INDEX_ERROR 1
#define PHK_ID_NONE 2
int phk_parse_id(const char *header, uint64_t header_len, char *id_out, uint64_t cap, uint64_t *id_len, int *status);
/* the ids of a parsed file, computed by the reader's threads from each record.id (what fileIO.get_fasta_ids
 * returns, scripts/fileIO.py:62-77): concatenated ids + id_offsets[n+1] + id_status[n]; borrowed pointers */
int phk_fasta_ids(const phk_fasta *f, const char **ids, const uint64_t **id_offsets, const uint8_t **id_status);
/* the same as a [n][width] zero-padded byte matrix (a NumPy 'S<width>' array) in caller memory */
int phk_fasta_ids_fixed(const phk_fasta *f, uint64_t width, char *out);
/* kmer.count_file's counting loop (scripts/kmer.py:135-139) on a parsed file: counts[n][4^k] int64 */
int phk_count_fasta(phk_ctx *ctx, const phk_fasta *f, int k, const char *symbols4, int64_t *counts);

/* ---- on-disk formats either side of the path (host only) ------------------------------- */
/* fileIO.save_counts (scripts/fileIO.py:169-181): `prefix` (the '# ' header block, NUL-terminated, may be NULL) then
 * one "id,c0,c1,...\n" line per row; counts are uint32 (elem_bytes 4) or int64 (8), [n][D].  ids: concatenated bytes
 * + id_offsets[n+1].  Formatted on all cores; byte-identical to the reference's np.savetxt output. */
int phk_write_counts_csv(const char *path, const char *prefix, const char *ids, const uint64_t *id_offsets,
                         const void *counts, int elem_bytes, uint64_t n, uint64_t D);
/* fileIO.save_phamer_scores (scripts/fileIO.py:241-253): "id, score\n" lines, the score written as
 * str(numpy.float64) writes it (shortest round-trip digits, Python's positional / scientific rule). */
int phk_write_scores_csv(const char *path, const char *prefix, const char *ids, const uint64_t *id_offsets,
                         const double *scores, uint64_t n);
/* the same two writers with the ids given as a NumPy 'U<id_width>' array as it lies in memory ([n][id_width] UCS-4 code
 * points, NUL padded; written as str(id).encode('latin-1', 'replace')): no per-id Python work for 10^6 rows */
int phk_write_counts_csv_ucs4(const char *path, const char *prefix, const uint32_t *ids, uint64_t id_width,
                              const void *counts, int elem_bytes, uint64_t n, uint64_t D);
int phk_write_scores_csv_ucs4(const char *path, const char *prefix, const uint32_t *ids, uint64_t id_width,
                              const double *scores, uint64_t n);
/* one float64 in that notation (NUL-terminated) */
int phk_format_float(double v, char *out, int cap);
/* fileIO.read_feature_file (scripts/fileIO.py:134-166) for files of the shape save_counts writes: '#' comment lines
 * and blank lines skipped, every other line "id,int,int,...".  phk_features_open maps the file and indexes its rows
 * (n rows, D count columns, the longest id in bytes); phk_features_read parses them on all cores into counts[n][D]
 * int64 and ids[n][id_width] (zero padded: a NumPy 'S<id_width>' array).  Anything np.loadtxt would treat differently
 * -- a '#' inside a line, a row with another number of fields, a field that is not a plain decimal integer, a
 * non-ASCII id -- gives PHK_ERR_UNSUPPORTED, and the caller reads the file the reference's way (np.loadtxt). */
typedef struct phk_features phk_features;
int phk_features_open(const char *path, phk_features **out, uint64_t *n, uint64_t *D, uint64_t *id_width);
int phk_features_read(const phk_features *f, int64_t *counts, char *ids, uint64_t id_width);
int phk_features_close(phk_features *f);

/* ---- device-resident contig batches (the facade's data path) ------------------------- */
/* What a PhaMers user calls on a FASTA input -- phamer_scorer.load_data + score_points (scripts/phamer.py:131, 139,
 * 579), kmer.count_file (scripts/kmer.py:114-140) -- with every intermediate kept on the device.  A batch is built
 * from host sequence bytes (uploaded once, in chunks through pinned staging buffers, copies overlapped with the packer) and owns
 * counts[n][4^k] uint32 + row sums in HBM; counts come back only when asked for (the features cache,
 * scripts/phamer.py:132-134), scores are the only per-call download. */
int phk_batch_from_ascii(phk_ctx *ctx, const char *bases, const uint64_t *offsets, uint64_t n, int k,
                         const char *symbols4, phk_batch **out);
int phk_batch_from_fasta(phk_ctx *ctx, const phk_fasta *f, int k, const char *symbols4, phk_batch **out);
/* FASTA file -> device-resident batch in one call (kmer.count_file as load_data uses it, scripts/kmer.py:114-140,
 * scripts/phamer.py:131): the records are measured in one pass over the file and their sequences then written straight into
 * the upload's pinned staging buffers, chunk by chunk, overlapped with the bus and the packer -- no host copy of the
 * sequences exists.  *index_out: titles, ids and lengths as phk_fasta_index gives them (free with phk_fasta_free). */
int phk_batch_from_fasta_file(phk_ctx *ctx, const char *path, int k, const char *symbols4, int threads,
                              phk_fasta **index_out, phk_batch **out);
/* The same for one rank's share of the file: the records whose '>' line begins in byte range `part` of `n_parts` equal
 * ranges (the ranges of phk_fasta_read_part).  What rank `part` of `python -m phamers_amd.phamer --gpus n_parts` loads
 * (scripts/phamer.py:131 on a shard; contigs are independent, scripts/kmer.py:102-105). */
int phk_batch_from_fasta_part(phk_ctx *ctx, const char *path, uint32_t part, uint32_t n_parts, int k,
                              const char *symbols4, int threads, phk_fasta **index_out, phk_batch **out);
/* A batch from a count matrix on the host -- the features cache read back by fileIO.read_feature_file
 * (scripts/phamer.py:132-136, scripts/fileIO.py:134-166): counts[n][D] int64 row-major, D = 4^k.  The run then scores from
 * the same resident integers as one that counted the FASTA file (the reference normalises the cached counts to float rows
 * first: the scores are equal to rounding, and equal bit for bit to the cold run's here).  total_bases of such a batch is 0.
 * PHK_ERR_UNSUPPORTED: D is not 4^k with k <= PHK_MAX_K, an entry is negative or >= 2^32, or a row's sum is >= 2^32 (a
 * batch keeps its row sums as uint32). */
int phk_batch_from_counts(phk_ctx *ctx, const int64_t *counts, uint64_t n, uint64_t D, phk_batch **out);
/* Sliding windows: the rows of the batch are the windows [j step, j step + window) of every sequence, j = 0 ..
 * (L - window) / step, sequence-major and ordered by start; a sequence shorter than `window` gives no row.  Row j holds
 * what a count of seq[j step : j step + window] gives (same bins, k-mers touching an invalid base skipped).  Every base
 * goes up and is packed once; the kernels derive a window from its predecessor (step k-mers enter, step leave).
 * `segment` = windows per work unit (the first window of a unit is counted in full), 0 = chosen by the launch: the
 * result does not depend on it.  The batch stands as one from phk_batch_from_ascii (total_bases = rows * window).
 * PHK_ERR_ARG: window < k, step < 1, a NULL pointer, or no window at all; PHK_ERR_UNSUPPORTED: k > PHK_MAX_K. */
int phk_batch_windows_from_ascii(phk_ctx *ctx, const char *bases, const uint64_t *offsets, uint64_t n, int k,
                                 const char *symbols4, uint64_t window, uint64_t step, uint32_t segment,
                                 phk_batch **out);
int phk_batch_windows_from_fasta(phk_ctx *ctx, const phk_fasta *f, int k, const char *symbols4,
                                 uint64_t window, uint64_t step, uint32_t segment, phk_batch **out);
/* *segments = the work units one window launch at this k takes in a single pass of its grid (more are taken by the
 * kernels' grid-stride loops): what a test has to exceed to reach those loops. */
int phk_windows_grid_pass(int k, uint64_t *segments);
int phk_batch_shape(const phk_batch *b, uint64_t *n, uint64_t *D, uint64_t *total_bases, int *any_invalid);
/* borrowed device pointers (valid until phk_batch_free): counts[n][D] uint32, row sums[n] uint32 */
int phk_batch_device_ptrs(const phk_batch *b, const uint32_t **d_counts, const uint32_t **d_rowsums);
/* kmer.count_file's count matrix as the reference returns it (int64, scripts/kmer.py:130-139) */
int phk_batch_counts_i64(phk_ctx *ctx, const phk_batch *b, int64_t *counts);
/* the same as the device holds it (uint32; half the download, what the features-cache writer takes) */
int phk_batch_counts_u32(phk_ctx *ctx, const phk_batch *b, uint32_t *counts);
/* kmer.normalize_counts of the batch (scripts/kmer.py:209-221; zero row -> NaN), float64 [n][D] to the host */
int phk_batch_normalized(phk_ctx *ctx, const phk_batch *b, double *rows);
/* rows[0..m) of a batch as a new batch: the row filter of phamer_scorer.screen_by_length (scripts/phamer.py:
 * 144-157) as a device gather */
int phk_batch_select(phk_ctx *ctx, const phk_batch *b, const uint64_t *rows, uint64_t m, phk_batch **out);
/* Column sums of a batch, sums[4^k] int64 to the host: kmer.count_directory's per-file np.sum(file_counts, axis=0)
 * (scripts/kmer.py:170-173), which is how a reference matrix row is regenerated from a genome file. */
int phk_batch_column_sums(phk_ctx *ctx, const phk_batch *b, int64_t *sums);
/* transform_kmers.transform_kmers (scripts/transform_kmers.py:68-88) on resident counts: a new batch with
 * out[r][j] = counts[r][table[j]] (table: 4^k host entries, each < 4^k; the reference's tables are not permutations, so
 * the row sums are recomputed on the device).  PHK_ERR_UNSUPPORTED, and no batch, when a gathered row's sum is >= 2^32. */
int phk_batch_gather_columns(phk_ctx *ctx, const phk_batch *b, const uint32_t *table, phk_batch **out);
/* Folds the two strands of every row, IN PLACE: counts[r][c] += counts[r][rc(c)] for the resident rows of a batch from
 * any producer, and every stored row sum doubled.  rc(c) is the column of the reverse-complement k-mer: the k base-4
 * digits of c in reverse order with the digits paired 0 <-> 1, 2 <-> 3 -- A <-> T(U), G <-> C under the symbol orders
 * "ATGC" (DNA) and "AUGC" (RNA); a batch counted over another order is paired by digit all the same.  The result is what
 * counting every sequence and its reverse complement gives, characters outside the symbols included, so a sequence and
 * its reverse complement fold to the same row.  Palindromic k-mers (rc(c) == c, 4^(k/2) of them at even k) are doubled.
 * The batch remembers that it is folded (phk_batch_strands; phk_batch_select and phk_batch_gather_columns hand the mark
 * on): a second fold is PHK_ERR_ARG and changes nothing.  Every row sum is checked on the device before anything is
 * written: with one of 2^31 or more the call returns PHK_ERR_UNSUPPORTED (the text has the number of such rows) and the
 * batch is untouched; below that no entry can overflow either (an entry and its partner are both part of the row sum).
 * n == 0 is PHK_OK. */
int phk_batch_fold_strands(phk_ctx *ctx, phk_batch *b);
/* *folded = 1 when the rows of the batch are folded (phk_batch_fold_strands), else 0 */
int phk_batch_strands(const phk_batch *b, int *folded);
/* *rows = the rows one launch of the fold kernel at this k takes in a single pass of its grid (more are taken by its
 * grid-stride loop): what a test has to exceed to reach that loop. */
int phk_fold_grid_pass(int k, uint64_t *rows);
/* phamer_scorer.score_points (scripts/phamer.py:177-195) on a batch: scores[n] float64 to the host.  PHK_ERR_NAN
 * when a row has no counted window (the reference's NaN row makes scikit-learn raise). */
int phk_batch_score(phk_ctx *ctx, const phk_model *model, const phk_batch *b, int method, double *scores);
int phk_batch_free(phk_ctx *ctx, phk_batch *b);

/* ---- scoring model ----------------------------------------------------------------- */
/* The training side of phamer_scorer.score_points (scripts/phamer.py:177-195): positive /
 * negative reference rows (float64, normalised, row-major [n][D]); train = vstack(pos, neg),
 * labels = 1 for pos rows, 0 for neg rows (scripts/phamer.py:186-187).  cpos / cneg are the
 * k-means centroids of the two classes (scripts/phamer.py:245-248, learning.get_centroids
 * scripts/learning.py:69-81) and may be NULL / 0 when only PHK_METHOD_KNN will be used.
 * kn = k_neighbors (scripts/phamer.py:79, default 3).  All pointers are HOST pointers; the
 * model keeps device copies. */
int phk_model_create(phk_ctx *ctx, const double *pos, uint64_t n_pos, const double *neg,
                     uint64_t n_neg, const double *cpos, uint64_t n_cpos, const double *cneg,
                     uint64_t n_cneg, uint64_t D, int kn, phk_model **out);
int phk_model_destroy(phk_ctx *ctx, phk_model *model);
/* Cross-validation service (cross_validator.cross_validate, scripts/cross_validate.py:57-101: N folds whose train
 * sets share (N-1)/N of the rows): ONE model holds every reference row; a fold is a column mask over its train rows
 * (mask[n_pos + n_neg] host bytes in vstack(pos, neg) order, non-zero = held out, excluded from the k-NN search;
 * NULL lifts the mask) plus that fold's centroids (same counts as at creation).  Scores then equal those of a model
 * built from the unmasked rows alone: the search is translation invariant, so keeping the full matrix's centring
 * vector changes nothing but the error bounds, which are evaluated for it.
 * phk_model_set_centroids, phk_model_set_column_mask and phk_model_set_bandwidths may come in any order and any number
 * of times (a mask replaces the previous one): every method then scores as a model built from the current unmasked rows
 * with the current centroids and bandwidths.  A mask that leaves a class without rows is accepted (it must leave at least
 * kn rows); the density method then returns PHK_ERR_ARG.  The svm fit is a snapshot: phk_model_fit_svm fits the rows
 * unmasked at the time of the call, and a later mask or centroid change leaves it as it is until the next fit. */
int phk_model_set_centroids(phk_ctx *ctx, phk_model *model, const double *cpos, uint64_t n_cpos, const double *cneg,
                            uint64_t n_cneg);
int phk_model_set_column_mask(phk_ctx *ctx, phk_model *model, const uint8_t *mask);
/* Bandwidths of the density method (phamer_scorer.positive_bandwidth / negative_bandwidth, scripts/phamer.py:82-83): the
 * Gaussian kernel widths of the positive and the negative class.  A model starts with the reference's 0.005 / 0.01.  Each must
 * be finite and > 0, else PHK_ERR_ARG (model unchanged). */
int phk_model_set_bandwidths(phk_ctx *ctx, phk_model *model, double h_pos, double h_neg);
/* Fits the svm method (phamer_scorer.svm_score_points, scripts/phamer.py:258-266: NuSVC().fit(train, labels)) on the
 * model's train rows that the column mask leaves in: Nu-SVC with an RBF kernel of width gamma (> 0; scikit-learn's 'scale'
 * is 1 / (D var(X)) over those rows, computed by the caller), nu in (0, 1], stopping tolerance tol -- see phk_nusvc_fit.
 * The support vectors are copied into the model; a later mask does not change them.  PHK_ERR_ARG for an infeasible nu, a
 * class without rows, a bad argument or a fit whose coefficients are not finite (the previous fit is then kept). */
int phk_model_fit_svm(phk_ctx *ctx, phk_model *model, double nu, double gamma, double tol);

/* Deterministic device k-means (opt-in alternative to the scikit-learn fit of scripts/learning.py:131-146,
 * whose centroids depend on the scikit-learn version): k-means++ seeding driven by splitmix64(seed + j),
 * Lloyd sweeps in float64 with index-ordered sums (bit-reproducible), empty clusters re-seeded with the
 * farthest point; stops when no label changes or after max_iter sweeps.  X[n][D] host float64 ->
 * centroids[k][D], labels[n] (may be NULL), number of sweeps (may be NULL).  Cluster c's centroid is the
 * mean of the points labelled c, as learning.get_centroids computes it (scripts/learning.py:69-81). */
int phk_kmeans(phk_ctx *ctx, const double *X, uint64_t n, uint64_t D, uint32_t k, uint64_t seed, int max_iter,
               double *centroids, uint32_t *labels, int *n_iter);
/* The Lloyd iteration of scikit-learn's KMeans.fit (scripts/learning.py:138; _kmeans_single_lloyd) on the device, from
 * GIVEN initial centres: E-step (float64 direct differences, ties to the lower centre), M-step, stop when no label changed
 * or when the summed squared centre shift is <= tol (scikit-learn: 1e-4 x the mean per-feature variance), in which case
 * one more E-step makes the labels match the final centres.  With the host-side k-means++ seeding of scikit-learn
 * (kmeans_plusplus on the mean-centred rows, RandomState(10): phamers_amd/learning.py) the labels -- and so the reference's
 * per-label means, learning.get_centroids -- equal those of KMeans(n_clusters=k, random_state=10).fit(X).
 * X[n][D], init[k][D] host float64 -> labels[n]; centres (may be NULL); sweeps; number of empty clusters met (scikit-learn
 * relocates an empty cluster, this entry does not: a caller that sees n_empty != 0 must use the host fit).
 * min_gap (may be NULL): the closest call any E-step made, min over points and sweeps of (d2_second - d2_best) / d2_second.
 * scikit-learn forms its distances as -2 x.c + |c|^2 in chunked matrix products, this entry by direct differences: the two
 * agree to ~1e-13 relative, so a label can differ only where min_gap is of that order -- the facade takes the host fit
 * below 1e-9 (phamers_amd/learning.py). */
int phk_kmeans_lloyd(phk_ctx *ctx, const double *X, uint64_t n, uint64_t D, uint32_t k, const double *init, double tol,
                     int max_iter, double *centres, uint32_t *labels, int *n_iter, int *n_empty, double *min_gap);

/* ---- host API: scoring ------------------------------------------------------------- */
/* phamer.score_points / phamer_scorer.score_points (scripts/phamer.py:451-468, 177-195) for
 * method in {knn, kmeans, combo, density, svm}: Q[N][D] float64 host rows -> scores[N] float64.
 *   knn    : 2*(majority label of the kn nearest train rows) - 1   (scripts/learning.py:118-128)
 *   kmeans : tanh((e- - e+)/(e+ + e-)), e+/- = distance to the nearest positive / negative
 *            centroid (scripts/phamer.py:198-210, 250-256; scripts/learning.py:47-66)
 *   combo  : knn + kmeans (scripts/phamer.py:303-313)
 *   density: L+ - L-, L = the Gaussian kernel density log-likelihood of the query under one class's unmasked train rows,
 *            bandwidth h+ / h- (phk_model_set_bandwidths): phamer_scorer.density_score_points (scripts/phamer.py:275-287),
 *            learning.get_density (scripts/learning.py:107-115).  float64 throughout; the result of a query does not depend
 *            on N, on the batch it came in or on the entry point.  PHK_ERR_ARG when a class has no unmasked row.
 *   svm    : 1.0 where libsvm's decision value sum_sv coef_sv exp(-gamma |q - x_sv|^2) - rho is <= 0, else 0.0: the
 *            predict of the NuSVC fitted by phk_model_fit_svm (scripts/phamer.py:258-266).  float64; the result of a query
 *            does not depend on N, the batch or the entry point.  PHK_ERR_ARG before a fit.
 * Returns PHK_ERR_NAN (scores untouched) if any query element is NaN -- the reference's
 * scikit-learn call raises on such input. */
int phk_score(phk_ctx *ctx, const phk_model *model, const double *Q, uint64_t N, int method,
              double *scores);

/* scikit-learn NuSVC(nu, kernel='rbf', gamma, tol, shrinking=False, max_iter).fit(X, labels) for labels in {0, 1}
 * (phamer_scorer.svm_score_points, scripts/phamer.py:258-266), as scikit-learn's libsvm fork solves it (svm.cpp
 * solve_nu_svc, Solver_NU; shrinking does not change the solution): the kernel matrix on the device, rounded to float32 as
 * libsvm's Qfloat, the solver in one workgroup.  X[n][D], labels[n] host arrays; gamma > 0 (scikit-learn's 'scale' /
 * 'auto' are computed by the caller); max_iter -1 = unlimited.  Out (host, capacity n): support[n_sv] = the rows of X that
 * are support vectors, in libsvm's order (label-0 rows first); dual_coef[n_sv] = libsvm's coefficients alpha_i y_i / r
 * with y = +1 for label 0 (scikit-learn's binary dual_coef_ is their negation); *rho = libsvm's rho (scikit-learn's binary
 * intercept_); *n_iter = solver iterations.  PHK_ERR_ARG for labels outside {0, 1}, a single class, an infeasible nu
 * (svm_check_parameter, svm.cpp:3129: nu (n0 + n1) / 2 > min(n0, n1)), nu outside (0, 1], more than 65536 rows, or
 * support-vector coefficients or rho that are not finite (r = 0; scikit-learn's fit raises there too). */
int phk_nusvc_fit(phk_ctx *ctx, const double *X, uint64_t n, uint64_t D, const double *labels, double nu, double gamma,
                  double tol, int32_t max_iter, int32_t *support, double *dual_coef, double *rho, int32_t *n_sv,
                  int32_t *n_iter);
/* libsvm's decision values (svm_predict_values, k_function of svm.cpp:452) of Q[N][D] under support vectors SV[n_sv][D]
 * with libsvm's coefficients and rho: dec[q] = sum_sv dual_coef_sv exp(-gamma |Q[q] - SV_sv|^2) - rho, float64, on the
 * MFMA Gram tile; the value of a query does not depend on N.  Host pointers.  scikit-learn's binary decision_function is
 * -dec; its predict is 1 (classes_[1]) where dec <= 0. */
int phk_nusvc_decision(phk_ctx *ctx, const double *SV, uint64_t n_sv, uint64_t D, const double *dual_coef, double rho,
                       double gamma, const double *Q, uint64_t N, double *dec);

/* phk_nusvc_fit over a grid gamma x nu x row subset, and phk_nusvc_decision of every fold's held-out rows: the fits behind a
 * choice of the svm method's nu and gamma.  Subset 0 is all rows; subset f + 1 (f < F) the rows whose fold_of is not f.
 * Problem (g, v, s) has index (g V + v)(F + 1) + s; it is solved in a workgroup of its own from one kernel matrix per gamma,
 * bit for bit as phk_nusvc_fit solves the rows of the subset (in their order) at gammas[g], nus[v], tol, max_iter.
 * X[n][D], labels[n] in {0, 1}, gammas[Gm], nus[V] host arrays; fold_of[n] int32 in [0, F), or F = 0 (fold_of and held_dec
 * may be NULL) for full fits only.  Out (host), per problem q: status[q] -- PHK_SVM_OK; PHK_SVM_INFEASIBLE: a class of the
 * subset has no rows or nu (n0 + n1) / 2 > min(n0, n1) on it, decided before any launch; PHK_SVM_NOT_FINITE: coefficients
 * or rho that are not finite (r = 0), where phk_nusvc_fit returns PHK_ERR_ARG -- n_iter[q], and for PHK_SVM_OK n_sv[q],
 * rho[q] (libsvm's; NaN otherwise) and coef[q][n]: libsvm's coefficients alpha_i y_i / r in the caller's row order, 0 off the
 * support (all 0 otherwise).  Per cell c = g V + v: held_dec[c][i] = libsvm's decision value of row i under the fit of
 * subset fold_of[i] + 1 of that cell, the bits phk_nusvc_decision gives for that model and row; NaN where that fit has
 * another status.  Private arguments (tests; no result depends on them): lds_rows -- the solver keeps alpha, G and y in LDS
 * when n is at most min(lds_rows, phk_nusvc_sweep_lds_rows()), in global memory otherwise; -1 = the device's capacity, 0 =
 * never; gammas_per_pass -- kernel matrices resident at a time, 0 = as many as 4 GiB hold; threads -- the solver's workgroup
 * size, a multiple of 64 up to 1024, 0 = chosen from n.  PHK_ERR_ARG for an empty axis, nu outside (0, 1], a gamma or tol
 * that is not finite and > 0, fold ids outside [0, F), labels outside {0, 1}, more than 65536 rows; PHK_ERR_NAN for NaN
 * rows.  No infeasible or non-finite problem is an error, and none disturbs another problem. */
#define PHK_SVM_OK 0
#define PHK_SVM_INFEASIBLE 1
#define PHK_SVM_NOT_FINITE 2
int phk_nusvc_sweep(phk_ctx *ctx, const double *X, uint64_t n, uint64_t D, const double *labels, const double *gammas,
                    uint32_t Gm, const double *nus, uint32_t V, const int32_t *fold_of, uint32_t F, double tol,
                    int32_t max_iter, int64_t lds_rows, uint32_t gammas_per_pass, uint32_t threads, int32_t *status,
                    int32_t *n_iter, int32_t *n_sv, double *rho, double *coef, double *held_dec);
/* rows whose solver state (17 bytes each) fits the LDS a workgroup of phk_nusvc_sweep may declare */
uint32_t phk_nusvc_sweep_lds_rows(void);

/* KernelDensity(kernel='gaussian', bandwidth=h).fit(X).score_samples(Q) (learning.get_density, scripts/learning.py:107-115):
 * out[q] = logsumexp_j(-|Q[q] - X[j]|^2 / (2 h^2)) - log(M) - (D/2) log(2 pi) - D log(h), float64, the density method's
 * kernel over one data set.  Host pointers.  h must be finite and > 0 (else PHK_ERR_ARG); a NaN query row gives PHK_ERR_NAN. */
int phk_kde_log_density(phk_ctx *ctx, const double *Q, uint64_t N, const double *X, uint64_t M, uint64_t D, double h,
                        double *out);

/* phk_kde_log_density at B bandwidths from one pass over the pairs: out[b][q] (out[B][N]) is bit for bit what
 * phk_kde_log_density(..., h[b], ...) writes to out[q].  Q and X go up once; a pass of the device carries up to
 * PHK_KDE_SWEEP_PER_PASS bandwidths through one Gram tile, more bandwidths run as further passes over the resident rows.
 * exclude_self != 0: N == M, query q is taken to be row q of X and the pair (q, q) is left out -- by index, an equal row
 * elsewhere still counts -- and the normaliser is log(M - 1): the leave-one-out density.  M == 1 is then PHK_ERR_ARG.
 * batch_rows: queries per device batch, 0 = the default (for tests; the result does not depend on it).  Host pointers.
 * Every h[b] must be finite and > 0 and B >= 1 (else PHK_ERR_ARG); a NaN query row gives PHK_ERR_NAN; N == 0 is PHK_OK. */
#define PHK_KDE_SWEEP_PER_PASS 8
int phk_kde_sweep(phk_ctx *ctx, const double *Q, uint64_t N, const double *X, uint64_t M, uint64_t D, const double *h,
                  uint32_t B, int exclude_self, uint64_t batch_rows, double *out);

/* ---- multinomial likelihood scoring (this project's own method) ------------------------------------
 * A contig is scored from its integer count row c (D bins) by the log-likelihood ratio of two mixtures of multinomials,
 * one component per reference row r with the smoothed profile p_r[j] = (x_r[j] + a) / (sum_j x_r[j] + D a):
 *     S[q, r]  = sum_j c_q[j] log p_r[j]
 *     l_C(q)   = logsumexp_{r in class C, not excluded for q} S[q, r] - log n_eff(q, C)
 *     score(q) = l_+(q) - l_-(q)              (nats; >= 0 reads as phage)
 * n_eff(q, C) = the rows of class C that are not excluded for q.  Row r is excluded for query q when both carry a group id
 * >= 0 and the two are equal (cross-validation: the group is the fold).  Everything is float64; the result of a query is a
 * function of its count row, its group and the table alone -- not of N, the batch split or the entry point.
 *
 * phk_lik_table_create: a resident table from the two HOST log tables log_pos[n_pos][D], log_neg[n_neg][D] (the values
 * log p_r[j]; the library never takes a logarithm of a profile) with optional group ids groups_pos[n_pos] / groups_neg[n_neg]
 * (NULL = none; a negative id = no group).  n_neg == 0 (log_neg NULL) makes a one-class table: l_- = 0, score = l_+.
 * PHK_ERR_NAN when a table entry is not finite; PHK_ERR_ARG for an empty positive table or D == 0. */
typedef struct phk_lik_table phk_lik_table;
int phk_lik_table_create(phk_ctx *ctx, const double *log_pos, uint64_t n_pos, const int32_t *groups_pos,
                         const double *log_neg, uint64_t n_neg, const int32_t *groups_neg, uint64_t D, phk_lik_table **out);
int phk_lik_table_destroy(phk_ctx *ctx, phk_lik_table *table);
/* score(q) of the formula above for the HOST count rows counts[N][D] (uint32), with optional group ids query_groups[N]
 * (NULL = none; they exclude rows only when the table has group ids too).  l_pos[N], l_neg[N] (either may be NULL) and
 * scores[N], float64, to the host.  batch_rows: queries per device batch, 0 = the default (for tests; no result depends on
 * it).  PHK_ERR_ARG, before any launch, when some query's n_eff is 0 in a class, or D is not the table's.  A row without
 * counts scores exactly 0: every S is 0 and both class terms are log 1.  N == 0 is PHK_OK. */
int phk_lik_score(phk_ctx *ctx, const phk_lik_table *table, const uint32_t *counts, uint64_t N, uint64_t D,
                  const int32_t *query_groups, uint64_t batch_rows, double *l_pos, double *l_neg, double *scores);
/* The same for the resident rows of a batch, read in place (folded rows when phk_batch_fold_strands has run -- the table
 * should then come from folded reference counts); no groups. */
int phk_batch_lik_score(phk_ctx *ctx, const phk_lik_table *table, const phk_batch *b, double *l_pos, double *l_neg,
                        double *scores);

/* ---- likelihood-ranked reference lookup (this project's own) ----------------------------------------
 * The first `top` rows of a HOST log table L[M][D] for every uint32 count row c, in order of (S descending, row index
 * ascending), S[q, r] = sum_j c_q[j] L[r, j] in float64 as the likelihood scorer's Gram tile gives it -- the bits of a
 * result do not depend on N, the batch split, the entry point or the run.  The library does not know what the table holds:
 * the multinomial log profiles of likelihood.py or the Markov log transition table of hosts.py.  With group ids on both sides
 * a row is skipped for a query when both ids are >= 0 and equal.
 *
 * phk_host_table_create: a resident table with optional group ids groups[M] (NULL = none; a negative id = no group).
 * PHK_ERR_NAN when a table entry is not finite; PHK_ERR_ARG for an empty table. */
#define PHK_HOSTS_MAX_TOP 16
typedef struct phk_host_table phk_host_table;
int phk_host_table_create(phk_ctx *ctx, const double *log_table, uint64_t M, uint64_t D, const int32_t *groups,
                          phk_host_table **out);
int phk_host_table_destroy(phk_ctx *ctx, phk_host_table *table);
/* idx[N][top] (int32) and s[N][top] (float64, nats) to the host for the HOST count rows counts[N][D], with optional group
 * ids query_groups[N].  batch_rows: queries per device batch, 0 = the default (for tests; no result depends on it).
 * PHK_ERR_ARG, before any launch, when top is not in 1..PHK_HOSTS_MAX_TOP or exceeds the rows some query has left.  A row
 * without counts gets rows 0..top-1 (of those it has left) with S = 0.  N == 0 is PHK_OK. */
int phk_host_rank(phk_ctx *ctx, const phk_host_table *table, const uint32_t *counts, uint64_t N, uint64_t D,
                  const int32_t *query_groups, int top, uint64_t batch_rows, int32_t *idx, double *s);
/* The same for the resident rows of a batch, read in place (folded rows when phk_batch_fold_strands has run); no groups. */
int phk_batch_host_rank(phk_ctx *ctx, const phk_host_table *table, const phk_batch *b, int top, int32_t *idx, double *s);
/* The null of the z-score: mu[M] and sigma[M] (sample standard deviation, ddof = 1) of l[p, r] = S[p, r] / n_p over the
 * HOST null count rows counts[P][D], n_p the row's total.  Two passes over the product, every column accumulated in row
 * order 0..P-1: no bit depends on batch_rows (0 = the default).  PHK_ERR_ARG for P < 2 or a null row without counts. */
int phk_host_null_fit(phk_ctx *ctx, const phk_host_table *table, const uint32_t *counts, uint64_t P, uint64_t D,
                      uint64_t batch_rows, double *mu, double *sigma);

/* ---- track segmentation: a two-state hidden Markov decode (this project's own) ----------------------
 * Per record r, over its windows t = offsets[r] .. offsets[r + 1] - 1 of the flat evidence x[n] (nats; a tempered
 * log-likelihood ratio): states 0 = host, 1 = phage, emission e_t = (1, exp(x_t)), transition trans = {A00, A01, A10, A11},
 * initial distribution init.  Host pointers.  The library never takes a logarithm of a parameter: the caller passes the
 * probabilities and their logarithms quantised to int64 units of 2^-PHK_SEG_QUANT_BITS nat (qlog_trans, qlog_init).
 *   posterior[n]   P(state_t = 1 | all x of the record), float64: forward-backward in the probability domain, sums of
 *                  products of positive numbers rescaled by powers of two only -- no cancellation; error bound in
 *                  tests/segment_ref.py.  exp(x_t) enters as exp(-|x_t|) on the disfavoured state: no |x_t| overflows, and an
 *                  underflow to 0 reads as "certain".
 *   state[n]       the Viterbi path, uint8: the plain left-to-right max-plus recurrence on exact integers -- x_t is
 *                  quantised to rint(clamp(x_t, -2^15, 2^15) 2^PHK_SEG_QUANT_BITS), so |x_t| beyond 2^15 nats counts as 2^15 --
 *                  ties to the predecessor with the smaller state, a tie at the final step to the smaller state.  With at most
 *                  2^31 windows per call no sum leaves int64.
 *   log_odds[R]    log sum_paths P(path, x): the log evidence against the all-host chain, float64
 *   path_score[R]  the Viterbi path's integer score (x 2^-PHK_SEG_QUANT_BITS = nats)
 * A record is cut into tiles of PHK_SEG_TILE windows from its own start and the tiles are carried in tile order: the result
 * of a record is a function of its x and the parameters alone -- not of the other records, its place among them, or the
 * launch.  PHK_ERR_ARG, before any launch, for a parameter outside (0, 1), a row of trans or init that does not sum to 1
 * within 4 ulp, offsets that do not run non-decreasing from 0 to n, n > 2^31; PHK_ERR_NAN for an x that is not finite.
 * R == 0 or n == 0 is PHK_OK; a record without windows gets log_odds 0 and path_score 0. */
#define PHK_SEG_TILE 64
#define PHK_SEG_QUANT_BITS 16
int phk_segment_decode(phk_ctx *ctx, const double *x, uint64_t n, const uint64_t *offsets, uint64_t R, const double trans[4],
                       const double init[2], const int64_t qlog_trans[4], const int64_t qlog_init[2], double *posterior,
                       uint8_t *state, double *log_odds, int64_t *path_score);
/* tiles one launch of the per-tile kernels covers; beyond it they stride (for tests) */
uint64_t phk_segment_grid_pass(void);

/* ---- fitting the chain's transition probabilities: Baum-Welch (this project's own) ------------------
 * phk_segment_expect is one E-step of the chain above at (trans, init): per record
 *   counts_rec[R][6]  xi(0->0), xi(0->1), xi(1->0), xi(1->1), gamma_0(0), gamma_0(1), with
 *                     xi(i->j) = sum_{t >= 1} P(s_{t-1} = i, s_t = j | x) and gamma_0(s) = P(s_0 = s | x); may be NULL
 *   log_odds[R]       bit for bit what phk_segment_decode returns; may be NULL
 * and over the records totals[6] (the column sums of counts_rec) and *log_evidence (the sum of log_odds): up to a term
 * that depends on no parameter, the log-likelihood of the tracks.  Every step's four terms alpha_{t-1}(i) A_ij e_t(j)
 * beta_t(j) are normalised by their own sum and added in step order, tile partials in tile order: a record's row is a
 * function of its x and the parameters alone.  The sums over records follow a tree fixed by the record index: blocks of 256
 * consecutive rows (a row past the end counts as +0.0), within a block v[i] += v[i + s] for s = 128, 64, .. 1, and the block
 * results reduced by the same rule until one is left -- a function of (R, the per-record values), not of the launch.  Error
 * bound: tests/segment_fit_ref.py.  Argument checks and error codes are phk_segment_decode's.  R == 0 or n == 0 is PHK_OK
 * with zeros; a record without windows contributes nothing, a record of one window only its gamma_0. */
int phk_segment_expect(phk_ctx *ctx, const double *x, uint64_t n, const uint64_t *offsets, uint64_t R, const double trans[4],
                       const double init[2], double *counts_rec, double totals[6], double *log_odds, double *log_evidence);

/* phk_segment_fit iterates E-step and M-step from start = {a, b, p_start} (a = A01, b = A10).  x, the offsets and the tile
 * lists go to the device once; an iteration brings back the six totals and the log evidence.  The M-step, in float64 and in
 * this order of operations, with c = prior_counts = {c00, c01, c10, c11} (finite, >= 0) and N, G the totals:
 *   a = (N01 + c01) / ((N00 + c00) + (N01 + c01)),  b = (N10 + c10) / ((N10 + c10) + (N11 + c11)),
 *   each clamped to [1e-12, 1 - 1e-12] (PHK_SEG_FIT_CLAMPED); a row whose denominator is 0 keeps its parameter
 *   (PHK_SEG_FIT_NO_TRANSITIONS);  trans = {1 - a, a, b, 1 - b}, init = {1 - p_start, p_start};
 *   p_start: PHK_SEG_START_FIXED kept; PHK_SEG_START_FREE G1 / (G0 + G1), clamped (kept when G0 + G1 = 0);
 *   PHK_SEG_START_STATIONARY a / (a + b) of the new a and b, clamped -- for the start parameters too: start[2] is not read.
 * trace[(max_iter + 1)][PHK_SEG_TRACE_COLS]: row i = a, b, p_start of iterate i, the six totals and the log evidence L_i AT
 * those parameters; rows 0 .. *n_iter are written (and possibly one more, to be ignored).  The loop stops when
 * L_i - L_{i-1} <= tol max(1, |L_i|) (PHK_SEG_FIT_CONVERGED) or after max_iter M-steps.  Fixed and free starts are exact EM
 * for prior_counts = 0: L never falls but by rounding.  The stationary start is a generalised step that may lower L: the loop
 * stops there too, and the result is the iterate before it.  fitted = row *n_iter's parameters, the largest L of the trace.
 * tol finite and >= 0, max_iter <= PHK_SEG_FIT_MAX_ITER, else PHK_ERR_ARG; the other checks as phk_segment_expect at the start
 * parameters.  The tempering of the evidence is not fitted: the evidence grows without bound in it. */
#define PHK_SEG_TRACE_COLS 10
#define PHK_SEG_FIT_MAX_ITER 100000u
#define PHK_SEG_START_FIXED 0
#define PHK_SEG_START_FREE 1
#define PHK_SEG_START_STATIONARY 2
#define PHK_SEG_FIT_CONVERGED 1u
#define PHK_SEG_FIT_CLAMPED 2u
#define PHK_SEG_FIT_NO_TRANSITIONS 4u
int phk_segment_fit(phk_ctx *ctx, const double *x, uint64_t n, const uint64_t *offsets, uint64_t R, const double start[3],
                    int start_mode, const double prior_counts[4], uint32_t max_iter, double tol, double *trace,
                    uint32_t *n_iter, uint32_t *status, double fitted[3]);

/* ---- mixtures of multinomials on count rows: the E-step (this project's own) -------------------------
 * K components with HOST log profiles log_profiles[K][D] and log weights log_weights[K] (the library takes no logarithm of a
 * profile or of a weight), uint32 count rows c_i:
 *     S[i, k] = sum_j c_i[j] log_profiles[k][j] + log_weights[k]      l_i = logsumexp_k S[i, k]      r[i, k] = exp(S[i, k] - l_i)
 *     T[k][j] = sum_i r[i, k] c_i[j]        Nk[k] = sum_i r[i, k]        L = sum_i l_i
 * A log weight of -inf (weight 0) leaves its component out of every row: r = 0, its T row and Nk are exactly 0.  Everything
 * is float64.  T, Nk and L are reduced in blocks of phk_mix_block_rows() rows anchored at the global row index, the blocks by
 * the fixed tree of phk_segment_expect: they are a function of (rows, table) alone -- the same bits for any batch_rows, from
 * host counts or a resident batch, run to run.
 *
 * phk_mix_table_create / _update: 1 <= K <= 256 and D >= 1, else PHK_ERR_ARG; a profile entry that is not finite, or a log
 * weight that is NaN or +inf, is PHK_ERR_NAN; every weight 0 is PHK_ERR_ARG.  _update replaces the values of a table of the
 * same shape (an EM iteration). */
typedef struct phk_mix_table phk_mix_table;
int phk_mix_table_create(phk_ctx *ctx, const double *log_profiles, const double *log_weights, uint64_t K, uint64_t D,
                         phk_mix_table **out);
int phk_mix_table_update(phk_ctx *ctx, phk_mix_table *table, const double *log_profiles, const double *log_weights, uint64_t K,
                         uint64_t D);
int phk_mix_table_destroy(phk_ctx *ctx, phk_mix_table *table);
uint64_t phk_mix_block_rows(void);
/* One E-step over the HOST count rows counts[N][D]: T[K][D], Nk[K], L[1] and, where asked for (NULL = not), per row l_i
 * (row_ll[N]), the component of the largest r (argmax[N], lowest index on ties) and that r (max_resp[N]).  The N x K matrix
 * stays on the device.  batch_rows: rows per device batch, 0 = the default (for tests; no result depends on it).
 * PHK_ERR_ARG when D is not the table's; N == 0 is PHK_OK with zeros. */
int phk_mix_expect(phk_ctx *ctx, const phk_mix_table *table, const uint32_t *counts, uint64_t N, uint64_t D,
                   uint64_t batch_rows, double *T, double *Nk, double *L, double *row_ll, int32_t *argmax, double *max_resp);
/* The same for the resident rows of a batch, read in place. */
int phk_batch_mix_expect(phk_ctx *ctx, const phk_mix_table *table, const phk_batch *b, uint64_t batch_rows, double *T,
                         double *Nk, double *L, double *row_ll, int32_t *argmax, double *max_resp);
/* r itself, resp[N][K], to the host (and row_ll[N] unless NULL): for the caller who asks for it; no fit does. */
int phk_mix_responsibilities(phk_ctx *ctx, const phk_mix_table *table, const uint32_t *counts, uint64_t N, uint64_t D,
                             uint64_t batch_rows, double *resp, double *row_ll);
int phk_batch_mix_responsibilities(phk_ctx *ctx, const phk_mix_table *table, const phk_batch *b, uint64_t batch_rows,
                                   double *resp, double *row_ll);

/* ---- many mixture E-steps in one call ---------------------------------------------------------------
 * A sweep object keeps count rows [N][D] (uploaded from the host, or a resident batch's rows, read where they lie: the batch
 * must outlive the sweep) and n_sets row sets: set s is the strictly ascending row indices set_rows[set_offsets[s] ..
 * set_offsets[s + 1]), gathered once into rows of its own (a set of all N rows is the source itself).  PHK_ERR_ARG for an empty
 * set, an index >= N or not ascending, N == 0 or N >= 2^32.
 *
 * phk_mix_sweep_step runs n_jobs jobs; job j is (row set job_set[j], K_j = job_K[j] components, 1 <= K_j <= 256).  The jobs'
 * log profiles [K_j][D] lie one after another in log_profiles, their log weights [K_j] one after another in log_weights.
 * expect != 0: out receives per job T[K_j][D], Nk[K_j] and L (K_j D + K_j + 1 doubles), job after job.  rows != 0: after
 * those (or, with expect == 0, alone) the row log-likelihoods l_i of every job's set, job after job.  Every job's values are
 * the bits phk_mix_expect returns for that job's rows and table alone: the jobs are processed in groups whose device buffers
 * stay within budget_bytes (0 = the default; a job larger than the budget forms a group of its own) and no result depends
 * on the grouping, the order of the jobs or the other jobs of the call.  Two launches and the fold levels per group.
 * n_jobs == 0 is PHK_OK with nothing launched.  PHK_ERR_NAN, naming the job, for a profile entry that is not finite or a log
 * weight that is NaN or +inf; PHK_ERR_ARG for a job whose weights are all 0. */
typedef struct phk_mix_sweep phk_mix_sweep;
int phk_mix_sweep_create(phk_ctx *ctx, const uint32_t *counts, uint64_t N, uint64_t D, const uint32_t *set_rows,
                         const uint64_t *set_offsets, uint64_t n_sets, phk_mix_sweep **out);
int phk_batch_mix_sweep_create(phk_ctx *ctx, const phk_batch *b, const uint32_t *set_rows, const uint64_t *set_offsets,
                               uint64_t n_sets, phk_mix_sweep **out);
int phk_mix_sweep_step(phk_ctx *ctx, const phk_mix_sweep *sweep, const uint32_t *job_set, const uint32_t *job_K,
                       uint64_t n_jobs, const double *log_profiles, const double *log_weights, int expect, int rows,
                       uint64_t budget_bytes, double *out);
int phk_mix_sweep_destroy(phk_ctx *ctx, phk_mix_sweep *sweep);

/* ---- S-state chain over the count rows of windows (chain.hip) ---------------------------------------
 * Records r have windows t = offsets[r] .. offsets[r + 1] - 1 (offsets[R + 1], non-decreasing from 0 to n) with uint32 count
 * rows [n][D]; S states, 2 <= S <= PHK_CHAIN_MAX_STATES.  A chain keeps the rows (uploaded once by phk_chain_create, or a
 * resident batch's rows read where they lie: the batch must outlive the chain), the offsets and every device buffer of its
 * calls.  phk_chain_create_from_emissions takes host emissions E[n][S] instead of rows: a general S-state decoder.
 *
 * phk_chain_set(log_profiles[S][D], trans[S][S], init[S], qlog_trans, qlog_init, temper) forms on the device
 *     E[t][s] = temper * sum_j c_t[j] log_profiles[s][j]       float64 on the matrix pipe, one multiply by temper afterwards
 * (a chain made from emissions takes log_profiles == NULL and keeps its E; temper is checked and not used).  The logarithms are
 * the caller's; qlog_* are log trans and log init in int64 units of 2^-PHK_SEG_QUANT_BITS nat, each in [-2^31, 0].  With
 * d[t][s] = E[t][s] - max_s' E[t][s'] <= 0:
 *   phk_chain_emissions  E[n][S] to the host.
 *   phk_chain_expect     one E-step.  xi[S][S] = sum_t P(s_{t-1} = i, s_t = j | rows), each step's S^2 terms normalised by
 *                        their own sum and added in step order per record; gamma0[S]; *log_evidence; the three summed over the
 *                        records by the fixed 256-row tree of phk_segment_expect; log_evidence_rec[R] unless NULL.
 *                        T[S][D] = sum_t gamma_t(s) c_t[j] and Ns[S] = sum_t gamma_t(s), reduced in blocks of
 *                        phk_mix_block_rows() rows anchored at the global row index and that tree (both NULL: not computed;
 *                        a chain made from emissions has none).  The posteriors and E stay on the device.
 *   phk_chain_decode     state[n] uint8: the path of the plain left-to-right max-plus recurrence on exact integers over
 *                        q[t][s] = rint(max(d[t][s], -2^15) 2^PHK_SEG_QUANT_BITS), ties to the smallest predecessor and, at the
 *                        end, to the smallest state; path_score[R] int64 unless NULL; posterior[n][S] and
 *                        log_evidence_rec[R] unless NULL (forward-backward in the probability domain on exp(d), rescaled by
 *                        powers of two; an exp that underflows to 0 reads as "certain").
 * Every result of a record is a function of its own rows and the parameters alone: the same bits for any batch_rows (rows per
 * device batch, 0 = the default), from host rows and from a batch, whatever the other records, the launch or the run.  At most
 * 2^30 windows per chain: with |q| and |qlog| <= 2^31 every integer sum stays inside 2^62.
 * PHK_ERR_ARG, before any launch: S outside 2..8, bad offsets (create); a parameter outside (0, 1), a row of trans or init
 * that does not sum to 1 within 4 ulp, a qlog outside [-2^31, 0], D not the rows', temper not finite and > 0 (set); a call
 * before a successful set.  PHK_ERR_NAN: a profile entry (set) or a host emission (create) that is not finite.  n == 0 or
 * R == 0 is PHK_OK with zeros; a record without windows contributes nothing, a record of one window only its gamma0 and
 * evidence.  phk_chain_grid_pass(): the most records one launch of the per-record kernels covers (further ones by grid
 * stride; for the tests). */
#define PHK_CHAIN_MAX_STATES 8
typedef struct phk_chain phk_chain;
int phk_chain_create(phk_ctx *ctx, const uint32_t *counts, uint64_t n, uint64_t D, const uint64_t *offsets, uint64_t R,
                     uint32_t S, uint64_t batch_rows, phk_chain **out);
int phk_batch_chain_create(phk_ctx *ctx, const phk_batch *b, const uint64_t *offsets, uint64_t R, uint32_t S,
                           uint64_t batch_rows, phk_chain **out);
int phk_chain_create_from_emissions(phk_ctx *ctx, const double *E, uint64_t n, const uint64_t *offsets, uint64_t R, uint32_t S,
                                    phk_chain **out);
int phk_chain_set(phk_ctx *ctx, phk_chain *chain, const double *log_profiles, uint64_t D, const double *trans,
                  const double *init, const int64_t *qlog_trans, const int64_t *qlog_init, double temper);
int phk_chain_emissions(phk_ctx *ctx, const phk_chain *chain, double *E);
int phk_chain_expect(phk_ctx *ctx, const phk_chain *chain, double *T, double *Ns, double *xi, double *gamma0,
                     double *log_evidence, double *log_evidence_rec);
int phk_chain_decode(phk_ctx *ctx, const phk_chain *chain, uint8_t *state, double *posterior, double *log_evidence_rec,
                     int64_t *path_score);
uint64_t phk_chain_grid_pass(void);
int phk_chain_destroy(phk_ctx *ctx, phk_chain *chain);

/* The tile scan of the chain: an opt-in route on which a long record is worked on in parallel.
 * phk_chain_set_scan(chain, scan_from): in every later phk_chain_expect and phk_chain_decode the records of at least scan_from
 * windows are cut into tiles of PHK_CHAIN_TILE consecutive windows counted from the record's own start (the last may be
 * partial); 0, the state after create, means no record.  A tile's transfer matrices (the ordered product of its steps' A diag(e)
 * in float64 rescaled by powers of two, and of its max-plus steps on int64) are formed in parallel over the tiles, carried
 * through the record's tiles in tile order, and the tiles then run the per-step recurrences from the vectors that enter them.
 * state and path_score of a scanned record are bit for bit those of the other route (integer max-plus is associative); its
 * posteriors, xi, gamma0, evidence, T and Ns lie within the bound of section 4.27 of the exact values, and are a function of its
 * own rows, the parameters and PHK_CHAIN_TILE alone.  A record below scan_from gives the bits it gives with the route off.
 * The call may come before or after phk_chain_set; it builds the tile tables and allocates the tile buffers.  PHK_ERR_ARG for a
 * NULL chain; PHK_OK with nothing allocated when no record reaches scan_from.  phk_chain_tile() returns PHK_CHAIN_TILE,
 * phk_chain_scan_grid_pass() the most tiles one launch of the per-tile kernels covers (further ones by grid stride; for the
 * tests). */
#define PHK_CHAIN_TILE 64
int phk_chain_set_scan(phk_ctx *ctx, phk_chain *chain, uint64_t scan_from);
uint64_t phk_chain_tile(void);
uint64_t phk_chain_scan_grid_pass(void);

/* Grouped chains: one set of parameters per group of consecutive records, all groups in one call.
 * phk_chain_set_groups(chain, group_offsets[G + 1], G): group g holds the records group_offsets[g] .. group_offsets[g + 1] - 1
 * (from 0 to R, non-decreasing; a group without records or without windows is legal).  G = 0 with NULL offsets returns the
 * chain to one set of parameters (phk_chain_set comes next).  PHK_ERR_ARG for a chain made from emissions, for offsets that
 * do not run from 0 to R or decrease, and while the tile scan is asked for (phk_chain_set_scan with a threshold on a grouped
 * chain is PHK_ERR_ARG too).
 * phk_chain_set_grouped(log_profiles[G][S][D], D, trans[G][S][S], init[G][S], qlog_trans, qlog_init, temper, active[G] or
 * NULL = all): the parameters of every group, checked as phk_chain_set checks them (PHK_ERR_ARG / PHK_ERR_NAN before any
 * launch; the chain then waits for a successful set) for the active groups only: the parameters of an inactive group are
 * not read.  Forms the emissions of the active groups.
 * phk_chain_expect_grouped: one E-step of every group: T[G][S][D], Ns[G][S], xi[G][S][S], gamma0[G][S], log_evidence[G] and
 * (or NULL) log_evidence_rec[R].  phk_chain_decode and phk_chain_emissions work on a grouped chain: every record with its
 * group's parameters.  Every result of a group is bit for bit what a chain made from that group's records alone gives with
 * phk_chain_set / phk_chain_expect / phk_chain_decode: the expectation blocks are anchored at the group's first window and
 * both trees run over the group's own vectors.  An inactive group, and a group without windows, is passed over by every
 * kernel: its outputs are zeros (T, Ns, xi, gamma0, evidence, emissions, state, posterior, path score).  phk_chain_set and
 * phk_chain_expect on a grouped chain, and the grouped calls on a chain without groups, are PHK_ERR_ARG. */
int phk_chain_set_groups(phk_ctx *ctx, phk_chain *chain, const uint64_t *group_offsets, uint64_t G);
int phk_chain_set_grouped(phk_ctx *ctx, phk_chain *chain, const double *log_profiles, uint64_t D, const double *trans,
                          const double *init, const int64_t *qlog_trans, const int64_t *qlog_init, double temper,
                          const uint8_t *active);
int phk_chain_expect_grouped(phk_ctx *ctx, const phk_chain *chain, double *T, double *Ns, double *xi, double *gamma0,
                             double *log_evidence, double *log_evidence_rec);

/* Segment boundaries refined to the base.  The sequences are n_seq records of a packed stream
 * (bases, seq_offsets[n_seq + 1] as phk_count_ascii takes them); the k-mer starting at base i of a sequence of L bases is
 * valid when i + k <= L and its k bases are symbols -- the rule of the count kernels; it never runs into the next sequence --
 * and code(i) is its column in a count row.  qtable[n_rows][D], D = 4^k, int64 with |q| <= 2^31 (segment.quantise of log
 * profiles: units of 2^-PHK_SEG_QUANT_BITS nat).  Boundary b = (seq, lo, x, hi, left_row, right_row) with
 * 0 <= lo <= x <= hi <= L_seq and hi - lo <= 2^30:
 *     d(i) = q[left_row][code(i)] - q[right_row][code(i)] for a valid k-mer, 0 otherwise
 *     P(p) = sum_{lo <= i < p} d(i)                       p = lo .. hi
 *     position[b]    = the p that maximises P; ties to the smallest |p - x|, then to the smallest p
 *     evidence[b][0] = P(position) - P(x)    the gain over the window boundary
 *     evidence[b][1] = P(position) - P(lo)   evidence[b][2] = P(position) - P(hi)
 *     support[b]     = the valid k-mers starting in [lo, hi)
 * All integer, exact, inside 2^63; a boundary's result is a function of its own sequence's bases in [lo, hi + k - 1), its two
 * rows, lo, x and hi alone: not of the other boundaries, their order or number, the launch or the run.  The bases go up once
 * and are packed by the packer of the count path; _fasta takes a parsed file's records.  PHK_ERR_ARG, before any launch: D not
 * 4^k, a row or sequence index out of range, lo > x, x > hi, hi > L_seq, hi - lo > 2^30, |q| > 2^31, a NULL where B > 0.
 * B == 0 is PHK_OK with nothing launched.  phk_refine_grid_pass(): the most boundaries one launch covers in one pass of its
 * grid (further ones by grid stride; for the tests). */
int phk_refine_boundaries_ascii(phk_ctx *ctx, const char *bases, const uint64_t *seq_offsets, uint64_t n_seq, int k,
                                const char *symbols4, const int64_t *qtable, uint64_t n_rows, uint64_t D, const uint64_t *seq,
                                const uint64_t *lo, const uint64_t *x, const uint64_t *hi, const uint32_t *left_row,
                                const uint32_t *right_row, uint64_t B, int64_t *position, int64_t *evidence, uint32_t *support);
int phk_refine_boundaries_fasta(phk_ctx *ctx, const phk_fasta *f, int k, const char *symbols4, const int64_t *qtable,
                                uint64_t n_rows, uint64_t D, const uint64_t *seq, const uint64_t *lo, const uint64_t *x,
                                const uint64_t *hi, const uint32_t *left_row, const uint32_t *right_row, uint64_t B,
                                int64_t *position, int64_t *evidence, uint32_t *support);
uint64_t phk_refine_grid_pass(void);

/* Boundary confidence: phk_refine_boundaries_* with a second kernel behind the first, which reads
 * P* = P(position) and the position from the first one's device outputs and walks the prefix sums again.  position, evidence
 * and support are the bits phk_refine_boundaries_* gives.  With drop_q >= 0 in units of 2^-16 nat, per boundary:
 *     interval[b][0] = lower    the smallest p in [lo, hi] with P(p) >= P* - drop_q (in bases of the sequence)
 *     interval[b][1] = upper    the largest such p          interval[b][2] = n_within, their number (they need not be contiguous)
 *     w(p) = exp(-(P* - P(p)) 2^-16), and w(p) = 0 exactly where P* - P(p) > 700 * 2^16 (an integer comparison)
 *     sums[b][0] = Z = sum_p w(p)                 sums[b][1] = M = sum of w(p) over lower <= p <= upper
 *     sums[b][2] = sum_{p < position} (position - p) w(p)        sums[b][3] = sum_{p > position} (p - position) w(p)
 *     sums[b][4] = sum_p (p - position)^2 w(p)
 * lower <= position <= upper, n_within >= 1 and Z >= 1 always; an empty interval gives (lo, lo, 1) and (1, 1, 0, 0, 0).  The
 * interval is exact.  The sums are float64, each weight one exp of an exact argument, added in an order that lo and hi alone
 * fix (the candidate lo; then per 1024 candidates: 16 in order per lane, the lanes by a butterfly, the total onto the running
 * sum): a boundary's eight numbers are the same bits whatever else the call holds and wherever its sequence lies in the
 * stream.  No logarithm, division or root is taken.  The errors of phk_refine_boundaries_*, and PHK_ERR_ARG for drop_q < 0 or a
 * NULL interval / sums where B > 0, before any launch. */
int phk_refine_confidence_ascii(phk_ctx *ctx, const char *bases, const uint64_t *seq_offsets, uint64_t n_seq, int k,
                                const char *symbols4, const int64_t *qtable, uint64_t n_rows, uint64_t D, const uint64_t *seq,
                                const uint64_t *lo, const uint64_t *x, const uint64_t *hi, const uint32_t *left_row,
                                const uint32_t *right_row, uint64_t B, int64_t drop_q, int64_t *position, int64_t *evidence,
                                uint32_t *support, int64_t *interval, double *sums);
int phk_refine_confidence_fasta(phk_ctx *ctx, const phk_fasta *f, int k, const char *symbols4, const int64_t *qtable,
                                uint64_t n_rows, uint64_t D, const uint64_t *seq, const uint64_t *lo, const uint64_t *x,
                                const uint64_t *hi, const uint32_t *left_row, const uint32_t *right_row, uint64_t B, int64_t drop_q,
                                int64_t *position, int64_t *evidence, uint32_t *support, int64_t *interval, double *sums);

/* Nearest-reference lookup: the k nearest rows of X[M][D] for every row of Q[N][D], what sorting a row of
 * learning.distances (scripts/learning.py:47-66) gives and what learning.knn (scripts/learning.py:118-128) folds into a
 * vote.  With d2(q, j) the direct-difference squared distance accumulated by fma in column order (the value phk_distances
 * takes the root of), a query's result is the first k rows in order of (d2, j): idx[N][k] int32, dist[N][k] = sqrt(d2),
 * equal distances by index.  1 <= k <= 28 and k <= the rows left by the column mask, else PHK_ERR_ARG; a NaN query row
 * gives PHK_ERR_NAN.  A float64 MFMA Gram-form proposal, an exact refinement of its candidates, a certificate and an exact
 * fallback over all rows: the result does not depend on N, the batch split, the entry point or the route.
 * phk_neighbors: host arrays; batch_rows = 0 picks the query batch, another value is rounded up to the query block of 128.
 * phk_model_neighbors: host float64 rows against the model's train rows under its column mask; indices point into
 * vstack(pos, neg).  phk_batch_neighbors: the rows of a resident batch, normalised on the device, nothing uploaded. */
int phk_neighbors(phk_ctx *ctx, const double *Q, uint64_t N, const double *X, uint64_t M, uint64_t D, int k, uint64_t batch_rows,
                  int32_t *idx, double *dist);
int phk_model_neighbors(phk_ctx *ctx, const phk_model *model, const double *Q, uint64_t N, int k, int32_t *idx, double *dist);
int phk_batch_neighbors(phk_ctx *ctx, const phk_model *model, const phk_batch *b, int k, int32_t *idx, double *dist);
/* out[0] = queries answered, out[1] = queries that took the fallback, since the last call; then both start from zero */
int phk_neighbors_stats(phk_ctx *ctx, uint64_t out[2]);
/* Diagnostics for the tests.  phk_neighbors_keep_details(ctx, 1): every later lookup on the context keeps, per query, the
 * certificate's bound E on |Gram-form value - d2| and whether it fell back, and per returned row its Gram-form value (NaN
 * for a row of a fallen-back query that the proposal had not kept).  phk_neighbors_details copies those of the last
 * lookup, which must have had this N and k: E[N], approx_d2[N][k], fell_back[N] bytes. */
int phk_neighbors_keep_details(phk_ctx *ctx, int on);
int phk_neighbors_details(phk_ctx *ctx, uint64_t N, int k, double *E, double *approx_d2, uint8_t *fell_back);

/* learning.silhouettes (scripts/learning.py:84-92, scikit-learn silhouette_samples): X[n][D] float64, labels[n] already
 * encoded 0..n_labels-1 -> out[n].  a = mean distance to the rest of the own cluster, b = smallest mean distance to another
 * cluster, s = (b - a) / max(a, b), 0 for a singleton.  Distances are float64 direct differences; every sum is taken in an
 * order fixed by the labels alone, so the result is bit-identical from run to run.  Host pointers.  PHK_ERR_ARG for a
 * label >= n_labels or n_labels outside 2..n-1; PHK_ERR_NAN for NaN rows. */
int phk_silhouettes(phk_ctx *ctx, const double *X, uint64_t n, uint64_t D, const uint32_t *labels, uint32_t n_labels,
                    double *out);

/* learning.dbscan (scripts/learning.py:149-163, scikit-learn DBSCAN(eps, min_samples).fit(X)): labels[n] (-1 = noise),
 * core[n] (1 = core sample; may be NULL), *n_clusters (may be NULL).  j is a neighbour of i iff the float64
 * direct-difference distance is <= eps (i itself included); core iff at least min_samples neighbours; clusters = the
 * connected components of the core points, numbered by their smallest row; a border point takes the smallest label among
 * its core neighbours.  Host pointers.  PHK_ERR_ARG for eps not finite and > 0 or min_samples < 1; PHK_ERR_NAN for NaN rows. */
int phk_dbscan(phk_ctx *ctx, const double *X, uint64_t n, uint64_t D, double eps, uint64_t min_samples, int64_t *labels,
               uint8_t *core, uint64_t *n_clusters);

/* ---- the DBSCAN eps x min_samples sweep (the parameters of learning.dbscan, scripts/learning.py:149-163).
 * The rows X[n][D] stay on the device (phk_dbscan_sweep_create; host pointer, float64; PHK_ERR_NAN for NaN rows).
 * phk_dbscan_sweep solves the C cells (eps[c], min_samples[c]), 1 <= C <= 64, in one call: every pair distance is computed
 * once per pass and serves all cells.  Per cell the result is phk_dbscan's for that cell alone:
 *   labels[C][n] int32 (-1 = noise), n_clusters[C] (may be NULL);
 *   coremask[n] (may be NULL): bit c = row i is a core sample of cell c.
 * tiles_per_launch: at most that many 64 x 64 pair tiles per launch of the count, union and border passes (0 = the
 * default); launches[3] (may be NULL) = the launches each of the three took.  A cell's results do not depend on C, on its
 * place in the list, on the other cells or on tiles_per_launch.  PHK_ERR_ARG for eps not finite and > 0, min_samples < 1
 * or C outside 1..64. */
typedef struct phk_dbscan_rows phk_dbscan_rows;
int phk_dbscan_sweep_create(phk_ctx *ctx, const double *X, uint64_t n, uint64_t D, phk_dbscan_rows **out);
int phk_dbscan_sweep_destroy(phk_ctx *ctx, phk_dbscan_rows *rows);
int phk_dbscan_sweep(phk_ctx *ctx, phk_dbscan_rows *rows, uint32_t C, const double *eps, const uint64_t *min_samples,
                     uint64_t tiles_per_launch, int32_t *labels, uint64_t *coremask, uint64_t *n_clusters, uint32_t *launches);

/* ---- batched per-contig placement (results_analyzer.get_taxonomy_prediction_dict, scripts/analysis.py:754-792; DESIGN.md
 * 4.9).  The reference rows X[n][D] stay on the device; phk_placement_run solves, for each of the B rows of Z[B][D], the
 * problem "k-means of X with the row appended (row n), then the silhouettes of the members of that row's cluster", the
 * problems of a chunk (`chunk` problems, 0 = the default) side by side in every launch.  Host pointers, float64.
 *   seeding: scikit-learn's k-means++ on the mean-centred rows with the caller's draws: first_seed = the first centre's
 *     row, draws[(k - 1)][T] = the uniform(size = T) of each further centre, T = 2 + int(ln k); seeds[B][k] (may be NULL) =
 *     the chosen rows; seed_margin[b] = the closest call of the fit's seeding decisions, relative to the potential (a
 *     draw's distance to the nearer prefix-sum value around it; the gap between the best trial's potential and the best
 *     trial on another row) -- scikit-learn's distances and sums round differently, the caller trusts the seeds above a guard;
 *   Lloyd: phk_kmeans_lloyd's iteration (same arithmetic: equal labels, sweeps and min_gap for equal centred rows and
 *     seeds), tolerance tol_rel * mean column variance of the appended matrix; labels[B][n + 1], n_iter[B], min_gap[B];
 *   silhouettes: sil[b][0 .. n_members[b]) = those of the members of row n's cluster, reference members in row order,
 *     the appended row last (sil is [B][n + 1]); sums in an order fixed by the labels alone;
 *   status[b]: PHK_PLACEMENT_DUPLICATE (the row equals a reference row bit for bit: every decision between the twins is an
 *     exact tie) | PHK_PLACEMENT_EMPTY (a cluster ran empty in some sweep; scikit-learn relocates it).
 * A problem's results do not depend on B, on its place in Z or on `chunk`.  PHK_ERR_NAN for NaN / infinite rows. */
#define PHK_PLACEMENT_DUPLICATE 1u
#define PHK_PLACEMENT_EMPTY 2u
typedef struct phk_placement phk_placement;
int phk_placement_create(phk_ctx *ctx, const double *X, uint64_t n, uint64_t D, phk_placement **out);
int phk_placement_destroy(phk_ctx *ctx, phk_placement *pl);
int phk_placement_run(phk_ctx *ctx, phk_placement *pl, const double *Z, uint64_t B, uint32_t k, uint32_t first_seed,
                      const double *draws, double tol_rel, int max_iter, uint32_t chunk, uint32_t *labels, uint32_t *seeds,
                      double *sil, uint32_t *n_members, uint32_t *status, int32_t *n_iter, double *min_gap,
                      double *seed_margin);

/* ---- the silhouette-against-k sweep (scripts/cluster.py:31-47): S k-means problems on the SAME rows
 * X[n][D] (resident, phk_sweep_create), problem s with its own k = ks[s], first centre first_seed[s] and draws, the problems
 * of a chunk (`chunk` problems, 0 = the default, 64) side by side in every launch.  Host pointers, float64.
 *   centring: the k-means stages run on X - column mean (NumPy's, bit for bit), the silhouettes on X as given;
 *   seeding: scikit-learn's k-means++ with the caller's draws, as phk_placement_run: draws + draw_off[s] = the
 *     (ks[s] - 1) x T_s uniforms of problem s, T_s = 2 + int(ln ks[s]) (draws may be NULL when every k is 1);
 *     seeds (may be NULL) = the chosen rows of all problems, concatenated (ks[0], then ks[1], ...); seed_margin[s];
 *   Lloyd: phk_kmeans_lloyd's iteration, tolerance tol_rel * mean column variance: labels[S][n], n_iter[S], min_gap[S]
 *     equal the single-problem path's bit for bit for equal seeds;
 *   silhouettes: sil[S][n] (may be NULL: the pass is skipped) = phk_silhouettes(X, labels[s], ks[s]) bit for bit, from ONE
 *     pass over the pairs for all problems: the distances d[n][n] are stored (and kept in the handle) when n * n * 8 bytes
 *     fit pair_budget (bytes; negative = a quarter of the free device memory at the call), else every problem takes
 *     phk_silhouettes' own pass;
 *   status[s]: PHK_SWEEP_EMPTY (a cluster ran empty in some sweep; scikit-learn relocates it).
 * A problem's results do not depend on S, on its place or on `chunk`.  PHK_ERR_NAN for NaN / infinite rows (at create);
 * PHK_ERR_ARG for k outside 1..n, with sil for k outside 2..n-1, for first_seed >= n, for k >= 2981. */
#define PHK_SWEEP_EMPTY PHK_PLACEMENT_EMPTY
typedef struct phk_sweep phk_sweep;
int phk_sweep_create(phk_ctx *ctx, const double *X, uint64_t n, uint64_t D, phk_sweep **out);
int phk_sweep_destroy(phk_ctx *ctx, phk_sweep *sw);
int phk_sweep_run(phk_ctx *ctx, phk_sweep *sw, uint64_t S, const uint32_t *ks, const uint32_t *first_seed, const double *draws,
                  const uint64_t *draw_off, double tol_rel, int max_iter, uint32_t chunk, int64_t pair_budget, uint32_t *labels,
                  uint32_t *seeds, double *sil, uint32_t *status, int32_t *n_iter, double *min_gap, double *seed_margin);

/* ---- the cross-validated k_neighbors x k_clusters grid of the knn / kmeans / combo methods.  Host
 * pointers, float64.  create: X[M][D] = vstack(positive, negative) with a held-out fold (< folds) and a class (non-zero =
 * positive) per row, all resident.  Train set `slot * folds + f` (slot 0 = positive, 1 = negative) = the rows of that class
 * outside fold f, in row order.
 *   fit: S k-means problems, problem s on train set set[s] with k = ks[s], first centre first_seed[s] (a position in the
 *     set) and draws as phk_sweep_run takes them; the stages run on the set's rows less set_mean[set][D] (the caller's:
 *     NumPy's column mean of those rows), tolerance set_tol[set] (absolute).  The problems of a chunk (`chunk`, 0 = 64) share
 *     their row count.  The centroids of problem s -- the mean of its clusters' member rows of X as given, summed in row
 *     order -- go to rows bank_off[s] .. + ks[s] of the resident bank of bank_rows rows (a call with another bank_rows makes
 *     a new, zeroed bank; S = 0 only does that).  status[s]: PHK_COMBO_GRID_EMPTY; n_iter, min_gap, seed_margin as
 *     phk_sweep_run reports them;
 *   get_centroids / put_centroids: rows row0 .. row0 + rows of the bank to / from the host;
 *   score: knn_out[Kn][M] = the vote (+-1.0, an even split is -1) of the first kn[i] <= 64 rows outside the row's own
 *     fold in order of (direct-difference chain, row index); km_out[Ku][M] = tanh((en - ep) / (ep + en)) of the square roots
 *     of the smallest chains to the positive / negative centroids of value j of the row's fold, the bank laid out as fold f at
 *     rows f * Cb, Cb = 2 * sum(ku): the positive segments ku[0], ku[1], ... then the negative ones.  Kn or Ku may be 0.
 *     rows_per_pass (0 = a 256 MiB block of the pair matrix; rounded up to 64) = query rows per launch of the pair passes.
 * A cell does not depend on the other values, on `chunk` or on rows_per_pass.  PHK_ERR_NAN for NaN / infinite rows (create);
 * PHK_ERR_ARG for folds < 2, M > 2^22, a k outside 1..n of its train set, kn outside 1..min(64, smallest train set), a bank
 * that does not match ku. */
#define PHK_COMBO_GRID_EMPTY PHK_PLACEMENT_EMPTY
typedef struct phk_combo_grid phk_combo_grid;
int phk_combo_grid_create(phk_ctx *ctx, const double *X, uint64_t M, uint64_t D, const uint32_t *fold_of, const uint8_t *is_positive,
                          uint32_t folds, phk_combo_grid **out);
int phk_combo_grid_destroy(phk_ctx *ctx, phk_combo_grid *g);
int phk_combo_grid_fit(phk_ctx *ctx, phk_combo_grid *g, uint64_t S, const uint32_t *set, const uint32_t *ks, const uint32_t *first_seed,
                       const double *draws, const uint64_t *draw_off, const double *set_mean, const double *set_tol, int max_iter,
                       uint32_t chunk, uint64_t bank_rows, const uint64_t *bank_off, uint32_t *status, int32_t *n_iter, double *min_gap,
                       double *seed_margin);
int phk_combo_grid_get_centroids(phk_ctx *ctx, phk_combo_grid *g, uint64_t row0, uint64_t rows, double *out);
int phk_combo_grid_put_centroids(phk_ctx *ctx, phk_combo_grid *g, uint64_t row0, uint64_t rows, const double *in);
int phk_combo_grid_score(phk_ctx *ctx, phk_combo_grid *g, uint32_t Kn, const uint32_t *kn, uint32_t Ku, const uint32_t *ku,
                         uint64_t rows_per_pass, double *knn_out, double *km_out);

/* ---- PCA and t-SNE (phamer_scorer.do_tsne, scripts/phamer.py:337-366).  Host pointers, float64 throughout;
 * every sum is taken in an order fixed by the shapes alone (no floating-point atomics): results are bit-identical from run
 * to run.  The callers (phamers_amd/manifold.py) reject NaN / infinite input first. ---- */

/* Column means mean[D] and the centred covariance cov[D][D] = Xc^T Xc / (n - 1) of X[n][D] (fp64 matrix pipe, rows cut
 * into chunks whose partial sums meet in chunk order).  2 <= n, 1 <= D <= 8192. */
int phk_pca_covariance(phk_ctx *ctx, const double *X, uint64_t n, uint64_t D, double *mean, double *cov);

/* out[n][n_components] = (X - mean) V^T for the component rows V[n_components][D], each sum in column order. */
int phk_pca_project(phk_ctx *ctx, const double *X, uint64_t n, uint64_t D, const double *mean, const double *V,
                    uint64_t n_components, double *out);

/* For every row of Z[n][d] its k nearest OTHER rows: idx[n][k] and the squared distances d2[n][k], ordered by
 * (distance, index).  Squared distances are float64 direct differences accumulated by fma in column order (the same bits
 * for (i, j) and (j, i)).  1 <= k <= min(n - 1, 4096); n < 2^24. */
int phk_tsne_neighbors(phk_ctx *ctx, const double *Z, uint64_t n, uint64_t d, uint64_t k, int32_t *idx, double *d2);

/* scikit-learn's _binary_search_perplexity on d2[n][k]: the conditional affinities P[n][k] and the precision beta[n] of
 * every row (beta from 1, at most 100 steps, entropy tolerance 1e-5). */
int phk_tsne_affinities(phk_ctx *ctx, const double *d2, uint64_t n, uint64_t k, double perplexity, double *P, double *beta);

/* The symmetric affinities (P + P^T) / sum(P + P^T) over the union of the directed edges idx[n][k] as CSR: indptr[n + 1],
 * and indices / values with room for 2 n k entries (columns ascending within a row); *nnz = entries written.  Host only. */
int phk_tsne_symmetrize(const int32_t *idx, const double *P, uint64_t n, uint64_t k, int64_t *indptr, int32_t *indices,
                        double *values, uint64_t *nnz);

/* The t-SNE objective at Y[n][2] for the CSR affinities times `exaggeration`: *kl = sum p log(max(p, eps) / max(q, eps))
 * over the entries, q_ij = w_ij / Z, w_ij = 1 / (1 + |y_i - y_j|^2), Z = sum_{i != j} w_ij, and
 * grad[n][2] = 4 (sum_j p_ij w_ij (y_i - y_j) - (1 / Z) sum_j w_ij^2 (y_i - y_j)), the second sum over ALL j. */
int phk_tsne_gradient(phk_ctx *ctx, const double *Y, uint64_t n, const int64_t *indptr, const int32_t *indices,
                      const double *values, double exaggeration, double *kl, double *grad);

/* Exactly n_steps updates of scikit-learn's _gradient_descent on Y[n][2] (in place), from update = 0 and gains = 1;
 * *kl (may be NULL) = the objective at the last gradient evaluation. */
int phk_tsne_descend(phk_ctx *ctx, double *Y, uint64_t n, const int64_t *indptr, const int32_t *indices, const double *values,
                     double exaggeration, double momentum, double learning_rate, double min_gain, uint64_t n_steps, double *kl);

/* TSNE._tsne: 250 iterations at momentum 0.5 with the affinities times early_exaggeration, then up to max_iter (>= 250) at
 * momentum 0.8 without; every 50th iteration the objective and the gradient norm decide n_iter_without_progress and
 * min_grad_norm as scikit-learn does.  Y[n][2] in place; *kl, *n_iter as TSNE.kl_divergence_, TSNE.n_iter_. */
int phk_tsne_fit(phk_ctx *ctx, double *Y, uint64_t n, const int64_t *indptr, const int32_t *indices, const double *values,
                 double early_exaggeration, double learning_rate, uint64_t max_iter, uint64_t n_iter_without_progress,
                 double min_grad_norm, double *kl, uint64_t *n_iter);

/* learning.distances (scripts/learning.py:47-56; with np.argmin on its result: learning.closest_to :59-66): the
 * Euclidean distances of every row of Q[N][D] to every row of X[M][D], out[N][M], float64, in the reference's
 * direct-difference form sqrt(sum_d (q_d - x_d)^2).  Host pointers. */
int phk_distances(phk_ctx *ctx, const double *Q, uint64_t N, const double *X, uint64_t M, uint64_t D, double *out);

/* ---- evaluation of score vectors (scripts/learning.py:185-243) ---- */

#define PHK_SORT_TILE 4096        /* keys per tile of the radix sort */
#define PHK_SORT_MAX_BLOCKS 512   /* workgroups of a sort pass; beyond PHK_SORT_TILE x this many keys a workgroup takes several tiles */

/* perm[n] = the permutation that orders keys[n] ascending (descending != 0: descending), STABLE both ways: equal keys stay
 * in index order; -0.0 and +0.0 are equal.  What np.argsort(keys, kind='stable') (of -keys when descending) returns.  A
 * least-significant-digit radix sort on order-preserving 64-bit images of the keys.  PHK_ERR_NAN when a key is NaN or
 * infinite, PHK_ERR_UNSUPPORTED for n >= 2^32; n == 0 is success.  Host pointers; the _dev form takes device pointers and
 * is stream ordered. */
int phk_argsort_f64(phk_ctx *ctx, const double *keys, uint64_t n, int descending, uint32_t *perm);
int phk_argsort_f64_dev(phk_ctx *ctx, const double *d_keys, uint64_t n, int descending, uint32_t *d_perm);

/* scikit-learn's roc_curve(labels, scores, drop_intermediate = flag) in integers: scores sorted descending, one point per
 * run of equal scores -- tps = positives (label != 0) so far, fps = 1 + index - tps, threshold = the run's score -- with the
 * flag set and more than two points every interior point at which the second differences of fps and tps are both zero
 * dropped, and (0, 0, +inf) put first.  fps, tps, thresholds: caller arrays of n + 1 places, *m = the points written;
 * *area2 = sum_i (fps_i - fps_i-1)(tps_i + tps_i-1) = 2 P N AUC exactly.  The rates fps / fps[m - 1], tps / tps[m - 1] and
 * area2 / (2 P N) are the caller's divisions.  Sort, scans and compaction run on the device; only the m points come back.
 * PHK_ERR_NAN when a score is NaN or infinite, PHK_ERR_UNSUPPORTED for n >= 2^32; a class without members is no error.
 * phk_roc_curve: host pointers.  _dev: d_scores[n] float64 (as phk_score_dev writes them) and d_labels[n] uint8 on the
 * device, the outputs on the host. */
int phk_roc_curve(phk_ctx *ctx, const double *scores, const uint8_t *labels, uint64_t n, int drop_intermediate, uint64_t *fps,
                  uint64_t *tps, double *thresholds, uint64_t *m, uint64_t *area2);
int phk_roc_curve_dev(phk_ctx *ctx, const double *d_scores, const uint8_t *d_labels, uint64_t n, int drop_intermediate,
                      uint64_t *fps, uint64_t *tps, double *thresholds, uint64_t *m, uint64_t *area2);

/* counts[4] = tp, fp, fn, tn at `threshold` (scripts/learning.py:206-209): positives (label != 0) with score >= threshold,
 * negatives with >=, positives with <, negatives with <.  Host pointers. */
int phk_truth_counts(phk_ctx *ctx, const double *scores, const uint8_t *labels, uint64_t n, double threshold, uint64_t *counts);

/* Paired comparison of the ROC areas of C score vectors over the SAME rows: DeLong's structural components
 * as integers, and a stratified bootstrap.  scores[C][n] float64, one row per cell, columns in vstack(positive, negative)
 * order: the first n_pos = P columns are the positives, N = n - P.  -0.0 == +0.0 as in the sort.
 *   twice-placements  t_pos[c][i] = 2 #{j : y_j < x_i} + #{j : y_j == x_i},  t_neg[c][j] = 2 #{i : x_i > y_j} + #{i : x_i == y_j}
 *                     (uint32); both sum to area2[c] = 2 P N AUC, the integer phk_roc_curve returns for the cell
 *   Gram matrices     g10[a][b] = sum_i t_pos[a][i] t_pos[b][i],  g01[a][b] = sum_j t_neg[a][j] t_neg[b][j] (uint64, exact)
 *   bootstrap         resample b draws P positives and N negatives with replacement: key(b, s) = splitmix64(splitmix64(seed) ^
 *                     (2 b + s)), s = 0 for the positives and 1 for the negatives; draw t = 0 .. n_s - 1 picks the class's row
 *                     (splitmix64(key + t) * n_s) >> 64; w[row] = times drawn; area2_boot[b][c] = sum_ij w_i w_j
 *                     (2 [x_i > y_j] + [x_i == y_j]) <= 2 P N.  Resample b depends on (seed, b) alone; all cells share it.
 * phk_compare_create uploads, sorts every cell and makes placements and Grams; the handle keeps the sorted orders for the
 * bootstrap.  PHK_ERR_ARG for C == 0, C > PHK_COMPARE_MAX_CELLS, n_pos == 0 or n_pos == n; PHK_ERR_NAN for a score that is
 * NaN or infinite; PHK_ERR_UNSUPPORTED for n >= 2^31 or when 4 N^2 P or 4 P^2 N reaches 2^64 (the Gram sums' bound).
 * phk_compare_placements: t_pos[C][P], t_neg[C][N].  phk_compare_grams: area2[C], g10[C][C], g01[C][C].
 * phk_compare_bootstrap: area2_boot[count][C] for the resamples first_resample .. first_resample + count - 1, per_launch of
 * them per launch (0 = the default; the results do not depend on it); PHK_ERR_UNSUPPORTED beyond
 * PHK_COMPARE_BOOT_MAX_ROWS rows (a resample's weights live in LDS).  Host pointers. */
#define PHK_COMPARE_MAX_CELLS 256
#define PHK_COMPARE_BOOT_MAX_ROWS 65535
typedef struct phk_compare phk_compare;
int phk_compare_create(phk_ctx *ctx, const double *scores, uint64_t C, uint64_t n, uint64_t n_pos, phk_compare **out);
int phk_compare_destroy(phk_ctx *ctx, phk_compare *cmp);
int phk_compare_placements(phk_ctx *ctx, phk_compare *cmp, uint32_t *t_pos, uint32_t *t_neg);
int phk_compare_grams(phk_ctx *ctx, phk_compare *cmp, uint64_t *area2, uint64_t *g10, uint64_t *g01);
int phk_compare_bootstrap(phk_ctx *ctx, phk_compare *cmp, uint64_t seed, uint64_t first_resample, uint64_t count,
                          uint64_t per_launch, uint64_t *area2_boot);

/* ---- device API -------------------------------------------------------------------- */
/* ASCII -> packed stream (+ mask).  d_any_invalid (one uint32, device) is set non-zero when
 * some base is not one of symbols4; it may be NULL. */
int phk_pack_ascii_dev(phk_ctx *ctx, const char *d_bases, uint64_t total_bases,
                       const char *symbols4, uint32_t *d_packed, uint32_t *d_mask,
                       uint32_t *d_any_invalid);
/* packed stream -> d_counts[n][4^k] uint32 and d_nwin[n] (= row sums = number of counted
 * windows; may be NULL).  d_mask may be NULL (all bases valid). */
int phk_count_dev(phk_ctx *ctx, const uint32_t *d_packed, const uint32_t *d_mask,
                  uint64_t total_bases, const uint64_t *d_offsets, uint64_t n, int k,
                  uint32_t *d_counts, uint32_t *d_nwin);
int phk_normalize_dev(phk_ctx *ctx, const uint32_t *d_counts, uint64_t n, uint64_t D,
                      double *d_out);
/* scores for device-resident float64 rows / for device-resident uint32 count rows (the
 * rows are normalised on the fly exactly as kmer.normalize_counts would).  d_status: one
 * uint32 (device), set to the number of NaN (zero-count) rows seen; their scores are NaN. */
int phk_score_dev(phk_ctx *ctx, const phk_model *model, const double *d_Q, uint64_t N,
                  int method, double *d_scores, uint32_t *d_status);
int phk_score_counts_dev(phk_ctx *ctx, const phk_model *model, const uint32_t *d_counts,
                         uint64_t N, int method, double *d_scores, uint32_t *d_status);
/* the whole hot path on device-resident input: count -> normalise -> score.  d_counts
 * ([n][4^k] uint32) receives the materialised counts. */
int phk_count_score_dev(phk_ctx *ctx, const phk_model *model, const uint32_t *d_packed,
                        const uint32_t *d_mask, uint64_t total_bases, const uint64_t *d_offsets,
                        uint64_t n, int k, int method, uint32_t *d_counts, double *d_scores,
                        uint32_t *d_status);

/* Verification on the device (a full-size batch of counts is tens of GB and is never brought to the host to be
 * checked): d_result[0] = number of rows of d_counts[n][D] whose sum differs from expected_rowsum (not evaluated when
 * expected_rowsum is UINT64_MAX), d_result[1] = number of words in which d_counts differs from d_other (not evaluated
 * when d_other is NULL).  d_result: two uint64 on the device.  A contig of L valid bases has L - k + 1 windows
 * (scripts/kmer.py:47), which is what the full-size tests pass as expected_rowsum. */
int phk_check_counts_dev(phk_ctx *ctx, const uint32_t *d_counts, const uint32_t *d_other, uint64_t n, uint64_t D,
                         uint64_t expected_rowsum, uint64_t *d_result);

/* Diagnostics of the most recent scoring call on this context, summed over its batches (synchronises the stream):
 * how many queries were resolved by the float64 brute-force fallback kernel and how many
 * (query, segment) orderings had to be decided by exact candidate distances rather than by
 * the certified fp32 margin.  Both are 0 on the all-float64 path. */
int phk_score_stats(phk_ctx *ctx, uint64_t *n_fallback, uint64_t *n_exact_resolved);
/* the same and more, out[0 .. n_out): [0] brute-forced queries, [1] orderings decided by exact distances, [2] queries
 * that took the second chance (split-query MFMA pass), [3..6] why the high-parts-only decision stage passed them on:
 * window wider than the refined candidates, window reaching past the lists, refined values too close, centroid
 * leader not certified; general D (k = 5, 6), int8 sweep: [7] rows re-swept alone with all three digits (the two-digit
 * window held more columns than the lists), [8] rows beyond the int8 operand, swept by the f16 count-exact kernel
 * (both are also counted in [2]) */
int phk_score_stats_ex(phk_ctx *ctx, uint64_t *out, int n_out);

/* Diagnostic of the arithmetic the MFMA proposal rests on: chains of v_mfma_f32_32x32x16_f16 on caller tiles.  Per tile
 * acc = C[32][32]; for s < steps: acc = A[s][32][16] (fp16 bits, row-major) x B[s][16][32] + acc, with D[tile][s][32][32] =
 * acc after step s.  Host pointers.  The parity tests use it to assert the per-instruction rounding charge of the
 * certification (2u (|acc_in| + sum |products|)) on adversarial inputs. */
int phk_mfma_f16_probe(phk_ctx *ctx, const uint16_t *A, const uint16_t *B, const float *C, uint64_t n_tiles, uint32_t steps,
                       float *D);

/* seeded synthetic batch generated on the device (phamers_amd/synth.py defines the hash):
 * n contigs of L bases, contig ids first_contig..first_contig+n-1; writes the packed stream,
 * the mask (if d_mask != NULL; required when invalid_ppm > 0) and offsets[n+1]. */
int phk_synth_packed_dev(phk_ctx *ctx, uint64_t seed, uint64_t first_contig, uint64_t n,
                         uint64_t L, uint32_t invalid_ppm, uint32_t *d_packed, uint32_t *d_mask,
                         uint64_t *d_offsets);

/* the ragged, composition-skewed variant (second bench workload): contig boundaries d_offsets[n+1] (device, any
 * lengths, d_offsets[n] = total_bases) are the caller's; every contig draws its own GC fraction
 * 1/2 +- gc_spread_permille / 2000 and bases from one hash per base (phamers_amd/synth.py: synth_ragged_codes). */
int phk_synth_ragged_dev(phk_ctx *ctx, uint64_t seed, uint64_t first_contig, uint64_t n, const uint64_t *d_offsets,
                         uint64_t total_bases, uint32_t gc_spread_permille, uint32_t invalid_ppm, uint32_t *d_packed,
                         uint32_t *d_mask);

/* ---- in-library kernel timing (HIP events on the context's stream) ------------------ */
int phk_profile_enable(phk_ctx *ctx, int on);
int phk_profile_reset(phk_ctx *ctx);
/* number of distinct kernels timed since the last reset */
int phk_profile_count(phk_ctx *ctx, int *count);
/* idx-th kernel: name (NUL-terminated, truncated to cap), total milliseconds, launches */
int phk_profile_get(phk_ctx *ctx, int idx, char *name, int cap, double *total_ms,
                    uint64_t *launches);

#ifdef __cplusplus
}
#endif
#endif /* PHAMERS_HIP_H */
