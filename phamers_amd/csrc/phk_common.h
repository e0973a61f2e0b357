// phk_common.h -- context, workspace, error and kernel-timing plumbing shared by the
// translation units of libphamers_hip.so.  gfx950 only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdarg.h>
#include <stdio.h>
#include <string>
#include <thread>
#include <functional>
#include <vector>

#include "../../include/phamers_hip.h"

#define PHK_WAVE 64

// Diagnostic code (phase timers, tuning overrides of the kernels' shape macros) compiles only in a build that says so;
// such a build reports another ABI version (phk_api.hip) and is refused by the loader.
#if (defined(I8_TIMERS) || defined(I8_NW) || defined(I8_NBUF) || defined(PHK_HI_REFINE) || \
     defined(PHK_RERANK_WAVES) || defined(PAIRS_ABL) || defined(F16H_ABL)) && !defined(PHK_DIAGNOSTIC_BUILD)
#error "kernel tuning / timer macros need -DPHK_DIAGNOSTIC_BUILD (make EXTRA_CXXFLAGS='-DPHK_DIAGNOSTIC_BUILD -D...')"
#endif

void phk_set_error(const char *fmt, ...);

#define PHK_HIP(call)                                                                      \
    do {                                                                                   \
        hipError_t e__ = (call);                                                           \
        if (e__ != hipSuccess) {                                                           \
            phk_set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e__), __FILE__, \
                          __LINE__);                                                       \
            return e__ == hipErrorOutOfMemory ? PHK_ERR_NOMEM : PHK_ERR_HIP;               \
        }                                                                                  \
    } while (0)

#define PHK_REQUIRE(cond, ...)        \
    do {                              \
        if (!(cond)) {                \
            phk_set_error(__VA_ARGS__); \
            return PHK_ERR_ARG;       \
        }                             \
    } while (0)

// first statement of every extern "C" entry that takes a context: the calling thread may have another device current
#define PHK_ENTER(ctx_, fname)                                   \
    do {                                                         \
        PHK_REQUIRE((ctx_) != nullptr, fname ": NULL ctx");      \
        PHK_HIP(hipSetDevice((ctx_)->device));                   \
    } while (0)

#define PHK_TRY(call)               \
    do {                            \
        int rc__ = (call);          \
        if (rc__ != PHK_OK) return rc__; \
    } while (0)

// workspace slots (device scratch owned by the context, grown on demand, reused)
enum PhkSlot {
    WS_ASCII = 0,   // host API: uploaded ASCII bases
    WS_PACKED,      // host API: packed stream
    WS_MASK,        // host API: validity mask
    WS_OFFSETS,     // host API: offsets
    WS_COUNTS,      // host API: uint32 counts
    WS_WIDE,        // host API: int64 / float64 staging
    WS_FLAGS,       // small flags / status words
    WS_Q64,         // scoring: float64 query rows
    WS_SCORES,      // scoring: float64 scores
    WS_DIST,        // scoring (exact path): distance tiles
    WS_QF32,        // scoring (MFMA path): fragment-ordered fp32 queries
    WS_CAND,        // scoring (MFMA path): candidate lists
    WS_NWIN,        // row sums
    WS_LONG,        // counting: contigs handed from the lane-pair kernel to the wave-per-contig kernel
    WS_OUT,         // batch API: scores on their way to the host
    WS_SUB,         // scoring at general D: dense count rows (+ row sums) of a second pass's sub-batch
    WS_QUEUE,       // scoring at general D: the two hand-over queues of the first pass
    WS_FRAG8,       // count -> score at k = 5: the int8 query fragments of the whole call, written by the count kernel's flush
    WS_BIG8,        // ... and their per-row flag words (+ the call's mode word)
    WS_SCTL,        // scoring (MFMA path): the call's statistics totals, the two sets of counters / query lists / striped words
    WS_CTL,         // small control words the kernels keep zeroed themselves (no memset per call): the count planner's two
                    // alternating blocks (PhkCountCtl), see phk_launch_count
    WS_KDE,         // density scoring: per-chunk (max, sum) partials + query norms (density.hip)
    WS_SORT,        // evaluation: the radix sort's key / index pairs and histograms, the ROC curve's points (evaluate.hip)
    WS_NN,          // neighbour lookup: a batch's merged candidate lists and its list of uncertified queries (neighbors.hip)
    WS_NNF,         // ... the gathered rows of the queries that fall back
    WS_NND,         // ... the kept details of a call (phk_neighbors_keep_details)
    WS_SEG,         // track segmentation: a call's evidence, outputs, tile and record arrays (segment.hip)
    WS_MIX,         // mixture E-step: a batch's responsibilities, the row outputs, the blocks' partial vectors (mixture.hip)
    WS_SLOTS
};

struct PhkBuf {
    void *ptr = nullptr;
    uint64_t bytes = 0;
    uint64_t gen = 0;    // counts (re)allocations: a user that keeps state in the buffer sees when it has to start over
};

struct PhkTimed {
    std::string name;
    std::vector<hipEvent_t> ev;  // start/stop pairs not yet folded
    double ms = 0.0;
    uint64_t launches = 0;
};

// workspace layout: hands out consecutive pieces of one allocation, every piece starting on a multiple of `align` bytes
struct PhkLayout {
    uint64_t bytes = 0;
    uint64_t align = 256;
    uint64_t take(uint64_t b) {
        const uint64_t o = bytes;
        bytes += (b + align - 1) / align * align;
        return o;
    }
};

// the "proposal" option (phk_set_option / PHK_PROPOSAL) as set_knob parses it.  A value that names no flavour is accepted
// and scores as the default does (PHK_PROP_OTHER); like every set value it keeps phk_count_score_dev from offering the int8
// operand hand-over.
enum PhkProposal { PHK_PROP_DEFAULT = 0, PHK_PROP_OTHER, PHK_PROP_F16, PHK_PROP_HI, PHK_PROP_CXF, PHK_PROP_I83 };

// The "count_lanes" option (phk_set_option / PHK_COUNT_LANES) as set_knob decodes its first character; nothing else looks at
// the character.  `slot path`: whether the slot kernels count a batch they are eligible for (count_route); `pairs`: threads
// of the two-windows-per-add kernel at k = 4 without a mask; `direct`: threads of the slot kernel, - = by k (512 at k = 3, 4).
//   value   slot path                pairs   direct   int8 operand offered (phk_count_score_dev)
//   unset   by the statistics        1024    -        yes
//   0       never (wave-per-contig)  .       .        no
//   f       whatever the batch       none    -        no
//   p       by the statistics        512     512      no
//   P       by the statistics        1024    -        no
//   q       whatever the batch       512     512      no
//   Q       whatever the batch       1024    -        no
//   d       by the statistics        none    512      no
//   D       by the statistics        none    1024     no     (k = 3 stays at 512)
//   other   by the statistics        none    -        no
struct PhkCountLanes {
    bool set = false;         // the option holds a value
    bool wave_only = false;   // '0'
    bool forced = false;      // f q Q: no stand-down by the batch statistics, no sorted walk
    uint16_t pairs = 1024;    // threads of phk_count_pairs_kernel, 0 = not launched
    uint16_t direct = 0;      // threads of phk_count_direct_kernel, 0 = no preference
};
static inline PhkCountLanes phk_count_lanes_of(char c) {   // set_knob's decoder: the table above, column by column
    PhkCountLanes l;
    l.set = c != 0;
    l.wave_only = c == '0';
    l.forced = c == 'f' || c == 'q' || c == 'Q';
    l.pairs = (c == 0 || c == 'P' || c == 'Q') ? 1024 : ((c == 'p' || c == 'q') ? 512 : 0);
    l.direct = (c == 'd' || c == 'p' || c == 'q') ? 512 : (c == 'D' ? 1024 : 0);
    return l;
}

// Tuning / diagnostic knobs.  Read ONCE from the environment when the context is created (PHK_<NAME>), changed
// afterwards only through phk_set_option(): no launch path calls getenv.
struct PhkKnobs {
    PhkCountLanes count_lanes; // which count kernels (count_route, count_shared.h), decoded once by set_knob: the table above
    bool force_exact = false;  // every model through the float64 path
    PhkProposal proposal = PHK_PROP_DEFAULT;   // first pass of the fast scorer, parsed once by set_knob (see the table at ScoreRoute, score_mfma.hip)
    char cx_cfg[8] = "";       // "<tiles per wave><waves per workgroup>": 14, 24, 28
    char rerank = 0;           // 'w' wave per query, 'g' 16 lanes per query for all
    bool count_sort = true;    // length-bucketed contig order for the slot count kernel on ragged batches
    uint64_t score_batch = 0;  // queries per scoring batch of the MFMA path (0 = default 2^20; tests shrink it)
    char i8_insert = 0;        // two-part int8 sweep, how a tile's values meet the lists: '0' test per eight and per value, '1' test per eight,
                               // '2' no test (0 = by the number of columns, phk_launch_proposal_i8_general)
    bool gen_seq = false;      // int8 sweep: the column groups as successive launches (each group's records L2-resident) instead of a 2-D launch
    int gen_groups = 0;        // column groups of the general-D sweep's 2-D launch (0 = default: PHK_GEN_GROUPS at D >= 2048, else 1)
    int ws_fail = 0;           // fault injection for the tests: the ws_fail-th workspace allocation from now on asks hipMalloc for
                               // 2^60 bytes (a genuine out-of-memory failure on the genuine error path), then the knob is spent
    bool tail_aside = true;    // multi-batch scoring at k = 4: a batch's hand-over kernels on the second stream beside the next
                               // batch's sweep (option "tail_aside" = 0: everything on one stream, for A/B runs)
};

// The int8 operand of the general-D sweep prepared by the count kernel (phk_count_score_dev at k = 5: the flush of
// phk_count_direct_kernel writes each row's centred int8 fragment pieces beside the counts, which saves the scorer a pass
// over the 4 KB count rows).  big[n] is the call's mode word: 0 = every row prepared, 1 = rows flagged PHK_PREP8_MISSING
// are not (contigs handed to the wave-per-contig kernel), 2 = nothing prepared (a ragged batch took the sorted slot
// kernel); phk_split_queries_i8_kernel completes the operand accordingly.
#define PHK_PREP8_MISSING 0x40000000u
#define PHK_I8_L1_MAX 65000u   // |c - c0|_1 of a row the sweep epilogue's 32-bit fold is exact for: (256 * 127 + 128) * 65000 < 2^31
struct PhkPrep8 {
    bool offered = false;               // phk_count_score_dev: the buffers below exist and belong to `counts`
    bool written = false;               // phk_launch_count: the one kernel that writes the fragments was launched for this matrix --
                                        // every other way through it (tiny or empty batches, knobs, the wave-per-contig kernel)
                                        // leaves it false, and the scorer prepares its operand itself
    const uint32_t *counts = nullptr;   // the count matrix the fragments belong to
    uint64_t n = 0, D = 0;
    void *frag = nullptr;               // [ceil(n / 32)][D / 32][64 lanes] x 16 bytes
    uint32_t *big = nullptr;            // [n + 1]
};

// What the count stage and the score stage of ONE phk_count_score_dev call tell each other.  It lives on that call's stack
// and is passed down as an optional trailing pointer (phk_launch_count, phk_score_rows, phk_score_fast,
// phk_launch_proposal_i8_general); every other caller passes none: the scorer then zeroes its own words with a memset and
// prepares its own operand.  Nothing of it is kept in the context, so a call that fails half way leaves nothing behind.
struct PhkStepLink {
    PhkPrep8 prep8;
    // words the count planner's kernel is asked to zero beside its own -- [0] the scorer's NaN counter, [1] the call totals of
    // its statistics (WS_SCTL) -- so that no memset stands in front of either stage; `planned` = that kernel was launched
    uint32_t *zero[2] = {nullptr, nullptr};
    uint32_t zero_words[2] = {0, 0};
    bool planned = false;
    bool zeroed(const uint32_t *p) const { return planned && p && (p == zero[0] || p == zero[1]); }
};

struct phk_ctx {
    int device = 0;
    PhkKnobs knobs;
    bool slots_lds0 = true;        // the slot count kernel's dynamic LDS starts at address 0 (checked at creation)
    hipStream_t stream = nullptr;
    bool own_stream = false;
    // second stream of multi-batch scoring calls (phk_score_fast): batch b's hand-over kernels -- second chance, merge, brute
    // force: a few % of the chip -- run here beside batch b + 1's sweep; forked from / joined to `stream` with events inside
    // the call, so the caller still sees one stream-ordered operation
    hipStream_t aux = nullptr;
    hipEvent_t ev_fork[2] = {nullptr, nullptr}, ev_tail[2] = {nullptr, nullptr};
    // Control words of the count planner (phk_launch_count): two blocks used alternately -- the planning kernel of a call
    // zeroes the block of the NEXT call, so no launch is preceded by a memset.  ctl_gen = the allocation the blocks were
    // zeroed for; ctl_epoch = calls so far (its parity picks the block); ctl_dirty = a call failed half way.
    uint64_t ctl_gen = 0, ctl_epoch = 0;
    bool ctl_dirty = true;
    // the scorer's control words (phk_score_fast, WS_SCTL): zeroed by the kernels that read them last; see there
    uint64_t score_ctl_gen = 0;
    bool score_ctl_dirty = true;
    int num_cus = 256;
    PhkBuf ws[WS_SLOTS];
    bool profile = false;
    bool last_score_fast = false;  // the last scoring call took the MFMA path: WS_SCTL's first words hold its totals (phk_score_stats)
    std::vector<PhkTimed> timed;
    std::vector<hipEvent_t> ev_pool;
    // pinned staging buffers of the sequence upload (phk_batch_from_ascii), allocated at the first multi-chunk upload
    void *stage[2] = {nullptr, nullptr};
    uint64_t stage_bytes = 0;
    // neighbour lookup (neighbors.hip): queries seen / fallen back since the last phk_neighbors_stats; whether calls keep
    // their details in WS_NND, and the shape of the call they belong to (0 rows: none)
    uint64_t nn_queries = 0, nn_fell_back = 0;
    bool nn_keep = false;
    uint64_t nn_det_n = 0;
    int nn_det_k = 0;
};

int phk_ws(phk_ctx *ctx, int slot, uint64_t bytes, void **out);

// One device allocation and its owner: freed when the owner goes (a handle's `delete`, a call's way out), so no create or
// run function frees by hand.  Move-only.  The context's own scratch is phk_ws above; this is for what a handle keeps and
// for the buffers of one call.
struct PhkDevMem {
    void *ptr = nullptr;
    uint64_t bytes = 0;
    PhkDevMem() = default;
    PhkDevMem(const PhkDevMem &) = delete;
    PhkDevMem &operator=(const PhkDevMem &) = delete;
    PhkDevMem(PhkDevMem &&o) noexcept : ptr(o.ptr), bytes(o.bytes) { o.ptr = nullptr; o.bytes = 0; }
    ~PhkDevMem() { release(); }
    void release() {
        if (ptr) (void)hipFree(ptr);
        ptr = nullptr;
        bytes = 0;
    }
    template <class T> T *as() const { return (T *)ptr; }
    // `bytes` of `what` for `fname`; what the owner held is freed first (the caller drains the stream if it may be in use).
    // A failure leaves the owner empty and no HIP error pending.
    int alloc(const char *fname, const char *what, uint64_t b) {
        release();
        if (hipMalloc(&ptr, b ? b : 1) != hipSuccess) {
            ptr = nullptr;
            (void)hipGetLastError();
            phk_set_error("%s: out of device memory (%llu bytes of %s)", fname, (unsigned long long)b, what);
            return PHK_ERR_NOMEM;
        }
        bytes = b;
        return PHK_OK;
    }
    // a handle's workspace, grown to `need` bytes (the stream is drained first: the old block may be in use)
    int grow(phk_ctx *ctx, const char *fname, uint64_t need, uint64_t problems) {
        if (bytes >= need) return PHK_OK;
        PHK_HIP(hipStreamSynchronize(ctx->stream));
        if (alloc(fname, "workspace", need) != PHK_OK) {
            phk_set_error("%s: out of device memory (%llu bytes for %llu problems at once)", fname, (unsigned long long)need,
                          (unsigned long long)problems);
            return PHK_ERR_NOMEM;
        }
        return PHK_OK;
    }
};

// Large transfers between caller arrays and the device go through the context's two pinned staging buffers (64 MB each),
// host threads copying on one side while the bus works on the other: an array handed to hipMemcpy as it is has its pages
// pinned inside the runtime and costs 0.05 - 0.1 s per GB to free afterwards (tools/diag/fasta_free_time.py).  Below 128 MB
// a plain stream-ordered copy.  phk_copy_to_host returns with the data in place; phk_copy_to_device is stream ordered.
// (batch.hip, strands.hip) a device-resident batch: what the opaque phk_batch of the header is
struct phk_batch {
    uint64_t n = 0, D = 0, T = 0;
    int k = 0;
    uint32_t *d_counts = nullptr;   // [n][D]
    uint32_t *d_nwin = nullptr;     // [n] row sums (= counted windows; twice that once folded)
    bool any_invalid = false;       // some base of the source batch was not one of the symbols (inherited by a selection:
                                    // "may hold invalid bases", not re-derived per row)
    bool folded = false;            // the rows are strand-symmetric: phk_batch_fold_strands has run (inherited by a selection
                                    // and by a column gather)
    std::vector<uint64_t> len;      // [n] bases per contig (host): what a selection's total_bases is summed from
};
// (batch.hip) the sequence bytes of a batch -> device, packed and counted; see there
// `windows` (windows.hip): the rows of the batch are not the sequences but their sliding windows [j step, j step + window),
// sequence-major by start, counted by phk_launch_windows instead of phk_launch_count; no window at all is PHK_ERR_ARG.
struct PhkWindowSpec {
    uint64_t window, step;
    uint32_t segment;   // windows per work unit, 0 = the launch chooses
};
int phk_batch_build(phk_ctx *ctx, const char *bases, const std::function<void(uint64_t, uint64_t, char *)> *fill,
                    const uint64_t *offsets, uint64_t n, int k, const char *symbols4, phk_batch **out,
                    const PhkWindowSpec *windows = nullptr);
// (batch.hip) the same from the RAW bytes of a FASTA file (title lines, line ends and all) + one layout entry per record:
// the bytes go up as they are and the device drops what is not sequence (phk_deline_pack_kernel, ingest.hip).
// phk_raw_to_device puts the file's bytes into the context's WS_ASCII workspace (staged copies; it may run on a thread of its
// own beside the host's index scan -- nothing else uses the context meanwhile); phk_batch_build_raw then takes the record
// layout and the side buffer of the irregular records (rbegin[r] indexes the raw bytes, or `side` where rlw[r] = 2^32 - 1).
int phk_raw_to_device(phk_ctx *ctx, const char *raw, uint64_t raw_bytes, const uint8_t **d_raw);
int phk_batch_build_raw(phk_ctx *ctx, const uint8_t *d_raw, const char *side, uint64_t side_bytes,
                        const uint64_t *rbegin, const uint32_t *rlw, const uint32_t *rtl, const uint64_t *offsets, uint64_t n,
                        int k, const char *symbols4, phk_batch **out);
#define PHK_STAGE_BYTES (64ull << 20)
// the context's two pinned staging buffers of PHK_STAGE_BYTES each, allocated on first use by whichever transfer needs them;
// a partial failure frees what it got (the next call starts from nothing) and returns PHK_ERR_NOMEM
int phk_stage_ensure(phk_ctx *ctx);
int phk_copy_to_host(phk_ctx *ctx, void *dst, const void *d_src, uint64_t bytes);
int phk_copy_to_device(phk_ctx *ctx, void *d_dst, const void *src, uint64_t bytes);

// kernel timing: PHK_LAUNCH(ctx, "name", kernel<<<...>>>(...)) brackets the launch with HIP
// events on the context's stream when profiling is on.
int phk_prof_begin(phk_ctx *ctx, const char *name, int *slot);
int phk_prof_end(phk_ctx *ctx, int slot);

#define PHK_LAUNCH(ctx, name, ...)                         \
    do {                                                   \
        int ps__ = -1;                                     \
        if ((ctx)->profile) PHK_TRY(phk_prof_begin((ctx), (name), &ps__)); \
        __VA_ARGS__;                                       \
        PHK_HIP(hipGetLastError());                        \
        if ((ctx)->profile) PHK_TRY(phk_prof_end((ctx), ps__)); \
    } while (0)

// A grid of 2^32 work-items or more is not launched whole: the excess is dropped without an error (round 5: a 30M-contig
// synthetic batch came out generated for its first 2.5M contigs only).  Launchers whose grid grows with the input's bases or
// rows go through this loop: slices of at most PHK_SLICE_BLOCKS blocks, the kernel is told the slice's first block.
#define PHK_SLICE_BLOCKS (1ull << 22)   // x 1024 threads at most = 2^32 / 1
#define PHK_LAUNCH_SLICED(ctx, name, total_blocks, block0, nblk, ...)                                        \
    for (uint64_t block0 = 0, tb__ = (total_blocks); block0 < tb__; block0 += PHK_SLICE_BLOCKS) {           \
        const unsigned nblk = (unsigned)(tb__ - block0 < PHK_SLICE_BLOCKS ? tb__ - block0 : PHK_SLICE_BLOCKS); \
        PHK_LAUNCH(ctx, name, __VA_ARGS__);                                                                  \
    }

// host-side parallel loop for the model builders (independent iterations, disjoint outputs)
template <typename F>
static inline void phk_parallel_for(uint64_t n, F fn) {
    unsigned nt = std::thread::hardware_concurrency();
    nt = nt < 1 ? 1 : (nt > 16 ? 16 : nt);
    if (n < 2 * (uint64_t)nt) nt = 1;
    if (nt == 1) {
        for (uint64_t i = 0; i < n; ++i) fn(i);
        return;
    }
    std::vector<std::thread> pool;
    for (unsigned t = 0; t < nt; ++t)
        pool.emplace_back([=]() {
            for (uint64_t i = n * t / nt; i < n * (t + 1) / nt; ++i) fn(i);
        });
    for (auto &th : pool) th.join();
}

// every value finite: what the resident handles ask of their rows before anything goes up (the caller's PHK_ERR_NAN)
static inline bool phk_rows_finite(const double *x, uint64_t count) {
    for (uint64_t i = 0; i < count; ++i)
        if (!(x[i] - x[i] == 0.0)) return false;
    return true;
}

// x / T for the elements of ONE count row: T and y = 1.0 / T (one IEEE division) are shared by the row, each element costs
// two Newton steps on the quotient -- 5 multiply-adds instead of the ~35 instructions of a float64 division (the general-D
// decision kernel spent a third of its vector instructions dividing).  The result IS the correctly rounded quotient, bit
// for bit what `x / T` returns: with y the correctly rounded reciprocal and q within one ulp of x / T,
// RN(q + (x - T q) y) = RN(x / T) (Markstein's theorem; fma makes the residual exact), and the first step brings
// q = RN(x y) within one ulp.  0 / 0 stays NaN (y = inf) -- and so does x / 0: a caller whose T can be zero beside non-zero
// entries divides such a row for real (phk_normalize_int_kernel).  tests/test_gpu_rows.py checks the result against NumPy's
// division, bit for bit, through every normalise entry point (row sums of 2^m - 1, 2^m, 2^m + 1 up to 2^52, entries up to
// 2^32 - 1, over 2 * 10^6 distinct (entry, row sum) pairs each): that pins the division as a whole -- q0 alone, a reciprocal
// approximation or relaxed floating-point flags fail there.  It does NOT pin the second step: for the integer operands
// every caller passes (|x|, |T| < 2^53; the signs change nothing) q1 is already the rounded quotient.
// q0 + (x - T q0) y differs from x / T by |x / T - q0| |T y - 1| < ulp * 2^-53, while x / T stays ulp / (2 T) or more away
// from every rounding midpoint: no misrounding is possible below T = 2^51, and above it the quotients nearest to a
// midpoint (x 2^54 = m T +- 1, m odd: quotients in [1/2, 1)) were searched in exact arithmetic without a case
// (tools/diag/div_exact_check.py --midpoints).  The second step is kept as the form the theorem covers for every operand.
__device__ __forceinline__ double phk_div_row(double x, double T, double y) {
    const double q0 = x * y;
    const double q1 = __builtin_fma(__builtin_fma(-q0, T, x), y, q0);
    return __builtin_fma(__builtin_fma(-q1, T, x), y, q1);
}

// Count rows enter the count-exact MFMA kernels CENTRED by an integer: c_i - c0 with c0 = the integer nearest to T / D
// (T = row sum); every kernel derives c0 from T with this one function (see score_lists.h).
__host__ __device__ __forceinline__ uint32_t phk_row_center(uint32_t T, uint32_t D) { return (T + D / 2) / D; }

static inline uint64_t phk_pow4(int k) { return 1ull << (2 * k); }
static inline uint64_t phk_div_up(uint64_t a, uint64_t b) { return (a + b - 1) / b; }

// ---- internal entry points implemented across translation units ----
// per-device kernel attributes (dynamic LDS above 64 KiB), set for the context's device at phk_create
int phk_count_init_device(phk_ctx *ctx);       // count_slots.hip
int phk_score_f16_init_device(phk_ctx *ctx);   // score_f16.hip
int phk_score_mfma_init_device(phk_ctx *ctx);  // score_mfma.hip
// ingest.hip
int phk_launch_pack(phk_ctx *ctx, const char *d_bases, uint64_t T, const char *symbols4,
                    uint32_t *d_packed, uint32_t *d_mask, uint32_t *d_any_invalid);
int phk_launch_deline_pack(phk_ctx *ctx, const uint8_t *d_raw, const uint8_t *d_side, const uint64_t *d_offsets, uint64_t n, const uint64_t *d_rbegin,
                           const uint32_t *d_rlw, const uint32_t *d_rtl, uint64_t T, const char *symbols4, uint32_t *d_packed,
                           uint32_t *d_mask, uint32_t *d_any_invalid);
// count.hip (the driver; its stages and the kernels' launchers: count_shared.h)
int phk_launch_count(phk_ctx *ctx, const uint32_t *d_packed, const uint32_t *d_mask, uint64_t T,
                     const uint64_t *d_offsets, uint64_t n, int k, uint32_t *d_counts,
                     uint32_t *d_nwin, uint64_t mean_bases = 0, PhkStepLink *link = nullptr);
// rows.hip
int phk_launch_widen(phk_ctx *ctx, const uint32_t *d_in, uint64_t count, int64_t *d_out);
int phk_launch_normalize_u32(phk_ctx *ctx, const uint32_t *d_counts, uint64_t n, uint64_t D,
                             double *d_out);
// density.hip: |x|^2 of the rows of d_X[n][D], float64, profiled as phk_kde_rownorm_kernel
int phk_launch_rownorm(phk_ctx *ctx, const double *d_X, uint64_t n, uint64_t D, double *d_out);
int phk_launch_normalize_i64(phk_ctx *ctx, const int64_t *d_counts, uint64_t n, uint64_t D,
                             double *d_out);
int phk_launch_normalize_f64(phk_ctx *ctx, const double *d_rows, uint64_t n, uint64_t D,
                             double *d_out);
int phk_launch_permute_columns(phk_ctx *ctx, const int64_t *d_in, uint64_t n, uint64_t D, const uint32_t *d_perm,
                               int64_t *d_out);
int phk_launch_check_counts(phk_ctx *ctx, const uint32_t *d_counts, const uint32_t *d_other, uint64_t n, uint64_t D,
                            uint64_t expected_rowsum, uint64_t *d_result);
// windows.hip: rows = the windows of every sequence (`offsets` is the HOST array); phk_windows_rows counts them
uint64_t phk_windows_rows(const uint64_t *offsets, uint64_t n, uint64_t window, uint64_t step);
int phk_launch_windows(phk_ctx *ctx, const uint32_t *d_packed, const uint32_t *d_mask, uint64_t T, const uint64_t *offsets,
                       uint64_t n, int k, uint64_t window, uint64_t step, uint32_t segment, uint32_t *d_counts, uint32_t *d_nwin);
// synth.hip
int phk_launch_synth(phk_ctx *ctx, uint64_t seed, uint64_t first, uint64_t n, uint64_t L,
                     uint32_t invalid_ppm, uint32_t *d_packed, uint32_t *d_mask,
                     uint64_t *d_offsets);
int phk_launch_synth_ragged(phk_ctx *ctx, uint64_t seed, uint64_t first, uint64_t n, const uint64_t *d_offsets,
                            uint64_t total_bases, uint32_t gc_spread_permille, uint32_t invalid_ppm, uint32_t *d_packed,
                            uint32_t *d_mask);
// cluster.hip: phk_silhouettes on rows that are on the device already (d_rows[n][D], free of NaN)
int phk_silhouettes_resident(phk_ctx *ctx, const double *d_rows, uint64_t n, uint64_t D, const uint32_t *labels, uint32_t n_labels,
                             double *out);
// score.hip
// out[q][x] = the direct-difference fma chain |Q[q] - X[x]|^2 (pair_tile.h; profiled as phk_dist2_f64_kernel), out[nq][nx]; masked rows -> +inf
// (phk_mask_dist_kernel)
int phk_launch_dist2(phk_ctx *ctx, const double *d_Q, uint64_t nq, const double *d_X, uint64_t nx, uint64_t D, double *d_out);
int phk_launch_mask_dist(phk_ctx *ctx, double *d_dist, uint64_t nq, uint64_t M, const uint8_t *d_mask);
struct phk_model;
int phk_score_rows(phk_ctx *ctx, const phk_model *m, const double *d_Q, const uint32_t *d_counts,
                   const uint32_t *d_rowsum, uint64_t N, int method, double *d_scores, uint32_t *d_status,
                   const PhkStepLink *link = nullptr);
