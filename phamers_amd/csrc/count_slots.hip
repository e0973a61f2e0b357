// count_slots.hip -- the slot count kernels (one histogram column per contig; k = 3, 4, 5), the planning and sorting kernels
// in front of them, their launchers and the per-device set-up (gfx950).  The driver that chains them: count.hip.
#include "count_shared.h"

// ------------------------------------------------------------------------------------
// Length-bucketed contig order for ragged batches.  The slot kernel pads every group of SLOTS contigs to its longest
// member, so a batch of mixed lengths in arbitrary order wastes most of its stages.  A counting sort by the number of
// 1024-window stages (descending: the longest groups start first, the short tail fills the machine at the end) makes
// every group homogeneous.  Three small kernels, all gated ON THE DEVICE by the batch statistics: for a batch that is
// not ragged they return at once (no host round trip decides this).
// What is sorted are work ITEMS (contig, piece): a contig of more than long_thr windows is cut into pieces of piece_w
// windows, each an item of its own with its own histogram column in the slot kernel, added onto the contig's (zeroed) row
// with atomics at the flush -- one 500 kb contig is shared by 15 columns instead of setting the length of its group.
//   key(item) = min(ceil(W_item / 1024), SORT_KEYS - 1)
// ------------------------------------------------------------------------------------

// The planning kernel: ONE launch in front of the count kernels (round 5; rounds 2-4 spent two memsets and four launches
// here: statistics, key histogram, scan, scatter -- all of them no-ops on a batch of similar lengths).
//   * batch statistics for the stand-down rule (phk_slots_apply): padded / counted windows over groups of `gs` contigs;
//   * sort != 0: the key histogram of the work items, whatever the batch looks like (a block's few non-empty keys);
//   * the LAST block to finish (a ticket) reads the totals back with device-scope loads, and -- only for a batch the
//     statistics call ragged -- turns the histogram into the scatter's cursors and writes the item count;
//   * every block zeroes its share of the NEXT call's control block and of up to two word ranges the caller names (the
//     scorer's NaN counter and call totals): no launch of the chain is preceded by a memset.
// The control block's words (CTL_*): count_shared.h.
__global__ __launch_bounds__(256) void phk_count_plan_kernel(const uint64_t *__restrict__ offsets, uint64_t n, int k,
                                                             uint32_t gs,  // contigs per slot workgroup (16 or 32)
                                                             uint32_t long_thr, uint32_t piece_w, int sort,
                                                             uint32_t *__restrict__ ctl, uint32_t *__restrict__ ctl_next,
                                                             uint32_t *__restrict__ z0, uint32_t z0n, uint32_t *__restrict__ z1, uint32_t z1n) {
    __shared__ uint32_t h[SORT_KEYS];
    __shared__ unsigned long long s_pad[4], s_used[4];
    __shared__ uint32_t s_last;
    const int tid = threadIdx.x;
    {
        const uint32_t g0 = blockIdx.x * 256u + (uint32_t)tid, gn = gridDim.x * 256u;
        for (uint32_t i = g0; i < (uint32_t)CTL_WORDS; i += gn) ctl_next[i] = 0;
        for (uint32_t i = g0; i < z0n; i += gn) z0[i] = 0;
        for (uint32_t i = g0; i < z1n; i += gn) z1[i] = 0;
    }
    if (sort)
        for (int i = tid; i < SORT_KEYS; i += 256) h[i] = 0;
    __syncthreads();
    unsigned long long pad = 0, used = 0;
    for (uint64_t base = (uint64_t)blockIdx.x * PLAN_PER_BLOCK; base < n; base += (uint64_t)gridDim.x * PLAN_PER_BLOCK) {
        // (all of a round's offsets are requested before any is used: as a load - use - load chain the eight rounds cost eight
        // exposed memory round trips, 25 us per 1M contigs)
        uint64_t o0[PLAN_PER_BLOCK / 256], o1[PLAN_PER_BLOCK / 256];
#pragma unroll
        for (int it = 0; it < PLAN_PER_BLOCK / 256; ++it) {
            const uint64_t c = base + (uint64_t)it * 256 + tid;
            const uint64_t cc = c < n ? c : n - 1;
            o0[it] = offsets[cc];
            o1[it] = offsets[cc + 1];
        }
#pragma unroll
        for (int it = 0; it < PLAN_PER_BLOCK / 256; ++it) {
            const uint64_t c = base + (uint64_t)it * 256 + tid;
            const bool have = c < n;
            uint64_t w = 0;
            if (have) {
                const uint64_t len = o1[it] - o0[it];
                w = len >= (uint64_t)k ? len - k + 1 : 0;
            }
            const unsigned long long wq = (have && w <= long_thr) ? w : 0ull;   // (longer ones leave the slot kernels)
            used += wq;
            unsigned long long mx = wq;
            for (uint32_t sft = 1; sft < gs; sft <<= 1) {
                const unsigned long long o = __shfl_xor(mx, (int)sft);
                mx = o > mx ? o : mx;
            }
            if (have && (c % gs) == 0) pad += (unsigned long long)gs * (((mx + 1023) >> 10) << 10);
            if (sort) {
                // (a batch of similar lengths has ONE key: 256 atomics on one LDS word per round cost this kernel 30 us per 1M
                // contigs -- a wave whose live lanes agree on the key adds their number once)
                const uint32_t np = (have && w > long_thr && piece_w) ? (uint32_t)((w + piece_w - 1) / piece_w) : 1u;
                const uint32_t key = phk_windows_key(phk_piece_windows(w, np, np - 1, piece_w));
                const unsigned long long live = __ballot(have);
                const uint32_t key0 = __builtin_amdgcn_readfirstlane(key);   // (the first ACTIVE lane's: all 64 are active here)
                if (__all(!have || (key == key0 && np == 1)) && (live & 1ull)) {
                    if ((tid & 63) == 0) atomicAdd(&h[key0], (uint32_t)__popcll(live));
                } else if (have) {
                    if (np > 1) atomicAdd(&h[phk_windows_key(piece_w)], np - 1);
                    atomicAdd(&h[key], 1u);
                }
            }
        }
    }
#pragma unroll
    for (int sft = 32; sft > 0; sft >>= 1) {
        pad += __shfl_xor(pad, sft);
        used += __shfl_xor(used, sft);
    }
    if ((tid & 63) == 0) {
        s_pad[tid >> 6] = pad;
        s_used[tid >> 6] = used;
    }
    __syncthreads();
    unsigned long long *stats = reinterpret_cast<unsigned long long *>(ctl + CTL_STATS);
    if (tid == 0) {   // one pair of atomics per workgroup: they all land on one line and retire one after the other
        pad = s_pad[0] + s_pad[1] + s_pad[2] + s_pad[3];
        used = s_used[0] + s_used[1] + s_used[2] + s_used[3];
        if (pad) {
            atomicAdd(stats, pad);
            atomicAdd(stats + 1, used);
        }
    }
    if (sort)
        for (int i = tid; i < SORT_KEYS; i += 256)
            if (h[i]) atomicAdd(ctl + CTL_CURSOR + i, h[i]);
    // ---- the last block to get here finishes the plan.  What the other blocks publish are device-scope atomics only (performed
    // at the memory side); each wave waits for its own to be done, then the block's ticket is drawn: no cache write-back or
    // invalidate is needed on this side (a __threadfence() here cost every block ~4 us), and the reader uses sc1 loads ----
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) s_last = atomicAdd(ctl + CTL_TICKET, 1u) == gridDim.x - 1 ? 1u : 0u;
    __syncthreads();
    if (!s_last || !sort) return;
    const unsigned long long pad_t = __hip_atomic_load(stats, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long used_t = __hip_atomic_load(stats + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (used_t * 10ull >= pad_t * 6ull) return;   // (phk_slots_apply: not ragged -- nobody reads the cursors)
    // cursor[key] = number of items with a LARGER key (descending order: the longest groups start first)
    for (int i = tid; i < SORT_KEYS; i += 256)
        h[i] = __hip_atomic_load(ctl + CTL_CURSOR + (SORT_KEYS - 1 - i), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    if (tid < 64) {   // exclusive scan of 2048 counts by one wave: 32 per lane, then across the lanes
        uint32_t loc = 0;
        for (int i = 0; i < SORT_KEYS / 64; ++i) loc += h[tid * (SORT_KEYS / 64) + i];
        uint32_t inc = loc;
#pragma unroll
        for (int sft = 1; sft < 64; sft <<= 1) {
            const uint32_t o = __shfl_up(inc, sft);
            if (tid >= sft) inc += o;
        }
        uint32_t run = inc - loc;
        for (int i = 0; i < SORT_KEYS / 64; ++i) {
            const uint32_t cnt = h[tid * (SORT_KEYS / 64) + i];
            h[tid * (SORT_KEYS / 64) + i] = run;
            run += cnt;
        }
        if (tid == 63) ctl[CTL_ITEMS] = run;
    }
    __syncthreads();
    for (int i = tid; i < SORT_KEYS; i += 256) ctl[CTL_CURSOR + (SORT_KEYS - 1 - i)] = h[i];
}

// every block reserves, per key, a range for its items with one global atomic, then places them; the row (and window
// count) of a contig that is cut into pieces is zeroed here, ahead of the pieces' atomic adds
__global__ __launch_bounds__(256) void phk_sort_scatter_kernel(const uint64_t *__restrict__ offsets, uint64_t n, int k,
                                                               uint32_t long_thr, uint32_t piece_w,
                                                               const unsigned long long *__restrict__ stats,
                                                               uint32_t *__restrict__ cursor, uint2 *__restrict__ items,
                                                               uint32_t *__restrict__ counts, uint32_t *__restrict__ nwin) {
    if (phk_slots_apply(stats)) return;
    __shared__ uint32_t h[SORT_KEYS];   // per-block count, then the block's base position, per key
    const uint64_t per_block = (n + gridDim.x - 1) / gridDim.x;
    const uint64_t lo = per_block * blockIdx.x, hi = lo + per_block < n ? lo + per_block : n;
    const uint64_t D = 1ull << (2 * k);
    for (int i = threadIdx.x; i < SORT_KEYS; i += blockDim.x) h[i] = 0;
    __syncthreads();
    for (uint64_t c = lo + threadIdx.x; c < hi; c += blockDim.x) {
        uint32_t np;
        const uint64_t w = phk_contig_windows(offsets, c, k, long_thr, piece_w, np);
        if (np > 1) atomicAdd(&h[phk_windows_key(piece_w)], np - 1);
        atomicAdd(&h[phk_windows_key(phk_piece_windows(w, np, np - 1, piece_w))], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < SORT_KEYS; i += blockDim.x)
        if (h[i]) h[i] = atomicAdd(cursor + i, h[i]);
    __syncthreads();
    for (uint64_t c = lo + threadIdx.x; c < hi; c += blockDim.x) {
        uint32_t np;
        const uint64_t w = phk_contig_windows(offsets, c, k, long_thr, piece_w, np);
        for (uint32_t pc = 0; pc < np; ++pc)
            items[atomicAdd(&h[phk_windows_key(phk_piece_windows(w, np, pc, piece_w))], 1u)] = make_uint2((uint32_t)c, pc);
        if (np > 1) {
            uint4 *row = reinterpret_cast<uint4 *>(counts + c * D);
            for (uint64_t i = 0; i < D / 4; ++i) row[i] = make_uint4(0, 0, 0, 0);
            if (nwin) nwin[c] = 0;
        }
    }
}

// ------------------------------------------------------------------------------------
// The slot kernels: one histogram COLUMN per contig.
//
// The wave-per-contig kernel (count_wave.hip) is bound by LDS bank conflicts: its 64 lanes add into ONE histogram, so a wave-wide
// ds_add lands on random banks (about 7.7 LDS cycles per instruction at the best replication,
// profiles/r01/count_lds_study.md), and replicas have to be summed again at the flush.  In the kernels below the 32
// histograms in a workgroup's LDS belong to 32 DIFFERENT contigs,
//     bins[code][slot]   (slot = lane & 31, so the LDS bank of an add is its lane's slot, whatever the code)
// every ds_add is conflict free (2 LDS cycles per wave instruction), there is nothing to reduce at the flush, and the
// address of a bin costs two VALU operations: ((word >> s) & (D-1) << 7) | slot * 4.  k = 5: 16 contigs per workgroup
// (a 1024-bin column set of 32 would not fit; bank = slot + 16 (code & 1): 3 LDS cycles per instruction on average).
// A lane reads its 64-base units straight from memory (the vector cache serves the other lanes' pieces of a line) and no
// wave waits for another before the flush.  In a batch of similar lengths the few contigs much longer than the mean are
// appended to `long_list` for the wave-per-contig kernel, which follows; a ragged batch is walked as a sorted list of
// (contig, piece) items, a long contig being cut into pieces that are columns like any other.
// ------------------------------------------------------------------------------------

// ------------------------------------------------------------------------------------
// TWO WINDOWS PER ADD (k = 4, no validity mask, batches the statistics do not call ragged; round 4).
// The slot kernel above is bound by the CU's LDS adder: one conflict-free wave-wide ds_add_u32 per ~4-6 cycles, one add per
// window (tools/micro/lds_add_rate.hip).  Two consecutive windows -- the 4-mers at bases p and p + 1 -- are
// one 5-mer (bases p .. p + 4): its upper 8 bits are the first window's code, its lower 8 bits the second's.  So the
// contig's windows are taken in PAIRS (p = first base, + 2, + 4, ..), each pair is ONE add into a histogram of stride-2
// 5-mers, and the 4-mer counts are that histogram's two marginals, formed at the flush:
//     count4[x] = sum_b n5[4 x + b]  +  sum_a n5[256 a + x]          (+ 1 for the last window of a contig with an odd number)
// The 1024 5-mer bins are 16-bit halves of 512 words -- bins[code5 >> 1][slot], increment 1 << 16 (code5 & 1) -- 64 KiB for
// 32 contigs; a half holds at most W / 2 <= 65 535 (longer contigs are handed on, as the slot kernel hands on its long
// ones).  Pairs are aligned to the CONTIG's first base: a contig that starts on an odd base has its words
// re-aligned by one base (v_alignbit + v_cndmask per word), after which every shift is an immediate as in the slot
// kernel.  Per add: 2 address operations + 2 for the increment, i.e. the slot kernel's VALU work per window and half its
// LDS adds; the flush reads every bin word twice (4 LDS reads per 4-mer instead of 1).
// ------------------------------------------------------------------------------------
template <int NTH>
__global__ __launch_bounds__(NTH) void phk_count_pairs_kernel(const uint32_t *__restrict__ packed, const uint64_t *__restrict__ offsets,
                                                             uint64_t n, uint64_t max_word, uint32_t long_thr,
                                                             uint32_t *__restrict__ counts, uint32_t *__restrict__ nwin,
                                                             uint2 *__restrict__ long_list, uint32_t *__restrict__ long_count,
                                                             uint32_t piece_w) {
    constexpr int K = 4;
    constexpr uint32_t D = 256, NWORD = 512;   // 4-mer bins of a row; pair words of a histogram column
    constexpr int SLOTS = 32;
    constexpr int PARTS = NTH / SLOTS;      // lanes per contig
    constexpr int XPT = (int)D / PARTS;     // 4-mer codes a thread flushes
    static_assert(XPT % 4 == 0, "flush geometry");
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];  // bins [NWORD][SLOTS] | single [SLOTS]
    uint32_t *single_s = lds + NWORD * SLOTS;
    if (!phk_slots_apply(reinterpret_cast<const unsigned long long *>(long_count + CTL_STATS))) return;   // ragged: the sorted slot kernel's
    const int t = threadIdx.x;
    const int slot = t & (SLOTS - 1), part = t / SLOTS;
    for (uint32_t b = t * 4; b < NWORD * SLOTS; b += 4 * NTH) *reinterpret_cast<uint4 *>(lds + b) = make_uint4(0, 0, 0, 0);
    __syncthreads();
    const uint32_t colb = (uint32_t)slot * 4u;
    const uint32_t pthr = long_thr < 131070u ? long_thr : 131070u;   // a 16-bit half holds W / 2
    typedef __attribute__((address_space(3))) uint32_t lds_u32;
    // the pair whose 5-mer starts at base o (even, <= 8) of `src`: bin word (code5 >> 1) at bits [15:7] of the byte address,
    // increment 1 or 65536 by the 5-mer's last bit
    auto pair_addr = [&](uint32_t src, int o) { return (lds_u32 *)(uintptr_t)(((src >> (16 - 2 * o)) & (0x1FFu << 7)) | colb); };
    auto pair_inc = [&](uint32_t src, int o) {   // (bfe + mad: hipcc turns the C form into and + compare + select)
        uint32_t bit, inc;
        asm("v_bfe_u32 %0, %1, %2, 1" : "=v"(bit) : "v"(src), "n"(22 - 2 * o));
        asm("v_mad_u32_u24 %0, %1, %2, 1" : "=v"(inc) : "v"(bit), "v"(65535u));
        return inc;
    };
#if defined(PHK_DIAGNOSTIC_BUILD) && defined(PAIRS_ABL) && PAIRS_ABL == 1   // timing only: no LDS adds (the operands are kept alive)
    auto add1 = [&](lds_u32 *p, uint32_t val) { asm volatile("" ::"v"(p), "v"(val)); };
#else
    auto add1 = [&](lds_u32 *p, uint32_t val) { __hip_atomic_fetch_add(p, val, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); };
#endif
    const uint64_t wlast = max_word + 1;   // the pad word: the last one that exists

    for (uint64_t batch = blockIdx.x; batch * SLOTS < n; batch += gridDim.x) {
        const uint64_t c = batch * SLOTS + slot;
        const bool have = c < n;
        const uint64_t st = have ? offsets[c] : 0;
        const uint64_t en = have ? offsets[c + 1] : 0;
        const uint64_t len = en - st;
        uint32_t W = len >= (uint64_t)K ? (uint32_t)((len - K + 1) < 0xFFFFFFFFull ? (len - K + 1) : 0xFFFFFFFFull) : 0;
        const bool handed_over = W > pthr;
        if (handed_over) {
            if (part == 0) {
                const uint32_t np = piece_w ? (W + piece_w - 1) / piece_w : 1u;
                const uint32_t base = atomicAdd(long_count, np);
                for (uint32_t pc = 0; pc < np; ++pc) long_list[base + pc] = make_uint2((uint32_t)c, pc);
            }
            W = 0;
        }
        const uint32_t par = (uint32_t)st & 1u;
        const uint32_t npair = W >> 1;
        // Units of four words (64 bases, 32 pairs), aligned in the stream; lane `part` of the contig takes units part, part +
        // PARTS, ..  No staging and no barrier until the flush: a lane reads its words straight from memory (the vector
        // cache serves the other lanes' pieces of a line).  Positions relative to the contig's first unit fit 32 bits
        // (W <= 131 070).
        const uint64_t U0 = st >> 6;
        const uint32_t rst = (uint32_t)(st - (U0 << 6));                 // the contig's first base
        const uint32_t rPL = rst + 2u * npair - 2u;                      // first base of its last pair (npair > 0)
        const uint32_t nunit = npair ? (rPL >> 6) + 1u : 0u;
        const uint32_t *pc = packed + 4 * U0;                            // the contig's first unit
        // the word after a unit is read only where the stream still has one (its bases are needed only then)
        const uint32_t wlim = (uint32_t)((wlast - 4 * U0) < 0x7FFFFFFFull ? (wlast - 4 * U0) : 0x7FFFFFFFull);
        if (part == 0) {   // the unpaired last window of a contig with an odd number of them
            uint32_t sg = 0xFFFFFFFFu;
            if (W & 1u) {
                const uint64_t lb = st + W - 1, wl = lb >> 4;
                const uint64_t f = ((uint64_t)packed[wl] << 32) | packed[wl + 1];
                sg = (uint32_t)(f >> (56 - 2 * (uint32_t)(lb & 15))) & 0xFFu;
            }
            single_s[slot] = sg;
        }
        auto load5 = [&](uint32_t j, uint32_t (&w)[5]) {
            const uint32_t w0 = 4u * j;
            if (w0 + 3 <= wlim) {
                const uint4 a = *reinterpret_cast<const uint4 *>(pc + w0);
                w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w;
            } else {   // the last words of the whole stream
                w[0] = pc[w0]; w[1] = pc[w0 + 1 < wlim ? w0 + 1 : wlim]; w[2] = pc[w0 + 2 < wlim ? w0 + 2 : wlim]; w[3] = pc[wlim];
            }
            w[4] = pc[w0 + 4 < wlim ? w0 + 4 : wlim];
        };
        uint32_t cur[5] = {0, 0, 0, 0, 0}, nxt[5] = {0, 0, 0, 0, 0};
        uint32_t j = (uint32_t)part;
        if (j < nunit) load5(j, cur);
        while (__any(j < nunit)) {
            const bool live = j < nunit;
            if (j + PARTS < nunit) load5(j + PARTS, nxt);
            const uint32_t s0 = 64u * j + par;                            // pair i of the unit starts at s0 + 2 i, i < 32
            const bool all = live && s0 >= rst && s0 + 62u <= rPL;
            // the unit's words, re-aligned to the contig's parity (of the fifth only the top bases are used)
            uint32_t sw[5];
#pragma unroll
            for (int i = 0; i < 4; ++i) sw[i] = par ? __builtin_amdgcn_alignbit(cur[i], cur[i + 1], 30) : cur[i];
            sw[4] = par ? cur[4] << 2 : cur[4];
            if (!__any(live && !all)) {   // wave-uniform: every live lane's unit is interior to its contig
                if (all) {
#pragma unroll
                    for (int wd = 0; wd < 4; ++wd) {
                        const uint32_t y = sw[wd], u = __builtin_amdgcn_alignbit(y, sw[wd + 1], 16);
#pragma unroll
                        for (int jp = 0; jp < 8; ++jp) {   // pairs at bases 0, 2, .., 8 of y and 10, 12, 14 = 2, 4, 6 of u
                            const uint32_t src = jp < 5 ? y : u;
                            const int o = jp < 5 ? 2 * jp : 2 * jp - 8;
                            add1(pair_addr(src, o), pair_inc(src, o));
                        }
                    }
                }
            } else if (live) {            // a lane at an edge of its contig: the pair's bit times the increment
                const uint32_t ilo = rst > s0 ? (rst - s0) >> 1 : 0u;
                const uint32_t ihi = (rPL - s0) >> 1 < 31u ? (rPL - s0) >> 1 : 31u;
                const uint32_t pm = (ihi - ilo == 31u) ? ~0u : (((1u << (ihi - ilo + 1)) - 1u) << (31 - ihi));   // bit 31 - i: pair i is counted
#pragma unroll
                for (int wd = 0; wd < 4; ++wd) {
                    const uint32_t y = sw[wd], u = __builtin_amdgcn_alignbit(y, sw[wd + 1], 16);
#pragma unroll
                    for (int jp = 0; jp < 8; ++jp) {
                        const uint32_t src = jp < 5 ? y : u;
                        const int o = jp < 5 ? 2 * jp : 2 * jp - 8;
                        add1(pair_addr(src, o), pair_inc(src, o) * __builtin_amdgcn_ubfe(pm, 31 - (8 * wd + jp), 1));
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < 5; ++i) cur[i] = nxt[i];
            j += PARTS;
        }
        phk_lds_barrier();  // every wave's adds (and the single windows) have landed
        // ---- flush: thread (slot, g) forms the 4-mer counts x in [g XPT, (g + 1) XPT) of contig `slot` from the two marginals ----
        {
            const uint32_t x0 = (uint32_t)part * XPT;
            uint32_t out[XPT];
            const uint32_t *col = lds + slot;
            // (v_sad_u16 with a zero operand adds both halves of a word onto an accumulator; v_mad_u32_u16 x 1 one half, chosen
            // by op_sel: the unpacking costs no instruction of its own)
#pragma unroll
            for (int i = 0; i < XPT; ++i) {                    // first window of the pair: 5-mers 4 x .. 4 x + 3 = words 2 x, 2 x + 1
                const uint32_t w0 = col[(2 * (x0 + i)) * SLOTS], w1 = col[(2 * (x0 + i) + 1) * SLOTS];
                out[i] = __builtin_amdgcn_sad_u16(w1, 0u, __builtin_amdgcn_sad_u16(w0, 0u, 0u));
            }
            const uint32_t one = 1u;
#pragma unroll
            for (int mm = 0; mm < XPT / 2; ++mm)               // second window: 5-mers 256 a + x = half x & 1 of word 128 a + x / 2
#pragma unroll
                for (int a = 0; a < 4; ++a) {
                    const uint32_t w = col[(128 * a + x0 / 2 + mm) * SLOTS];
                    asm("v_mad_u32_u16 %0, %1, %2, %0" : "+v"(out[2 * mm]) : "v"(w), "v"(one));
                    asm("v_mad_u32_u16 %0, %1, %2, %0 op_sel:[1,0,0,0]" : "+v"(out[2 * mm + 1]) : "v"(w), "v"(one));
                }
            const uint32_t sg = single_s[slot];
#pragma unroll
            for (int i = 0; i < XPT; ++i) out[i] += (sg == x0 + i) ? 1u : 0u;
            phk_lds_barrier();   // every thread has read what it needs: the columns may be cleared
            uint32_t *zc = lds + (2 * x0) * SLOTS + slot;
#pragma unroll
            for (int i = 0; i < 2 * XPT; ++i) zc[i * SLOTS] = 0;
            uint32_t *rowo = counts + c * D + x0;
#if defined(PHK_DIAGNOSTIC_BUILD) && defined(PAIRS_ABL) && PAIRS_ABL == 2   // timing only: rows are stored for one batch in 64
            if (have && (!handed_over || piece_w) && (batch & 63) == 0) {
#else
            if (have && (!handed_over || piece_w)) {           // (a contig handed over in pieces gets its zero row here)
#endif
#pragma unroll
                for (int i = 0; i < XPT / 4; ++i)
                    *reinterpret_cast<uint4 *>(rowo + 4 * i) = make_uint4(out[4 * i], out[4 * i + 1], out[4 * i + 2], out[4 * i + 3]);
            }
            if (nwin && have && part == 0 && (!handed_over || piece_w)) nwin[c] = W;
        }
        phk_lds_barrier();   // the columns are clear and single_s may be rewritten
    }
}

// ------------------------------------------------------------------------------------
// The slot kernel WITHOUT staging and stage barriers (k = 5, no validity mask, batches the statistics do not call ragged;
// round 4): what made the two-windows-per-add kernel above fast was, as much as its halved adds, that a lane reads its
// words straight from memory and no wave waits for another before the flush.  The bins described above
// (bins[code][slot], 16 contigs per workgroup at k = 5), one add per window, 64 windows per lane and round.
// ------------------------------------------------------------------------------------
template <int K, int SLOTS, int NTH, bool MASK, bool ORDERED>
__global__ __launch_bounds__(NTH) void phk_count_direct_kernel(const uint32_t *__restrict__ packed, const uint32_t *__restrict__ mask,
                                                              const uint64_t *__restrict__ offsets,
                                                              uint64_t n, uint64_t max_word, uint32_t long_thr,
                                                              uint32_t *__restrict__ counts, uint32_t *__restrict__ nwin,
                                                              uint2 *__restrict__ long_list, uint32_t *__restrict__ long_count,
                                                              const uint2 *__restrict__ order,   // sorted (contig, piece) items of a ragged batch, or NULL
                                                              uint32_t piece_w,
                                                              uint32_t skip_plain,             // 1: a batch that is not ragged is another kernel's (pairs)
                                                              uint4 *__restrict__ frag8,      // the scorer's int8 operand (PhkPrep8), or NULL
                                                              uint32_t *__restrict__ big8) {
    constexpr uint32_t D = 1u << (2 * K);
    constexpr int PARTS = NTH / SLOTS;      // lanes per contig
    constexpr int XPT = (int)D / PARTS;     // codes a thread flushes
    constexpr int SHB = SLOTS == 32 ? 7 : 6;  // log2 of a bin row in bytes
    static_assert(XPT % 4 == 0 && K <= 5, "flush geometry / window fits the funnel");
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];  // bins [D][SLOTS] | counted windows [SLOTS] | piece owner [SLOTS]
    uint32_t *nwin_s = lds + D * SLOTS;
    uint32_t *split_s = nwin_s + SLOTS;
    // Two instances are launched back to back and decide on the device which of them counts the batch: the plain walk
    // (ORDERED = false) when the statistics allow it, else the sorted work list (ORDERED = true).
    // The plain instance carries none of the sorted walk's code: with it the k = 5 kernel ran 15 % slower.
    const bool plain = phk_slots_apply(reinterpret_cast<const unsigned long long *>(long_count + CTL_STATS));
    if (ORDERED) {
        if (plain || !order) return;
        n = long_count[CTL_ITEMS];   // items, counted by the sort kernels
        frag8 = nullptr;
        big8 = nullptr;
    } else {
        if (!plain) {
            if (big8 && blockIdx.x == 0 && threadIdx.x == 0) big8[n] = 2u;   // (nothing prepared for the scorer)
            return;
        }
        if (skip_plain) return;
        order = nullptr;
    }
    const int t = threadIdx.x;
    const int slot = t & (SLOTS - 1), part = t / SLOTS;
    for (uint32_t b = t * 4; b < D * SLOTS; b += 4 * NTH) *reinterpret_cast<uint4 *>(lds + b) = make_uint4(0, 0, 0, 0);
    if (t < SLOTS) nwin_s[t] = 0;
    __syncthreads();
    const uint32_t colb = (uint32_t)slot * 4u;
    typedef __attribute__((address_space(3))) uint32_t lds_u32;
    auto bin = [&](uint32_t src, int o) {   // the window starting at base o (< 8) of `src`
        constexpr uint32_t msk = (D - 1u) << SHB;
        const int sh = 32 - 2 * K - 2 * o - SHB;
        return (lds_u32 *)(uintptr_t)(((src >> sh) & msk) | colb);
    };
    auto add1 = [&](lds_u32 *p, uint32_t val) { __hip_atomic_fetch_add(p, val, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); };
    const uint64_t wlast = max_word + 1;   // the pad word: the last one that exists
    const uint64_t mlast = (max_word >> 1) + 1;   // last mask word that exists (ceil(T / 32) + 1 words)

    for (uint64_t batch = blockIdx.x; batch * SLOTS < n; batch += gridDim.x) {
        const uint64_t ci = batch * SLOTS + slot;
        const bool have = ci < n;
        const uint2 item = (ORDERED && have) ? order[ci] : make_uint2(0, 0);
        const uint64_t c = have ? (ORDERED ? (uint64_t)item.x : ci) : 0;
        uint64_t st = have ? offsets[c] : 0;
        const uint64_t en = have ? offsets[c + 1] : 0;
        const uint64_t len = en - st;
        uint32_t W = len >= (uint64_t)K ? (uint32_t)((len - K + 1) < 0xFFFFFFFFull ? (len - K + 1) : 0xFFFFFFFFull) : 0;
        // an item of the sorted work list is a whole contig or one piece of a long one: the piece's windows start at
        // st + piece * piece_w, and its histogram is added onto the contig's row (zeroed by the sort) at the flush
        const bool split = ORDERED && piece_w && W > long_thr;
        if (split) {
            const uint64_t first = (uint64_t)item.y * piece_w;
            st += first;
            W = (uint32_t)((uint64_t)W - first < piece_w ? (uint64_t)W - first : piece_w);
        }
        const bool handed_over = !ORDERED && W > long_thr;
        if (ORDERED && part == 0) split_s[slot] = split ? (uint32_t)c + 1u : 0u;
        if (handed_over) {
            if (part == 0) {
                const uint32_t np = piece_w ? (W + piece_w - 1) / piece_w : 1u;
                const uint32_t base = atomicAdd(long_count, np);
                for (uint32_t pc = 0; pc < np; ++pc) long_list[base + pc] = make_uint2((uint32_t)c, pc);
            }
            W = 0;
        }
        // units of four words (64 windows), aligned in the stream; positions relative to the contig's first unit
        const uint64_t U0 = st >> 6;
        const uint32_t rst = (uint32_t)(st - (U0 << 6));
        const uint64_t rlast64 = (uint64_t)rst + W - 1;                  // the last window (W > 0)
        const uint32_t rlast = rlast64 < 0xFFFFFFC0ull ? (uint32_t)rlast64 : 0xFFFFFFC0u;   // (long_thr / piece_w keep W far below this)
        const uint32_t nunit = W ? (rlast >> 6) + 1u : 0u;
        const uint32_t *pc = packed + 4 * U0;
        const uint32_t wlim = (uint32_t)((wlast - 4 * U0) < 0x7FFFFFFFull ? (wlast - 4 * U0) : 0x7FFFFFFFull);
        const uint32_t *pm = MASK ? mask + 2 * U0 : nullptr;            // validity words of the first unit (2 per unit + the next)
        const uint32_t mlim = MASK ? (uint32_t)((mlast - 2 * U0) < 0x7FFFFFFFull ? (mlast - 2 * U0) : 0x7FFFFFFFull) : 0u;
        auto load5 = [&](uint32_t j, uint32_t (&w)[5], uint32_t (&mk)[3]) {
            const uint32_t w0 = 4u * j;
            if (w0 + 3 <= wlim) {
                const uint4 a = *reinterpret_cast<const uint4 *>(pc + w0);
                w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w;
            } else {   // the last words of the whole stream
                w[0] = pc[w0]; w[1] = pc[w0 + 1 < wlim ? w0 + 1 : wlim]; w[2] = pc[w0 + 2 < wlim ? w0 + 2 : wlim]; w[3] = pc[wlim];
            }
            w[4] = pc[w0 + 4 < wlim ? w0 + 4 : wlim];
            if (MASK) {
#pragma unroll
                for (int i = 0; i < 3; ++i) mk[i] = pm[2 * j + i < mlim ? 2 * j + i : mlim];
            }
        };
        uint32_t cur[5] = {0, 0, 0, 0, 0}, nxt[5] = {0, 0, 0, 0, 0}, mcur[3] = {0, 0, 0}, mnxt[3] = {0, 0, 0};
        uint32_t cnt_ok = 0;
        uint32_t j = (uint32_t)part;
        if (j < nunit) load5(j, cur, mcur);
        while (__any(j < nunit)) {
            const bool live = j < nunit;
            if (j + PARTS < nunit) load5(j + PARTS, nxt, mnxt);
            const uint32_t fb = 64u * j;                                  // window i of the unit starts at fb + i
            bool all = live && fb >= rst && fb + 63u <= rlast;
            uint64_t wv = 0;                                              // bit 63 - i: window i is counted
            if (MASK ? live : (live && !all)) {   // (without a mask only the units at a contig's edges need their window bits)
                const uint32_t lo = rst > fb ? rst - fb : 0u;
                const uint32_t hi = rlast - fb < 63u ? rlast - fb : 63u;
                wv = (hi - lo == 63u) ? ~0ull : (((1ull << (hi - lo + 1)) - 1ull) << (63 - hi));
                if (MASK) {
                    const uint64_t vb = ((uint64_t)mcur[0] << 32) | mcur[1];   // bit 63 - i: base i of the unit valid
                    uint64_t w = vb;
#pragma unroll
                    for (int jj = 1; jj < K; ++jj) w &= (vb << jj) | ((uint64_t)mcur[2] >> (32 - jj));
                    wv &= w;
                    all = all && w == ~0ull;
                    cnt_ok += (uint32_t)__popcll(wv);
                }
            }
            if (!__any(live && !all)) {   // wave-uniform: every live lane's unit is interior to its contig (and all valid)
                if (all) {
#pragma unroll
                    for (int wd = 0; wd < 4; ++wd) {
                        const uint32_t y = cur[wd], u = __builtin_amdgcn_alignbit(y, cur[wd + 1], 16);
#pragma unroll
                        for (int jw = 0; jw < 16; ++jw) add1(bin(jw < 8 ? y : u, jw & 7), 1u);
                    }
                }
            } else if (live) {            // a lane at an edge of its contig / with an invalid base: the window's bit instead of 1
                if (!MASK && all) wv = ~0ull;   // (an interior unit in a wave that has an edge unit elsewhere)
                const uint32_t vhi = (uint32_t)(wv >> 32), vlo = (uint32_t)wv;
#pragma unroll
                for (int wd = 0; wd < 4; ++wd) {
                    const uint32_t y = cur[wd], u = __builtin_amdgcn_alignbit(y, cur[wd + 1], 16);
#pragma unroll
                    for (int jw = 0; jw < 16; ++jw) {
                        const int wi = 16 * wd + jw;
                        add1(bin(jw < 8 ? y : u, jw & 7), __builtin_amdgcn_ubfe(wi < 32 ? vhi : vlo, 31 - (wi & 31), 1));
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < 5; ++i) cur[i] = nxt[i];
            if (MASK) {
#pragma unroll
                for (int i = 0; i < 3; ++i) mcur[i] = mnxt[i];
            }
            j += PARTS;
        }
        if (MASK && cnt_ok) atomicAdd(nwin_s + slot, cnt_ok);
        phk_lds_barrier();  // every wave's adds have landed
        // ---- pieces first: wave w adds the columns of slots w, w + NTH / 64, .. onto their contigs' rows, 64 consecutive codes per
        // instruction (coalesced global atomics)
        if (ORDERED) {
            for (int sl = t >> 6; sl < SLOTS; sl += NTH / 64) {
                const uint32_t cs = split_s[sl];
                if (!cs) continue;
                uint32_t *rowp = counts + (uint64_t)(cs - 1u) * D;
                for (uint32_t code = (uint32_t)(t & 63); code < D; code += 64) {
                    const uint32_t v = lds[code * SLOTS + sl];
                    if (v) atomicAdd(rowp + code, v);
                }
            }
            phk_lds_barrier();
        }
        {   // flush: thread (slot, g) writes codes [g XPT, (g + 1) XPT) of contig `slot` and clears them
            uint32_t *cellb = lds + ((uint32_t)part * XPT) * SLOTS + slot;
            uint32_t *rowo = counts + c * D + (uint32_t)part * XPT;
            const uint32_t Wc = MASK ? nwin_s[slot] : W;   // counted windows = the row sum
            // ... and, for the scorer's int8 sweep (score_i8.hip), the same codes as int8 around the row's centre in fragment
            // order: piece (k-step s = dims / 32, half h) of query c at [(c / 32) (D / 32) + s][32 h + c % 32]
            const int cen = (int)phk_row_center(Wc, D);
            uint32_t mx = 0, l1 = 0;
            constexpr int PZ = XPT >= 16 ? XPT / 16 : 1, CPZ = XPT >= 16 ? 4 : XPT / 4;   // 16-code pieces per thread, uint4 loads per piece
#pragma unroll
            for (uint32_t pz = 0; pz < (uint32_t)PZ; ++pz) {
                uint32_t pk[4] = {0, 0, 0, 0};
#pragma unroll
                for (uint32_t i = 0; i < (uint32_t)CPZ; ++i) {
                    uint32_t *cell = cellb + (16 * pz + 4 * i) * SLOTS;
                    const uint4 o = make_uint4(cell[0], cell[SLOTS], cell[2 * SLOTS], cell[3 * SLOTS]);
                    cell[0] = 0; cell[SLOTS] = 0; cell[2 * SLOTS] = 0; cell[3 * SLOTS] = 0;
                    // (a contig handed over in pieces gets its zero row here: the pieces are added onto it atomically)
                    if (!split && have && (!handed_over || piece_w)) *reinterpret_cast<uint4 *>(rowo + 16 * pz + 4 * i) = o;
                    if (XPT >= 16) {
                        const uint32_t cc[4] = {o.x, o.y, o.z, o.w};
                        uint32_t word = 0;
#pragma unroll
                        for (int b = 0; b < 4; ++b) {
                            const int d = (int)cc[b] - cen;
                            const uint32_t ad = (uint32_t)(d < 0 ? -d : d);
                            mx = max(mx, ad);
                            l1 += min(ad, 127u);
                            const int q = d < -127 ? -127 : (d > 127 ? 127 : d);
                            word |= ((uint32_t)q & 0xFFu) << (8 * b);
                        }
                        pk[i] = word;
                    }
                }
                if (XPT >= 16 && frag8 && have && !handed_over) {
                    const uint32_t dim16 = (uint32_t)part * PZ + pz;   // which 16 dimensions of the row
                    frag8[((c >> 5) * (D / 32) + (dim16 >> 1)) * 64 + 32u * (dim16 & 1u) + (uint32_t)(c & 31)] = make_uint4(pk[0], pk[1], pk[2], pk[3]);
                }
            }
            if (big8 && have) {
                if (handed_over) {   // counted later, in pieces: the scorer's own fragment kernel takes this row
                    if (part == 0) {
                        big8[c] = PHK_PREP8_MISSING;
                        atomicOr(big8 + n, 1u);
                    }
                } else {
                    if (mx > 127u) atomicOr(big8 + c, 0x80000000u);
                    if (2ull * Wc + D > PHK_I8_L1_MAX) atomicAdd(big8 + c, l1);
                }
            }
            if (nwin && have && part == 0) {
                if (split) atomicAdd(nwin + c, Wc);
                else if (!handed_over || piece_w) nwin[c] = Wc;
            }
        }
        phk_lds_barrier();
        if (MASK) {
            if (t < SLOTS) nwin_s[t] = 0;
            phk_lds_barrier();
        }
    }
}

// ------------------------------------------------------------------------------------
// The instances, named once: what phk_count_init_device prepares is what the launchers below pick from.
// ------------------------------------------------------------------------------------
typedef void (*PairsKern)(const uint32_t *, const uint64_t *, uint64_t, uint64_t, uint32_t, uint32_t *, uint32_t *, uint2 *, uint32_t *,
                          uint32_t);
typedef void (*DirectKern)(const uint32_t *, const uint32_t *, const uint64_t *, uint64_t, uint64_t, uint32_t, uint32_t *, uint32_t *,
                           uint2 *, uint32_t *, const uint2 *, uint32_t, uint32_t, uint4 *, uint32_t *);
struct PairsShape {
    unsigned threads;
    PairsKern kern;
};
struct DirectShape {
    int k;
    unsigned slots, threads;
    DirectKern kern[2][2];   // [mask][ordered]
};
#define DIRECT_SHAPE(K_, S_, T_)                                                                                  \
    {K_, S_, T_, {{phk_count_direct_kernel<K_, S_, T_, false, false>, phk_count_direct_kernel<K_, S_, T_, false, true>}, \
                  {phk_count_direct_kernel<K_, S_, T_, true, false>, phk_count_direct_kernel<K_, S_, T_, true, true>}}}
static const PairsShape PAIRS_SHAPES[] = {{512, phk_count_pairs_kernel<512>}, {1024, phk_count_pairs_kernel<1024>}};
static const DirectShape DIRECT_SHAPES[] = {DIRECT_SHAPE(3, 32, 512), DIRECT_SHAPE(4, 32, 512), DIRECT_SHAPE(4, 32, 1024),
                                            DIRECT_SHAPE(5, 16, 512), DIRECT_SHAPE(5, 16, 1024)};
#undef DIRECT_SHAPE

// Per-device set-up, called from phk_create with the context's device current: raise the dynamic LDS limit of every
// slot kernel instance and verify that it has no static LDS -- its bin addresses are
// formed as integers on the assumption that the dynamic array starts at LDS address 0.  If a toolchain ever lays
// the kernel out differently the slot kernel is simply not used on this context (the wave-per-contig kernel
// serves every k): a host-side refusal instead of a device-side abort.
static int slots_instance_init(const void *kern, bool *ok) {
    PHK_HIP(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024));
    hipFuncAttributes fa;
    PHK_HIP(hipFuncGetAttributes(&fa, kern));
    if (fa.sharedSizeBytes != 0) *ok = false;
    return PHK_OK;
}

int phk_count_init_device(phk_ctx *ctx) {
    bool ok = true;
    for (const PairsShape &p : PAIRS_SHAPES) PHK_TRY(slots_instance_init((const void *)p.kern, &ok));
    for (const DirectShape &d : DIRECT_SHAPES)
        for (int i = 0; i < 4; ++i) PHK_TRY(slots_instance_init((const void *)d.kern[i >> 1][i & 1], &ok));
    ctx->slots_lds0 = ok;
    return PHK_OK;
}

// ------------------------------------------------------------------------------------
// Launchers: each launches what the route (count_route, count_shared.h) says, with the pointers the driver carved.
// ------------------------------------------------------------------------------------
// `link`: the words a caller's next stage wants zeroed beside the next call's control block (PhkStepLink)
int phk_launch_count_plan(phk_ctx *ctx, const CountRoute &r, const CountCall &c, const PhkStepLink *link) {
    PHK_LAUNCH(ctx, "phk_count_plan_kernel",
               phk_count_plan_kernel<<<dim3(r.plan_blocks), dim3(256), 0, ctx->stream>>>(
                   c.offsets, r.plan_n, r.k, r.slots, r.long_thr, r.piece_w, r.sorted ? 1 : 0, c.ctl, c.ctl_next,
                   link ? link->zero[0] : nullptr, link ? link->zero_words[0] : 0u, link ? link->zero[1] : nullptr,
                   link ? link->zero_words[1] : 0u));
    return PHK_OK;
}

// returns at once on the device unless the statistics call the batch ragged
int phk_launch_sort_scatter(phk_ctx *ctx, const CountRoute &r, const CountCall &c) {
    PHK_LAUNCH(ctx, "phk_sort_scatter_kernel",
               phk_sort_scatter_kernel<<<dim3(r.sort_blocks), dim3(256), 0, ctx->stream>>>(
                   c.offsets, r.n, r.k, r.long_thr, r.piece_w, (const unsigned long long *)(c.ctl + CTL_STATS), c.ctl + CTL_CURSOR,
                   c.order, c.counts, c.nwin));
    return PHK_OK;
}

// k = 4 without a validity mask: a batch the statistics do not call ragged is counted two windows per add; the direct
// kernel then only serves the ragged case (both decide on the device)
int phk_launch_count_pairs(phk_ctx *ctx, const CountRoute &r, const CountCall &c) {
    for (const PairsShape &p : PAIRS_SHAPES) {
        if (p.threads != r.pairs_threads) continue;
        PHK_LAUNCH(ctx, "phk_count_pairs_kernel",
                   p.kern<<<dim3(phk_count_grid(ctx, r.pairs_groups, r.pairs_per_cu)), dim3(p.threads), r.pairs_lds, ctx->stream>>>(
                       c.packed, c.offsets, r.n, r.max_word, r.long_thr, c.counts, c.nwin, c.long_list, c.ctl, r.piece_w));
        return PHK_OK;
    }
    phk_set_error("phk_count: no two-windows-per-add kernel of %u threads", r.pairs_threads);
    return PHK_ERR_UNSUPPORTED;
}

// The unstaged slot kernel for everything else the slot path counts: masked batches, the sorted walk of ragged batches,
// k = 3 and k = 5.  Up to two instances, which decide on the device which of them counts the batch: the plain walk unless
// the pairs kernel has it (skip_plain), the ordered walk iff the route is sorted.
// At k = 5 without a mask the plain instance also writes the scorer's int8 operand when phk_count_score_dev offered it for
// this matrix (PhkPrep8): `written` is set here and nowhere else -- this is the one kernel that writes the fragments.
int phk_launch_count_direct(phk_ctx *ctx, const CountRoute &r, const CountCall &c, PhkStepLink *link) {
    const bool prep = r.k == 5 && !r.masked && link && link->prep8.offered && link->prep8.counts == c.counts && link->prep8.n == r.n &&
                      link->prep8.D == 1024;
    uint4 *frag8 = prep ? (uint4 *)link->prep8.frag : nullptr;
    uint32_t *big8 = prep ? link->prep8.big : nullptr;
    if (link) link->prep8.written = prep;
    for (const DirectShape &d : DIRECT_SHAPES) {
        if (d.k != r.k || d.threads != r.direct_threads) continue;
        const unsigned blocks = phk_count_grid(ctx, r.direct_groups, r.direct_per_cu);
        for (int ordered = 0; ordered < 2; ++ordered) {
            if (ordered ? !r.sorted : r.skip_plain) continue;   // (skip_plain: the pairs kernel's, launched before)
            PHK_LAUNCH(ctx, "phk_count_direct_kernel",
                       d.kern[r.masked][ordered]<<<dim3(blocks), dim3(d.threads), r.direct_lds, ctx->stream>>>(
                           c.packed, c.mask, c.offsets, r.n, r.max_word, r.long_thr, c.counts, c.nwin, c.long_list, c.ctl, c.order,
                           r.piece_w, r.skip_plain ? 1u : 0u, frag8, big8));
        }
        return PHK_OK;
    }
    phk_set_error("phk_count: no slot kernel for k = %d with %u threads", r.k, r.direct_threads);
    return PHK_ERR_UNSUPPORTED;
}
