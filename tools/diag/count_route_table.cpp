// count_route_table.cpp -- prints the route of phk_launch_count (count_route, csrc/count_shared.h: pure host code) for a grid of
// (count_lanes, k, masked, n, T, count_sort), the edges included: T = 1024 / 1025, n = 2^32 - 1 / 2^32, long_thr saturating.
// A stand-alone program, meant to be built with the host sanitizers and run on any machine (no GPU is touched):
//   hipcc -x hip --offload-arch=gfx950 -O1 -g -Xarch_host -fsanitize=address,undefined tools/diag/count_route_table.cpp -o count_route_table
// Grids are printed for a device of 256 CUs.
#include "../../phamers_amd/csrc/count_shared.h"

static void row(char lanes, int k, bool masked, uint64_t n, uint64_t T, bool sort, uint64_t mean_bases = 0) {
    PhkKnobs knobs;
    knobs.count_lanes = phk_count_lanes_of(lanes);
    knobs.count_sort = sort;
    phk_ctx ctx;
    const CountRoute r = count_route(knobs, true, k, masked, n, T, mean_bases);
    printf("| %c | %d | %d | %llu | %llu | %d | ", lanes ? lanes : '-', k, (int)masked, (unsigned long long)n, (unsigned long long)T, (int)sort);
    if (!r.slot_path) {
        printf("wave only | | | | | | | |\n");
        return;
    }
    char pairs[64] = "-", direct[96];
    if (r.pairs_threads)
        snprintf(pairs, sizeof(pairs), "%u x %u, %zu B", phk_count_grid(&ctx, r.pairs_groups, r.pairs_per_cu), r.pairs_threads, r.pairs_lds);
    const int plain = !r.skip_plain, ordered = r.sorted;
    snprintf(direct, sizeof(direct), "%u x %u, %zu B, %s%s%s", phk_count_grid(&ctx, r.direct_groups, r.direct_per_cu), r.direct_threads,
             r.direct_lds, plain ? "plain" : "", plain && ordered ? " + " : "", ordered ? "ordered" : (plain ? "" : "none"));
    printf("%u | %d%d | %u | %u | %llu | %u (n = %llu) / %u | %s | %s |\n", r.slots, (int)r.forced, (int)r.sorted, r.piece_w, r.long_thr,
           (unsigned long long)r.max_items, r.plan_blocks, (unsigned long long)r.plan_n, r.sort_blocks, pairs, direct);
}

int main() {
    printf("| lanes | k | masked | n | T | count_sort | slots | forced, sorted | piece_w | long_thr | max_items | plan (n) / sort blocks | pairs: grid x threads, LDS | direct: grid x threads, LDS, instances |\n");
    printf("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|\n");
    const uint64_t n = 1000000, T = 5000000000ull;
    for (int k = 1; k <= 7; ++k) row(0, k, false, n, T, true);
    for (int k = 3; k <= 5; ++k) row(0, k, true, n, T, true);
    for (const char *c = "0fpPqQdD2"; *c; ++c) row(*c, 4, false, n, T, true);
    for (const char *c = "dDp"; *c; ++c) row(*c, 5, false, n, T, true);
    row('D', 3, false, n, T, true);
    row(0, 4, false, n, T, false);
    row(0, 5, true, n, T, false);
    row(0, 4, false, 3, 1024, true);                          // max_word 63: no slot path
    row(0, 4, false, 3, 1025, true);                          // max_word 64
    row(0, 4, false, 300, 750000, true);                      // the chain tests' uniform batch
    row(0, 4, false, (1ull << 32) - 1, 1ull << 36, true);
    row(0, 4, false, 1ull << 32, 1ull << 36, true);           // n no longer fits the work items' 32 bits
    row(0, 4, false, 2, 1ull << 34, true);                    // mean 2^33 bases: long_thr saturates
    row(0, 4, false, 2, 1ull << 34, false);
    row(0, 4, false, 1000, 5000000, true, 1ull << 31);        // a caller's mean_bases: 4 (2^31 + 1) + 1024 saturates
    row(0, 4, false, 1000, 5000000, false, 20000);
    return 0;
}
