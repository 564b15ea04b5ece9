// The launch plan (readserver_amd/csrc/launch_plan.h) on a table of inputs: for every row what the launcher of that kind
// would ask for -- cap, kernel choice, grid, draw -- composed from the header's functions the way the launcher composes
// them, with the knobs of this process's environment.  tests/test_launch_plan.py runs it once per environment and
// holds every line to the rules restated there.  A line: `kind name in=.. in=.. => out=.. out=..`.
#include <stdio.h>
#include <string.h>

#include "launch_plan.h"

using namespace rsb;

// (the kernels' constants: wave_lines.h, search_solo.h, extract_lines.hip, locate.hip, kmer_reads.hip, sets.hip)
constexpr size_t WG_WAVES = 4, MIN_WGS = 4, WALK1MM_WGS = 3, WALK_MIN_WGS = 4, WALK_WAVES = 4, KR_WAVES = 4;
constexpr uint32_t ROW_CHUNK = 256;

struct knobs_t {
    size_t wave_wgs, walk1mm_wgs, extract_wgs, spare;
    int choice;
};

static knobs_t read_knobs() {
    knobs_t k;
    k.wave_wgs = (size_t)knob_int("RSBWT_WAVE_WGS_PER_CU", 1, INT_MAX, MIN_WGS);
    k.walk1mm_wgs = (size_t)knob_int("RSBWT_WALK1MM_WGS_PER_CU", 1, WALK1MM_WGS, WALK1MM_WGS);
    k.extract_wgs = (size_t)knob_int("RSBWT_EXTRACT_WGS_PER_CU", 1, 20, WALK_MIN_WGS);
    k.spare = (size_t)knob_int("RSBWT_SEARCH_SPARE_WGS", 1, LLONG_MAX, 0);
    const char *e = getenv("RSBWT_SEARCH_KERNEL");
    k.choice = e && !strcmp(e, "pair") ? SEARCH_PAIR : e && !strcmp(e, "solo") ? SEARCH_SOLO : SEARCH_AUTO;
    return k;
}

struct search_row { const char *name; size_t Q, S; bool narrow, resumed, table_build; };
struct mm1_row { const char *name; size_t m, S; unsigned k, tn; };
struct walk_row { const char *name; size_t total, S; };
struct grid_row { const char *name; size_t items; };

int main() {
    const knobs_t kn = read_knobs();
    printf("knobs all wave_wgs=%zu walk1mm_wgs=%zu extract_wgs=%zu spare=%zu choice=%d side_log2=%lld table_prepass=%d wide_rows=%lld "
           "no_staged=%d\n",
           kn.wave_wgs, kn.walk1mm_wgs, kn.extract_wgs, kn.spare, kn.choice, knob_int("RSBWT_SET_1MM_SIDE_LOG2", 10, 40, 26),
           (int)(knob_int("RSBWT_SET_1MM_TABLE_PREPASS", INT_MIN, INT_MAX, 1) != 0), knob_int("RSBWT_KMER_WIDE_ROWS", 1, LLONG_MAX, 1ll << 22),
           (int)knob_set("RSBWT_NO_STAGED_RESULTS"));
    const int cus_of[] = {256, 1, 0};  // (0: no launcher is reached with it; locate alone says what it would do)
    for (int cus : cus_of) {
        const search_row searches[] = {
            {"headline", 10000000, 8, true, false, false},    {"window", 4096, 8, true, false, false},
            {"threshold", 32768, 8, true, false, false},      {"below", 32767, 8, true, false, false},
            {"wide", 32768, 8, false, false, false},          {"resumed", 32768, 8, false, true, false},
            {"one", 1, 1, false, false, false},               {"one_narrow", 1, 1, true, false, false},
            {"table", 1u << 24, 1, true, false, true},        {"odd", 12345, 3, true, false, false},
            {"one_shard_full", 4000000, 1, true, false, false},
        };
        for (const search_row &r : searches) {
            const size_t nrec = r.Q * r.S, cap = resident_cap(cus, kn.wave_wgs, kn.spare);
            const bool solo = plan_lone_lanes(kn.choice, r.table_build, nrec, cap, WG_WAVES, r.resumed, r.narrow);
            const size_t grid = plan_grid(nrec, (solo ? 64u : 32u) * WG_WAVES, cap);
            const uint32_t draw = plan_draw(1024, solo ? 64 : 32, grid * WG_WAVES, 4, nrec);
            printf("search %s cus=%d Q=%zu S=%zu narrow=%d resumed=%d table=%d => cap=%zu solo=%d grid=%zu draw=%u\n", r.name, cus, r.Q, r.S,
                   (int)r.narrow, (int)r.resumed, (int)r.table_build, cap, (int)solo, grid, draw);
        }
        const mm1_row mm1[] = {{"slice", 400000, 8, 31, 16}, {"one", 1, 1, 31, 16}, {"few", 300, 8, 31, 30}, {"shallow", 5000, 3, 20, 1}};
        for (const mm1_row &r : mm1) {
            const size_t cap = resident_cap(cus, kn.walk1mm_wgs, kn.spare), items = r.m * r.S;
            const size_t grid = plan_grid(items, 64u * WG_WAVES, cap);
            printf("walk %s cus=%d m=%zu S=%zu k=%u tn=%u => cap=%zu grid=%zu draw=%u\n", r.name, cus, r.m, r.S, r.k, r.tn, cap, grid,
                   plan_draw(1024, 64, grid * WG_WAVES, 4, items));
        }
        for (const mm1_row &r : mm1) {
            const size_t cap = resident_cap(cus, kn.wave_wgs, kn.spare), implicit = r.m * 3u * (size_t)(r.k - r.tn), wl_cap = r.m * 3u * r.tn;
            const size_t grid = plan_grid((implicit + wl_cap) * r.S, 64u * WG_WAVES, cap);
            printf("worklist %s cus=%d m=%zu S=%zu k=%u tn=%u wl_cap=%zu => cap=%zu grid=%zu draw=%u\n", r.name, cus, r.m, r.S, r.k, r.tn, wl_cap,
                   cap, grid, plan_draw(1024, 64, grid * WG_WAVES, 4, implicit * r.S));
        }
        // (total: the rows of all shards -- n x S of a padded extraction, the sum of the segments of a ragged one)
        const walk_row walks[] = {{"full", 1000000, 1},   {"full", 8000000, 8}, {"full", 3000000, 3}, {"window", 242, 1}, {"window", 300, 8},
                                  {"window", 1936, 8},    {"mid", 50000, 3},    {"mid", 200000, 8},   {"one", 1, 1},      {"one", 1, 8},
                                  {"one_each", 8, 8},     {"seven", 7, 8}};
        for (const walk_row &r : walks) {
            const size_t cap = resident_cap(cus, kn.extract_wgs), grid = plan_grid(r.total, 64 * WALK_WAVES, cap, r.S);
            printf("extract %s cus=%d total=%zu S=%zu => cap=%zu grid=%zu draw=%u\n", r.name, cus, r.total, r.S, cap, grid,
                   plan_draw(ROW_CHUNK, 1, grid * WALK_WAVES, 2, r.total));
        }
        for (const walk_row &r : walks) {
            const size_t cap = resident_cap(cus, WALK_MIN_WGS), grid = plan_grid(r.total, 64 * WALK_WAVES, cap, r.S, 1);
            printf("locate %s cus=%d n=%zu S=%zu => cap=%zu grid=%zu draw=%u\n", r.name, cus, r.total, r.S, cap, grid,
                   plan_draw(256, 64, waves_per_shard(grid, WALK_WAVES, r.S), 2, r.total));
        }
        const grid_row grids[] = {{"one", 1}, {"wg", 256}, {"wg_and_one", 257}, {"full", 6400000}};
        for (const grid_row &r : grids) {
            printf("branch %s cus=%d items=%zu => grid=%zu\n", r.name, cus, r.items, plan_grid(r.items, 64 * WG_WAVES, resident_cap(cus, MIN_WGS)));
            printf("kmer_reads %s cus=%d items=%zu => grid=%zu\n", r.name, cus, r.items, plan_grid(r.items, 64 * KR_WAVES, resident_cap(cus, 4)));
        }
    }
    return 0;
}
