// launch_plan.h -- how a persistent-kernel launch is sized: the environment knobs, the number of workgroups the chip
// holds at once, the grid, how many items a wave draws from its shard's counter at a time, and which kernel a plain
// search runs on.  Pure arithmetic on (items, shards, CUs, knobs) shared by every launcher (search_lines.hip,
// extract_lines.hip, locate.hip, mm1_worklist.hip, kmer_reads.hip); plain C++ with no HIP in it, so that
// tests/native/launch_plan_test.cpp holds it to the rules on a CPU.
#ifndef RSBWT_LAUNCH_PLAN_H
#define RSBWT_LAUNCH_PLAN_H

#include <limits.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

namespace rsb {

// The environment's tuning knobs (tools/README.md).  A caller keeps the answer in a `static const`: a knob is read
// once per process.  knob_int: the value where it parses to lo..hi, `fallback` for anything else and when unset.
inline long long knob_int(const char *name, long long lo, long long hi, long long fallback) {
    const char *e = getenv(name);
    if (!e) return fallback;
    const long long v = atoll(e);
    return v >= lo && v <= hi ? v : fallback;
}
inline bool knob_set(const char *name) { return getenv(name) != nullptr; }

// Workgroups resident at once: a persistent launch asks for no more.
// spare = RSBWT_SEARCH_SPARE_WGS = n (the three search launches alone): n workgroups fewer than the chip holds.  A search
// launch is persistent (its workgroups stay until the batch is done) and fills every CU's registers (4 waves x 128 VGPRs
// per SIMD) and LDS: a kernel that should run BESIDE it -- RCCL's, gathering the previous batch at N > 1 -- finds room
// only on CUs a workgroup short.  bench.py sets it for its N > 1 ranks (32: a workgroup slot on 32 CUs for the
// collective's channels).
inline size_t resident_cap(int num_cus, size_t wgs_per_cu, size_t spare = 0) {
    const size_t cap_all = (size_t)num_cus * wgs_per_cu;
    return cap_all > 2 * spare ? cap_all - spare : cap_all;
}

// The grid: a workgroup per items_per_wg items, `cap` at the most.  even_shards = nshards for the walkers, whose waves
// start on shard (workgroup % nshards): every shard starts with as many workgroups as any other.  at_least: locate's 1.
inline size_t plan_grid(size_t items, size_t items_per_wg, size_t cap, size_t even_shards = 0, size_t at_least = 0) {
    size_t g = (items + items_per_wg - 1) / items_per_wg;
    if (g > cap) g = cap;
    if (even_shards && g >= even_shards) g -= g % even_shards;
    return g < at_least ? at_least : g;
}

// Items per draw from a shard's counter: `most` for a launch that fills the chip, halved down to `least` for a small
// one until every one of the `waves` that share the items draws `draws` times or more -- a batch of a few thousand
// queries (a service micro-batch, the k-mers of a 1-mismatch slice) then still occupies every wave launched instead of
// the first few.  (Until round 5 an extraction of a few hundred rows -- the rows of a service window's intervals -- gave
// all of them to the first wave that asked: 242 rows took four walks one after the other, 1.24 ms,
// tools/probe_setquery.py.)
//   search on lane pairs   1024 .. 32, 4 draws      extraction  ROW_CHUNK .. 1, 2 draws
//   on lone lanes          1024 .. 64, 4 draws      locate      256 .. 64, 2 draws, of the waves of ONE shard
inline uint32_t plan_draw(uint32_t most, uint32_t least, size_t waves, uint32_t draws, size_t items) {
    uint32_t chunk = most;
    while (chunk > least && (size_t)chunk * waves * draws > items) chunk >>= 1;
    return chunk;
}
// (locate's waves walk one shard at a time: a shard's list is shared by its part of the launch)
inline size_t waves_per_shard(size_t grid, size_t wg_waves, size_t nshards) {
    const size_t w = grid * wg_waves / nshards;
    return w ? w : 1;
}

// Which kernel a plain search runs on.  RSBWT_SEARCH_KERNEL = pair | solo | auto (default).
enum search_kernel_knob { SEARCH_PAIR = 0, SEARCH_SOLO = 1, SEARCH_AUTO = 2 };
// one lane per search (search_solo.h) where intervals are narrow for most of a search: shards whose
// k-mer tables are deep (`narrow`: what is left of a hit are steps inside one window); behind
// a shallow table the first steps are wide, where pairs take one pass and a lone lane two
// (and only when the batch fills every lane of the launch: below that nothing is saturated and the
// pairs answer sooner -- a lone request of the service loop takes half the passes).
// Until round 5 several shards per launch stayed on lane pairs ("at the request ceiling already"): the
// launch is bound by the instructions a SIMD issues, not by requests (+ 12.6 % VALU = + 5.7 %
// time, the same build), a pair spends a whole lane on `upper` where 97 % of the steps find it in the line
// `lower - 1` staged, and the lone lanes run the headline's 8 x 20 GB shards in 19.05 ms against 20.04
// (`resumed`: the variants of a 1-mismatch search that resume from a trace start on their k-mer's narrow interval and
// live 2.4 steps: what bounds their launch is how fast searches are taken up, and a wave of lone lanes takes up 64 per
// pass where pairs take 32 -- any number of shards: 25.0 -> 23.5 ms per batch of 4e5 31-mers x 8 shards)
inline bool plan_lone_lanes(int knob, bool table_build, size_t searches, size_t cap, size_t wg_waves, bool resumed, bool narrow) {
    return !table_build && (knob == SEARCH_SOLO || (knob == SEARCH_AUTO && searches >= cap * wg_waves * 64u && (resumed || narrow)));
}

}  // namespace rsb
#endif
