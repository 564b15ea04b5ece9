// walk.hip -- extension counts and walks through the reads' k-mer graph on the GPU (gfx950): "what do the reads say
// comes next?" (include/rsbwt.h: the definition).  A seed's candidates are its context of ctx symbols with A, C, G or T
// put on the walking side; a candidate's count in a shard is the width of its findInterval (plus that of its reverse
// complement when both strands are asked for); the support of a symbol is the sum over every shard.  A backward search
// cannot grow a pattern to the right, so every appended symbol costs fresh searches of ctx + 1 symbols, and the
// decision needs the sum over the shards: a dependent loop, which walk_kernel keeps inside one launch.
//
// MAPPING.  A workgroup of NW waves owns 8 seeds.  The 64 lanes of every wave are (seed, base, strand) =
// 8 x 4 x 2: lane = seed * 8 + base * 2 + strand; with one strand the odd lanes idle.  Wave w searches shards w,
// w + NW, ... one after the other, so the shard is uniform per wave -- what match_lanes.h / wave_lines.h assume --
// and a lane adds its shards' counts in a register.  NW is WG_WAVES (4) from four shards on, 2 for two or three and 1 for
// one: a wave without a shard would only hold registers and a stage buffer that a workgroup of other seeds can use.
//   * SEARCH (walk_search): overlap_kernel's pass without the '$' rank.  START: the shard's k-mer table entry of the
//     candidate's last T symbols when T >= 2 and ctx + 1 >= T, by start_record's rule (search_lines.hip: not KTAB_WIDE,
//     lower + width <= n, width != 0); a refused entry starts over from initInterval of the last symbol.  PASS: Occ(c, .)
//     at lo - 1 and at hi, both off ONE fetched line when hi lies in lo - 1's window among that line's own pieces, else a
//     pass per position; lo == 0 fetches nothing for that side; a position past its line's own pieces goes through the
//     scalar reader (view_occ).  END: the step that empties the interval; nothing past it is looked at.  Every lane of
//     the wave is in every glds_fetch: a lane with nothing to rank asks for nothing.
//   * STEP of the walk: the waves' partial counts meet in LDS (s_part, one slot per wave: no atomics, nothing to zero);
//     barrier; every lane reads the four sums of its seed and takes the same decision; wave 0 stores the appended
//     symbol and its support, moves the seed's context on by one symbol -- a ring of ctx bytes per seed in LDS, so the
//     output is never read back -- and counts the seeds still walking into s_live; barrier; the loop ends when s_live is
//     0.  That exit is read from LDS after a barrier, so it is the same for the whole workgroup; a stopped, an invalid or
//     a missing seed (Q need not be a multiple of 8) idles its lanes and keeps them in the loop, and a wave without a
//     shard (fewer shards than waves) writes zeros and reaches both barriers.  The loop runs max_steps times at the
//     most, whatever the data says.
// extension_kernel is the evaluation without the decision: a wave owns (8 seeds, one shard) and writes that shard's
// counts.  Sets over several device groups walk with it, one round trip per step (set_graph.hip).
// unitig_kernel is the walk both ways with the joins looked at: the unit of work is the item (seed, side), and a step
// evaluates onward and then, in the opposite direction, the node the one live symbol enters (unitig_rule.h: the decision).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "capi_internal.h"
#include "kernels.h"
#include "line_format.h"
#include "match_lanes.h"
#include "rank_device.h"
#include "unitig_rule.h"
#include "walk_search.h"
#include "wave_lines.h"

namespace rsb {

namespace {

template <int NW>  // the waves of a workgroup: 1, 2 or WG_WAVES (launch_walk: no more than the shards can keep busy)
__global__ void __launch_bounds__(64 * NW)
walk_kernel(const shard_view *__restrict__ shards, const uint32_t nshards, const walk_batch bt, char *__restrict__ ext, uint32_t *__restrict__ steps_out,
            uint8_t *__restrict__ stop_out, uint32_t *__restrict__ support, unsigned long long *__restrict__ last, unsigned long long *__restrict__ work) {
    __shared__ uint4 s_stage[NW][64 * SLOT_U4];
    __shared__ uint8_t s_ring[WALK_SEEDS][WALK_RING];
    __shared__ unsigned long long s_part[NW][WALK_SEEDS * 4];
    __shared__ uint32_t s_bad[WALK_SEEDS];
    __shared__ uint32_t s_live;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint4 *stage = s_stage[wave];
    const uint32_t stage_lds = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)(lds_void_ptr)stage);
    const staged_line L = {own_stage_row(stage, lane), lane & 7u};
    const uint32_t seed = lane >> 3, base = (lane >> 1) & 3u, rev = lane & 1u;
    const bool both = (bt.flags & RSBWT_WALK_BOTH_STRANDS) != 0u, left = (bt.flags & RSBWT_WALK_LEFT) != 0u;
    const size_t first_q = (size_t)blockIdx.x * WALK_SEEDS, q = first_q + seed;
    const bool writer = wave == 0u && (lane & 7u) == 0u;  // the one lane that stores its seed's answers

    if (threadIdx.x < WALK_SEEDS) s_bad[threadIdx.x] = 0u;
    __syncthreads();
    walk_load_rings(bt, first_q, s_ring, s_bad, threadIdx.x, blockDim.x);
    __syncthreads();

    // the seed's state, the same in every lane of the seed in every wave: it is a function of the sums in LDS alone
    bool walking = q < bt.Q && walk_seed_len(bt, q) >= bt.ctx && s_bad[seed] == 0u;
    uint32_t nsteps = 0, appended = 0;
    walk_cand cd = {s_ring[seed], 0u, bt.ctx, base + 1u, left, rev != 0u};
    walk_tally tally;
    if (writer && q < bt.Q && !walking) {  // an invalid seed
        steps_out[q] = 0u;
        stop_out[q] = (uint8_t)RSBWT_WALK_INVALID;
        if (last)
            for (uint32_t i = 0; i < 4u; ++i) last[4u * q + i] = 0ull;
    }

    for (uint32_t it = 0; it < bt.max_steps; ++it) {  // (a walking seed appends one symbol per round)
        unsigned long long cnt = 0;
        for (uint32_t sid = wave; sid < nshards; sid += (uint32_t)NW)
            cnt += walk_search(shards + sid, walking && (both || rev == 0u), cd, lane, stage_lds, L, tally);
        cnt += __shfl_xor(cnt, 1, 64);  // the two strands
        if (rev == 0u) s_part[wave][seed * 4u + base] = cnt;
        __syncthreads();
        if (walking) {
            unsigned long long sup[4];
            uint32_t nlive = 0, pick = 0;
            for (uint32_t b = 0; b < 4u; ++b) {
                sup[b] = 0;
                for (uint32_t w = 0; w < (uint32_t)NW; ++w) sup[b] += s_part[w][seed * 4u + b];
                if (sup[b] >= bt.min_count) {
                    ++nlive;
                    pick = b;
                }
            }
            uint32_t stop = 0;
            if (nlive == 1u) {
                if (writer) {
                    const size_t at = q * (size_t)bt.max_steps + nsteps;
                    ext[at] = "ACGT"[pick];
                    if (support) support[at] = sup[pick] > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)sup[pick];
                    ++appended;
                }
                // the context moves on by one symbol
                if (left) {
                    cd.head = cd.head == 0u ? cd.ctx - 1u : cd.head - 1u;
                    if (writer) s_ring[seed][cd.head] = (uint8_t)(pick + 1u);
                } else {
                    if (writer) s_ring[seed][cd.head] = (uint8_t)(pick + 1u);
                    cd.head = cd.head + 1u == cd.ctx ? 0u : cd.head + 1u;
                }
                if (++nsteps == bt.max_steps) stop = RSBWT_WALK_LIMIT;
            } else {
                stop = nlive == 0u ? RSBWT_WALK_DEAD_END : RSBWT_WALK_BRANCH;
            }
            if (stop != 0u) {
                walking = false;
                if (writer) {
                    steps_out[q] = nsteps;
                    stop_out[q] = (uint8_t)stop;
                    if (last)
                        for (uint32_t b = 0; b < 4u; ++b) last[4u * q + b] = stop == RSBWT_WALK_LIMIT ? 0ull : sup[b];
                }
            }
        }
        if (wave == 0u) {  // (every lane of wave 0 is in the ballot)
            const uint64_t still = __builtin_amdgcn_ballot_w64(walking && (lane & 7u) == 0u);
            if (lane == 0u) s_live = (uint32_t)__builtin_popcountll(still);
        }
        __syncthreads();
        if (s_live == 0u) break;  // (LDS after a barrier: the same for every lane of the workgroup)
    }
    walk_add_work(work, lane, tally, appended);
}

// ---- unitigs: both ways from the seed, stopping where another path joins (include/rsbwt.h) ----
// The unit of work is the ITEM (seed, side): side 0 walks right from s[-ctx:], side 1 left from s[:ctx], each with a ring
// of its own.  A workgroup owns 8 items = 4 seeds x 2 sides, a wave's lanes are (item, base, strand), item = lane >> 3 =
// output index i - 8 * blockIdx.x, and the waves share the shards as in walk_kernel.  A step is two evaluations through ONE
// call site of walk_search (the pass loop): ONWARD, the walk's own; then, for the items that found exactly one live symbol,
// RETURN: the node entered, searched in the opposite direction.  The tentative symbol goes into the ring where the context
// moves to, so with the head moved on the ring holds exactly that node.
constexpr uint32_t UNITIG_ITEMS = 8;  // items of a wave's lanes: 4 seeds x 2 sides

__device__ __forceinline__ void unitig_load_rings(const walk_batch &bt, size_t first_q, uint8_t (*ring)[WALK_RING], uint32_t *bad, uint32_t tid,
                                                  uint32_t nthreads) {
    const uint8_t *text = reinterpret_cast<const uint8_t *>(bt.text);
    for (uint32_t it = 0; it < UNITIG_ITEMS; ++it) {
        const size_t q = first_q + (it >> 1);
        const uint64_t Lq = walk_seed_len(bt, q);
        if (Lq < bt.ctx) continue;
        const uint64_t from = (it & 1u) ? bt.off[q] : bt.off[q + 1] - bt.ctx;  // the side is the item's
        for (uint32_t i = tid; i < bt.ctx; i += nthreads) {
            const uint32_t r = ms_rank(text[from + i]);
            ring[it][i] = (uint8_t)r;
            if (r == 0u) bad[it] = 1u;
        }
    }
}

template <int NW>  // the waves of a workgroup, as walk_kernel's
__global__ void __launch_bounds__(64 * NW)
unitig_kernel(const shard_view *__restrict__ shards, const uint32_t nshards, const walk_batch bt, char *__restrict__ ext,
              uint32_t *__restrict__ steps_out, uint8_t *__restrict__ stop_out, uint32_t *__restrict__ support, unsigned long long *__restrict__ last,
              unsigned long long *__restrict__ work) {
    __shared__ uint4 s_stage[NW][64 * SLOT_U4];
    __shared__ uint8_t s_ring[UNITIG_ITEMS][WALK_RING];
    __shared__ unsigned long long s_part[NW][UNITIG_ITEMS * 4];
    __shared__ uint32_t s_bad[UNITIG_ITEMS];
    __shared__ uint32_t s_live, s_tent;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint4 *stage = s_stage[wave];
    const uint32_t stage_lds = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)(lds_void_ptr)stage);
    const staged_line L = {own_stage_row(stage, lane), lane & 7u};
    const uint32_t item = lane >> 3, base = (lane >> 1) & 3u, rev = lane & 1u;
    const bool both = (bt.flags & RSBWT_WALK_BOTH_STRANDS) != 0u, left = (item & 1u) != 0u;
    const size_t first_q = (size_t)blockIdx.x * (UNITIG_ITEMS / 2u), q = first_q + (item >> 1);
    const size_t i = (size_t)blockIdx.x * UNITIG_ITEMS + item;  // = 2 * q + side
    const bool writer = wave == 0u && (lane & 7u) == 0u;        // the one lane that stores its item's answers

    if (threadIdx.x < UNITIG_ITEMS) s_bad[threadIdx.x] = 0u;
    __syncthreads();
    unitig_load_rings(bt, first_q, s_ring, s_bad, threadIdx.x, blockDim.x);
    __syncthreads();

    // the item's state, the same in every lane of the item in every wave: a function of the sums in LDS alone
    bool walking = q < bt.Q && walk_seed_len(bt, q) >= bt.ctx && s_bad[item] == 0u;
    bool tent = false;  // a tentative symbol waits for its node's return evaluation
    uint32_t nsteps = 0, head = 0, next_head = 0, pick = 0;
    uint32_t appended = 0, n_onward = 0, n_return = 0;  // (the writer's)
    uint64_t sums[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // the step's: [0..3] onward, [4..7] return
    walk_tally tally;
    // the writer's stores when its item stops: LIMIT and INVALID leave zeros in last
    auto stopped = [&](uint32_t why) {
        steps_out[i] = nsteps;
        stop_out[i] = (uint8_t)why;
        if (last) {
            const bool zeros = why == RSBWT_WALK_LIMIT || why == RSBWT_WALK_INVALID;
            for (uint32_t b = 0; b < 8u; ++b) last[8u * i + b] = zeros || (b >= 4u && why != RSBWT_WALK_JOIN) ? 0ull : sums[b];
        }
    };
    if (writer && q < bt.Q && !walking) stopped(RSBWT_WALK_INVALID);  // (a side whose sibling walks writes here, once)

    for (uint32_t it = 0; it < bt.max_steps; ++it) {  // (a walking item appends one symbol per round, or stops)
#pragma nounroll
        for (uint32_t pass = 0; pass < 2u; ++pass) {  // 0: onward; 1: return, of the items that hold a tentative symbol
            if (pass != 0u && s_tent == 0u) break;    // (LDS after a barrier: the same for every lane of the workgroup)
            const walk_cand cd = {s_ring[item], pass != 0u ? next_head : head, bt.ctx, base + 1u, left != (pass != 0u), rev != 0u};
            const bool go = walking && (pass == 0u || tent) && (both || rev == 0u);
            unsigned long long cnt = 0;
            for (uint32_t sid = wave; sid < nshards; sid += (uint32_t)NW) cnt += walk_search(shards + sid, go, cd, lane, stage_lds, L, tally);
            cnt += __shfl_xor(cnt, 1, 64);  // the two strands
            if (rev == 0u) s_part[wave][item * 4u + base] = cnt;
            __syncthreads();
            if (pass == 0u) {
                if (walking) {
                    for (uint32_t b = 0; b < 4u; ++b) {
                        sums[b] = 0;
                        for (uint32_t w = 0; w < (uint32_t)NW; ++w) sums[b] += s_part[w][item * 4u + b];
                    }
                    if (writer) ++n_onward;
                    const uint32_t why = unitig_onward(sums, bt.min_count, nsteps, bt.max_steps, &pick);
                    if (why == UNITIG_GO) {
                        // the node entered: the tentative symbol where the context moves to, the head moved on
                        tent = true;
                        if (left) {
                            next_head = head == 0u ? bt.ctx - 1u : head - 1u;
                            if (writer) s_ring[item][next_head] = (uint8_t)(pick + 1u);
                        } else {
                            if (writer) s_ring[item][head] = (uint8_t)(pick + 1u);
                            next_head = head + 1u == bt.ctx ? 0u : head + 1u;
                        }
                    } else {
                        walking = false;
                        if (writer) stopped(why);
                    }
                }
                if (wave == 0u) {  // (every lane of wave 0 is in the ballot)
                    const uint64_t held = __builtin_amdgcn_ballot_w64(tent && (lane & 7u) == 0u);
                    if (lane == 0u) s_tent = (uint32_t)__builtin_popcountll(held);
                }
                __syncthreads();
            }
        }
        if (tent) {  // (the return pass ran: s_tent counted this item)
            tent = false;
            for (uint32_t b = 0; b < 4u; ++b) {
                sums[4u + b] = 0;
                for (uint32_t w = 0; w < (uint32_t)NW; ++w) sums[4u + b] += s_part[w][item * 4u + b];
            }
            if (writer) ++n_return;
            if (unitig_return(sums + 4, bt.min_count) != UNITIG_GO) {
                walking = false;  // (the ring stays advanced: nobody reads it again)
                if (writer) stopped(RSBWT_WALK_JOIN);
            } else {
                if (writer) {
                    const size_t at = i * (size_t)bt.max_steps + nsteps;
                    ext[at] = "ACGT"[pick];
                    if (support) support[at] = unitig_saturate(sums[pick]);
                    ++appended;
                }
                head = next_head;
                if (++nsteps == bt.max_steps) {
                    walking = false;
                    if (writer) stopped(RSBWT_WALK_LIMIT);
                }
            }
        }
        if (wave == 0u) {
            const uint64_t still = __builtin_amdgcn_ballot_w64(walking && (lane & 7u) == 0u);
            if (lane == 0u) s_live = (uint32_t)__builtin_popcountll(still);
        }
        __syncthreads();
        if (s_live == 0u) break;  // (LDS after a barrier: the same for every lane of the workgroup)
    }
    walk_add_work(work, lane, tally, appended);
    if (work) {
        const unsigned long long s6 = ms_wave_sum(n_onward), s7 = ms_wave_sum(n_return);
        if (lane == 0u) {
            if (s6) atomicAdd(&work[6], s6);
            if (s7) atomicAdd(&work[7], s7);
        }
    }
}

// One evaluation per (seed, shard): counts[shard][q][base].  Wave u of the grid owns seeds 8 * (u / nshards) .. + 7 in
// shard u % nshards; the four waves of a workgroup keep their own rings.
__global__ void __launch_bounds__(64 * WG_WAVES)
extension_kernel(const shard_view *__restrict__ shards, const uint32_t nshards, const walk_batch bt, unsigned long long *__restrict__ counts,
                 unsigned long long *__restrict__ work) {
    __shared__ uint4 s_stage[WG_WAVES][64 * SLOT_U4];
    __shared__ uint8_t s_ring[WG_WAVES][WALK_SEEDS][WALK_RING];
    __shared__ uint32_t s_bad[WG_WAVES][WALK_SEEDS];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint4 *stage = s_stage[wave];
    const uint32_t stage_lds = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)(lds_void_ptr)stage);
    const staged_line L = {own_stage_row(stage, lane), lane & 7u};
    const uint32_t seed = lane >> 3, base = (lane >> 1) & 3u, rev = lane & 1u;
    const bool both = (bt.flags & RSBWT_WALK_BOTH_STRANDS) != 0u, left = (bt.flags & RSBWT_WALK_LEFT) != 0u;
    const size_t groups = (bt.Q + WALK_SEEDS - 1) / WALK_SEEDS;
    const size_t unit = (size_t)blockIdx.x * WG_WAVES + wave;
    const size_t grp = unit / nshards;
    const uint32_t sid = (uint32_t)(unit % nshards);
    const bool mine = grp < groups;  // (a wave past the last unit idles and reaches the barriers)
    const size_t first_q = grp * WALK_SEEDS, q = first_q + seed;

    if (lane < WALK_SEEDS) s_bad[wave][lane] = 0u;
    __syncthreads();
    if (mine) walk_load_rings(bt, first_q, s_ring[wave], s_bad[wave], lane, 64u);
    __syncthreads();

    const bool valid = mine && q < bt.Q && walk_seed_len(bt, q) >= bt.ctx && s_bad[wave][seed] == 0u;
    const walk_cand cd = {s_ring[wave][seed], 0u, bt.ctx, base + 1u, left, rev != 0u};
    walk_tally tally;
    unsigned long long cnt = walk_search(shards + sid, valid && (both || rev == 0u), cd, lane, stage_lds, L, tally);
    cnt += __shfl_xor(cnt, 1, 64);  // the two strands
    if (mine && q < bt.Q && rev == 0u) counts[((size_t)sid * bt.Q + q) * 4u + base] = cnt;
    walk_add_work(work, lane, tally, 0u);
}

thread_local uint64_t walk_last[6] = {0, 0, 0, 0, 0, 0};
thread_local uint64_t unitig_last[8] = {0, 0, 0, 0, 0, 0, 0, 0};

static_assert(UNITIG_DEAD_END == RSBWT_WALK_DEAD_END && UNITIG_BRANCH == RSBWT_WALK_BRANCH && UNITIG_LIMIT == RSBWT_WALK_LIMIT &&
                  UNITIG_JOIN == RSBWT_WALK_JOIN,
              "unitig_rule.h speaks include/rsbwt.h's stop codes");

#define WK_HIP(x)                                              \
    do {                                                       \
        hipError_t _e = (x);                                   \
        if (_e != hipSuccess) return fail_hip(_e, #x);         \
    } while (0)

// the scratch of a call goes back after the stream has drained: the launches may still run when the call leaves early
struct give_back {
    scratch_cache &sc;
    scratch_cache::lease &l;
    hipStream_t st;
    ~give_back() {
        (void)hipStreamSynchronize(st);
        sc.give(l, st);
    }
};

}  // namespace

hipError_t launch_walk(const shard_view *d_shards, uint32_t nshards, const walk_batch &bt, void *d_ext, void *d_steps, void *d_stop, void *d_support,
                       void *d_last, unsigned long long *d_work, hipStream_t stream) {
    if (bt.Q == 0 || nshards == 0) return hipSuccess;
    if (bt.ctx == 0u || bt.ctx >= WALK_RING || bt.max_steps == 0u || bt.min_count == 0ull) return hipErrorInvalidValue;
    const size_t blocks = (bt.Q + WALK_SEEDS - 1) / WALK_SEEDS;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    // every byte past a walk's steps is 0
    hipError_t e = hipMemsetAsync(d_ext, 0, bt.Q * (size_t)bt.max_steps, stream);
    if (e == hipSuccess && d_support) e = hipMemsetAsync(d_support, 0, bt.Q * (size_t)bt.max_steps * 4, stream);
    if (e != hipSuccess) return e;
    // no more waves per workgroup than the shards can keep busy
    auto go = [&](auto kernel, unsigned waves) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(64 * waves), 0, stream, d_shards, nshards, bt, (char *)d_ext, (uint32_t *)d_steps,
                           (uint8_t *)d_stop, (uint32_t *)d_support, (unsigned long long *)d_last, d_work);
    };
    if (nshards >= (uint32_t)WG_WAVES) go(walk_kernel<WG_WAVES>, WG_WAVES);
    else if (nshards >= 2u) go(walk_kernel<2>, 2);
    else go(walk_kernel<1>, 1);
    return hipGetLastError();
}

hipError_t launch_extensions(const shard_view *d_shards, uint32_t nshards, const walk_batch &bt, void *d_counts, unsigned long long *d_work,
                             hipStream_t stream) {
    if (bt.Q == 0 || nshards == 0) return hipSuccess;
    if (bt.ctx == 0u || bt.ctx >= WALK_RING) return hipErrorInvalidValue;
    const size_t units = ((bt.Q + WALK_SEEDS - 1) / WALK_SEEDS) * nshards, blocks = (units + WG_WAVES - 1) / WG_WAVES;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(extension_kernel, dim3((unsigned)blocks), dim3(64 * WG_WAVES), 0, stream, d_shards, nshards, bt,
                       (unsigned long long *)d_counts, d_work);
    return hipGetLastError();
}

hipError_t launch_unitigs(const shard_view *d_shards, uint32_t nshards, const walk_batch &bt, void *d_ext, void *d_steps, void *d_stop,
                          void *d_support, void *d_last, unsigned long long *d_work, hipStream_t stream) {
    if (bt.Q == 0 || nshards == 0) return hipSuccess;
    if (bt.ctx == 0u || bt.ctx >= WALK_RING || bt.max_steps == 0u || bt.min_count == 0ull) return hipErrorInvalidValue;
    if ((bt.flags & ~(uint32_t)RSBWT_WALK_BOTH_STRANDS) != 0u) return hipErrorInvalidValue;  // (the side is the item's)
    const size_t items = 2 * bt.Q, blocks = (items + UNITIG_ITEMS - 1) / UNITIG_ITEMS;
    if (blocks > 0x7FFFFFFFull || (uint64_t)items * bt.max_steps >= (1ull << 31)) return hipErrorInvalidValue;
    // every byte past a side's steps is 0
    hipError_t e = hipMemsetAsync(d_ext, 0, items * (size_t)bt.max_steps, stream);
    if (e == hipSuccess && d_support) e = hipMemsetAsync(d_support, 0, items * (size_t)bt.max_steps * 4, stream);
    if (e != hipSuccess) return e;
    auto go = [&](auto kernel, unsigned waves) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(64 * waves), 0, stream, d_shards, nshards, bt, (char *)d_ext, (uint32_t *)d_steps,
                           (uint8_t *)d_stop, (uint32_t *)d_support, (unsigned long long *)d_last, d_work);
    };
    if (nshards >= (uint32_t)WG_WAVES) go(unitig_kernel<WG_WAVES>, WG_WAVES);
    else if (nshards >= 2u) go(unitig_kernel<2>, 2);
    else go(unitig_kernel<1>, 1);
    return hipGetLastError();
}

void unitig_set_last_work(const uint64_t work8[8]) {
    for (int i = 0; i < 8; ++i) unitig_last[i] = work8 ? work8[i] : 0;
}
void unitig_get_last_work(uint64_t work8[8]) { memcpy(work8, unitig_last, sizeof unitig_last); }

int unitig_check_args(uint32_t ctx, uint32_t flags, uint32_t max_steps, size_t Q) {
    if (ctx < 1u || ctx > 255u) return fail(RSBWT_EINVAL, "ctx = %u: 1 to 255", ctx);
    if (flags & ~(uint32_t)RSBWT_WALK_BOTH_STRANDS) return fail(RSBWT_EINVAL, "flags 0x%x: a unitig takes RSBWT_WALK_BOTH_STRANDS only", flags);
    if (max_steps < 1u || max_steps > 65535u) return fail(RSBWT_EINVAL, "max_steps = %u: 1 to 65,535", max_steps);
    if ((uint64_t)Q >= (1ull << 31) || 2ull * Q * max_steps >= (1ull << 31))
        return fail(RSBWT_ERANGE, "%zu seeds x 2 sides x %u steps: under 2^31 in one call", Q, max_steps);
    return RSBWT_OK;
}

// A unitig call on one device on `st`: the batch goes up, ONE launch walks both sides of every seed over the shards of
// d_views, the answers come back (support and last are optional); work8[1..7] += the launch's counters.  Synchronises `st`.
int unitig_host_views(scratch_cache &scratch, hipStream_t st, const shard_view *d_views, uint32_t S, const char *t0, const uint64_t *rel, size_t Q,
                      size_t N, uint32_t ctx, uint64_t min_count, uint32_t max_steps, uint32_t flags, char *ext, uint32_t *steps, uint8_t *stop,
                      uint32_t *support, uint64_t *last, uint64_t *work8) {
    if (Q == 0 || S == 0) return RSBWT_OK;
    const size_t items = 2 * Q, cells = items * (size_t)max_steps;
    const size_t a_text = al256(N + 1), a_off = al256((Q + 1) * 8), a_ext = al256(cells), a_steps = al256(items * 4), a_stop = al256(items),
                 a_sup = support ? al256(cells * 4) : 0, a_last = last ? al256(items * 64) : 0;
    scratch_cache::lease mem;
    hipError_t e = scratch.take(a_text + a_off + a_ext + a_steps + a_stop + a_sup + a_last + 256, st, &mem);
    if (e != hipSuccess) return fail(RSBWT_ENOMEM, "%zu seeds x %u steps do not fit the device's free memory: %s", Q, max_steps, hipGetErrorString(e));
    give_back give{scratch, mem, st};
    uint8_t *d_text = (uint8_t *)mem.p, *d_off = d_text + a_text, *d_ext = d_off + a_off, *d_steps = d_ext + a_ext, *d_stop = d_steps + a_steps,
            *d_sup = d_stop + a_stop, *d_last = d_sup + a_sup, *d_wk = d_last + a_last;
    if (N) WK_HIP(hipMemcpyAsync(d_text, t0, N, hipMemcpyHostToDevice, st));
    WK_HIP(hipMemcpyAsync(d_off, rel, (Q + 1) * 8, hipMemcpyHostToDevice, st));
    WK_HIP(hipMemsetAsync(d_wk, 0, 256, st));
    walk_batch bt;
    bt.text = (const char *)d_text;
    bt.off = (const uint64_t *)d_off;
    bt.Q = Q;
    bt.N = N;
    bt.ctx = ctx;
    bt.max_steps = max_steps;
    bt.min_count = min_count ? min_count : 1ull;
    bt.flags = flags;
    e = launch_unitigs(d_views, S, bt, d_ext, d_steps, d_stop, support ? d_sup : nullptr, last ? d_last : nullptr, (unsigned long long *)d_wk, st);
    if (e != hipSuccess) return fail_hip(e, "unitig kernel launch");
    unsigned long long hwk[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    WK_HIP(hipMemcpyAsync(ext, d_ext, cells, hipMemcpyDeviceToHost, st));
    WK_HIP(hipMemcpyAsync(steps, d_steps, items * 4, hipMemcpyDeviceToHost, st));
    WK_HIP(hipMemcpyAsync(stop, d_stop, items, hipMemcpyDeviceToHost, st));
    if (support) WK_HIP(hipMemcpyAsync(support, d_sup, cells * 4, hipMemcpyDeviceToHost, st));
    if (last) WK_HIP(hipMemcpyAsync(last, d_last, items * 64, hipMemcpyDeviceToHost, st));
    WK_HIP(hipMemcpyAsync(hwk, d_wk, sizeof hwk, hipMemcpyDeviceToHost, st));
    WK_HIP(hipStreamSynchronize(st));
    if (work8)
        for (int i = 1; i < 8; ++i) work8[i] += hwk[i];
    return RSBWT_OK;
}

void walk_set_last_work(const uint64_t work6[6]) {
    for (int i = 0; i < 6; ++i) walk_last[i] = work6 ? work6[i] : 0;
}
void walk_get_last_work(uint64_t work6[6]) { memcpy(work6, walk_last, sizeof walk_last); }

int walk_check_args(uint32_t ctx, uint32_t flags, const uint32_t *max_steps, size_t Q) {
    if (ctx < 1u || ctx > 255u) return fail(RSBWT_EINVAL, "ctx = %u: 1 to 255", ctx);
    if (flags & ~(uint32_t)(RSBWT_WALK_LEFT | RSBWT_WALK_BOTH_STRANDS)) return fail(RSBWT_EINVAL, "unknown flag bits 0x%x", flags);
    if (max_steps) {
        if (*max_steps < 1u || *max_steps > 65535u) return fail(RSBWT_EINVAL, "max_steps = %u: 1 to 65,535", *max_steps);
        if ((uint64_t)Q * *max_steps >= (1ull << 31)) return fail(RSBWT_ERANGE, "%zu seeds x %u steps: under 2^31 in one call", Q, *max_steps);
    }
    return RSBWT_OK;
}

// One device's share of an extensions call on `st`: the batch goes up, one launch evaluates every (seed, shard of
// d_views), counts u64[S][Q][4] come back; work6[2..5] += {candidate searches, LF steps, lane-passes that fetched a
// line, table starts}.  Synchronises `st`.
int extension_host_views(scratch_cache &scratch, hipStream_t st, const shard_view *d_views, uint32_t S, const char *t0, const uint64_t *rel, size_t Q,
                         size_t N, uint32_t ctx, uint32_t flags, uint64_t *counts, uint64_t *work6) {
    if (Q == 0 || S == 0) return RSBWT_OK;
    const size_t cells = (size_t)S * Q * 4;
    const size_t a_text = al256(N + 1), a_off = al256((Q + 1) * 8), a_cnt = al256(cells * 8);
    scratch_cache::lease mem;
    hipError_t e = scratch.take(a_text + a_off + a_cnt + 256, st, &mem);
    if (e != hipSuccess) return fail(RSBWT_ENOMEM, "%zu seeds x %u shards do not fit the device's free memory: %s", Q, S, hipGetErrorString(e));
    give_back give{scratch, mem, st};
    uint8_t *d_text = (uint8_t *)mem.p, *d_off = d_text + a_text, *d_cnt = d_off + a_off, *d_wk = d_cnt + a_cnt;
    if (N) WK_HIP(hipMemcpyAsync(d_text, t0, N, hipMemcpyHostToDevice, st));
    WK_HIP(hipMemcpyAsync(d_off, rel, (Q + 1) * 8, hipMemcpyHostToDevice, st));
    WK_HIP(hipMemsetAsync(d_wk, 0, 256, st));
    walk_batch bt;
    bt.text = (const char *)d_text;
    bt.off = (const uint64_t *)d_off;
    bt.Q = Q;
    bt.N = N;
    bt.ctx = ctx;
    bt.max_steps = 1u;
    bt.min_count = 1ull;
    bt.flags = flags;
    e = launch_extensions(d_views, S, bt, d_cnt, (unsigned long long *)d_wk, st);
    if (e != hipSuccess) return fail_hip(e, "extension kernel launch");
    unsigned long long hwk[6] = {0, 0, 0, 0, 0, 0};
    WK_HIP(hipMemcpyAsync(counts, d_cnt, cells * 8, hipMemcpyDeviceToHost, st));
    WK_HIP(hipMemcpyAsync(hwk, d_wk, sizeof hwk, hipMemcpyDeviceToHost, st));
    WK_HIP(hipStreamSynchronize(st));
    if (work6)
        for (int i = 2; i < 6; ++i) work6[i] += hwk[i];
    return RSBWT_OK;
}

// A walk call on one device on `st`: the batch goes up, ONE launch walks every seed over the shards of d_views, the
// answers come back (support and last are optional); work6[1..5] += {appended symbols, candidate searches, LF steps,
// lane-passes that fetched a line, table starts}.  Synchronises `st`.
int walk_host_views(scratch_cache &scratch, hipStream_t st, const shard_view *d_views, uint32_t S, const char *t0, const uint64_t *rel, size_t Q,
                    size_t N, uint32_t ctx, uint64_t min_count, uint32_t max_steps, uint32_t flags, char *ext, uint32_t *steps, uint8_t *stop,
                    uint32_t *support, uint64_t *last, uint64_t *work6) {
    if (Q == 0 || S == 0) return RSBWT_OK;
    const size_t cells = Q * (size_t)max_steps;
    const size_t a_text = al256(N + 1), a_off = al256((Q + 1) * 8), a_ext = al256(cells), a_steps = al256(Q * 4), a_stop = al256(Q),
                 a_sup = support ? al256(cells * 4) : 0, a_last = last ? al256(Q * 32) : 0;
    scratch_cache::lease mem;
    hipError_t e = scratch.take(a_text + a_off + a_ext + a_steps + a_stop + a_sup + a_last + 256, st, &mem);
    if (e != hipSuccess) return fail(RSBWT_ENOMEM, "%zu seeds x %u steps do not fit the device's free memory: %s", Q, max_steps, hipGetErrorString(e));
    give_back give{scratch, mem, st};
    uint8_t *d_text = (uint8_t *)mem.p, *d_off = d_text + a_text, *d_ext = d_off + a_off, *d_steps = d_ext + a_ext, *d_stop = d_steps + a_steps,
            *d_sup = d_stop + a_stop, *d_last = d_sup + a_sup, *d_wk = d_last + a_last;
    if (N) WK_HIP(hipMemcpyAsync(d_text, t0, N, hipMemcpyHostToDevice, st));
    WK_HIP(hipMemcpyAsync(d_off, rel, (Q + 1) * 8, hipMemcpyHostToDevice, st));
    WK_HIP(hipMemsetAsync(d_wk, 0, 256, st));
    walk_batch bt;
    bt.text = (const char *)d_text;
    bt.off = (const uint64_t *)d_off;
    bt.Q = Q;
    bt.N = N;
    bt.ctx = ctx;
    bt.max_steps = max_steps;
    bt.min_count = min_count ? min_count : 1ull;
    bt.flags = flags;
    e = launch_walk(d_views, S, bt, d_ext, d_steps, d_stop, support ? d_sup : nullptr, last ? d_last : nullptr, (unsigned long long *)d_wk, st);
    if (e != hipSuccess) return fail_hip(e, "walk kernel launch");
    unsigned long long hwk[6] = {0, 0, 0, 0, 0, 0};
    WK_HIP(hipMemcpyAsync(ext, d_ext, cells, hipMemcpyDeviceToHost, st));
    WK_HIP(hipMemcpyAsync(steps, d_steps, Q * 4, hipMemcpyDeviceToHost, st));
    WK_HIP(hipMemcpyAsync(stop, d_stop, Q, hipMemcpyDeviceToHost, st));
    if (support) WK_HIP(hipMemcpyAsync(support, d_sup, cells * 4, hipMemcpyDeviceToHost, st));
    if (last) WK_HIP(hipMemcpyAsync(last, d_last, Q * 32, hipMemcpyDeviceToHost, st));
    WK_HIP(hipMemcpyAsync(hwk, d_wk, sizeof hwk, hipMemcpyDeviceToHost, st));
    WK_HIP(hipStreamSynchronize(st));
    if (work6)
        for (int i = 1; i < 6; ++i) work6[i] += hwk[i];
    return RSBWT_OK;
}

}  // namespace rsb
