// paths.hip -- every path from a seed through the reads' k-mer graph, depth first, on the GPU (gfx950): where a walk stops
// at the first fork, rsbwt_set_paths goes through it, A before C before G before T, and comes back for the others
// (include/rsbwt.h: the definition; paths_rule.h: the decisions).  The dependent loop -- an evaluation needs the sum over
// every shard, the next node needs the evaluation, a backtrack needs the path before it -- stays inside one launch.
//
// MAPPING: walk_kernel's (walk.hip).  A workgroup of NW waves owns 8 seeds, the lanes of every wave are (seed, base,
// strand), wave w searches shards w, w + NW, ... with walk_search (walk_search.h), the partial counts meet in s_part.
// What is new is the state of a seed's search, and it belongs to ONE lane: the seed's WRITER, lane 8 * seed of wave 0.
//   * ROUND.  barrier; every lane reads s_live (0: the workgroup leaves), and of its seed s_go and s_head; the lanes of the
//     seeds that go search the current node's four candidates; s_part; barrier; each writer sums its seed's counts, takes
//     every decision up to the next node to evaluate -- the append, the end test, a path's outputs, the state, the backtrack
//     -- and publishes {s_go, s_head}; wave 0 counts the seeds still searching into s_live.  A round is one evaluation of
//     every seed still searching, so the loop runs max_evals times at the most whatever the data says (the end test gives
//     BUDGET after that many); a stopped, an invalid or a missing seed idles its lanes inside the loop and a wave without
//     a shard writes zeros and reaches both barriers.
//   * PATH STORE: the output itself.  The current path is written into its own slot of d_ext as it grows; a backtrack to
//     depth d copies the d symbols it keeps from the slot of the path just finished into the next slot.
//   * FRAME STORE: HBM scratch, min(max_steps, max_evals) frames of 32 bytes per seed (paths_rule.h).
//   * The context ring is rebuilt after a backtrack from the seed's text and the new slot's last symbols.
//   Both stores are written AND read back by the seed's writer lane alone, so every read-back is a thread's load of its
//   own earlier store: program order, no cache and no barrier to rely on.  The other lanes learn of a backtrack through
//   LDS only (the rebuilt ring, s_head).  No workgroup reads what another wrote; nothing synchronises across the grid.
//   * The targets sit in LDS as ranks beside the rings (a symbol outside ACGT is rank 0 and equals no ring symbol), so the
//     end test reads LDS alone.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "capi_internal.h"
#include "kernels.h"
#include "paths_rule.h"
#include "walk_search.h"

namespace rsb {

namespace {

static_assert(PATHS_DEAD_END == RSBWT_WALK_DEAD_END && PATHS_LIMIT == RSBWT_WALK_LIMIT && PATHS_TARGET == RSBWT_WALK_TARGET &&
                  PATHS_BUDGET == RSBWT_WALK_BUDGET && PATHS_COMPLETE == RSBWT_PATHS_COMPLETE && PATHS_MORE == RSBWT_PATHS_MORE &&
                  PATHS_OUT_OF_BUDGET == RSBWT_PATHS_BUDGET && PATHS_INVALID == RSBWT_PATHS_INVALID,
              "paths_rule.h speaks include/rsbwt.h's stop codes and seed states");
static_assert(sizeof(paths_frame) == 32, "a frame is 32 bytes");

// the length of seed q's target: 0 where there is none, where it does not fit the targets' text or is longer than ctx
__device__ __forceinline__ uint32_t paths_target_len(const paths_batch &pb, size_t q) {
    if (!pb.ttext || !pb.toff || q >= pb.seeds.Q) return 0u;
    const uint64_t b = pb.toff[q], e = pb.toff[q + 1];
    return (b <= e && e <= (uint64_t)pb.TN && e - b <= (uint64_t)pb.seeds.ctx) ? (uint32_t)(e - b) : 0u;
}

template <int NW>  // the waves of a workgroup, as walk_kernel's
__global__ void __launch_bounds__(64 * NW)
paths_kernel(const shard_view *__restrict__ shards, const uint32_t nshards, const paths_batch pb, paths_frame *frames, char *ext,
             uint32_t *__restrict__ steps_out, uint8_t *__restrict__ stop_out, uint32_t *__restrict__ min_out, uint32_t *__restrict__ npaths_out,
             uint8_t *__restrict__ state_out, unsigned long long *__restrict__ work) {
    __shared__ uint4 s_stage[NW][64 * SLOT_U4];
    __shared__ uint8_t s_ring[WALK_SEEDS][WALK_RING];
    __shared__ uint8_t s_target[WALK_SEEDS][WALK_RING];
    __shared__ unsigned long long s_part[NW][WALK_SEEDS * 4];
    __shared__ uint32_t s_bad[WALK_SEEDS], s_tlen[WALK_SEEDS], s_go[WALK_SEEDS], s_head[WALK_SEEDS];
    __shared__ uint32_t s_live;
    const walk_batch &bt = pb.seeds;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint4 *stage = s_stage[wave];
    const uint32_t stage_lds = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)(lds_void_ptr)stage);
    const staged_line L = {own_stage_row(stage, lane), lane & 7u};
    const uint32_t seed = lane >> 3, base = (lane >> 1) & 3u, rev = lane & 1u;
    const bool both = (bt.flags & RSBWT_WALK_BOTH_STRANDS) != 0u, left = (bt.flags & RSBWT_WALK_LEFT) != 0u;
    const size_t first_q = (size_t)blockIdx.x * WALK_SEEDS, q = first_q + seed;
    const bool writer = wave == 0u && (lane & 7u) == 0u;  // the one lane that holds its seed's search
    const uint32_t ctx = bt.ctx, max_steps = bt.max_steps;

    if (threadIdx.x < WALK_SEEDS) {
        s_bad[threadIdx.x] = 0u;
        s_tlen[threadIdx.x] = paths_target_len(pb, first_q + threadIdx.x);
    }
    __syncthreads();
    walk_load_rings(bt, first_q, s_ring, s_bad, threadIdx.x, blockDim.x);
    for (uint32_t s = 0; s < WALK_SEEDS; ++s) {  // the targets as ranks (s_tlen <= ctx < WALK_RING, inside the targets' text)
        const uint32_t tl = s_tlen[s];
        if (tl == 0u) continue;
        const uint8_t *tt = reinterpret_cast<const uint8_t *>(pb.ttext) + pb.toff[first_q + s];
        for (uint32_t i = threadIdx.x; i < tl; i += blockDim.x) s_target[s][i] = (uint8_t)ms_rank(tt[i]);
    }
    __syncthreads();

    // ---- the writer's state of its seed's search
    const bool valid = q < bt.Q && walk_seed_len(bt, q) >= ctx && s_bad[seed] == 0u;
    bool searching = valid;
    uint32_t steps = 0, evals = 0, nframes = 0, npaths = 0, min_cur = PATHS_NO_SUPPORT, head = 0;
    uint32_t appended = 0;  // (the writer's)
    walk_tally tally;
    const uint32_t tlen = s_tlen[seed];
    paths_frame *const my_frames = frames + (q < bt.Q ? q : 0) * (size_t)paths_frames(max_steps, pb.max_evals);
    const uint8_t *const seed_ctx = reinterpret_cast<const uint8_t *>(bt.text) + (valid ? (left ? bt.off[q] : bt.off[q + 1] - ctx) : 0);
    char *slot = ext + (q < bt.Q ? q : 0) * (size_t)pb.max_paths * max_steps;  // the current path's
    // are the symbols at the walking end the target's?  (the ring holds the ctx symbols at that end, in the sequence's order)
    auto at_target = [&]() -> bool {
        if (tlen == 0u) return false;
        const uint32_t from = left ? 0u : ctx - tlen;
        for (uint32_t i = 0; i < tlen; ++i) {
            uint32_t at = head + from + i;
            if (at >= ctx) at -= ctx;
            if (s_ring[seed][at] != s_target[seed][i]) return false;
        }
        return true;
    };
    if (writer) {
        if (q < bt.Q && !valid) {  // an invalid seed
            npaths_out[q] = 0u;
            state_out[q] = (uint8_t)PATHS_INVALID;
        }
        s_go[seed] = searching ? 1u : 0u;
        s_head[seed] = 0u;
    }
    if (wave == 0u) {  // (every lane of wave 0 is in the ballot)
        const uint64_t still = __builtin_amdgcn_ballot_w64(searching && (lane & 7u) == 0u);
        if (lane == 0u) s_live = (uint32_t)__builtin_popcountll(still);
    }

    for (uint32_t round = 0; round < pb.max_evals; ++round) {  // (a searching seed makes one evaluation per round)
        __syncthreads();
        if (s_live == 0u) break;  // (LDS after a barrier: the same for every lane of the workgroup)
        const bool go = s_go[seed] != 0u;
        const walk_cand cd = {s_ring[seed], s_head[seed], ctx, base + 1u, left, rev != 0u};
        unsigned long long cnt = 0;
        for (uint32_t sid = wave; sid < nshards; sid += (uint32_t)NW)
            cnt += walk_search(shards + sid, go && (both || rev == 0u), cd, lane, stage_lds, L, tally);
        cnt += __shfl_xor(cnt, 1, 64);  // the two strands
        if (rev == 0u) s_part[wave][seed * 4u + base] = cnt;
        __syncthreads();
        if (writer && searching) {
            uint64_t sup[4];
            for (uint32_t b = 0; b < 4u; ++b) {
                sup[b] = 0;
                for (uint32_t w = 0; w < (uint32_t)NW; ++w) sup[b] += s_part[w][seed * 4u + b];
            }
            ++evals;
            const uint32_t live = paths_live(sup, bt.min_count);
            uint32_t stop = PATHS_DEAD_END;
            if (live != 0u) {
                const uint32_t pick = paths_advance(my_frames, &nframes, steps, live, sup, &min_cur);
                slot[steps++] = "ACGT"[pick];
                ++appended;
                // the context moves on by one symbol
                if (left) {
                    head = head == 0u ? ctx - 1u : head - 1u;
                    s_ring[seed][head] = (uint8_t)(pick + 1u);
                } else {
                    s_ring[seed][head] = (uint8_t)(pick + 1u);
                    head = head + 1u == ctx ? 0u : head + 1u;
                }
                stop = paths_end(at_target(), steps, max_steps, evals, pb.max_evals);
            }
            while (stop != PATHS_GO) {  // (max_paths times at the most: every turn puts a path out)
                const size_t at = q * (size_t)pb.max_paths + npaths;
                steps_out[at] = steps;
                stop_out[at] = (uint8_t)stop;
                if (min_out) min_out[at] = paths_min_out(steps, min_cur);
                ++npaths;
                const uint32_t state = paths_done(stop, nframes, npaths, pb.max_paths);
                if (state != PATHS_GO) {
                    npaths_out[q] = npaths;
                    state_out[q] = (uint8_t)state;
                    searching = false;
                    break;
                }
                // ---- the backtrack: the path is path[:d] + c, in the next slot (npaths < max_paths)
                uint32_t d = 0;
                const uint32_t c = paths_backtrack(my_frames, &nframes, &d, &min_cur);
                char *next = slot + max_steps;
                for (uint32_t i = 0; i < d; ++i) next[i] = slot[i];
                next[d] = "ACGT"[c];
                slot = next;
                steps = d + 1u;
                ++appended;
                // the ring anew, head at 0: the ctx symbols at the walking end of seed + path (reverse(path) + seed)
                head = 0u;
                for (uint32_t i = 0; i < ctx; ++i) {
                    uint32_t r;
                    if (left) r = i < steps ? ms_rank((uint8_t)slot[steps - 1u - i]) : ms_rank(seed_ctx[i - steps]);
                    else r = steps + i < ctx ? ms_rank(seed_ctx[steps + i]) : ms_rank((uint8_t)slot[steps + i - ctx]);
                    s_ring[seed][i] = (uint8_t)r;
                }
                stop = paths_end(at_target(), steps, max_steps, evals, pb.max_evals);
            }
            s_go[seed] = searching ? 1u : 0u;
            s_head[seed] = head;
        }
        if (wave == 0u) {
            const uint64_t still = __builtin_amdgcn_ballot_w64(searching && (lane & 7u) == 0u);
            if (lane == 0u) s_live = (uint32_t)__builtin_popcountll(still);
        }
    }
    walk_add_work(work, lane, tally, appended);
    if (work) {
        const unsigned long long s6 = ms_wave_sum(writer ? evals : 0u), s7 = ms_wave_sum(writer ? npaths : 0u);
        if (lane == 0u) {
            if (s6) atomicAdd(&work[6], s6);
            if (s7) atomicAdd(&work[7], s7);
        }
    }
}

thread_local uint64_t paths_last[8] = {0, 0, 0, 0, 0, 0, 0, 0};

#define PT_HIP(x)                                              \
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

size_t paths_frame_bytes(size_t Q, uint32_t max_steps, uint32_t max_evals) {
    return Q * (size_t)paths_frames(max_steps, max_evals) * sizeof(paths_frame);
}

hipError_t launch_paths(const shard_view *d_shards, uint32_t nshards, const paths_batch &pb, void *d_frames, void *d_ext, void *d_steps, void *d_stop,
                        void *d_min_support, void *d_npaths, void *d_state, unsigned long long *d_work, hipStream_t stream) {
    const walk_batch &bt = pb.seeds;
    if (bt.Q == 0 || nshards == 0) return hipSuccess;
    if (bt.ctx == 0u || bt.ctx >= WALK_RING || bt.max_steps == 0u || bt.max_steps > 65535u || bt.min_count == 0ull) return hipErrorInvalidValue;
    if (pb.max_paths == 0u || pb.max_paths > 256u || pb.max_evals == 0u || pb.max_evals > (1u << 20)) return hipErrorInvalidValue;
    if ((pb.ttext == nullptr) != (pb.toff == nullptr) || !d_frames) return hipErrorInvalidValue;
    const size_t blocks = (bt.Q + WALK_SEEDS - 1) / WALK_SEEDS, slots = bt.Q * (size_t)pb.max_paths;
    if (blocks > 0x7FFFFFFFull || (uint64_t)slots * bt.max_steps >= (1ull << 31)) return hipErrorInvalidValue;
    // every byte past a path's steps and every unused slot is 0
    hipError_t e = hipMemsetAsync(d_ext, 0, slots * (size_t)bt.max_steps, stream);
    if (e == hipSuccess) e = hipMemsetAsync(d_steps, 0, slots * 4, stream);
    if (e == hipSuccess) e = hipMemsetAsync(d_stop, 0, slots, stream);
    if (e == hipSuccess && d_min_support) e = hipMemsetAsync(d_min_support, 0, slots * 4, stream);
    if (e != hipSuccess) return e;
    // no more waves per workgroup than the shards can keep busy
    auto go = [&](auto kernel, unsigned waves) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(64 * waves), 0, stream, d_shards, nshards, pb, (paths_frame *)d_frames, (char *)d_ext,
                           (uint32_t *)d_steps, (uint8_t *)d_stop, (uint32_t *)d_min_support, (uint32_t *)d_npaths, (uint8_t *)d_state, d_work);
    };
    if (nshards >= (uint32_t)WG_WAVES) go(paths_kernel<WG_WAVES>, WG_WAVES);
    else if (nshards >= 2u) go(paths_kernel<2>, 2);
    else go(paths_kernel<1>, 1);
    return hipGetLastError();
}

void paths_set_last_work(const uint64_t work8[8]) {
    for (int i = 0; i < 8; ++i) paths_last[i] = work8 ? work8[i] : 0;
}
void paths_get_last_work(uint64_t work8[8]) { memcpy(work8, paths_last, sizeof paths_last); }

int paths_check_args(uint32_t ctx, uint32_t flags, uint32_t max_steps, uint32_t max_paths, uint32_t max_evals, size_t Q) {
    if (ctx < 1u || ctx > 255u) return fail(RSBWT_EINVAL, "ctx = %u: 1 to 255", ctx);
    if (flags & ~(uint32_t)(RSBWT_WALK_LEFT | RSBWT_WALK_BOTH_STRANDS)) return fail(RSBWT_EINVAL, "unknown flag bits 0x%x", flags);
    if (max_steps < 1u || max_steps > 65535u) return fail(RSBWT_EINVAL, "max_steps = %u: 1 to 65,535", max_steps);
    if (max_paths < 1u || max_paths > 256u) return fail(RSBWT_EINVAL, "max_paths = %u: 1 to 256", max_paths);
    if (max_evals < 1u || max_evals > (1u << 20)) return fail(RSBWT_EINVAL, "max_evals = %u: 1 to 2^20", max_evals);
    // (Q < 2^31 first: the product below then fits 64 bits)
    if ((uint64_t)Q >= (1ull << 31) || (uint64_t)Q * max_paths * max_steps >= (1ull << 31))
        return fail(RSBWT_ERANGE, "%zu seeds x %u paths x %u steps: under 2^31 in one call", Q, max_paths, max_steps);
    return RSBWT_OK;
}

// A paths call on one device on `st`: seeds and targets go up, ONE launch searches every seed over the shards of d_views,
// the answers come back; work8[1..7] += the launch's counters.  Synchronises `st`.
int paths_host_views(scratch_cache &scratch, hipStream_t st, const shard_view *d_views, uint32_t S, const char *t0, const uint64_t *rel, size_t Q,
                     size_t N, const char *tt0, const uint64_t *trel, size_t TN, uint32_t ctx, uint64_t min_count, uint32_t max_steps,
                     uint32_t max_paths, uint32_t max_evals, uint32_t flags, char *ext, uint32_t *steps, uint8_t *stop, uint32_t *min_support,
                     uint32_t *npaths, uint8_t *state, uint64_t *work8) {
    if (Q == 0 || S == 0) return RSBWT_OK;
    const size_t slots = Q * (size_t)max_paths, cells = slots * (size_t)max_steps;
    const size_t a_text = al256(N + 1), a_off = al256((Q + 1) * 8), a_tt = trel ? al256(TN + 1) : 0, a_toff = trel ? al256((Q + 1) * 8) : 0,
                 a_ext = al256(cells), a_steps = al256(slots * 4), a_stop = al256(slots), a_min = min_support ? al256(slots * 4) : 0,
                 a_np = al256(Q * 4), a_state = al256(Q), a_frames = al256(paths_frame_bytes(Q, max_steps, max_evals));
    scratch_cache::lease mem;
    hipError_t e = scratch.take(a_text + a_off + a_tt + a_toff + a_ext + a_steps + a_stop + a_min + a_np + a_state + a_frames + 256, st, &mem);
    if (e != hipSuccess)
        return fail(RSBWT_ENOMEM, "%zu seeds x %u paths x %u steps do not fit the device's free memory: %s", Q, max_paths, max_steps,
                    hipGetErrorString(e));
    give_back give{scratch, mem, st};
    uint8_t *d_text = (uint8_t *)mem.p, *d_off = d_text + a_text, *d_tt = d_off + a_off, *d_toff = d_tt + a_tt, *d_ext = d_toff + a_toff,
            *d_steps = d_ext + a_ext, *d_stop = d_steps + a_steps, *d_min = d_stop + a_stop, *d_np = d_min + a_min, *d_state = d_np + a_np,
            *d_frames = d_state + a_state, *d_wk = d_frames + a_frames;
    if (N) PT_HIP(hipMemcpyAsync(d_text, t0, N, hipMemcpyHostToDevice, st));
    PT_HIP(hipMemcpyAsync(d_off, rel, (Q + 1) * 8, hipMemcpyHostToDevice, st));
    if (trel) {
        if (TN) PT_HIP(hipMemcpyAsync(d_tt, tt0, TN, hipMemcpyHostToDevice, st));
        PT_HIP(hipMemcpyAsync(d_toff, trel, (Q + 1) * 8, hipMemcpyHostToDevice, st));
    }
    PT_HIP(hipMemsetAsync(d_wk, 0, 256, st));
    paths_batch pb;
    pb.seeds.text = (const char *)d_text;
    pb.seeds.off = (const uint64_t *)d_off;
    pb.seeds.Q = Q;
    pb.seeds.N = N;
    pb.seeds.ctx = ctx;
    pb.seeds.max_steps = max_steps;
    pb.seeds.min_count = min_count ? min_count : 1ull;
    pb.seeds.flags = flags;
    pb.ttext = trel ? (const char *)d_tt : nullptr;
    pb.toff = trel ? (const uint64_t *)d_toff : nullptr;
    pb.TN = trel ? TN : 0;
    pb.max_paths = max_paths;
    pb.max_evals = max_evals;
    e = launch_paths(d_views, S, pb, d_frames, d_ext, d_steps, d_stop, min_support ? d_min : nullptr, d_np, d_state, (unsigned long long *)d_wk, st);
    if (e != hipSuccess) return fail_hip(e, "paths kernel launch");
    unsigned long long hwk[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    PT_HIP(hipMemcpyAsync(ext, d_ext, cells, hipMemcpyDeviceToHost, st));
    PT_HIP(hipMemcpyAsync(steps, d_steps, slots * 4, hipMemcpyDeviceToHost, st));
    PT_HIP(hipMemcpyAsync(stop, d_stop, slots, hipMemcpyDeviceToHost, st));
    if (min_support) PT_HIP(hipMemcpyAsync(min_support, d_min, slots * 4, hipMemcpyDeviceToHost, st));
    PT_HIP(hipMemcpyAsync(npaths, d_np, Q * 4, hipMemcpyDeviceToHost, st));
    PT_HIP(hipMemcpyAsync(state, d_state, Q, hipMemcpyDeviceToHost, st));
    PT_HIP(hipMemcpyAsync(hwk, d_wk, sizeof hwk, hipMemcpyDeviceToHost, st));
    PT_HIP(hipStreamSynchronize(st));
    if (work8)
        for (int i = 1; i < 8; ++i) work8[i] += hwk[i];
    return RSBWT_OK;
}

}  // namespace rsb
