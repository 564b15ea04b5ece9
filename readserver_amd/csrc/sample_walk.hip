// sample_walk.hip -- walks through ONE SAMPLE SET's reads on the GPU (gfx950): rsbwt_set_walk_samples /
// rsbwt_set_extension_samples (include/rsbwt.h: the definition; sample_walk_rule.h: the host's share).  The support of a
// symbol is not the width of its candidate's interval (walk.hip) but the sum, over the distinct reads that hold the
// candidate, of their records whose sample the caller's mask names: rsbwt_set_sample_counts' tally, reduced to one number
// per (seed, base, strand) and made once per appended symbol.
//
// A FIXED SEQUENCE OF LAUNCHES PER STEP, enqueued blind max_steps times (DESIGN 8p says why not one persistent launch:
// a step's rows differ by orders of magnitude between seeds and need a lane per row, so the step wants grids of its own,
// and launch_locate is a persistent draw kernel already).  The host never waits between steps: what a launch needs to
// know -- whether any seed still walks, how many rows the step has -- it reads from HBM: live[it] (seeds walking when step
// `it` starts; every launch of the step leaves at once where it is 0) and total[it].
//   INIT    a lane per seed: the context as ranks into the seed's ring (HBM, 256 bytes), validity, live[0].
//   SEARCH  walk_kernel's mapping: a workgroup of NW waves owns 8 seeds, lanes = (seed, base, strand), wave w searches
//           shards w, w + NW, ...; the rings of the 8 seeds are copied to LDS first, walk_search runs off them.  Every
//           (unit = seed x 8 + base x 2 + strand, shard) interval goes to iv[] as {lower, rows}.
//   PLAN    one workgroup: matches of every unit over the shards; WIDE per seed (any unit above max_rows: none of the
//           seed's rows are made); ufirst[] = the exclusive scan of the units' rows; total[it]; the set's slot mask for
//           this step (a power of two above twice the rows).
//   ROWS    a lane per row: unit by binary search in ufirst[], shard by walking the unit's S widths; and the step's
//           slots of the set are emptied -- the set is CLEARED PER STEP, only as far as this step uses it.
//   LOCATE  launch_locate with the device's count (d_n): a lane per row, whatever the widths.
//   TALLY   a lane per row: head bit; (shard, unit, ordinal) into the open-addressing set of u64 keys -- every access to a
//           slot is the 64-bit compare-and-swap itself (sample_counts.hip says why: L2 is per XCD); the carrier reads its
//           records (sample_records.h, record_sums) and adds ONE number to msup[unit]: the records whose code's column
//           has its bit in the mask (the bitmap and the dictionary's keys in LDS while the keys fit TALLY_LDS_BYTES),
//           or their c fields with RSBWT_WALK_SAMPLE_COPIES.  No matrix is built.
//   DECIDE  a lane per seed: the two strands added, a negative total 0, WIDE first, then sample_walk_step; the symbol,
//           its support and the moved ring are stored, live[it + 1] counted, msup[] zeroed for the next step.
// All sums are integers and every add is an atomic on a cell of its own: bit-identical from run to run.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "../../include/rsbwt.h"
#include "capi_internal.h"
#include "kernels.h"
#include "line_format.h"
#include "match_lanes.h"
#include "rank_device.h"
#include "sample_records.h"
#include "sample_walk_rule.h"
#include "walk_search.h"
#include "wave_lines.h"

namespace rsb {

namespace {

static_assert(SAMPLE_WALK_DEAD_END == RSBWT_WALK_DEAD_END && SAMPLE_WALK_BRANCH == RSBWT_WALK_BRANCH && SAMPLE_WALK_LIMIT == RSBWT_WALK_LIMIT &&
                  SAMPLE_WALK_INVALID == RSBWT_WALK_INVALID && SAMPLE_WALK_WIDE == RSBWT_WALK_WIDE && SAMPLE_WALK_COPIES == RSBWT_WALK_SAMPLE_COPIES,
              "sample_walk_rule.h speaks include/rsbwt.h's codes");

constexpr unsigned long long SW_EMPTY = ~0ull;
constexpr uint32_t SW_PLAN_THREADS = 1024;

struct sw_dev {
    const shard_view *views;
    const meta_view *meta;
    uint32_t S;
    walk_batch bt;
    uint64_t max_rows;
    const uint64_t *keys;
    const uint32_t *mask_bits;
    uint32_t C, size_of_sample, has_other, copies, evaluate_only;
    // the slice's state
    uint8_t *ring;     // [Q][WALK_RING]
    uint32_t *head;    // [Q]
    uint8_t *alive;    // [Q]
    uint8_t *wide;     // [Q]
    ulonglong2 *iv;    // [Q * 8][S]: {lower, rows}
    uint64_t *umatch;  // [Q * 8]
    uint64_t *ufirst;  // [Q * 8 + 1]
    long long *msup;   // [Q * 8]
    uint64_t *total;   // [steps]
    uint32_t *live;    // [steps + 1]
    uint64_t *setmask;  // [1]
    unsigned long long *set;
    uint64_t *rows, *od;  // [cap]
    uint32_t *sh;         // [cap]
    // outputs
    char *ext;
    uint32_t *steps;
    uint8_t *stop;
    uint32_t *support;
    unsigned long long *last;
    long long *raw;
    uint64_t *matches8;
    uint8_t *wide_out;
    unsigned long long *work, *locate_work;
};

__device__ __forceinline__ void sw_count(unsigned long long *work, int which, unsigned long long v) {
    if (v) atomicAdd(&work[(size_t)which * TALLY_WORK_STRIDE], v);
}

__global__ void __launch_bounds__(256)
sw_init_kernel(const sw_dev a) {
    const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= a.bt.Q) return;
    const uint64_t Lq = walk_seed_len(a.bt, q);
    bool ok = Lq >= a.bt.ctx;
    if (ok) {
        const uint8_t *text = reinterpret_cast<const uint8_t *>(a.bt.text);
        const uint64_t from = (a.bt.flags & RSBWT_WALK_LEFT) ? a.bt.off[q] : a.bt.off[q + 1] - a.bt.ctx;
        for (uint32_t i = 0; i < a.bt.ctx; ++i) {
            const uint32_t r = ms_rank(text[from + i]);
            a.ring[q * WALK_RING + i] = (uint8_t)r;
            if (r == 0u) ok = false;
        }
    }
    a.head[q] = 0u;
    a.alive[q] = ok ? 1u : 0u;
    a.wide[q] = 0u;
    for (uint32_t l = 0; l < 8u; ++l) a.msup[q * 8u + l] = 0ll;
    if (!a.evaluate_only) {
        a.steps[q] = 0u;
        if (!ok) {
            a.stop[q] = (uint8_t)RSBWT_WALK_INVALID;
            if (a.last)
                for (uint32_t b = 0; b < 4u; ++b) a.last[4u * q + b] = 0ull;
        }
    }
    if (ok) atomicAdd(&a.live[0], 1u);
}

template <int NW>
__global__ void __launch_bounds__(64 * NW)
sw_search_kernel(const sw_dev a, const uint32_t it) {
    __shared__ uint4 s_stage[NW][64 * SLOT_U4];
    __shared__ uint8_t s_ring[WALK_SEEDS][WALK_RING];
    if (a.live[it] == 0u) return;  // (the same for every lane of the launch)
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint4 *stage = s_stage[wave];
    const uint32_t stage_lds = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)(lds_void_ptr)stage);
    const staged_line L = {own_stage_row(stage, lane), lane & 7u};
    const uint32_t seed = lane >> 3, base = (lane >> 1) & 3u, rev = lane & 1u;
    const bool both = (a.bt.flags & RSBWT_WALK_BOTH_STRANDS) != 0u, left = (a.bt.flags & RSBWT_WALK_LEFT) != 0u;
    const size_t first_q = (size_t)blockIdx.x * WALK_SEEDS, q = first_q + seed;
    for (uint32_t s = 0; s < WALK_SEEDS; ++s)
        if (first_q + s < a.bt.Q)
            for (uint32_t i = threadIdx.x; i < a.bt.ctx; i += blockDim.x) s_ring[s][i] = a.ring[(first_q + s) * WALK_RING + i];
    __syncthreads();
    const bool walking = q < a.bt.Q && a.alive[q] != 0u;
    const walk_cand cd = {s_ring[seed], walking ? a.head[q] : 0u, a.bt.ctx, base + 1u, left, rev != 0u};
    walk_tally tally;
    for (uint32_t sid = wave; sid < a.S; sid += (uint32_t)NW) {
        uint64_t lo = 0;
        const uint64_t rows = walk_search(a.views + sid, walking && (both || rev == 0u), cd, lane, stage_lds, L, tally, &lo);
        if (q < a.bt.Q) a.iv[(q * 8u + (lane & 7u)) * a.S + sid] = make_ulonglong2(rows ? lo : 0ull, rows);
    }
    const unsigned long long s1 = ms_wave_sum(tally.searches), s2 = ms_wave_sum(tally.steps);
    if (lane == 0u) {
        sw_count(a.work, SW_WORK_SEARCHES, s1);
        sw_count(a.work, SW_WORK_SEARCH_STEPS, s2);
    }
}

__global__ void __launch_bounds__(SW_PLAN_THREADS)
sw_plan_kernel(const sw_dev a, const uint32_t it) {
    __shared__ uint64_t s_sum[SW_PLAN_THREADS];
    if (a.live[it] == 0u) return;
    const uint32_t tid = threadIdx.x;
    const size_t U = a.bt.Q * 8u;
    for (size_t u = tid; u < U; u += SW_PLAN_THREADS) {
        uint64_t m = 0;
        for (uint32_t p = 0; p < a.S; ++p) m += a.iv[u * a.S + p].y;
        a.umatch[u] = m;
    }
    __syncthreads();
    for (size_t q = tid; q < a.bt.Q; q += SW_PLAN_THREADS) a.wide[q] = a.alive[q] != 0u && sample_walk_wide(a.umatch + q * 8u, a.max_rows) ? 1u : 0u;
    __syncthreads();
    // the exclusive scan of the units' rows: a thread sums a run of units, the runs' sums are scanned in LDS
    const size_t chunk = (U + SW_PLAN_THREADS - 1) / SW_PLAN_THREADS, u0 = (size_t)tid * chunk, u1 = u0 + chunk < U ? u0 + chunk : U;
    uint64_t mine = 0;
    for (size_t u = u0; u < u1; ++u) mine += a.wide[u >> 3] ? 0ull : a.umatch[u];
    s_sum[tid] = mine;
    __syncthreads();
    for (uint32_t d = 1; d < SW_PLAN_THREADS; d <<= 1) {
        const uint64_t add = tid >= d ? s_sum[tid - d] : 0ull;
        __syncthreads();
        s_sum[tid] += add;
        __syncthreads();
    }
    uint64_t at = s_sum[tid] - mine;
    for (size_t u = u0; u < u1; ++u) {
        a.ufirst[u] = at;
        at += a.wide[u >> 3] ? 0ull : a.umatch[u];
    }
    if (tid == SW_PLAN_THREADS - 1u) {
        const uint64_t total = s_sum[tid];
        a.ufirst[U] = total;
        a.total[it] = total;
        a.setmask[0] = sample_walk_set_slots(total) - 1ull;
        sw_count(a.work, SW_WORK_ROWS, total);
    }
}

// the unit of row t: the last u with ufirst[u] <= t (its successor's first row lies above t, so it has rows)
__device__ __forceinline__ size_t sw_unit_of(const uint64_t *ufirst, size_t U, uint64_t t) {
    size_t lo = 0, hi = U;
    while (hi - lo > 1) {
        const size_t mid = lo + (hi - lo) / 2;
        if (ufirst[mid] <= t) lo = mid;
        else hi = mid;
    }
    return lo;
}

__global__ void __launch_bounds__(256)
sw_rows_kernel(const sw_dev a, const uint32_t it) {
    if (a.live[it] == 0u) return;
    const uint64_t T = a.total[it], slots = a.setmask[0] + 1ull;
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (uint64_t)gridDim.x * blockDim.x;
    const size_t U = a.bt.Q * 8u;
    for (uint64_t i = g; i < slots; i += stride) a.set[i] = SW_EMPTY;
    for (uint64_t t = g; t < T; t += stride) {
        const size_t u = sw_unit_of(a.ufirst, U, t);
        uint64_t r = t - a.ufirst[u], row = ~0ull;
        uint32_t sh = ~0u;
        for (uint32_t p = 0; p < a.S; ++p) {
            const ulonglong2 v = a.iv[u * a.S + p];
            if (r < v.y) {
                row = v.x + r;
                sh = p;
                break;
            }
            r -= v.y;
        }
        a.rows[t] = row;
        a.sh[t] = sh;
    }
}

template <bool KEYS_IN_LDS>
__global__ void __launch_bounds__(256)
sw_tally_kernel(const sw_dev a, const uint32_t it) {
    extern __shared__ uint64_t lds_keys[];
    if (a.live[it] == 0u) return;
    const uint64_t T = a.total[it];
    if (T == 0ull) return;  // (the same for every lane of the launch)
    const tally_dict d = tally_dict_of<KEYS_IN_LDS>(a.keys, a.C, lds_keys);
    const uint32_t *bits = a.mask_bits;
    if (KEYS_IN_LDS) {
        uint32_t *lb = reinterpret_cast<uint32_t *>(lds_keys + a.C);
        for (uint32_t i = threadIdx.x; i < (uint32_t)sample_walk_mask_words(a.C); i += blockDim.x) lb[i] = a.mask_bits[i];
        __syncthreads();
        bits = lb;
    }
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t R = a.size_of_sample + (a.has_other ? 2u : 0u);
    const size_t U = a.bt.Q * 8u;
    const uint64_t slotmask = a.setmask[0];
    const uint64_t gw = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nw = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    unsigned long long n_heads = 0, n_carriers = 0, n_lost = 0, n_records = 0;
    for (uint64_t t0 = gw * 64ull; t0 < T; t0 += nw * 64ull) {  // (every lane of a wave makes the same rounds)
        const uint64_t t = t0 + lane;
        bool carrier = false;
        uint64_t o = 0;
        size_t u = 0;
        meta_view mv = {nullptr, nullptr, 0, nullptr};
        if (t < T) {
            const uint32_t sh = a.sh[t];
            o = a.od[t];
            const bool lost = o == ~0ull;  // (launch_locate: the walk did not end)
            bool head = false;
            if (!lost && sh < a.S) {
                mv = a.meta[sh];
                head = mv.off && mv.heads && o < mv.num_strings && o < (1ull << 40) && ((mv.heads[o >> 5] >> (o & 31u)) & 1u);
            }
            n_lost += lost ? 1u : 0u;
            if (head) {
                ++n_heads;
                u = sw_unit_of(a.ufirst, U, t);
                const unsigned long long key = sample_walk_key(sh, (uint32_t)u, o);
                uint64_t h = key * 0x9E3779B97F4A7C15ull;
                uint64_t slot = (h ^ (h >> 29)) & slotmask;
                for (;;) {
                    const unsigned long long old = atomicCAS(&a.set[slot], SW_EMPTY, key);
                    if (old == SW_EMPTY) {
                        carrier = true;
                        break;
                    }
                    if (old == key) break;
                    slot = (slot + 1ull) & slotmask;
                }
            }
        }
        uint64_t nrec = 0;
        const uint8_t *val = nullptr;
        if (carrier) {
            const uint64_t b0 = mv.off[o], b1 = mv.off[o + 1];
            nrec = (b1 - b0) / R;  // (the tail that is no whole record is dropped)
            val = mv.bytes + b0;
            ++n_carriers;
            n_records += nrec;
        }
        const long long sum = record_sums(R, lane, nrec, val, [&](const uint8_t *p) -> long long {
            uint64_t key = 0;
            for (uint32_t b = 0; b < a.size_of_sample; ++b) key = (key << 8) | p[b];
            if (!sample_walk_counts(bits, a.C, tally_column(d, key))) return 0ll;
            return a.copies && a.has_other ? (long long)(int)(signed char)p[a.size_of_sample] - 33ll : 1ll;
        });
        if (carrier && sum != 0ll) atomicAdd(reinterpret_cast<unsigned long long *>(a.msup) + u, (unsigned long long)sum);
    }
    const unsigned long long w1 = ms_wave_sum(n_heads), w2 = ms_wave_sum(n_carriers), w3 = ms_wave_sum(n_lost), w4 = ms_wave_sum(n_records);
    if (lane == 0u) {
        sw_count(a.work, SW_WORK_HEADS, w1);
        sw_count(a.work, SW_WORK_CARRIERS, w2);
        sw_count(a.work, SW_WORK_LOST, w3);
        sw_count(a.work, SW_WORK_RECORDS, w4);
    }
}

__global__ void __launch_bounds__(256)
sw_decide_kernel(const sw_dev a, const uint32_t it) {
    const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= a.bt.Q) return;
    const bool any = a.live[it] != 0u;
    const bool alive = any && a.alive[q] != 0u;
    if (a.evaluate_only) {  // (one evaluation: what this device's shards say, undecided)
        const bool wide = alive && a.wide[q] != 0u;
        for (uint32_t l = 0; l < 8u; ++l) {
            a.raw[q * 8u + l] = alive && !wide ? a.msup[q * 8u + l] : 0ll;
            a.matches8[q * 8u + l] = alive ? a.umatch[q * 8u + l] : 0ull;
        }
        a.wide_out[q] = wide ? 1u : 0u;
        return;
    }
    if (!alive) return;
    uint64_t sup[4];
    for (uint32_t b = 0; b < 4u; ++b) {
        sup[b] = sample_walk_support(a.msup[q * 8u + 2u * b], a.msup[q * 8u + 2u * b + 1u]);
        a.msup[q * 8u + 2u * b] = 0ll;
        a.msup[q * 8u + 2u * b + 1u] = 0ll;
    }
    const bool wide = a.wide[q] != 0u;
    uint32_t pick = 0, nsteps = a.steps[q];
    uint32_t why = sample_walk_step(sup, wide, a.bt.min_count, &pick);
    if (why == SAMPLE_WALK_GO) {
        const size_t at = q * (size_t)a.bt.max_steps + nsteps;
        a.ext[at] = "ACGT"[pick];
        if (a.support) a.support[at] = sup[pick] > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)sup[pick];
        sw_count(a.work, SW_WORK_APPENDED, 1ull);
        // the context moves on by one symbol (walk_kernel's ring)
        uint32_t head = a.head[q];
        if (a.bt.flags & RSBWT_WALK_LEFT) {
            head = head == 0u ? a.bt.ctx - 1u : head - 1u;
            a.ring[q * WALK_RING + head] = (uint8_t)(pick + 1u);
        } else {
            a.ring[q * WALK_RING + head] = (uint8_t)(pick + 1u);
            head = head + 1u == a.bt.ctx ? 0u : head + 1u;
        }
        a.head[q] = head;
        a.steps[q] = ++nsteps;
        if (nsteps == a.bt.max_steps) why = SAMPLE_WALK_LIMIT;
    }
    if (why == SAMPLE_WALK_GO) {
        atomicAdd(&a.live[it + 1u], 1u);
        return;
    }
    if (why == SAMPLE_WALK_WIDE) sw_count(a.work, SW_WORK_WIDE, 1ull);
    a.alive[q] = 0u;
    a.stop[q] = (uint8_t)why;
    if (a.last)
        for (uint32_t b = 0; b < 4u; ++b) a.last[4u * q + b] = why == SAMPLE_WALK_LIMIT || why == SAMPLE_WALK_WIDE ? 0ull : sup[b];
}

// the slice's locate counters into the call's
__global__ void sw_fold_kernel(const sw_dev a) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    sw_count(a.work, SW_WORK_LOCATED, a.locate_work[0]);
    sw_count(a.work, SW_WORK_LOCATE_STEPS, a.locate_work[1]);
}

__global__ void sw_status_kernel(const unsigned long long *__restrict__ work, uint64_t *__restrict__ status8) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    auto w = [&](int which) { return (uint64_t)work[(size_t)which * TALLY_WORK_STRIDE]; };
    status8[0] = w(SW_WORK_ROWS);
    status8[1] = w(SW_WORK_HEADS);
    status8[2] = w(SW_WORK_CARRIERS);
    status8[3] = w(SW_WORK_RECORDS);
    status8[4] = w(SW_WORK_APPENDED);
    status8[5] = w(SW_WORK_LOCATE_STEPS);
    status8[6] = w(SW_WORK_LOST);
    status8[7] = w(SW_WORK_WIDE);
}

// the scratch of a slice, in this order; `ctl` bytes from the front are zeroed before the walk
struct sw_layout {
    size_t ring, head, alive, wide, iv, umatch, ufirst, msup, total, live, setmask, locate_work, ctl, rows, od, sh, set, bytes;
};

sw_layout sw_lay(size_t Q, uint32_t S, uint32_t steps, uint64_t max_rows) {
    sw_layout l;
    size_t at = 0;
    auto put = [&](size_t bytes) {
        const size_t here = at;
        at += al256(bytes);
        return here;
    };
    const uint64_t cap = sample_walk_cap_rows(Q, max_rows);
    l.ring = put(Q * WALK_RING);
    l.head = put(Q * 4);
    l.alive = put(Q);
    l.wide = put(Q);
    l.iv = put(Q * 8 * (size_t)S * 16);
    l.umatch = put(Q * 8 * 8);
    l.ufirst = put((Q * 8 + 1) * 8);
    l.msup = put(Q * 8 * 8);
    l.total = put((size_t)steps * 8);
    l.live = put(((size_t)steps + 1) * 4);
    l.setmask = put(8);
    l.locate_work = put(16);
    l.ctl = at;
    l.rows = put((size_t)cap * 8);
    l.od = put((size_t)cap * 8);
    l.sh = put((size_t)cap * 4);
    l.set = put((size_t)sample_walk_set_slots(cap) * 8);
    l.bytes = at;
    return l;
}

}  // namespace

size_t sample_walk_bytes(size_t Q, uint32_t S, uint32_t max_steps, uint64_t max_rows) { return sw_lay(Q, S, max_steps, max_rows).bytes; }

hipError_t sample_walk_enqueue(scratch_cache &scratch, const sample_walk_args &g, void *d_scratch, hipStream_t stream) {
    const size_t Q = g.bt.Q;
    if (Q == 0 || g.S == 0) return hipSuccess;
    if (g.bt.ctx == 0u || g.bt.ctx >= WALK_RING || g.bt.min_count == 0ull || !sample_walk_rows_ok(g.max_rows) || Q > SAMPLE_WALK_SLICE_SEEDS ||
        g.S > SAMPLE_WALK_MAX_SHARDS || g.C == 0u)
        return hipErrorInvalidValue;
    const uint32_t steps = g.evaluate_only ? 1u : g.bt.max_steps;
    if (steps == 0u) return hipErrorInvalidValue;
    const sw_layout l = sw_lay(Q, g.S, steps, g.max_rows);
    uint8_t *b = (uint8_t *)d_scratch;
    sw_dev a;
    a.views = g.views;
    a.meta = g.meta;
    a.S = g.S;
    a.bt = g.bt;
    a.max_rows = g.max_rows;
    a.keys = g.keys;
    a.mask_bits = g.mask_bits;
    a.C = g.C;
    a.size_of_sample = g.size_of_sample;
    a.has_other = g.has_other;
    a.copies = (g.bt.flags & RSBWT_WALK_SAMPLE_COPIES) ? 1u : 0u;
    a.evaluate_only = g.evaluate_only ? 1u : 0u;
    a.ring = b + l.ring;
    a.head = (uint32_t *)(b + l.head);
    a.alive = b + l.alive;
    a.wide = b + l.wide;
    a.iv = (ulonglong2 *)(b + l.iv);
    a.umatch = (uint64_t *)(b + l.umatch);
    a.ufirst = (uint64_t *)(b + l.ufirst);
    a.msup = (long long *)(b + l.msup);
    a.total = (uint64_t *)(b + l.total);
    a.live = (uint32_t *)(b + l.live);
    a.setmask = (uint64_t *)(b + l.setmask);
    a.locate_work = (unsigned long long *)(b + l.locate_work);
    a.rows = (uint64_t *)(b + l.rows);
    a.od = (uint64_t *)(b + l.od);
    a.sh = (uint32_t *)(b + l.sh);
    a.set = (unsigned long long *)(b + l.set);
    a.ext = (char *)g.ext;
    a.steps = (uint32_t *)g.steps;
    a.stop = (uint8_t *)g.stop;
    a.support = (uint32_t *)g.support;
    a.last = (unsigned long long *)g.last;
    a.raw = (long long *)g.raw;
    a.matches8 = (uint64_t *)g.matches8;
    a.wide_out = (uint8_t *)g.wide;
    a.work = g.work;

    hipError_t e = hipMemsetAsync(b, 0, l.ctl, stream);
    if (e != hipSuccess) return e;
    if (!g.evaluate_only) {
        // every byte past a walk's steps is 0
        if ((e = hipMemsetAsync(g.ext, 0, Q * (size_t)g.bt.max_steps, stream)) != hipSuccess) return e;
        if (g.support && (e = hipMemsetAsync(g.support, 0, Q * (size_t)g.bt.max_steps * 4, stream)) != hipSuccess) return e;
    }
    const unsigned per_seed = (unsigned)((Q + 255) / 256), groups = (unsigned)((Q + WALK_SEEDS - 1) / WALK_SEEDS);
    const uint64_t cap = sample_walk_cap_rows(Q, g.max_rows);
    const uint64_t want = (cap + 255) / 256, most = (uint64_t)(g.num_cus > 0 ? g.num_cus : 64) * 8u;
    const unsigned per_row = (unsigned)(want < most ? (want ? want : 1) : most);
    const bool in_lds = (size_t)g.C * 8 <= TALLY_LDS_BYTES;
    const size_t lds = in_lds ? (size_t)g.C * 8 + sample_walk_mask_words(g.C) * 4 : 0;
    auto mark = [&]() {
        hipEvent_t ev = nullptr;
        if (g.marks && hipEventCreate(&ev) == hipSuccess) {
            (void)hipEventRecord(ev, stream);
            g.marks->push_back(ev);
        }
    };
    mark();
    hipLaunchKernelGGL(sw_init_kernel, dim3(per_seed), dim3(256), 0, stream, a);
    mark();
    for (uint32_t it = 0; it < steps; ++it) {
        if (g.S >= (uint32_t)WG_WAVES) hipLaunchKernelGGL(sw_search_kernel<WG_WAVES>, dim3(groups), dim3(64 * WG_WAVES), 0, stream, a, it);
        else if (g.S >= 2u) hipLaunchKernelGGL(sw_search_kernel<2>, dim3(groups), dim3(128), 0, stream, a, it);
        else hipLaunchKernelGGL(sw_search_kernel<1>, dim3(groups), dim3(64), 0, stream, a, it);
        mark();
        hipLaunchKernelGGL(sw_plan_kernel, dim3(1), dim3(SW_PLAN_THREADS), 0, stream, a, it);
        mark();
        hipLaunchKernelGGL(sw_rows_kernel, dim3(per_row), dim3(256), 0, stream, a, it);
        mark();
        if ((e = hipGetLastError()) != hipSuccess) return e;
        e = launch_locate(scratch, g.views, g.S, a.sh, a.rows, (size_t)cap, g.max_locate_steps, nullptr, a.od, nullptr, a.locate_work, g.num_cus, stream,
                          a.total + it);
        if (e != hipSuccess) return e;
        mark();
        if (in_lds) hipLaunchKernelGGL(sw_tally_kernel<true>, dim3(per_row), dim3(256), lds, stream, a, it);
        else hipLaunchKernelGGL(sw_tally_kernel<false>, dim3(per_row), dim3(256), 0, stream, a, it);
        mark();
        hipLaunchKernelGGL(sw_decide_kernel, dim3(per_seed), dim3(256), 0, stream, a, it);
        mark();
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(sw_fold_kernel, dim3(1), dim3(64), 0, stream, a);
    return hipGetLastError();
}

namespace {
// mask u8[C] -> a bit per column, a lane per word (sample_walk_mask_bits on the device)
__global__ void __launch_bounds__(256)
sw_mask_kernel(const uint8_t *__restrict__ mask, size_t C, uint32_t *__restrict__ bits) {
    const size_t w = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= sample_walk_mask_words(C)) return;
    uint32_t v = 0;
    for (uint32_t i = 0; i < 32u && w * 32u + i < C; ++i) v |= mask[w * 32u + i] ? 1u << i : 0u;
    bits[w] = v;
}
}  // namespace

hipError_t launch_sample_walk_mask(const void *d_mask, size_t C, void *d_bits, hipStream_t stream) {
    hipLaunchKernelGGL(sw_mask_kernel, dim3((unsigned)((sample_walk_mask_words(C) + 255) / 256)), dim3(256), 0, stream, (const uint8_t *)d_mask, C,
                       (uint32_t *)d_bits);
    return hipGetLastError();
}

hipError_t launch_sample_walk_status(const unsigned long long *d_work, void *d_status8, hipStream_t stream) {
    hipLaunchKernelGGL(sw_status_kernel, dim3(1), dim3(64), 0, stream, d_work, (uint64_t *)d_status8);
    return hipGetLastError();
}

}  // namespace rsb
