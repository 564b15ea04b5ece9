// sample_counts.hip -- rsbwt_set_sample_counts (include/rsbwt.h): which samples carry each query, tallied on the GPU
// (gfx950).  The front half is the capped locate's (search, interval totals / fill, launch_locate: sets.hip); what is
// new here reduces the located rows of a batch to the per-query matrices without a row, an ordinal or a value byte
// leaving the device.
//
//   REGION ROWS  one lane per row: how many rows each shard has (they size the shards' regions of the set below).
//   TALLY        one lane per located row (query by binary search in first[], as interval_rows.hip's fill):
//     1. the head bit of its ordinal in its shard's table (one dword load); a row on an ordinal that is no head is done.
//     2. (query, ordinal) goes into an open-addressing set of u64 keys, one region per shard (so the shard is no part of
//        the key).  EVERY access to a slot is the 64-bit compare-and-swap itself -- a plain load may be served by one
//        XCD's L2 and miss the insert of another XCD; the atomic is performed where all XCDs meet.  Old value empty: the
//        lane is the CARRIER; equal: a duplicate, done; another key: next slot.  A region has more slots than rows, so a
//        probe always meets an empty slot.  Which of two equal rows wins does not matter: they would add the same.
//     3. a carrier reads off[o], off[o + 1] and tallies the whole records of its value: sample_records.h (a lane up to 16
//        records, the wave above that, the dictionary's keys in LDS while 8 C <= 32 KiB).
//     4. carriers[q] and the work counters: one atomic per wave and distinct query / per wave and pass, the counters 256
//        bytes apart.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "sample_records.h"

namespace rsb {

namespace {

constexpr unsigned long long TALLY_EMPTY = ~0ull;

__global__ void __launch_bounds__(256)
sample_region_rows_kernel(const uint32_t *__restrict__ shard, const uint64_t *__restrict__ first, size_t Q, uint64_t cap, uint32_t S,
                          unsigned long long *__restrict__ rows_of) {
    const uint64_t total = first[Q];
    if (total > cap) return;  // (the rows were not made: launch_interval_fill)
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t sh = t < total ? shard[t] : ~0u;
    // the rows of a wave are consecutive rows of the batch: a few shards at most, one add per shard
    uint64_t left = __builtin_amdgcn_ballot_w64(sh < S);
    while (left) {
        const int j = __builtin_ctzll(left);
        const uint32_t s0 = (uint32_t)__shfl((int)sh, j, 64);
        const uint64_t same = __builtin_amdgcn_ballot_w64(sh == s0);
        if (lane == (uint32_t)j) atomicAdd(&rows_of[s0], (unsigned long long)__builtin_popcountll(same));
        left &= ~same;
    }
}

// A shard's region: a power of two of slots strictly above its rows, and at least twice its rows unless `tight`; under
// 4 x rows + 1 either way, so 4 x (all rows) + S slots hold every region.
__global__ void sample_regions_kernel(const unsigned long long *__restrict__ rows_of, uint32_t S, uint32_t tight, uint64_t *__restrict__ region) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    uint64_t at = 0;
    for (uint32_t p = 0; p < S; ++p) {
        const uint64_t r = rows_of[p];
        uint64_t slots = 1;
        while (slots <= r || (!tight && slots < 2ull * r)) slots <<= 1;
        region[2u * p] = at;
        region[2u * p + 1u] = slots - 1ull;
        at += slots;
    }
}

// status8 = {rows, rows on a head ordinal, carriers, records, records with an unknown code, LF steps, rows not located, 0}
__global__ void sample_status_kernel(const uint64_t *__restrict__ first, size_t Q, const unsigned long long *__restrict__ work,
                                     const unsigned long long *__restrict__ locate_work2, uint64_t *__restrict__ status8) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    status8[0] = first[Q];
    status8[1] = work[TALLY_WORK_HEADS * TALLY_WORK_STRIDE];
    status8[2] = work[TALLY_WORK_CARRIERS * TALLY_WORK_STRIDE];
    status8[3] = work[TALLY_WORK_RECORDS * TALLY_WORK_STRIDE];
    status8[4] = work[TALLY_WORK_UNKNOWN * TALLY_WORK_STRIDE];
    status8[5] = locate_work2 ? locate_work2[1] : 0ull;
    status8[6] = work[TALLY_WORK_LOST * TALLY_WORK_STRIDE];
    status8[7] = 0ull;
}

template <bool KEYS_IN_LDS>
__global__ void __launch_bounds__(256)
sample_tally_kernel(const sample_tally a) {
    extern __shared__ uint64_t lds_keys[];
    const tally_dict d = tally_dict_of<KEYS_IN_LDS>(a.keys, a.C, lds_keys);
    const tally_cells cells = {a.strings, a.copies, a.size_of_sample, a.has_other};
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t R = a.size_of_sample + (a.has_other ? 2u : 0u);
    bool head = false, carrier = false, lost = false;
    uint64_t q = 0, o = 0;
    meta_view mv = {nullptr, nullptr, 0, nullptr};
    const uint64_t total = a.first[a.Q];  // (wave-uniform; above a.total the rows were not made and nothing is tallied)
    if (total <= a.total && t < total) {
        const uint32_t sh = a.shard[t];
        o = a.ordinal[t];
        lost = o == ~0ull;  // (launch_locate: the walk did not end)
        if (!lost && sh < a.S) {
            mv = a.meta[sh];
            head = mv.off && mv.heads && o < mv.num_strings && o < (1ull << 40) && ((mv.heads[o >> 5] >> (o & 31u)) & 1u);
        }
        if (head) {
            // the query: first[q] <= t < first[q + 1] (interval_rows.hip's fill)
            size_t lo = 0, hi = a.Q;
            while (hi - lo > 1) {
                const size_t mid = lo + (hi - lo) / 2;
                if (a.first[mid] <= t) lo = mid;
                else hi = mid;
            }
            q = lo;
            const unsigned long long key = ((unsigned long long)q << 40) | o;  // q < 2^24, o < 2^40: never all ones (o < num_strings < 2^40)
            unsigned long long *tab = a.set + a.region[2u * sh];
            const uint64_t mask = a.region[2u * sh + 1u];
            uint64_t h = key * 0x9E3779B97F4A7C15ull;
            uint64_t slot = (h ^ (h >> 29)) & mask;
            for (;;) {
                const unsigned long long old = atomicCAS(&tab[slot], TALLY_EMPTY, key);
                if (old == TALLY_EMPTY) {
                    carrier = true;
                    break;
                }
                if (old == key) break;
                slot = (slot + 1ull) & mask;
            }
        }
    }
    // ---- the carriers' values
    uint64_t nrec = 0;
    const uint8_t *val = nullptr;
    if (carrier) {
        const uint64_t b0 = mv.off[o], b1 = mv.off[o + 1];
        nrec = (b1 - b0) / R;  // (the tail that is no whole record is dropped)
        val = mv.bytes + b0;
    }
    const uint32_t unknown = tally_values(cells, d, a.C, lane, nrec, val, q);
    // ---- carriers[q]: one add per wave and distinct query
    const uint64_t carriers_in_wave = wave_count_by_query(a.carriers, carrier, q, lane);
    // ---- the counters, 256 bytes apart
    const uint64_t heads = __builtin_amdgcn_ballot_w64(head), losts = __builtin_amdgcn_ballot_w64(lost);
    if (lane == 0u) {
        if (heads) atomicAdd(&a.work[TALLY_WORK_HEADS * TALLY_WORK_STRIDE], (unsigned long long)__builtin_popcountll(heads));
        if (carriers_in_wave) atomicAdd(&a.work[TALLY_WORK_CARRIERS * TALLY_WORK_STRIDE], (unsigned long long)carriers_in_wave);
        if (losts) atomicAdd(&a.work[TALLY_WORK_LOST * TALLY_WORK_STRIDE], (unsigned long long)__builtin_popcountll(losts));
    }
    // (records: every whole record of every carrier, known code or not)
    uint64_t mine = carrier ? nrec : 0ull;
    for (int s = 32; s > 0; s >>= 1) mine += __shfl_xor(mine, s, 64);
    if (lane == 0u && mine) atomicAdd(&a.work[TALLY_WORK_RECORDS * TALLY_WORK_STRIDE], (unsigned long long)mine);
    wave_count(&a.work[TALLY_WORK_UNKNOWN * TALLY_WORK_STRIDE], unknown, lane);
}

__global__ void __launch_bounds__(256)
meta_heads_kernel(const uint64_t *__restrict__ ordinal, const uint64_t *__restrict__ copies, size_t n, uint32_t *__restrict__ heads,
                  uint64_t num_strings) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t c = copies[i], o = ordinal[i];
    if (c == 0ull || o >= num_strings) return;
    atomicOr(&heads[o >> 5], 1u << (o & 31u));
}

}  // namespace

hipError_t launch_sample_regions(const void *d_shard, const void *d_first, size_t Q, uint64_t cap, uint32_t S, bool tight, void *d_rows_of,
                                 void *d_region, hipStream_t stream) {
    if (cap != 0) {
        hipLaunchKernelGGL(sample_region_rows_kernel, dim3((unsigned)((cap + 255) / 256)), dim3(256), 0, stream, (const uint32_t *)d_shard,
                           (const uint64_t *)d_first, Q, cap, S, (unsigned long long *)d_rows_of);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(sample_regions_kernel, dim3(1), dim3(64), 0, stream, (const unsigned long long *)d_rows_of, S, tight ? 1u : 0u,
                       (uint64_t *)d_region);
    return hipGetLastError();
}

hipError_t launch_sample_status(const void *d_first, size_t Q, const void *d_work, const void *d_locate_work2, void *d_status8, hipStream_t stream) {
    hipLaunchKernelGGL(sample_status_kernel, dim3(1), dim3(64), 0, stream, (const uint64_t *)d_first, Q, (const unsigned long long *)d_work,
                       (const unsigned long long *)d_locate_work2, (uint64_t *)d_status8);
    return hipGetLastError();
}

hipError_t launch_sample_tally(const sample_tally &a, hipStream_t stream) {
    if (a.total == 0) return hipSuccess;
    sample_tally b = a;
    b.keys_in_lds = (size_t)a.C * 8 <= TALLY_LDS_BYTES ? 1u : 0u;
    const dim3 grid((unsigned)((a.total + 255) / 256));
    if (b.keys_in_lds) hipLaunchKernelGGL(sample_tally_kernel<true>, grid, dim3(256), (size_t)a.C * 8, stream, b);
    else hipLaunchKernelGGL(sample_tally_kernel<false>, grid, dim3(256), 0, stream, b);
    return hipGetLastError();
}

hipError_t launch_meta_heads(const void *d_ordinal, const void *d_copies, size_t n, void *d_heads, uint64_t num_strings, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(meta_heads_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, (const uint64_t *)d_ordinal,
                       (const uint64_t *)d_copies, n, (uint32_t *)d_heads, num_strings);
    return hipGetLastError();
}

}  // namespace rsb
