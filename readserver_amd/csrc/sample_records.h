// sample_records.h -- the record parse of the sample tallies, shared by sample_counts.hip (rsbwt_set_sample_counts: a carrier
// is a located row) and site_counts.hip (rsbwt_set_site_sample_counts: a carrier is an aligned read that was kept).  Device code.
//
// A carrier's value is cut into records of R = size_of_sample + (has_other ? 2 : 0) bytes; every whole record adds 1 to
// strings[q][col] and c to copies[q][col], col = the column of its code (C: a code the dictionary lacks).  Up to
// TALLY_LANE_RECORDS = 16 records the carrier's own lane parses; a longer value the whole wave takes, one holder after the
// other (ballot + broadcast, lanes striding over the records): read_meta.hip's division of labour.  16: a lane then runs at
// most 16 binary searches and 32 adds while its 63 neighbours run theirs, where a wave pass over so few records would leave
// three quarters of the lanes idle; above it a lone lane would hold its wave for one search per record (2,000 for a read of
// a common sequence) with 63 lanes idle, and the wave does the same in records / 64 passes.
// code -> column: binary search over the dictionary's u64 keys (sample_codes.h), in LDS while 8 C <= TALLY_LDS_BYTES (five
// blocks of 256 threads still share a CU's 160 KiB), else over the copy in HBM.
// The adds are agent-scope atomicAdd on the u32 / i64 cells and are not combined inside the wave: lanes differ in query and
// column, and integer sums do not depend on the order -- the matrices are bit-identical from run to run.
#ifndef RSBWT_SAMPLE_RECORDS_H
#define RSBWT_SAMPLE_RECORDS_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rsb {

constexpr uint32_t TALLY_LANE_RECORDS = 16;

struct tally_dict {
    const uint64_t *keys;  // LDS or HBM
    uint32_t C;
};

// the matrices of a launch and the shape of a record
struct tally_cells {
    uint32_t *strings;  // [Q][C + 1]; may be nullptr
    long long *copies;  // [Q][C + 1]; may be nullptr
    uint32_t size_of_sample, has_other;
};

// the dictionary of a block: its keys copied to lds_keys by the whole block (KEYS_IN_LDS), else read where they are
template <bool KEYS_IN_LDS>
__device__ __forceinline__ tally_dict tally_dict_of(const uint64_t *__restrict__ keys, uint32_t C, uint64_t *lds_keys) {
    tally_dict d;
    d.C = C;
    if (KEYS_IN_LDS) {
        for (uint32_t i = threadIdx.x; i < C; i += blockDim.x) lds_keys[i] = keys[i];
        __syncthreads();
        d.keys = lds_keys;
    } else {
        d.keys = keys;
    }
    return d;
}

__device__ __forceinline__ uint32_t tally_column(const tally_dict &d, uint64_t key) {
    uint32_t lo = 0, hi = d.C;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (d.keys[mid] < key) lo = mid + 1u;
        else hi = mid;
    }
    return lo < d.C && d.keys[lo] == key ? lo : d.C;
}

// the record at p: one add per matrix; returns 1 when its code is not in the dictionary
__device__ __forceinline__ uint32_t tally_record(const tally_cells &a, const tally_dict &d, const uint8_t *p, uint64_t cell0) {
    uint64_t key = 0;
    for (uint32_t b = 0; b < a.size_of_sample; ++b) key = (key << 8) | p[b];
    const uint32_t col = tally_column(d, key);
    if (a.strings) atomicAdd(&a.strings[cell0 + col], 1u);
    if (a.copies) {
        const long long c = a.has_other ? (long long)(int)(signed char)p[a.size_of_sample] - 33ll : 1ll;
        atomicAdd(reinterpret_cast<unsigned long long *>(a.copies) + cell0 + col, (unsigned long long)c);
    }
    return col == d.C ? 1u : 0u;
}

// Every lane of the wave is here (nothing above returns): a lane that holds a carrier brings the nrec whole records at val
// for row q of the matrices, the others nrec = 0.  Returns the records with an unknown code this lane added.
__device__ __forceinline__ uint32_t tally_values(const tally_cells &a, const tally_dict &d, uint32_t C, uint32_t lane, uint64_t nrec,
                                                 const uint8_t *val, uint64_t q) {
    const uint32_t R = a.size_of_sample + (a.has_other ? 2u : 0u);
    const uint64_t width = (uint64_t)C + 1ull;
    uint32_t unknown = 0;
    if (nrec != 0ull && nrec <= TALLY_LANE_RECORDS)
        for (uint32_t i = 0; i < (uint32_t)nrec; ++i) unknown += tally_record(a, d, val + (size_t)i * R, q * width);
    uint64_t longs = __builtin_amdgcn_ballot_w64(nrec > TALLY_LANE_RECORDS);
    while (longs) {
        const int j = __builtin_ctzll(longs);
        longs &= longs - 1ull;
        const uint64_t wn = __shfl(nrec, j, 64), wq = __shfl(q, j, 64);
        const uint8_t *wv = reinterpret_cast<const uint8_t *>(__shfl((uint64_t)(uintptr_t)val, j, 64));
        for (uint64_t i = lane; i < wn; i += 64u) unknown += tally_record(a, d, wv + i * R, wq * width);
    }
    return unknown;
}

// The same division of labour for a caller that needs a SUM per carrier and no matrix (sample_walk.hip: hit or miss against
// a mask of columns): value(p) is the number a record at p adds.  Every lane of the wave is here; a lane that holds a carrier
// brings the nrec whole records of R bytes at val.  A short value's sum comes back in its own lane; a long value's is summed
// over the wave and comes back in the holder's lane.
template <class F>
__device__ __forceinline__ long long record_sums(uint32_t R, uint32_t lane, uint64_t nrec, const uint8_t *val, F &&value) {
    long long mine = 0;
    if (nrec != 0ull && nrec <= TALLY_LANE_RECORDS)
        for (uint32_t i = 0; i < (uint32_t)nrec; ++i) mine += value(val + (size_t)i * R);
    uint64_t longs = __builtin_amdgcn_ballot_w64(nrec > TALLY_LANE_RECORDS);
    while (longs) {
        const int j = __builtin_ctzll(longs);
        longs &= longs - 1ull;
        const uint64_t wn = __shfl(nrec, j, 64);
        const uint8_t *wv = reinterpret_cast<const uint8_t *>(__shfl((uint64_t)(uintptr_t)val, j, 64));
        long long part = 0;
        for (uint64_t i = lane; i < wn; i += 64u) part += value(wv + i * R);
        for (int s = 32; s > 0; s >>= 1) part += __shfl_xor(part, s, 64);
        if (lane == (uint32_t)j) mine = part;
    }
    return mine;
}

// counter += the sum over the wave of a small per-lane number: one atomic
__device__ __forceinline__ void wave_count(unsigned long long *counter, uint32_t mine, uint32_t lane) {
    uint32_t v = mine;
    for (int s = 32; s > 0; s >>= 1) v += (uint32_t)__shfl_xor((int)v, s, 64);
    if (lane == 0u && v) atomicAdd(counter, (unsigned long long)v);
}

// per[q] += the lanes of the wave with `mine` set, one add per wave and distinct q (per may be nullptr); returns their number
__device__ __forceinline__ uint32_t wave_count_by_query(unsigned long long *per, bool mine, uint64_t q, uint32_t lane) {
    uint64_t left = __builtin_amdgcn_ballot_w64(mine);
    const uint32_t all = (uint32_t)__builtin_popcountll(left);
    while (left) {
        const int j = __builtin_ctzll(left);
        const uint64_t q0 = __shfl(q, j, 64);
        const uint64_t same = __builtin_amdgcn_ballot_w64(mine && q == q0);
        if (per && lane == (uint32_t)j) atomicAdd(&per[q0], (unsigned long long)__builtin_popcountll(same));
        left &= ~same;
    }
    return all;
}

}  // namespace rsb
#endif
