// match_lanes.h -- what the one-lane-per-item kernels that walk a query backwards share (match_stats.hip, overlaps.hip):
// the symbol ranks, Occ off a staged window line, the query of a position of a batch, and a wave's sum.
#ifndef RSBWT_MATCH_LANES_H
#define RSBWT_MATCH_LANES_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "line_format.h"
#include "rank_device.h"
#include "wave_lines.h"

namespace rsb {

__device__ __forceinline__ uint32_t ms_rank(uint32_t ch) {  // A..T -> 1..4, anything else 0
    return ch == 'A' ? 1u : ch == 'C' ? 2u : ch == 'G' ? 3u : ch == 'T' ? 4u : 0u;
}

// Occ of symbol b among the first o symbols (1 <= o <= span) of a staged window line's own pieces plus what the header
// counts before the window (gt_narrow.hip, gt_staged_occ)
__device__ __forceinline__ uint64_t ms_staged_occ(const staged_line &L, const line_head &h, uint32_t o, uint32_t b, const sym_tab &tab) {
    const uint32_t cq = (o > h.s1 ? 1u : 0u) + (o > h.s2 ? 1u : 0u) + (o > h.s3 ? 1u : 0u);
    const uint32_t start = cq == 0u ? 0u : cq == 1u ? h.s1 : cq == 2u ? h.s2 : h.s3;
    uint64_t d = read_count(L, b);
    if (cq >= 2u) d += read_half(L, b);
    if (cq & 1u) d += matched24(L, HDR_DWORDS + 6u * (cq & 2u), tab);
    uint32_t r6[6];
    load24(L, HDR_DWORDS + 6u * cq, r6);
    return d + rank24(r6, tab, b, o - start);
}

// the query of position t: off[q] <= t < off[q + 1] (t < off[Q]; queries of no symbols are stepped over)
__device__ __forceinline__ size_t ms_query_of(const uint64_t *__restrict__ off, size_t Q, uint64_t t) {
    size_t lo = 0, hi = Q - 1;
    while (lo < hi) {
        const size_t mid = lo + ((hi - lo) >> 1);
        if (off[mid + 1] > t) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

__device__ __forceinline__ unsigned long long ms_wave_sum(unsigned long long v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

}  // namespace rsb
#endif
