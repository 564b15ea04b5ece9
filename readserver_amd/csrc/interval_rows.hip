// interval_rows.hip -- a batch's intervals turned into its rows on the GPU, with a limit on the rows one query may bring.
//
// What rsbwt_set_query / rsbwt_set_query_var did on the host (sets.hip, set_query_rows: every [S][Q] interval copied
// back, every (shard, row) spelled into a vector by a scalar loop, regrouped by shard, padded and uploaded again):
//   * totals: one thread per query sums its widths over the S shards -- lane q reads pair [i][q], so a wave's 64 loads
//     are one kilobyte of consecutive pairs -- and applies the limit: a query over it keeps no row, its full total is
//     still reported;
//   * scan: first[] = exclusive scan of the kept totals (rocPRIM's device scan, u64);
//   * fill: one thread per OUTPUT ROW.  It finds its query by binary search in first[] and its shard by walking that
//     query's S widths, so an interval of 10^5 rows beside thousands of 3-row ones costs what an even batch costs, and
//     the stores of a wave are 64 consecutive u64 / u32.
// The rows in the caller's order (query-major, shard ascending, SA row ascending) are what rsbwt_set_interval_rows_dev
// hands out.  The walk kernels want a shard's rows together (extract_lines.hip: everything shard-specific sits in scalar
// registers), so the fill can also write them by CELL: cell (i, q) = shard i's rows of query q, the cells in shard-major
// order -- an exclusive scan of the kept widths [S][Q] in that order gives every cell's first row, and shard i's
// segment is cellpos[i * Q] .. cellpos[(i + 1) * Q]: no padding, whatever the spread over the shards.  dest[t] names the
// cell row of output row t for the copy back.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string.h>  // (rocPRIM's texture iterator calls memset without including it)

#include <rocprim/rocprim.hpp>

#include "kernels.h"
#include "line_format.h"

namespace rsb {

namespace {

// rows of shard i for a query: its interval, if it is one of rows of that shard (sets.hip, intervals_to_rows_host's rule): the empty
// (1, 0), the reference's (0, 2^64 - 1) corner and upper >= n all give 0
__device__ __forceinline__ uint64_t pair_width(const ulonglong2 p, uint64_t n) {
    return (p.x <= p.y && p.y < n) ? p.y - p.x + 1ull : 0ull;
}

// kept[Q + 1]: the totals the scan runs over (0 for a query over the limit; kept[Q] = 0, so that the exclusive scan's
// last element is the grand total); *over += queries over the limit
__global__ void __launch_bounds__(256)
ir_totals_kernel(const shard_view *__restrict__ views, uint32_t S, const ulonglong2 *__restrict__ pairs, size_t Q, uint64_t max_rows,
                 uint64_t *__restrict__ matches, uint64_t *__restrict__ kept, unsigned long long *__restrict__ over) {
    const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool is_over = false;
    if (q < Q) {
        uint64_t m = 0;
        for (uint32_t i = 0; i < S; ++i) m += pair_width(pairs[(size_t)i * Q + q], views[i].n);
        is_over = max_rows != 0ull && m > max_rows;
        matches[q] = m;
        kept[q] = is_over ? 0ull : m;
    } else if (q == Q) {
        kept[Q] = 0ull;
    }
    const uint64_t mask = __builtin_amdgcn_ballot_w64(is_over);
    if (mask != 0ull && (threadIdx.x & 63u) == 0u) atomicAdd(over, (unsigned long long)__builtin_popcountll(mask));
}

// cellw[S * Q + 1]: the kept widths in shard-major order (cellw[S * Q] = 0)
__global__ void __launch_bounds__(256)
ir_cells_kernel(const shard_view *__restrict__ views, uint32_t S, const ulonglong2 *__restrict__ pairs, size_t Q, uint64_t max_rows,
                const uint64_t *__restrict__ matches, uint64_t *__restrict__ cellw) {
    const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x, cells = (size_t)S * Q;
    if (c > cells) return;
    uint64_t w = 0;
    if (c < cells) {
        const size_t i = c / Q, q = c - i * Q;
        if (!(max_rows != 0ull && matches[q] > max_rows)) w = pair_width(pairs[c], views[i].n);
    }
    cellw[c] = w;
}

// Output row t.  Nothing is written when the rows do not fit `cap` (the caller sizes from first[Q] and calls again).
template <bool CELLS>
__global__ void __launch_bounds__(256)
ir_fill_kernel(const shard_view *__restrict__ views, uint32_t S, const ulonglong2 *__restrict__ pairs, size_t Q,
               const uint64_t *__restrict__ first, size_t cap, uint32_t *__restrict__ shard_of, uint64_t *__restrict__ rows,
               const uint64_t *__restrict__ cellpos, uint64_t *__restrict__ cell_rows, uint32_t *__restrict__ dest) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, total = first[Q];
    if (total > cap || t >= total) return;
    // the query: first[q] <= t < first[q + 1] (queries without rows share their neighbour's value and are never landed on)
    size_t lo = 0, hi = Q;
    while (hi - lo > 1) {
        const size_t mid = lo + ((hi - lo) >> 1);
        if (first[mid] <= t) lo = mid;
        else hi = mid;
    }
    const size_t q = lo;
    uint64_t r = t - first[q];
    for (uint32_t i = 0; i < S; ++i) {
        const ulonglong2 p = pairs[(size_t)i * Q + q];
        const uint64_t w = pair_width(p, views[i].n);
        if (r < w) {
            shard_of[t] = i;
            if (rows) rows[t] = p.x + r;
            if (CELLS) {
                const uint64_t c = cellpos[(size_t)i * Q + q] + r;
                cell_rows[c] = p.x + r;
                dest[t] = (uint32_t)c;
            }
            return;
        }
        r -= w;
    }
}

hipError_t scan_u64(void *d_temp, size_t temp_bytes, const uint64_t *d_in, uint64_t *d_out, size_t n, hipStream_t stream) {
    size_t need = temp_bytes;
    return rocprim::exclusive_scan(d_temp, need, d_in, d_out, (uint64_t)0, n, rocprim::plus<uint64_t>(), stream);
}

}  // namespace

size_t interval_rows_scan_bytes(size_t n) {
    size_t bytes = 0;
    if (rocprim::exclusive_scan(nullptr, bytes, (const uint64_t *)nullptr, (uint64_t *)nullptr, (uint64_t)0, n, rocprim::plus<uint64_t>(),
                                (hipStream_t) nullptr) != hipSuccess)
        return 0;
    return (bytes + 255) & ~(size_t)255;
}

hipError_t launch_interval_totals(const shard_view *d_views, uint32_t S, const void *d_pairs, size_t Q, uint64_t max_rows, void *d_matches,
                                  void *d_kept, void *d_first, void *d_over, void *d_temp, size_t temp_bytes, hipStream_t stream) {
    hipError_t e = hipMemsetAsync(d_over, 0, 8, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(ir_totals_kernel, dim3((unsigned)((Q + 1 + 255) / 256)), dim3(256), 0, stream, d_views, S, (const ulonglong2 *)d_pairs, Q,
                       max_rows, (uint64_t *)d_matches, (uint64_t *)d_kept, (unsigned long long *)d_over);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    return scan_u64(d_temp, temp_bytes, (const uint64_t *)d_kept, (uint64_t *)d_first, Q + 1, stream);
}

hipError_t launch_interval_cells(const shard_view *d_views, uint32_t S, const void *d_pairs, size_t Q, uint64_t max_rows, const void *d_matches,
                                 void *d_cellw, void *d_cellpos, void *d_temp, size_t temp_bytes, hipStream_t stream) {
    const size_t cells = (size_t)S * Q + 1;
    hipLaunchKernelGGL(ir_cells_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, stream, d_views, S, (const ulonglong2 *)d_pairs, Q,
                       max_rows, (const uint64_t *)d_matches, (uint64_t *)d_cellw);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return scan_u64(d_temp, temp_bytes, (const uint64_t *)d_cellw, (uint64_t *)d_cellpos, cells, stream);
}

hipError_t launch_interval_fill(const shard_view *d_views, uint32_t S, const void *d_pairs, size_t Q, const void *d_first, size_t cap,
                                void *d_shard, void *d_rows, const void *d_cellpos, void *d_cell_rows, void *d_dest, hipStream_t stream) {
    if (cap == 0 || Q == 0) return hipSuccess;
    const dim3 grid((unsigned)((cap + 255) / 256)), block(256);
    if (d_cellpos)
        hipLaunchKernelGGL(ir_fill_kernel<true>, grid, block, 0, stream, d_views, S, (const ulonglong2 *)d_pairs, Q, (const uint64_t *)d_first, cap,
                           (uint32_t *)d_shard, (uint64_t *)d_rows, (const uint64_t *)d_cellpos, (uint64_t *)d_cell_rows, (uint32_t *)d_dest);
    else
        hipLaunchKernelGGL(ir_fill_kernel<false>, grid, block, 0, stream, d_views, S, (const ulonglong2 *)d_pairs, Q, (const uint64_t *)d_first, cap,
                           (uint32_t *)d_shard, (uint64_t *)d_rows, (const uint64_t *)nullptr, (uint64_t *)nullptr, (uint32_t *)nullptr);
    return hipGetLastError();
}

}  // namespace rsb
