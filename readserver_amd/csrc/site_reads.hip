// site_reads.hip -- rsbwt_set_site_reads / rsbwt_set_site_read_counts (include/rsbwt.h): the reads align_gt_read keeps for
// each site request, laid out for the caller on the GPU (gfx950).  Stages 1 to 4 are site_counts.hip's (its launch_site_rows
// with no sample table takes every kept row, not the head copies alone); what is here is what that file's tally is replaced
// by: the reads' string classes, and the answer's layout.
//
//   CLASSES  rsbwt_set_gt_aligned_reads reports a string once per (request, shard), under the smallest read_row it has.  The
//     distinct reads of a batch lie sorted by (shard, read_row) (launch_site_reads).  Why comparing a read with the one before
//     it is exact:
//       (a) the rows of the suffixes `READ$` of equal reads are adjacent in a shard's BWT (nothing sorts between two equal
//           strings), so the copies of a string stand on consecutive read_rows;
//       (b) every copy of a string lies in the same leg intervals at the same offsets, with the same span and the same needed
//           length (site_counts.hip's header), so when one copy is a candidate of a request every copy is, and the distinct
//           reads of the batch hold all copies of every string they hold;
//     hence the copies of a string are a run of neighbours in the sorted distinct reads, and a read repeats a string iff its
//     shard, its length and its bytes equal its predecessor's.  16 lanes compare a read with its predecessor 16 bytes a lane
//     and step, through raddr / rlen (one may lie in the narrow buffer and the other in the wide one; both start 16-byte
//     aligned).  flag[r] = 1 where a class begins; its exclusive scan numbers the classes.
//   LAYOUT   the items sorted by (request << 31 | read number): read numbers ascend with (shard, read_row), so this is the
//     answer's order -- request, shard, read_row.  An item is reported iff its verdict is one of the three KEEPs and the item
//     before it is not a kept item of the same request and class (equal strings have equal verdicts).  The exclusive scan of
//     that flag is the item's place in the answer; first[q * S + p] is the scan's value at the first item of (q, p) or above.
//   GATHER   16 lanes per reported read copy it from where it lies into its slot at read_stride, 16 bytes a lane and step
//     when the stride is a multiple of 16 (a byte a lane otherwise), and fill the slot's rest with zeros: every byte of the
//     output is written once.  A read longer than the stride leaves a zeroed slot and the length UINT32_MAX.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>  // (rocPRIM's texture iterator calls memset without including it)

#include <algorithm>

#include <rocprim/rocprim.hpp>

#include "../../include/rsbwt.h"
#include "kernels.h"
#include "sample_records.h"

namespace rsb {

namespace {

constexpr uint32_t RID_BITS = 31;  // (launch_site_reads takes fewer than 2^31 items: a read number fits)

__device__ __forceinline__ unsigned long long *site_counter(unsigned long long *work, int which) { return work + (size_t)which * TALLY_WORK_STRIDE; }

// the first `valid` (1..16) bytes of two 16-byte pieces differ
__device__ __forceinline__ bool differ16(const uint4 x, const uint4 y, uint32_t valid) {
    const uint32_t a[4] = {x.x, x.y, x.z, x.w}, b[4] = {y.x, y.y, y.z, y.w};
    bool d = false;
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
        const uint32_t have = valid > 4u * j ? valid - 4u * j : 0u;
        const uint32_t mask = have >= 4u ? 0xFFFFFFFFu : (1u << (8u * have)) - 1u;
        d = d || ((a[j] ^ b[j]) & mask) != 0u;
    }
    return d;
}

// the first `valid` (0..16) bytes kept, the rest zero
__device__ __forceinline__ uint4 keep16(const uint4 x, uint32_t valid) {
    uint32_t a[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
        const uint32_t have = valid > 4u * j ? valid - 4u * j : 0u;
        a[j] &= have >= 4u ? 0xFFFFFFFFu : (1u << (8u * have)) - 1u;
    }
    return make_uint4(a[0], a[1], a[2], a[3]);
}

// flag[r] = 1 where read r begins a string class, flag[R] = 0: 16 lanes per read
__global__ void __launch_bounds__(256)
site_class_kernel(const uint64_t *__restrict__ raddr, const uint32_t *__restrict__ rlen, const uint64_t *__restrict__ seg, uint32_t S, size_t R,
                  uint64_t *__restrict__ flag) {
    const size_t r = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    const uint32_t lane = threadIdx.x & 63u, sub = threadIdx.x & 15u;
    const bool have = r < R;
    const uint32_t len = have ? rlen[r] : 0u;
    bool compare = have && r > 0 && len != 0xFFFFFFFFu && rlen[r - 1] == len;
    if (compare) {  // the first read of a shard has no predecessor there: seg[] ascends, look for r in it
        uint32_t lo = 0, hi = S + 1u;
        while (lo < hi) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (seg[mid] < (uint64_t)r) lo = mid + 1u;
            else hi = mid;
        }
        compare = !(lo <= S && seg[lo] == (uint64_t)r);
    }
#ifdef RSB_SITE_MUTANT_NO_CLASS_COMPARE
    compare = false;  // (the mutant: every read a class of its own)
#endif
    bool differ = false;
    if (compare) {
        const uint8_t *a = (const uint8_t *)(uintptr_t)raddr[r], *b = (const uint8_t *)(uintptr_t)raddr[r - 1];
        for (uint32_t k = 16u * sub; k < len && !differ; k += 256u) {
            const uint4 x = *reinterpret_cast<const uint4 *>(a + k), y = *reinterpret_cast<const uint4 *>(b + k);
            differ = differ16(x, y, len - k < 16u ? len - k : 16u);
        }
    }
    const uint64_t any = __builtin_amdgcn_ballot_w64(differ);
    const bool group_differs = ((any >> (lane & ~15u)) & 0xFFFFull) != 0ull;
    if (have && sub == 0u) flag[r] = !compare || group_differs ? 1ull : 0ull;
    if (blockIdx.x == 0 && threadIdx.x == 0) flag[R] = 0ull;
}

__global__ void __launch_bounds__(256)
site_layout_keys_kernel(const site_item *__restrict__ items, size_t n, uint64_t *__restrict__ key, uint32_t *__restrict__ idx) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    key[i] = ((uint64_t)items[i].q << RID_BITS) | items[i].rid;
    idx[i] = (uint32_t)i;
}

__device__ __forceinline__ bool site_kept(uint8_t v) { return v == RSBWT_GT_KEEP_PLAIN || v == RSBWT_GT_KEEP_RIGHT || v == RSBWT_GT_KEEP_LEFT; }

// over the sorted items: keep[j] = 1 for an item that is reported, keep[n] = 0
__global__ void __launch_bounds__(256)
site_keep_kernel(const uint64_t *__restrict__ key, const uint32_t *__restrict__ idx, size_t n, const uint8_t *__restrict__ verdict,
                 const uint64_t *__restrict__ cflag, const uint64_t *__restrict__ cfirst, uint64_t *__restrict__ keep, unsigned long long *__restrict__ work) {
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool pass = false;
    if (j < n) {
        const uint64_t kj = key[j];
        pass = site_kept(verdict[idx[j]]);
        bool repeat = false;
        if (pass && j > 0) {
            const uint64_t kp = key[j - 1];
            const uint64_t rj = kj & ((1ull << RID_BITS) - 1ull), rp = kp & ((1ull << RID_BITS) - 1ull);
            repeat = (kj >> RID_BITS) == (kp >> RID_BITS) && cfirst[rj] + cflag[rj] == cfirst[rp] + cflag[rp] && site_kept(verdict[idx[j - 1]]);
        }
        keep[j] = pass && !repeat ? 1ull : 0ull;
    } else if (j == n) {
        keep[j] = 0ull;
    }
    const uint64_t passed = __builtin_amdgcn_ballot_w64(pass);
    if ((threadIdx.x & 63u) == 0u && passed) atomicAdd(site_counter(work, SITE_WORK_KEPT), (unsigned long long)__builtin_popcountll(passed));
}

// the reported items' read numbers and rows at their places, and first[] of the group's (request, shard) cells
__global__ void __launch_bounds__(256)
site_emit_kernel(const uint64_t *__restrict__ key, size_t n, const uint64_t *__restrict__ keep, const uint64_t *__restrict__ place,
                 const uint64_t *__restrict__ rows, const uint64_t *__restrict__ seg, uint32_t S, size_t Q, uint32_t *__restrict__ out_rid,
                 uint64_t *__restrict__ out_row, uint64_t *__restrict__ first) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n && keep[t]) {
        const uint32_t rid = (uint32_t)(key[t] & ((1ull << RID_BITS) - 1ull));
        out_rid[place[t]] = rid;
        out_row[place[t]] = rows[rid];
    }
    const size_t cells = Q * (size_t)S;
    if (t <= cells) {
        size_t lo = n;
        if (t < cells) {  // the first item of request q on a read of shard p or a later one
            const uint64_t want = ((uint64_t)(t / S) << RID_BITS) | seg[t % S];
            size_t hi = n;
            lo = 0;
            while (lo < hi) {
                const size_t mid = lo + ((hi - lo) >> 1);
                if (key[mid] < want) lo = mid + 1;
                else hi = mid;
            }
        }
        first[t] = place[lo];
    }
}

template <bool BY16>
__global__ void __launch_bounds__(256)
site_gather_kernel(const uint32_t *__restrict__ out_rid, size_t n, const uint64_t *__restrict__ raddr, const uint32_t *__restrict__ rlen,
                   uint8_t *__restrict__ out, uint32_t stride, uint32_t *__restrict__ out_len) {
    const size_t o = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    const uint32_t sub = threadIdx.x & 15u;
    if (o >= n) return;
    const uint32_t rid = out_rid[o];
    const uint32_t len = rlen[rid];
    const bool fits = len <= stride;
    const uint32_t copy = fits ? len : 0u;
    const uint8_t *src = (const uint8_t *)(uintptr_t)raddr[rid];
    uint8_t *dst = out + o * (size_t)stride;
    if (sub == 0u) out_len[o] = fits ? len : 0xFFFFFFFFu;
    if (BY16) {
        for (uint32_t k = 16u * sub; k < stride; k += 256u) {
            uint4 x = make_uint4(0, 0, 0, 0);
            if (k < copy) x = keep16(*reinterpret_cast<const uint4 *>(src + k), copy - k < 16u ? copy - k : 16u);
            *reinterpret_cast<uint4 *>(dst + k) = x;
        }
    } else {
        for (uint32_t k = sub; k < stride; k += 16u) dst[k] = k < copy ? src[k] : (uint8_t)0;
    }
}

inline dim3 grid_of(size_t n) { return dim3((unsigned)((n + 255) / 256)); }
inline size_t al256(size_t b) { return (b + 255) & ~(size_t)255; }

size_t layout_sort_bytes(size_t n) {
    size_t bytes = 0;
    if (rocprim::radix_sort_pairs(nullptr, bytes, (const uint64_t *)nullptr, (uint64_t *)nullptr, (const uint32_t *)nullptr, (uint32_t *)nullptr, n, 0u,
                                  64u, (hipStream_t) nullptr) != hipSuccess)
        return 0;
    return al256(bytes);
}

}  // namespace

// d_tmp of launch_site_layout: the sorted keys and indices, the keep flags and their scan, then the sort's and the scan's own
size_t site_layout_tmp_bytes(size_t n) {
    const size_t own = std::max(layout_sort_bytes(n), meta_scan_bytes(n + 1));
    return al256(n * 8) + al256(n * 4) + 2 * al256((n + 1) * 8) + own + 256;
}

hipError_t launch_site_classes(const void *d_raddr, const void *d_rlen, const void *d_seg, uint32_t S, size_t R, void *d_cflag, void *d_cfirst,
                               void *d_tmp, size_t tmp_bytes, hipStream_t stream) {
    hipLaunchKernelGGL(site_class_kernel, grid_of(std::max<size_t>(R, 1) * 16), dim3(256), 0, stream, (const uint64_t *)d_raddr, (const uint32_t *)d_rlen,
                       (const uint64_t *)d_seg, S, R, (uint64_t *)d_cflag);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_meta_scan(d_tmp, tmp_bytes, d_cflag, d_cfirst, R + 1, stream);
}

hipError_t launch_site_layout(const void *d_items, size_t n, size_t Q, uint32_t S, const void *d_verdict, const void *d_cflag, const void *d_cfirst,
                              const void *d_rows, const void *d_seg, void *d_key, void *d_idx, void *d_tmp, size_t tmp_bytes, void *d_out_rid,
                              void *d_out_row, void *d_first, void *d_nout, unsigned long long *d_work, hipStream_t stream) {
    if (n == 0 || n >= (1ull << RID_BITS) || Q == 0 || Q > (1ull << 24)) return hipErrorInvalidValue;
    uint8_t *p = (uint8_t *)d_tmp;
    uint64_t *key = (uint64_t *)p;
    uint32_t *idx = (uint32_t *)(p + al256(n * 8));
    uint64_t *keep = (uint64_t *)(p + al256(n * 8) + al256(n * 4)), *place = keep + al256((n + 1) * 8) / 8;
    uint8_t *own = (uint8_t *)(place + al256((n + 1) * 8) / 8);
    if (own > p + tmp_bytes) return hipErrorInvalidValue;
    size_t own_bytes = (size_t)(p + tmp_bytes - own);
    hipLaunchKernelGGL(site_layout_keys_kernel, grid_of(n), dim3(256), 0, stream, (const site_item *)d_items, n, (uint64_t *)d_key, (uint32_t *)d_idx);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    uint32_t q_bits = 1;
    while ((1ull << q_bits) < (uint64_t)Q) ++q_bits;
    e = rocprim::radix_sort_pairs(own, own_bytes, (const uint64_t *)d_key, key, (const uint32_t *)d_idx, idx, n, 0u, RID_BITS + q_bits, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(site_keep_kernel, grid_of(n + 1), dim3(256), 0, stream, key, idx, n, (const uint8_t *)d_verdict, (const uint64_t *)d_cflag,
                       (const uint64_t *)d_cfirst, keep, d_work);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = launch_meta_scan(own, (size_t)(p + tmp_bytes - own), keep, place, n + 1, stream)) != hipSuccess) return e;
    hipLaunchKernelGGL(site_emit_kernel, grid_of(std::max<size_t>(n, Q * (size_t)S + 1)), dim3(256), 0, stream, key, n, keep, place, (const uint64_t *)d_rows,
                       (const uint64_t *)d_seg, S, Q, (uint32_t *)d_out_rid, (uint64_t *)d_out_row, (uint64_t *)d_first);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    return hipMemcpyAsync(d_nout, place + n, 8, hipMemcpyDeviceToDevice, stream);
}

hipError_t launch_site_gather(const void *d_out_rid, size_t n, const void *d_raddr, const void *d_rlen, void *d_out, uint32_t stride, void *d_out_len,
                              hipStream_t stream) {
    if (n == 0) return hipSuccess;
    // (the reads start 16-byte aligned wherever they lie; the slots do when the stride keeps them so)
    if (stride % 16u == 0u && ((uintptr_t)d_out & 15u) == 0u)
        hipLaunchKernelGGL(site_gather_kernel<true>, grid_of(n * 16), dim3(256), 0, stream, (const uint32_t *)d_out_rid, n, (const uint64_t *)d_raddr,
                           (const uint32_t *)d_rlen, (uint8_t *)d_out, stride, (uint32_t *)d_out_len);
    else
        hipLaunchKernelGGL(site_gather_kernel<false>, grid_of(n * 16), dim3(256), 0, stream, (const uint32_t *)d_out_rid, n, (const uint64_t *)d_raddr,
                           (const uint32_t *)d_rlen, (uint8_t *)d_out, stride, (uint32_t *)d_out_len);
    return hipGetLastError();
}

}  // namespace rsb
