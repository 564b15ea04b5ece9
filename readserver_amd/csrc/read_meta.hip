// read_meta.hip -- the per-read sample table: "which samples carry this read", gathered from HBM by read ordinal (gfx950).
//
// The reference keeps a read's samples in RocksDB under the read string (sdb->Get(read, &value),
// src/service/service.cpp:1292-1348).  Here the FM index is the hash: a whole-read search from the terminator rows
// (read_lookup.hip) gives the read's ordinal, and a shard's table is
//     off   u64[num_strings + 1]
//     bytes the values back to back: the value of ordinal o is bytes[off[o] .. off[o+1])
// raw bytes, whatever a record is.  A lookup is three launches and no atomics:
//   * SIZES: one lane per item: its length and where its bytes start in its shard's table;
//   * SCAN:  first[] = exclusive scan of the lengths (rocPRIM's device scan, as interval_rows.hip);
//   * COPY:  the bytes, unaligned at both ends.  A value of up to META_SHORT bytes is copied by its own lane -- in dwords
//     where source and destination share their residue mod 4 (byte head and tail), else byte by byte.  A longer one is
//     copied by the whole wave, one item after the other (ballot + broadcast: no list, no second launch): byte head up to
//     the destination's next 16-byte boundary, then 16-byte stores -- 1 KiB per wave instruction -- fed by 16-byte loads
//     where the source is as aligned, by four dword loads where it is dword aligned, else assembled from bytes; byte tail.
//
// META_SHORT = 64: typical values are a few records of 2-4 bytes, and one lane moves 64 bytes in at most 16 dword
// stores (64 byte stores at worst) while its 63 neighbours move theirs -- the wave loop would instead spend a whole
// wave pass (head, body, tail: three instructions with at most 4 of 64 lanes storing) on each such value, one after the
// other.  Above 64 bytes a lane alone would hold its wave for len / 4 stores or more (1,250 for a 5,000-byte value) with
// 63 lanes idle; the wave moves the same value in len / 1024 + 2 passes.
//
// The build (rsbwt_set_meta_build) runs on the same table from the other side: WINNERS takes atomicMax(index + 1) per
// ordinal (the pair given last wins: batch.Put overwrites, load_data_into_rocksdb.cpp:50), WINNER VALUES turns the winners
// of a chunk of pairs into lengths and source offsets, the scan gives off[], and the COPY kernel moves the value bytes
// from the uploaded chunk into the table.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string.h>  // (rocPRIM's texture iterator calls memset without including it)

#include <rocprim/rocprim.hpp>

#include "kernels.h"

namespace rsb {

namespace {

constexpr uint32_t META_SHORT = 64;

__global__ void __launch_bounds__(256)
meta_sizes_kernel(const meta_view *__restrict__ meta, uint32_t S, const uint32_t *__restrict__ shard, const uint64_t *__restrict__ ordinal,
                  const uint64_t *__restrict__ copies, size_t Q, size_t n, uint64_t *__restrict__ len, uint64_t *__restrict__ src) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n) return;
    if (i == n) {
        len[n] = 0ull;
        return;
    }
    uint32_t sh = 0;
    uint64_t o;
    bool ok = true;
    if (Q) {
        const size_t q = i / S;
        sh = (uint32_t)(i - q * S);
        const size_t at = (size_t)sh * Q + q;
        o = ordinal[at];
        ok = copies[at] != 0ull;
    } else {
        if (shard) sh = shard[i];
        o = ordinal[i];
    }
    uint64_t l = 0, at0 = META_NONE;
    if (ok && sh < S) {
        const meta_view mv = meta[sh];
        if (mv.off && o < mv.num_strings) {
            at0 = mv.off[o];
            l = mv.off[o + 1] - at0;
            if (l == 0ull) at0 = META_NONE;
        }
    }
    len[i] = l;
    src[i] = at0;
}

// one lane, l <= META_SHORT bytes
__device__ __forceinline__ void copy_lane(uint8_t *d, const uint8_t *s, uint32_t l) {
    if ((((uintptr_t)d ^ (uintptr_t)s) & 3u) == 0u) {
        while (l && ((uintptr_t)d & 3u)) {
            *d++ = *s++;
            --l;
        }
        for (; l >= 4u; l -= 4u, d += 4, s += 4) *reinterpret_cast<uint32_t *>(d) = *reinterpret_cast<const uint32_t *>(s);
    }
    for (; l; --l) *d++ = *s++;
}

// the whole wave, l > META_SHORT bytes; d, s, l are the same in every lane
__device__ __forceinline__ void copy_wave(uint8_t *d, const uint8_t *s, uint64_t l, uint32_t lane) {
    const uint32_t head = (uint32_t)((16u - ((uintptr_t)d & 15u)) & 15u);  // < 16 < l
    if (lane < head) d[lane] = s[lane];
    d += head;
    s += head;
    l -= head;
    const uint64_t nv = l >> 4;
    const uint32_t sa = (uint32_t)((uintptr_t)s & 15u);
    if (sa == 0u) {
        for (uint64_t v = lane; v < nv; v += 64u) reinterpret_cast<uint4 *>(d)[v] = reinterpret_cast<const uint4 *>(s)[v];
    } else if ((sa & 3u) == 0u) {
        for (uint64_t v = lane; v < nv; v += 64u) {
            const uint32_t *p = reinterpret_cast<const uint32_t *>(s + (v << 4));
            uint4 x;
            x.x = p[0];
            x.y = p[1];
            x.z = p[2];
            x.w = p[3];
            reinterpret_cast<uint4 *>(d)[v] = x;
        }
    } else {
        for (uint64_t v = lane; v < nv; v += 64u) {
            uint4 x;
            __builtin_memcpy(&x, s + (v << 4), 16);
            reinterpret_cast<uint4 *>(d)[v] = x;
        }
    }
    const uint32_t tail = (uint32_t)(l & 15u);
    if (lane < tail) d[(nv << 4) + lane] = s[(nv << 4) + lane];
}

__global__ void __launch_bounds__(256)
meta_copy_kernel(const meta_view *__restrict__ meta, uint32_t S, const uint32_t *__restrict__ shard, size_t Q, const uint8_t *__restrict__ base,
                 const uint64_t *__restrict__ src, const uint64_t *__restrict__ first, size_t n, uint8_t *__restrict__ dst, uint64_t cap) {
    if (first[n] > cap) return;  // (the caller sizes from first[n] and calls again)
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    uint64_t l = 0;
    const uint8_t *s = nullptr;
    uint8_t *d = nullptr;
    if (i < n) {
        const uint64_t so = src[i];
        if (so != META_NONE) {
            const uint64_t a = first[i];
            l = first[i + 1] - a;
            const uint8_t *b = base;
            if (!b) {
                const uint32_t sh = Q ? (uint32_t)(i % S) : (shard ? shard[i] : 0u);
                b = meta[sh].bytes;  // (sh < S: META_NONE otherwise)
            }
            s = b + so;
            d = dst + a;
        }
    }
    if (l != 0ull && l <= META_SHORT) copy_lane(d, s, (uint32_t)l);
    uint64_t longs = __builtin_amdgcn_ballot_w64(l > META_SHORT);
    while (longs) {
        const int j = __builtin_ctzll(longs);
        longs &= longs - 1ull;
        const uint64_t wl = __shfl(l, j, 64);
        const uint8_t *ws = reinterpret_cast<const uint8_t *>(__shfl((uint64_t)(uintptr_t)s, j, 64));
        uint8_t *wd = reinterpret_cast<uint8_t *>(__shfl((uint64_t)(uintptr_t)d, j, 64));
        copy_wave(wd, ws, wl, lane);
    }
}

__global__ void __launch_bounds__(256)
meta_winners_kernel(const uint64_t *__restrict__ ordinal, const uint64_t *__restrict__ copies, size_t n, uint64_t base,
                    unsigned long long *__restrict__ win, uint64_t num_strings) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t c = copies[i], o = ordinal[i];
    if (c == 0ull || o >= num_strings || c > num_strings - o) return;  // (never for an answer of the '$' count)
    for (uint64_t t = 0; t < c; ++t) atomicMax(&win[o + t], (unsigned long long)(base + i + 1ull));
}

__global__ void __launch_bounds__(256)
meta_winner_values_kernel(const uint64_t *__restrict__ win, uint64_t num_strings, const uint64_t *__restrict__ voff, uint64_t c0, uint64_t c1,
                          uint64_t *__restrict__ len, uint64_t *__restrict__ src, unsigned long long *__restrict__ given) {
    const uint64_t o = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool mine = false;
    if (o < num_strings) {
        const uint64_t w = win[o];  // 0: nobody; else pair w - 1
        mine = w > c0 && w <= c1;
        if (mine) {
            const uint64_t a = voff[w - 1ull - c0], b = voff[w - c0];
            if (len) len[o] = b - a;
            if (src) src[o] = b > a ? a - voff[0] : META_NONE;
        } else if (src) {
            src[o] = META_NONE;
        }
    }
    if (given) {
        const uint64_t m = __builtin_amdgcn_ballot_w64(mine);
        if (m != 0ull && (threadIdx.x & 63u) == 0u) atomicAdd(given, (unsigned long long)__builtin_popcountll(m));
    }
}

}  // namespace

size_t meta_scan_bytes(size_t n) {
    size_t bytes = 0;
    if (rocprim::exclusive_scan(nullptr, bytes, (const uint64_t *)nullptr, (uint64_t *)nullptr, (uint64_t)0, n, rocprim::plus<uint64_t>(),
                                (hipStream_t) nullptr) != hipSuccess)
        return 0;
    return (bytes + 255) & ~(size_t)255;
}

hipError_t launch_meta_scan(void *d_temp, size_t temp_bytes, const void *d_len, void *d_first, size_t n, hipStream_t stream) {
    size_t need = temp_bytes;
    return rocprim::exclusive_scan(d_temp, need, (const uint64_t *)d_len, (uint64_t *)d_first, (uint64_t)0, n, rocprim::plus<uint64_t>(), stream);
}

hipError_t launch_meta_sizes(const meta_view *d_meta, uint32_t S, const void *d_shard, const void *d_ordinal, const void *d_copies,
                             size_t Q, size_t n, void *d_len, void *d_src, hipStream_t stream) {
    hipLaunchKernelGGL(meta_sizes_kernel, dim3((unsigned)((n + 1 + 255) / 256)), dim3(256), 0, stream, d_meta, S, (const uint32_t *)d_shard,
                       (const uint64_t *)d_ordinal, (const uint64_t *)d_copies, Q, n, (uint64_t *)d_len, (uint64_t *)d_src);
    return hipGetLastError();
}

hipError_t launch_meta_copy(const meta_view *d_meta, uint32_t S, const void *d_shard, size_t Q, const void *d_base, const void *d_src,
                            const void *d_first, size_t n, void *d_dst, uint64_t cap, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(meta_copy_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, d_meta, S, (const uint32_t *)d_shard, Q,
                       (const uint8_t *)d_base, (const uint64_t *)d_src, (const uint64_t *)d_first, n, (uint8_t *)d_dst, cap);
    return hipGetLastError();
}

hipError_t launch_meta_winners(const void *d_ordinal, const void *d_copies, size_t n, uint64_t base, void *d_win, uint64_t num_strings,
                               hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(meta_winners_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, (const uint64_t *)d_ordinal,
                       (const uint64_t *)d_copies, n, base, (unsigned long long *)d_win, num_strings);
    return hipGetLastError();
}

hipError_t launch_meta_winner_values(const void *d_win, uint64_t num_strings, const void *d_voff, uint64_t c0, uint64_t c1, void *d_len,
                                     void *d_src, void *d_given, hipStream_t stream) {
    hipLaunchKernelGGL(meta_winner_values_kernel, dim3((unsigned)((num_strings + 1 + 255) / 256)), dim3(256), 0, stream, (const uint64_t *)d_win,
                       num_strings, (const uint64_t *)d_voff, c0, c1, (uint64_t *)d_len, (uint64_t *)d_src, (unsigned long long *)d_given);
    return hipGetLastError();
}

}  // namespace rsb
