// site_counts.hip -- rsbwt_set_site_sample_counts (include/rsbwt.h): which samples carry each allele of a site, on the GPU
// (gfx950).  The search, the walks, the span filter, the extraction and the alignment are the existing ones (gt_narrow.hip,
// interval_rows.hip, locate.hip, extract_lines.hip, ksw_align.hip); what is here is the hand-off between them, so that
// from the narrowing to the matrices no row record, read byte or verdict crosses PCIe (kernels.h lists the launches).
//
//   STAGE 2  one lane per row the span filter kept (gt_site_row: the filter's record with the row's ordinal):
//     1. the head bit of its ordinal (one dword load).  A row on a copy that is no head is done: every copy of a string lies
//        in the same leg intervals at the same offsets, so the head copy is among the kept rows whenever any copy is.
//        (rsbwt_set_site_reads, site_reads.hip, has no sample table and skips this step: every kept row goes on.)
//     2. (request << 40 | ordinal) goes into an open-addressing set, one region per shard (sample_counts.hip's regions and
//        its discipline: EVERY access to a slot's key is the agent-scope 64-bit compare-and-swap itself, never a plain load
//        that one XCD's L2 could serve stale).  Old value empty or equal: this is the entry's slot; another key: next slot.
//     3. beside the key: the winner of the CAS stores the read's read_row (every row of the entry would store the same; it
//        is read by the next launch only), and EVERY row takes atomicMin on the entry's needed read length: 0 for a row
//        that is not pending, gt_left_needed_len for a pending LEFT row (gt_span_rule.h).  A read is a candidate iff any of
//        its rows passes, that is iff its length reaches the smallest need.
//   STAGE 3  one lane per slot compacts the entries into site_item records (a wave claims its records with one atomic);
//     the distinct (shard, read_row) among them: radix sort of shard << row_bits | read_row, a flag where the key changes,
//     an exclusive scan -> every item's read number, the distinct reads' rows shard by shard and the shards' segments, which
//     is what launch_extract_ragged takes.  Requests that share a window share their reads.  A read that did not fit the
//     first stride is extracted again at a stride over 4,096; raddr[] then says where each read lies.
//   STAGE 4  one lane per item: its read's length against its need; a survivor is handed to launch_gt_align through the
//     batch's indirection (rid / raddr / rlen) under its request's number, the others under UINT64_MAX, which the alignment
//     answers RSBWT_GT_INVALID without running.  perm: the items sorted by their longest pass (radix sort on 13 bits), so
//     that a wave's lanes finish together and a block's class fits it closely, as the host form arranges.
//   STAGE 5  one lane per item with one of the three KEEP verdicts tallies its value's records (sample_records.h).
// aligned[q] and carriers[q] take one add per wave and distinct request; the work counters sit 256 bytes apart.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>  // (rocPRIM's texture iterator calls memset without including it)

#include <algorithm>

#include <rocprim/rocprim.hpp>

#include "../../include/rsbwt.h"
#include "gt_span_rule.h"
#include "kernels.h"
#include "sample_records.h"

namespace rsb {

namespace {

constexpr unsigned long long SITE_EMPTY = ~0ull;
constexpr uint64_t ORDINAL_MASK = (1ull << 40) - 1ull;

__device__ __forceinline__ unsigned long long *site_counter(unsigned long long *work, int which) { return work + (size_t)which * TALLY_WORK_STRIDE; }

// base + the number of set lanes below this one: a wave claims popcount(mask) records with one atomic
__device__ __forceinline__ uint64_t wave_claim(unsigned long long *counter, uint64_t mask, uint32_t lane) {
    unsigned long long base = 0;
    if (lane == 0u) base = atomicAdd(counter, (unsigned long long)__builtin_popcountll(mask));
    base = ((unsigned long long)__builtin_amdgcn_readfirstlane((uint32_t)(base >> 32)) << 32) | __builtin_amdgcn_readfirstlane((uint32_t)base);
    return base + (uint64_t)__builtin_popcountll(mask & ((1ull << lane) - 1ull));
}

__global__ void __launch_bounds__(256)
site_legs_kernel(const gt_leg *__restrict__ legs, size_t cells, unsigned long long *__restrict__ work) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool leg = t < cells && legs[t].a != 0xFFFFFFFFu;
    const uint64_t mask = __builtin_amdgcn_ballot_w64(leg);
    if ((threadIdx.x & 63u) == 0u && mask) atomicAdd(site_counter(work, SITE_WORK_LEGS), (unsigned long long)__builtin_popcountll(mask));
}

__global__ void __launch_bounds__(256)
site_region_rows_kernel(const gt_site_row *__restrict__ rows, const unsigned long long *__restrict__ nrows, uint64_t cap, uint32_t S,
                        unsigned long long *__restrict__ rows_of) {
    const uint64_t n = *nrows < cap ? *nrows : cap;
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t sh = t < n ? rows[t].shard : ~0u;
    uint64_t left = __builtin_amdgcn_ballot_w64(sh < S);
    while (left) {
        const int j = __builtin_ctzll(left);
        const uint32_t s0 = (uint32_t)__shfl((int)sh, j, 64);
        const uint64_t same = __builtin_amdgcn_ballot_w64(sh == s0);
        if (lane == (uint32_t)j) atomicAdd(&rows_of[s0], (unsigned long long)__builtin_popcountll(same));
        left &= ~same;
    }
}

// HEADS: the counts call's rule, a row on a head copy of a shard with a sample table; else (rsbwt_set_site_reads) every row
template <bool HEADS>
__global__ void __launch_bounds__(256)
site_rows_kernel(const gt_batch bt, const gt_leg *__restrict__ legs, const gt_site_row *__restrict__ rows, const unsigned long long *__restrict__ nrows,
                 uint64_t cap, const meta_view *__restrict__ meta, uint32_t S, const site_set set, unsigned long long *__restrict__ work) {
    const uint64_t n = *nrows < cap ? *nrows : cap;
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool head = false;
    if (t < n) {
        const gt_site_row r = rows[t];
        const uint64_t o = r.ordinal;
        if (!HEADS) {
            head = r.shard < S && o <= ORDINAL_MASK;
        } else if (r.shard < S) {
            const meta_view mv = meta[r.shard];
            head = mv.off && mv.heads && o < mv.num_strings && o <= ORDINAL_MASK && ((mv.heads[o >> 5] >> (o & 31u)) & 1u);
#ifdef RSB_SITE_MUTANT_NO_HEAD_TEST
            head = mv.off && o < mv.num_strings && o <= ORDINAL_MASK;
#endif
        }
        if (head) {
            const uint64_t q = bt.slot_query[r.item >> 1];
            uint64_t need = 0;
            if (r.pending) {
                need = gt_left_needed_len(bt.q_pos[q], legs[(size_t)r.shard * bt.nitems + r.item].b, r.offset, bt.k);
                if (need > SITE_NEED_MAX) need = SITE_NEED_MAX;
#ifdef RSB_SITE_MUTANT_NEED_ZERO_PENDING
                need = 0;
#endif
            }
            const unsigned long long key = ((unsigned long long)q << 40) | o;  // q < 2^24, o < num_strings < 2^40: never all ones
            const uint64_t base = set.region[2u * r.shard], mask = set.region[2u * r.shard + 1u];
            uint64_t h = key * 0x9E3779B97F4A7C15ull;
            uint64_t slot = (h ^ (h >> 29)) & mask;
            for (;;) {  // (a region has more slots than rows: a probe always meets its key or an empty slot)
                const unsigned long long old = atomicCAS(&set.keys[base + slot], SITE_EMPTY, key);
                if (old == SITE_EMPTY) {
                    set.row[base + slot] = r.read_row;
                    break;
                }
                if (old == key) break;
                slot = (slot + 1ull) & mask;
            }
#ifdef RSB_SITE_MUTANT_NEED_BY_MAX
            atomicMax(&set.need[base + slot], need ? (uint32_t)need : 0u);  // (the mutant's set_need starts at 0: launch_site_rows)
#else
            atomicMin(&set.need[base + slot], (uint32_t)need);
#endif
        }
    }
    const uint64_t heads = __builtin_amdgcn_ballot_w64(head);
    if ((threadIdx.x & 63u) == 0u && heads) atomicAdd(site_counter(work, SITE_WORK_HEADS), (unsigned long long)__builtin_popcountll(heads));
}

// the shard whose region holds slot t: the last one that starts at or before it (the regions ascend)
__device__ __forceinline__ uint32_t site_shard_of_slot(const uint64_t *__restrict__ region, uint32_t S, uint64_t t) {
    uint32_t lo = 0, hi = S;
    while (hi - lo > 1u) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (region[2u * mid] <= t) lo = mid;
        else hi = mid;
    }
    return lo;
}

__global__ void __launch_bounds__(256)
site_compact_kernel(const site_set set, uint32_t S, uint32_t row_bits, site_item *__restrict__ items, uint64_t *__restrict__ sort_key,
                    uint32_t *__restrict__ sort_idx, uint64_t cap, unsigned long long *__restrict__ work) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    const unsigned long long key = t < set.nslots ? set.keys[t] : SITE_EMPTY;  // (the inserts ended with the launch before this one)
    const bool full = key != SITE_EMPTY;
    const uint64_t mask = __builtin_amdgcn_ballot_w64(full);
    if (mask == 0ull) return;  // (wave-uniform)
    const uint64_t at = wave_claim(site_counter(work, SITE_WORK_ITEMS), mask, lane);
    if (full && at < cap) {
        const uint32_t sh = site_shard_of_slot(set.region, S, t);
        const uint64_t rr = set.row[t];
        items[at] = site_item{key & ORDINAL_MASK, rr, (uint32_t)(key >> 40), sh, set.need[t], 0u};
        sort_key[at] = ((uint64_t)sh << row_bits) | rr;
        sort_idx[at] = (uint32_t)at;
    }
}

// flag[i] = 1 where the sorted key differs from the one before it; flag[n] = 0 (the scan's last element is then the total)
__global__ void __launch_bounds__(256)
site_flags_kernel(const uint64_t *__restrict__ key, size_t n, uint64_t *__restrict__ flag) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n) return;
    flag[i] = i < n && (i == 0 || key[i] != key[i - 1]) ? 1ull : 0ull;
}

__global__ void __launch_bounds__(256)
site_assign_kernel(const uint64_t *__restrict__ key, const uint32_t *__restrict__ idx, const uint64_t *__restrict__ flag, const uint64_t *__restrict__ first,
                   size_t n, uint32_t S, uint32_t row_bits, site_item *__restrict__ items, uint64_t *__restrict__ rows, uint64_t *__restrict__ seg,
                   uint64_t *__restrict__ nreads) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        const uint64_t r = first[i] + flag[i] - 1ull;  // (i = 0 is flagged: never below 0)
        items[idx[i]].rid = (uint32_t)r;
        if (flag[i]) rows[r] = key[i] & ((1ull << row_bits) - 1ull);
    }
    if (i <= S) {  // seg[p] = the distinct reads of the shards below p: first[] at the first key of shard p or above
        const uint64_t want = (uint64_t)i << row_bits;
        size_t lo = 0, hi = n;
        while (lo < hi) {
            const size_t mid = lo + ((hi - lo) >> 1);
            if (key[mid] < want) lo = mid + 1;
            else hi = mid;
        }
        seg[i] = first[lo];
    }
    if (i == 0) *nreads = first[n];
}

__global__ void __launch_bounds__(256)
site_over_kernel(const uint32_t *__restrict__ rlen, size_t R, uint64_t *__restrict__ over, unsigned long long *__restrict__ longest) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t len = i < R ? rlen[i] : 0u;
    if (i <= R) over[i] = len == 0xFFFFFFFFu ? 1ull : 0ull;
    // *longest = the longest read that fit (it bounds the alignment's classes): one atomic per wave
    uint32_t v = len == 0xFFFFFFFFu ? 0u : len;
    for (int s = 32; s > 0; s >>= 1) {
        const uint32_t other = (uint32_t)__shfl_xor((int)v, s, 64);
        v = v > other ? v : other;
    }
    if ((threadIdx.x & 63u) == 0u && v) atomicMax(longest, (unsigned long long)v);
}

__global__ void __launch_bounds__(256)
site_wide_kernel(const uint64_t *__restrict__ rows, const uint64_t *__restrict__ seg, uint32_t S, size_t R, const uint64_t *__restrict__ over,
                 const uint64_t *__restrict__ ofirst, uint64_t *__restrict__ wrows, uint64_t *__restrict__ wseg) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < R && over[i]) wrows[ofirst[i]] = rows[i];
    if (i <= S) wseg[i] = ofirst[seg[i]];  // (seg[i] <= R, and ofirst has R + 1 entries)
}

__global__ void __launch_bounds__(256)
site_addr_kernel(const char *__restrict__ narrow, uint32_t stride, const char *__restrict__ wide, uint32_t wide_stride, const uint64_t *__restrict__ over,
                 const uint64_t *__restrict__ ofirst, const uint32_t *__restrict__ wlen, size_t R, uint64_t *__restrict__ raddr, uint32_t *__restrict__ rlen) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= R) return;
    if (wide && over[i]) {
        const uint64_t w = ofirst[i];
        raddr[i] = (uint64_t)(uintptr_t)(wide + w * (size_t)wide_stride);
#ifndef RSB_SITE_MUTANT_WIDE_LEN
        rlen[i] = wlen[w];
#endif
    } else {
        raddr[i] = (uint64_t)(uintptr_t)(narrow + i * (size_t)stride);
    }
}

#ifdef RSB_SITE_MUTANT_FIRST_WINDOW
// (mutant only) firstq[rid] = the smallest request that named the read
__global__ void __launch_bounds__(256)
site_first_request_kernel(const site_item *__restrict__ items, size_t n, uint32_t *__restrict__ firstq) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) atomicMin(&firstq[items[i].rid], items[i].q);
}
#endif

__global__ void __launch_bounds__(256)
site_items_kernel(const site_item *__restrict__ items, size_t n, const uint32_t *__restrict__ rlen, const uint64_t *__restrict__ off, size_t Q,
                  uint64_t *__restrict__ req, uint32_t *__restrict__ rid, uint32_t *__restrict__ perm_key, uint32_t *__restrict__ perm_idx,
                  unsigned long long *__restrict__ aligned, unsigned long long *__restrict__ work, const uint32_t *__restrict__ firstq) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    bool pass = false, too_long = false;
    uint64_t q = 0;
    if (i < n) {
        const site_item it = items[i];
        const uint32_t len = rlen[it.rid];
        q = it.q;
        too_long = len == 0xFFFFFFFFu || len > (uint32_t)RSBWT_KSW_MAX_LEN;
        pass = !too_long && q < Q && len >= it.need;
#ifdef RSB_SITE_MUTANT_NO_LENGTH_RULE
        pass = !too_long && q < Q;
#endif
        uint64_t to = q;
#ifdef RSB_SITE_MUTANT_FIRST_WINDOW
        to = firstq[it.rid];
#endif
        const uint64_t wl = pass ? off[to + 1] - off[to] : 0ull;
        req[i] = pass ? to : ~0ull;
        rid[i] = it.rid;
        perm_key[i] = pass ? (len > wl ? len : (uint32_t)wl) : 0u;
        perm_idx[i] = (uint32_t)i;
    }
    const uint32_t passed = wave_count_by_query(aligned, pass, q, lane);
    const uint64_t longs = __builtin_amdgcn_ballot_w64(too_long);
    if (lane == 0u) {
        if (passed) atomicAdd(site_counter(work, SITE_WORK_ALIGNED), (unsigned long long)passed);
        if (longs) atomicAdd(site_counter(work, SITE_WORK_TOO_LONG), (unsigned long long)__builtin_popcountll(longs));
    }
}

template <bool KEYS_IN_LDS>
__global__ void __launch_bounds__(256)
site_tally_kernel(const site_tally a) {
    extern __shared__ uint64_t lds_keys[];
    const tally_dict d = tally_dict_of<KEYS_IN_LDS>(a.keys, a.C, lds_keys);
    const tally_cells cells = {a.strings, a.copies, a.size_of_sample, a.has_other};
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t R = a.size_of_sample + (a.has_other ? 2u : 0u);
    bool carrier = false;
    uint64_t q = 0, nrec = 0;
    const uint8_t *val = nullptr;
    if (i < a.n) {
        const uint8_t v = a.verdict[i];
        carrier = v == RSBWT_GT_KEEP_PLAIN || v == RSBWT_GT_KEEP_RIGHT || v == RSBWT_GT_KEEP_LEFT;
#ifdef RSB_SITE_MUTANT_KEEP_SITE_MISMATCH
        carrier = carrier || v == RSBWT_GT_SITE_MISMATCH;
#endif
        if (carrier) {
            const site_item it = a.items[i];
            q = it.q;
            const meta_view mv = a.meta[it.shard];  // (an item exists only for a head ordinal of a shard with a table)
            const uint64_t b0 = mv.off[it.ordinal], b1 = mv.off[it.ordinal + 1];
            nrec = (b1 - b0) / R;  // (the tail that is no whole record is dropped)
            val = mv.bytes + b0;
        }
    }
    const uint32_t unknown = tally_values(cells, d, a.C, lane, nrec, val, q);
    const uint32_t kept = wave_count_by_query(a.carriers, carrier, q, lane);
    if (lane == 0u && kept) atomicAdd(site_counter(a.work, SITE_WORK_KEPT), (unsigned long long)kept);
    uint64_t mine = nrec;
    for (int s = 32; s > 0; s >>= 1) mine += __shfl_xor(mine, s, 64);
    if (lane == 0u && mine) atomicAdd(site_counter(a.work, SITE_WORK_RECORDS), (unsigned long long)mine);
    wave_count(site_counter(a.work, SITE_WORK_UNKNOWN), unknown, lane);
}

inline dim3 grid_of(size_t n) { return dim3((unsigned)((n + 255) / 256)); }
inline size_t al256(size_t b) { return (b + 255) & ~(size_t)255; }

size_t sort_pairs_bytes64(size_t n) {
    size_t bytes = 0;
    if (rocprim::radix_sort_pairs(nullptr, bytes, (const uint64_t *)nullptr, (uint64_t *)nullptr, (const uint32_t *)nullptr, (uint32_t *)nullptr, n, 0u,
                                  64u, (hipStream_t) nullptr) != hipSuccess)
        return 0;
    return al256(bytes);
}

size_t sort_pairs_bytes32(size_t n) {
    size_t bytes = 0;
    if (rocprim::radix_sort_pairs(nullptr, bytes, (const uint32_t *)nullptr, (uint32_t *)nullptr, (const uint32_t *)nullptr, (uint32_t *)nullptr, n, 0u,
                                  32u, (hipStream_t) nullptr) != hipSuccess)
        return 0;
    return al256(bytes);
}

}  // namespace

// d_tmp of launch_site_reads: the sorted keys and indices, the flags and their scan, then the sort's and the scan's own
size_t site_reads_tmp_bytes(size_t n) {
    const size_t own = std::max(sort_pairs_bytes64(n), meta_scan_bytes(n + 1));
    return al256(n * 8) + al256(n * 4) + 2 * al256((n + 1) * 8) + own + 256;
}

size_t site_perm_tmp_bytes(size_t n) { return sort_pairs_bytes32(n) + 256; }

hipError_t launch_site_legs(const void *d_legs, size_t cells, unsigned long long *d_work, hipStream_t stream) {
    if (cells == 0) return hipSuccess;
    hipLaunchKernelGGL(site_legs_kernel, grid_of(cells), dim3(256), 0, stream, (const gt_leg *)d_legs, cells, d_work);
    return hipGetLastError();
}

hipError_t launch_site_rows(const gt_batch &bt, const void *d_legs, const void *d_rows, const unsigned long long *d_nrows, uint64_t cap,
                            const meta_view *d_meta, bool heads_only, uint32_t S, bool tight, void *d_rows_of, const site_set &set,
                            unsigned long long *d_work, hipStream_t stream) {
    if (cap == 0) return hipSuccess;
    if (heads_only && !d_meta) return hipErrorInvalidValue;  // (the head test needs the sample table: never a quiet "every row")
    hipError_t e = hipMemsetAsync(d_rows_of, 0, (size_t)S * 8, stream);
    if (e == hipSuccess) e = hipMemsetAsync(set.keys, 0xFF, set.nslots * 8, stream);
#ifdef RSB_SITE_MUTANT_NEED_BY_MAX
    if (e == hipSuccess) e = hipMemsetAsync(set.need, 0, set.nslots * 4, stream);
#else
    if (e == hipSuccess) e = hipMemsetAsync(set.need, 0xFF, set.nslots * 4, stream);
#endif
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(site_region_rows_kernel, grid_of(cap), dim3(256), 0, stream, (const gt_site_row *)d_rows, d_nrows, cap, S,
                       (unsigned long long *)d_rows_of);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    // (cap 0: the regions alone, from the counts just made)
    if ((e = launch_sample_regions(nullptr, nullptr, 0, 0, S, tight, d_rows_of, set.region, stream)) != hipSuccess) return e;
    if (heads_only)
        hipLaunchKernelGGL(site_rows_kernel<true>, grid_of(cap), dim3(256), 0, stream, bt, (const gt_leg *)d_legs, (const gt_site_row *)d_rows, d_nrows, cap,
                           d_meta, S, set, d_work);
    else
        hipLaunchKernelGGL(site_rows_kernel<false>, grid_of(cap), dim3(256), 0, stream, bt, (const gt_leg *)d_legs, (const gt_site_row *)d_rows, d_nrows, cap,
                           d_meta, S, set, d_work);
    return hipGetLastError();
}

hipError_t launch_site_compact(const site_set &set, uint32_t S, uint32_t row_bits, void *d_items, void *d_sort_key, void *d_sort_idx, uint64_t cap,
                               unsigned long long *d_work, hipStream_t stream) {
    if (set.nslots == 0) return hipSuccess;
    hipLaunchKernelGGL(site_compact_kernel, grid_of(set.nslots), dim3(256), 0, stream, set, S, row_bits, (site_item *)d_items, (uint64_t *)d_sort_key,
                       (uint32_t *)d_sort_idx, cap, d_work);
    return hipGetLastError();
}

hipError_t launch_site_reads(void *d_items, size_t n, uint32_t S, uint32_t row_bits, void *d_sort_key, void *d_sort_idx, void *d_tmp, size_t tmp_bytes,
                             void *d_rows, void *d_seg, void *d_nreads, hipStream_t stream) {
    if (n == 0 || n >= (1ull << 31)) return hipErrorInvalidValue;
    uint8_t *p = (uint8_t *)d_tmp;
    uint64_t *key = (uint64_t *)p;
    uint32_t *idx = (uint32_t *)(p + al256(n * 8));
    uint64_t *flag = (uint64_t *)(p + al256(n * 8) + al256(n * 4)), *first = flag + al256((n + 1) * 8) / 8;
    uint8_t *own = (uint8_t *)(first + al256((n + 1) * 8) / 8);
    if (own > p + tmp_bytes) return hipErrorInvalidValue;
    size_t own_bytes = (size_t)(p + tmp_bytes - own);
    uint32_t shard_bits = 0;
    while ((1ull << shard_bits) < (uint64_t)S + 1ull) ++shard_bits;  // (seg[S] searches for the key S << row_bits)
    const unsigned end_bit = row_bits + shard_bits > 64u ? 64u : row_bits + shard_bits;
    hipError_t e = rocprim::radix_sort_pairs(own, own_bytes, (const uint64_t *)d_sort_key, key, (const uint32_t *)d_sort_idx, idx, n, 0u, end_bit, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(site_flags_kernel, grid_of(n + 1), dim3(256), 0, stream, key, n, flag);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = launch_meta_scan(own, (size_t)(p + tmp_bytes - own), flag, first, n + 1, stream)) != hipSuccess) return e;
    hipLaunchKernelGGL(site_assign_kernel, grid_of(std::max<size_t>(n, (size_t)S + 1)), dim3(256), 0, stream, key, idx, flag, first, n, S, row_bits,
                       (site_item *)d_items, (uint64_t *)d_rows, (uint64_t *)d_seg, (uint64_t *)d_nreads);
    return hipGetLastError();
}

hipError_t launch_site_over(const void *d_rlen, size_t R, void *d_over, void *d_ofirst, unsigned long long *d_longest, void *d_tmp, size_t tmp_bytes,
                            hipStream_t stream) {
    hipLaunchKernelGGL(site_over_kernel, grid_of(R + 1), dim3(256), 0, stream, (const uint32_t *)d_rlen, R, (uint64_t *)d_over, d_longest);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_meta_scan(d_tmp, tmp_bytes, d_over, d_ofirst, R + 1, stream);
}

hipError_t launch_site_wide(const void *d_rows, const void *d_seg, uint32_t S, size_t R, const void *d_over, const void *d_ofirst, void *d_wrows,
                            void *d_wseg, hipStream_t stream) {
    hipLaunchKernelGGL(site_wide_kernel, grid_of(std::max<size_t>(R, (size_t)S + 1)), dim3(256), 0, stream, (const uint64_t *)d_rows, (const uint64_t *)d_seg,
                       S, R, (const uint64_t *)d_over, (const uint64_t *)d_ofirst, (uint64_t *)d_wrows, (uint64_t *)d_wseg);
    return hipGetLastError();
}

hipError_t launch_site_addr(const void *d_narrow, uint32_t stride, const void *d_wide, uint32_t wide_stride, const void *d_over, const void *d_ofirst,
                            const void *d_wlen, size_t R, void *d_raddr, void *d_rlen, hipStream_t stream) {
    if (R == 0) return hipSuccess;
    hipLaunchKernelGGL(site_addr_kernel, grid_of(R), dim3(256), 0, stream, (const char *)d_narrow, stride, (const char *)d_wide, wide_stride,
                       (const uint64_t *)d_over, (const uint64_t *)d_ofirst, (const uint32_t *)d_wlen, R, (uint64_t *)d_raddr, (uint32_t *)d_rlen);
    return hipGetLastError();
}

hipError_t launch_site_items(const void *d_items, size_t n, const void *d_rlen, const void *d_off, size_t Q, void *d_req, void *d_rid,
                             void *d_perm_key, void *d_perm_idx, unsigned long long *d_aligned, unsigned long long *d_work, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const uint32_t *firstq = nullptr;
#ifdef RSB_SITE_MUTANT_FIRST_WINDOW
    // (mutant only: its scratch is taken from the stream's pool and goes back there)
    uint32_t *fq = nullptr;
    hipError_t em = hipMallocAsync((void **)&fq, n * 4, stream);
    if (em == hipSuccess) em = hipMemsetAsync(fq, 0xFF, n * 4, stream);
    if (em != hipSuccess) return em;
    hipLaunchKernelGGL(site_first_request_kernel, grid_of(n), dim3(256), 0, stream, (const site_item *)d_items, n, fq);
    firstq = fq;
#endif
    hipLaunchKernelGGL(site_items_kernel, grid_of(n), dim3(256), 0, stream, (const site_item *)d_items, n, (const uint32_t *)d_rlen, (const uint64_t *)d_off,
                       Q, (uint64_t *)d_req, (uint32_t *)d_rid, (uint32_t *)d_perm_key, (uint32_t *)d_perm_idx, d_aligned, d_work, firstq);
    const hipError_t e = hipGetLastError();
#ifdef RSB_SITE_MUTANT_FIRST_WINDOW
    (void)hipFreeAsync(fq, stream);
#endif
    return e;
}

hipError_t launch_site_perm(void *d_perm_key, void *d_perm_idx, size_t n, void *d_key_out, void *d_perm, void *d_tmp, size_t tmp_bytes,
                            hipStream_t stream) {
    if (n == 0) return hipSuccess;
    size_t bytes = tmp_bytes;
    // (a pass has at most 4,096 rows: 13 bits)
    return rocprim::radix_sort_pairs(d_tmp, bytes, (const uint32_t *)d_perm_key, (uint32_t *)d_key_out, (const uint32_t *)d_perm_idx, (uint32_t *)d_perm, n,
                                     0u, 13u, stream);
}

hipError_t launch_site_tally(const site_tally &a, hipStream_t stream) {
    if (a.n == 0) return hipSuccess;
    if ((size_t)a.C * 8 <= TALLY_LDS_BYTES) hipLaunchKernelGGL(site_tally_kernel<true>, grid_of(a.n), dim3(256), (size_t)a.C * 8, stream, a);
    else hipLaunchKernelGGL(site_tally_kernel<false>, grid_of(a.n), dim3(256), 0, stream, a);
    return hipGetLastError();
}

}  // namespace rsb
