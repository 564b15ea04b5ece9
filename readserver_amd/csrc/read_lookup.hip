// read_lookup.hip -- "is w itself a read, and how many copies of it does the shard hold?" by backward search from the
// terminator rows (gfx950).
//
// In SGA's multi-string BWT the rows [0, num_strings) = [0, C['A']) are the suffixes that begin with a terminator.
// Stepping w backwards from that row range (updateInterval, src/bwt/query.cpp:11-15, right to left) ends on the rows
// whose suffix is w$: the reads that END with w.  Such a row holds '$' in the BWT exactly when its read also BEGINS
// there, so
//
//     copies(w) = Occ('$', upper) - Occ('$', lower - 1)        (Occ(., -1) = 0)
//
// is the number of reads equal to w, and upper - lower + 1 the number of reads ending with it.  query_exactmatch's
// boolean (src/bwt/query.cpp:102-120) is copies > 0 -- without enumerating the interval of w, extracting its reads and
// comparing them, and without the select samples / psi hints extraction needs.
//
// Three launches:
//   * a SEED kernel writes one start record per (query, shard), [s][Q] as the search launch expects them:
//     { 0 | L << 40 | INIT_EXPLICIT | INIT_VAR, C['A'] - 1 } -- the interval is all terminator rows, the next symbol is
//     index L - 1, so all L symbols are stepped; no k-mer table is consulted (the pattern ends in '$');
//   * the search launch as it is (search_lines.hip, search_extra::d_init), results as {lower, upper} pairs;
//   * the '$'-COUNT kernel below: one lane per result, one 128-byte line fetch per non-empty result.  Its Occ('$', lower - 1)
//     is also the first of the dense read numbers (rsbwt_locate's ordinal) of the reads equal to w: an optional third
//     output, what the sample table is keyed by (read_meta.hip).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "line_format.h"
#include "rank_device.h"
#include "wave_lines.h"

namespace rsb {

__device__ __forceinline__ ulonglong2 seed_record(const shard_view &ix, bool ok, uint32_t L) {
    ulonglong2 rec;
    // (a shard without terminator rows: C['A'] - 1 would wrap into an interval that looks alive)
    if (!ok || L == 0u || L > 65535u || ix.C[1] == 0ull) {
        rec.x = INIT_INVALID;
        rec.y = 0;
    } else {
        rec.x = ((uint64_t)L << COUNT_BITS) | INIT_EXPLICIT | INIT_VAR;  // lower = 0; next symbol: L - 1
        rec.y = ix.C[1] - 1ull;
    }
    return rec;
}

// one thread per (query, shard): init[s * Q + q]; every query has k symbols (search_init_kernel's twin)
__global__ void __launch_bounds__(256)
read_seed_kernel(const shard_view *__restrict__ shards, uint32_t nshards, const uint8_t *__restrict__ valid, size_t Q, uint32_t k,
                 ulonglong2 *__restrict__ init) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= Q * nshards) return;
    const size_t q = i / nshards, s = i - q * nshards;
    init[s * Q + q] = seed_record(shards[s], valid[q] != 0, k);
}

// the same for queries of lengths of their own, len[q] (search_init_var_kernel's twin)
__global__ void __launch_bounds__(256)
read_seed_var_kernel(const shard_view *__restrict__ shards, uint32_t nshards, const uint8_t *__restrict__ valid,
                     const uint32_t *__restrict__ len, size_t Q, ulonglong2 *__restrict__ init) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= Q * nshards) return;
    const size_t q = i / nshards, s = i - q * nshards;
    init[s * Q + q] = seed_record(shards[s], valid[q] != 0, len[q]);
}

// work[] words of a counting launch (beside the search launch's, search_lines.hip WORK_*)
enum { WORK_RL_RANKED = 13, WORK_RL_CONT = 14, WORK_RL_SECOND = 15 };

// One lane per (query, shard) result; blockIdx.y = shard, so a wave's lines come from one shard.  pairs[s][Q] =
// {lower, upper} as the search left them.  A proper interval (lower <= upper < n) fetches upper's window line; lower - 1
// is ranked off the same line when it lies among that line's own pieces, is the header's count when it is the last
// position of the window before, and goes through the scalar reader (view_occ) otherwise: past the line's own pieces
// (spill chunk / far line), or in another window.
__global__ void __launch_bounds__(64 * WG_WAVES)
read_dollar_count_kernel(const shard_view *__restrict__ shards, const ulonglong2 *__restrict__ pairs, size_t Q,
                         uint64_t *__restrict__ copies, uint64_t *__restrict__ ending, unsigned long long *__restrict__ work,
                         uint64_t *__restrict__ ordinal) {
    __shared__ uint4 s_stage[WG_WAVES][64 * SLOT_U4];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint4 *stage = s_stage[wave];
    const uint32_t stage_lds = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)(lds_void_ptr)stage);
    const uint32_t sid = blockIdx.y;
    const shard_view *sv = shards + sid;
    const char *lines_bytes = reinterpret_cast<const char *>(sv->lines);
    const uint32_t S = sv->sp.S;
    const double inv = sv->sp.inv;
    const uint64_t n = sv->n;
    const uint32_t nlines = (uint32_t)sv->nlines;

    const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool in = q < Q;
    const size_t at = (size_t)sid * Q + q;
    ulonglong2 iv = {1, 0};
    if (in) iv = pairs[at];
    const uint64_t lo = iv.x, hi = iv.y;
    const bool proper = in && lo <= hi && hi < n;

    uint32_t w = 0, oU = 0, want = ~0u;
    if (proper) {
        uint32_t pin;
        w = fast_window(hi, S, inv, pin);
        oU = pin + 1u;
        want = w + (w >> GROUP_SHIFT);
        if (want >= nlines) want = 0;  // never for upper < n; keeps a bad position from faulting
    }
    glds_fetch(lines_bytes, want, lane, stage_lds);  // (every lane takes part: lanes with nothing to rank ask for nothing)
    glds_wait();

    uint64_t cp = 0, en = 0, first = 0;
    uint32_t conts = 0;
    bool second = false;
    if (proper) {
        const staged_line L = {own_stage_row(stage, lane), lane & 7u};
        const line_head h = read_head(L);
        // '$' before the window = w * S - (A + C + G + T)   (line_format.h)
        const uint64_t before = (uint64_t)w * S - (read_count(L, 1u) + read_count(L, 2u) + read_count(L, 3u) + read_count(L, 4u));
        uint64_t occU, occL = 0;
        if (oU <= h.span) {
            occU = before + staged_dollars(L, h, oU);
        } else {
            occU = view_occ(*sv, 0u, hi);
            conts += 1u;
        }
        if (lo != 0ull) {  // Occ('$', -1) = 0
            const uint64_t pL = lo - 1ull, w0 = (uint64_t)w * S;
            if (pL >= w0) {  // the same window
                const uint32_t oL = (uint32_t)(pL - w0) + 1u;
                if (oL <= h.span) {
                    occL = before + staged_dollars(L, h, oL);
                } else {
                    occL = view_occ(*sv, 0u, pL);
                    conts += 1u;
                }
            } else if (pL + 1ull == w0) {  // the last position of the window before: everything the header counts
                occL = before;
            } else {  // the interval spans windows
                occL = view_occ(*sv, 0u, pL);
                second = true;
            }
        }
        cp = occU - occL;
        en = hi - lo + 1ull;
        first = cp ? occL : 0ull;  // the reads equal to the query are the ordinals [occL, occL + cp)
    }
    if (in) {
        copies[at] = cp;
        if (ending) ending[at] = en;
        if (ordinal) ordinal[at] = first;
    }
    if (work) {
        const uint32_t ranked = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(proper));
        const uint32_t c = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(conts >= 1u)) +
                           (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(conts >= 2u));
        const uint32_t s2 = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(second));
        if (lane == 0u) {
            if (ranked) atomicAdd(&work[WORK_RL_RANKED], (unsigned long long)ranked);
            if (c) atomicAdd(&work[WORK_RL_CONT], (unsigned long long)c);
            if (s2) atomicAdd(&work[WORK_RL_SECOND], (unsigned long long)s2);
        }
    }
}

hipError_t launch_read_seed(const shard_view *d_shards, uint32_t nshards, const void *d_valid, const void *d_len, size_t Q, uint32_t k,
                            void *d_init, hipStream_t stream) {
    if (Q == 0 || nshards == 0) return hipSuccess;
    const size_t nrec = Q * nshards;
    const dim3 grid((unsigned)((nrec + 255) / 256));
    if (d_len)
        hipLaunchKernelGGL(read_seed_var_kernel, grid, dim3(256), 0, stream, d_shards, nshards, (const uint8_t *)d_valid,
                           (const uint32_t *)d_len, Q, (ulonglong2 *)d_init);
    else
        hipLaunchKernelGGL(read_seed_kernel, grid, dim3(256), 0, stream, d_shards, nshards, (const uint8_t *)d_valid, Q, k,
                           (ulonglong2 *)d_init);
    return hipGetLastError();
}

hipError_t launch_dollar_count(const shard_view *d_shards, uint32_t nshards, const void *d_pairs, size_t Q, void *d_copies,
                               void *d_ending, unsigned long long *d_work, hipStream_t stream, void *d_ordinal) {
    if (Q == 0 || nshards == 0) return hipSuccess;
    if (nshards > 65535u) return hipErrorInvalidValue;  // (the shard is the grid's y)
    const dim3 grid((unsigned)((Q + 64 * WG_WAVES - 1) / (64 * WG_WAVES)), nshards);
    hipLaunchKernelGGL(read_dollar_count_kernel, grid, dim3(64 * WG_WAVES), 0, stream, d_shards, (const ulonglong2 *)d_pairs, Q,
                       (uint64_t *)d_copies, (uint64_t *)d_ending, d_work, (uint64_t *)d_ordinal);
    return hipGetLastError();
}

}  // namespace rsb
