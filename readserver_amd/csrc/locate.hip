// locate.hip -- where a row lies: SA row -> (row of its read's full suffix, dense read number, offset in the read)
// (gfx950).
//
// For a row r the LF walk of extractPrefix (src/bwt/query.cpp:49-57): while BWT[r] != '$': r = C[b] + Occ(b, r) - 1.
//   read_row  the row the walk ends on (the read identity of kmer_reads.hip, kr_ident_kernel)
//   offset    the LF steps taken = the length extractPrefix returns
//   ordinal   Occ('$', read_row) - 1, in [0, num_strings): the read's number among the shard's reads
// A row >= bwlen, or one whose walk needs more than max_steps steps, is NOT LOCATED: read_row = ordinal = UINT64_MAX,
// offset = UINT32_MAX.
//
// The walk is extract_lines.hip's prefix walk without its characters: one lane per row, a window line per octet of lanes
// through LDS (wave_lines.h), symbol and rank off one look at the quarter's 24 pieces (rank_device.h, char_rank24), spill
// chunks and far chains continued lazily in the lane's next pass.  No psi walk, no character stores, no prefix move.  At
// the terminal step the lane holds the line of read_row: '$' before the window is w * S - (A + C + G + T) from its header,
// those inside it staged_dollars (wave_lines.h) -- read_lookup.hip's count; a terminal position inside a continuation
// goes through the scalar reader (view_occ).
//
// Rows are (shard, row) pairs in any order.  A wave walks ONE shard at a time (everything shard-specific in scalar
// registers, as the extraction's launch over a set): it draws blocks of 64 entries from that shard's counter over the
// WHOLE list, keeps the mask of the entries that name its shard, and gives them to free lanes; when the list is
// drained and its own walks have ended it moves to the next shard.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../include/rsbwt.h"
#include "capi_guard.h"
#include "capi_internal.h"
#include "kernels.h"
#include "line_format.h"
#include "rank_device.h"
#include "wave_lines.h"

namespace rsb {

#ifndef RSB_WALK_WG_WAVES
#define RSB_WALK_WG_WAVES 4
#endif
#ifndef RSB_WALK_MIN_WGS
#define RSB_WALK_MIN_WGS 4
#endif
constexpr int LC_WAVES = RSB_WALK_WG_WAVES;
constexpr uint32_t LC_DEFAULT_STEPS = 1u << 20;  // max_steps == 0 (kmer_reads.hip, KR_MAX_STEPS)

// position of the r-th (0-based) set bit of m; r < popcount(m)
__device__ __forceinline__ uint32_t nth_set_bit(uint64_t m, uint32_t r) {
    uint32_t x = (uint32_t)m, pos = 0;
    const uint32_t c0 = (uint32_t)__builtin_popcount(x);
    if (r >= c0) {
        r -= c0;
        x = (uint32_t)(m >> 32);
        pos = 32;
    }
#pragma unroll
    for (uint32_t shift = 16; shift != 0u; shift >>= 1) {
        const uint32_t part = x & ((1u << shift) - 1u);
        const uint32_t c = (uint32_t)__builtin_popcount(part);
        if (r >= c) {
            r -= c;
            x >>= shift;
            pos += shift;
        } else {
            x = part;
        }
    }
    return pos;
}

// the answers of one row: each array may be absent; one plain vector store per array
__device__ __forceinline__ void locate_store(uint64_t *__restrict__ read_row, uint64_t *__restrict__ ordinal,
                                             uint32_t *__restrict__ offset, uint64_t e, uint64_t rr, uint64_t od, uint32_t of) {
    if (read_row) read_row[e] = rr;
    if (ordinal) ordinal[e] = od;
    if (offset) offset[e] = of;
}

// shard_of == nullptr: every entry is a row of shard 0 (nshards == 1).  pools: one counter per shard, POOL_STRIDE u64
// apart, zeroed by the launcher.  row_chunk: entries per draw, a multiple of 64.  work (optional): [0] += rows that
// ended on '$', [1] += LF steps.  n_dev (optional): the list ends at min(n, *n_dev) -- a count only the device knows.
__global__ void __launch_bounds__(64 * LC_WAVES, RSB_WALK_MIN_WGS)
locate_wave_kernel(const shard_view *__restrict__ shards, uint32_t nshards, const uint32_t *__restrict__ shard_of,
                   const uint64_t *__restrict__ rows, uint64_t n, uint32_t max_steps, uint64_t *__restrict__ read_row,
                   uint64_t *__restrict__ ordinal, uint32_t *__restrict__ offset, unsigned long long *__restrict__ pools,
                   unsigned long long *__restrict__ work, uint32_t row_chunk, const uint64_t *__restrict__ n_dev) {
    __shared__ uint4 s_stage[LC_WAVES][64 * SLOT_U4];
    if (n_dev != nullptr) {  // (the same for every lane of the launch)
        const uint64_t nd = *n_dev;
        n = nd < n ? nd : n;
        if (n == 0ull) return;
    }
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint4 *stage = s_stage[wave];
    const uint32_t stage_lds = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)(lds_void_ptr)stage);
    const staged_line L = {own_stage_row(stage, lane), lane & 7u};
    const uint64_t below = (1ull << lane) - 1ull;
    unsigned long long walked = 0, steps_all = 0;
    uint32_t sid = blockIdx.x % nshards;
    for (uint32_t visited = 0; visited < nshards; ++visited, sid = (sid + 1u == nshards) ? 0u : sid + 1u) {
    const shard_view *sv = shards + sid;
    const char *lines_bytes = reinterpret_cast<const char *>(sv->lines);
    const uint32_t S = sv->sp.S, nlines = (uint32_t)sv->nlines;
    const double inv = sv->sp.inv;
    const uint64_t ix_n = sv->n;
    unsigned long long *pool = pools + (size_t)sid * POOL_STRIDE;
    uint32_t ctab_lo, ctab_hi;  // C[1..4] in lanes 0..3, read with ds_bpermute
    {
        const uint32_t l3 = lane & 3u;
        const uint64_t cv = l3 == 0u ? sv->C[1] : l3 == 1u ? sv->C[2] : l3 == 2u ? sv->C[3] : sv->C[4];
        ctab_lo = (uint32_t)cv;
        ctab_hi = (uint32_t)(cv >> 32);
    }
    // the hand-out (wave-uniform): the chunk drawn from the shard's counter, the block of 64 entries being given out
    // and which of its entries name this shard and are not given out yet; myrow: the row of entry blk + lane
    uint64_t next = 0, end = 0, blk = 0, mmask = 0;
    bool drained = false;
    uint64_t myrow = 0;
    bool have = false;
    uint64_t ent = 0, idx = 0;
    uint32_t steps = 0;
    uint32_t cont = 0, cblk = 0, cdw = 0, co = 0, tries = 0, w = 0;
    uint32_t acc_lo[4] = {0, 0, 0, 0}, acc_hi = 0;
    for (;;) {
        // ---- rows to the lanes that have none
        uint64_t want_mask = __builtin_amdgcn_ballot_w64(!have);
        while (want_mask != 0ull) {
            if (mmask == 0ull) {
                if (drained) break;
                if (next >= end) {
                    unsigned long long c0 = 0;
                    if (lane == 0u) c0 = atomicAdd(pool, (unsigned long long)row_chunk);
                    c0 = ((unsigned long long)__builtin_amdgcn_readfirstlane((uint32_t)(c0 >> 32)) << 32) | __builtin_amdgcn_readfirstlane((uint32_t)c0);
                    if (c0 >= n) {
                        drained = true;
                        next = end = 0;
                        break;
                    }
                    next = c0;
                    end = c0 + row_chunk < n ? c0 + row_chunk : n;
                }
                blk = next;
                next = next + 64u < end ? next + 64u : end;
                const uint64_t e = blk + lane;
                // (an entry that names no shard of the launch is answered, as not located, by the waves on shard 0)
                const uint32_t tag = e < end && shard_of != nullptr ? shard_of[e] : 0u;
                const bool mine = e < end && (tag == sid || (sid == 0u && tag >= nshards));
                myrow = mine ? (tag < nshards ? rows[e] : ~0ull) : 0ull;
                mmask = __builtin_amdgcn_ballot_w64(mine);
                continue;
            }
            const uint32_t nw = (uint32_t)__builtin_popcountll(want_mask), nm = (uint32_t)__builtin_popcountll(mmask);
            const uint32_t k = nw < nm ? nw : nm;
            const uint32_t rj = (uint32_t)__builtin_popcountll(want_mask & below);
            const bool take = !have && rj < k;
            const uint32_t src = nth_set_bit(mmask, take ? rj : 0u);
            // (every lane is active here: a ds_bpermute returns 0 from a masked-off source lane)
            const uint32_t rlo = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(src << 2), (int)(uint32_t)myrow);
            const uint32_t rhi = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(src << 2), (int)(uint32_t)(myrow >> 32));
            if (take) {
                ent = blk + src;
                idx = ((uint64_t)rhi << 32) | rlo;
                steps = 0;
                cont = 0;
                have = true;
                if (idx >= ix_n) {  // not a row of this shard
                    locate_store(read_row, ordinal, offset, ent, ~0ull, ~0ull, 0xFFFFFFFFu);
                    have = false;
                }
            }
            mmask = k == nm ? 0ull : mmask & ~((1ull << nth_set_bit(mmask, k)) - 1ull);
            want_mask = __builtin_amdgcn_ballot_w64(!have);
        }
        if (__builtin_amdgcn_ballot_w64(have) == 0ull) {
            if (drained) break;
            continue;
        }
        // ---- this lane's line (extract_prefix_wave_kernel's pass, without the characters)
        uint32_t line = 0, o = 0;
        if (have && cont == 0u) {
            uint32_t pin;
            w = fast_window(idx, S, inv, pin);
            line = w + (w >> GROUP_SHIFT);
            o = pin + 1u;
            if (line >= nlines) line = 0;
            tries = 0;
        }
        const uint32_t want = have ? (cont ? cblk : line) : ~0u;
        glds_fetch(lines_bytes, want, lane, stage_lds);
        glds_wait();
        const bool in_chunk = cont == KIND_CHUNK;
        bool scan = false, forced = false;
        uint32_t dw = HDR_DWORDS, rem = 0, cq = 0;
        if (have) {
            if (!in_chunk) {  // a window line, or the far line that continues one (same header)
                const line_head h = read_head(L);
                const uint32_t oe = cont ? co : o;
                if (oe <= h.span) {
                    cq = (oe > h.s1 ? 1u : 0u) + (oe > h.s2 ? 1u : 0u) + (oe > h.s3 ? 1u : 0u);
                    const uint32_t start = cq == 0u ? 0u : cq == 1u ? h.s1 : cq == 2u ? h.s2 : h.s3;
                    dw = HDR_DWORDS + 6u * cq;
                    rem = oe - start;
                    scan = true;
                } else if (h.kind == KIND_FAR) {
                    cblk = L.dword(LINE_DWORDS - 1u);
                    if (cblk >= nlines) cblk = 0;
                    cont = KIND_FAR;
                    co = oe - h.span;
                } else if (h.kind == KIND_CHUNK && cont == 0u) {
                    const uint4 h0 = L.u4(0), h1 = L.u4(4);  // the four count words (dwords 0..7)
                    acc_lo[0] = h0.x; acc_lo[1] = h0.z; acc_lo[2] = h1.x; acc_lo[3] = h1.z;
                    acc_hi = (h0.y & 0xFFu) | ((h0.w & 0xFFu) << 8) | ((h1.y & 0xFFu) << 16) | (h1.w << 24);
                    cdw = read_chunk_dword(L);
                    cblk = (w >> GROUP_SHIFT) * (GROUP + 1u) + GROUP;
                    if (cblk >= nlines) cblk = 0;
                    cont = KIND_CHUNK;
                    co = oe - h.span;
                } else {
                    scan = forced = true;  // beyond what the index holds: never for idx < n
                }
            } else {
                dw = cdw + 2u;
                rem = co;
                scan = true;
            }
            if (!scan && ++tries > 72u) scan = forced = true;  // a corrupt chain
        }
        uint32_t r6[6];
        load24(L, dw, r6);
        const char_rank cr = char_rank24(r6, scan ? rem : 0u, 0u);
        const uint32_t c = cr.c;
        const uint32_t ci = (c - 1u) & 3u;
        uint64_t base;
        if (in_chunk) {
            const uint2 hd = L.u2(cdw);
            const uint32_t hw = ci < 2u ? hd.x : hd.y;
            const uint32_t alo = ci == 0u ? acc_lo[0] : ci == 1u ? acc_lo[1] : ci == 2u ? acc_lo[2] : acc_lo[3];
            base = (((uint64_t)((acc_hi >> (8u * ci)) & 0xFFu) << 32) | alo) + ((hw >> (12u * (ci & 1u))) & 0xFFFu);
        } else {
            const uint32_t hb = read_half(L, ci + 1u);
            const uint32_t m = matched24(L, HDR_DWORDS + 6u * (cq & 2u), cr.tab);
            base = read_count(L, ci + 1u) + (cq >= 2u ? hb : 0u) + ((cq & 1u) ? m : 0u);
        }
        // C[c], with every lane active
        const uint64_t pc = ((uint64_t)(uint32_t)__builtin_amdgcn_ds_bpermute((int)(ci << 2), (int)ctab_hi) << 32) |
                            (uint32_t)__builtin_amdgcn_ds_bpermute((int)(ci << 2), (int)ctab_lo);
        if (scan) {
            if (forced) {  // the index does not hold the position: no answer, and the walk ends
                locate_store(read_row, ordinal, offset, ent, ~0ull, ~0ull, 0xFFFFFFFFu);
                have = false;
            } else if (c == 0u || c > 4u) {  // '$': idx is the row of the read's full suffix (query.cpp:52)
                uint64_t od = 0;
                if (ordinal) {
                    if (cont == 0u) {
                        // the window line of idx is staged and the position lies among its own pieces
                        const line_head h = read_head(L);
                        const uint64_t before = (uint64_t)w * S - (read_count(L, 1u) + read_count(L, 2u) + read_count(L, 3u) + read_count(L, 4u));
                        od = before + staged_dollars(L, h, o) - 1ull;
                    } else {
                        od = view_occ(*sv, 0u, idx) - 1ull;  // in a spill chunk / far line: the scalar reader
                    }
                }
                locate_store(read_row, ordinal, offset, ent, idx, od, steps);
                ++walked;
                have = false;
            } else if (steps >= max_steps) {
                locate_store(read_row, ordinal, offset, ent, ~0ull, ~0ull, 0xFFFFFFFFu);
                have = false;
            } else {
                idx = pc + base + cr.occ - 1ull;  // C[b] + Occ(b, idx) - 1 (query.cpp:55-56)
                ++steps;
                ++steps_all;
                cont = 0;
            }
        }
    }
    }  // (the next shard)
    // (two atomics per lane that walked at all: once per launch)
    if (work) {
        if (walked) atomicAdd(&work[0], walked);
        if (steps_all) atomicAdd(&work[1], steps_all);
    }
}

hipError_t launch_locate(scratch_cache &scratch, const shard_view *d_shards, uint32_t nshards, const void *d_shard_of, const void *d_rows,
                         size_t n, uint32_t max_steps, void *d_read_row, void *d_ordinal, void *d_offset, unsigned long long *d_work2,
                         int num_cus, hipStream_t stream, const void *d_n) {
    if (n == 0 || nshards == 0) return hipSuccess;
    if (!d_shard_of && nshards != 1) return hipErrorInvalidValue;
    pool_lease mem(scratch, stream, 0, 1, nshards);
    if (mem.error() != hipSuccess) return mem.error();
    // (grid: the extraction's rules -- what is resident at once and no more, every shard starting with as many
    // workgroups as any other; launch_plan.h)
    const size_t g = plan_grid(n, 64 * LC_WAVES, resident_cap(num_cus, RSB_WALK_MIN_WGS), nshards, 1);
    // entries per draw: every wave that starts on a shard draws twice or more from its list, 64 entries at the least
    const uint32_t row_chunk = plan_draw(256, 64, waves_per_shard(g, LC_WAVES, nshards), 2, n);
    hipLaunchKernelGGL(locate_wave_kernel, dim3((unsigned)g), dim3(64 * LC_WAVES), 0, stream, d_shards, nshards, (const uint32_t *)d_shard_of,
                       (const uint64_t *)d_rows, (uint64_t)n, max_steps ? max_steps : LC_DEFAULT_STEPS, (uint64_t *)d_read_row,
                       (uint64_t *)d_ordinal, (uint32_t *)d_offset, mem.pool(0, nshards), d_work2, row_chunk, (const uint64_t *)d_n);
    return hipGetLastError();
}

namespace {
thread_local uint64_t locate_last[2] = {0, 0};

#define LC_HIP(x)                                              \
    do {                                                       \
        hipError_t _e = (x);                                   \
        if (_e != hipSuccess) return fail_hip(_e, #x);         \
    } while (0)
}  // namespace

void locate_set_last_work(uint64_t walked, uint64_t steps) {
    locate_last[0] = walked;
    locate_last[1] = steps;
}

// rows in host memory through c's staging buffer, slice by slice: the launch over `d_views` (nshards of them; shard_of
// null = one shard), the answers back into the caller's arrays (each optional), work2 += the slices' counters
int locate_host_views(scratch_cache &scratch, call_ctx &c, const shard_view *d_views, uint32_t nshards, int num_cus, const uint32_t *shard_of,
                      const uint64_t *rows, size_t n, uint32_t max_steps, uint64_t *read_row, uint64_t *ordinal, uint32_t *offset,
                      uint64_t *work2) {
    hipStream_t st = c.st[0];
    const size_t SLICE = 1u << 22;
    for (size_t i0 = 0; i0 < n; i0 += SLICE) {
        const size_t m = std::min(SLICE, n - i0);
        const size_t a8 = al256(m * 8), a4 = al256(m * 4);
        const int rc = c.stage(3 * a8 + 2 * a4 + 256);
        if (rc != RSBWT_OK) return rc;
        uint8_t *d_rows = (uint8_t *)c.d_stage, *d_rr = d_rows + a8, *d_od = d_rr + a8, *d_of = d_od + a8, *d_sh = d_of + a4, *d_wk = d_sh + a4;
        LC_HIP(hipMemcpyAsync(d_rows, rows + i0, m * 8, hipMemcpyHostToDevice, st));
        if (shard_of) LC_HIP(hipMemcpyAsync(d_sh, shard_of + i0, m * 4, hipMemcpyHostToDevice, st));
        LC_HIP(hipMemsetAsync(d_wk, 0, 16, st));
        const hipError_t e = launch_locate(scratch, d_views, nshards, shard_of ? d_sh : nullptr, d_rows, m, max_steps, read_row ? d_rr : nullptr,
                                           ordinal ? d_od : nullptr, offset ? d_of : nullptr, (unsigned long long *)d_wk, num_cus, st);
        if (e != hipSuccess) return fail_hip(e, "locate kernel launch");
        unsigned long long wk[2] = {0, 0};
        if (read_row) LC_HIP(hipMemcpyAsync(read_row + i0, d_rr, m * 8, hipMemcpyDeviceToHost, st));
        if (ordinal) LC_HIP(hipMemcpyAsync(ordinal + i0, d_od, m * 8, hipMemcpyDeviceToHost, st));
        if (offset) LC_HIP(hipMemcpyAsync(offset + i0, d_of, m * 4, hipMemcpyDeviceToHost, st));
        LC_HIP(hipMemcpyAsync(wk, d_wk, 16, hipMemcpyDeviceToHost, st));
        LC_HIP(hipStreamSynchronize(st));
        if (work2) {
            work2[0] += wk[0];
            work2[1] += wk[1];
        }
    }
    return RSBWT_OK;
}

}  // namespace rsb

// ---- C-ABI ------------------------------------------------------------------------------------------------------
extern "C" {

int rsbwt_locate(rsbwt_t *h, const uint64_t *rows, size_t n, uint32_t max_steps, uint64_t *read_row, uint64_t *ordinal, uint32_t *offset) {
    return rsb::guarded("rsbwt_locate", [&]() -> int {
        rsb::locate_set_last_work(0, 0);
        if (!h) return rsb::fail(RSBWT_EINVAL, "null handle");
        if (!read_row && !ordinal && !offset) return rsb::fail(RSBWT_EINVAL, "null argument: no output array");
        if (n == 0) return RSBWT_OK;
        if (!rows) return rsb::fail(RSBWT_EINVAL, "null argument");
        if (h->view.n == 0) return rsb::fail(RSBWT_EINVAL, "empty index");
        int rc = rsb::use_device(h->device);
        if (rc) return rc;
        rsb::call_ctx *c = h->pool.acquire();
        if (!c) return rsb::fail(RSBWT_EHIP, "cannot create a HIP stream");
        struct release_t {
            rsbwt_t *h;
            rsb::call_ctx *c;
            ~release_t() { h->pool.release(c); }
        } release{h, c};
        uint64_t wk[2] = {0, 0};
        rc = rsb::locate_host_views(h->scratch, *c, h->d_view, 1, h->num_cus, nullptr, rows, n, max_steps, read_row, ordinal, offset, wk);
        rsb::locate_set_last_work(wk[0], wk[1]);
        return rc;
    });
}

int rsbwt_locate_dev(rsbwt_t *h, const void *d_rows, size_t n, uint32_t max_steps, void *d_read_row, void *d_ordinal, void *d_offset,
                     void *stream) {
    if (!h) return rsb::fail(RSBWT_EINVAL, "null handle");
    if (!d_read_row && !d_ordinal && !d_offset) return rsb::fail(RSBWT_EINVAL, "null argument: no output array");
    if (n == 0) return RSBWT_OK;
    if (!d_rows) return rsb::fail(RSBWT_EINVAL, "null argument");
    if (h->view.n == 0) return rsb::fail(RSBWT_EINVAL, "empty index");
    const int rc = rsb::use_device(h->device);
    if (rc) return rc;
    const hipError_t e = rsb::launch_locate(h->scratch, h->d_view, 1, nullptr, d_rows, n, max_steps, d_read_row, d_ordinal, d_offset, nullptr,
                                            h->num_cus, (hipStream_t)stream);
    return e == hipSuccess ? RSBWT_OK : rsb::fail_hip(e, "locate kernel launch");
}

void rsbwt_locate_last_work(uint64_t *work2) {
    if (!work2) return;
    work2[0] = rsb::locate_last[0];
    work2[1] = rsb::locate_last[1];
}

}  // extern "C"
