// gt_narrow.hip -- SiteMatch's candidate legs: find_gt_reads' narrowing search (src/service/service.cpp:507-711) on
// the GPU (gfx950), and the span filter over the rows of the legs it leaves.
//
// find_gt_reads takes tile i of a query (w[s0:e0), s0 = (skip + 1) i, e0 = s0 + k) and, while the tile's interval holds
// more than max_interval_size rows, lengthens the string one symbol at a time and calls findInterval again on the longer
// string (:523-565, :594-635, :662-693) -- a loop of whole searches.  Here one lane owns one (query, tile, leg, shard)
// and runs that loop to its end:
//   * the tile's own search comes first (every leg needs it: a tile at or under the limit has ONE leg, the tile);
//   * growth to the LEFT (a--) is one more LF step from the interval in hand: findInterval of the longer string takes
//     the same steps and then this one;
//   * growth to the RIGHT (b++) changes the symbol the search starts from, so it is a fresh search of w[a:b) -- from
//     the shard's k-mer table where the string has T symbols or more, else from initInterval;
//   * a search ends the way findInterval does (query.cpp:24-41): at the first empty interval after an update, or with
//     its last symbol; a string holding a symbol outside ACGT is the empty (1, 0) of the C-ABI (rsbwt.h);
//   * the leg ends at the first width <= M at or after its mandatory first step; a leg that would need a < 0 or
//     b > L has no answer (the reference loops forever or throws there).
// The lanes of a wave share one shard (blockIdx.y), fetch one window line per lane and pass through LDS (wave_lines.h)
// and rank the symbol off the staged line (rank_device.h, rank24); a position past its line's own pieces (spill chunk,
// far line) goes through the scalar reader (line_format.h, view_occ), as read_lookup.hip's count does.
//
// gt_filter_kernel then takes the rows of the legs (interval_rows.hip makes them, locate.hip walks them), applies
// the span filter of :534-543 / :604-613 where the walk's offset decides it -- RIGHT rows for good, COVERING rows are all
// kept, LEFT rows are kept unless no read could span them (their test needs the read's length: sets.hip) -- and compacts:
// only the kept rows' records are written, and only those are copied to the host.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "line_format.h"
#include "rank_device.h"
#include "wave_lines.h"

namespace rsb {

namespace {

__device__ __forceinline__ uint32_t gt_rank(uint32_t ch) {  // A..T -> 1..4, anything else 0
    return ch == 'A' ? 1u : ch == 'C' ? 2u : ch == 'G' ? 3u : ch == 'T' ? 4u : 0u;
}

// Occ of symbol b among the first o symbols (1 <= o <= span) of a staged window line's own pieces, plus what the
// header counts before the window: whole quarters from the header, an odd quarter's predecessor 4 runs per v_dot4,
// the quarter holding the position by rank24 (wave_lines.h, staged_dollars, for a base)
__device__ __forceinline__ uint64_t gt_staged_occ(const staged_line &L, const line_head &h, uint32_t o, uint32_t b) {
    const sym_tab tab = make_sym_tab(b);
    const uint32_t cq = (o > h.s1 ? 1u : 0u) + (o > h.s2 ? 1u : 0u) + (o > h.s3 ? 1u : 0u);
    const uint32_t start = cq == 0u ? 0u : cq == 1u ? h.s1 : cq == 2u ? h.s2 : h.s3;
    uint64_t d = read_count(L, b);
    if (cq >= 2u) d += read_half(L, b);
    if (cq & 1u) d += matched24(L, HDR_DWORDS + 6u * (cq & 2u), tab);
    uint32_t r6[6];
    load24(L, HDR_DWORDS + 6u * cq, r6);
    return d + rank24(r6, tab, b, o - start);
}

// where a tile lies: find_gt_reads' three branches (:522, :593, :661) on 0-based half-open [s0, e0)
enum : uint32_t { GT_LEFT = 0, GT_RIGHT = 1, GT_COVER = 2 };
__device__ __forceinline__ uint32_t gt_kind(uint64_t pos, uint32_t s0, uint32_t e0) {
    return pos > (uint64_t)e0 ? GT_LEFT : (pos <= (uint64_t)s0 ? GT_RIGHT : GT_COVER);
}

__global__ void __launch_bounds__(64 * WG_WAVES)
gt_narrow_kernel(const shard_view *__restrict__ shards, const gt_batch bt, gt_leg *__restrict__ legs, ulonglong2 *__restrict__ pairs,
                 unsigned long long *__restrict__ work) {
    __shared__ uint4 s_stage[WG_WAVES][64 * SLOT_U4];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint4 *stage = s_stage[wave];
    const uint32_t stage_lds = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)(lds_void_ptr)stage);
    const staged_line L = {own_stage_row(stage, lane), lane & 7u};
    const uint32_t sid = blockIdx.y;
    const shard_view *sv = shards + sid;
    const char *lines_bytes = reinterpret_cast<const char *>(sv->lines);
    const uint32_t S = sv->sp.S, nlines = (uint32_t)sv->nlines;
    const double inv = sv->sp.inv;
    const uint64_t n = sv->n;
    const uint32_t T = sv->ktab != nullptr && sv->ktab_depth >= 2u ? sv->ktab_depth : 0u;

    const size_t item = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool mine = item < bt.nitems;
    const uint32_t leg = (uint32_t)(item & 1u);
    uint64_t base = 0, pos = 0;
    uint32_t Lq = 0, s0 = 0, e0 = 0;
    if (mine) {
        const size_t slot = item >> 1;
        const uint32_t q = bt.slot_query[slot];
        base = bt.q_off[q];
        Lq = bt.q_len[q];
        pos = bt.q_pos[q];
        s0 = bt.step * bt.slot_tile[slot];
        e0 = s0 + bt.k;
    }
    const uint32_t kind = gt_kind(pos, s0, e0);
    const uint8_t *text = reinterpret_cast<const uint8_t *>(bt.text) + base;
    const uint32_t *nprev = bt.nprev + base;

    // the lane's search: w[a:b), (lo, hi) = the interval of w[j+1:b), j the next symbol to take
    uint32_t a = s0, b = e0, c = 0, phase = 0, stage_grow = 0;
    int32_t j = 0;
    uint64_t lo = 1, hi = 0, occ_lo = 0;
    bool active = mine, need_start = true, complete = false, fresh = false, pending = false;
    gt_leg out = {0xFFFFFFFFu, 0xFFFFFFFFu, ~0ull, ~0ull, 0u, 0u};  // no leg
    unsigned long long steps = 0;

    for (;;) {
        // ---- everything a lane can do without a rank: start a search, end one, judge the width, grow the string
        while (active && !pending) {
            if (need_start) {
                need_start = false;
                complete = false;
                if (nprev[b - 1u] > a) {  // a symbol outside ACGT in w[a:b)
                    lo = 1;
                    hi = 0;
                    complete = true;
                } else {
                    bool tabulated = false;
                    if (T != 0u && b - a >= T) {
                        uint64_t code = 0;
                        for (uint32_t i = 0; i < T; ++i) code |= (uint64_t)(gt_rank(text[b - T + i]) - 1u) << (2u * i);
                        const uint64_t e = ktab_entry(sv->ktab, sv->ktab_fmt, T, sv->ktab_stride, code);
                        const uint32_t width = (uint32_t)(e >> COUNT_BITS);
                        if (width != KTAB_WIDE && (e & COUNT_MASK) + width <= n) {  // (search_lines.hip, start_record's rule)
                            lo = e & COUNT_MASK;
                            hi = lo + width - 1ull;
                            j = (int32_t)(b - T) - 1;
                            fresh = false;
                            tabulated = true;
                        }
                    }
                    if (!tabulated) {  // initInterval, query.cpp:18-21: not looked at before its first update (:33-37)
                        const uint32_t cb = gt_rank(text[b - 1u]);
                        lo = sv->C[cb];
                        hi = lo + sv->total[cb] - 1ull;
                        j = (int32_t)b - 2;
                        fresh = true;
                    }
                }
            }
            if (!complete) {
                if ((!fresh && lo > hi) || j < (int32_t)a) {
                    complete = true;
                } else if (lo == 0ull && hi == ~0ull) {
                    // the reference's (0, 2^64 - 1): a symbol that is absent (initInterval), or an A that no row of the
                    // interval sees before it, on a shard where no '$' row lies before the rows that begin with A
                    // (C[A] == 0).  query.cpp:35 does not end the search there (0 > 2^64 - 1 is false) and the next
                    // updateInterval takes getOcc(c, -1) = 0 on both sides: (C[c], C[c] - 1), an LF step that reads no
                    // position -- the search ends on it, or stays in the corner where C[c] == 0
                    c = gt_rank(text[j]);
                    lo = sv->C[c];
                    hi = lo - 1ull;
                    --j;
                    fresh = false;
                    steps += stage_grow;
                    continue;
                } else {
                    c = gt_rank(text[j]);
                    occ_lo = 0;
                    phase = lo == 0ull ? 1u : 0u;  // Occ(., -1) = 0
                    pending = true;
                    break;
                }
            }
            // ---- w[a:b) is searched: the tile decides how many legs there are, a leg ends at the first width <= M
            const uint64_t W = (lo <= hi && hi < n) ? hi - lo + 1ull : 0ull;
            bool grow = false;
            if (stage_grow == 0u) {
                if (W <= bt.M) {
                    if (leg == 0u) out = gt_leg{a, b, lo, hi, 0u, 0u};
                    active = false;
                } else {
                    stage_grow = 1u;
                    // leg 2 of a LEFT tile starts at s0 - 1, leg 2 of a RIGHT tile at e0 + 1 (:546, :616)
                    const bool exists = leg == 0u || kind == GT_COVER || (kind == GT_LEFT ? s0 > 0u : e0 < Lq);
                    if (exists) grow = true;
                    else active = false;
                }
            } else if (W <= bt.M) {
                out = gt_leg{a, b, lo, hi, leg + 1u, 0u};
                active = false;
            } else {
                grow = true;
            }
            if (grow) {
                const bool left = kind == GT_LEFT ? (leg == 1u && a > 0u) : kind == GT_RIGHT ? (leg == 0u || b >= Lq) : leg == 1u;
                if (left) {
                    if (a == 0u) {
                        active = false;  // would need a < 0
                        out.reserved = 1u;
                    } else {
                        a -= 1u;  // j == a: one more LF step from the interval in hand
                        complete = false;
                        fresh = false;
                        if (gt_rank(text[a]) == 0u) {
                            lo = 1;
                            hi = 0;
                            complete = true;
                        }
                    }
                } else if (b >= Lq) {
                    active = false;  // would need b > L
                    out.reserved = 1u;
                } else {
                    b += 1u;
                    need_start = true;
                }
            }
        }
        if (__builtin_amdgcn_ballot_w64(active) == 0ull) break;
        // ---- one rank per lane and pass: Occ(c, lo - 1), then Occ(c, hi) (updateInterval, query.cpp:11-15)
        uint64_t p = 0;
        uint32_t w = 0, o = 0, want = ~0u;
        bool bad = false;
        if (pending) {
            p = phase ? hi : lo - 1ull;
            if (p >= n) {
                // a defensive end, unreachable: a search is ranked only while lo <= hi (or before initInterval's first
                // update, where hi = C[c] + total[c] - 1 < n unless it is the corner), every interval an update or a
                // table entry of this shard gives has hi < n or is (0, 2^64 - 1), the corner is stepped above without a
                // rank, and lo == 0 takes Occ(., -1) = 0 without one.  Nothing is read at p; the leg has no answer
                bad = true;
            } else {
                uint32_t pin;
                w = fast_window(p, S, inv, pin);
                o = pin + 1u;
                want = w + (w >> GROUP_SHIFT);
                if (want >= nlines) want = 0;
            }
        }
        glds_fetch(lines_bytes, want, lane, stage_lds);  // (every lane takes part: lanes with nothing to rank ask for nothing)
        glds_wait();
        if (pending) {
            if (bad) {
                active = false;
                pending = false;
                out.reserved = 1u;
            } else {
                const line_head h = read_head(L);
                const uint64_t occ = o <= h.span ? gt_staged_occ(L, h, o, c) : view_occ(*sv, c, p);
                if (phase == 0u) {
                    occ_lo = occ;
                    phase = 1u;
                } else {
                    const uint64_t pc = sv->C[c];
                    lo = pc + occ_lo;
                    hi = pc + occ - 1ull;
                    --j;
                    fresh = false;
                    pending = false;
                    steps += stage_grow;
                }
            }
        }
    }
    if (mine) {
        const size_t at = (size_t)sid * bt.nitems + item;
        legs[at] = out;
        pairs[at] = out.a == 0xFFFFFFFFu ? make_ulonglong2(~0ull, ~0ull) : make_ulonglong2(out.lower, out.upper);
    }
    if (work && steps) atomicAdd(&work[0], steps);
}

// Row t of the legs' rows (interval_rows.hip's order: item by item, shard ascending, SA row ascending): its item by
// binary search in first[], its leg's record, the span filter as far as the walk's offset decides it, and the
// COMPACTION: a wave counts the rows it keeps, claims that many records from counters[0] with one atomic and every
// kept row writes its record -- so only kept rows ever leave the device (in no particular order: the host sorts by
// read).  counters[1] += rows whose walk did not end on a '$' row (locate's UINT32_MAX offset).
// REC = gt_site_row: the record also carries the row's ordinal (launch_locate's d_ordinal) -- site_counts.hip's input.
__device__ __forceinline__ void gt_filter_record(gt_kept_row *out, uint32_t item, uint32_t shard, uint32_t off, uint32_t pending, uint64_t read_row,
                                                 const uint64_t *, uint64_t) {
    *out = gt_kept_row{item, shard, off, pending, read_row};
}
__device__ __forceinline__ void gt_filter_record(gt_site_row *out, uint32_t item, uint32_t shard, uint32_t off, uint32_t pending, uint64_t read_row,
                                                 const uint64_t *ordinal, uint64_t t) {
    *out = gt_site_row{item, shard, off, pending, read_row, ordinal[t]};
}

template <class REC>
__global__ void __launch_bounds__(256)
gt_filter_kernel(const gt_batch bt, const gt_leg *__restrict__ legs, const uint64_t *__restrict__ first, const uint32_t *__restrict__ shard_of,
                 const uint32_t *__restrict__ offset, const uint64_t *__restrict__ read_row, const uint64_t *__restrict__ ordinal, uint64_t total,
                 REC *__restrict__ out, unsigned long long *__restrict__ counters) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t f = 0, item32 = 0, shard = 0, off = 0;
    bool lost = false;
    if (t < total) {
        size_t lo = 0, hi = bt.nitems;
        while (hi - lo > 1) {
            const size_t mid = lo + ((hi - lo) >> 1);
            if (first[mid] <= t) lo = mid;
            else hi = mid;
        }
        const size_t item = lo, slot = item >> 1;
        shard = shard_of[t];
        const gt_leg rec = legs[(size_t)shard * bt.nitems + item];
        const uint64_t pos = bt.q_pos[bt.slot_query[slot]];
        const uint32_t s0 = bt.step * bt.slot_tile[slot];
        const uint32_t kind = gt_kind(pos, s0, s0 + bt.k);
        off = offset[t];
        item32 = (uint32_t)item;
        if (rec.a != 0xFFFFFFFFu) {
            if (off == 0xFFFFFFFFu) {
                lost = true;
            } else if (kind == GT_COVER) {
                f = 1;
            } else if (kind == GT_RIGHT) {  // start - pos > prefix_size + indel_allowance: dropped (:608), unsigned as there
                f = ((uint64_t)rec.a + 1ull) - pos <= (uint64_t)off + 4ull ? 1u : 0u;
            } else {  // pos - end > postfix_size - k + indel_allowance (:538): no read is longer than the extraction allows
                f = pos - (uint64_t)rec.b <= 65536ull + 4ull ? 2u : 0u;
            }
        }
    }
    // (every lane of the wave is here: the block is a whole number of waves and nothing above returns)
    const uint64_t mask = __builtin_amdgcn_ballot_w64(f != 0u), lost_mask = __builtin_amdgcn_ballot_w64(lost);
    if (mask != 0ull) {
        unsigned long long base = 0;
        if (lane == 0u) base = atomicAdd(&counters[0], (unsigned long long)__builtin_popcountll(mask));
        base = ((unsigned long long)__builtin_amdgcn_readfirstlane((uint32_t)(base >> 32)) << 32) | __builtin_amdgcn_readfirstlane((uint32_t)base);
        if (f != 0u) {
            const uint64_t at = base + (uint64_t)__builtin_popcountll(mask & ((1ull << lane) - 1ull));
            if (at < total) gt_filter_record(&out[at], item32, shard, off, f == 2u ? 1u : 0u, read_row[t], ordinal, t);
        }
    }
    if (lost_mask != 0ull && lane == 0u) atomicAdd(&counters[1], (unsigned long long)__builtin_popcountll(lost_mask));
}

}  // namespace

hipError_t launch_gt_narrow(const shard_view *d_shards, uint32_t nshards, const gt_batch &bt, void *d_legs, void *d_pairs,
                            unsigned long long *d_work, hipStream_t stream) {
    if (bt.nitems == 0 || nshards == 0) return hipSuccess;
    if (nshards > 65535u) return hipErrorInvalidValue;  // (the shard is the grid's y)
    const dim3 grid((unsigned)((bt.nitems + 64 * WG_WAVES - 1) / (64 * WG_WAVES)), nshards);
    hipLaunchKernelGGL(gt_narrow_kernel, grid, dim3(64 * WG_WAVES), 0, stream, d_shards, bt, (gt_leg *)d_legs, (ulonglong2 *)d_pairs, d_work);
    return hipGetLastError();
}

hipError_t launch_gt_filter(const gt_batch &bt, const void *d_legs, const void *d_first, const void *d_shard_of, const void *d_offset,
                            const void *d_read_row, uint64_t total, void *d_kept_rows, unsigned long long *d_counters, hipStream_t stream,
                            const void *d_ordinal) {
    if (total == 0) return hipSuccess;
    const dim3 grid((unsigned)((total + 255) / 256));
    if (d_ordinal)
        hipLaunchKernelGGL(gt_filter_kernel<gt_site_row>, grid, dim3(256), 0, stream, bt, (const gt_leg *)d_legs, (const uint64_t *)d_first,
                           (const uint32_t *)d_shard_of, (const uint32_t *)d_offset, (const uint64_t *)d_read_row, (const uint64_t *)d_ordinal, total,
                           (gt_site_row *)d_kept_rows, d_counters);
    else
        hipLaunchKernelGGL(gt_filter_kernel<gt_kept_row>, grid, dim3(256), 0, stream, bt, (const gt_leg *)d_legs, (const uint64_t *)d_first,
                           (const uint32_t *)d_shard_of, (const uint32_t *)d_offset, (const uint64_t *)d_read_row, (const uint64_t *)nullptr, total,
                           (gt_kept_row *)d_kept_rows, d_counters);
    return hipGetLastError();
}

}  // namespace rsb
