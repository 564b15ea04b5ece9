// walk_search.h -- the candidate search of the k-mer graph kernels (walk.hip: walk_kernel, unitig_kernel, extension_kernel;
// paths.hip: paths_kernel), with what they share around it: a lane's candidate over its seed's context ring, the counters a
// lane keeps of its own work, the load of the rings from a batch and the sum of the counters at the end.  walk.hip's header
// says how the lanes of a wave are mapped and what a pass of the search does.
#ifndef RSBWT_WALK_SEARCH_H
#define RSBWT_WALK_SEARCH_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "line_format.h"
#include "match_lanes.h"
#include "rank_device.h"
#include "wave_lines.h"

namespace rsb {

namespace {

constexpr uint32_t WALK_SEEDS = 8;   // seeds of a wave's lanes
constexpr uint32_t WALK_RING = 256;  // bytes of a seed's context ring (ctx <= 255)

// what a lane counts of its own work, summed per wave at the end
struct walk_tally {
    uint32_t searches = 0, steps = 0, passes = 0, tab_starts = 0;
};

// A lane's candidate: ctx + 1 ranks (1..4).  The context is ring[(head + i) % ctx], i = 0 .. ctx - 1 in the sequence's
// own order; `base` goes behind it (a walk to the right) or in front of it (to the left); the reverse strand reads the
// complement from the other end.
struct walk_cand {
    const uint8_t *ring;
    uint32_t head, ctx, base;
    bool left, rev;
    __device__ __forceinline__ uint32_t fwd(uint32_t i) const {
        if (left) {
            if (i == 0u) return base;
            i -= 1u;
        } else if (i == ctx) {
            return base;
        }
        uint32_t at = head + i;
        if (at >= ctx) at -= ctx;
        return ring[at];
    }
    __device__ __forceinline__ uint32_t at(uint32_t i) const { return rev ? 5u - fwd(ctx - i) : fwd(i); }
};

// The rows of findInterval(candidate) in shard *sv (0 when `live` is false), for the 64 candidates of a wave at once.
// Every lane of the wave must be in the call.  lower (optional): the interval's first row where the rows are not 0.
__device__ __forceinline__ uint64_t walk_search(const shard_view *sv, bool live, const walk_cand &cd, uint32_t lane, uint32_t stage_lds,
                                                const staged_line &L, walk_tally &tally, uint64_t *lower = nullptr) {
    const char *lines_bytes = reinterpret_cast<const char *>(sv->lines);
    const uint32_t S = sv->sp.S, nlines = (uint32_t)sv->nlines;
    const double inv = sv->sp.inv;
    const uint64_t n = sv->n;
    const uint32_t T = sv->ktab != nullptr && sv->ktab_depth >= 2u ? sv->ktab_depth : 0u;
    const uint64_t C1 = sv->C[1], C2 = sv->C[2], C3 = sv->C[3], C4 = sv->C[4];
    const uint32_t K = cd.ctx + 1u;

    // the candidate's suffix of j symbols has interval (lo, hi)
    uint64_t lo = 1, hi = 0, occ_lo = 0, rows = 0;
    uint32_t j = 0, c = 0, phase = 0;
    bool active = false, pending = false;
    if (live) {
        ++tally.searches;
        bool tabulated = false;
        if (T != 0u && K >= T) {
            uint64_t code = 0;
            for (uint32_t i = 0; i < T; ++i) code |= (uint64_t)((cd.at(K - T + i) - 1u) & 3u) << (2u * i);
            const uint64_t en = ktab_entry(sv->ktab, sv->ktab_fmt, T, sv->ktab_stride, code);
            const uint32_t width = (uint32_t)(en >> COUNT_BITS);
            if (width != KTAB_WIDE && (en & COUNT_MASK) + width <= n && width != 0u) {  // (search_lines.hip, start_record's rule)
                lo = en & COUNT_MASK;
                hi = lo + width - 1ull;
                j = T;
                tabulated = true;
                ++tally.tab_starts;
            }
        }
        if (!tabulated) {  // initInterval (query.cpp:18-21) of the last symbol
            const uint32_t cb = cd.at(K - 1u);
            const uint64_t a = sv->C[cb], z = a + sv->total[cb] - 1ull;
            if (a <= z && z < n) {
                lo = a;
                hi = z;
                j = 1u;
            }
        }
        active = j != 0u;
    }

    for (;;) {  // (2 * ctx + 1 rounds at the most: every pass of a lane ranks a position or ends the lane)
        if (active && !pending) {
            if (j >= K) {
                rows = hi - lo + 1ull;  // the whole candidate: its interval is proper
                if (lower) *lower = lo;
                active = false;
            } else {
                c = cd.at(K - 1u - j);
                occ_lo = 0;
                phase = lo == 0ull ? 1u : 0u;  // Occ(., -1) = 0
                pending = true;
            }
        }
        if (__builtin_amdgcn_ballot_w64(active) == 0ull) break;
        // ---- one line per lane and pass: lo - 1's, and hi off the same line where it can be; else hi's in a pass of its own
        uint64_t p = 0;
        uint32_t o = 0, want = ~0u;
        bool bad = false;
        if (pending) {
            p = phase ? hi : lo - 1ull;
            if (p >= n) {
                bad = true;  // (never for an interval of this shard's rows)
            } else {
                uint32_t pin;
                const uint32_t w = fast_window(p, S, inv, pin);
                o = pin + 1u;
                want = w + (w >> GROUP_SHIFT);
                if (want >= nlines) want = 0;
            }
        }
        glds_fetch(lines_bytes, want, lane, stage_lds);  // (every lane takes part: lanes with nothing to rank ask for nothing)
        glds_wait();
        if (pending) {
            if (bad) {
                active = false;  // the search ends where it stands, with no rows
                pending = false;
            } else {
                ++tally.passes;
                const sym_tab tab = make_sym_tab(c);
                const line_head h = read_head(L);
                const bool own = o <= h.span;
                const uint64_t at_p = own ? ms_staged_occ(L, h, o, c, tab) : view_occ(*sv, c, p);
                uint64_t at_hi = at_p;
                bool done = phase != 0u;
                if (!done) {
                    occ_lo = at_p;
                    const uint64_t oh = (uint64_t)o + (hi - p);  // hi's offset in lo - 1's window, if it lies there
                    if (own && hi >= p && oh <= (uint64_t)h.span) {
                        at_hi = ms_staged_occ(L, h, (uint32_t)oh, c, tab);
                        done = true;
                    } else {
                        phase = 1u;
                    }
                }
                if (done) {
                    pending = false;
                    ++tally.steps;
                    const uint64_t pc = c == 1u ? C1 : c == 2u ? C2 : c == 3u ? C3 : C4;
                    const uint64_t nlo = pc + occ_lo, nhi = pc + at_hi - 1ull;
                    if (nlo <= nhi && nhi < n) {
                        lo = nlo;
                        hi = nhi;
                        ++j;
                    } else {
                        active = false;  // the step that emptied the search: nothing past it is looked at
                    }
                }
            }
        }
    }
    return rows;
}

// The contexts of seeds first_q .. first_q + 7 into their rings as ranks, by `nthreads` threads (tid = 0 .. nthreads - 1);
// bad[s] = 1 where a context holds a symbol outside ACGT.  bad[] must be zero and a barrier passed before the call; a
// barrier after it makes rings and flags visible.
__device__ __forceinline__ uint64_t walk_seed_len(const walk_batch &bt, size_t q) {
    if (q >= bt.Q) return 0;
    const uint64_t b = bt.off[q], e = bt.off[q + 1];
    // (offsets that do not fit the batch must not send a lane outside the text)
    return (b <= e && e <= (uint64_t)bt.N) ? e - b : 0ull;
}
__device__ __forceinline__ void walk_load_rings(const walk_batch &bt, size_t first_q, uint8_t (*ring)[WALK_RING], uint32_t *bad, uint32_t tid,
                                                uint32_t nthreads) {
    const uint8_t *text = reinterpret_cast<const uint8_t *>(bt.text);
    for (uint32_t s = 0; s < WALK_SEEDS; ++s) {
        const size_t q = first_q + s;
        const uint64_t Lq = walk_seed_len(bt, q);
        if (Lq < bt.ctx) continue;
        const uint64_t from = (bt.flags & RSBWT_WALK_LEFT) ? bt.off[q] : bt.off[q + 1] - bt.ctx;
        for (uint32_t i = tid; i < bt.ctx; i += nthreads) {
            const uint32_t r = ms_rank(text[from + i]);
            ring[s][i] = (uint8_t)r;
            if (r == 0u) bad[s] = 1u;
        }
    }
}

__device__ __forceinline__ void walk_add_work(unsigned long long *work, uint32_t lane, const walk_tally &t, uint32_t appended) {
    if (!work) return;
    const unsigned long long s1 = ms_wave_sum(appended), s2 = ms_wave_sum(t.searches), s3 = ms_wave_sum(t.steps), s4 = ms_wave_sum(t.passes),
                             s5 = ms_wave_sum(t.tab_starts);
    if (lane == 0u) {
        if (s1) atomicAdd(&work[1], s1);
        if (s2) atomicAdd(&work[2], s2);
        if (s3) atomicAdd(&work[3], s3);
        if (s4) atomicAdd(&work[4], s4);
        if (s5) atomicAdd(&work[5], s5);
    }
}

}  // namespace

}  // namespace rsb
#endif
