// overlaps.hip -- suffix-prefix overlaps on the GPU (gfx950): for every suffix x of every query of a batch and every
// shard, how many reads BEGIN with x and which ones (include/rsbwt.h: the definition).  In a multi-string BWT a row of
// findInterval(x) holds '$' exactly when a read begins with x there (read_lookup.hip), so
//
//     count(x)   = Occ('$', upper) - Occ('$', lower - 1)        (Occ(., -1) = 0)
//     ordinal(x) = Occ('$', lower - 1)                          the first of `count` consecutive rsbwt_locate ordinals
//
// and ONE backward search of the query from its right end passes through the interval of every suffix.  The two
// positions whose '$' rank is wanted at a depth are the two positions the next LF step ranks its own symbol at, so the
// whole profile costs one search: the '$' rank is taken off the line (or lines) the step has staged anyway.
//
// One lane owns one (query, shard), in the pattern of match_stats.hip, whose helpers (match_lanes.h) it shares: the shard
// is blockIdx.y, the lanes of a wave take consecutive queries and pass through the wave's LDS stage.
//   * START: the shard's k-mer table entry of the query's last T symbols -- only when T >= 2, min_overlap >= T and
//     min(L, limit) >= T, so that no depth that could be reported is skipped -- taken by start_record's rule
//     (search_lines.hip: not KTAB_WIDE, lower + width <= n) when it holds a row; a refused entry starts over from
//     initInterval of the last symbol (query.cpp:18-21).
//   * PASS: at depth j the lane wants Occ(c, .) for the next symbol c to the left (when a step follows) and, when
//     j >= min_overlap, Occ('$', .), both at lo - 1 and at hi.  Both positions come off ONE fetched line when hi lies in
//     lo - 1's window among that line's own pieces, else one pass per position; lo == 0 fetches nothing for that side; a
//     position past its line's own pieces goes through the scalar reader (view_occ's walk, both symbols in one).  The
//     symbol of the step after this one is read one step ahead, so that it travels with the line.
//   * '$' ALONE: a pass is spent on '$' only where no LF step follows a reported depth: at depth min(L, limit), or when
//     the next symbol to the left is not ACGT.
//   * END: the first improper interval, the limit, or a symbol outside ACGT; nothing past the step that emptied the item
//     is looked at.
//   * RESULT: {ordinal, count} at position off[q + 1] - j for every reported depth j with count > 0 (and {lower, upper}
//     beside it when the records are wanted); every other entry is zeroed by a memset in front of the launch.  No atomics
//     but the work counters', summed per wave.
// overlap_records_kernel compacts the entries with count > 0 as match_smem_kernel does: a ballot, a popcount and one
// atomic per wave; only those records leave the device.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "capi_internal.h"
#include "kernels.h"
#include "line_format.h"
#include "match_lanes.h"
#include "rank_device.h"
#include "wave_lines.h"

namespace rsb {

namespace {

// what one position of a staged line answers: Occ(c, p) when c != 0, Occ('$', p) when dollars are wanted (0 otherwise)
struct ov_ranks {
    uint64_t occ, dol;
};

// view_occ (line_format.h: the scalar reader, for a position past its line's own pieces) for the step's symbol and for '$'
// in ONE walk of the window
__device__ __forceinline__ ov_ranks ov_view_ranks(const shard_view &v, uint32_t c, bool want_d, uint64_t p) {
    const uint64_t w = window_of(v.sp, p);
    uint32_t rem = (uint32_t)(p - w * v.sp.S) + 1u, in_c = 0, in_d = 0;
    walk_window(v, w, [&](uint32_t sym, uint32_t len) {
        const uint32_t take = len < rem ? len : rem;
        if (sym == c) in_c += take;
        if (sym == 0u) in_d += take;
        rem -= take;
        return rem == 0u;
    });
    ov_ranks r = {0, 0};
    if (c != 0u) r.occ = count_before_window(v, w, c) + in_c;
    if (want_d) r.dol = count_before_window(v, w, 0u) + in_d;
    return r;
}

__global__ void __launch_bounds__(64 * WG_WAVES)
overlap_kernel(const shard_view *__restrict__ shards, const overlap_batch bt, ulonglong2 *__restrict__ pairs, ulonglong2 *__restrict__ ivals,
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
    const uint64_t C1 = sv->C[1], C2 = sv->C[2], C3 = sv->C[3], C4 = sv->C[4];  // (uniform: picked by compares, no load per step)
    const uint32_t mo = bt.min_overlap;

    const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint8_t *text = reinterpret_cast<const uint8_t *>(bt.text);

    // the lane's suffix: text[e-j .. e) with interval (lo, hi); limit = min(L, max_overlap)
    uint64_t e = 0;
    uint32_t j = 0, limit = 0, c = 0, phase = 0, sym = 0;  // sym = text[e - j - 1], read one step ahead
    uint64_t lo = 1, hi = 0, occ_lo = 0, dol_lo = 0;
    bool active = false, pending = false, want_d = false;
    uint32_t steps = 0, passes = 0, tab_starts = 0, dollar_only = 0, entries = 0;
    if (q < bt.Q) {
        const uint64_t b = bt.off[q];
        e = bt.off[q + 1];
        // (offsets that do not fit the batch must not send a lane outside the text or the outputs)
        const uint64_t Lq = (b <= e && e <= (uint64_t)bt.N && e - b <= 0x7FFFFFFFull) ? e - b : 0ull;
        limit = (uint32_t)(bt.max_overlap != 0u && Lq > bt.max_overlap ? bt.max_overlap : Lq);
        if (limit != 0u) {
            bool tabulated = false;
            if (T != 0u && mo >= T && limit >= T) {
                uint64_t code = 0;
                bool acgt = true;
                for (uint32_t i = 0; i < T; ++i) {
                    const uint32_t r = ms_rank(text[e - T + i]);
                    acgt = acgt && r != 0u;
                    code |= (uint64_t)((r - 1u) & 3u) << (2u * i);
                }
                if (acgt) {
                    const uint64_t en = ktab_entry(sv->ktab, sv->ktab_fmt, T, sv->ktab_stride, code);
                    const uint32_t width = (uint32_t)(en >> COUNT_BITS);
                    if (width != KTAB_WIDE && (en & COUNT_MASK) + width <= n && width != 0u) {  // (search_lines.hip, start_record's rule)
                        lo = en & COUNT_MASK;
                        hi = lo + width - 1ull;
                        j = T;
                        tabulated = true;
                        tab_starts = 1u;
                    }
                }
            }
            if (!tabulated) {  // initInterval (query.cpp:18-21) of the last symbol
                const uint32_t cb = ms_rank(text[e - 1ull]);
                if (cb != 0u) {
                    const uint64_t a = sv->C[cb], z = a + sv->total[cb] - 1ull;
                    if (a <= z && z < n) {
                        lo = a;
                        hi = z;
                        j = 1u;
                    }
                }
            }
            active = j != 0u;
            if (active && j < limit) sym = text[e - j - 1ull];
        }
    }

    for (;;) {
        // ---- what needs no rank: the item ends where neither a step nor a reported depth asks for one
        if (active && !pending) {
            want_d = j >= mo;
            c = j < limit ? ms_rank(sym) : 0u;
            if (c == 0u && !want_d) {
                active = false;
            } else {
                occ_lo = 0;
                dol_lo = 0;
                phase = lo == 0ull ? 1u : 0u;  // Occ(., -1) = 0
                pending = true;
            }
        }
        if (__builtin_amdgcn_ballot_w64(active) == 0ull) break;
        // ---- one line per lane and pass: lo - 1's, and hi off the same line where it can be; else hi's in a pass of its own
        uint64_t p = 0;
        uint32_t o = 0, w = 0, want = ~0u;
        bool bad = false;
        if (pending) {
            p = phase ? hi : lo - 1ull;
            if (p >= n) {
                bad = true;  // (never for an interval of this shard's rows)
            } else {
                uint32_t pin;
                w = fast_window(p, S, inv, pin);
                o = pin + 1u;
                want = w + (w >> GROUP_SHIFT);
                if (want >= nlines) want = 0;
            }
        }
        // the symbol of the step after this one travels with the line: a step then waits for memory once, not twice
        uint32_t sym_next = 0;
        if (pending && c != 0u && j + 1u < limit) sym_next = text[e - j - 2ull];
        glds_fetch(lines_bytes, want, lane, stage_lds);  // (every lane takes part: lanes with nothing to rank ask for nothing)
        glds_wait();
        if (pending) {
            if (bad) {
                active = false;  // the item ends where it stands
                pending = false;
            } else {
                ++passes;
                if (c == 0u) ++dollar_only;
                const sym_tab tab = make_sym_tab(c);
                const line_head h = read_head(L);
                const bool own = o <= h.span;
                // '$' before the window = w * S - (A + C + G + T)   (line_format.h; read_lookup.hip)
                uint64_t before = 0;
                if (want_d && own) before = (uint64_t)w * S - (read_count(L, 1u) + read_count(L, 2u) + read_count(L, 3u) + read_count(L, 4u));
                auto rank_at = [&](uint32_t oo, uint64_t pp, bool in_line) -> ov_ranks {
                    if (!in_line) return ov_view_ranks(*sv, c, want_d, pp);
                    ov_ranks r = {0, 0};
                    if (c != 0u) r.occ = ms_staged_occ(L, h, oo, c, tab);
                    if (want_d) r.dol = before + staged_dollars(L, h, oo);
                    return r;
                };
                const ov_ranks at_p = rank_at(o, p, own);
                ov_ranks at_hi = at_p;
                bool done = phase != 0u;
                if (!done) {
                    occ_lo = at_p.occ;
                    dol_lo = at_p.dol;
                    const uint64_t oh = (uint64_t)o + (hi - p);  // hi's offset in lo - 1's window, if it lies there
                    if (own && hi >= p && oh <= (uint64_t)h.span) {
                        at_hi = rank_at((uint32_t)oh, hi, true);
                        done = true;
                    } else {
                        phase = 1u;
                    }
                }
                if (done) {
                    pending = false;
                    if (want_d && at_hi.dol > dol_lo) {  // reads begin with this suffix: [dol_lo, at_hi.dol)
                        const size_t at = (size_t)sid * bt.N + (size_t)(e - j);
                        pairs[at] = make_ulonglong2(dol_lo, at_hi.dol - dol_lo);
                        if (ivals) ivals[at] = make_ulonglong2(lo, hi);
                        ++entries;
                    }
                    if (c == 0u) {
                        active = false;  // the limit, or a symbol outside ACGT
                    } else {
                        ++steps;
                        const uint64_t pc = c == 1u ? C1 : c == 2u ? C2 : c == 3u ? C3 : C4;
                        const uint64_t nlo = pc + occ_lo, nhi = pc + at_hi.occ - 1ull;
                        if (nlo <= nhi && nhi < n) {
                            lo = nlo;
                            hi = nhi;
                            ++j;
                            sym = sym_next;
                        } else {
                            active = false;  // the step that emptied the item: nothing past it is looked at
                        }
                    }
                }
            }
        }
    }
    if (work) {  // (every lane of the wave is here: nothing above returns)
        const unsigned long long s0 = ms_wave_sum(steps), s1 = ms_wave_sum(passes), s2 = ms_wave_sum(tab_starts), s3 = ms_wave_sum(dollar_only),
                                 s4 = ms_wave_sum(entries);
        if (lane == 0u) {
            if (s0) atomicAdd(&work[0], s0);
            if (s1) atomicAdd(&work[1], s1);
            if (s2) atomicAdd(&work[2], s2);
            if (s3) atomicAdd(&work[3], s3);
            if (s4) atomicAdd(&work[4], s4);
        }
    }
}

// Position t of shard blockIdx.y is kept iff its count > 0; the kept positions' records are compacted: a wave counts
// them, claims that many records from *counter with one atomic and every kept lane writes its own (in no particular
// order: the host sorts).  shard = the launch's number.
__global__ void __launch_bounds__(256)
overlap_records_kernel(const overlap_batch bt, const ulonglong2 *__restrict__ pairs, const ulonglong2 *__restrict__ ivals,
                       rsbwt_overlap *__restrict__ out, uint64_t cap_records, unsigned long long *__restrict__ counter) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u, sid = blockIdx.y;
    bool keep = false;
    rsbwt_overlap rec = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (t < bt.N) {
        const size_t at = (size_t)sid * bt.N + t;
        const ulonglong2 oc = pairs[at];
        if (oc.y != 0ull) {
            keep = true;
            const size_t q = ms_query_of(bt.off, bt.Q, t);
            const ulonglong2 iv = ivals[at];
            rec = rsbwt_overlap{(uint64_t)q, sid, (uint32_t)(t - bt.off[q]), (uint32_t)(bt.off[q + 1] - t), 0u, oc.x, oc.y, iv.x, iv.y};
        }
    }
    // (every lane of the wave is here: the block is a whole number of waves and nothing above returns)
    const uint64_t mask = __builtin_amdgcn_ballot_w64(keep);
    if (mask != 0ull) {
        unsigned long long base = 0;
        if (lane == 0u) base = atomicAdd(counter, (unsigned long long)__builtin_popcountll(mask));
        base = ((unsigned long long)__builtin_amdgcn_readfirstlane((uint32_t)(base >> 32)) << 32) | __builtin_amdgcn_readfirstlane((uint32_t)base);
        if (keep) {
            const uint64_t at = base + (uint64_t)__builtin_popcountll(mask & ((1ull << lane) - 1ull));
            if (at < cap_records) out[at] = rec;
        }
    }
}

thread_local uint64_t overlap_last[6] = {0, 0, 0, 0, 0, 0};

#define OV_HIP(x)                                              \
    do {                                                       \
        hipError_t _e = (x);                                   \
        if (_e != hipSuccess) return fail_hip(_e, #x);         \
    } while (0)

}  // namespace

hipError_t launch_overlaps(const shard_view *d_shards, uint32_t nshards, const overlap_batch &bt, void *d_pairs, void *d_ivals,
                           unsigned long long *d_work, hipStream_t stream) {
    if (bt.N == 0 || bt.Q == 0 || nshards == 0) return hipSuccess;
    if (nshards > 65535u) return hipErrorInvalidValue;  // (the shard is the grid's y)
    const size_t blocks = (bt.Q + 64 * WG_WAVES - 1) / (64 * WG_WAVES);
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    // every entry the kernel does not write is 0
    const hipError_t e = hipMemsetAsync(d_pairs, 0, (size_t)nshards * bt.N * 16, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(overlap_kernel, dim3((unsigned)blocks, nshards), dim3(64 * WG_WAVES), 0, stream, d_shards, bt, (ulonglong2 *)d_pairs,
                       (ulonglong2 *)d_ivals, d_work);
    return hipGetLastError();
}

hipError_t launch_overlap_records(uint32_t nshards, const overlap_batch &bt, const void *d_pairs, const void *d_ivals, void *d_out,
                                  uint64_t cap_records, unsigned long long *d_counter, hipStream_t stream) {
    if (bt.N == 0 || bt.Q == 0 || nshards == 0) return hipSuccess;
    if (nshards > 65535u) return hipErrorInvalidValue;
    const size_t blocks = (bt.N + 255) / 256;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(overlap_records_kernel, dim3((unsigned)blocks, nshards), dim3(256), 0, stream, bt, (const ulonglong2 *)d_pairs,
                       (const ulonglong2 *)d_ivals, (rsbwt_overlap *)d_out, cap_records, d_counter);
    return hipGetLastError();
}

void overlap_set_last_work(const uint64_t work6[6]) {
    for (int i = 0; i < 6; ++i) overlap_last[i] = work6 ? work6[i] : 0;
}
void overlap_get_last_work(uint64_t work6[6]) { memcpy(work6, overlap_last, sizeof overlap_last); }

// One device's share of a host-buffer call on `st`: the batch goes up once, one launch walks every (query, shard of
// d_views), and -- when recs is asked for -- a second one compacts the entries with count > 0 where they are.  pairs
// ({ordinal, count}[S][N]) and recs (shard = d_views' number, unordered) are each optional; work5 += {LF steps,
// lane-passes that fetched a line, table starts, lane-passes fetched for '$' alone, entries with count > 0}.
// Synchronises `st`.
int overlap_host_views(scratch_cache &scratch, hipStream_t st, const shard_view *d_views, uint32_t S, const char *t0, const uint64_t *rel, size_t Q,
                       size_t N, uint32_t min_overlap, uint32_t max_overlap, uint64_t *pairs, std::vector<rsbwt_overlap> *recs, uint64_t *work5) {
    if (N == 0 || Q == 0 || S == 0) return RSBWT_OK;
    const size_t cells = (size_t)S * N;
    const size_t a_text = al256(N + 1), a_off = al256((Q + 1) * 8), a_pairs = al256(cells * 16), a_iv = recs ? al256(cells * 16) : 0,
                 a_rec = recs ? al256(cells * sizeof(rsbwt_overlap)) : 0;
    scratch_cache::lease mem;
    hipError_t e = scratch.take(a_text + a_off + a_pairs + a_iv + a_rec + 256, st, &mem);
    if (e != hipSuccess) return fail(RSBWT_ENOMEM, "%zu positions x %u shards do not fit the device's free memory: %s", N, S, hipGetErrorString(e));
    struct give_back {  // after the stream has drained: the launches may still run when the call leaves early
        scratch_cache &sc;
        scratch_cache::lease &l;
        hipStream_t st;
        ~give_back() {
            (void)hipStreamSynchronize(st);
            sc.give(l, st);
        }
    } give{scratch, mem, st};
    uint8_t *d_text = (uint8_t *)mem.p, *d_off = d_text + a_text, *d_pairs = d_off + a_off, *d_iv = d_pairs + a_pairs, *d_rec = d_iv + a_iv,
            *d_wk = d_rec + a_rec;
    OV_HIP(hipMemcpyAsync(d_text, t0, N, hipMemcpyHostToDevice, st));
    OV_HIP(hipMemcpyAsync(d_off, rel, (Q + 1) * 8, hipMemcpyHostToDevice, st));
    OV_HIP(hipMemsetAsync(d_wk, 0, 256, st));
    overlap_batch bt;
    bt.text = (const char *)d_text;
    bt.off = (const uint64_t *)d_off;
    bt.Q = Q;
    bt.N = N;
    bt.min_overlap = min_overlap ? min_overlap : 1u;
    bt.max_overlap = max_overlap;
    unsigned long long *wk = (unsigned long long *)d_wk;  // [0..4] the walk's counters, [5] records
    e = launch_overlaps(d_views, S, bt, d_pairs, recs ? d_iv : nullptr, wk, st);
    if (e != hipSuccess) return fail_hip(e, "overlap kernel launch");
    if (recs) {
        e = launch_overlap_records(S, bt, d_pairs, d_iv, d_rec, cells, wk + 5, st);
        if (e != hipSuccess) return fail_hip(e, "overlap-records kernel launch");
    }
    if (pairs) OV_HIP(hipMemcpyAsync(pairs, d_pairs, cells * 16, hipMemcpyDeviceToHost, st));
    unsigned long long hwk[6] = {0, 0, 0, 0, 0, 0};
    OV_HIP(hipMemcpyAsync(hwk, d_wk, sizeof hwk, hipMemcpyDeviceToHost, st));
    OV_HIP(hipStreamSynchronize(st));
    if (recs) {  // the counter first (it sizes the copy), then the records and nothing else
        if (hwk[5] > cells) return fail(RSBWT_EHIP, "the overlap-records kernel kept %llu of %zu positions", hwk[5], cells);
        recs->resize((size_t)hwk[5]);
        if (hwk[5]) {
            OV_HIP(hipMemcpyAsync(recs->data(), d_rec, (size_t)hwk[5] * sizeof(rsbwt_overlap), hipMemcpyDeviceToHost, st));
            OV_HIP(hipStreamSynchronize(st));
        }
    }
    if (work5)
        for (int i = 0; i < 5; ++i) work5[i] += hwk[i];
    return RSBWT_OK;
}

}  // namespace rsb
