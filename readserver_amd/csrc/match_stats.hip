// match_stats.hip -- matching statistics on the GPU (gfx950): for every END position t of a batch of queries and every
// shard, the longest string ending at t that the shard still supports, and its interval (include/rsbwt.h: the
// definition).  findInterval answers for a string whose two ends the caller chose and forgets how deep it got when it
// dies (query.cpp:24-41: an empty interval that depends on the step it died at); here the search of text[.. t] runs
// backwards from t until the first LF step that leaves fewer than m rows, and the depth reached IS the answer.  W(x)
// cannot grow when x grows to the left (Occ(c, hi) - Occ(c, lo - 1) <= hi - lo + 1 for any run stream), so that first
// failing step is where the longest match ends: nothing past it is looked at.
//
// One lane owns one (position, shard), in the pattern of gt_narrow.hip: the shard is blockIdx.y, the lanes of a wave
// take consecutive positions, fetch one window line per lane and pass through the wave's LDS stage (wave_lines.h) and
// rank the symbol off the staged line (rank_device.h, rank24); a position past its line's own pieces (spill chunk, far
// line) goes through the scalar reader (line_format.h, view_occ).
//   * START: the shard's k-mer table entry of text[t-T+1 .. t] where min(e, cap) >= T and those T symbols are all ACGT,
//     taken iff it passes start_record's rule (search_lines.hip: not KTAB_WIDE, lower + width <= n) AND holds m rows or
//     more: depth T at no LF step.  A refused entry says only that the depth is below T (an absent T-mer in either
//     format, a grouped record that gives up, an interval narrower than m): the lane starts over from initInterval of
//     text[t] (query.cpp:18-21), depth 1 if that symbol's rows pass.
//   * STEP: Occ(c, lo - 1) and Occ(c, hi) off ONE fetched line in one pass when hi lies in lo - 1's window among that
//     line's own pieces -- nearly every step of a deep match -- else one pass per position; lo == 0 is Occ(., -1) = 0 and
//     fetches nothing for that side.  A step that leaves m rows or more is taken; any other ends the item with the
//     interval it held.  An item also ends, fetching nothing more, at depth min(e, cap) or when the next symbol to the
//     left is not ACGT: the lane reads that symbol anyway (it is the step's symbol, read one step ahead so that it
//     travels with the line), so no side array of the queries' other symbols is needed, and the device-resident form
//     needs no pass over the text before the launch.
//   * RESULT: one u32 and, when asked for, one 16-byte {lower, upper} per item; no atomics but the work counters'.
// match_smem_kernel then flags the positions whose match no neighbour contains (len > 0 and the query ends here or the
// next position's match is not longer: the starts t - len never decrease along a query) and compacts them as
// gt_filter_kernel does: a ballot, a popcount and one atomic per wave; only those records leave the device.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "capi_internal.h"
#include "kernels.h"
#include "line_format.h"
#include "match_lanes.h"
#include "rank_device.h"
#include "wave_lines.h"

namespace rsb {

namespace {

__global__ void __launch_bounds__(64 * WG_WAVES)
match_stats_kernel(const shard_view *__restrict__ shards, const match_batch bt, uint32_t *__restrict__ len, ulonglong2 *__restrict__ pairs,
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
    const uint64_t n = sv->n, m = bt.m;
    const uint32_t T = sv->ktab != nullptr && sv->ktab_depth >= 2u ? sv->ktab_depth : 0u;
    const uint64_t C1 = sv->C[1], C2 = sv->C[2], C3 = sv->C[3], C4 = sv->C[4];  // (uniform: picked by compares, no load per step)

    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool mine = t < bt.N;
    const uint8_t *text = reinterpret_cast<const uint8_t *>(bt.text);

    // the lane's match: text[t-l+1 .. t] with interval (lo, hi); limit = min(e, cap)
    uint32_t l = 0, limit = 0, c = 0, phase = 0, sym = 0;  // sym = text[t - l], read one step ahead
    uint64_t lo = 1, hi = 0, occ_lo = 0;
    bool active = false, pending = false;
    uint32_t steps = 0, passes = 0, tab_starts = 0, restarts = 0;
    if (mine) {
        const size_t q = ms_query_of(bt.off, bt.Q, t);
        uint64_t e = t - bt.off[q] + 1ull;  // (at most 2^31 - 1: the host refuses longer queries)
        if (e > (uint64_t)t + 1ull) e = (uint64_t)t + 1ull;  // (offsets that do not fit N must not send a lane in front of the text)
        limit = (uint32_t)(bt.cap != 0u && e > bt.cap ? bt.cap : e);
        bool tabulated = false;
        if (T != 0u && limit >= T) {
            uint64_t code = 0;
            bool acgt = true;
            for (uint32_t i = 0; i < T; ++i) {
                const uint32_t r = ms_rank(text[t - T + 1u + i]);
                acgt = acgt && r != 0u;
                code |= (uint64_t)((r - 1u) & 3u) << (2u * i);
            }
            if (acgt) {
                const uint64_t en = ktab_entry(sv->ktab, sv->ktab_fmt, T, sv->ktab_stride, code);
                const uint32_t width = (uint32_t)(en >> COUNT_BITS);
                if (width != KTAB_WIDE && (en & COUNT_MASK) + width <= n && (uint64_t)width >= m) {  // (search_lines.hip, start_record's rule)
                    lo = en & COUNT_MASK;
                    hi = lo + width - 1ull;
                    l = T;
                    tabulated = true;
                    tab_starts = 1u;
                } else {
                    restarts = 1u;  // the depth is below T: from initInterval
                }
            }
        }
        if (!tabulated) {  // initInterval (query.cpp:18-21) of text[t]: its rows are the symbol's total
            const uint32_t cb = ms_rank(text[t]);
            if (cb != 0u) {
                const uint64_t a = sv->C[cb], b = a + sv->total[cb] - 1ull;
                const uint64_t W = (a <= b && b < n) ? b - a + 1ull : 0ull;
                if (W >= m) {
                    lo = a;
                    hi = b;
                    l = 1u;
                }
            }
        }
        active = l != 0u;
        if (active && l < limit) sym = text[t - l];
    }

    for (;;) {
        // ---- what needs no rank: the item ends at its limit or at a symbol outside ACGT, else the next step is set up
        if (active && !pending) {
            if (l == limit) {
                active = false;
            } else {
                c = ms_rank(sym);
                if (c == 0u) {
                    active = false;
                } else {
                    occ_lo = 0;
                    phase = lo == 0ull ? 1u : 0u;  // Occ(., -1) = 0
                    pending = true;
                }
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
        // the symbol of the step after this one travels with the line: a step then waits for memory once, not twice
        uint32_t sym_next = 0;
        if (pending && l + 1u < limit) sym_next = text[t - l - 1u];
        glds_fetch(lines_bytes, want, lane, stage_lds);  // (every lane takes part: lanes with nothing to rank ask for nothing)
        glds_wait();
        if (pending) {
            if (bad) {
                active = false;  // the item ends where it stands
                pending = false;
            } else {
                ++passes;
                const sym_tab tab = make_sym_tab(c);
                const line_head h = read_head(L);
                const bool own = o <= h.span;
                const uint64_t occ = own ? ms_staged_occ(L, h, o, c, tab) : view_occ(*sv, c, p);
                uint64_t occ_hi = occ;
                bool done = phase != 0u;
                if (!done) {
                    occ_lo = occ;
                    const uint64_t oh = (uint64_t)o + (hi - p);  // hi's offset in lo - 1's window, if it lies there
                    if (own && hi >= p && oh <= (uint64_t)h.span) {
                        occ_hi = ms_staged_occ(L, h, (uint32_t)oh, c, tab);
                        done = true;
                    } else {
                        phase = 1u;
                    }
                }
                if (done) {
                    ++steps;
                    pending = false;
                    const uint64_t pc = c == 1u ? C1 : c == 2u ? C2 : c == 3u ? C3 : C4;
                    const uint64_t nlo = pc + occ_lo, nhi = pc + occ_hi - 1ull;
                    const uint64_t W = (nlo <= nhi && nhi < n) ? nhi - nlo + 1ull : 0ull;
                    if (W >= m) {
                        lo = nlo;
                        hi = nhi;
                        ++l;
                        sym = sym_next;
                    } else {
                        active = false;  // the first failing step: the match ends with the interval it held
                    }
                }
            }
        }
    }
    if (mine) {
        const size_t at = (size_t)sid * bt.N + t;
        len[at] = l;
        if (pairs) pairs[at] = l != 0u ? make_ulonglong2(lo, hi) : make_ulonglong2(1ull, 0ull);
    }
    if (work) {  // (every lane of the wave is here: nothing above returns)
        const unsigned long long s0 = ms_wave_sum(steps), s1 = ms_wave_sum(passes), s2 = ms_wave_sum(tab_starts), s3 = ms_wave_sum(restarts);
        if (lane == 0u) {
            if (s0) atomicAdd(&work[0], s0);
            if (s1) atomicAdd(&work[1], s1);
            if (s2) atomicAdd(&work[2], s2);
            if (s3) atomicAdd(&work[3], s3);
        }
    }
}

// Position t of shard blockIdx.y is a SMEM iff len > 0 and (the query ends at t or len[t + 1] <= len[t]); the kept
// positions' records are compacted: a wave counts them, claims that many records from *counter with one atomic and
// every kept lane writes its own (in no particular order: the host sorts).  shard = the launch's number.
__global__ void __launch_bounds__(256)
match_smem_kernel(const match_batch bt, const uint32_t *__restrict__ len, const ulonglong2 *__restrict__ pairs, rsbwt_smem *__restrict__ out,
                  uint64_t cap_records, unsigned long long *__restrict__ counter) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u, sid = blockIdx.y;
    bool keep = false;
    rsbwt_smem rec = {0, 0, 0, 0, 0, 0, 0};
    if (t < bt.N) {
        const size_t at = (size_t)sid * bt.N + t;
        const uint32_t l = len[at];
        if (l != 0u) {
            const size_t q = ms_query_of(bt.off, bt.Q, t);
            if (t + 1 == bt.off[q + 1] || len[at + 1] <= l) {
                keep = true;
                const uint32_t e = (uint32_t)(t - bt.off[q] + 1ull);
                const ulonglong2 iv = pairs[at];
                rec = rsbwt_smem{(uint64_t)q, sid, e - l, e, 0u, iv.x, iv.y};
            }
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

thread_local uint64_t match_last[6] = {0, 0, 0, 0, 0, 0};

#define MS_HIP(x)                                              \
    do {                                                       \
        hipError_t _e = (x);                                   \
        if (_e != hipSuccess) return fail_hip(_e, #x);         \
    } while (0)

}  // namespace

hipError_t launch_match_stats(const shard_view *d_shards, uint32_t nshards, const match_batch &bt, void *d_len, void *d_pairs,
                              unsigned long long *d_work, hipStream_t stream) {
    if (bt.N == 0 || bt.Q == 0 || nshards == 0) return hipSuccess;
    if (nshards > 65535u) return hipErrorInvalidValue;  // (the shard is the grid's y)
    const size_t blocks = (bt.N + 64 * WG_WAVES - 1) / (64 * WG_WAVES);
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(match_stats_kernel, dim3((unsigned)blocks, nshards), dim3(64 * WG_WAVES), 0, stream, d_shards, bt, (uint32_t *)d_len,
                       (ulonglong2 *)d_pairs, d_work);
    return hipGetLastError();
}

hipError_t launch_match_smems(uint32_t nshards, const match_batch &bt, const void *d_len, const void *d_pairs, void *d_smems, uint64_t cap_records,
                              unsigned long long *d_counter, hipStream_t stream) {
    if (bt.N == 0 || bt.Q == 0 || nshards == 0) return hipSuccess;
    if (nshards > 65535u) return hipErrorInvalidValue;
    const size_t blocks = (bt.N + 255) / 256;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(match_smem_kernel, dim3((unsigned)blocks, nshards), dim3(256), 0, stream, bt, (const uint32_t *)d_len,
                       (const ulonglong2 *)d_pairs, (rsbwt_smem *)d_smems, cap_records, d_counter);
    return hipGetLastError();
}

void match_set_last_work(const uint64_t work6[6]) {
    for (int i = 0; i < 6; ++i) match_last[i] = work6 ? work6[i] : 0;
}
void match_get_last_work(uint64_t work6[6]) { memcpy(work6, match_last, sizeof match_last); }

// What every host-buffer call checks first: off[] ascending, no query over 2^31 - 1 symbols, the batch under 2^31
// positions; rel = the offsets from off[0], *N = the positions
int match_check_batch(const char *text, const uint64_t *off, size_t Q, std::vector<uint64_t> *rel, size_t *N) {
    *N = 0;
    rel->clear();
    if (Q == 0) return RSBWT_OK;
    if (!off) return fail(RSBWT_EINVAL, "null argument");
    rel->resize(Q + 1);
    for (size_t q = 0; q < Q; ++q) {
        if (off[q] > off[q + 1]) return fail(RSBWT_EINVAL, "query %zu: offsets not ascending", q);
        const uint64_t Lq = off[q + 1] - off[q];
        if (Lq > 0x7FFFFFFFull) return fail(RSBWT_EINVAL, "query %zu: %llu symbols, at most 2^31 - 1", q, (unsigned long long)Lq);
        (*rel)[q] = off[q] - off[0];
    }
    (*rel)[Q] = off[Q] - off[0];
    if ((*rel)[Q] >= (1ull << 31)) return fail(RSBWT_ERANGE, "%llu positions in one call: at most 2^31 - 1", (unsigned long long)(*rel)[Q]);
    if ((*rel)[Q] != 0 && !text) return fail(RSBWT_EINVAL, "null argument");
    *N = (size_t)(*rel)[Q];
    return RSBWT_OK;
}

// One device's share of a host-buffer call on `st`: the batch goes up once, one launch ranks every (position, shard of
// d_views), and -- when smems is asked for -- a second one flags and compacts the SMEMs where they are.  len / pairs
// ([S][N], pairs as {lower, upper}) and smems (shard = d_views' number, unordered) are each optional; work4 += {LF
// steps, lane-passes that fetched a line, table starts, restarts}.  Synchronises `st`.
int match_host_views(scratch_cache &scratch, hipStream_t st, const shard_view *d_views, uint32_t S, const char *t0, const uint64_t *rel, size_t Q,
                     size_t N, uint32_t cap, uint64_t m, uint32_t *len, uint64_t *pairs, std::vector<rsbwt_smem> *smems, uint64_t *work4) {
    if (N == 0 || Q == 0 || S == 0) return RSBWT_OK;
    const size_t cells = (size_t)S * N;
    const bool want_pairs = pairs != nullptr || smems != nullptr;
    const size_t a_text = al256(N + 1), a_off = al256((Q + 1) * 8), a_len = al256(cells * 4 + 4), a_pairs = want_pairs ? al256(cells * 16) : 0,
                 a_rec = smems ? al256(cells * sizeof(rsbwt_smem)) : 0;
    scratch_cache::lease mem;
    hipError_t e = scratch.take(a_text + a_off + a_len + a_pairs + a_rec + 256, st, &mem);
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
    uint8_t *d_text = (uint8_t *)mem.p, *d_off = d_text + a_text, *d_len = d_off + a_off, *d_pairs = d_len + a_len, *d_rec = d_pairs + a_pairs,
            *d_wk = d_rec + a_rec;
    MS_HIP(hipMemcpyAsync(d_text, t0, N, hipMemcpyHostToDevice, st));
    MS_HIP(hipMemcpyAsync(d_off, rel, (Q + 1) * 8, hipMemcpyHostToDevice, st));
    MS_HIP(hipMemsetAsync(d_wk, 0, 256, st));
    match_batch bt;
    bt.text = (const char *)d_text;
    bt.off = (const uint64_t *)d_off;
    bt.Q = Q;
    bt.N = N;
    bt.cap = cap;
    bt.m = m ? m : 1;
    unsigned long long *wk = (unsigned long long *)d_wk;  // [0..3] the search's counters, [4] SMEMs
    e = launch_match_stats(d_views, S, bt, d_len, want_pairs ? d_pairs : nullptr, wk, st);
    if (e != hipSuccess) return fail_hip(e, "matching-statistics kernel launch");
    if (smems) {
        e = launch_match_smems(S, bt, d_len, d_pairs, d_rec, cells, wk + 4, st);
        if (e != hipSuccess) return fail_hip(e, "SMEM kernel launch");
    }
    if (len) MS_HIP(hipMemcpyAsync(len, d_len, cells * 4, hipMemcpyDeviceToHost, st));
    if (pairs) MS_HIP(hipMemcpyAsync(pairs, d_pairs, cells * 16, hipMemcpyDeviceToHost, st));
    unsigned long long hwk[5] = {0, 0, 0, 0, 0};
    MS_HIP(hipMemcpyAsync(hwk, d_wk, sizeof hwk, hipMemcpyDeviceToHost, st));
    MS_HIP(hipStreamSynchronize(st));
    if (smems) {  // the counter first (it sizes the copy), then the SMEMs' records and nothing else
        if (hwk[4] > cells) return fail(RSBWT_EHIP, "the SMEM kernel kept %llu of %zu positions", hwk[4], cells);
        smems->resize((size_t)hwk[4]);
        if (hwk[4]) {
            MS_HIP(hipMemcpyAsync(smems->data(), d_rec, (size_t)hwk[4] * sizeof(rsbwt_smem), hipMemcpyDeviceToHost, st));
            MS_HIP(hipStreamSynchronize(st));
        }
    }
    if (work4)
        for (int i = 0; i < 4; ++i) work4[i] += hwk[i];
    return RSBWT_OK;
}

}  // namespace rsb
