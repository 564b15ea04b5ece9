// kmer_reads.hip -- KmerMatch's Count / Reads (src/service/service.cpp:466-502, find_kmer_reads; KmerTask::run :871-960)
// over a shard set, with each distinct read extracted ONCE.
//
// The reference tiles the query into k-mers (get_tiles(w, k, skip), :232-246), runs find_reads on every tile -- for
// k < min_read_length the reads of EVERY row of the tile's interval, an LF walk and a psi walk per row (:718-753) --
// and only then folds the strings into an unordered_set.  A read that covers the query is extracted once per tile it
// holds.  Here:
//   1. one batched search of all tiles of all jobs over all shards (rsbwt_set_find_intervals_var);
//   2. the candidate rows (every row of every tile's interval) are numbered on the device by a prefix sum of the
//      interval widths: candidate c lies in segment seg (binary search of seg_first) at row seg_lo + (c - seg_first);
//   3. READ IDENTITY (kr_ident_kernel): every candidate row is mapped to the row of its read's full suffix, the row
//      an LF walk reaches where the BWT symbol is '$'.  A row of the tile at position p >= skip + 1 whose skip + 1
//      LF predecessors spell w[p-skip-1 .. p-1] lands inside the interval of the tile at p-skip-1, in the same read:
//      it stops there and names that row as its parent.  Only rows without such a predecessor walk on to '$'.  The
//      chains are resolved by pointer jumping (kr_jump_kernel);
//   4. the distinct identities of each shard are extracted once (rsbwt_set_extract);
//   5. the host replays the reference's unordered_set inserts -- find_reads' vector of each tile, in the reference's
//      visit order, every row standing for its read's string -- into a real std::unordered_set<std::string>, so that
//      iteration order and string-level dedupe (equal reads of different identities) are the reference's.
// Walks follow extract_lines.hip's prefix walk: one lane per walk, a window line per octet of lanes through LDS
// (wave_lines.h), symbol and rank off one look at the quarter's 24 pieces (rank_device.h, char_rank24).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <iterator>
#include <new>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "../../include/rsbwt.h"
#include "capi_guard.h"
#include "capi_internal.h"
#include "kmer_reads.h"
#include "rank_device.h"
#include "wave_lines.h"

namespace rsb {
namespace {

constexpr int KR_WAVES = 4;
constexpr uint64_t KR_NONE = ~0ull;
constexpr uint32_t KR_MAX_STEPS = 1u << 20;  // a walk longer than any read of a collection this service holds: a corrupt index

// candidate c -> its segment: the last seg with seg_first[seg] <= c (seg_first ascending, seg_first[nseg] = ncand)
__device__ __forceinline__ uint32_t kr_segment(const uint64_t *__restrict__ seg_first, uint32_t nseg, uint64_t c) {
    uint32_t lo = 0, hi = nseg;  // seg_first[lo] <= c < seg_first[hi]
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (seg_first[mid] <= c) lo = mid;
        else hi = mid;
    }
    return lo;
}

// One lane per candidate row, drawn in chunks of 64 from one counter.  par[c] = c and id[c] = the '$' row for a row
// that walked to its read's start; par[c] = the candidate it landed on for a chain member.  work[0] += rows walked to
// '$', work[1] += LF steps.
__global__ void __launch_bounds__(64 * KR_WAVES)
kr_ident_kernel(const shard_view *__restrict__ sv, const uint64_t *__restrict__ seg_first, const uint64_t *__restrict__ seg_lo,
                const uint32_t *__restrict__ seg_pred, const uint64_t *__restrict__ seg_chk, const uint32_t *__restrict__ seg_chklen,
                uint32_t nseg, const char *__restrict__ text, uint64_t ncand, uint64_t *__restrict__ par, uint64_t *__restrict__ id,
                unsigned long long *__restrict__ pool, unsigned long long *__restrict__ work) {
    __shared__ uint4 s_stage[KR_WAVES][64 * SLOT_U4];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint4 *stage = s_stage[wave];
    const uint32_t stage_lds = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)(lds_void_ptr)stage);
    const staged_line L = {own_stage_row(stage, lane), lane & 7u};
    const char *lines_bytes = reinterpret_cast<const char *>(sv->lines);
    const uint32_t S = sv->sp.S, nlines = (uint32_t)sv->nlines;
    const double inv = sv->sp.inv;
    const uint64_t ix_n = sv->n;
    uint32_t ctab_lo, ctab_hi;  // C[1..4] in lanes 0..3, read with ds_bpermute
    {
        const uint32_t l3 = lane & 3u;
        const uint64_t cv = l3 == 0u ? sv->C[1] : l3 == 1u ? sv->C[2] : l3 == 2u ? sv->C[3] : sv->C[4];
        ctab_lo = (uint32_t)cv;
        ctab_hi = (uint32_t)(cv >> 32);
    }
    unsigned long long walked = 0, steps_all = 0;
    uint64_t next = 0, end = 0;  // this wave's chunk of candidates (wave-uniform)
    bool drained = false, have = false;
    uint64_t cand = 0, idx = 0, chk_pos = 0;
    uint32_t seg = 0, chk_left = 0, steps = 0;
    uint32_t cont = 0, cblk = 0, cdw = 0, co = 0, tries = 0, w = 0;
    uint32_t acc_lo[4] = {0, 0, 0, 0}, acc_hi = 0;
    for (;;) {
        // ---- hand candidates to the lanes that have none
        const uint64_t want_mask = __builtin_amdgcn_ballot_w64(!have);
        if (want_mask != 0ull && !drained) {
            if (next >= end) {
                unsigned long long c0 = 0;
                if (lane == 0u) c0 = atomicAdd(pool, 64ull);
                c0 = ((unsigned long long)__builtin_amdgcn_readfirstlane((uint32_t)(c0 >> 32)) << 32) | __builtin_amdgcn_readfirstlane((uint32_t)c0);
                if (c0 >= ncand) {
                    drained = true;
                    next = end = 0;
                } else {
                    next = c0;
                    end = c0 + 64u < ncand ? c0 + 64u : ncand;
                }
            }
            if (!drained) {
                const uint64_t mine = next + __builtin_popcountll(want_mask & ((1ull << lane) - 1ull));
                if (!have && mine < end) {
                    cand = mine;
                    seg = kr_segment(seg_first, nseg, cand);
                    idx = seg_lo[seg] + (cand - seg_first[seg]);
                    chk_left = seg_pred[seg] != 0xFFFFFFFFu ? seg_chklen[seg] : 0u;
                    chk_pos = seg_chk[seg];
                    steps = 0;
                    cont = 0;
                    have = true;
                    if (idx >= ix_n) {  // (not a row of this shard: the host never makes one)
                        par[cand] = cand;
                        id[cand] = KR_NONE;
                        have = false;
                    }
                }
                const uint64_t taken = next + __builtin_popcountll(want_mask);
                next = taken < end ? taken : end;
            }
        }
        if (__builtin_amdgcn_ballot_w64(have) == 0ull) {
            if (drained) break;
            continue;
        }
        // ---- this lane's line (extract_prefix_wave_kernel's pass, without the characters' output)
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
        bool scan = false;
        uint32_t dw = HDR_DWORDS, rem = 0, cq = 0;
        if (have) {
            if (!in_chunk) {
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
                    const uint4 h0 = L.u4(0), h1 = L.u4(4);
                    acc_lo[0] = h0.x; acc_lo[1] = h0.z; acc_lo[2] = h1.x; acc_lo[3] = h1.z;
                    acc_hi = (h0.y & 0xFFu) | ((h0.w & 0xFFu) << 8) | ((h1.y & 0xFFu) << 16) | (h1.w << 24);
                    cdw = read_chunk_dword(L);
                    cblk = (w >> GROUP_SHIFT) * (GROUP + 1u) + GROUP;
                    if (cblk >= nlines) cblk = 0;
                    cont = KIND_CHUNK;
                    co = oe - h.span;
                } else {
                    scan = true;
                }
            } else {
                dw = cdw + 2u;
                rem = co;
                scan = true;
            }
            if (!scan && ++tries > 72u) scan = true;
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
        const uint64_t pc = ((uint64_t)(uint32_t)__builtin_amdgcn_ds_bpermute((int)(ci << 2), (int)ctab_hi) << 32) |
                            (uint32_t)__builtin_amdgcn_ds_bpermute((int)(ci << 2), (int)ctab_lo);
        if (scan) {
            if (c == 0u || c > 4u) {  // '$': idx is the row of the read's full suffix
                par[cand] = cand;
                id[cand] = idx;
                ++walked;
                have = false;
            } else if (steps >= KR_MAX_STEPS) {
                par[cand] = cand;
                id[cand] = KR_NONE;
                have = false;
            } else {
                const uint32_t ch = (0x54474341u >> (8u * ci)) & 0xFFu;  // "ACGT"[c-1]
                idx = pc + base + cr.occ - 1ull;  // LF (query.cpp:55-56)
                ++steps;
                ++steps_all;
                cont = 0;
                if (chk_left != 0u) {
                    if ((uint32_t)(uint8_t)text[chk_pos] != ch) {
                        chk_left = 0;  // not the query's preceding symbol: walk on to '$'
                    } else if (--chk_left == 0u) {
                        const uint32_t ps = seg_pred[seg];
                        const uint64_t plo = seg_lo[ps], pw = seg_first[ps + 1u] - seg_first[ps];
                        if (idx >= plo && idx - plo < pw) {  // in the interval of the tile at p - skip - 1: a chain member
                            par[cand] = seg_first[ps] + (idx - plo);
                            id[cand] = KR_NONE;
                            have = false;
                        }
                    } else {
                        --chk_pos;
                    }
                }
            }
        }
    }
    // (two atomics per lane that walked at all: once per launch)
    if (walked) atomicAdd(&work[0], walked);
    if (steps_all) atomicAdd(&work[1], steps_all);
}

// One round of pointer jumping: par[c] = par[par[c]] (in place: a value only ever moves towards its chain's root).
__global__ void __launch_bounds__(256) kr_jump_kernel(uint64_t *__restrict__ par, uint64_t n) {
    const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n) return;
    par[c] = par[par[c]];
}
// ident[c] = id[root of c]
__global__ void __launch_bounds__(256) kr_resolve_kernel(const uint64_t *__restrict__ par, const uint64_t *__restrict__ id,
                                                         uint64_t *__restrict__ ident, uint64_t n) {
    const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n) return;
    const uint64_t r = par[c];
    ident[c] = par[r] == r ? id[r] : KR_NONE;  // (a root after the rounds; KR_NONE only for a chain longer than 2^rounds)
}

#define KR_HIP(x)                                              \
    do {                                                       \
        hipError_t _e = (x);                                   \
        if (_e != hipSuccess) return fail_hip(_e, #x);         \
    } while (0)

struct dev_buf {
    void *p = nullptr;
    ~dev_buf() {
        if (p) (void)hipFree(p);
    }
};

}  // namespace

int kmer_ident_shard(rsbwt_t *h, const kr_segments &sg, const std::string &text, std::vector<uint64_t> *ident, kmer_work *work) {
    const uint64_t ncand = sg.first.empty() ? 0 : sg.first.back();
    ident->assign(ncand, KR_NONE);
    if (ncand == 0) return RSBWT_OK;
    const uint32_t nseg = (uint32_t)sg.lo.size();
    int rc = use_device(h->device);
    if (rc) return rc;
    call_ctx *cx = h->pool.acquire();
    if (!cx) return fail(RSBWT_EHIP, "cannot create a HIP stream");
    struct release_t {
        rsbwt_t *h;
        call_ctx *c;
        ~release_t() { h->pool.release(c); }
    } release{h, cx};
    hipStream_t st = cx->st[0];
    auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t a_first = al((nseg + 1) * 8), a_lo = al(nseg * 8), a_pred = al(nseg * 4), a_chk = al(nseg * 8), a_len = al(nseg * 4),
                 a_text = al(text.size() + 1), a_cand = al(ncand * 8), a_misc = 256;
    const size_t total = a_first + a_lo + a_pred + a_chk + a_len + a_text + 3 * a_cand + a_misc;
    dev_buf mem;
    if (hipMalloc(&mem.p, total) != hipSuccess) {
        (void)hipGetLastError();
        mem.p = nullptr;
        return fail(RSBWT_ENOMEM, "%zu bytes of device memory for %llu candidate rows", total, (unsigned long long)ncand);
    }
    uint8_t *b = (uint8_t *)mem.p;
    uint64_t *d_first = (uint64_t *)b; b += a_first;
    uint64_t *d_lo = (uint64_t *)b; b += a_lo;
    uint32_t *d_pred = (uint32_t *)b; b += a_pred;
    uint64_t *d_chk = (uint64_t *)b; b += a_chk;
    uint32_t *d_len = (uint32_t *)b; b += a_len;
    char *d_text = (char *)b; b += a_text;
    uint64_t *d_par = (uint64_t *)b; b += a_cand;
    uint64_t *d_id = (uint64_t *)b; b += a_cand;
    uint64_t *d_ident = (uint64_t *)b; b += a_cand;
    unsigned long long *d_misc = (unsigned long long *)b;  // [0] candidate pool, [8..9] work
    KR_HIP(hipMemcpyAsync(d_first, sg.first.data(), (nseg + 1) * 8, hipMemcpyHostToDevice, st));
    KR_HIP(hipMemcpyAsync(d_lo, sg.lo.data(), nseg * 8, hipMemcpyHostToDevice, st));
    KR_HIP(hipMemcpyAsync(d_pred, sg.pred.data(), nseg * 4, hipMemcpyHostToDevice, st));
    KR_HIP(hipMemcpyAsync(d_chk, sg.chk.data(), nseg * 8, hipMemcpyHostToDevice, st));
    KR_HIP(hipMemcpyAsync(d_len, sg.chklen.data(), nseg * 4, hipMemcpyHostToDevice, st));
    if (!text.empty()) KR_HIP(hipMemcpyAsync(d_text, text.data(), text.size(), hipMemcpyHostToDevice, st));
    KR_HIP(hipMemsetAsync(d_misc, 0, a_misc, st));
    const size_t g = plan_grid((size_t)ncand, 64 * KR_WAVES, resident_cap(h->num_cus, 4));
    hipLaunchKernelGGL(kr_ident_kernel, dim3((uint32_t)g), dim3(64 * KR_WAVES), 0, st, h->d_view, d_first, d_lo, d_pred, d_chk, d_len, nseg,
                       d_text, ncand, d_par, d_id, d_misc, d_misc + 8);
    KR_HIP(hipGetLastError());
    // pointer jumping: a chain hop moves skip + 1 >= 1 symbols back inside one read, so 2^rounds > the longest read
    // the walk allows resolves every chain
    const uint32_t blocks = (uint32_t)((ncand + 255) / 256);
    for (int r = 0; r < 21; ++r) {
        hipLaunchKernelGGL(kr_jump_kernel, dim3(blocks), dim3(256), 0, st, d_par, ncand);
        KR_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(kr_resolve_kernel, dim3(blocks), dim3(256), 0, st, d_par, d_id, d_ident, ncand);
    KR_HIP(hipGetLastError());
    unsigned long long wk[2] = {0, 0};
    KR_HIP(hipMemcpyAsync(ident->data(), d_ident, ncand * 8, hipMemcpyDeviceToHost, st));
    KR_HIP(hipMemcpyAsync(wk, d_misc + 8, sizeof(wk), hipMemcpyDeviceToHost, st));
    KR_HIP(hipStreamSynchronize(st));
    if (work) {
        work->candidates += ncand;
        work->walked += wk[0];
        work->lf_steps += wk[1];
    }
    return RSBWT_OK;
}

namespace {

inline double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

inline bool all_acgt(const std::string &t) { return t.find_first_not_of("ACGT") == std::string::npos; }

// get_tiles(w, kmer, skip) (service.cpp:232-246): the same container filled in the same order, so that iterating it
// visits the tiles in the reference's order on the same standard library
std::vector<std::string> tiles_in_order(const std::string &w, size_t kmer, size_t skip) {
    std::unordered_set<std::string> vs;
    if (w.size() >= kmer)
        for (size_t i = 0; i <= w.size() - kmer; i += skip + 1) vs.insert(w.substr(i, kmer));
    return std::vector<std::string>(vs.begin(), vs.end());
}

// find_reads' order of a wide interval (service.cpp:724-751; service_slice.cpp, chunked_head): the rows that are left
// after the 2,048-row chunks come first
inline size_t chunked_head(size_t n) {
    const size_t large = 2048;  // service.cpp:86
    size_t start = 0;
    while (n != 0 && (n - 1) - start > 2 * large) start += large;
    return start;
}

struct kr_tile {
    size_t job;
    std::string s;
    size_t pred = SIZE_MAX;  // the tile at p - skip - 1 (global index), when a position p >= skip + 1 allows the check
    uint64_t chk = 0;        // offset of w[p - 1] in the jobs' text
    uint32_t chklen = 0;     // skip + 1
};

}  // namespace

int kmer_reads_batch(rsbwt_set_t *set, const std::vector<kmer_job> &jobs, size_t MINL, size_t MAXL, uint32_t read_stride,
                     std::vector<std::vector<std::vector<std::string>>> *out, std::vector<char> *failed, kmer_work *work) {
    const size_t J = jobs.size(), S = rsbwt_set_size(set);
    const double t_call = now_ms();
    out->assign(J, std::vector<std::vector<std::string>>(S));
    failed->assign(J, 0);
    if (J == 0) return RSBWT_OK;
    if (read_stride == 0) return fail(RSBWT_EINVAL, "read_stride must be positive");
    // ---- the tiles of every job, in the order find_kmer_reads visits them (:472-498): the last tile of the iteration
    // order first (the synchronous call, :487-491), if it is all ACGT, then the other ACGT tiles in iteration order
    std::vector<kr_tile> tiles;
    std::vector<std::vector<size_t>> visit(J);  // job -> global tile indices, in visit order
    std::string jtext;                           // the jobs' strings back to back (the walks' check symbols)
    for (size_t j = 0; j < J; ++j) {
        const kmer_job &jb = jobs[j];
        const uint64_t base = jtext.size();
        jtext += jb.w;
        if (jb.k <= 0 || jb.skip < 0 || jb.w.size() < (size_t)jb.k) continue;
        const size_t K = (size_t)jb.k, step = (size_t)jb.skip + 1;
        const std::vector<std::string> it = tiles_in_order(jb.w, K, step - 1);
        std::unordered_map<std::string, size_t> index;
        auto add = [&](const std::string &t) {
            index[t] = tiles.size();
            visit[j].push_back(tiles.size());
            tiles.push_back(kr_tile{j, t});
        };
        if (!it.empty() && all_acgt(it.back())) add(it.back());
        for (size_t i = 0; i + 1 < it.size(); ++i)
            if (all_acgt(it[i])) add(it[i]);
        // the chain check (k < min_read_length only: longer tiles walk nothing): the first position p >= skip + 1 of the
        // tile whose predecessor tile is all ACGT
        if (K >= MINL) continue;
        for (size_t p = step; p + K <= jb.w.size(); p += step) {
            auto me = index.find(jb.w.substr(p, K));
            if (me == index.end() || tiles[me->second].pred != SIZE_MAX) continue;
            auto pr = index.find(jb.w.substr(p - step, K));
            if (pr == index.end()) continue;
            tiles[me->second].pred = pr->second;
            tiles[me->second].chk = base + p - 1;
            tiles[me->second].chklen = (uint32_t)step;
        }
    }
    const size_t G = tiles.size();
    if (G == 0) return RSBWT_OK;
    // ---- one search of all the tiles over every shard
    std::string ttext;
    std::vector<uint64_t> toff(G + 1, 0);
    for (size_t g = 0; g < G; ++g) {
        ttext += tiles[g].s;
        toff[g + 1] = ttext.size();
    }
    std::vector<uint64_t> lo(S * G), up(S * G);
    kmer_work wk;
    double t_dev = now_ms();
    int rc = rsbwt_set_find_intervals_var(set, ttext.data(), toff.data(), G, lo.data(), up.data());
    wk.ms_device += now_ms() - t_dev;
    if (rc != RSBWT_OK) return rc;
    auto width = [&](size_t p, size_t g) -> uint64_t {
        const uint64_t l = lo[p * G + g], u = up[p * G + g];
        return (l <= u && u < rsbwt_bwlen(rsbwt_set_shard(set, p))) ? u - l + 1 : 0;
    };
    // ---- tiles of min_read_length or more (find_reads :755-797): their sub-tiles that are reads, per shard
    // sub[g][p]: the strings find_reads puts first for tile g in shard p; rows[g]: whether its interval's rows follow
    std::vector<std::vector<std::vector<const std::string *>>> sub(G);
    std::vector<std::string> subs;  // the sub-tile strings (stable: filled before any pointer is taken)
    {
        struct ask { size_t g, len; std::vector<size_t> idx; };  // a tile's sub-tiles of one length, indices into subs
        std::vector<ask> asks;
        for (size_t g = 0; g < G; ++g) {
            const size_t sz = tiles[g].s.size();
            std::vector<size_t> lens;
            if (sz < MINL) continue;
            if (sz < MAXL) { if (sz != MINL) lens.push_back(MINL); }
            else { lens.push_back(MAXL); if (MINL != MAXL) lens.push_back(MINL); }
            for (size_t T : lens) {
                ask a{g, T, {}};
                for (const std::string &t : tiles_in_order(tiles[g].s, T, 0)) { a.idx.push_back(subs.size()); subs.push_back(t); }
                asks.push_back(std::move(a));
            }
        }
        std::vector<std::vector<uint8_t>> found(S, std::vector<uint8_t>(subs.size(), 0));
        std::vector<std::vector<size_t>> by_len(MAXL + 1);
        for (const ask &a : asks) by_len[a.len].insert(by_len[a.len].end(), a.idx.begin(), a.idx.end());
        for (size_t T = 1; T <= MAXL; ++T) {
            const std::vector<size_t> &ix = by_len[T];
            if (ix.empty()) continue;
            std::string flat(ix.size() * T, 'N');
            for (size_t i = 0; i < ix.size(); ++i) memcpy(&flat[i * T], subs[ix[i]].data(), T);
            std::vector<uint8_t> f(ix.size());
            for (size_t p = 0; p < S; ++p) {
                t_dev = now_ms();
                rc = rsbwt_query_exactmatch(rsbwt_set_shard(set, p), flat.data(), ix.size(), (uint32_t)T, T, f.data());
                wk.ms_device += now_ms() - t_dev;
                if (rc != RSBWT_OK) return rc;
                for (size_t i = 0; i < ix.size(); ++i) found[p][ix[i]] = f[i];
            }
        }
        for (size_t g = 0; g < G; ++g) sub[g].resize(S);
        for (const ask &a : asks)
            for (size_t p = 0; p < S; ++p)
                for (size_t i : a.idx)
                    if (found[p][i]) sub[a.g][p].push_back(&subs[i]);
    }
    auto has_rows = [&](size_t g) { return tiles[g].s.size() < MAXL; };  // (|tile| >= max_read_length: sub-tiles only)
    // ---- jobs into passes: the ordinary ones together, every job with more than `wide` candidate rows on its own
    // (RSBWT_KMER_WIDE_ROWS overrides the 2^22: tests/test_gpu_kmer_match.py)
    const uint64_t wide = (uint64_t)knob_int("RSBWT_KMER_WIDE_ROWS", 1, LLONG_MAX, 1ll << 22);
    std::vector<std::vector<size_t>> passes(1);
    for (size_t j = 0; j < J; ++j) {
        uint64_t c = 0;
        for (size_t g : visit[j])
            if (has_rows(g))
                for (size_t p = 0; p < S; ++p) c += width(p, g);
        if (c > wide) passes.push_back({j});
        else passes[0].push_back(j);
    }
    auto run_pass = [&](const std::vector<size_t> &pass) -> int {
        // per shard: segments (the pass's tiles with rows in that shard), identities of their rows
        std::vector<std::vector<uint64_t>> ident(S), seg_first(S);
        std::vector<std::vector<size_t>> seg_tile(S);
        std::vector<std::unordered_map<size_t, uint32_t>> seg_of(S);
        std::vector<std::vector<uint64_t>> distinct(S);
        for (size_t p = 0; p < S; ++p) {
            kr_segments sg;
            sg.first.push_back(0);
            for (size_t j : pass)
                for (size_t g : visit[j]) {
                    const uint64_t wd = has_rows(g) ? width(p, g) : 0;
                    if (wd == 0) continue;
                    seg_of[p][g] = (uint32_t)sg.lo.size();
                    seg_tile[p].push_back(g);
                    sg.lo.push_back(lo[p * G + g]);
                    sg.first.push_back(sg.first.back() + wd);
                }
            sg.pred.assign(sg.lo.size(), 0xFFFFFFFFu);
            sg.chk.assign(sg.lo.size(), 0);
            sg.chklen.assign(sg.lo.size(), 0);
            for (size_t i = 0; i < seg_tile[p].size(); ++i) {
                const kr_tile &t = tiles[seg_tile[p][i]];
                if (t.pred == SIZE_MAX) continue;
                auto ps = seg_of[p].find(t.pred);
                if (ps == seg_of[p].end()) continue;
                sg.pred[i] = ps->second;
                sg.chk[i] = t.chk;
                sg.chklen[i] = t.chklen;
            }
            const double t0 = now_ms();
            const int rc = kmer_ident_shard(rsbwt_set_shard(set, p), sg, jtext, &ident[p], &wk);
            wk.ms_device += now_ms() - t0;
            if (rc != RSBWT_OK) return rc;
            seg_first[p] = std::move(sg.first);
            distinct[p] = ident[p];
            std::sort(distinct[p].begin(), distinct[p].end());
            distinct[p].erase(std::unique(distinct[p].begin(), distinct[p].end()), distinct[p].end());
            if (!distinct[p].empty() && distinct[p].back() == KR_NONE) distinct[p].pop_back();
            wk.identities += distinct[p].size();
        }
        // ---- every distinct identity extracted once (the '$' row: its postfix walk is the whole read)
        std::vector<uint32_t> shard_of;
        std::vector<uint64_t> rows;
        for (size_t p = 0; p < S; ++p)
            for (uint64_t r : distinct[p]) { shard_of.push_back((uint32_t)p); rows.push_back(r); }
        std::vector<std::string> reads(rows.size());
        if (!rows.empty()) {
            std::vector<char> buf(rows.size() * (size_t)read_stride, 0);
            std::vector<uint32_t> rlen(rows.size(), 0);
            double t0 = now_ms();
            int rc = rsbwt_set_extract(set, shard_of.data(), rows.data(), rows.size(), buf.data(), read_stride, rlen.data(), nullptr);
            wk.ms_device += now_ms() - t0;
            if (rc != RSBWT_OK) return rc;
            wk.extracted += rows.size();
            std::vector<size_t> over;  // reads longer than read_stride: once more, at the widest stride the service allows
            for (size_t r = 0; r < rows.size(); ++r) {
                if (rlen[r] == 0xFFFFFFFFu) over.push_back(r);
                else reads[r].assign(buf.data() + r * (size_t)read_stride, rlen[r]);
            }
            if (!over.empty()) {
                const uint32_t wide_stride = 65536;
                std::vector<uint32_t> osh(over.size()), olen(over.size());
                std::vector<uint64_t> orow(over.size());
                for (size_t i = 0; i < over.size(); ++i) { osh[i] = shard_of[over[i]]; orow[i] = rows[over[i]]; }
                std::vector<char> obuf(over.size() * (size_t)wide_stride, 0);
                t0 = now_ms();
                rc = rsbwt_set_extract(set, osh.data(), orow.data(), over.size(), obuf.data(), wide_stride, olen.data(), nullptr);
                wk.ms_device += now_ms() - t0;
                if (rc != RSBWT_OK) return rc;
                wk.extracted += over.size();
                for (size_t i = 0; i < over.size(); ++i) {
                    if (olen[i] == 0xFFFFFFFFu)
                        return fail(RSBWT_EINVAL, "shard %u row %llu: a read longer than %u symbols (or a walk that does not end)", osh[i],
                                    (unsigned long long)orow[i], wide_stride);
                    reads[over[i]].assign(obuf.data() + i * (size_t)wide_stride, olen[i]);
                }
            }
        }
        std::vector<size_t> shard_base(S + 1, 0);
        for (size_t p = 0; p < S; ++p) shard_base[p + 1] = shard_base[p] + distinct[p].size();
        // read index (into reads / rows) of an identity of shard p; SIZE_MAX for none
        auto read_of = [&](size_t p, uint64_t id) -> size_t {
            if (id == KR_NONE) return SIZE_MAX;
            const auto b = distinct[p].begin();
            return shard_base[p] + (size_t)(std::lower_bound(b, distinct[p].end(), id) - b);
        };
        // ---- the reference's inserts (find_kmer_reads :487-498; find_reads' vector of each tile), first occurrences only.
        // libstdc++'s unique-key range insert inserts element by element with no size hint (bits/hashtable_policy.h,
        // _Insert_base::_M_insert_range), so the set's iteration order is fixed by the order in which distinct strings
        // are first inserted: a row whose identity has been seen in this (job, shard) adds nothing, and each identity's
        // string is inserted once, at its first row.
        std::vector<size_t> seen(rows.size(), SIZE_MAX);  // read index -> the last (job, shard) it was inserted for
        size_t stamp = 0;
        for (size_t j : pass)
            for (size_t p = 0; p < S; ++p, ++stamp) {
                std::unordered_set<std::string> seqs;
                for (size_t g : visit[j]) {
                    for (const std::string *t : sub[g][p]) seqs.insert(*t);
                    auto sp = seg_of[p].find(g);
                    if (sp == seg_of[p].end()) continue;
                    const uint64_t f = seg_first[p][sp->second], cnt = seg_first[p][sp->second + 1] - f;
                    // rows of a tile shorter than min_read_length: find_reads' chunk order; otherwise query()'s row order
                    const size_t head = tiles[g].s.size() < MINL ? chunked_head((size_t)cnt) : 0;
                    for (uint64_t t = 0; t < cnt; ++t) {
                        const uint64_t r = t + head < cnt ? t + head : t + head - cnt;
                        const size_t ri = read_of(p, ident[p][f + r]);
                        if (ri == SIZE_MAX || seen[ri] == stamp) continue;
                        seen[ri] = stamp;
                        seqs.insert(reads[ri]);
                    }
                }
                (*out)[j][p].assign(seqs.begin(), seqs.end());
            }
        return RSBWT_OK;
    };
    int first_rc = RSBWT_OK;
    for (size_t pi = 0; pi < passes.size(); ++pi) {
        const std::vector<size_t> &pass = passes[pi];
        if (pass.empty()) continue;
        int prc;
        try {
            prc = run_pass(pass);
        } catch (const std::bad_alloc &) {
            prc = fail(RSBWT_ENOMEM, "host allocation failed");
        }
        if (prc == RSBWT_OK) continue;
        // the ordinary jobs' pass fails the call; a wide job's own pass only empties that job
        if (pi == 0 && first_rc == RSBWT_OK) first_rc = prc;
        fprintf(stderr, "rsbwt kmer reads: %zu job(s) answered empty: %s\n", pass.size(), rsbwt_last_error());
        for (size_t j : pass) {
            (*failed)[j] = 1;
            for (auto &l : (*out)[j]) l.clear();
        }
    }
    wk.ms_total = now_ms() - t_call;
    if (work) *work = wk;
    return first_rc;
}

}  // namespace rsb

// ---- C-ABI ------------------------------------------------------------------------------------------------------
namespace {
thread_local rsb::kmer_work kr_last;
// the service code's way in (kmer_reads.h)
struct register_hooks {
    register_hooks() {
        rsb::kmer_engine_hooks.batch = rsb::kmer_reads_batch;
        rsb::kmer_engine_hooks.opened_for_reads = rsbwt_opened_for_reads;
    }
} register_hooks_now;
}

extern "C" {

static int kmer_set_call(rsbwt_set_t *s, const char *text, const uint64_t *off, size_t Q, int32_t k, int32_t skip, uint32_t min_read_length,
                         uint32_t max_read_length, std::vector<std::vector<std::vector<std::string>>> *res, uint32_t stride) {
    if (!s || (!off && Q)) return rsb::fail(RSBWT_EINVAL, "null argument");
    if (Q && !text && off[Q] != off[0]) return rsb::fail(RSBWT_EINVAL, "null argument");
    for (size_t q = 0; q < Q; ++q)
        if (off[q] > off[q + 1]) return rsb::fail(RSBWT_EINVAL, "query %zu: offsets not ascending", q);
    std::vector<rsb::kmer_job> jobs(Q);
    for (size_t q = 0; q < Q; ++q) {
        jobs[q].w.assign(text + off[q], (size_t)(off[q + 1] - off[q]));
        jobs[q].k = k;
        jobs[q].skip = skip;
    }
    std::vector<char> failed;
    rsb::kmer_work wk;
    const int rc = rsb::kmer_reads_batch(s, jobs, min_read_length ? min_read_length : 73, max_read_length ? max_read_length : 100, stride, res,
                                         &failed, &wk);
    kr_last = wk;
    if (rc != RSBWT_OK) return rc;
    for (char f : failed)
        if (f) return rsb::fail(RSBWT_ENOMEM, "a query could not be answered");
    return RSBWT_OK;
}

int rsbwt_set_kmer_reads(rsbwt_set_t *s, const char *text, const uint64_t *off, size_t Q, int32_t k, int32_t skip, uint32_t min_read_length,
                         uint32_t max_read_length, uint64_t *first, char *reads, uint32_t read_stride, uint32_t *read_len, size_t cap_reads,
                         size_t *nreads) {
    return rsb::guarded("rsbwt_set_kmer_reads", [&]() -> int {
        if (!nreads || (!first && Q)) return rsb::fail(RSBWT_EINVAL, "null argument");
        *nreads = 0;
        if (read_stride == 0) return rsb::fail(RSBWT_EINVAL, "read_stride must be positive");
        std::vector<std::vector<std::vector<std::string>>> res;
        const int rc = kmer_set_call(s, text, off, Q, k, skip, min_read_length, max_read_length, &res, std::max<uint32_t>(read_stride, 256));
        if (rc != RSBWT_OK) return rc;
        const size_t S = rsbwt_set_size(s);
        size_t total = 0;
        for (size_t q = 0; q < Q; ++q)
            for (size_t p = 0; p < S; ++p) {
                first[q * S + p] = total;
                total += res[q][p].size();
            }
        first[Q * S] = total;
        *nreads = total;
        if (total > cap_reads) return rsb::fail(RSBWT_ERANGE, "%zu reads, room for %zu", total, cap_reads);
        if (total == 0) return RSBWT_OK;
        if (!reads || !read_len) return rsb::fail(RSBWT_EINVAL, "null argument");
        size_t r = 0;
        for (size_t q = 0; q < Q; ++q)
            for (size_t p = 0; p < S; ++p)
                for (const std::string &x : res[q][p]) {
                    if (x.size() > read_stride) {
                        read_len[r] = 0xFFFFFFFFu;
                    } else {
                        memcpy(reads + r * (size_t)read_stride, x.data(), x.size());
                        read_len[r] = (uint32_t)x.size();
                    }
                    ++r;
                }
        return RSBWT_OK;
    });
}

int rsbwt_set_kmer_count(rsbwt_set_t *s, const char *text, const uint64_t *off, size_t Q, int32_t k, int32_t skip, uint32_t min_read_length,
                         uint32_t max_read_length, uint64_t *counts) {
    return rsb::guarded("rsbwt_set_kmer_count", [&]() -> int {
        if (!counts && Q) return rsb::fail(RSBWT_EINVAL, "null argument");
        std::vector<std::vector<std::vector<std::string>>> res;
        const int rc = kmer_set_call(s, text, off, Q, k, skip, min_read_length, max_read_length, &res, 256);
        if (rc != RSBWT_OK) return rc;
        const size_t S = rsbwt_set_size(s);
        for (size_t q = 0; q < Q; ++q)
            for (size_t p = 0; p < S; ++p) counts[q * S + p] = res[q][p].size();
        return RSBWT_OK;
    });
}

void rsbwt_set_kmer_last_times(double *ms3) {
    if (!ms3) return;
    ms3[0] = kr_last.ms_total;
    ms3[1] = kr_last.ms_device;
    ms3[2] = kr_last.ms_total - kr_last.ms_device;
}

void rsbwt_set_kmer_last_work(uint64_t *work5) {
    if (!work5) return;
    work5[0] = kr_last.candidates;
    work5[1] = kr_last.walked;
    work5[2] = kr_last.lf_steps;
    work5[3] = kr_last.identities;
    work5[4] = kr_last.extracted;
}

}  // extern "C"
