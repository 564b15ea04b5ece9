// sets.hip -- shard sets: the shards one process holds on its GPU(s), searched by one
// call.  Every query goes to every shard (src/service/server.cpp:124,578); per-shard results are only
// concatenated (intervals) or summed (counts) (server.cpp:184-197,404-410).
//
// The shards of one device form a GROUP and are searched by ONE fused launch (search_lines.hip:
// (query, shard) pairs drawn from per-shard pools): the batch is uploaded and packed once per device,
// not once per shard.  Devices are driven concurrently, one host thread each.  With more than one
// device the per-device count sums are reduced onto the first device over RCCL (xGMI) and cross PCIe
// once; interval gathers onto one GPU are offered for GPU-resident consumers
// (rsbwt_set_gather_intervals_dev).  RCCL is bound at run time (dlopen): a single-GPU deployment
// needs no librccl.
#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <new>
#include <string>
#include <thread>
#include <unordered_set>
#include <utility>
#include <vector>

#include "../../include/rsbwt.h"
#include "capi_guard.h"
#include "capi_internal.h"
#include "gt_span_rule.h"
#include "meta_file.h"
#include "sample_codes.h"
#include "service.h"
#include "set_internal.h"

#ifndef RSB_1MM_TABLE_PREPASS_DEFAULT
#define RSB_1MM_TABLE_PREPASS_DEFAULT true
#endif

namespace {

struct rccl_api {
    void *lib = nullptr;
    ncclResult_t (*CommInitAll)(ncclComm_t *, int, const int *) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    ncclResult_t (*Send)(const void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Recv)(void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Reduce)(const void *, void *, size_t, ncclDataType_t, ncclRedOp_t, int, ncclComm_t, hipStream_t) = nullptr;
    const char *(*GetErrorString)(ncclResult_t) = nullptr;
    bool ok = false;
};

rccl_api &rccl() {
    static rccl_api api = [] {
        rccl_api a;
        for (const char *name : {"librccl.so.1", "librccl.so"}) {
            a.lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
            if (a.lib) break;
        }
        if (!a.lib) return a;
#define RCCL_SYM(field, sym) a.field = reinterpret_cast<decltype(a.field)>(dlsym(a.lib, sym))
        RCCL_SYM(CommInitAll, "ncclCommInitAll");
        RCCL_SYM(CommDestroy, "ncclCommDestroy");
        RCCL_SYM(GroupStart, "ncclGroupStart");
        RCCL_SYM(GroupEnd, "ncclGroupEnd");
        RCCL_SYM(Send, "ncclSend");
        RCCL_SYM(Recv, "ncclRecv");
        RCCL_SYM(Reduce, "ncclReduce");
        RCCL_SYM(GetErrorString, "ncclGetErrorString");
#undef RCCL_SYM
        a.ok = a.CommInitAll && a.CommDestroy && a.GroupStart && a.GroupEnd && a.Send && a.Recv && a.Reduce && a.GetErrorString;
        return a;
    }();
    return api;
}

// counts[S][m] -> sum[m]
__global__ void __launch_bounds__(256)
sum_rows_kernel(const uint64_t *__restrict__ rows, uint32_t S, size_t m, uint64_t *__restrict__ sum) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    uint64_t s = 0;
    for (uint32_t r = 0; r < S; ++r) s += rows[(size_t)r * m + i];
    sum[i] = s;
}

int publish_views(rsbwt_set_t *s) {
    for (dev_group *g : s->groups) {
        int rc = use_device(g->device);
        if (rc) return rc;
        std::vector<shard_view> v;
        for (size_t i : g->idx) v.push_back(s->shards[i]->view);
        HIP_OK(hipMemcpy(g->d_views, v.data(), v.size() * sizeof(shard_view), hipMemcpyHostToDevice));
    }
    return RSBWT_OK;
}

int make_groups(rsbwt_set_t *s) {
    for (size_t i = 0; i < s->shards.size(); ++i) {
        rsbwt_t *h = s->shards[i];
        if (!h) return fail(RSBWT_EINVAL, "null shard handle");
        dev_group *g = nullptr;
        for (dev_group *x : s->groups)
            if (x->logical == h->logical_device) g = x;
        if (!g) {
            g = new (std::nothrow) dev_group();
            if (!g) return fail(RSBWT_ENOMEM, "host allocation failed");
            g->device = h->device;
            g->logical = h->logical_device;
            g->num_cus = h->num_cus;
            s->groups.push_back(g);
        }
        g->idx.push_back(i);
    }
    for (dev_group *g : s->groups) {
        int rc = use_device(g->device);
        if (rc) return rc;
        HIP_OK(hipMalloc(&g->d_views, g->idx.size() * sizeof(shard_view)));
        HIP_OK(hipMalloc(&g->d_work, WORK_WORDS * sizeof(unsigned long long)));
        for (int i = 0; i < search_meter::RING; ++i) {
            HIP_OK(hipEventCreate(&g->ev_start[i]));
            HIP_OK(hipEventCreate(&g->ev_stop[i]));
        }
    }
    return publish_views(s);
}

// one communicator per device group, all in this process (ncclCommInitAll); false = no RCCL here
bool ensure_comms(rsbwt_set_t *s) {
    std::lock_guard<std::mutex> lock(s->mu);
    if (s->comms_tried) return s->comms_ok;
    s->comms_tried = true;
    if (s->groups.size() < 2 || !rccl().ok) return false;
    std::vector<int> devs;
    for (dev_group *g : s->groups) {
        // two groups on one GPU (logical devices of the test hook, capi.hip resolve_device): RCCL refuses two ranks
        // on one device, and the set goes the way a box without librccl goes
        if (std::find(devs.begin(), devs.end(), g->device) != devs.end()) return false;
        devs.push_back(g->device);
    }
    std::vector<ncclComm_t> comms(devs.size());
    if (rccl().CommInitAll(comms.data(), (int)devs.size(), devs.data()) != ncclSuccess) return false;
    for (size_t i = 0; i < devs.size(); ++i) s->groups[i]->comm = comms[i];
    s->comms_ok = true;
    return true;
}

// search_extra::narrow for a fused launch over a group's shards: every one of them behind a k-mer table deep enough
// that what is left of a search are steps inside one window (capi_internal.h, view_is_narrow) -- the launch then runs
// one lane per search (search_solo.h)
bool group_is_narrow(const rsbwt_set_t *s, const dev_group *g, uint32_t k) {
    for (size_t i : g->idx)
        if (!view_is_narrow(s->shards[i]->view, k)) return false;
    return !g->idx.empty();
}

// Inside for_each_group, for calls that answer [num_shards][Q] arrays in the set's shard order (b: an optional second
// array): fn(g, a', b') does group gi's work into [S_g][Q] blocks.  When the group's shards sit next to each other in
// the set (the usual map: shard s -> GPU s / 8) those blocks ARE the caller's rows; else they are temporaries whose
// row j is copied to row idx[j].
template <class F>
int group_scatter(rsbwt_set_t *s, size_t gi, size_t Q, uint64_t *a, uint64_t *b, F &&fn) {
    dev_group *g = s->groups[gi];
    int rc = use_device(g->device);
    if (rc) return rc;
    const size_t Sg = g->idx.size(), at = g->idx.front() * Q;
    if (g->idx.back() - g->idx.front() + 1 == Sg) return fn(g, a + at, b ? b + at : nullptr);
    std::vector<uint64_t> ta(Sg * Q), tb(b ? Sg * Q : 0);
    if ((rc = fn(g, ta.data(), b ? tb.data() : nullptr)) != RSBWT_OK) return rc;
    for (size_t j = 0; j < Sg; ++j) {
        memcpy(a + g->idx[j] * Q, ta.data() + j * Q, Q * 8);
        if (b) memcpy(b + g->idx[j] * Q, tb.data() + j * Q, Q * 8);
    }
    return RSBWT_OK;
}

// Group g's share of the caller's (shard_of, rows): the shards as the group numbers them, their rows, and where each
// entry stands in the caller's arrays (ascending)
struct group_share {
    std::vector<uint32_t> shard;
    std::vector<uint64_t> rows;
    std::vector<size_t> pos;
};
group_share share_of_group(const rsbwt_set_t *s, const dev_group *g, const uint32_t *shard_of, const uint64_t *rows, size_t n) {
    std::vector<uint32_t> local(s->shards.size(), ~0u);
    for (size_t j = 0; j < g->idx.size(); ++j) local[g->idx[j]] = (uint32_t)j;
    group_share sh;
    for (size_t i = 0; i < n; ++i)
        if (local[shard_of[i]] != ~0u) {
            sh.shard.push_back(local[shard_of[i]]);
            sh.rows.push_back(rows[i]);
            sh.pos.push_back(i);
        }
    return sh;
}

// The copy back of one extracted read: the kept bytes of cell src of a launch's answers (ho [.][stride], hl, hp) to slot
// dst of the caller's arrays.  A read that did not fit its stride (length 0xFFFFFFFF) brings no bytes and keeps its mark.
void scatter_read(const char *ho, const uint32_t *hl, const uint32_t *hp, size_t src, char *out, uint32_t stride, uint32_t *len,
                  uint32_t *prefix_len, size_t dst) {
    const uint32_t keep = hl[src] == 0xFFFFFFFFu ? 0u : hl[src];
    if (keep) memcpy(out + dst * (size_t)stride, ho + src * (size_t)stride, keep);
    if (len) len[dst] = hl[src];
    if (prefix_len) prefix_len[dst] = hp[src];
}

}  // namespace

static void meta_free(rsbwt_set_t *s);  // the sample tables (below, rsbwt_set_meta_*)

extern "C" {

void rsbwt_set_close(rsbwt_set_t *s) {
    if (!s) return;
    meta_free(s);
    for (dev_group *g : s->groups) {
        (void)hipSetDevice(g->device);
        if (g->d_meta) (void)hipFree(g->d_meta);
        g->pool.destroy();
        if (g->comm && rccl().ok) (void)rccl().CommDestroy(g->comm);
        if (g->d_ktab) {  // shards that outlive the set lose the table that lived in it
            for (size_t i : g->idx)
                if (!s->owns && s->shards[i]) (void)detach_ktab(s->shards[i]);
            (void)hipFree(g->d_ktab);
        }
        for (int i = 0; i < dev_group::FORK; ++i) {
            if (g->fork_st[i]) {
                (void)hipStreamSynchronize(g->fork_st[i]);
                (void)hipStreamDestroy(g->fork_st[i]);
            }
            if (g->join_ev[i]) (void)hipEventDestroy(g->join_ev[i]);
        }
        if (g->fork_ev) (void)hipEventDestroy(g->fork_ev);
        if (g->peer_ready) (void)hipEventDestroy(g->peer_ready);
        if (g->peer_done) (void)hipEventDestroy(g->peer_done);
        if (g->d_views) (void)hipFree(g->d_views);
        if (g->d_xviews) (void)hipFree(g->d_xviews);
        if (g->d_work) (void)hipFree(g->d_work);
        g->scratch.destroy();
        for (int i = 0; i < search_meter::RING; ++i) {
            if (g->ev_start[i]) (void)hipEventDestroy(g->ev_start[i]);
            if (g->ev_stop[i]) (void)hipEventDestroy(g->ev_stop[i]);
        }
        delete g;
    }
    if (s->owns)
        for (rsbwt_t *h : s->shards) rsbwt_close(h);
    delete s;
}

static int rsbwt_set_from_handles_body(rsbwt_t *const *handles, size_t num_shards, rsbwt_set_t **out) {
    if (!out || (!handles && num_shards)) return fail(RSBWT_EINVAL, "null argument");
    *out = nullptr;
    if (num_shards == 0) return fail(RSBWT_EINVAL, "a shard set needs at least one shard");
    if (num_shards > (1u << 16)) return fail(RSBWT_ERANGE, "%zu shards: a set holds at most 65536", num_shards);
    rsbwt_set_t *s = new (std::nothrow) rsbwt_set();
    if (!s) return fail(RSBWT_ENOMEM, "host allocation failed");
    s->owns = false;
    try {
        s->shards.assign(handles, handles + num_shards);
    } catch (...) {
        delete s;
        throw;  // guarded() turns it into RSBWT_ENOMEM
    }
    int rc = make_groups(s);
    if (rc) { rsbwt_set_close(s); return rc; }
    *out = s;
    return RSBWT_OK;
}
int rsbwt_set_from_handles(rsbwt_t *const *handles, size_t num_shards, rsbwt_set_t **out) {
    return guarded("rsbwt_set_from_handles", [&]() -> int { return rsbwt_set_from_handles_body(handles, num_shards, out); });
}


static int rsbwt_set_attach_ktabs_body(rsbwt_set_t *s, uint32_t depth, uint32_t format);
static int rsbwt_set_open_body(const char *const *bwt_paths, size_t num_shards, const int *device_map,
                   uint32_t flags, rsbwt_set_t **out) {
    if (!out || (!bwt_paths && num_shards)) return fail(RSBWT_EINVAL, "null argument");
    *out = nullptr;
    if (num_shards == 0) return fail(RSBWT_EINVAL, "a shard set needs at least one shard");
    if (num_shards > (1u << 16)) return fail(RSBWT_ERANGE, "%zu shards: a set holds at most 65536", num_shards);
    rsbwt_set_t *s = new (std::nothrow) rsbwt_set();
    if (!s) return fail(RSBWT_ENOMEM, "host allocation failed");
    s->owns = true;
    // The k-mer tables of the shards of one GPU share what HBM the lines leave, so with depth "auto"
    // the shards are opened without tables and the depth is chosen per device afterwards.
    const uint32_t T_req = (flags & RSBWT_KTAB_MASK) >> RSBWT_KTAB_SHIFT;
    const uint32_t open_flags = T_req == 0u ? ((flags & ~RSBWT_KTAB_MASK) | RSBWT_KTAB_NONE) : flags;
    for (size_t i = 0; i < num_shards; ++i) {
        rsbwt_t *h = nullptr;
        int rc = rsbwt_open(bwt_paths[i], device_map ? device_map[i] : 0, open_flags, &h);
        if (rc) { rsbwt_set_close(s); return rc; }
        s->shards.push_back(h);
    }
    int rc = make_groups(s);
    // (RSBWT_OPEN_KTAB_GROUPED: the grouped format where it is a level deeper and nearly every T-mer occurs, else plain)
    if (rc == RSBWT_OK && T_req == 0u)
        rc = rsbwt_set_attach_ktabs_body(s, 0, (flags & RSBWT_OPEN_KTAB_GROUPED) ? RSBWT_KTAB_FORMAT_AUTO : RSBWT_KTAB_FORMAT_PLAIN);
    if (rc) { rsbwt_set_close(s); return rc; }
    *out = s;
    return RSBWT_OK;
}
int rsbwt_set_open(const char *const *bwt_paths, size_t num_shards, const int *device_map,
                   uint32_t flags, rsbwt_set_t **out) {
    return guarded("rsbwt_set_open", [&]() -> int { return rsbwt_set_open_body(bwt_paths, num_shards, device_map, flags, out); });
}


// The depth rsbwt_set_attach_ktabs(s, 0) would give the shards of device group g: the deepest T whose
// tables (one per shard of that device without one) fit three quarters of the device's free HBM and leave 8 GiB of it
// (the shards are resident when this is asked: what is free is what the tables and the caller's batch buffers share --
// a third of it, the rule until round 4, left 8 x 20 GB shards at 13-mer tables where 15-mer ones fit), none larger
// than 5/4 of its shard's lines, with 4^T <= the smallest shard's length; at most 16 (grouped: 17); 0 = none.
// *fmt: in = the format asked for (KTAB_PLAIN / KTAB_GROUPED), out = the one to build (auto_ktab_depth_for).
static uint32_t auto_ktab_depth(rsbwt_set_t *s, dev_group *g, uint32_t *fmt, uint64_t keep_free = 0) {
    if (use_device(g->device)) return 0;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = 0;
    uint64_t min_n = ~0ull, min_bytes = ~0ull, need = 0;
    for (size_t i : g->idx) {
        const rsbwt_t *h = s->shards[i];
        if (h->view.ktab || h->view.n == 0) continue;
        ++need;
        min_n = std::min(min_n, h->view.n);
        min_bytes = std::min(min_bytes, h->hbm_bytes);
    }
    if (!need) return 0;
    // (keep_free: what the caller wants left of the free HBM; 0 = the set's own rule, a quarter of it and at least 8 GiB)
    const uint64_t keep = keep_free ? keep_free : std::max<uint64_t>(8ull << 30, free_b / 4);
    const uint64_t budget = std::min<uint64_t>(min_bytes + min_bytes / 4, (free_b > keep ? free_b - keep : 0) / need);
    return auto_ktab_depth_for(budget, min_n, fmt);
}

// THE table-sizing rule, for every caller (rsbwt_set_open, rsbwt_set_attach_ktabs*(depth 0), bench.py, onehost.py --
// until round 5 bench.py restated it in Python and rsbwt_set_auto_ktab_depth answered for the plain format only):
// the depth and the format the shards of the set that have no table yet would get, one pair for the whole set (the
// shallowest over its devices; plain if any device must).  format_in: RSBWT_KTAB_FORMAT_PLAIN / _GROUPED / _AUTO
// (grouped where that is deeper and its records can say what four siblings hold).
int rsbwt_set_auto_ktab(rsbwt_set_t *s, uint32_t format_in, uint64_t keep_free_bytes, uint32_t *depth, uint32_t *format_out) {
    if (!s || !depth || !format_out) return fail(RSBWT_EINVAL, "null argument");
    if (format_in > RSBWT_KTAB_FORMAT_AUTO) return fail(RSBWT_EINVAL, "k-mer table format %u", format_in);
    uint32_t T = ~0u, F = KTAB_GROUPED;
    for (dev_group *g : s->groups) {
        uint32_t fmt = format_in == RSBWT_KTAB_FORMAT_PLAIN ? KTAB_PLAIN : KTAB_GROUPED;
        const uint32_t t = auto_ktab_depth(s, g, &fmt, keep_free_bytes);
        if (t < T || (t == T && fmt == KTAB_PLAIN)) {
            if (t < T) F = fmt;
            else F = KTAB_PLAIN;
            T = t;
        }
    }
    if (T == ~0u) T = 0;
    // one format for the set: a device that must take the plain format at the common depth decides it
    if (F == KTAB_GROUPED)
        for (dev_group *g : s->groups) {
            uint64_t min_n = ~0ull;
            for (size_t i : g->idx)
                if (!s->shards[i]->view.ktab && s->shards[i]->view.n) min_n = std::min(min_n, s->shards[i]->view.n);
            if (min_n != ~0ull && !ktab_grouped_sensible(min_n, T)) F = KTAB_PLAIN;
        }
    *depth = T;
    *format_out = T >= 2u ? (F == KTAB_GROUPED ? RSBWT_KTAB_FORMAT_GROUPED : RSBWT_KTAB_FORMAT_PLAIN) : RSBWT_KTAB_FORMAT_PLAIN;
    return RSBWT_OK;
}

uint32_t rsbwt_set_auto_ktab_depth(rsbwt_set_t *s) {  // (the plain format's depth: rsbwt_set_auto_ktab names the format too)
    uint32_t T = 0, F = 0;
    return rsbwt_set_auto_ktab(s, RSBWT_KTAB_FORMAT_PLAIN, 0, &T, &F) == RSBWT_OK ? T : 0u;
}

// Builds the k-mer tables of the shards that have none.  depth 0 = per device, auto_ktab_depth.  The
// tables of one device are interleaved in one allocation of the set (line_format.h): the start
// records of a query for all shards come out of one stretch of 8 x shards (grouped: 12 x shards) bytes.
// format: RSBWT_KTAB_FORMAT_PLAIN / _GROUPED / _AUTO (grouped where the smallest shard's groups fit their records).
static int rsbwt_set_attach_ktabs_body(rsbwt_set_t *s, uint32_t depth, uint32_t format) {
    if (!s) return fail(RSBWT_EINVAL, "null set");
    if (format > RSBWT_KTAB_FORMAT_AUTO) return fail(RSBWT_EINVAL, "k-mer table format %u", format);
    for (dev_group *g : s->groups) {
        if (g->d_ktab) continue;
        std::vector<size_t> need;
        uint64_t min_n = ~0ull;
        for (size_t i : g->idx)
            if (!s->shards[i]->view.ktab && s->shards[i]->view.n) {
                need.push_back(i);
                min_n = std::min(min_n, s->shards[i]->view.n);
            }
        if (need.empty()) continue;
        uint32_t fmt = format == RSBWT_KTAB_FORMAT_PLAIN ? KTAB_PLAIN : KTAB_GROUPED;
        uint32_t T = depth;
        if (T == 0u) T = auto_ktab_depth(s, g, &fmt);
        else if (format == RSBWT_KTAB_FORMAT_AUTO && !ktab_grouped_sensible(min_n, T)) fmt = KTAB_PLAIN;
        if (T < 2u) continue;
        const uint32_t Tmax = fmt == KTAB_GROUPED ? KTAB_MAX_DEPTH_GROUPED : KTAB_MAX_DEPTH_PLAIN;
        if (T > Tmax) T = Tmax;
        int rc = use_device(g->device);
        if (rc) return rc;
        const uint64_t per = fmt == KTAB_GROUPED ? KTAB_GROUP_BYTES : 8u;  // bytes of one shard's entry / record in a stretch
        hipError_t e = hipMalloc(&g->d_ktab, ktab_bytes(fmt, T) * need.size());
        if (e != hipSuccess) return fail_hip(e, "allocating the k-mer tables");
        for (size_t j = 0; j < need.size(); ++j) {
            rsbwt_t *h = s->shards[need[j]];
            rc = attach_ktab_into(h, T, reinterpret_cast<uint64_t *>(reinterpret_cast<char *>(g->d_ktab) + j * per), (uint32_t)need.size(), fmt);
            if (rc) return rc;
            h->ktab_owned = false;
        }
    }
    return publish_views(s);
}
int rsbwt_set_attach_ktabs(rsbwt_set_t *s, uint32_t depth) {
    return guarded("rsbwt_set_attach_ktabs", [&]() -> int { return rsbwt_set_attach_ktabs_body(s, depth, RSBWT_KTAB_FORMAT_PLAIN); });
}
int rsbwt_set_attach_ktabs_format(rsbwt_set_t *s, uint32_t depth, uint32_t format) {
    return guarded("rsbwt_set_attach_ktabs_format", [&]() -> int { return rsbwt_set_attach_ktabs_body(s, depth, format); });
}


size_t rsbwt_set_size(const rsbwt_set_t *s) { return s ? s->shards.size() : 0; }
rsbwt_t *rsbwt_set_shard(rsbwt_set_t *s, size_t i) { return (s && i < s->shards.size()) ? s->shards[i] : nullptr; }
size_t rsbwt_set_devices(const rsbwt_set_t *s) { return s ? s->groups.size() : 0; }

// Host buffers.  lower/upper: [num_shards][Q] in the set's shard order.
static int rsbwt_set_find_intervals_body(rsbwt_set_t *s, const char *kmers, size_t Q, uint32_t k, size_t stride,
                             uint64_t *lower, uint64_t *upper) {
    if (!s) return fail(RSBWT_EINVAL, "null set");
    if (Q == 0) return RSBWT_OK;
    if (!kmers || !lower || !upper) return fail(RSBWT_EINVAL, "null argument");
    if (stride < k) return fail(RSBWT_EINVAL, "stride %zu < k %u", stride, k);
    const size_t S = s->shards.size();
    if (k == 0) {
        for (size_t i = 0; i < S * Q; ++i) { lower[i] = 1; upper[i] = 0; }
        return RSBWT_OK;
    }
    for (rsbwt_t *h : s->shards)
        if (h->view.n == 0) return fail(RSBWT_EINVAL, "empty index in the set");
    return for_each_group(s, [&](size_t gi) -> int {
        return group_scatter(s, gi, Q, lower, upper, [&](dev_group *g, uint64_t *lo, uint64_t *up) -> int {
            return search_host_views(*g, g->pool, g->d_views, (uint32_t)g->idx.size(), g->num_cus, kmers, Q, k, stride, lo, up, false,
                                     group_is_narrow(s, g, k));
        });
    });
}
int rsbwt_set_find_intervals(rsbwt_set_t *s, const char *kmers, size_t Q, uint32_t k, size_t stride,
                             uint64_t *lower, uint64_t *upper) {
    return guarded("rsbwt_set_find_intervals", [&]() -> int { return rsbwt_set_find_intervals_body(s, kmers, Q, k, stride, lower, upper); });
}

// Queries of lengths of their own: query q = text[off[q] .. off[q+1]) -- a window of the service loop in ONE search
// (search_lines.hip, search_init_var_kernel).  lower / upper: [num_shards][Q]; an empty query, one with a symbol
// outside ACGT or one longer than 65,535 symbols ends as (1, 0).
static int rsbwt_set_find_intervals_var_body(rsbwt_set_t *s, const char *text, const uint64_t *off, size_t Q, uint64_t *lower,
                                             uint64_t *upper, bool counts_only) {
    if (!s) return fail(RSBWT_EINVAL, "null set");
    if (Q == 0) return RSBWT_OK;
    if (!off || !lower || (!upper && !counts_only) || (!text && off[Q] != off[0])) return fail(RSBWT_EINVAL, "null argument");
    for (rsbwt_t *h : s->shards)
        if (h->view.n == 0) return fail(RSBWT_EINVAL, "empty index in the set");
    uint64_t kmax = 0;
    for (size_t q = 0; q < Q; ++q)
        if (off[q + 1] >= off[q] && off[q + 1] - off[q] <= 65535ull) kmax = std::max(kmax, off[q + 1] - off[q]);
    return for_each_group(s, [&](size_t gi) -> int {
        return group_scatter(s, gi, Q, lower, counts_only ? nullptr : upper, [&](dev_group *g, uint64_t *lo, uint64_t *up) -> int {
            return search_host_views_var(*g, g->pool, g->d_views, (uint32_t)g->idx.size(), g->num_cus, text, off, Q, lo, up, counts_only,
                                         kmax != 0 && group_is_narrow(s, g, (uint32_t)kmax));
        });
    });
}
int rsbwt_set_find_intervals_var(rsbwt_set_t *s, const char *text, const uint64_t *off, size_t Q, uint64_t *lower, uint64_t *upper) {
    return guarded("rsbwt_set_find_intervals_var", [&]() -> int { return rsbwt_set_find_intervals_var_body(s, text, off, Q, lower, upper, false); });
}
// counts[Q] summed over the set's shards (what rsbwt_set_count gives for one length); the sum is made on the host
int rsbwt_set_count_var(rsbwt_set_t *s, const char *text, const uint64_t *off, size_t Q, uint64_t *counts) {
    return guarded("rsbwt_set_count_var", [&]() -> int {
        if (!s || (!counts && Q)) return fail(RSBWT_EINVAL, "null argument");
        if (Q == 0) return RSBWT_OK;
        const size_t S = s->shards.size();
        std::vector<uint64_t> c(S * Q);
        const int rc = rsbwt_set_find_intervals_var_body(s, text, off, Q, c.data(), nullptr, true);
        if (rc) return rc;
        for (size_t q = 0; q < Q; ++q) {
            uint64_t t = 0;
            for (size_t i = 0; i < S; ++i) t += c[i * Q + q];
            counts[q] = t;
        }
        return RSBWT_OK;
    });
}

// Whole-read matches of queries of lengths of their own (read_lookup.hip): copies / ending [num_shards][Q] in the set's
// shard order, per device group one launch sequence over its shards, sliced as rsbwt_set_count_var is (for_each_var_slice).
static int rsbwt_set_read_copies_var_body(rsbwt_set_t *s, const char *text, const uint64_t *off, size_t Q, uint64_t *copies,
                                          uint64_t *ending, uint64_t *ordinal = nullptr, std::atomic<uint64_t> *lf_steps = nullptr) {
    if (!s) return fail(RSBWT_EINVAL, "null set");
    if (Q == 0) return RSBWT_OK;
    if (!off || !copies || (!text && off[Q] != off[0])) return fail(RSBWT_EINVAL, "null argument");
    for (rsbwt_t *h : s->shards)
        if (h->view.n == 0) return fail(RSBWT_EINVAL, "empty index in the set");
    if (ordinal) {  // (group_scatter carries two arrays: the ordinals ride in the second one's place)
        if (ending) return fail(RSBWT_EINVAL, "ordinal and ending in one call");
        return for_each_group(s, [&](size_t gi) -> int {
            return group_scatter(s, gi, Q, copies, ordinal, [&](dev_group *g, uint64_t *cp, uint64_t *od) -> int {
                uint64_t steps = 0;
                const int rc = read_copies_host_views_var(*g, g->pool, g->d_views, (uint32_t)g->idx.size(), g->num_cus, text, off, Q, cp, nullptr, od,
                                                          lf_steps ? &steps : nullptr);
                if (lf_steps) *lf_steps += steps;
                return rc;
            });
        });
    }
    return for_each_group(s, [&](size_t gi) -> int {
        return group_scatter(s, gi, Q, copies, ending, [&](dev_group *g, uint64_t *cp, uint64_t *en) -> int {
            return read_copies_host_views_var(*g, g->pool, g->d_views, (uint32_t)g->idx.size(), g->num_cus, text, off, Q, cp, en);
        });
    });
}
int rsbwt_set_read_copies_var(rsbwt_set_t *s, const char *text, const uint64_t *off, size_t Q, uint64_t *copies, uint64_t *ending) {
    return guarded("rsbwt_set_read_copies_var", [&]() -> int { return rsbwt_set_read_copies_var_body(s, text, off, Q, copies, ending); });
}
// rsbwt_exactmatch_by_search on every shard of the set
int rsbwt_set_exactmatch_by_search(rsbwt_set_t *s, int on) {
    if (!s) return fail(RSBWT_EINVAL, "null set");
    for (rsbwt_t *h : s->shards) {
        const int rc = rsbwt_exactmatch_by_search(h, on);
        if (rc) return rc;
    }
    return RSBWT_OK;
}


// counts[Q] summed over the set's shards, the way the front-end sums per-partition replies
// (src/service/server.cpp:184-197): per device one fused search + a row sum; the per-device sums
// are reduced onto the first device over RCCL when there are several, and cross PCIe once.
static int rsbwt_set_count_body(rsbwt_set_t *s, const char *kmers, size_t Q, uint32_t k, size_t stride, uint64_t *counts) {
    if (!s || (!counts && Q)) return fail(RSBWT_EINVAL, "null argument");
    if (Q == 0) return RSBWT_OK;
    if (!kmers) return fail(RSBWT_EINVAL, "null argument");
    if (stride < k) return fail(RSBWT_EINVAL, "stride %zu < k %u", stride, k);
    if (k == 0) {
        for (size_t q = 0; q < Q; ++q) counts[q] = 0;
        return RSBWT_OK;
    }
    if (k > 65535u) return fail(RSBWT_ERANGE, "k %u: at most 65535 symbols per k-mer", k);
    for (rsbwt_t *h : s->shards)
        if (h->view.n == 0) return fail(RSBWT_EINVAL, "empty index in the set");
    const size_t G = s->groups.size();
    const bool use_rccl = G > 1 && ensure_comms(s);
    const uint32_t wpq = words_per_kmer(k);
    const size_t SLICE = 1u << 20;
    std::vector<std::vector<uint64_t>> part(use_rccl ? 0 : G);
    for (size_t q0 = 0; q0 < Q; q0 += SLICE) {
        const size_t m = std::min(SLICE, Q - q0);
        std::vector<call_ctx *> ctx(G, nullptr);
        std::vector<uint64_t *> d_sum(G, nullptr);
        // phase 1, per device concurrently: upload, pack, fused count search, row sum
        int rc = for_each_group(s, [&](size_t gi) -> int {
            dev_group *g = s->groups[gi];
            int r = use_device(g->device);
            if (r) return r;
            call_ctx *c = g->pool.acquire();
            if (!c) return fail(RSBWT_EHIP, "cannot create a HIP stream");
            ctx[gi] = c;
            const size_t Sg = g->idx.size();
            const size_t ascii_bytes = (m - 1) * stride + k;
            const size_t a_ascii = (ascii_bytes + 15) & ~(size_t)15, a_pk = (m * wpq * 8 + 15) & ~(size_t)15, a_ok = (m + 15) & ~(size_t)15;
            if ((r = c->stage(a_ascii + a_pk + a_ok + (Sg + 2) * m * 8)) != RSBWT_OK) return r;
            uint8_t *d_ascii = (uint8_t *)c->d_stage, *d_pk = d_ascii + a_ascii, *d_ok = d_pk + a_pk;
            uint64_t *d_cnt = (uint64_t *)(d_ok + a_ok);
            d_sum[gi] = d_cnt + Sg * m;  // followed by m more words: the reduced total on the root
            hipStream_t st = c->st[0];
            HIP_OK(hipMemcpyAsync(d_ascii, kmers + q0 * stride, ascii_bytes, hipMemcpyHostToDevice, st));
            hipError_t e = launch_pack(d_ascii, m, k, stride, d_pk, d_ok, st);
            if (e != hipSuccess) return fail_hip(e, "pack kernel launch");
            search_extra ex;
            ex.narrow = group_is_narrow(s, g, k);
            r = search_launch(*g, g->d_views, (uint32_t)Sg, g->num_cus, d_pk, d_ok, m, k, d_cnt, nullptr, true, st, &ex);
            if (r) return r;
            hipLaunchKernelGGL(sum_rows_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, d_cnt, (uint32_t)Sg, m, d_sum[gi]);
            HIP_OK(hipGetLastError());
            if (!use_rccl) {
                part[gi].resize(m);
                HIP_OK(hipMemcpyAsync(part[gi].data(), d_sum[gi], m * 8, hipMemcpyDeviceToHost, st));
                HIP_OK(hipStreamSynchronize(st));
            }
            return RSBWT_OK;
        });
        // phase 2: one sum over the devices
        if (rc == RSBWT_OK && use_rccl) {
            std::lock_guard<std::mutex> comm_lock(s->comm_mu);
            ncclResult_t nr = rccl().GroupStart();
            for (size_t gi = 0; gi < G && nr == ncclSuccess; ++gi) {
                (void)hipSetDevice(s->groups[gi]->device);
                nr = rccl().Reduce(d_sum[gi], d_sum[gi] + m, m, ncclUint64, ncclSum, 0, s->groups[gi]->comm, ctx[gi]->st[0]);
            }
            const ncclResult_t ne = rccl().GroupEnd();
            if (nr == ncclSuccess) nr = ne;
            if (nr != ncclSuccess) rc = fail(RSBWT_EHIP, "ncclReduce: %s", rccl().GetErrorString(nr));
            if (rc == RSBWT_OK) {
                (void)hipSetDevice(s->groups[0]->device);
                hipError_t e = hipMemcpyAsync(counts + q0, d_sum[0] + m, m * 8, hipMemcpyDeviceToHost, ctx[0]->st[0]);
                for (size_t gi = 0; gi < G && e == hipSuccess; ++gi) {
                    (void)hipSetDevice(s->groups[gi]->device);
                    e = hipStreamSynchronize(ctx[gi]->st[0]);
                }
                if (e != hipSuccess) rc = fail_hip(e, "count reduction");
            }
        } else if (rc == RSBWT_OK) {
            for (size_t i = 0; i < m; ++i) {
                uint64_t t = 0;
                for (size_t gi = 0; gi < G; ++gi) t += part[gi][i];
                counts[q0 + i] = t;
            }
        }
        for (size_t gi = 0; gi < G; ++gi)
            if (ctx[gi]) {
                (void)hipSetDevice(s->groups[gi]->device);
                (void)hipStreamSynchronize(ctx[gi]->st[0]);
                s->groups[gi]->pool.release(ctx[gi]);
            }
        if (rc) return rc;
    }
    return RSBWT_OK;
}
int rsbwt_set_count(rsbwt_set_t *s, const char *kmers, size_t Q, uint32_t k, size_t stride, uint64_t *counts) {
    return guarded("rsbwt_set_count", [&]() -> int { return rsbwt_set_count_body(s, kmers, Q, k, stride, counts); });
}


// Device-resident, for a set whose shards all sit on one device: one fused launch on `stream`;
// d_lower/d_upper: [num_shards][Q].  Nothing is synchronised.
int rsbwt_set_find_intervals_dev(rsbwt_set_t *s, const void *d_packed, const void *d_valid, size_t Q, uint32_t k,
                                 void *d_lower, void *d_upper, void *stream) {
    dev_group *g = nullptr;
    int rc = one_device_group(s, &g);
    if (rc) return rc;
    search_extra ex;
    ex.narrow = group_is_narrow(s, g, k);
    return search_launch(*g, g->d_views, (uint32_t)g->idx.size(), g->num_cus, d_packed, d_valid, Q, k, d_lower, d_upper,
                         false, (hipStream_t)stream, &ex);
}

int rsbwt_set_find_interval_pairs_dev(rsbwt_set_t *s, const void *d_packed, const void *d_valid, size_t Q, uint32_t k,
                                      void *d_pairs, void *stream) {
    dev_group *g = nullptr;
    int rc = one_device_group(s, &g);
    if (rc) return rc;
    search_extra ex;
    ex.pairs = true;
    ex.narrow = group_is_narrow(s, g, k);
    return search_launch(*g, g->d_views, (uint32_t)g->idx.size(), g->num_cus, d_packed, d_valid, Q, k, d_pairs, nullptr,
                         false, (hipStream_t)stream, &ex);
}

// The same search in two halves, so that a pipelined caller can compute the start records of batch i + 1 on a
// second stream while batch i is searched (they depend on the batch's k-mers and the k-mer tables only):
// rsbwt_set_prepare_dev fills d_records ([num_shards][Q] x 16 B) on `stream`; the caller orders it before
// rsbwt_set_find_interval_pairs_prepared_dev (an event, or the same stream), which runs the search kernel alone.
size_t rsbwt_set_records_bytes(const rsbwt_set_t *s, size_t Q) { return s ? s->shards.size() * Q * 16 : 0; }

int rsbwt_set_prepare_dev(rsbwt_set_t *s, const void *d_packed, const void *d_valid, size_t Q, uint32_t k, void *d_records,
                          void *stream) {
    dev_group *g = nullptr;
    int rc = one_device_group(s, &g);
    if (rc) return rc;
    if (Q == 0) return RSBWT_OK;
    if (!d_packed || !d_valid || !d_records) return fail(RSBWT_EINVAL, "null argument");
    if (k == 0 || k > 65535u) return fail(RSBWT_ERANGE, "k %u: 1..65535 symbols per k-mer", k);
    const hipError_t e = launch_search_init(g->d_views, (uint32_t)g->idx.size(), d_packed, d_valid, Q, k, d_records, (hipStream_t)stream);
    return e == hipSuccess ? RSBWT_OK : fail_hip(e, "start-record kernel launch");
}

int rsbwt_set_find_interval_pairs_prepared_dev(rsbwt_set_t *s, const void *d_packed, const void *d_valid, const void *d_records,
                                               size_t Q, uint32_t k, void *d_pairs, void *stream) {
    dev_group *g = nullptr;
    int rc = one_device_group(s, &g);
    if (rc) return rc;
    if (Q && !d_records) return fail(RSBWT_EINVAL, "null argument");
    search_extra ex;
    ex.pairs = true;
    ex.d_init = d_records;
    ex.narrow = group_is_narrow(s, g, k);
    return search_launch(*g, g->d_views, (uint32_t)g->idx.size(), g->num_cus, d_packed, d_valid, Q, k, d_pairs, nullptr,
                         false, (hipStream_t)stream, &ex);
}

int rsbwt_set_count_dev(rsbwt_set_t *s, const void *d_packed, const void *d_valid, size_t Q, uint32_t k,
                        void *d_counts, void *stream) {
    dev_group *g = nullptr;
    int rc = one_device_group(s, &g);
    if (rc) return rc;
    search_extra ex;
    ex.narrow = group_is_narrow(s, g, k);
    return search_launch(*g, g->d_views, (uint32_t)g->idx.size(), g->num_cus, d_packed, d_valid, Q, k, d_counts, nullptr,
                         true, (hipStream_t)stream, &ex);
}

// Device-resident forms for a set on ONE device (one process per GPU drives its shards this way: bench.py).
// Three ways, best first: (1) all the shards in ONE traced and ONE resumed launch (fused_1mm_applies, below: tables of
// one depth); (2) else side by side; (3) at or above 2^26 variant searches per shard the shards take turns on the
// stream: each turn is a batch large enough to fill the GPU by itself.
// Below this many variant searches per shard (2^26 = 7e5 31-mers; a scratch per shard is what bounds it) the shards of
// the set work SIDE BY SIDE, each on a stream of its own with a scratch of its own (forked from and joined to the
// caller's stream with events), instead of taking turns: a shard's own sequence -- variants, start records, the traced
// and the resumed search, three small compaction launches -- leaves gaps and tails another shard's kernels fill
// (8 resident 20 GB shards, per batch: 4e4 31-mers 5.7 -> 4.3 ms, 1e5 9.4 -> 7.8, 4e5 30.7 -> 27.9:
// profiles/r03_set_side_by_side.json).
static size_t side_by_side_below() {
    static const size_t v = (size_t)1 << knob_int("RSBWT_SET_1MM_SIDE_LOG2", 10, 40, 26);  // A/B knob (tools/README.md)
    return v;
}
#define SIDE_BY_SIDE_BELOW side_by_side_below()

// ONE launch sequence for all the shards of the device (below the same size): the k-mers traced in every shard by one
// fused launch (traces [S][m][tn]), their variants resumed in every shard by another (sparse results [S][mv], hit maps
// [S][hit_map_words(mv)]), one three-launch compaction with a segment per shard.  A (31-mer x shard) search is then
// one of S * m * (3k+1) in a launch that fills the GPU where a shard's own m * (3k+1) do not, and the set's tails
// are one tail.  Needs what the fused exact search needs -- one device -- and one trace length for all shards (k-mer
// tables of one depth: rsbwt_set_attach_ktabs gives every shard of a device the same).
// The table entries of the variants inside the tables' reach are read ahead for all shards by a kernel of their own
// (mm1_worklist.hip, wl_table_entries_kernel) instead of by the search kernel's lanes: the S shards' records of a variant
// are ONE stretch of the interleaved tables, which S waves on S XCDs otherwise fetch S times (round 5: 14.07 -> 13.60 ms
// per 4e5 31-mers x 8 shards, 1.74 -> 1.69 at 4e4; round 4 measured the same idea 2 % SLOWER -- the search kernel it
// relieved was then bound by instruction issue, not by requests).  RSBWT_SET_1MM_TABLE_PREPASS=0: A/B knob (tools/README.md)
static bool table_prepass() {
    static const bool on = knob_int("RSBWT_SET_1MM_TABLE_PREPASS", INT_MIN, INT_MAX, RSB_1MM_TABLE_PREPASS_DEFAULT) != 0;
    return on;
}
struct fused_1mm_layout {
    uint32_t tn;
    size_t trace, own, sparse, bits, blocks, total;  // byte sizes of the parts behind the variants, each 256-aligned
    // the hit lists by WORKLIST (mm1_worklist.hip): k <= 32 with something left of the tables' reach -- the variants'
    // searches are records of live searches (a record per variant at most), no variants spelled out, no start records
    bool worklist;
    size_t wl_cap, wl, counts;
    size_t pre;  // the table-part variants' entries read ahead for all shards (RSBWT_SET_1MM_TABLE_PREPASS): u64 [S][m * 3 (k - tn)], or 0
};
static bool fused_1mm_applies(const rsbwt_set_t *s, size_t m, uint32_t k, fused_1mm_layout *L, bool dense = false) {
    static const bool off = knob_set("RSBWT_SET_1MM_UNFUSED");  // A/B knob (tools/README.md)
    const size_t S = s->shards.size(), mv = m * (3 * (size_t)k + 1);
    if (off || S < 2 || S > 1024 || s->groups.size() != 1 || mv >= SIDE_BY_SIDE_BELOW || k > 32767u) return false;  // (S: a grid row per shard)
    const uint32_t tn = trace_entries(s->shards[0]->view, k);
    for (const rsbwt_t *h : s->shards)
        if (trace_entries(h->view, k) != tn || h->view.n == 0) return false;
    auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
    L->tn = tn;
    L->sparse = al(S * mv * 16);
    L->bits = al(S * hit_map_words(mv) * 8);
    L->blocks = al(S * compact_hits_block_words(mv) * 8);
    static const bool no_worklist = knob_set("RSBWT_SET_1MM_NO_WORKLIST");  // A/B knob (tools/README.md): round 3's launches
    static const bool no_walk = knob_set("RSBWT_SET_1MM_NO_WALK");          // A/B knob: the traced launch + the branch kernel
    L->worklist = !no_worklist && tn > 0 && tn < k && k <= 32u && m * (size_t)tn < 0xFFFFFFFFull;
    // the trace ([S][m][tn] intervals) and the k-mers' own intervals are what the TRACED launch leaves: the default
    // worklist path walks the k-mers instead (search_solo.h, WALK) and touches neither (0.87 GB of scratch at 4e5
    // 31-mers x 8 shards that the tables can have: ADVICE r04)
    // (dense: rsbwt_set_find_intervals_1mm_dev's [S][m][3k+1] matrices -- always the traced and the resumed launch)
    const bool traced = dense || !L->worklist || no_walk;
    L->trace = traced ? al(S * m * (size_t)tn * 16) : 0;
    L->own = traced && tn ? al(S * m * 16) : 0;  // the k-mers' own intervals ({lower, upper}[S][m]: nobody reads them)
    L->wl_cap = L->worklist ? m * 3u * (size_t)tn : 0;  // (a record per variant substituted left of the tables' reach, at most)
    L->wl = L->worklist ? al(S * L->wl_cap * 32) : 0;
    L->counts = L->worklist ? al(S * 8 * (size_t)WL_COUNT_STRIDE) : 0;
    L->pre = (L->worklist && table_prepass() && S <= 256) ? al(S * m * 3u * (size_t)(k - tn) * 8) : 0;
    L->total = L->trace + L->own + L->sparse + L->bits + L->blocks + L->wl + L->counts + L->pre;
    return true;
}

// The two fused launches: the k-mers traced in every shard (when the tables leave something to trace), then their
// variants (expanded at d_var: variants_of_batch_dev's layout) resumed in every shard.  d_bits != nullptr: sparse
// results at d_lower + the hit maps; else dense [S][m][3k+1] lower and upper.
static int fused_1mm_launches(rsbwt_set_t *s, dev_group *g, const fused_1mm_layout &L, const void *d_packed, const void *d_valid,
                              size_t m, uint32_t k, const uint8_t *d_var, uint8_t *d_trace, uint8_t *d_own, void *d_lower,
                              void *d_upper, void *d_bits, hipStream_t st) {
    const uint32_t S = (uint32_t)s->shards.size();
    const size_t V = 3 * (size_t)k + 1, mv = m * V;
    const uint8_t *d_vok = d_var + ((mv * words_per_kmer(k) * 8 + 15) & ~(size_t)15);
    search_extra resumed;
    if (L.tn) {
        search_extra traced;
        traced.d_trace_out = d_trace;
        traced.trace_n = L.tn;
        traced.pairs = true;
        const int rc = search_launch(*g, g->d_views, S, g->num_cus, d_packed, d_valid, m, k, d_own, nullptr, false, st, &traced);
        if (rc) return rc;
        resumed.d_trace_in = d_trace;
        resumed.trace_n = L.tn;
        resumed.variants = (uint32_t)V;
    }
    resumed.d_hit_bits = d_bits;
    return search_launch(*g, g->d_views, S, g->num_cus, d_var, d_vok, mv, k, d_lower, d_upper, false, st, &resumed);
}

// 1-mismatch search over the shards of a one-device set: the fused launches above where they apply (dense
// results: the resumed launch writes [S][m][3k+1] lower and upper itself), else the shards take turns on the stream,
// each turn m x (3k+1) searches of one shard.
size_t rsbwt_set_1mm_scratch_bytes(const rsbwt_set_t *s, size_t m, uint32_t k) {
    size_t need = 0;
    if (!s) return 0;
    for (rsbwt_t *h : s->shards) need = std::max(need, rsbwt_1mm_scratch_bytes(h, m, k));
    fused_1mm_layout L;
    if (fused_1mm_applies(s, m, k, &L, true)) need = std::max(need, ((variants_bytes(m, k) + 255) & ~(size_t)255) + L.trace + L.own);
    return need;
}

static int rsbwt_set_find_intervals_1mm_dev_body(rsbwt_set_t *s, const void *d_packed, const void *d_valid, size_t m, uint32_t k,
                                     void *d_lower, void *d_upper, void *d_scratch, void *stream) {
    dev_group *g = nullptr;
    int rc = one_device_group(s, &g);
    if (rc) return rc;
    if (m == 0) return RSBWT_OK;
    if (!d_lower || !d_upper) return fail(RSBWT_EINVAL, "null argument");
    const size_t row = m * (3 * (size_t)k + 1) * 8;
    fused_1mm_layout L;
    if (fused_1mm_applies(s, m, k, &L, true)) {
        if (!d_packed || !d_valid || !d_scratch) return fail(RSBWT_EINVAL, "null argument");
        uint8_t *d_var = (uint8_t *)d_scratch, *d_trace = d_var + ((variants_bytes(m, k) + 255) & ~(size_t)255), *d_own = d_trace + L.trace;
        if ((rc = variants_of_batch_dev(d_packed, d_valid, m, k, d_var, (hipStream_t)stream)) != RSBWT_OK) return rc;
        return fused_1mm_launches(s, g, L, d_packed, d_valid, m, k, d_var, d_trace, d_own, d_lower, d_upper, nullptr, (hipStream_t)stream);
    }
    for (size_t i = 0; i < s->shards.size(); ++i) {
        rc = rsbwt_find_intervals_1mm_dev(s->shards[i], d_packed, d_valid, m, k, (uint8_t *)d_lower + i * row,
                                          (uint8_t *)d_upper + i * row, d_scratch, stream);
        if (rc) return rc;
    }
    return RSBWT_OK;
}
int rsbwt_set_find_intervals_1mm_dev(rsbwt_set_t *s, const void *d_packed, const void *d_valid, size_t m, uint32_t k,
                                     void *d_lower, void *d_upper, void *d_scratch, void *stream) {
    return guarded("rsbwt_set_find_intervals_1mm_dev", [&]() -> int { return rsbwt_set_find_intervals_1mm_dev_body(s, d_packed, d_valid, m, k, d_lower, d_upper, d_scratch, stream); });
}


// Gathers per-device interval blocks onto the first device of the set over RCCL (xGMI): d_blocks[g]
// = device g's [S_g][Q] x {lower, upper} block of `bytes[g]` bytes on that device; d_root on device 0
// receives them back to back in device order.  One call per batch; nothing is synchronised beyond
// the streams given (streams[g] on device g).  With one device it is a device-to-device copy.
static int rsbwt_set_gather_intervals_dev_body(rsbwt_set_t *s, const void *const *d_blocks, const size_t *bytes, void *d_root,
                                   void *const *streams) {
    if (!s || !d_blocks || !bytes || !d_root || !streams) return fail(RSBWT_EINVAL, "null argument");
    const size_t G = s->groups.size();
    (void)hipSetDevice(s->groups[0]->device);
    HIP_OK(hipMemcpyAsync(d_root, d_blocks[0], bytes[0], hipMemcpyDeviceToDevice, (hipStream_t)streams[0]));
    if (G == 1) return RSBWT_OK;
    size_t off = bytes[0];
    std::lock_guard<std::mutex> comm_lock(s->comm_mu);
    if (!ensure_comms(s)) {
        // No RCCL (no librccl on the box, or groups that share a GPU): the root PULLS every block with a peer copy
        // on its own stream, behind an event the block's stream records ("ready"), and tells that stream when the
        // block has been read ("done") -- the stream order ncclSend / ncclRecv would have given.  xGMI peer copies
        // by the copy engines; slower to start than one grouped RCCL call, the same bytes over the same links.
        static const bool quiet = getenv("RSBWT_QUIET") != nullptr;
        static bool said = false;
        if (!said && !quiet) {
            said = true;
            fprintf(stderr, "rsbwt: interval gather over peer copies (%s)\n", rccl().ok ? "device groups share a GPU" : "librccl not found");
        }
        for (size_t g = 1; g < G; ++g) {
            dev_group *grp = s->groups[g];
            (void)hipSetDevice(grp->device);
            if (!grp->peer_ready) HIP_OK(hipEventCreateWithFlags(&grp->peer_ready, hipEventDisableTiming));
            if (!grp->peer_done) HIP_OK(hipEventCreateWithFlags(&grp->peer_done, hipEventDisableTiming));
            HIP_OK(hipEventRecord(grp->peer_ready, (hipStream_t)streams[g]));
            (void)hipSetDevice(s->groups[0]->device);
            HIP_OK(hipStreamWaitEvent((hipStream_t)streams[0], grp->peer_ready, 0));
            HIP_OK(hipMemcpyPeerAsync((uint8_t *)d_root + off, s->groups[0]->device, d_blocks[g], grp->device, bytes[g], (hipStream_t)streams[0]));
            HIP_OK(hipEventRecord(grp->peer_done, (hipStream_t)streams[0]));
            (void)hipSetDevice(grp->device);
            HIP_OK(hipStreamWaitEvent((hipStream_t)streams[g], grp->peer_done, 0));
            off += bytes[g];
        }
        return RSBWT_OK;
    }
    ncclResult_t nr = rccl().GroupStart();
    for (size_t g = 1; g < G && nr == ncclSuccess; ++g) {
        (void)hipSetDevice(s->groups[g]->device);
        nr = rccl().Send(d_blocks[g], bytes[g], ncclUint8, 0, s->groups[g]->comm, (hipStream_t)streams[g]);
        if (nr != ncclSuccess) break;
        (void)hipSetDevice(s->groups[0]->device);
        nr = rccl().Recv((uint8_t *)d_root + off, bytes[g], ncclUint8, (int)g, s->groups[0]->comm, (hipStream_t)streams[0]);
        off += bytes[g];
    }
    const ncclResult_t ne = rccl().GroupEnd();
    if (nr == ncclSuccess) nr = ne;
    if (nr != ncclSuccess) return fail(RSBWT_EHIP, "RCCL gather: %s", rccl().GetErrorString(nr));
    return RSBWT_OK;
}
int rsbwt_set_gather_intervals_dev(rsbwt_set_t *s, const void *const *d_blocks, const size_t *bytes, void *d_root,
                                   void *const *streams) {
    return guarded("rsbwt_set_gather_intervals_dev", [&]() -> int { return rsbwt_set_gather_intervals_dev_body(s, d_blocks, bytes, d_root, streams); });
}


// ---- configs[3] / configs[4] over a set that may span devices -------------------------------------------
// The reference's front-end sends every request to every partition and CONCATENATES the per-partition
// read lists (src/service/server.cpp:124,199-261); a partition answers with what ITS BWT holds.  So the
// set-level forms of the 1-mismatch search and of locate + extract are per-shard results laid side by
// side: the devices work concurrently (one host thread each), a device's shards take turns on it, and
// what crosses PCIe is each device's own lists / reads, straight to the caller's host buffers.

// every shard's rsbwt_hits_1mm list, in shard order: hits[first[i] .. first[i+1]) are shard i's
static int rsbwt_set_hits_1mm_body(rsbwt_set_t *s, const char *kmers, size_t Q, uint32_t k, size_t stride,
                                   rsbwt_hit_1mm *hits, size_t cap, uint64_t *first, size_t *nhits) {
    if (!s || !nhits || !first) return fail(RSBWT_EINVAL, "null argument");
    const size_t S = s->shards.size();
    *nhits = 0;
    for (size_t i = 0; i <= S; ++i) first[i] = 0;
    if (Q == 0) return RSBWT_OK;
    if (!kmers || (!hits && cap)) return fail(RSBWT_EINVAL, "null argument");
    std::vector<std::vector<rsbwt_hit_1mm>> part(S);
    int rc = for_each_group(s, [&](size_t gi) -> int {
        dev_group *g = s->groups[gi];
        for (size_t i : g->idx) {
            std::vector<rsbwt_hit_1mm> &v = part[i];
            v.resize(std::max<size_t>(4 * Q, 1024));
            size_t n = 0;
            int r = rsbwt_hits_1mm(s->shards[i], kmers, Q, k, stride, v.data(), v.size(), &n);
            if (r == RSBWT_ERANGE && n > v.size()) {  // (k out of range also says ERANGE: n stays 0)
                v.resize(n);
                r = rsbwt_hits_1mm(s->shards[i], kmers, Q, k, stride, v.data(), v.size(), &n);
            }
            if (r) return r;
            v.resize(n);
        }
        return RSBWT_OK;
    });
    if (rc) return rc;
    size_t total = 0;
    for (size_t i = 0; i < S; ++i) {
        first[i] = total;
        total += part[i].size();
    }
    first[S] = total;
    *nhits = total;
    if (total > cap) return fail(RSBWT_ERANGE, "%zu hits over the set, room for %zu", total, cap);
    for (size_t i = 0; i < S; ++i)
        if (!part[i].empty()) memcpy(hits + first[i], part[i].data(), part[i].size() * sizeof(rsbwt_hit_1mm));
    return RSBWT_OK;
}
int rsbwt_set_hits_1mm(rsbwt_set_t *s, const char *kmers, size_t Q, uint32_t k, size_t stride, rsbwt_hit_1mm *hits,
                       size_t cap, uint64_t *first, size_t *nhits) {
    return guarded("rsbwt_set_hits_1mm", [&]() -> int { return rsbwt_set_hits_1mm_body(s, kmers, Q, k, stride, hits, cap, first, nhits); });
}

// The group's shard views WITH the shards' select samples, for the fused extraction (extract_lines.hip: ONE launch sequence
// walks the rows of every shard of the group): an array of its own (d_xviews), made on the first call from the shards'
// extraction views -- the array the searches read (d_views) is not touched, so an extraction may start beside searches
// on the same set.
static int ensure_group_xviews(rsbwt_set_t *s, dev_group *g, hipStream_t stream) {
    if (g->xviews_ready.load(std::memory_order_acquire)) return RSBWT_OK;
    std::lock_guard<std::mutex> lock(s->mu);
    if (g->xviews_ready.load(std::memory_order_relaxed)) return RSBWT_OK;
    std::vector<shard_view> v;
    for (size_t i : g->idx) {
        rsbwt_t *h = s->shards[i];
        if (h->view.n == 0) return fail(RSBWT_EINVAL, "empty index");
        const int rc = ensure_samples(h, stream);
        if (rc != RSBWT_OK) return rc;
        v.push_back(h->xview);
    }
    shard_view *dx = nullptr;
    HIP_OK(hipMalloc(&dx, v.size() * sizeof(shard_view)));
    const hipError_t e = hipMemcpy(dx, v.data(), v.size() * sizeof(shard_view), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(dx);
        return fail_hip(e, "publishing the extraction views");
    }
    g->d_xviews = dx;
    g->xviews_ready.store(true, std::memory_order_release);
    return RSBWT_OK;
}

// row i = SA row rows[i] of shard shard_of[i]
static int rsbwt_set_extract_body(rsbwt_set_t *s, const uint32_t *shard_of, const uint64_t *rows, size_t n, char *out,
                                  uint32_t stride, uint32_t *len, uint32_t *prefix_len) {
    if (!s) return fail(RSBWT_EINVAL, "null set");
    if (n == 0) return RSBWT_OK;
    if (!shard_of || !rows || !out) return fail(RSBWT_EINVAL, "null argument");
    const size_t S = s->shards.size();
    for (size_t i = 0; i < n; ++i)
        if (shard_of[i] >= S) return fail(RSBWT_EINVAL, "row %zu names shard %u of %zu", i, shard_of[i], S);
    static const bool turns_only = knob_set("RSBWT_SET_EXTRACT_TURNS");  // A/B knob (tools/README.md): a launch sequence per shard
    return for_each_group(s, [&](size_t gi) -> int {
        dev_group *g = s->groups[gi];
        const group_share sh = share_of_group(s, g, shard_of, rows, n);
        const size_t Sg = g->idx.size(), ng = sh.pos.size();
        if (ng == 0) return RSBWT_OK;
        std::vector<std::vector<size_t>> where(Sg);  // per shard of the group: its entries of the share, in the caller's order
        for (size_t t = 0; t < ng; ++t) where[sh.shard[t]].push_back(t);
        size_t nmax = 0;
        for (const std::vector<size_t> &w : where) nmax = std::max(nmax, w.size());
        // The rows of all the group's shards in ONE launch sequence (the fused extraction bench.py --mode extract times):
        // [S_g][nmax] rows, a shard with fewer padded with rows past any index (they end at once).  What a window of the
        // service loop asks for -- a few hundred rows spread over the partitions -- then costs one walk's latency, not
        // one per partition (round 5; until then a launch sequence and a copy back per shard).
        if (!turns_only && Sg > 1 && nmax < (1ull << 31) && Sg * nmax <= 4 * ng + 4096) {
            group_call gc(g);
            if (gc.rc) return gc.rc;
            call_ctx *c = gc.c;
            hipStream_t st = gc.st;
            int rc = ensure_group_xviews(s, g, st);
            if (rc != RSBWT_OK) return rc;
            const size_t cells = Sg * nmax;
            const size_t a_rows = al256(cells * 8), a_out = al256(cells * (size_t)stride), a_u32 = al256(cells * 4);
            if ((rc = c->stage(a_rows + a_out + 2 * a_u32)) != RSBWT_OK) return rc;
            uint8_t *d_rows = (uint8_t *)c->d_stage, *d_out = d_rows + a_rows, *d_len = d_out + a_out, *d_pl = d_len + a_u32;
            std::vector<uint64_t> hr(cells, ~0ull);
            for (size_t j = 0; j < Sg; ++j)
                for (size_t t = 0; t < where[j].size(); ++t) hr[j * nmax + t] = sh.rows[where[j][t]];
            HIP_OK(hipMemcpyAsync(d_rows, hr.data(), cells * 8, hipMemcpyHostToDevice, st));
            const hipError_t e = launch_extract_wave(g->scratch, g->d_xviews, (uint32_t)Sg, d_rows, nmax, d_out, stride, d_pl, d_len, g->num_cus, st, nullptr);
            if (e != hipSuccess) return fail_hip(e, "extract kernel launch");
            std::vector<char> ho(cells * (size_t)stride);
            std::vector<uint32_t> hl(cells), hp(cells);
            HIP_OK(hipMemcpyAsync(ho.data(), d_out, cells * (size_t)stride, hipMemcpyDeviceToHost, st));
            HIP_OK(hipMemcpyAsync(hl.data(), d_len, cells * 4, hipMemcpyDeviceToHost, st));
            HIP_OK(hipMemcpyAsync(hp.data(), d_pl, cells * 4, hipMemcpyDeviceToHost, st));
            HIP_OK(hipStreamSynchronize(st));
            for (size_t j = 0; j < Sg; ++j)
                for (size_t t = 0; t < where[j].size(); ++t)
                    scatter_read(ho.data(), hl.data(), hp.data(), j * nmax + t, out, stride, len, prefix_len, sh.pos[where[j][t]]);
            return RSBWT_OK;
        }
        for (size_t j = 0; j < Sg; ++j) {
            const std::vector<size_t> &w = where[j];
            if (w.empty()) continue;
            const size_t m = w.size();
            std::vector<uint64_t> r(m);
            std::vector<char> o(m * (size_t)stride);
            std::vector<uint32_t> ln(m), pl(m);
            for (size_t t = 0; t < m; ++t) r[t] = sh.rows[w[t]];
            const int rc = rsbwt_extract(s->shards[g->idx[j]], r.data(), m, o.data(), stride, ln.data(), pl.data());
            if (rc) return rc;
            for (size_t t = 0; t < m; ++t) scatter_read(o.data(), ln.data(), pl.data(), t, out, stride, len, prefix_len, sh.pos[w[t]]);
        }
        return RSBWT_OK;
    });
}
int rsbwt_set_extract(rsbwt_set_t *s, const uint32_t *shard_of, const uint64_t *rows, size_t n, char *out, uint32_t stride,
                      uint32_t *len, uint32_t *prefix_len) {
    return guarded("rsbwt_set_extract", [&]() -> int { return rsbwt_set_extract_body(s, shard_of, rows, n, out, stride, len, prefix_len); });
}

// THE host-side rule that turns a batch's intervals lo / up [S][Q] into rows, for every call whose set spans several
// device groups: shard i brings query q its interval if it is one of rows of that shard (rsbwt_query's rule: capi.hip,
// interval_rows) -- matches[q] (optional) counts them over the shards; a query with more than max_rows of them
// (0 = no limit) brings none; first[] is the running total of the rows kept.  With room for them (total <= cap) the rows
// themselves follow as (shard_of, rows) in the caller's order: query by query, shard ascending, SA row ascending.
struct expanded_rows {
    size_t total = 0;
    uint64_t over = 0;  // queries over the limit
    std::vector<uint32_t> shard_of;
    std::vector<uint64_t> rows;
};
static expanded_rows intervals_to_rows_host(const rsbwt_set_t *s, size_t Q, const std::vector<uint64_t> &lo, const std::vector<uint64_t> &up,
                                            uint64_t max_rows, size_t cap, uint64_t *first, uint64_t *matches) {
    const size_t S = s->shards.size();
    auto width = [&](size_t i, size_t q) -> uint64_t {
        const uint64_t l = lo[i * Q + q], u = up[i * Q + q];
        return (l <= u && u < s->shards[i]->view.n) ? u - l + 1 : 0;
    };
    expanded_rows hr;
    for (size_t q = 0; q < Q; ++q) {
        uint64_t m = 0;
        for (size_t i = 0; i < S; ++i) m += width(i, q);
        if (matches) matches[q] = m;
        first[q] = hr.total;
        if (max_rows && m > max_rows) ++hr.over;
        else hr.total += (size_t)m;
    }
    first[Q] = hr.total;
    if (hr.total > cap) return hr;
    hr.shard_of.reserve(hr.total);
    hr.rows.reserve(hr.total);
    for (size_t q = 0; q < Q; ++q) {
        if (first[q + 1] == first[q]) continue;
        for (size_t i = 0; i < S; ++i)
            for (uint64_t r = 0, w = width(i, q); r < w; ++r) {
                hr.shard_of.push_back((uint32_t)i);
                hr.rows.push_back(lo[i * Q + q] + r);
            }
    }
    return hr;
}

// what rsbwt_set_query makes of the batch's intervals lo / up [S][Q]: first[] (and matches[], *over: intervals_to_rows_host),
// and the rows' reads in the caller's order
static int set_query_rows(rsbwt_set_t *s, size_t Q, const std::vector<uint64_t> &lo, const std::vector<uint64_t> &up, uint64_t max_rows,
                          uint64_t *first, uint64_t *matches, uint64_t *over, uint32_t *read_shard, char *reads, uint32_t read_stride,
                          uint32_t *read_len, size_t cap_reads, size_t *nreads) {
    const expanded_rows hr = intervals_to_rows_host(s, Q, lo, up, max_rows, cap_reads, first, matches);
    *nreads = hr.total;
    if (over) *over = hr.over;
    if (hr.total > cap_reads) return fail(RSBWT_ERANGE, "%zu reads over the set, room for %zu", hr.total, cap_reads);
    if (hr.total == 0) return RSBWT_OK;
    if (!reads || !read_len) return fail(RSBWT_EINVAL, "null argument");
    if (read_shard) memcpy(read_shard, hr.shard_of.data(), hr.total * sizeof(uint32_t));
    return rsbwt_set_extract_body(s, hr.shard_of.data(), hr.rows.data(), hr.total, reads, read_stride, read_len, nullptr);
}

// query() of every shard (query.cpp:87-100), k-mer by k-mer: k-mer q's reads are first[q] .. first[q+1],
// shard 0's first (each shard's in SA-row order), read_shard[r] naming the shard read r came from
static int rsbwt_set_query_body(rsbwt_set_t *s, const char *kmers, size_t Q, uint32_t k, size_t stride, uint64_t *first,
                                uint32_t *read_shard, char *reads, uint32_t read_stride, uint32_t *read_len, size_t cap_reads,
                                size_t *nreads) {
    if (!s || !nreads || (!first && Q)) return fail(RSBWT_EINVAL, "null argument");
    *nreads = 0;
    if (Q == 0) return RSBWT_OK;
    if (!kmers) return fail(RSBWT_EINVAL, "null argument");
    if (read_stride == 0) return fail(RSBWT_EINVAL, "read_stride must be positive");
    const size_t S = s->shards.size();
    if (k == 0) {  // (rsbwt_query: no rows)
        for (size_t q = 0; q <= Q; ++q) first[q] = 0;
        return RSBWT_OK;
    }
    // ONE search of the batch over all the shards (a fused launch per device), then ONE extraction of the intervals' rows
    // addressed as (shard, row) in the order the caller gets them.  (Until round 5 every shard ran rsbwt_query by itself,
    // twice -- to size, then to fetch: 2 S searches and S extractions, each a launch sequence with a copy back of its
    // own; a window of the service loop made one such call per distinct query length.)
    std::vector<uint64_t> lo(S * Q), up(S * Q);
    const int rc = rsbwt_set_find_intervals_body(s, kmers, Q, k, stride, lo.data(), up.data());
    if (rc) return rc;
    return set_query_rows(s, Q, lo, up, 0, first, nullptr, nullptr, read_shard, reads, read_stride, read_len, cap_reads, nreads);
}
// the same for queries of lengths of their own (rsbwt_set_find_intervals_var): one call answers a window of the service loop
int rsbwt_set_query_var(rsbwt_set_t *s, const char *text, const uint64_t *off, size_t Q, uint64_t *first, uint32_t *read_shard,
                        char *reads, uint32_t read_stride, uint32_t *read_len, size_t cap_reads, size_t *nreads) {
    return guarded("rsbwt_set_query_var", [&]() -> int {
        if (!s || !nreads || (!first && Q)) return fail(RSBWT_EINVAL, "null argument");
        *nreads = 0;
        if (Q == 0) return RSBWT_OK;
        if (read_stride == 0) return fail(RSBWT_EINVAL, "read_stride must be positive");
        const size_t S = s->shards.size();
        std::vector<uint64_t> lo(S * Q), up(S * Q);
        const int rc = rsbwt_set_find_intervals_var_body(s, text, off, Q, lo.data(), up.data(), false);
        if (rc) return rc;
        return set_query_rows(s, Q, lo, up, 0, first, nullptr, nullptr, read_shard, reads, read_stride, read_len, cap_reads, nreads);
    });
}
int rsbwt_set_query(rsbwt_set_t *s, const char *kmers, size_t Q, uint32_t k, size_t stride, uint64_t *first,
                    uint32_t *read_shard, char *reads, uint32_t read_stride, uint32_t *read_len, size_t cap_reads,
                    size_t *nreads) {
    return guarded("rsbwt_set_query", [&]() -> int {
        return rsbwt_set_query_body(s, kmers, Q, k, stride, first, read_shard, reads, read_stride, read_len, cap_reads, nreads);
    });
}

// ---- rsbwt_set_query_var with a limit on the rows of one query; the intervals' rows made on the GPU (interval_rows.hip) ----
namespace {
// the calling thread's last capped query: rows expanded on the device, rows uploaded from the host, queries over the
// limit, bytes copied to the host before the extraction was launched
thread_local uint64_t capped_last_work[4] = {0, 0, 0, 0};

enum { CAPPED_TAKE_HOST = 1 };  // (not an error: the device path leaves the call to the host path)

// What the capped calls of a set on ONE device group start with, on gc's stream: the search leaves its pairs [S][Q] in HBM,
// the totals make matches[], first[] and the count of queries over the limit there; first[], matches[] (optional) and
// that count cross to the host (the caller's answers; first[Q] sizes what follows) and the stream is waited for once --
// never an interval or a row.  Everything sits in gc.la, with extra_bytes of the caller's own (d_extra) and scan scratch
// for scan_items items (d_tmp: interval_rows_scan_bytes).
struct capped_intervals {
    uint8_t *d_pairs, *d_matches, *d_first, *d_extra, *d_tmp;
    size_t tmp_bytes;
    uint64_t total, over;  // first[Q]; queries over the limit
};
int capped_intervals_device(rsbwt_set_t *s, group_call &gc, const char *text, const uint64_t *off, size_t Q, uint64_t max_rows,
                            size_t extra_bytes, size_t scan_items, const char *scratch_for, uint64_t *first, uint64_t *matches,
                            capped_intervals *ci) {
    dev_group *g = gc.g;
    hipStream_t st = gc.st;
    const uint32_t S = (uint32_t)g->idx.size();
    const size_t a_pairs = al256((size_t)S * Q * 16), a_q = al256((Q + 1) * 8);
    hipError_t e = g->scratch.take(a_pairs + 3 * a_q + extra_bytes + 256 + interval_rows_scan_bytes(scan_items) + 256, st, &gc.la);
    if (e != hipSuccess) return fail_hip(e, scratch_for);
    uint8_t *d_pairs = (uint8_t *)gc.la.p, *d_matches = d_pairs + a_pairs, *d_kept = d_matches + a_q, *d_first = d_kept + a_q,
            *d_extra = d_first + a_q, *d_over = d_extra + extra_bytes, *d_tmp = d_over + 256;
    // ---- the search (for_each_var_slice); every slice's pairs land in the batch's [S][Q] block: the only slice writes
    // them there, one of several leaves them behind its start records and they are copied over row by row
    auto a_rec = [&](size_t mq) { return al256((size_t)S * mq * 16); };
    int rc = for_each_var_slice(
        *gc.c, st, text, off, Q, [&](size_t mq) { return a_rec(mq) + (mq == Q ? 0 : al256((size_t)S * mq * 16)); },
        [&](size_t q0, size_t mq) -> int {  // nothing to search: pairs of all ones are no interval of any shard (upper >= n)
            HIP_OK(hipMemset2DAsync(d_pairs + q0 * 16, Q * 16, 0xFF, mq * 16, S, st));
            return RSBWT_OK;
        },
        [&](const var_slice &sl) -> int {
            const size_t q0 = sl.q0, mq = sl.mq;
            uint8_t *d_rec = sl.d_extra, *d_res = mq == Q ? d_pairs : d_rec + a_rec(mq);
            const hipError_t ei = launch_search_init_var(g->d_views, S, sl.d_pk, sl.d_ok, sl.d_len, mq, sl.wpq, d_rec, st);
            if (ei != hipSuccess) return fail_hip(ei, "start-record kernel launch");
            search_extra ex;
            ex.narrow = group_is_narrow(s, g, sl.k);
            ex.d_init = d_rec;
            ex.pairs = true;
            const int rs = search_launch(*g, g->d_views, S, g->num_cus, sl.d_pk, sl.d_ok, mq, sl.k, d_res, nullptr, false, st, &ex);
            if (rs) return rs;
            if (mq != Q) HIP_OK(hipMemcpy2DAsync(d_pairs + q0 * 16, Q * 16, d_res, mq * 16, mq * 16, S, hipMemcpyDeviceToDevice, st));
            return RSBWT_OK;
        });
    if (rc) return rc;
    // ---- totals, the limit, first[]
    const size_t tmp_bytes = interval_rows_scan_bytes(scan_items);
    e = launch_interval_totals(g->d_views, S, d_pairs, Q, max_rows, d_matches, d_kept, d_first, d_over, d_tmp, tmp_bytes, st);
    if (e != hipSuccess) return fail_hip(e, "interval-rows kernels");
    *ci = capped_intervals{d_pairs, d_matches, d_first, d_extra, d_tmp, tmp_bytes, 0, 0};
    HIP_OK(hipMemcpyAsync(first, d_first, (Q + 1) * 8, hipMemcpyDeviceToHost, st));
    if (matches) HIP_OK(hipMemcpyAsync(matches, d_matches, Q * 8, hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(&ci->over, d_over, 8, hipMemcpyDeviceToHost, st));  // (the caller's struct: it outlives gc's synchronise)
    HIP_OK(hipStreamSynchronize(st));
    ci->total = first[Q];
    return RSBWT_OK;
}

// The reads of a capped query on one device group: the cells of the kept rows, the rows by cell for the ragged walks
// (extract_lines.hip) and as (shard, cell row) in the caller's order, all made and taken where they are in HBM.
int query_capped_device(rsbwt_set_t *s, const char *text, const uint64_t *off, size_t Q, uint64_t max_rows, uint64_t *first,
                        uint32_t *read_shard, char *reads, uint32_t read_stride, uint32_t *read_len, size_t cap_reads, size_t *nreads,
                        uint64_t *matches) {
    capped_intervals ci;  // (before gc: a copy into it may still be in flight when gc waits for the stream)
    group_call gc(s->groups[0], true);
    if (gc.rc) return gc.rc;
    dev_group *g = gc.g;
    hipStream_t st = gc.st;
    const uint32_t S = (uint32_t)g->idx.size();
    const size_t cells = (size_t)S * Q, a_cells = al256((cells + 1) * 8);
    int rc = capped_intervals_device(s, gc, text, off, Q, max_rows, 2 * a_cells, cells + 1, "scratch for a capped query", first, matches, &ci);
    if (rc) return rc;
    const uint64_t total = ci.total;
    *nreads = (size_t)total;
    capped_last_work[2] = ci.over;
    capped_last_work[3] = (Q + 1) * 8 + (matches ? Q * 8 : 0) + 8;
    if (total > cap_reads) return fail(RSBWT_ERANGE, "%llu reads over the set, room for %zu", (unsigned long long)total, cap_reads);
    if (total == 0) return RSBWT_OK;
    if (!reads || !read_len) return fail(RSBWT_EINVAL, "null argument");
    if (total >= (1ull << 31)) return CAPPED_TAKE_HOST;  // (the walk kernels number a launch's rows in 32 bits)
    uint8_t *d_cellw = ci.d_extra, *d_cellpos = d_cellw + a_cells;
    hipError_t e = launch_interval_cells(g->d_views, S, ci.d_pairs, Q, max_rows, ci.d_matches, d_cellw, d_cellpos, ci.d_tmp, ci.tmp_bytes, st);
    if (e != hipSuccess) return fail_hip(e, "interval-rows kernels");
    if ((rc = ensure_group_xviews(s, g, st)) != RSBWT_OK) return rc;
    const size_t a_rows = al256(total * 8), a_u32 = al256(total * 4), a_out = al256(total * (size_t)read_stride);
    e = g->scratch.take(a_rows + 4 * a_u32 + a_out, st, &gc.lb);
    if (e != hipSuccess) return fail(RSBWT_ENOMEM, "%llu reads of %u bytes do not fit the device's free memory: %s", (unsigned long long)total,
                                     read_stride, hipGetErrorString(e));
    uint8_t *d_crow = (uint8_t *)gc.lb.p, *d_out = d_crow + a_rows, *d_dest = d_out + a_out, *d_shard = d_dest + a_u32, *d_plen = d_shard + a_u32,
            *d_rlen = d_plen + a_u32;
    e = launch_interval_fill(g->d_views, S, ci.d_pairs, Q, ci.d_first, (size_t)total, d_shard, nullptr, d_cellpos, d_crow, d_dest, st);
    if (e == hipSuccess)
        e = launch_extract_ragged(g->scratch, g->d_xviews, S, d_crow, (size_t)total, d_cellpos, Q, d_out, read_stride, d_plen, d_rlen, g->num_cus, st);
    if (e != hipSuccess) return fail_hip(e, "row expansion and extract kernel launches");
    capped_last_work[0] = total;
    std::vector<char> ho(total * (size_t)read_stride);
    std::vector<uint32_t> hl(total), hd(total), hs(total);
    HIP_OK(hipMemcpyAsync(ho.data(), d_out, total * (size_t)read_stride, hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(hl.data(), d_rlen, total * 4, hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(hd.data(), d_dest, total * 4, hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(hs.data(), d_shard, total * 4, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    for (size_t t = 0; t < total; ++t) {
        scatter_read(ho.data(), hl.data(), nullptr, hd[t], reads, read_stride, read_len, nullptr, t);
        if (read_shard) read_shard[t] = (uint32_t)g->idx[hs[t]];
    }
    return RSBWT_OK;
}

int query_capped_body(rsbwt_set_t *s, const char *text, const uint64_t *off, size_t Q, uint64_t max_rows, uint64_t *first,
                      uint32_t *read_shard, char *reads, uint32_t read_stride, uint32_t *read_len, size_t cap_reads, size_t *nreads,
                      uint64_t *matches) {
    if (!s || !nreads || (!first && Q)) return fail(RSBWT_EINVAL, "null argument");
    *nreads = 0;
    for (uint64_t &w : capped_last_work) w = 0;
    if (Q == 0) return RSBWT_OK;
    if (read_stride == 0) return fail(RSBWT_EINVAL, "read_stride must be positive");
    if (!off || (!text && off[Q] != off[0])) return fail(RSBWT_EINVAL, "null argument");
    for (rsbwt_t *h : s->shards)
        if (h->view.n == 0) return fail(RSBWT_EINVAL, "empty index in the set");
    const size_t S = s->shards.size();
    static const bool turns_only = knob_set("RSBWT_SET_EXTRACT_TURNS");        // A/B knobs (tools/README.md)
    static const bool host_rows = knob_set("RSBWT_SET_QUERY_HOST_ROWS");
    if (s->groups.size() == 1 && S <= 1024 && !turns_only && !host_rows) {
        const int rc = query_capped_device(s, text, off, Q, max_rows, first, read_shard, reads, read_stride, read_len, cap_reads, nreads, matches);
        if (rc != CAPPED_TAKE_HOST) return rc;
        for (uint64_t &w : capped_last_work) w = 0;
    }
    // several device groups (or a batch of 2^31 rows): the intervals come to the host, the limit is applied there
    // (intervals_to_rows_host), and the rows go the way rsbwt_set_query_var's go
    std::vector<uint64_t> lo(S * Q), up(S * Q);
    const int rc = rsbwt_set_find_intervals_var_body(s, text, off, Q, lo.data(), up.data(), false);
    if (rc) return rc;
    capped_last_work[3] = S * Q * 16;
    const int rq = set_query_rows(s, Q, lo, up, max_rows, first, matches, &capped_last_work[2], read_shard, reads, read_stride, read_len, cap_reads, nreads);
    if (rq == RSBWT_OK) capped_last_work[1] = *nreads;
    return rq;
}

// the service code's way in (service.h: service_slice.cpp is also linked into host harnesses without the engine)
struct register_query_hooks {
    register_query_hooks() { rsb::query_engine_hooks.query_var_capped = rsbwt_set_query_var_capped; }
} register_query_hooks_now;
}  // namespace

int rsbwt_set_query_var_capped(rsbwt_set_t *s, const char *text, const uint64_t *off, size_t Q, uint64_t max_rows, uint64_t *first,
                               uint32_t *read_shard, char *reads, uint32_t read_stride, uint32_t *read_len, size_t cap_reads,
                               size_t *nreads, uint64_t *matches) {
    return guarded("rsbwt_set_query_var_capped", [&]() -> int {
        return query_capped_body(s, text, off, Q, max_rows, first, read_shard, reads, read_stride, read_len, cap_reads, nreads, matches);
    });
}

void rsbwt_set_query_last_work(uint64_t *work4) {
    if (work4) memcpy(work4, capped_last_work, sizeof capped_last_work);
}

// the expansion alone, on the caller's buffers and stream: one-device set, nothing synchronised
int rsbwt_set_interval_rows_dev(rsbwt_set_t *s, const void *d_pairs, size_t Q, uint64_t max_rows, void *d_first, void *d_matches,
                                void *d_shard, void *d_rows, size_t cap, void *stream) {
    return guarded("rsbwt_set_interval_rows_dev", [&]() -> int {
        dev_group *g = nullptr;
        int rc = one_device_group(s, &g);
        if (rc) return rc;
        if (!d_first || (Q && (!d_pairs || !d_matches)) || (cap && (!d_shard || !d_rows))) return fail(RSBWT_EINVAL, "null argument");
        if (cap >= (1ull << 38)) return fail(RSBWT_ERANGE, "room for %zu rows: at most 2^38 per call", cap);
        hipStream_t st = (hipStream_t)stream;
        if (Q == 0) {
            HIP_OK(hipMemsetAsync(d_first, 0, 8, st));
            return RSBWT_OK;
        }
        const size_t a_q = ((Q + 1) * 8 + 255) & ~(size_t)255, tmp_bytes = interval_rows_scan_bytes(Q + 1);
        scratch_cache::lease mem;
        hipError_t e = g->scratch.take(a_q + 256 + tmp_bytes + 256, st, &mem);
        if (e != hipSuccess) return fail_hip(e, "scratch for the interval rows");
        uint8_t *d_kept = (uint8_t *)mem.p, *d_over = d_kept + a_q, *d_tmp = d_over + 256;
        const uint32_t S = (uint32_t)g->idx.size();
        e = launch_interval_totals(g->d_views, S, d_pairs, Q, max_rows, d_matches, d_kept, d_first, d_over, d_tmp, tmp_bytes, st);
        if (e == hipSuccess) e = launch_interval_fill(g->d_views, S, d_pairs, Q, d_first, cap, d_shard, d_rows, nullptr, nullptr, nullptr, st);
        g->scratch.give(mem, st);
        return e == hipSuccess ? RSBWT_OK : fail_hip(e, "interval-rows kernels");
    });
}

// ---- locate (locate.hip): rows of several shards, and the matches of queries as positions instead of strings ----
// entry i = SA row rows[i] of shard shard_of[i]; one launch per device group walks all of that group's shards
static int set_locate_body(rsbwt_set_t *s, const uint32_t *shard_of, const uint64_t *rows, size_t n, uint32_t max_steps, uint64_t *read_row,
                           uint64_t *ordinal, uint32_t *offset, uint64_t *work2) {
    const size_t S = s->shards.size();
    for (size_t i = 0; i < n; ++i)
        if (shard_of[i] >= S) return fail(RSBWT_EINVAL, "row %zu names shard %u of %zu", i, shard_of[i], S);
    std::atomic<uint64_t> walked{0}, steps{0};
    const int rc = for_each_group(s, [&](size_t gi) -> int {
        dev_group *g = s->groups[gi];
        const bool whole = s->groups.size() == 1;  // (the group's shard numbers are the set's: the caller's arrays as they are)
        group_share sh;
        if (!whole) {
            sh = share_of_group(s, g, shard_of, rows, n);
            if (sh.pos.empty()) return RSBWT_OK;
        }
        group_call gc(g);
        if (gc.rc) return gc.rc;
        int rg;
        uint64_t wk[2] = {0, 0};
        if (whole) {
            rg = locate_host_views(g->scratch, *gc.c, g->d_views, (uint32_t)g->idx.size(), g->num_cus, shard_of, rows, n, max_steps, read_row, ordinal,
                                   offset, wk);
        } else {
            const size_t m = sh.pos.size();
            std::vector<uint64_t> rr(read_row ? m : 0), od(ordinal ? m : 0);
            std::vector<uint32_t> of(offset ? m : 0);
            rg = locate_host_views(g->scratch, *gc.c, g->d_views, (uint32_t)g->idx.size(), g->num_cus, sh.shard.data(), sh.rows.data(), m, max_steps,
                                   read_row ? rr.data() : nullptr, ordinal ? od.data() : nullptr, offset ? of.data() : nullptr, wk);
            if (rg == RSBWT_OK)
                for (size_t t = 0; t < m; ++t) {
                    if (read_row) read_row[sh.pos[t]] = rr[t];
                    if (ordinal) ordinal[sh.pos[t]] = od[t];
                    if (offset) offset[sh.pos[t]] = of[t];
                }
        }
        walked += wk[0];
        steps += wk[1];
        return rg;
    });
    if (work2) {
        work2[0] += walked.load();
        work2[1] += steps.load();
    }
    return rc;
}

int rsbwt_set_locate(rsbwt_set_t *s, const uint32_t *shard_of, const uint64_t *rows, size_t n, uint32_t max_steps, uint64_t *read_row,
                     uint64_t *ordinal, uint32_t *offset) {
    return guarded("rsbwt_set_locate", [&]() -> int {
        locate_set_last_work(0, 0);
        if (!s) return fail(RSBWT_EINVAL, "null set");
        if (!read_row && !ordinal && !offset) return fail(RSBWT_EINVAL, "null argument: no output array");
        if (n == 0) return RSBWT_OK;
        if (!shard_of || !rows) return fail(RSBWT_EINVAL, "null argument");
        uint64_t wk[2] = {0, 0};
        const int rc = set_locate_body(s, shard_of, rows, n, max_steps, read_row, ordinal, offset, wk);
        locate_set_last_work(wk[0], wk[1]);
        return rc;
    });
}

// one-device set, the caller's buffers and stream, nothing synchronised
int rsbwt_set_locate_dev(rsbwt_set_t *s, const void *d_shard, const void *d_rows, size_t n, uint32_t max_steps, void *d_read_row,
                         void *d_ordinal, void *d_offset, void *stream) {
    return guarded("rsbwt_set_locate_dev", [&]() -> int {
        dev_group *g = nullptr;
        int rc = one_device_group(s, &g);
        if (rc) return rc;
        if (!d_read_row && !d_ordinal && !d_offset) return fail(RSBWT_EINVAL, "null argument: no output array");
        if (n == 0) return RSBWT_OK;
        if (!d_shard || !d_rows) return fail(RSBWT_EINVAL, "null argument");
        const hipError_t e = launch_locate(g->scratch, g->d_views, (uint32_t)g->idx.size(), d_shard, d_rows, n, max_steps, d_read_row, d_ordinal,
                                           d_offset, nullptr, g->num_cus, (hipStream_t)stream);
        return e == hipSuccess ? RSBWT_OK : fail_hip(e, "locate kernel launch");
    });
}

namespace {
// One device group holding every shard: search, totals / limit / first[], the rows as (shard, row) and their walks all
// stay in HBM; first[] and matches[] cross to the host before the rows are made (first[Q] sizes them), the answers after.
int locate_capped_device(rsbwt_set_t *s, const char *text, const uint64_t *off, size_t Q, uint64_t max_rows, uint32_t max_steps,
                         uint64_t *first, uint32_t *read_shard, uint64_t *rows, uint64_t *read_row, uint64_t *ordinal, uint32_t *offset,
                         size_t cap, size_t *nrows, uint64_t *matches, uint64_t *work2) {
    capped_intervals ci;  // (before gc: a copy into it may still be in flight when gc waits for the stream)
    group_call gc(s->groups[0], true);
    if (gc.rc) return gc.rc;
    dev_group *g = gc.g;
    hipStream_t st = gc.st;
    const uint32_t S = (uint32_t)g->idx.size();
    const int rc = capped_intervals_device(s, gc, text, off, Q, max_rows, 0, Q + 1, "scratch for a capped locate", first, matches, &ci);
    if (rc) return rc;
    const uint64_t total = ci.total;
    *nrows = (size_t)total;
    if (total > cap) return fail(RSBWT_ERANGE, "%llu rows over the set, room for %zu", (unsigned long long)total, cap);
    if (total == 0) return RSBWT_OK;
    const size_t a8 = al256(total * 8), a4 = al256(total * 4);
    hipError_t e = g->scratch.take(3 * a8 + 2 * a4 + 256, st, &gc.lb);
    if (e != hipSuccess) return fail(RSBWT_ENOMEM, "%llu rows do not fit the device's free memory: %s", (unsigned long long)total, hipGetErrorString(e));
    uint8_t *d_rows = (uint8_t *)gc.lb.p, *d_rr = d_rows + a8, *d_od = d_rr + a8, *d_of = d_od + a8, *d_sh = d_of + a4, *d_wk = d_sh + a4;
    e = launch_interval_fill(g->d_views, S, ci.d_pairs, Q, ci.d_first, (size_t)total, d_sh, d_rows, nullptr, nullptr, nullptr, st);
    if (e != hipSuccess) return fail_hip(e, "row expansion");
    const bool walk = read_row || ordinal || offset;
    unsigned long long wk[2] = {0, 0};
    if (walk) {
        HIP_OK(hipMemsetAsync(d_wk, 0, 16, st));
        e = launch_locate(g->scratch, g->d_views, S, d_sh, d_rows, (size_t)total, max_steps, read_row ? d_rr : nullptr, ordinal ? d_od : nullptr,
                          offset ? d_of : nullptr, (unsigned long long *)d_wk, g->num_cus, st);
        if (e != hipSuccess) return fail_hip(e, "locate kernel launch");
        HIP_OK(hipMemcpyAsync(wk, d_wk, 16, hipMemcpyDeviceToHost, st));
    }
    if (read_shard) HIP_OK(hipMemcpyAsync(read_shard, d_sh, total * 4, hipMemcpyDeviceToHost, st));
    if (rows) HIP_OK(hipMemcpyAsync(rows, d_rows, total * 8, hipMemcpyDeviceToHost, st));
    if (read_row) HIP_OK(hipMemcpyAsync(read_row, d_rr, total * 8, hipMemcpyDeviceToHost, st));
    if (ordinal) HIP_OK(hipMemcpyAsync(ordinal, d_od, total * 8, hipMemcpyDeviceToHost, st));
    if (offset) HIP_OK(hipMemcpyAsync(offset, d_of, total * 4, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    if (read_shard)
        for (size_t t = 0; t < total; ++t) read_shard[t] = (uint32_t)g->idx[read_shard[t]];
    work2[0] += wk[0];
    work2[1] += wk[1];
    return RSBWT_OK;
}
}  // namespace

int rsbwt_set_locate_var_capped(rsbwt_set_t *s, const char *text, const uint64_t *off, size_t Q, uint64_t max_rows, uint32_t max_steps,
                                uint64_t *first, uint32_t *read_shard, uint64_t *rows, uint64_t *read_row, uint64_t *ordinal,
                                uint32_t *offset, size_t cap, size_t *nrows, uint64_t *matches) {
    return guarded("rsbwt_set_locate_var_capped", [&]() -> int {
        locate_set_last_work(0, 0);
        if (!s || !nrows || (!first && Q)) return fail(RSBWT_EINVAL, "null argument");
        *nrows = 0;
        if (Q == 0) return RSBWT_OK;
        if (!off || (!text && off[Q] != off[0])) return fail(RSBWT_EINVAL, "null argument");
        for (rsbwt_t *h : s->shards)
            if (h->view.n == 0) return fail(RSBWT_EINVAL, "empty index in the set");
        const size_t S = s->shards.size();
        uint64_t wk[2] = {0, 0};
        if (s->groups.size() == 1 && S <= 1024) {
            const int rc = locate_capped_device(s, text, off, Q, max_rows, max_steps, first, read_shard, rows, read_row, ordinal, offset, cap,
                                                nrows, matches, wk);
            locate_set_last_work(wk[0], wk[1]);
            return rc;
        }
        // several device groups: the intervals come to the host, the limit and the expansion run there
        // (intervals_to_rows_host), and the rows go the way rsbwt_set_locate's go
        std::vector<uint64_t> lo(S * Q), up(S * Q);
        int rc = rsbwt_set_find_intervals_var_body(s, text, off, Q, lo.data(), up.data(), false);
        if (rc) return rc;
        const expanded_rows hr = intervals_to_rows_host(s, Q, lo, up, max_rows, cap, first, matches);
        const size_t total = hr.total;
        *nrows = total;
        if (total > cap) return fail(RSBWT_ERANGE, "%zu rows over the set, room for %zu", total, cap);
        if (total == 0) return RSBWT_OK;
        if (read_shard) memcpy(read_shard, hr.shard_of.data(), total * sizeof(uint32_t));
        if (rows) memcpy(rows, hr.rows.data(), total * sizeof(uint64_t));
        if (!read_row && !ordinal && !offset) return RSBWT_OK;
        rc = set_locate_body(s, hr.shard_of.data(), hr.rows.data(), total, max_steps, read_row, ordinal, offset, wk);
        locate_set_last_work(wk[0], wk[1]);
        return rc;
    });
}

// ---- SiteMatch candidates (gt_narrow.hip): find_gt_reads (src/service/service.cpp:507-711) over every shard ----
namespace {
// the calling thread's last gt call: legs, legs with no answer, LF steps spent lengthening, candidate rows, rows kept by
// the device's filter, reads extracted
thread_local uint64_t gt_last_work[6] = {0, 0, 0, 0, 0, 0};

// the host side of a batch (kernels.h, gt_batch): the queries that can have tiles, their all-ACGT tiles as slots
struct gt_plan {
    std::vector<uint64_t> q_off, q_pos;
    std::vector<uint32_t> q_len, nprev, slot_query, slot_tile;
    size_t nitems = 0;
    uint32_t k = 0, step = 0;
    uint64_t M = 0;
    size_t text_len = 0;
};
struct gt_row {  // a row the device's filter kept
    uint32_t item, shard, offset;  // shard: the set's number
    uint32_t pending;              // a LEFT row: its read's length decides
    uint64_t read_row;
};
struct gt_group_out {
    std::vector<gt_leg> legs;  // [S_g][nitems]
    std::vector<gt_row> rows;
    uint64_t steps = 0, candidates = 0, kept = 0;
};

int gt_make_plan(const char *text, const uint64_t *off, size_t Q, const uint64_t *pos, int32_t k, int32_t skip, uint64_t M, gt_plan *pl) {
    pl->M = M ? M : 10000;  // service.cpp:85, max_interval_size
    pl->text_len = Q ? (size_t)(off[Q] - off[0]) : 0;
    pl->q_off.resize(Q);
    pl->q_pos.assign(pos, pos + Q);
    pl->q_len.resize(Q);
    pl->nprev.assign(pl->text_len, 0);
    const char *t0 = Q ? text + off[0] : nullptr;
    for (size_t q = 0; q < Q; ++q) {
        const uint64_t L = off[q + 1] - off[q];
        if (L > 0x7FFFFFFFull) return fail(RSBWT_EINVAL, "query %zu: %llu symbols, at most 2^31 - 1", q, (unsigned long long)L);
        if (q >= 0xFFFFFFFFull) return fail(RSBWT_EINVAL, "at most 2^32 - 1 queries per call");
        const uint64_t base = off[q] - off[0];
        pl->q_off[q] = base;
        pl->q_len[q] = (uint32_t)L;
        uint32_t last = 0;
        for (uint64_t i = 0; i < L; ++i) {
            const char ch = t0[base + i];
            if (ch != 'A' && ch != 'C' && ch != 'G' && ch != 'T') last = (uint32_t)i + 1u;
            pl->nprev[base + i] = last;
        }
        if (k <= 0 || skip < 0 || L < (uint64_t)k || pos[q] > L) continue;
        const uint64_t step = (uint64_t)skip + 1;
        for (uint64_t i = 0; i <= (L - (uint64_t)k) / step; ++i) {
            const uint64_t s0 = step * i, e0 = s0 + (uint64_t)k;
            if (pl->nprev[base + e0 - 1] > s0) continue;  // don't bother with N (:513)
            pl->slot_query.push_back((uint32_t)q);
            pl->slot_tile.push_back((uint32_t)i);
        }
    }
    pl->k = k > 0 ? (uint32_t)k : 0;
    pl->step = skip >= 0 ? (uint32_t)skip + 1u : 1u;
    pl->nitems = 2 * pl->slot_query.size();
    if (pl->nitems >= (1ull << 31)) return fail(RSBWT_ERANGE, "%zu tile legs in one call: at most 2^31", pl->nitems);
    return RSBWT_OK;
}

// The front of a group's share, in gc.la: the batch uploaded, the narrowing launch enqueued.  d_wk: [0] lengthening steps,
// [1] rows kept, [2] rows whose walk did not end, zeroed.  d_extra: extra_bytes more for the caller, behind everything else.
struct gt_front {
    gt_batch bt;
    uint8_t *d_legs = nullptr, *d_pairs = nullptr, *d_matches = nullptr, *d_keptq = nullptr, *d_first = nullptr, *d_over = nullptr, *d_wk = nullptr,
            *d_tmp = nullptr, *d_extra = nullptr;
    size_t tmp_bytes = 0;
};
int gt_front_enqueue(dev_group *g, group_call &gc, const gt_plan &pl, const char *t0, size_t extra_bytes, gt_front *f) {
    hipStream_t st = gc.st;
    const uint32_t S = (uint32_t)g->idx.size();
    const size_t Q = pl.q_off.size(), slots = pl.slot_query.size(), N = pl.nitems, cells = (size_t)S * N;
    const size_t a_text = al256(pl.text_len + 1), a_np = al256(pl.text_len * 4 + 4), a_q8 = al256(Q * 8), a_q4 = al256(Q * 4), a_s4 = al256(slots * 4),
                 a_legs = al256(cells * sizeof(gt_leg)), a_pairs = al256(cells * 16), a_i = al256((N + 1) * 8),
                 tmp_bytes = interval_rows_scan_bytes(N + 1);
    hipError_t e = g->scratch.take(a_text + a_np + 2 * a_q8 + a_q4 + 2 * a_s4 + a_legs + a_pairs + 3 * a_i + 512 + al256(tmp_bytes) + 256 + extra_bytes, st,
                                   &gc.la);
    if (e != hipSuccess) return fail_hip(e, "scratch for the SiteMatch legs");
    uint8_t *d_text = (uint8_t *)gc.la.p, *d_np = d_text + a_text, *d_qoff = d_np + a_np, *d_qpos = d_qoff + a_q8, *d_qlen = d_qpos + a_q8,
            *d_sq = d_qlen + a_q4, *d_stile = d_sq + a_s4, *d_legs = d_stile + a_s4, *d_pairs = d_legs + a_legs, *d_matches = d_pairs + a_pairs,
            *d_keptq = d_matches + a_i, *d_first = d_keptq + a_i, *d_over = d_first + a_i, *d_wk = d_over + 256, *d_tmp = d_wk + 256;
    f->d_legs = d_legs;
    f->d_pairs = d_pairs;
    f->d_matches = d_matches;
    f->d_keptq = d_keptq;
    f->d_first = d_first;
    f->d_over = d_over;
    f->d_wk = d_wk;
    f->d_tmp = d_tmp;
    f->tmp_bytes = tmp_bytes;
    f->d_extra = d_tmp + al256(tmp_bytes) + 256;
    if (pl.text_len) {
        HIP_OK(hipMemcpyAsync(d_text, t0, pl.text_len, hipMemcpyHostToDevice, st));
        HIP_OK(hipMemcpyAsync(d_np, pl.nprev.data(), pl.text_len * 4, hipMemcpyHostToDevice, st));
    }
    HIP_OK(hipMemcpyAsync(d_qoff, pl.q_off.data(), Q * 8, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(d_qpos, pl.q_pos.data(), Q * 8, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(d_qlen, pl.q_len.data(), Q * 4, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(d_sq, pl.slot_query.data(), slots * 4, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(d_stile, pl.slot_tile.data(), slots * 4, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemsetAsync(d_wk, 0, 256, st));
    gt_batch &bt = f->bt;
    bt.text = (const char *)d_text;
    bt.nprev = (const uint32_t *)d_np;
    bt.q_off = (const uint64_t *)d_qoff;
    bt.q_len = (const uint32_t *)d_qlen;
    bt.q_pos = (const uint64_t *)d_qpos;
    bt.slot_query = (const uint32_t *)d_sq;
    bt.slot_tile = (const uint32_t *)d_stile;
    bt.nitems = N;
    bt.k = pl.k;
    bt.step = pl.step;
    bt.M = pl.M;
    e = launch_gt_narrow(g->d_views, S, bt, d_legs, d_pairs, (unsigned long long *)d_wk, st);
    if (e != hipSuccess) return fail_hip(e, "SiteMatch narrowing kernel launch");
    return RSBWT_OK;
}

// One device group's share: the batch goes up once, every (item, shard of the group) is narrowed by one launch, and --
// for the read calls -- the legs' rows are made, walked and filtered where they are; what comes back is the legs and
// the rows the filter kept.
int gt_group_run(rsbwt_set_t *s, dev_group *g, const gt_plan &pl, const char *t0, bool want_rows, gt_group_out *out) {
    group_call gc(g, true);
    if (gc.rc) return gc.rc;
    hipStream_t st = gc.st;
    const uint32_t S = (uint32_t)g->idx.size();
    const size_t N = pl.nitems, cells = (size_t)S * N;
    gt_front f;
    const int rc = gt_front_enqueue(g, gc, pl, t0, 0, &f);
    if (rc) return rc;
    const gt_batch &bt = f.bt;
    uint8_t *d_legs = f.d_legs, *d_pairs = f.d_pairs, *d_matches = f.d_matches, *d_keptq = f.d_keptq, *d_first = f.d_first, *d_over = f.d_over,
            *d_wk = f.d_wk, *d_tmp = f.d_tmp;
    const size_t tmp_bytes = f.tmp_bytes;
    unsigned long long *wk = (unsigned long long *)d_wk;
    hipError_t e = hipSuccess;
    out->legs.resize(cells);
    HIP_OK(hipMemcpyAsync(out->legs.data(), d_legs, cells * sizeof(gt_leg), hipMemcpyDeviceToHost, st));
    uint64_t total = 0;
    if (want_rows) {
        e = launch_interval_totals(g->d_views, S, d_pairs, N, 0, d_matches, d_keptq, d_first, d_over, d_tmp, tmp_bytes, st);
        if (e != hipSuccess) return fail_hip(e, "interval-rows kernels");
        HIP_OK(hipMemcpyAsync(&total, d_first + N * 8, 8, hipMemcpyDeviceToHost, st));
    }
    HIP_OK(hipStreamSynchronize(st));
    unsigned long long hwk[3] = {0, 0, 0};
    if (total >= (1ull << 31)) return fail(RSBWT_ERANGE, "%llu candidate rows in one call: at most 2^31", (unsigned long long)total);
    if (total != 0) {
        const size_t a8 = al256(total * 8), a4 = al256(total * 4), a_rec = al256(total * sizeof(gt_kept_row));
        e = g->scratch.take(2 * a8 + 2 * a4 + a_rec, st, &gc.lb);
        if (e != hipSuccess) return fail(RSBWT_ENOMEM, "%llu candidate rows do not fit the device's free memory: %s", (unsigned long long)total, hipGetErrorString(e));
        uint8_t *d_rows = (uint8_t *)gc.lb.p, *d_rr = d_rows + a8, *d_sh = d_rr + a8, *d_of = d_sh + a4, *d_rec = d_of + a4;
        e = launch_interval_fill(g->d_views, S, d_pairs, N, d_first, (size_t)total, d_sh, d_rows, nullptr, nullptr, nullptr, st);
        if (e == hipSuccess) e = launch_locate(g->scratch, g->d_views, S, d_sh, d_rows, (size_t)total, 0, d_rr, nullptr, d_of, nullptr, g->num_cus, st);
        if (e == hipSuccess) e = launch_gt_filter(bt, d_legs, d_first, d_sh, d_of, d_rr, total, d_rec, wk + 1, st);
        if (e != hipSuccess) return fail_hip(e, "row expansion, locate and filter kernel launches");
        // the counters first (they size the copy), then the kept rows' records and nothing else
        HIP_OK(hipMemcpyAsync(hwk, d_wk, sizeof hwk, hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        if (hwk[2] != 0)
            return fail(RSBWT_EINVAL, "%llu candidate rows whose walk to their read's start does not end (a corrupt index, or a read longer than 2^20 symbols)",
                        hwk[2]);
        if (hwk[1] > total) return fail(RSBWT_EHIP, "the row filter kept %llu of %llu rows", hwk[1], (unsigned long long)total);
        std::vector<gt_kept_row> kr((size_t)hwk[1]);
        if (!kr.empty()) {
            HIP_OK(hipMemcpyAsync(kr.data(), d_rec, kr.size() * sizeof(gt_kept_row), hipMemcpyDeviceToHost, st));
            HIP_OK(hipStreamSynchronize(st));
        }
        out->rows.reserve(kr.size());
        for (const gt_kept_row &r : kr) out->rows.push_back(gt_row{r.item, (uint32_t)g->idx[r.shard], r.offset, r.pending, r.read_row});
    } else {
        HIP_OK(hipMemcpyAsync(hwk, d_wk, 16, hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
    }
    out->steps = hwk[0];
    out->candidates = total;
    out->kept = hwk[1];
    return RSBWT_OK;
}

// reads[q * S + p]: the (read_row, string) pairs of query q in shard p, ascending read_row, a string once (null: legs only)
typedef std::vector<std::vector<std::pair<uint64_t, std::string>>> gt_reads_t;

int gt_call(rsbwt_set_t *s, const char *text, const uint64_t *off, size_t Q, const uint64_t *pos, int32_t k, int32_t skip, uint64_t M,
            std::vector<rsbwt_gt_leg> *legs, std::vector<uint64_t> *legs_first, gt_reads_t *reads, uint32_t stride) {
    for (uint64_t &w : gt_last_work) w = 0;
    if (!s || (Q && (!off || !pos))) return fail(RSBWT_EINVAL, "null argument");
    if (Q && !text && off[Q] != off[0]) return fail(RSBWT_EINVAL, "null argument");
    for (size_t q = 0; q < Q; ++q)
        if (off[q] > off[q + 1]) return fail(RSBWT_EINVAL, "query %zu: offsets not ascending", q);
    const size_t S = s->shards.size();
    for (rsbwt_t *h : s->shards) {
        if (h->view.n == 0) return fail(RSBWT_EINVAL, "empty index in the set");
        if (reads && !rsbwt_opened_for_reads(h)) return fail(RSBWT_EINVAL, "SiteMatch reads need shards opened with RSBWT_OPEN_READS");
    }
    if (S > 65535) return fail(RSBWT_EINVAL, "%zu shards: at most 65535", S);
    if (legs_first) legs_first->assign(Q + 1, 0);
    if (reads) reads->assign(Q * S, {});
    gt_plan pl;
    int rc = gt_make_plan(text, off, Q, pos, k, skip, M, &pl);
    if (rc) return rc;
    if (pl.nitems == 0) return RSBWT_OK;
    const size_t N = pl.nitems;
    std::vector<gt_group_out> outs(s->groups.size());
    rc = for_each_group(s, [&](size_t gi) -> int { return gt_group_run(s, s->groups[gi], pl, text + off[0], reads != nullptr, &outs[gi]); });
    if (rc) return rc;
    // ---- the legs in (query, tile, leg, shard) order; where shard p's record of an item lies
    std::vector<std::pair<size_t, size_t>> where(S);  // shard of the set -> (group, shard of the group)
    for (size_t gi = 0; gi < s->groups.size(); ++gi)
        for (size_t j = 0; j < s->groups[gi]->idx.size(); ++j) where[s->groups[gi]->idx[j]] = {gi, j};
    auto rec_of = [&](size_t p, size_t item) -> const gt_leg & { return outs[where[p].first].legs[where[p].second * N + item]; };
    uint64_t nlegs = 0, nnone = 0;
    // (a tile is one leg in one shard and two in another: the order is by the leg's label, not by the item that made it)
    std::vector<rsbwt_gt_leg> of_tile;
    for (size_t slot = 0; slot < N / 2; ++slot) {
        const uint32_t q = pl.slot_query[slot];
        of_tile.clear();
        for (size_t item = 2 * slot; item < 2 * slot + 2; ++item)
            for (size_t p = 0; p < S; ++p) {
                const gt_leg &r = rec_of(p, item);
                if (r.a == 0xFFFFFFFFu) nnone += r.reserved;
                else of_tile.push_back(rsbwt_gt_leg{q, pl.slot_tile[slot], r.label, (uint32_t)p, r.a, r.b, 0u, r.lower, r.upper});
            }
        std::sort(of_tile.begin(), of_tile.end(),
                  [](const rsbwt_gt_leg &x, const rsbwt_gt_leg &y) { return x.leg != y.leg ? x.leg < y.leg : x.shard < y.shard; });
        nlegs += of_tile.size();
        if (legs_first) (*legs_first)[q + 1] += of_tile.size();
        if (legs) legs->insert(legs->end(), of_tile.begin(), of_tile.end());
    }
    if (legs_first)
        for (size_t q = 0; q < Q; ++q) (*legs_first)[q + 1] += (*legs_first)[q];
    gt_last_work[0] = nlegs;
    gt_last_work[1] = nnone;
    for (const gt_group_out &o : outs) {
        gt_last_work[2] += o.steps;
        gt_last_work[3] += o.candidates;
        gt_last_work[4] += o.kept;
    }
    if (!reads) return RSBWT_OK;
    // ---- every distinct read of a kept row extracted once (kmer_reads.hip's rule for a read longer than the stride: it is
    // fetched again at 64 KB and still counts as one read extracted)
    std::vector<std::pair<uint32_t, uint64_t>> ids;
    for (const gt_group_out &o : outs)
        for (const gt_row &r : o.rows) ids.push_back({r.shard, r.read_row});
    std::sort(ids.begin(), ids.end());
    ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
    const size_t R = ids.size();
    if (R == 0) return RSBWT_OK;
    std::vector<uint32_t> shard_of(R), rlen(R);
    std::vector<uint64_t> rows(R);
    for (size_t i = 0; i < R; ++i) {
        shard_of[i] = ids[i].first;
        rows[i] = ids[i].second;
    }
    std::vector<std::string> str(R);
    {
        std::vector<char> buf(R * (size_t)stride);
        rc = rsbwt_set_extract_body(s, shard_of.data(), rows.data(), R, buf.data(), stride, rlen.data(), nullptr);
        if (rc) return rc;
        gt_last_work[5] += R;
        std::vector<size_t> over;
        for (size_t i = 0; i < R; ++i) {
            if (rlen[i] == 0xFFFFFFFFu) over.push_back(i);
            else str[i].assign(buf.data() + i * (size_t)stride, rlen[i]);
        }
        if (!over.empty()) {
            const uint32_t wide = 65536;
            std::vector<uint32_t> osh(over.size()), olen(over.size());
            std::vector<uint64_t> orow(over.size());
            for (size_t i = 0; i < over.size(); ++i) {
                osh[i] = shard_of[over[i]];
                orow[i] = rows[over[i]];
            }
            std::vector<char> obuf(over.size() * (size_t)wide);
            rc = rsbwt_set_extract_body(s, osh.data(), orow.data(), over.size(), obuf.data(), wide, olen.data(), nullptr);
            if (rc) return rc;
            for (size_t i = 0; i < over.size(); ++i) {
                if (olen[i] == 0xFFFFFFFFu)
                    return fail(RSBWT_EINVAL, "shard %u row %llu: a read longer than %u symbols (or a walk that does not end)", osh[i],
                                (unsigned long long)orow[i], wide);
                str[over[i]].assign(obuf.data() + i * (size_t)wide, olen[i]);
            }
        }
    }
    // ---- a LEFT row stays iff pos - end <= (|postfix| - k) + 4, unsigned as the reference takes it (:538); then each
    // (query, shard)'s reads by read_row, a string once
    for (const gt_group_out &o : outs)
        for (const gt_row &r : o.rows) {
            const size_t ri = (size_t)(std::lower_bound(ids.begin(), ids.end(), std::make_pair(r.shard, r.read_row)) - ids.begin());
            const uint32_t q = pl.slot_query[r.item >> 1];
            if (r.pending) {
                if (!gt_left_row_stays(pl.q_pos[q], rec_of(r.shard, r.item).b, r.offset, pl.k, (uint64_t)str[ri].size())) continue;
            }
            (*reads)[(size_t)q * S + r.shard].push_back({r.read_row, std::string()});
            (*reads)[(size_t)q * S + r.shard].back().second = str[ri];
        }
    for (auto &cell : *reads) {
        std::sort(cell.begin(), cell.end());
        std::vector<std::pair<uint64_t, std::string>> kept;
        std::unordered_set<std::string> seen;
        for (auto &pr : cell)
            if (seen.insert(pr.second).second) kept.push_back(std::move(pr));
        cell.swap(kept);
    }
    return RSBWT_OK;
}
}  // namespace

int rsbwt_set_gt_legs(rsbwt_set_t *s, const char *text, const uint64_t *off, size_t Q, const uint64_t *pos, int32_t k, int32_t skip, uint64_t M,
                      uint64_t *first, rsbwt_gt_leg *legs, size_t cap, size_t *nlegs) {
    return guarded("rsbwt_set_gt_legs", [&]() -> int {
        if (!nlegs || (!first && Q)) return fail(RSBWT_EINVAL, "null argument");
        *nlegs = 0;
        std::vector<rsbwt_gt_leg> out;
        std::vector<uint64_t> fq;
        const int rc = gt_call(s, text, off, Q, pos, k, skip, M, &out, &fq, nullptr, 0);
        if (rc) return rc;
        if (first) memcpy(first, fq.data(), (Q + 1) * 8);
        *nlegs = out.size();
        if (out.size() > cap) return fail(RSBWT_ERANGE, "%zu legs, room for %zu", out.size(), cap);
        if (out.empty()) return RSBWT_OK;
        if (!legs) return fail(RSBWT_EINVAL, "null argument");
        memcpy(legs, out.data(), out.size() * sizeof(rsbwt_gt_leg));
        return RSBWT_OK;
    });
}

int rsbwt_set_gt_reads(rsbwt_set_t *s, const char *text, const uint64_t *off, size_t Q, const uint64_t *pos, int32_t k, int32_t skip, uint64_t M,
                       uint64_t *first, char *reads, uint32_t read_stride, uint32_t *read_len, uint64_t *read_row, size_t cap_reads,
                       size_t *nreads) {
    return guarded("rsbwt_set_gt_reads", [&]() -> int {
        if (!nreads || (!first && Q)) return fail(RSBWT_EINVAL, "null argument");
        *nreads = 0;
        if (read_stride == 0) return fail(RSBWT_EINVAL, "read_stride must be positive");
        gt_reads_t res;
        const int rc = gt_call(s, text, off, Q, pos, k, skip, M, nullptr, nullptr, &res, std::max<uint32_t>(read_stride, 256));
        if (rc) return rc;
        size_t total = 0;
        for (size_t c = 0; c < res.size(); ++c) {
            first[c] = total;
            total += res[c].size();
        }
        if (first) first[res.size()] = total;
        *nreads = total;
        if (total > cap_reads) return fail(RSBWT_ERANGE, "%zu reads, room for %zu", total, cap_reads);
        if (total == 0) return RSBWT_OK;
        if (!reads || !read_len) return fail(RSBWT_EINVAL, "null argument");
        size_t r = 0;
        for (const auto &cell : res)
            for (const auto &pr : cell) {
                if (pr.second.size() > read_stride) {
                    read_len[r] = 0xFFFFFFFFu;
                } else {
                    memcpy(reads + r * (size_t)read_stride, pr.second.data(), pr.second.size());
                    read_len[r] = (uint32_t)pr.second.size();
                }
                if (read_row) read_row[r] = pr.first;
                ++r;
            }
        return RSBWT_OK;
    });
}

int rsbwt_set_gt_count(rsbwt_set_t *s, const char *text, const uint64_t *off, size_t Q, const uint64_t *pos, int32_t k, int32_t skip, uint64_t M,
                       uint64_t *counts) {
    return guarded("rsbwt_set_gt_count", [&]() -> int {
        if (!counts && Q) return fail(RSBWT_EINVAL, "null argument");
        gt_reads_t res;
        const int rc = gt_call(s, text, off, Q, pos, k, skip, M, nullptr, nullptr, &res, 256);
        if (rc) return rc;
        for (size_t c = 0; c < res.size(); ++c) counts[c] = res[c].size();
        return RSBWT_OK;
    });
}

void rsbwt_set_gt_last_work(uint64_t *work6) {
    if (work6) memcpy(work6, gt_last_work, sizeof gt_last_work);
}

namespace {
// gt_call's reads cut down to those align_gt_read keeps (ksw_align.hip).  Each device group aligns the reads of its own
// shards against their requests, the groups side by side; a group sends only the requests that have a read there.  The
// known host trip: the reads came down from the extraction as strings and go up again here.
int gt_aligned_call(rsbwt_set_t *s, const char *text, const uint64_t *off, size_t Q, const uint64_t *pos, const char *alt, const uint8_t *isalt,
                    int32_t k, int32_t skip, uint64_t M, gt_reads_t *res, uint32_t stride) {
    gt_align_set_last_work(nullptr);
    if (Q && (!alt || !isalt)) return fail(RSBWT_EINVAL, "null argument");
    int rc = gt_call(s, text, off, Q, pos, k, skip, M, nullptr, nullptr, res, stride);
    if (rc) return rc;
    const size_t S = s->shards.size(), G = s->groups.size();
    std::vector<std::vector<uint8_t>> verdicts(G);
    std::vector<std::vector<uint64_t>> works(G, std::vector<uint64_t>(14, 0));
    rc = for_each_group(s, [&](size_t gi) -> int {
        const dev_group *g = s->groups[gi];
        std::string rbuf, wbuf, walt;
        std::vector<uint64_t> roff{0}, item, woff{0}, wpos;
        std::vector<uint8_t> wisalt;
        for (size_t q = 0; q < Q; ++q) {
            const size_t before = item.size();
            for (size_t p : g->idx)
                for (const auto &pr : (*res)[q * S + p]) {
                    rbuf += pr.second;
                    roff.push_back(rbuf.size());
                    item.push_back(wpos.size());
                }
            if (item.size() == before) continue;
            wbuf.append(text + off[q], (size_t)(off[q + 1] - off[q]));
            woff.push_back(wbuf.size());
            wpos.push_back(pos[q]);
            walt.push_back(alt[q]);
            wisalt.push_back(isalt[q]);
        }
        if (item.empty()) return RSBWT_OK;
        verdicts[gi].resize(item.size());
        return gt_align_host(g->device, rbuf.data(), roff.data(), item.data(), item.size(), wbuf.data(), woff.data(), wpos.data(), walt.data(),
                             wisalt.data(), wpos.size(), verdicts[gi].data(), works[gi].data());
    });
    if (rc) return rc;
    uint64_t work14[14] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (size_t gi = 0; gi < G; ++gi) {
        size_t at = 0;  // (the order the group's batch was made in)
        for (size_t q = 0; q < Q; ++q)
            for (size_t p : s->groups[gi]->idx) {
                auto &cell = (*res)[q * S + p];
                std::vector<std::pair<uint64_t, std::string>> kept;
                for (auto &pr : cell) {
                    const uint8_t v = verdicts[gi][at++];
                    if (v == RSBWT_GT_KEEP_PLAIN || v == RSBWT_GT_KEEP_RIGHT || v == RSBWT_GT_KEEP_LEFT) kept.push_back(std::move(pr));
                }
                cell.swap(kept);
            }
        for (int i = 0; i < 14; ++i) work14[i] += works[gi][i];
    }
    gt_align_set_last_work(work14);
    return RSBWT_OK;
}
}  // namespace

int rsbwt_set_gt_aligned_reads(rsbwt_set_t *s, const char *text, const uint64_t *off, size_t Q, const uint64_t *pos, const char *alt,
                               const uint8_t *isalt, int32_t k, int32_t skip, uint64_t M, uint64_t *first, char *reads, uint32_t read_stride,
                               uint32_t *read_len, uint64_t *read_row, size_t cap_reads, size_t *nreads) {
    return guarded("rsbwt_set_gt_aligned_reads", [&]() -> int {
        if (!nreads || (!first && Q)) return fail(RSBWT_EINVAL, "null argument");
        *nreads = 0;
        if (read_stride == 0) return fail(RSBWT_EINVAL, "read_stride must be positive");
        gt_reads_t res;
        // (every read is fetched whole, whatever the caller's stride: the alignment needs all of it)
        const int rc = gt_aligned_call(s, text, off, Q, pos, alt, isalt, k, skip, M, &res, std::max<uint32_t>(read_stride, 256));
        if (rc) return rc;
        size_t total = 0;
        for (size_t c = 0; c < res.size(); ++c) {
            first[c] = total;
            total += res[c].size();
        }
        if (first) first[res.size()] = total;
        *nreads = total;
        if (total > cap_reads) return fail(RSBWT_ERANGE, "%zu reads, room for %zu", total, cap_reads);
        if (total == 0) return RSBWT_OK;
        if (!reads || !read_len) return fail(RSBWT_EINVAL, "null argument");
        size_t r = 0;
        for (const auto &cell : res)
            for (const auto &pr : cell) {
                if (pr.second.size() > read_stride) {
                    read_len[r] = 0xFFFFFFFFu;
                } else {
                    memcpy(reads + r * (size_t)read_stride, pr.second.data(), pr.second.size());
                    read_len[r] = (uint32_t)pr.second.size();
                }
                if (read_row) read_row[r] = pr.first;
                ++r;
            }
        return RSBWT_OK;
    });
}

int rsbwt_set_gt_aligned_count(rsbwt_set_t *s, const char *text, const uint64_t *off, size_t Q, const uint64_t *pos, const char *alt,
                               const uint8_t *isalt, int32_t k, int32_t skip, uint64_t M, uint64_t *counts) {
    return guarded("rsbwt_set_gt_aligned_count", [&]() -> int {
        if (!counts && Q) return fail(RSBWT_EINVAL, "null argument");
        gt_reads_t res;
        const int rc = gt_aligned_call(s, text, off, Q, pos, alt, isalt, k, skip, M, &res, 256);
        if (rc) return rc;
        for (size_t c = 0; c < res.size(); ++c) counts[c] = res[c].size();
        return RSBWT_OK;
    });
}

// ---- matching statistics (match_stats.hip): the longest supported match at every end position, in every shard ----
namespace {
// Each device group runs its shards' rows of the (position, shard) grid; answers are per (position, shard), so the host
// only puts group gi's row j at row idx[j].  len / lower / upper [S][N] and smems (ordered by (query, shard, end)) are
// each optional.
int match_call(rsbwt_set_t *s, const char *text, const uint64_t *off, size_t Q, uint32_t max_len, uint64_t min_rows, uint32_t *len, uint64_t *lower,
               uint64_t *upper, std::vector<rsbwt_smem> *smems) {
    match_set_last_work(nullptr);
    // (no set can be had on a box without a GPU: the call says so instead of blaming the argument)
    if (!s && rsbwt_device_count() == 0) return fail(RSBWT_ENODEV, "no HIP device is visible: the popBWT engine has no CPU fallback");
    if (!s) return fail(RSBWT_EINVAL, "null set");
    if ((lower == nullptr) != (upper == nullptr)) return fail(RSBWT_EINVAL, "lower and upper: both or neither");
    std::vector<uint64_t> rel;
    size_t N = 0;
    int rc = match_check_batch(text, off, Q, &rel, &N);
    if (rc) return rc;
    if (N == 0) return RSBWT_OK;
    if (!len && !smems) return fail(RSBWT_EINVAL, "null argument");
    const size_t S = s->shards.size();
    for (rsbwt_t *h : s->shards)
        if (h->view.n == 0) return fail(RSBWT_EINVAL, "empty index in the set");
    if (S > 65535) return fail(RSBWT_EINVAL, "%zu shards: at most 65535", S);
    struct group_out {
        std::vector<uint32_t> len;
        std::vector<uint64_t> pairs;
        std::vector<rsbwt_smem> smems;
        uint64_t work[4] = {0, 0, 0, 0};
    };
    std::vector<group_out> outs(s->groups.size());
    rc = for_each_group(s, [&](size_t gi) -> int {
        dev_group *g = s->groups[gi];
        group_call gc(g);
        if (gc.rc) return gc.rc;
        group_out &o = outs[gi];
        const size_t Sg = g->idx.size();
        // (a group whose shards sit next to each other in the set answers straight into the caller's rows)
        const bool straight = g->idx.back() - g->idx.front() + 1 == Sg;
        uint32_t *glen = nullptr;
        if (len) {
            if (straight) glen = len + g->idx.front() * N;
            else {
                o.len.resize(Sg * N);
                glen = o.len.data();
            }
        }
        if (lower) o.pairs.resize(2 * Sg * N);
        return match_host_views(g->scratch, gc.st, g->d_views, (uint32_t)Sg, text + off[0], rel.data(), Q, N, max_len, min_rows, glen,
                                lower ? o.pairs.data() : nullptr, smems ? &o.smems : nullptr, o.work);
    });
    if (rc) return rc;
    uint64_t work6[6] = {(uint64_t)S * N, 0, 0, 0, 0, 0};
    for (size_t gi = 0; gi < outs.size(); ++gi) {
        const dev_group *g = s->groups[gi];
        const group_out &o = outs[gi];
        for (size_t j = 0; j < g->idx.size(); ++j) {
            const size_t p = g->idx[j];
            if (len && !o.len.empty()) memcpy(len + p * N, o.len.data() + j * N, N * 4);
            if (lower)
                for (size_t t = 0; t < N; ++t) {
                    lower[p * N + t] = o.pairs[2 * (j * N + t)];
                    upper[p * N + t] = o.pairs[2 * (j * N + t) + 1];
                }
        }
        for (int i = 0; i < 4; ++i) work6[1 + i] += o.work[i];
        if (smems)
            for (rsbwt_smem r : o.smems) {
                r.shard = (uint32_t)g->idx[r.shard];
                smems->push_back(r);
            }
    }
    if (smems) {
        std::sort(smems->begin(), smems->end(), [](const rsbwt_smem &x, const rsbwt_smem &y) {
            return x.query != y.query ? x.query < y.query : x.shard != y.shard ? x.shard < y.shard : x.end < y.end;
        });
        work6[5] = smems->size();
    }
    match_set_last_work(work6);
    return RSBWT_OK;
}
}  // namespace

int rsbwt_set_match_lengths(rsbwt_set_t *s, const char *text, const uint64_t *off, size_t Q, uint32_t max_len, uint64_t min_rows, uint32_t *len,
                            uint64_t *lower, uint64_t *upper) {
    return guarded("rsbwt_set_match_lengths", [&]() -> int {
        return match_call(s, text, off, Q, max_len, min_rows, len, lower, upper, nullptr);
    });
}

int rsbwt_set_smems(rsbwt_set_t *s, const char *text, const uint64_t *off, size_t Q, uint32_t max_len, uint64_t min_rows, uint64_t *first,
                    rsbwt_smem *out, size_t cap, size_t *nsmems) {
    return guarded("rsbwt_set_smems", [&]() -> int {
        if (!nsmems || (!first && Q)) return fail(RSBWT_EINVAL, "null argument");
        *nsmems = 0;
        std::vector<rsbwt_smem> recs;
        const int rc = match_call(s, text, off, Q, max_len, min_rows, nullptr, nullptr, nullptr, &recs);
        if (rc) return rc;
        const size_t S = s->shards.size();
        if (first) {
            for (size_t c = 0; c <= Q * S; ++c) first[c] = 0;
            for (const rsbwt_smem &r : recs) first[(size_t)r.query * S + r.shard + 1] += 1;
            for (size_t c = 0; c < Q * S; ++c) first[c + 1] += first[c];
        }
        *nsmems = recs.size();
        if (recs.size() > cap) return fail(RSBWT_ERANGE, "%zu SMEMs, room for %zu", recs.size(), cap);
        if (recs.empty()) return RSBWT_OK;
        if (!out) return fail(RSBWT_EINVAL, "null argument");
        memcpy(out, recs.data(), recs.size() * sizeof(rsbwt_smem));
        return RSBWT_OK;
    });
}

int rsbwt_set_match_lengths_dev(rsbwt_set_t *s, const void *d_text, const void *d_off, size_t Q, size_t N, uint32_t max_len, uint64_t min_rows,
                                void *d_len, void *d_pairs, void *stream) {
    dev_group *g = nullptr;
    const int rc = one_device_group(s, &g);
    if (rc) return rc;
    if (Q == 0 || N == 0) return RSBWT_OK;
    if (!d_text || !d_off || !d_len) return fail(RSBWT_EINVAL, "null argument");
    if (N >= (1ull << 31)) return fail(RSBWT_ERANGE, "%zu positions in one call: at most 2^31 - 1", N);
    for (rsbwt_t *h : s->shards)
        if (h->view.n == 0) return fail(RSBWT_EINVAL, "empty index in the set");
    if (s->shards.size() > 65535) return fail(RSBWT_EINVAL, "%zu shards: at most 65535", s->shards.size());
    match_batch bt;
    bt.text = (const char *)d_text;
    bt.off = (const uint64_t *)d_off;
    bt.Q = Q;
    bt.N = N;
    bt.cap = max_len;
    bt.m = min_rows ? min_rows : 1;
    const hipError_t e = launch_match_stats(g->d_views, (uint32_t)g->idx.size(), bt, d_len, d_pairs, nullptr, (hipStream_t)stream);
    return e == hipSuccess ? RSBWT_OK : fail_hip(e, "matching-statistics kernel launch");
}

void rsbwt_set_match_last_work(uint64_t *work6) {
    if (work6) match_get_last_work(work6);
}

// ---- overlaps (overlaps.hip): the reads that begin with a suffix of a query, in every shard ----
namespace {
// Each device group walks its shards' rows of the (query, shard) grid; answers are per (position, shard), so the host
// only puts group gi's row j at row idx[j].  count / ordinal [S][N] and recs (ordered by (query, shard, start)) are each
// optional.
int overlap_call(rsbwt_set_t *s, const char *text, const uint64_t *off, size_t Q, uint32_t min_overlap, uint32_t max_overlap, uint64_t *count,
                 uint64_t *ordinal, std::vector<rsbwt_overlap> *recs) {
    overlap_set_last_work(nullptr);
    // (no set can be had on a box without a GPU: the call says so instead of blaming the argument)
    if (!s && rsbwt_device_count() == 0) return fail(RSBWT_ENODEV, "no HIP device is visible: the popBWT engine has no CPU fallback");
    if (!s) return fail(RSBWT_EINVAL, "null set");
    std::vector<uint64_t> rel;
    size_t N = 0;
    int rc = match_check_batch(text, off, Q, &rel, &N);
    if (rc) return rc;
    if (N == 0) return RSBWT_OK;
    if (!count && !recs) return fail(RSBWT_EINVAL, "null argument");
    const size_t S = s->shards.size();
    for (rsbwt_t *h : s->shards)
        if (h->view.n == 0) return fail(RSBWT_EINVAL, "empty index in the set");
    if (S > 65535) return fail(RSBWT_EINVAL, "%zu shards: at most 65535", S);
    struct group_out {
        std::vector<uint64_t> pairs;
        std::vector<rsbwt_overlap> recs;
        uint64_t work[5] = {0, 0, 0, 0, 0};
    };
    std::vector<group_out> outs(s->groups.size());
    rc = for_each_group(s, [&](size_t gi) -> int {
        dev_group *g = s->groups[gi];
        group_call gc(g);
        if (gc.rc) return gc.rc;
        group_out &o = outs[gi];
        const size_t Sg = g->idx.size();
        if (count) o.pairs.resize(2 * Sg * N);
        return overlap_host_views(g->scratch, gc.st, g->d_views, (uint32_t)Sg, text + off[0], rel.data(), Q, N, min_overlap, max_overlap,
                                  count ? o.pairs.data() : nullptr, recs ? &o.recs : nullptr, o.work);
    });
    if (rc) return rc;
    uint64_t work6[6] = {(uint64_t)S * Q, 0, 0, 0, 0, 0};
    for (size_t gi = 0; gi < outs.size(); ++gi) {
        const dev_group *g = s->groups[gi];
        const group_out &o = outs[gi];
        for (size_t j = 0; count && j < g->idx.size(); ++j) {
            const size_t p = g->idx[j];
            for (size_t t = 0; t < N; ++t) {
                if (ordinal) ordinal[p * N + t] = o.pairs[2 * (j * N + t)];
                count[p * N + t] = o.pairs[2 * (j * N + t) + 1];
            }
        }
        for (int i = 0; i < 5; ++i) work6[1 + i] += o.work[i];
        if (recs)
            for (rsbwt_overlap r : o.recs) {
                r.shard = (uint32_t)g->idx[r.shard];
                recs->push_back(r);
            }
    }
    if (recs)
        std::sort(recs->begin(), recs->end(), [](const rsbwt_overlap &x, const rsbwt_overlap &y) {
            return x.query != y.query ? x.query < y.query : x.shard != y.shard ? x.shard < y.shard : x.start < y.start;
        });
    overlap_set_last_work(work6);
    return RSBWT_OK;
}

// first[] of records ordered by (query, shard): cell c = q * S + p holds records first[c] .. first[c + 1]
void overlap_first(const std::vector<rsbwt_overlap> &recs, size_t cells, size_t S, uint64_t *first) {
    for (size_t c = 0; c <= cells; ++c) first[c] = 0;
    for (const rsbwt_overlap &r : recs) first[(size_t)r.query * S + r.shard + 1] += 1;
    for (size_t c = 0; c < cells; ++c) first[c + 1] += first[c];
}
}  // namespace

int rsbwt_set_overlaps(rsbwt_set_t *s, const char *text, const uint64_t *off, size_t Q, uint32_t min_overlap, uint32_t max_overlap,
                       uint64_t *count, uint64_t *ordinal) {
    return guarded("rsbwt_set_overlaps", [&]() -> int {
        if (s && Q && !count) return fail(RSBWT_EINVAL, "null argument");  // (ordinal alone is not a form of the call)
        return overlap_call(s, text, off, Q, min_overlap, max_overlap, count, ordinal, nullptr);
    });
}

int rsbwt_set_overlap_records(rsbwt_set_t *s, const char *text, const uint64_t *off, size_t Q, uint32_t min_overlap, uint32_t max_overlap,
                              uint64_t *first, rsbwt_overlap *out, size_t cap, size_t *nrecords) {
    return guarded("rsbwt_set_overlap_records", [&]() -> int {
        if (!nrecords || (!first && Q)) return fail(RSBWT_EINVAL, "null argument");
        *nrecords = 0;
        std::vector<rsbwt_overlap> recs;
        const int rc = overlap_call(s, text, off, Q, min_overlap, max_overlap, nullptr, nullptr, &recs);
        if (rc) return rc;
        if (first) overlap_first(recs, Q * s->shards.size(), s->shards.size(), first);
        *nrecords = recs.size();
        if (recs.size() > cap) return fail(RSBWT_ERANGE, "%zu overlap records, room for %zu", recs.size(), cap);
        if (recs.empty()) return RSBWT_OK;
        if (!out) return fail(RSBWT_EINVAL, "null argument");
        memcpy(out, recs.data(), recs.size() * sizeof(rsbwt_overlap));
        return RSBWT_OK;
    });
}

// The reads call is a composition of what exists: the records; per (query, shard) the union of their ordinal ranges taken
// from the longest overlap down, so that a read is reported once, at its longest; the ordinals to rows by getOccAt('$',
// o + 1), a launch per shard; the set extraction.
int rsbwt_set_overlap_reads(rsbwt_set_t *s, const char *text, const uint64_t *off, size_t Q, uint32_t min_overlap, uint32_t max_overlap,
                            uint64_t max_reads, uint64_t *first, char *reads, uint32_t read_stride, uint32_t *read_len, uint32_t *overlap,
                            uint64_t *ordinal, size_t cap_reads, size_t *nreads, uint64_t *matches) {
    return guarded("rsbwt_set_overlap_reads", [&]() -> int {
        if (!nreads || (!first && Q)) return fail(RSBWT_EINVAL, "null argument");
        *nreads = 0;
        if (s)
            for (rsbwt_t *h : s->shards)
                if (!rsbwt_opened_for_reads(h)) return fail(RSBWT_EINVAL, "overlap reads need shards opened with RSBWT_OPEN_READS");
        if (s && Q && read_stride == 0) return fail(RSBWT_EINVAL, "read_stride must be positive");
        std::vector<rsbwt_overlap> recs;
        const int rc = overlap_call(s, text, off, Q, min_overlap, max_overlap, nullptr, nullptr, &recs);
        if (rc) return rc;
        const size_t S = s->shards.size(), cells = Q * S;
        if (first)
            for (size_t c = 0; c <= cells; ++c) first[c] = 0;
        for (size_t c = 0; matches && c < cells; ++c) matches[c] = 0;
        // the records of a cell arrive longest suffix first; what a shorter suffix's range adds are the ordinals no
        // longer one has covered (a range lies inside a later one exactly when the shorter suffix is a prefix of the
        // longer: a periodic query)
        struct piece {
            uint64_t a, b;  // ordinals [a, b)
            uint32_t overlap;
        };
        std::vector<piece> pieces;
        std::vector<size_t> piece_first(cells + 1, 0);
        uint64_t total = 0;
        for (size_t i = 0; i < recs.size();) {
            const size_t cell = (size_t)recs[i].query * S + recs[i].shard;
            std::vector<std::pair<uint64_t, uint64_t>> covered;  // disjoint, ascending
            const size_t p0 = pieces.size();
            uint64_t distinct = 0;
            for (; i < recs.size() && (size_t)recs[i].query * S + recs[i].shard == cell; ++i) {
                const uint64_t a = recs[i].ordinal, b = a + recs[i].count;
                uint64_t at = a;
                std::vector<std::pair<uint64_t, uint64_t>> next;
                size_t k = 0;
                for (; k < covered.size() && covered[k].second <= a; ++k) next.push_back(covered[k]);
                uint64_t lo = a, hi = b;
                for (; k < covered.size() && covered[k].first < b; ++k) {
                    if (covered[k].first > at) pieces.push_back(piece{at, covered[k].first, recs[i].length});
                    at = std::max(at, covered[k].second);
                    lo = std::min(lo, covered[k].first);
                    hi = std::max(hi, covered[k].second);
                }
                if (at < b) pieces.push_back(piece{at, b, recs[i].length});
                next.emplace_back(lo, hi);
                for (; k < covered.size(); ++k) next.push_back(covered[k]);
                covered.swap(next);
            }
            for (size_t k = p0; k < pieces.size(); ++k) distinct += pieces[k].b - pieces[k].a;
            if (matches) matches[cell] = distinct;
            if (max_reads && distinct > max_reads) pieces.resize(p0);  // over the limit: none, and nobody else's are touched
            else total += distinct;
            piece_first[cell + 1] = pieces.size();
        }
        for (size_t c = 0; c < cells; ++c) piece_first[c + 1] = std::max(piece_first[c + 1], piece_first[c]);
        if (first) {
            uint64_t run = 0;
            for (size_t c = 0; c < cells; ++c) {
                first[c] = run;
                for (size_t k = piece_first[c]; k < piece_first[c + 1]; ++k) run += pieces[k].b - pieces[k].a;
            }
            first[cells] = run;
        }
        *nreads = (size_t)total;
        if (total > cap_reads) return fail(RSBWT_ERANGE, "%llu reads over the set, room for %zu", (unsigned long long)total, cap_reads);
        if (total == 0) return RSBWT_OK;
        if (!reads || !read_len) return fail(RSBWT_EINVAL, "null argument");
        // the ordinals in the caller's order, then per shard their rows: getOccAt('$', o + 1)
        std::vector<uint32_t> shard_of((size_t)total);
        std::vector<uint64_t> ords((size_t)total), rows((size_t)total);
        size_t r = 0;
        for (size_t c = 0; c < cells; ++c)
            for (size_t k = piece_first[c]; k < piece_first[c + 1]; ++k)
                for (uint64_t o = pieces[k].a; o < pieces[k].b; ++o, ++r) {
                    shard_of[r] = (uint32_t)(c % S);
                    ords[r] = o;
                    if (overlap) overlap[r] = pieces[k].overlap;
                    if (ordinal) ordinal[r] = o;
                }
        for (size_t p = 0; p < S; ++p) {
            std::vector<size_t> where;
            std::vector<uint64_t> bc;
            for (size_t t = 0; t < (size_t)total; ++t)
                if (shard_of[t] == p) {
                    where.push_back(t);
                    bc.push_back(ords[t] + 1);
                }
            if (where.empty()) continue;
            const std::vector<char> syms(where.size(), '$');
            std::vector<uint64_t> got(where.size());
            const int ro = rsbwt_occ_at_batch(s->shards[p], syms.data(), bc.data(), bc.size(), got.data());
            if (ro) return ro;
            for (size_t t = 0; t < where.size(); ++t) rows[where[t]] = got[t];
        }
        return rsbwt_set_extract_body(s, shard_of.data(), rows.data(), (size_t)total, reads, read_stride, read_len, nullptr);
    });
}

int rsbwt_set_overlaps_dev(rsbwt_set_t *s, const void *d_text, const void *d_off, size_t Q, size_t N, uint32_t min_overlap,
                           uint32_t max_overlap, void *d_pairs, void *stream) {
    dev_group *g = nullptr;
    const int rc = one_device_group(s, &g);
    if (rc) return rc;
    if (Q == 0 || N == 0) return RSBWT_OK;
    if (!d_text || !d_off || !d_pairs) return fail(RSBWT_EINVAL, "null argument");
    if (N >= (1ull << 31)) return fail(RSBWT_ERANGE, "%zu positions in one call: at most 2^31 - 1", N);
    for (rsbwt_t *h : s->shards)
        if (h->view.n == 0) return fail(RSBWT_EINVAL, "empty index in the set");
    if (s->shards.size() > 65535) return fail(RSBWT_EINVAL, "%zu shards: at most 65535", s->shards.size());
    overlap_batch bt;
    bt.text = (const char *)d_text;
    bt.off = (const uint64_t *)d_off;
    bt.Q = Q;
    bt.N = N;
    bt.min_overlap = min_overlap ? min_overlap : 1u;
    bt.max_overlap = max_overlap;
    const hipError_t e = launch_overlaps(g->d_views, (uint32_t)g->idx.size(), bt, d_pairs, nullptr, nullptr, (hipStream_t)stream);
    return e == hipSuccess ? RSBWT_OK : fail_hip(e, "overlap kernel launch");
}

void rsbwt_set_overlap_last_work(uint64_t *work6) {
    if (work6) overlap_get_last_work(work6);
}

static size_t hits_1mm_scratch_one(const rsbwt_set_t *s, size_t m, uint32_t k) {
    size_t need = 0;
    for (rsbwt_t *h : s->shards) need = std::max(need, rsbwt_hits_1mm_scratch_bytes(h, m, k));
    return (need + 255) & ~(size_t)255;
}

// scratch of a set's hit-list search: the batch's variants, expanded ONCE for all shards (they depend on the k-mers
// alone), then a slot per shard that works at the same time (or the fused launches' parts)
size_t rsbwt_set_hits_1mm_scratch_bytes(const rsbwt_set_t *s, size_t m, uint32_t k) {
    if (!s) return 0;
    const size_t one = hits_1mm_scratch_one(s, m, k);
    const bool side = s->shards.size() > 1 && m * (3 * (size_t)k + 1) < SIDE_BY_SIDE_BELOW;
    const size_t slots = side ? std::min<size_t>(s->shards.size(), dev_group::FORK) : 1;
    fused_1mm_layout L;
    const size_t fused = fused_1mm_applies(s, m, k, &L) ? L.total : 0;
    return ((variants_bytes(m, k) + 255) & ~(size_t)255) + std::max(one * slots, fused);
}

// 1: rsbwt_set_hits_1mm_dev of m k-mers runs as the fused launches (for a caller that prices them: bench.py)
int rsbwt_set_hits_1mm_is_fused(const rsbwt_set_t *s, size_t m, uint32_t k) {
    fused_1mm_layout L;
    static const bool turns_only = knob_set("RSBWT_SET_1MM_TURNS");
    return s && m && k && !turns_only && fused_1mm_applies(s, m, k, &L) ? 1 : 0;
}

static int set_hits_1mm_fused(rsbwt_set_t *s, dev_group *g, const fused_1mm_layout &L, const void *d_packed, const void *d_valid,
                              size_t m, uint32_t k, void *d_hits, size_t cap_per_shard, void *d_totals, const uint8_t *d_var,
                              uint8_t *d_parts, hipStream_t st) {
    const uint32_t S = (uint32_t)s->shards.size();
    const size_t mv = m * (3 * (size_t)k + 1);
    uint8_t *d_trace = d_parts, *d_own = d_trace + L.trace, *d_sparse = d_own + L.own, *d_bits = d_sparse + L.sparse;
    uint8_t *d_blocks = d_bits + L.bits;
    HIP_OK(hipMemsetAsync(d_bits, 0, (size_t)S * hit_map_words(mv) * 8, st));
    int rc;
    if (L.worklist) {
        // the k-mers traced; the step of the three substitutions of every traced position off one fetch, the variants
        // inside the tables' reach from their table entries: worklists of live searches; then ONE launch runs them
        // (d_pre: the table entries of the variants inside the tables' reach, read ahead for all shards by the worklist
        // launch's first kernel: mm1_worklist.hip, wl_table_entries_kernel)
        uint8_t *d_wl = d_blocks + L.blocks, *d_counts = d_wl + L.wl, *d_pre = L.pre ? d_counts + L.counts : nullptr;
        static const bool no_walk = knob_set("RSBWT_SET_1MM_NO_WALK");  // A/B knob (tools/README.md): the traced launch + the branch kernel
        if (!no_walk) {
            // ONE walk of the k-mers: their own searches, and at every position left of the tables' reach the step of the
            // three substitutions off the same fetch -- the survivors appended to the worklists (search_solo.h, WALK)
            HIP_OK(hipMemsetAsync(d_counts, 0, L.counts, st));
            if ((rc = search_launch_walk(*g, g->d_views, S, g->num_cus, d_packed, d_valid, m, L.tn, d_wl, d_counts, L.wl_cap, k, d_sparse, d_bits, st)) != RSBWT_OK) return rc;
        } else {
            search_extra traced;
            traced.d_trace_out = d_trace;
            traced.trace_n = L.tn;
            traced.pairs = true;
            if ((rc = search_launch(*g, g->d_views, S, g->num_cus, d_packed, d_valid, m, k, d_own, nullptr, false, st, &traced)) != RSBWT_OK) return rc;
            const hipError_t ew = launch_mm1_worklists(g->d_views, S, d_packed, d_valid, m, k, L.tn, d_trace, d_own, d_wl, L.wl_cap, d_counts,
                                                       d_sparse, d_bits, g->num_cus, st, g->counting ? g->d_work : nullptr);
            if (ew != hipSuccess) return fail_hip(ew, "worklist kernels");
        }
        rc = search_launch_worklist(*g, g->d_views, S, g->num_cus, d_packed, d_valid, m, L.tn, d_wl, d_counts, L.wl_cap, k, d_sparse, d_bits, st, d_pre);
    } else {
        rc = fused_1mm_launches(s, g, L, d_packed, d_valid, m, k, d_var, d_trace, d_own, d_sparse, nullptr, d_bits, st);
    }
    if (rc) return rc;
    const hipError_t e = launch_compact_hits(d_bits, d_sparse, mv, d_hits, cap_per_shard, d_totals, d_blocks, st, S);
    return e == hipSuccess ? RSBWT_OK : fail_hip(e, "hit list kernels");
}

// d_hits: [num_shards][cap_per_shard] records of 32 B (rsbwt_hits_1mm_dev's), d_totals: u64[num_shards]
int rsbwt_set_hits_1mm_dev(rsbwt_set_t *s, const void *d_packed, const void *d_valid, size_t m, uint32_t k, void *d_hits,
                           size_t cap_per_shard, void *d_totals, void *d_scratch, void *stream) {
    dev_group *g = nullptr;
    int rc = one_device_group(s, &g);
    if (rc) return rc;
    if (!d_totals || (!d_hits && cap_per_shard)) return fail(RSBWT_EINVAL, "null argument");
    const size_t S = s->shards.size();
    if (m == 0) {
        HIP_OK(hipMemsetAsync(d_totals, 0, 8 * S, (hipStream_t)stream));
        return RSBWT_OK;
    }
    if (!d_packed || !d_valid || !d_scratch) return fail(RSBWT_EINVAL, "null argument");
    if (k == 0) return fail(RSBWT_EINVAL, "k must be at least 1");
    static const bool turns_only = knob_set("RSBWT_SET_1MM_TURNS");  // A/B knob (tools/README.md)
    const bool side = !turns_only && S > 1 && m * (3 * (size_t)k + 1) < SIDE_BY_SIDE_BELOW;
    const size_t one = hits_1mm_scratch_one(s, m, k);
    uint8_t *d_var = (uint8_t *)d_scratch, *d_slots = d_var + ((variants_bytes(m, k) + 255) & ~(size_t)255);
    fused_1mm_layout FL;
    const bool fused = !turns_only && fused_1mm_applies(s, m, k, &FL);
    // (the worklist form spells no variants out)
    if (!(fused && FL.worklist) && (rc = variants_of_batch_dev(d_packed, d_valid, m, k, d_var, (hipStream_t)stream)) != RSBWT_OK) return rc;
    if (fused)
        return set_hits_1mm_fused(s, g, FL, d_packed, d_valid, m, k, d_hits, cap_per_shard, d_totals, d_var, d_slots, (hipStream_t)stream);
    auto one_shard = [&](size_t i, uint8_t *slot, hipStream_t st) {
        return hits_1mm_dev_shared(s->shards[i], d_packed, d_valid, m, k, (uint8_t *)d_hits + i * cap_per_shard * 32, cap_per_shard,
                                   (uint8_t *)d_totals + i * 8, slot, st, d_var);
    };
    if (!side) {
        for (size_t i = 0; i < S; ++i)
            if ((rc = one_shard(i, d_slots, (hipStream_t)stream)) != RSBWT_OK) return rc;
        return RSBWT_OK;
    }
    std::lock_guard<std::mutex> lock(g->fork_mu);  // one fork / join sequence at a time uses the side streams' events
    if ((rc = g->ensure_fork()) != RSBWT_OK) return rc;
    HIP_OK(hipEventRecord(g->fork_ev, (hipStream_t)stream));  // (behind the variants)
    // (a failure inside the loop leaves it through `rc`, never by returning: what was already enqueued on the side
    // streams reads and writes the caller's buffers and is joined below before the caller's stream goes on)
    auto hip_rc = [](hipError_t e, const char *what) { return e == hipSuccess ? RSBWT_OK : fail_hip(e, what); };
    for (size_t i = 0; i < S && rc == RSBWT_OK; ++i) {
        hipStream_t st = g->fork_st[i % dev_group::FORK];
        if ((rc = hip_rc(hipStreamWaitEvent(st, g->fork_ev, 0), "hipStreamWaitEvent")) != RSBWT_OK) break;
        if ((rc = one_shard(i, d_slots + (i % dev_group::FORK) * one, st)) != RSBWT_OK) break;
        if (i + dev_group::FORK >= S) {  // the last shard of each side stream: its event joins the caller's stream
            if ((rc = hip_rc(hipEventRecord(g->join_ev[i % dev_group::FORK], st), "hipEventRecord")) != RSBWT_OK) break;
            rc = hip_rc(hipStreamWaitEvent((hipStream_t)stream, g->join_ev[i % dev_group::FORK], 0), "hipStreamWaitEvent");
        }
    }
    if (rc) {  // whatever was enqueued still finishes before the caller's stream goes on
        for (int i = 0; i < dev_group::FORK; ++i) {
            if (hipEventRecord(g->join_ev[i], g->fork_st[i]) == hipSuccess) (void)hipStreamWaitEvent((hipStream_t)stream, g->join_ev[i], 0);
        }
    }
    return rc;
}

// d_rows: [num_shards][n] SA rows (row numbers are per shard); d_out [num_shards][n][stride], d_len / d_prefix_len [num_shards][n].
// ONE launch sequence walks the rows of all the shards (extract_lines.hip): a walk kernel ends in a tail as long as its
// longest walk, and a launch per shard -- round 3: side by side on streams of the set -- has a tail per shard and a
// fraction of the rows per lane.
int rsbwt_set_extract_dev(rsbwt_set_t *s, const void *d_rows, size_t n, void *d_out, uint32_t stride, void *d_len,
                          void *d_prefix_len, void *stream) {
    dev_group *g = nullptr;
    int rc = one_device_group(s, &g);
    if (rc) return rc;
    if (n == 0) return RSBWT_OK;
    if (!d_rows || !d_out || !d_len || !d_prefix_len) return fail(RSBWT_EINVAL, "null argument");
    if (stride == 0) return fail(RSBWT_EINVAL, "stride must be positive");
    const size_t S = s->shards.size();
    static const bool turns_only = knob_set("RSBWT_SET_EXTRACT_TURNS");  // A/B knob (tools/README.md): a launch sequence per shard
    if (turns_only || n > (1ull << 31)) {
        for (size_t i = 0; i < S; ++i) {
            rc = rsbwt_extract_dev(s->shards[i], (const uint8_t *)d_rows + i * n * 8, n, (uint8_t *)d_out + i * n * (size_t)stride,
                                   stride, (uint8_t *)d_len + i * n * 4, (uint8_t *)d_prefix_len + i * n * 4, stream);
            if (rc) return rc;
        }
        return RSBWT_OK;
    }
    if ((rc = ensure_group_xviews(s, g, (hipStream_t)stream)) != RSBWT_OK) return rc;
    unsigned long long *work = nullptr;
    if (g->counting) {  // rsbwt_set_set_counting: the walk kernels' counters over all shards, read with rsbwt_set_last_search_counters
        work = g->d_work;
        HIP_OK(hipMemsetAsync(work, 0, WORK_WORDS * sizeof(unsigned long long), (hipStream_t)stream));
    }
    const hipError_t e = launch_extract_wave(g->scratch, g->d_xviews, (uint32_t)S, d_rows, n, d_out, stride, d_prefix_len, d_len, g->num_cus,
                                             (hipStream_t)stream, work);
    if (e != hipSuccess) return fail_hip(e, "extract kernel launch");
    return RSBWT_OK;
}

}  // extern "C"

// ---- the per-read sample table (read_meta.hip): build / load / clear, and the lookups by ordinal and by string ----
namespace {

// the calling thread's last lookup: items, items with a value, value bytes copied, LF steps of the string searches
thread_local uint64_t meta_last_work[4] = {0, 0, 0, 0};

inline size_t meta_head_words(uint64_t num_strings) { return (size_t)((num_strings + 31) / 32); }

// what a build allocates on the way and lets go of when it leaves, however it leaves
struct dev_tmp {
    std::vector<void *> p;
    ~dev_tmp() {
        for (void *x : p) (void)hipFree(x);
    }
    hipError_t get(size_t bytes, void **out) {
        *out = nullptr;
        const hipError_t e = hipMalloc(out, bytes ? bytes : 1);
        if (e == hipSuccess) p.push_back(*out);
        return e;
    }
};

// One shard's table from the pairs' (ordinal, copies) in that shard (ord / cp: n entries), on the current device.  Three
// passes over the pairs in chunks: winners (atomicMax of index + 1 per ordinal), the winners' lengths -> scan -> off[],
// the winners' bytes from each uploaded chunk of values into the table (read_meta.hip's copy kernel).
int meta_build_shard(hipStream_t st, uint64_t ns, const uint64_t *ord, const uint64_t *cp, const uint8_t *values, const uint64_t *voff, size_t n,
                     rsbwt_set::meta_shard *out, uint64_t *bytes, uint64_t *given) {
    const size_t CH = (size_t)1 << 20;           // pairs per chunk
    const uint64_t VB = (uint64_t)64 << 20;      // value bytes per chunk (one value may be longer: a chunk of its own)
    dev_tmp tmp;
    void *d_win, *d_len, *d_src, *d_given, *d_a, *d_b, *d_voff, *d_scan;
    const size_t m_max = std::min(n, CH), scan_bytes = meta_scan_bytes(ns + 1);
    HIP_OK(tmp.get((ns + 1) * 8, &d_win));
    HIP_OK(tmp.get((ns + 1) * 8, &d_len));
    HIP_OK(tmp.get((ns + 1) * 8, &d_src));
    HIP_OK(tmp.get(8, &d_given));
    HIP_OK(tmp.get(m_max * 8, &d_a));
    HIP_OK(tmp.get(m_max * 8, &d_b));
    HIP_OK(tmp.get((m_max + 1) * 8, &d_voff));
    HIP_OK(tmp.get(scan_bytes, &d_scan));
    HIP_OK(hipMemsetAsync(d_win, 0, (ns + 1) * 8, st));
    HIP_OK(hipMemsetAsync(d_len, 0, (ns + 1) * 8, st));
    HIP_OK(hipMemsetAsync(d_given, 0, 8, st));
    const size_t head_bytes = meta_head_words(ns) * 4;
    HIP_OK(hipMalloc((void **)&out->d_heads, head_bytes ? head_bytes : 4));
    HIP_OK(hipMemsetAsync(out->d_heads, 0, head_bytes ? head_bytes : 4, st));
    hipError_t e;
    for (size_t c0 = 0; c0 < n; c0 += CH) {
        const size_t m = std::min(CH, n - c0);
        HIP_OK(hipMemcpyAsync(d_a, ord + c0, m * 8, hipMemcpyHostToDevice, st));
        HIP_OK(hipMemcpyAsync(d_b, cp + c0, m * 8, hipMemcpyHostToDevice, st));
        if ((e = launch_meta_winners(d_a, d_b, m, c0, d_win, ns, st)) != hipSuccess) return fail_hip(e, "winner kernel launch");
        if ((e = launch_meta_heads(d_a, d_b, m, out->d_heads, ns, st)) != hipSuccess) return fail_hip(e, "head-bit kernel launch");
    }
    for (size_t c0 = 0; c0 < n; c0 += CH) {
        const size_t m = std::min(CH, n - c0);
        HIP_OK(hipMemcpyAsync(d_voff, voff + c0, (m + 1) * 8, hipMemcpyHostToDevice, st));
        if ((e = launch_meta_winner_values(d_win, ns, d_voff, c0, c0 + m, d_len, nullptr, d_given, st)) != hipSuccess)
            return fail_hip(e, "winner-length kernel launch");
    }
    HIP_OK(hipMalloc((void **)&out->d_off, (ns + 1) * 8));
    if ((e = launch_meta_scan(d_scan, scan_bytes, d_len, out->d_off, ns + 1, st)) != hipSuccess) return fail_hip(e, "offset scan");
    uint64_t total = 0;
    HIP_OK(hipMemcpyAsync(&total, out->d_off + ns, 8, hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(given, d_given, 8, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    HIP_OK(hipMalloc((void **)&out->d_bytes, total ? total : 1));
    *bytes = total;
    void *d_val = nullptr;
    uint64_t val_room = 0;
    for (size_t c0 = 0; c0 < n && total;) {
        size_t c1 = c0 + 1;
        while (c1 < n && c1 - c0 < CH && voff[c1 + 1] - voff[c0] <= VB) ++c1;
        const uint64_t vb = voff[c1] - voff[c0];
        if (vb) {
            if (vb > val_room) {
                HIP_OK(hipStreamSynchronize(st));
                HIP_OK(tmp.get(vb, &d_val));  // (the smaller one goes with the rest)
                val_room = vb;
            }
            HIP_OK(hipMemcpyAsync(d_val, values + voff[c0], vb, hipMemcpyHostToDevice, st));
            HIP_OK(hipMemcpyAsync(d_voff, voff + c0, (c1 - c0 + 1) * 8, hipMemcpyHostToDevice, st));
            if ((e = launch_meta_winner_values(d_win, ns, d_voff, c0, c1, nullptr, d_src, nullptr, st)) != hipSuccess)
                return fail_hip(e, "winner-offset kernel launch");
            if ((e = launch_meta_copy(nullptr, 1, nullptr, 0, d_val, d_src, out->d_off, ns, out->d_bytes, total, st)) != hipSuccess)
                return fail_hip(e, "value copy kernel launch");
        }
        c0 = c1;
    }
    HIP_OK(hipStreamSynchronize(st));
    return RSBWT_OK;
}

// the tables' views, as the lookups of group g read them
int meta_publish(rsbwt_set_t *s) {
    for (dev_group *g : s->groups) {
        int rc = use_device(g->device);
        if (rc) return rc;
        std::vector<meta_view> v;
        for (size_t i : g->idx) {
            meta_view mv = {nullptr, nullptr, 0, nullptr};
            if (!s->meta.empty()) mv = {s->meta[i].d_off, s->meta[i].d_bytes, s->shards[i]->view.C[1], s->meta[i].d_heads};
            v.push_back(mv);
        }
        if (!g->d_meta) HIP_OK(hipMalloc((void **)&g->d_meta, v.size() * sizeof(meta_view)));
        HIP_OK(hipMemcpy(g->d_meta, v.data(), v.size() * sizeof(meta_view), hipMemcpyHostToDevice));
    }
    return RSBWT_OK;
}

void meta_free_tables(rsbwt_set_t *s, std::vector<rsbwt_set::meta_shard> &tabs) {
    for (size_t i = 0; i < tabs.size(); ++i) {
        if (!tabs[i].d_off && !tabs[i].d_bytes && !tabs[i].d_heads) continue;
        (void)hipSetDevice(s->shards[i]->device);
        if (tabs[i].d_off) (void)hipFree(tabs[i].d_off);
        if (tabs[i].d_bytes) (void)hipFree(tabs[i].d_bytes);
        if (tabs[i].d_heads) (void)hipFree(tabs[i].d_heads);
    }
    tabs.clear();
}

int set_meta_build_body(rsbwt_set_t *s, const char *text, const uint64_t *off, const uint8_t *values, const uint64_t *voff, size_t n,
                        uint64_t *stats4) {
    if (!s) return fail(RSBWT_EINVAL, "null set");
    if (n && (!off || !voff || (!text && off[n] != off[0]) || (!values && voff[n] != voff[0]))) return fail(RSBWT_EINVAL, "null argument");
    for (size_t i = 0; i < n; ++i)
        if (voff[i + 1] < voff[i]) return fail(RSBWT_EINVAL, "pair %zu: its value's end lies before its start", i);
    for (rsbwt_t *h : s->shards)
        if (h->view.n == 0) return fail(RSBWT_EINVAL, "empty index in the set");
    const size_t S = s->shards.size();
    std::vector<uint64_t> ord(S * n), cp(S * n);
    int rc = n ? rsbwt_set_read_copies_var_body(s, text, off, n, cp.data(), nullptr, ord.data()) : RSBWT_OK;
    if (rc) return rc;
    std::vector<rsbwt_set::meta_shard> tabs(S);
    std::vector<uint64_t> bytes(S, 0), given(S, 0);
    rc = for_each_group(s, [&](size_t gi) -> int {
        dev_group *g = s->groups[gi];
        group_call gc(g);
        if (gc.rc) return gc.rc;
        for (size_t i : g->idx) {
            const int rb = meta_build_shard(gc.st, s->shards[i]->view.C[1], ord.data() + i * n, cp.data() + i * n, values, voff, n, &tabs[i],
                                            &bytes[i], &given[i]);
            if (rb) return rb;
        }
        return RSBWT_OK;
    });
    if (rc) {
        meta_free_tables(s, tabs);
        return rc;
    }
    meta_free_tables(s, s->meta);
    s->meta = std::move(tabs);
    s->meta_bytes = 0;
    s->meta_head_bytes = 0;
    uint64_t st[4] = {0, 0, 0, 0};
    for (size_t i = 0; i < S; ++i) {
        s->meta_bytes += (s->shards[i]->view.C[1] + 1) * 8 + bytes[i];
        s->meta_head_bytes += meta_head_words(s->shards[i]->view.C[1]) * 4;
        st[2] += given[i];
        st[3] += bytes[i];
    }
    for (size_t q = 0; q < n; ++q) {
        bool any = false;
        for (size_t i = 0; i < S && !any; ++i) any = cp[i * n + q] != 0;
        st[any ? 0 : 1] += 1;
    }
    if (stats4) memcpy(stats4, st, sizeof st);
    return meta_publish(s);
}

// One device group's items (shards as the group numbers them; sh nullptr: its shard 0): first[m + 1] always; the bytes
// into `bytes` when they fit cap, or into *own (resized) when that is given.
int meta_group_lookup(dev_group *g, const uint32_t *sh, const uint64_t *od, size_t m, uint64_t *first, uint8_t *bytes, size_t cap,
                      std::vector<uint8_t> *own) {
    group_call gc(g, true);
    if (gc.rc) return gc.rc;
    hipStream_t st = gc.st;
    const size_t a4 = al256(m * 4), a8 = al256((m + 1) * 8), a_tmp = meta_scan_bytes(m + 1);
    hipError_t e = g->scratch.take(a4 + 4 * a8 + a_tmp, st, &gc.la);
    if (e != hipSuccess) return fail_hip(e, "scratch for a sample lookup");
    uint8_t *d_sh = (uint8_t *)gc.la.p, *d_od = d_sh + a4, *d_len = d_od + a8, *d_src = d_len + a8, *d_first = d_src + a8, *d_tmp = d_first + a8;
    if (sh) HIP_OK(hipMemcpyAsync(d_sh, sh, m * 4, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(d_od, od, m * 8, hipMemcpyHostToDevice, st));
    const uint32_t S = (uint32_t)g->idx.size();
    if ((e = launch_meta_sizes(g->d_meta, S, sh ? d_sh : nullptr, d_od, nullptr, 0, m, d_len, d_src, st)) != hipSuccess)
        return fail_hip(e, "sample sizes kernel launch");
    if ((e = launch_meta_scan(d_tmp, a_tmp, d_len, d_first, m + 1, st)) != hipSuccess) return fail_hip(e, "sample offsets scan");
    HIP_OK(hipMemcpyAsync(first, d_first, (m + 1) * 8, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    const uint64_t total = first[m];
    if (own) own->resize(total);
    else if (total > cap) return RSBWT_OK;  // (the caller reports the size)
    if (total == 0) return RSBWT_OK;
    if ((e = g->scratch.take(total, st, &gc.lb)) != hipSuccess)
        return fail(RSBWT_ENOMEM, "%llu value bytes do not fit the device's free memory: %s", (unsigned long long)total, hipGetErrorString(e));
    if ((e = launch_meta_copy(g->d_meta, S, sh ? d_sh : nullptr, 0, nullptr, d_src, d_first, m, gc.lb.p, total, st)) != hipSuccess)
        return fail_hip(e, "sample copy kernel launch");
    HIP_OK(hipMemcpyAsync(own ? own->data() : bytes, gc.lb.p, total, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    return RSBWT_OK;
}

int set_meta_by_ordinal_body(rsbwt_set_t *s, const uint32_t *shard_of, const uint64_t *ordinal, size_t n, uint64_t *first, uint8_t *bytes,
                             size_t cap, size_t *nbytes) {
    const size_t S = s->shards.size();
    for (size_t i = 0; i < n; ++i)
        if (shard_of[i] >= S) return fail(RSBWT_EINVAL, "item %zu names shard %u of %zu", i, shard_of[i], S);
    if (s->groups.size() == 1) {
        const int rc = meta_group_lookup(s->groups[0], shard_of, ordinal, n, first, bytes, bytes ? cap : 0, nullptr);
        if (rc) return rc;
    } else {
        // several device groups: each gathers its share where its tables are; the host lays the values out in the order asked
        const size_t G = s->groups.size();
        std::vector<group_share> share(G);
        std::vector<std::vector<uint64_t>> gfirst(G);
        std::vector<std::vector<uint8_t>> gbytes(G);
        const int rc = for_each_group(s, [&](size_t gi) -> int {
            share[gi] = share_of_group(s, s->groups[gi], shard_of, ordinal, n);
            const size_t m = share[gi].pos.size();
            gfirst[gi].assign(m + 1, 0);
            if (m == 0) return RSBWT_OK;
            return meta_group_lookup(s->groups[gi], share[gi].shard.data(), share[gi].rows.data(), m, gfirst[gi].data(), nullptr, 0, &gbytes[gi]);
        });
        if (rc) return rc;
        for (size_t gi = 0; gi < G; ++gi)
            for (size_t t = 0; t < share[gi].pos.size(); ++t) first[share[gi].pos[t] + 1] = gfirst[gi][t + 1] - gfirst[gi][t];
        first[0] = 0;
        for (size_t i = 0; i < n; ++i) first[i + 1] += first[i];
        if (bytes && first[n] <= cap)
            for (size_t gi = 0; gi < G; ++gi)
                for (size_t t = 0; t < share[gi].pos.size(); ++t) {
                    const uint64_t l = gfirst[gi][t + 1] - gfirst[gi][t];
                    if (l) memcpy(bytes + first[share[gi].pos[t]], gbytes[gi].data() + gfirst[gi][t], l);
                }
    }
    *nbytes = (size_t)first[n];
    meta_last_work[0] = n;
    for (size_t i = 0; i < n; ++i) meta_last_work[1] += first[i + 1] != first[i];
    if (first[n] > (bytes ? cap : 0)) return fail(RSBWT_ERANGE, "%llu value bytes, room for %zu", (unsigned long long)first[n], bytes ? cap : 0);
    meta_last_work[2] = first[n];
    return RSBWT_OK;
}

// One device group holding every shard: per slice of the batch the whole-read search, the sizes, the scan and the copy run
// in HBM; the slice's first[] and copies cross to the host before its bytes (they size them), the bytes after.
int meta_read_device(rsbwt_set_t *s, const char *text, const uint64_t *off, size_t Q, uint64_t *first, uint8_t *bytes, size_t cap,
                     uint64_t *copies, uint64_t *lf_steps) {
    dev_group *g = s->groups[0];
    group_call gc(g, true);
    if (gc.rc) return gc.rc;
    hipStream_t st = gc.st;
    const uint32_t S = (uint32_t)g->idx.size();
    auto a_scr = [&](size_t mq) { return al256(read_copies_scratch_bytes(S, mq)); };
    auto a_res = [&](size_t mq) { return al256((size_t)S * mq * 8 + 8); };
    uint64_t base = 0;
    std::vector<uint64_t> hf;
    const int rc = for_each_var_slice(
        *gc.c, st, text, off, Q, [&](size_t mq) { return a_scr(mq) + 5 * a_res(mq) + meta_scan_bytes(S * mq + 1); },
        [&](size_t q0, size_t mq) -> int {
            for (size_t i = 0; i < mq * S; ++i) first[q0 * S + i] = base;
            if (copies)
                for (uint32_t p = 0; p < S; ++p) memset(copies + p * Q + q0, 0, mq * 8);
            return RSBWT_OK;
        },
        [&](const var_slice &sl) -> int {
            const size_t q0 = sl.q0, mq = sl.mq, items = mq * S, a_tmp = meta_scan_bytes(items + 1);
            uint8_t *d_scr = sl.d_extra, *d_cp = d_scr + a_scr(mq), *d_od = d_cp + a_res(mq), *d_len = d_od + a_res(mq), *d_src = d_len + a_res(mq),
                    *d_first = d_src + a_res(mq), *d_tmp = d_first + a_res(mq);
            int r = read_copies_launch(*g, g->d_views, S, g->num_cus, sl.d_pk, sl.d_ok, sl.d_len, mq, sl.k, d_scr, d_cp, nullptr, st, d_od);
            if (r) return r;
            unsigned long long w0 = 0;
            if (g->counting) HIP_OK(hipMemcpyAsync(&w0, g->d_work, sizeof w0, hipMemcpyDeviceToHost, st));
            hipError_t e = launch_meta_sizes(g->d_meta, S, nullptr, d_od, d_cp, mq, items, d_len, d_src, st);
            if (e != hipSuccess) return fail_hip(e, "sample sizes kernel launch");
            if ((e = launch_meta_scan(d_tmp, a_tmp, d_len, d_first, items + 1, st)) != hipSuccess) return fail_hip(e, "sample offsets scan");
            hf.resize(items + 1);
            HIP_OK(hipMemcpyAsync(hf.data(), d_first, (items + 1) * 8, hipMemcpyDeviceToHost, st));
            if (copies)
                for (uint32_t p = 0; p < S; ++p) HIP_OK(hipMemcpyAsync(copies + p * Q + q0, d_cp + (size_t)p * mq * 8, mq * 8, hipMemcpyDeviceToHost, st));
            HIP_OK(hipStreamSynchronize(st));
            *lf_steps += w0;
            const uint64_t total = hf[items];
            for (size_t i = 0; i < items; ++i) first[q0 * S + i] = base + hf[i];
            if (total && bytes && base + total <= cap) {
                scratch_cache::lease mem;
                if ((e = g->scratch.take(total, st, &mem)) != hipSuccess)
                    return fail(RSBWT_ENOMEM, "%llu value bytes do not fit the device's free memory: %s", (unsigned long long)total, hipGetErrorString(e));
                e = launch_meta_copy(g->d_meta, S, nullptr, mq, nullptr, d_src, d_first, items, mem.p, total, st);
                if (e == hipSuccess) e = hipMemcpyAsync(bytes + base, mem.p, total, hipMemcpyDeviceToHost, st);
                if (e == hipSuccess) e = hipStreamSynchronize(st);
                g->scratch.give(mem, st);
                if (e != hipSuccess) return fail_hip(e, "sample copy");
            }
            base += total;
            return RSBWT_OK;
        });
    if (rc) return rc;
    first[Q * S] = base;
    return RSBWT_OK;
}

int set_read_meta_var_body(rsbwt_set_t *s, const char *text, const uint64_t *off, size_t Q, uint64_t *first, uint8_t *bytes, size_t cap,
                           size_t *nbytes, uint64_t *copies) {
    const size_t S = s->shards.size();
    for (rsbwt_t *h : s->shards)
        if (h->view.n == 0) return fail(RSBWT_EINVAL, "empty index in the set");
    uint64_t steps = 0;
    if (s->groups.size() == 1 && S <= 1024) {
        const int rc = meta_read_device(s, text, off, Q, first, bytes, bytes ? cap : 0, copies, &steps);
        if (rc) return rc;
    } else {
        // several device groups: the ordinals come to the host and go the way rsbwt_set_meta_by_ordinal's go
        std::vector<uint64_t> od(S * Q), cp_own(copies ? 0 : S * Q);
        uint64_t *cp = copies ? copies : cp_own.data();
        std::atomic<uint64_t> st{0};
        int rc = rsbwt_set_read_copies_var_body(s, text, off, Q, cp, nullptr, od.data(), &st);
        if (rc) return rc;
        steps = st.load();
        std::vector<uint32_t> sh(Q * S);
        std::vector<uint64_t> it(Q * S);
        for (size_t q = 0; q < Q; ++q)
            for (size_t p = 0; p < S; ++p) {
                sh[q * S + p] = (uint32_t)p;
                it[q * S + p] = cp[p * Q + q] ? od[p * Q + q] : ~0ull;
            }
        size_t nb = 0;
        rc = set_meta_by_ordinal_body(s, sh.data(), it.data(), Q * S, first, bytes, cap, &nb);
        if (rc && rc != RSBWT_ERANGE) return rc;
    }
    const size_t n = Q * S;
    *nbytes = (size_t)first[n];
    meta_last_work[0] = n;
    meta_last_work[1] = 0;
    for (size_t i = 0; i < n; ++i) meta_last_work[1] += first[i + 1] != first[i];
    meta_last_work[2] = 0;
    meta_last_work[3] = steps;
    if (first[n] > (bytes ? cap : 0)) return fail(RSBWT_ERANGE, "%llu value bytes, room for %zu", (unsigned long long)first[n], bytes ? cap : 0);
    meta_last_work[2] = first[n];
    return RSBWT_OK;
}

// ---- sample counts (sample_counts.hip): the located rows of a batch reduced to per-query sample matrices ----
// the calling thread's last call: candidate rows, rows on a head ordinal, distinct carriers, records added, records with an
// unknown code, LF steps of the rows' walks (counting mode only)
thread_local uint64_t sample_last_work[6] = {0, 0, 0, 0, 0, 0};

// (read at every call: a test turns it on and off inside one process)
bool sample_tight_set() {
    const char *e = getenv("RSBWT_SAMPLE_TIGHT_SET");
    return e && e[0] == '1' && e[1] == 0;
}

inline size_t sample_tally_scratch(uint32_t S, uint64_t cap) {
    return al256((size_t)S * 8) + al256((size_t)S * 16) + al256(TALLY_WORK_COUNTERS * TALLY_WORK_STRIDE * 8) + al256((size_t)(4 * cap + S) * 8);
}

// What follows the walks, enqueued on st and nothing else: the matrices and carriers[] zeroed, the set's regions sized from
// the rows each shard has, the tally, and status8 (launch_sample_status).  d_scratch: sample_tally_scratch(S, cap) bytes.
int sample_tally_enqueue(dev_group *g, hipStream_t st, uint8_t *d_scratch, const void *d_first, size_t Q, const void *d_sh, const void *d_od,
                         uint64_t cap, const void *d_keys, const sample_dict &d, bool tight, const void *d_locate_work2, void *d_strings,
                         void *d_copies, void *d_carriers, void *d_status8) {
    const uint32_t S = (uint32_t)g->idx.size();
    const size_t cells = Q * ((size_t)d.C + 1), work_bytes = TALLY_WORK_COUNTERS * TALLY_WORK_STRIDE * 8, slots = (size_t)(4 * cap + S);
    uint8_t *d_rows_of = d_scratch, *d_region = d_rows_of + al256((size_t)S * 8), *d_work = d_region + al256((size_t)S * 16),
            *d_set = d_work + al256(work_bytes);
    if (d_strings) HIP_OK(hipMemsetAsync(d_strings, 0, cells * 4, st));
    if (d_copies) HIP_OK(hipMemsetAsync(d_copies, 0, cells * 8, st));
    if (d_carriers) HIP_OK(hipMemsetAsync(d_carriers, 0, Q * 8, st));
    HIP_OK(hipMemsetAsync(d_rows_of, 0, (size_t)S * 8, st));
    HIP_OK(hipMemsetAsync(d_work, 0, work_bytes, st));
    HIP_OK(hipMemsetAsync(d_set, 0xFF, slots * 8, st));
    hipError_t e = launch_sample_regions(d_sh, d_first, Q, cap, S, tight, d_rows_of, d_region, st);
    if (e != hipSuccess) return fail_hip(e, "region kernel launches");
    sample_tally a;
    a.meta = g->d_meta;
    a.S = S;
    a.first = (const uint64_t *)d_first;
    a.Q = Q;
    a.shard = (const uint32_t *)d_sh;
    a.ordinal = (const uint64_t *)d_od;
    a.total = cap;
    a.set = (unsigned long long *)d_set;
    a.region = (const uint64_t *)d_region;
    a.keys = (const uint64_t *)d_keys;
    a.C = d.C;
    a.size_of_sample = d.size_of_sample;
    a.has_other = d.has_other;
    a.keys_in_lds = 0;
    a.strings = (uint32_t *)d_strings;
    a.copies = (long long *)d_copies;
    a.carriers = (unsigned long long *)d_carriers;
    a.work = (unsigned long long *)d_work;
    if ((e = launch_sample_tally(a, st)) != hipSuccess) return fail_hip(e, "tally kernel launch");
    if ((e = launch_sample_status(d_first, Q, d_work, d_locate_work2, d_status8, st)) != hipSuccess) return fail_hip(e, "status kernel launch");
    return RSBWT_OK;
}

// One device group's `total` rows of mq queries -> that group's matrices in host memory (each optional), on gc's stream and
// in gc.lb.  The rows' first[] is d_first_in in HBM, or h_first to upload; fill(d_sh, d_rows) enqueues what makes the rows.
// Once that is enqueued nothing of gc.la is read again (first[] has been copied), and the lease goes back: a call then
// holds one lease plus a launch's own short one, so eight calls at once stay inside the cache's 16 slots.
// work6 += the group's counters (work6[0], the rows, is the caller's).
template <class Fill>
int sample_group_counts(dev_group *g, group_call &gc, size_t mq, const void *d_first_in, const uint64_t *h_first, uint64_t total,
                        const sample_dict &d, bool tight, uint32_t max_steps, Fill &&fill, uint32_t *strings, int64_t *copies, uint64_t *carriers,
                        uint64_t *work6) {
    hipStream_t st = gc.st;
    const uint32_t S = (uint32_t)g->idx.size();
    const size_t cells = mq * ((size_t)d.C + 1);
    const size_t a8 = al256(total * 8), a4 = al256(total * 4), a_first = al256((mq + 1) * 8), a_keys = al256((size_t)d.C * 8),
                 a_str = strings ? al256(cells * 4) : 0, a_cp = copies ? al256(cells * 8) : 0, a_car = al256(mq * 8);
    hipError_t e = g->scratch.take(2 * a8 + a4 + a_first + a_keys + a_str + a_cp + a_car + 512 + sample_tally_scratch(S, total), st, &gc.lb);
    if (e != hipSuccess)
        return fail(RSBWT_ENOMEM, "%llu rows and %zu matrix cells do not fit the device's free memory: %s", (unsigned long long)total, cells,
                    hipGetErrorString(e));
    uint8_t *d_rows = (uint8_t *)gc.lb.p, *d_od = d_rows + a8, *d_sh = d_od + a8, *d_first = d_sh + a4, *d_keys = d_first + a_first,
            *d_str = d_keys + a_keys, *d_cp = d_str + a_str, *d_car = d_cp + a_cp, *d_wk = d_car + a_car, *d_status = d_wk + 256,
            *d_scratch = d_status + 256;
    if (d_first_in) HIP_OK(hipMemcpyAsync(d_first, d_first_in, (mq + 1) * 8, hipMemcpyDeviceToDevice, st));
    else HIP_OK(hipMemcpyAsync(d_first, h_first, (mq + 1) * 8, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(d_keys, d.keys.data(), (size_t)d.C * 8, hipMemcpyHostToDevice, st));
    int rc = fill(d_sh, d_rows);
    if (rc) return rc;
    if (gc.la.slot >= 0) {
        g->scratch.give(gc.la, st);
        gc.la = scratch_cache::lease();
    }
    HIP_OK(hipMemsetAsync(d_wk, 0, 16, st));
    e = launch_locate(g->scratch, g->d_views, S, d_sh, d_rows, (size_t)total, max_steps, nullptr, d_od, nullptr, (unsigned long long *)d_wk,
                      g->num_cus, st);
    if (e != hipSuccess) return fail_hip(e, "locate kernel launch");
    rc = sample_tally_enqueue(g, st, d_scratch, d_first, mq, d_sh, d_od, total, d_keys, d, tight, d_wk, strings ? d_str : nullptr,
                              copies ? d_cp : nullptr, d_car, d_status);
    if (rc) return rc;
    uint64_t status[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (strings) HIP_OK(hipMemcpyAsync(strings, d_str, cells * 4, hipMemcpyDeviceToHost, st));
    if (copies) HIP_OK(hipMemcpyAsync(copies, d_cp, cells * 8, hipMemcpyDeviceToHost, st));
    if (carriers) HIP_OK(hipMemcpyAsync(carriers, d_car, mq * 8, hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(status, d_status, sizeof status, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    if (status[6] != 0)
        return fail(RSBWT_EINVAL, "%llu rows whose walk to their read's start does not end within max_steps (a corrupt index, or a read longer than the limit)",
                    (unsigned long long)status[6]);
    for (int i = 1; i <= 4; ++i) work6[i] += status[i];
    if (g->counting) work6[5] += status[5];
    return RSBWT_OK;
}

void sample_zero(size_t mq, size_t C, uint32_t *strings, int64_t *copies, uint64_t *carriers) {
    const size_t cells = mq * (C + 1);
    if (strings) memset(strings, 0, cells * 4);
    if (copies) memset(copies, 0, cells * 8);
    if (carriers) memset(carriers, 0, mq * 8);
}

// a slice of mq queries on a set of ONE device group: nothing but first[], matches[] and the answers leaves the device
int sample_counts_device(rsbwt_set_t *s, const char *text, const uint64_t *off, size_t mq, const sample_dict &d, bool tight, uint64_t max_rows,
                         uint32_t max_steps, uint32_t *strings, int64_t *copies, uint64_t *matches, uint64_t *carriers, uint64_t *work6) {
    capped_intervals ci;  // (before gc: a copy into it may still be in flight when gc waits for the stream)
    std::vector<uint64_t> first(mq + 1);
    group_call gc(s->groups[0], true);
    if (gc.rc) return gc.rc;
    dev_group *g = gc.g;
    const uint32_t S = (uint32_t)g->idx.size();
    int rc = capped_intervals_device(s, gc, text, off, mq, max_rows, 0, mq + 1, "scratch for sample counts", first.data(), matches, &ci);
    if (rc) return rc;
    const uint64_t total = ci.total;
    work6[0] += total;
    if (total == 0) {
        sample_zero(mq, d.C, strings, copies, carriers);
        return RSBWT_OK;
    }
    if (total >= (1ull << 38)) return fail(RSBWT_ERANGE, "%llu rows in one slice: at most 2^38 (set max_rows)", (unsigned long long)total);
    return sample_group_counts(
        g, gc, mq, ci.d_first, nullptr, total, d, tight, max_steps,
        [&](uint8_t *d_sh, uint8_t *d_rows) -> int {
            const hipError_t e = launch_interval_fill(g->d_views, S, ci.d_pairs, mq, ci.d_first, (size_t)total, d_sh, d_rows, nullptr, nullptr, nullptr, gc.st);
            return e == hipSuccess ? RSBWT_OK : fail_hip(e, "row expansion");
        },
        strings, copies, carriers, work6);
}

// the same over several device groups: the intervals come to the host, the limit and the expansion run there
// (intervals_to_rows_host); every group locates and tallies its shards' rows into matrices of its own, and the host adds them
int sample_counts_groups(rsbwt_set_t *s, const char *text, const uint64_t *off, size_t mq, const sample_dict &d, bool tight, uint64_t max_rows,
                         uint32_t max_steps, uint32_t *strings, int64_t *copies, uint64_t *matches, uint64_t *carriers, uint64_t *work6) {
    const size_t S = s->shards.size(), G = s->groups.size(), cells = mq * ((size_t)d.C + 1);
    std::vector<uint64_t> lo(S * mq), up(S * mq), first(mq + 1);
    int rc = rsbwt_set_find_intervals_var_body(s, text, off, mq, lo.data(), up.data(), false);
    if (rc) return rc;
    const expanded_rows hr = intervals_to_rows_host(s, mq, lo, up, max_rows, ~(size_t)0, first.data(), matches);
    work6[0] += hr.total;
    sample_zero(mq, d.C, strings, copies, carriers);
    if (hr.total == 0) return RSBWT_OK;
    std::vector<uint32_t> group_of(S, 0), local(S, 0);
    for (size_t gi = 0; gi < G; ++gi)
        for (size_t j = 0; j < s->groups[gi]->idx.size(); ++j) {
            group_of[s->groups[gi]->idx[j]] = (uint32_t)gi;
            local[s->groups[gi]->idx[j]] = (uint32_t)j;
        }
    struct share_t {
        std::vector<uint64_t> first, rows, carriers;
        std::vector<uint32_t> shard, strings;
        std::vector<int64_t> copies;
        uint64_t work[6] = {0, 0, 0, 0, 0, 0};
    };
    std::vector<share_t> sh(G);
    for (share_t &x : sh) x.first.assign(mq + 1, 0);
    for (size_t q = 0; q < mq; ++q) {
        for (size_t gi = 0; gi < G; ++gi) sh[gi].first[q] = sh[gi].rows.size();
        for (uint64_t t = first[q]; t < first[q + 1]; ++t) {
            share_t &x = sh[group_of[hr.shard_of[t]]];
            x.shard.push_back(local[hr.shard_of[t]]);
            x.rows.push_back(hr.rows[t]);
        }
    }
    for (size_t gi = 0; gi < G; ++gi) sh[gi].first[mq] = sh[gi].rows.size();
    rc = for_each_group(s, [&](size_t gi) -> int {
        share_t &x = sh[gi];
        const size_t m = x.rows.size();
        if (m == 0) return RSBWT_OK;
        if (strings) x.strings.resize(cells);
        if (copies) x.copies.resize(cells);
        x.carriers.resize(mq);
        group_call gc(s->groups[gi], true);
        if (gc.rc) return gc.rc;
        return sample_group_counts(
            gc.g, gc, mq, nullptr, x.first.data(), m, d, tight, max_steps,
            [&](uint8_t *d_sh, uint8_t *d_rows) -> int {
                HIP_OK(hipMemcpyAsync(d_sh, x.shard.data(), m * 4, hipMemcpyHostToDevice, gc.st));
                HIP_OK(hipMemcpyAsync(d_rows, x.rows.data(), m * 8, hipMemcpyHostToDevice, gc.st));
                return RSBWT_OK;
            },
            strings ? x.strings.data() : nullptr, copies ? x.copies.data() : nullptr, x.carriers.data(), x.work);
    });
    if (rc) return rc;
    for (const share_t &x : sh) {
        if (x.rows.empty()) continue;
        for (size_t i = 0; i < cells; ++i) {
            if (strings) strings[i] += x.strings[i];
            if (copies) copies[i] += x.copies[i];
        }
        if (carriers)
            for (size_t q = 0; q < mq; ++q) carriers[q] += x.carriers[q];
        for (int i = 1; i < 6; ++i) work6[i] += x.work[i];
    }
    return RSBWT_OK;
}

int set_sample_counts_body(rsbwt_set_t *s, const char *text, const uint64_t *off, size_t Q, const uint8_t *codes, size_t C, uint32_t size_of_sample,
                           int has_other, uint64_t max_rows, uint32_t max_steps, uint32_t *strings, int64_t *copies, uint64_t *matches,
                           uint64_t *carriers) {
    int rc = sample_set_ok(s);
    if (rc) return rc;
    sample_dict d;
    if ((rc = sample_dict_make(codes, C, size_of_sample, has_other, &d)) != RSBWT_OK) return rc;
    if (!strings && !copies && !matches && !carriers) return fail(RSBWT_EINVAL, "null argument: no output array");
    if (Q == 0) return RSBWT_OK;
    if (!off || (!text && off[Q] != off[0])) return fail(RSBWT_EINVAL, "null argument");
    // slices: a query number of the set's keys has 24 bits, and a slice's matrices (12 bytes a cell) stay under 1.5 GiB of HBM
    const size_t width = C + 1, SLICE = std::min<size_t>((size_t)1 << 24, std::max<size_t>(1, ((size_t)1 << 27) / width));
    const bool tight = sample_tight_set(), on_device = s->groups.size() == 1 && s->shards.size() <= 1024;
    for (size_t q0 = 0; q0 < Q; q0 += SLICE) {
        const size_t mq = std::min(SLICE, Q - q0);
        uint32_t *st = strings ? strings + q0 * width : nullptr;
        int64_t *cp = copies ? copies + q0 * width : nullptr;
        uint64_t *mt = matches ? matches + q0 : nullptr, *ca = carriers ? carriers + q0 : nullptr;
        rc = on_device ? sample_counts_device(s, text, off + q0, mq, d, tight, max_rows, max_steps, st, cp, mt, ca, sample_last_work)
                       : sample_counts_groups(s, text, off + q0, mq, d, tight, max_rows, max_steps, st, cp, mt, ca, sample_last_work);
        if (rc) return rc;
    }
    return RSBWT_OK;
}

// ---- site sample counts (site_counts.hip): SiteMatch's kept reads reduced to per-request sample matrices ----
// the calling thread's last call: legs, LF steps spent lengthening, candidate rows, rows the span filter kept, of those rows
// on a head ordinal, distinct reads extracted, (request, read) items aligned, items kept, records added, records with an
// unknown code
thread_local uint64_t site_last_work[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};

// ... and, while RSBWT_SITE_TIMES=1, the device time of its stages in ms, from events around each stage's launches on the
// call's stream, summed over the device groups and slices: {narrowing + rows + walks + filter, head test + set + compaction,
// sort / unique + extraction, length rule + ordering, alignment, tally}
thread_local double site_last_ms[6] = {0, 0, 0, 0, 0, 0};

struct site_marks {
    bool on = false;
    hipStream_t st = nullptr;
    hipEvent_t ev[12] = {};
    bool open_[6] = {};
    double ms[6] = {0, 0, 0, 0, 0, 0};
    site_marks(hipStream_t stream) : st(stream) {
        const char *e = getenv("RSBWT_SITE_TIMES");
        on = e && e[0] == '1' && e[1] == 0;
    }
    site_marks(const site_marks &) = delete;
    void begin(int stage) {
        if (!on || open_[stage]) return;
        if (!ev[2 * stage] && (hipEventCreate(&ev[2 * stage]) != hipSuccess || hipEventCreate(&ev[2 * stage + 1]) != hipSuccess)) {
            on = false;
            return;
        }
        open_[stage] = hipEventRecord(ev[2 * stage], st) == hipSuccess;
    }
    void end(int stage) {  // (a stage enqueued twice -- the second extraction's round -- adds up)
        if (!on || !open_[stage]) return;
        open_[stage] = false;
        if (hipEventRecord(ev[2 * stage + 1], st) != hipSuccess || hipEventSynchronize(ev[2 * stage + 1]) != hipSuccess) return;
        float t = 0;
        if (hipEventElapsedTime(&t, ev[2 * stage], ev[2 * stage + 1]) == hipSuccess) ms[stage] += t;
    }
    ~site_marks() {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};

constexpr uint32_t SITE_STRIDE = 256;          // the first extraction's stride
constexpr uint32_t SITE_WIDE_STRIDE = 4096 + 64;  // the second's: a read of RSBWT_KSW_MAX_LEN symbols and padding

struct site_requests {  // a slice's requests beside the plan
    std::vector<uint64_t> off;  // [mq + 1], off[0] = 0
    const char *alt = nullptr;
    const uint8_t *isalt = nullptr;
    uint32_t lo_w = 1, hi_w = 1;  // the shortest (at least 1) and the longest window
};

struct site_group_out {
    std::vector<uint32_t> strings;
    std::vector<int64_t> copies;
    std::vector<uint64_t> aligned, carriers;
    uint64_t work[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    double ms[6] = {0, 0, 0, 0, 0, 0};
};

// rsbwt_set_site_reads' share of a group's run (site_reads.hip): what the group answers instead of the matrices.  work[] is
// then {legs, lengthening steps, candidate rows, rows kept, distinct reads, string classes, items aligned, items kept,
// reads reported}.
struct site_reads_out {
    bool want_bytes = false;  // false: first[] alone (the count call)
    uint32_t stride = 0;
    // where the reads go when the group's order is the caller's (one group: the copy from the device lands there); else null
    char *reads = nullptr;
    uint32_t *len = nullptr;
    uint64_t *row = nullptr;
    size_t cap = 0;  // the reads there is room for: a group with more gathers nothing
    bool stored = false;
    uint64_t nout = 0;
    std::vector<uint64_t> first;  // [Q * S_g + 1]
    std::vector<char> bytes_v;    // (several groups: the group's reads in its own order)
    std::vector<uint32_t> len_v;
    std::vector<uint64_t> row_v;
};

// a lease beyond a group_call's two: goes back when the call leaves, after the stream has drained
struct site_lease {
    dev_group *g;
    hipStream_t st;
    scratch_cache::lease l;
    site_lease(dev_group *grp, hipStream_t stream) : g(grp), st(stream) {}
    site_lease(const site_lease &) = delete;
    void drop() {  // (the launches that used it are enqueued: give() asks no more)
        if (l.slot >= 0) g->scratch.give(l, st);
        l = scratch_cache::lease();
    }
    ~site_lease() {
        if (l.slot < 0) return;
        (void)hipStreamSynchronize(st);
        g->scratch.give(l, st);
    }
};

// The tail of a run that answers rsbwt_set_site_reads (site_reads.hip), after the alignment: the answer laid out where it
// is.  The sort's buffers and the layout's scratch are gc.lb's, free since the distinct reads were made; the reported
// reads' numbers and rows take the alignment's order and request arrays, which the alignment read for the last time.
struct site_tail_args {
    uint8_t *d_items, *d_verdict, *d_cflag, *d_cfirst, *d_drows, *d_seg, *d_sort_key, *d_sort_idx, *d_reads_tmp, *d_pkey, *d_req, *d_gfirst, *d_sizes,
        *d_raddr, *d_rlen;
    size_t reads_tmp, Q, R;
    uint64_t n;
    uint32_t S;
    unsigned long long *work;
};
int site_reads_tail(dev_group *g, group_call &gc, const site_tail_args &a, site_reads_out *rd, uint64_t *classes) {
    hipStream_t st = gc.st;
    hipError_t e;
    e = launch_site_layout(a.d_items, (size_t)a.n, a.Q, a.S, a.d_verdict, a.d_cflag, a.d_cfirst, a.d_drows, a.d_seg, a.d_sort_key, a.d_sort_idx,
                           a.d_reads_tmp, a.reads_tmp, a.d_pkey, a.d_req, a.d_gfirst, a.d_sizes + 16, a.work, st);
    if (e != hipSuccess) return fail_hip(e, "answer layout kernel launches");
    uint64_t nout = 0;
    HIP_OK(hipMemcpyAsync(&nout, a.d_sizes + 16, 8, hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(classes, a.d_cfirst + a.R * 8, 8, hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(rd->first.data(), a.d_gfirst, rd->first.size() * 8, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    if (nout > a.n || *classes == 0 || *classes > a.R)
        return fail(RSBWT_EHIP, "%llu reads reported of %llu items, %llu classes of %zu reads", (unsigned long long)nout, (unsigned long long)a.n,
                    (unsigned long long)*classes, a.R);
    rd->nout = nout;
    if (rd->want_bytes && nout != 0 && nout <= rd->cap) {
        // the rows, the set and the items are done with: their lease goes back and the reads' slots take its place
        g->scratch.give(gc.lb, st);
        gc.lb = scratch_cache::lease();
        const size_t a_out = al256((size_t)nout * rd->stride);
        e = g->scratch.take(a_out + al256((size_t)nout * 4), st, &gc.lb);
        if (e != hipSuccess)
            return fail(RSBWT_ENOMEM, "%llu reads at stride %u do not fit the device's free memory: %s", (unsigned long long)nout, rd->stride,
                        hipGetErrorString(e));
        uint8_t *d_out = (uint8_t *)gc.lb.p, *d_olen = d_out + a_out;
        if ((e = launch_site_gather(a.d_pkey, (size_t)nout, a.d_raddr, a.d_rlen, d_out, rd->stride, d_olen, st)) != hipSuccess)
            return fail_hip(e, "read gather kernel launch");
        char *hb = rd->reads;
        uint32_t *hl = rd->len;
        uint64_t *hr = rd->row;
        if (!hb) {
            rd->bytes_v.resize((size_t)nout * rd->stride);
            rd->len_v.resize((size_t)nout);
            rd->row_v.resize((size_t)nout);
            hb = rd->bytes_v.data();
            hl = rd->len_v.data();
            hr = rd->row_v.data();
        }
        HIP_OK(hipMemcpyAsync(hb, d_out, (size_t)nout * rd->stride, hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(hl, d_olen, (size_t)nout * 4, hipMemcpyDeviceToHost, st));
        if (hr) HIP_OK(hipMemcpyAsync(hr, a.d_req, (size_t)nout * 8, hipMemcpyDeviceToHost, st));
        rd->stored = true;
    }
    return RSBWT_OK;
}

// One device group's share of a slice (site_counts.hip has the stages).  The host reads back, eight bytes each: the row
// total, the kept rows / rows not located / items, the distinct reads, the reads over the first stride and the longest that
// fit; then the matrices, the two count vectors and the counters.  Three leases at most are held at a time (gc.la: the
// batch; gc.lb: rows, set and items; lc: reads and what the alignment and the tally need) plus a launch's own short one,
// so four calls at once stay inside the cache's 16 slots.
// rd: the run answers rsbwt_set_site_reads instead (site_reads.hip): no head test, no dictionary, no tally; after the
// alignment the answer is laid out on the device and the host reads back two more sizes (string classes, reads reported),
// the group's first[] and the reported reads' slots, lengths and rows, which take gc.lb's place once its rows are done with.
int site_group_run(rsbwt_set_t *s, dev_group *g, const gt_plan &pl, const char *t0, const site_requests &rq, const sample_dict &d, bool tight,
                   uint32_t row_bits, bool want_strings, bool want_copies, site_group_out *out, site_reads_out *rd = nullptr) {
    group_call gc(g, true);
    if (gc.rc) return gc.rc;
    hipStream_t st = gc.st;
    site_lease lc(g, st);
    site_marks tm(st);
    tm.begin(0);
    const uint32_t S = (uint32_t)g->idx.size();
    const size_t Q = pl.q_off.size(), N = pl.nitems, cells = (size_t)S * N, mcells = Q * ((size_t)d.C + 1);
    const size_t work_bytes = SITE_WORK_COUNTERS * TALLY_WORK_STRIDE * 8;
    const size_t a_off = al256((Q + 1) * 8), a_q1 = al256(Q), a_keys = al256((size_t)d.C * 8), a_work = al256(work_bytes);
    gt_front f;
    int rc = gt_front_enqueue(g, gc, pl, t0, a_off + 2 * a_q1 + a_keys + a_work + 256, &f);
    if (rc) return rc;
    uint8_t *d_off = f.d_extra, *d_alt = d_off + a_off, *d_isalt = d_alt + a_q1, *d_keys = d_isalt + a_q1, *d_work = d_keys + a_keys,
            *d_sizes = d_work + a_work;  // d_sizes: [0] distinct reads, [1] the longest read that fit
    unsigned long long *work = (unsigned long long *)d_work, *wk = (unsigned long long *)f.d_wk;
    HIP_OK(hipMemcpyAsync(d_off, rq.off.data(), (Q + 1) * 8, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(d_alt, rq.alt, Q, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(d_isalt, rq.isalt, Q, hipMemcpyHostToDevice, st));
    if (d.C) HIP_OK(hipMemcpyAsync(d_keys, d.keys.data(), (size_t)d.C * 8, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemsetAsync(d_work, 0, work_bytes + 256, st));
    hipError_t e = launch_site_legs(f.d_legs, cells, work, st);
    if (e == hipSuccess) e = launch_interval_totals(g->d_views, S, f.d_pairs, N, 0, f.d_matches, f.d_keptq, f.d_first, f.d_over, f.d_tmp, f.tmp_bytes, st);
    if (e != hipSuccess) return fail_hip(e, "leg count and interval-rows kernels");
    uint64_t total = 0;
    HIP_OK(hipMemcpyAsync(&total, f.d_first + N * 8, 8, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    if (want_strings) out->strings.assign(mcells, 0);
    if (want_copies) out->copies.assign(mcells, 0);
    out->aligned.assign(Q, 0);
    out->carriers.assign(Q, 0);
    std::vector<unsigned long long> hwork(SITE_WORK_COUNTERS * TALLY_WORK_STRIDE, 0);
    unsigned long long hwk[3] = {0, 0, 0};
    uint64_t nreads = 0, classes = 0;
    if (rd) rd->first.assign(Q * (size_t)S + 1, 0);
    auto finish = [&]() -> int {  // the counters, once everything is enqueued
        HIP_OK(hipMemcpyAsync(hwork.data(), d_work, work_bytes, hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(hwk, f.d_wk, sizeof hwk, hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        auto w = [&](int which) { return (uint64_t)hwork[(size_t)which * TALLY_WORK_STRIDE]; };
        if (w(SITE_WORK_TOO_LONG) != 0)
            return fail(RSBWT_EINVAL, "%llu candidate reads longer than %d symbols", (unsigned long long)w(SITE_WORK_TOO_LONG), RSBWT_KSW_MAX_LEN);
        const uint64_t mine[10] = {w(SITE_WORK_LEGS), hwk[0], total, hwk[1], w(SITE_WORK_HEADS), nreads, w(SITE_WORK_ALIGNED), w(SITE_WORK_KEPT),
                                   w(SITE_WORK_RECORDS), w(SITE_WORK_UNKNOWN)};
        for (int i = 0; i < 10; ++i) out->work[i] = mine[i];
        if (rd) {
            const uint64_t reads9[10] = {w(SITE_WORK_LEGS), hwk[0], total, hwk[1], nreads, classes, w(SITE_WORK_ALIGNED), w(SITE_WORK_KEPT), rd->nout, 0};
            for (int i = 0; i < 10; ++i) out->work[i] = reads9[i];
        }
        for (int i = 0; i < 6; ++i) {
            tm.end(i);
            out->ms[i] = tm.ms[i];
        }
        return RSBWT_OK;
    };
    if (total == 0) return finish();
    if (total >= (1ull << 31)) return fail(RSBWT_ERANGE, "%llu candidate rows in one call: at most 2^31", (unsigned long long)total);
    // ---- stage 1 (rows, walks, filter) and stages 2, 3a in gc.lb
    const uint64_t nslots = 4 * total + S;
    const size_t a8 = al256(total * 8), a4 = al256(total * 4), a_rec = al256(total * sizeof(gt_site_row)), a_s8 = al256((size_t)(S + 1) * 8),
                 a_region = al256((size_t)S * 16), a_set8 = al256(nslots * 8), a_set4 = al256(nslots * 4), a_items = al256(total * sizeof(site_item)),
                 reads_tmp = std::max(site_reads_tmp_bytes(total), rd ? site_layout_tmp_bytes(total) : (size_t)0);
    e = g->scratch.take(5 * a8 + 3 * a4 + a_rec + 2 * a_s8 + a_region + 2 * a_set8 + a_set4 + a_items + reads_tmp, st, &gc.lb);
    if (e != hipSuccess)
        return fail(RSBWT_ENOMEM, "%llu candidate rows do not fit the device's free memory: %s", (unsigned long long)total, hipGetErrorString(e));
    uint8_t *d_rows = (uint8_t *)gc.lb.p, *d_rr = d_rows + a8, *d_od = d_rr + a8, *d_sh = d_od + a8, *d_of = d_sh + a4, *d_rec = d_of + a4,
            *d_rows_of = d_rec + a_rec, *d_seg = d_rows_of + a_s8, *d_region = d_seg + a_s8, *d_skeys = d_region + a_region, *d_srow = d_skeys + a_set8,
            *d_sneed = d_srow + a_set8, *d_items = d_sneed + a_set4, *d_sort_key = d_items + a_items, *d_sort_idx = d_sort_key + a8,
            *d_drows = d_sort_idx + a4, *d_reads_tmp = d_drows + a8;
    e = launch_interval_fill(g->d_views, S, f.d_pairs, N, f.d_first, (size_t)total, d_sh, d_rows, nullptr, nullptr, nullptr, st);
    if (e == hipSuccess) e = launch_locate(g->scratch, g->d_views, S, d_sh, d_rows, (size_t)total, 0, d_rr, d_od, d_of, nullptr, g->num_cus, st);
    if (e == hipSuccess) e = launch_gt_filter(f.bt, f.d_legs, f.d_first, d_sh, d_of, d_rr, total, d_rec, wk + 1, st, d_od);
    if (e != hipSuccess) return fail_hip(e, "row expansion, locate and filter kernel launches");
    tm.end(0);
    tm.begin(1);
    site_set set;
    set.keys = (unsigned long long *)d_skeys;
    set.row = (uint64_t *)d_srow;
    set.need = (uint32_t *)d_sneed;
    set.region = (uint64_t *)d_region;
    set.nslots = nslots;
    e = launch_site_rows(f.bt, f.d_legs, d_rec, wk + 1, total, rd ? nullptr : g->d_meta, rd == nullptr, S, tight, d_rows_of, set, work, st);
    if (e == hipSuccess) e = launch_site_compact(set, S, row_bits, d_items, d_sort_key, d_sort_idx, total, work, st);
    if (e != hipSuccess) return fail_hip(e, "head test and set kernel launches");
    tm.end(1);
    uint64_t n = 0;
    HIP_OK(hipMemcpyAsync(hwk, f.d_wk, sizeof hwk, hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(&n, work + (size_t)SITE_WORK_ITEMS * TALLY_WORK_STRIDE, 8, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    if (hwk[2] != 0)
        return fail(RSBWT_EINVAL, "%llu candidate rows whose walk to their read's start does not end (a corrupt index, or a read longer than 2^20 symbols)",
                    hwk[2]);
    if (hwk[1] > total || n > hwk[1]) return fail(RSBWT_EHIP, "the row filter kept %llu of %llu rows, %llu items", hwk[1], (unsigned long long)total, (unsigned long long)n);
    if (n == 0) return finish();
    // ---- stage 3b: the distinct reads
    tm.begin(2);
    e = launch_site_reads(d_items, (size_t)n, S, row_bits, d_sort_key, d_sort_idx, d_reads_tmp, reads_tmp, d_drows, d_seg, d_sizes, st);
    if (e != hipSuccess) return fail_hip(e, "sort and unique of the candidate reads");
    tm.end(2);
    HIP_OK(hipMemcpyAsync(&nreads, d_sizes, 8, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    const size_t R = (size_t)nreads;
    if (R == 0 || R > n) return fail(RSBWT_EHIP, "%zu distinct reads of %llu items", R, (unsigned long long)n);
    if ((rc = ensure_group_xviews(s, g, st)) != RSBWT_OK) return rc;
    // ---- the reads and everything behind them in lc; taken again with room for the second extraction if a read needs it
    const size_t scan_tmp = meta_scan_bytes(R + 1), perm_tmp = site_perm_tmp_bytes((size_t)n);
    const size_t a_r4 = al256(R * 4), a_r8 = al256((R + 1) * 8), a_n8 = al256((size_t)n * 8), a_n4 = al256((size_t)n * 4), a_n1 = al256((size_t)n),
                 a_q8 = al256(Q * 8), a_str = want_strings ? al256(mcells * 4) : 0, a_cp = want_copies ? al256(mcells * 8) : 0,
                 a_first = rd ? al256((Q * (size_t)S + 1) * 8) : 0, a_cls = rd ? 2 * a_r8 : 0;
    uint64_t n_over = 0, longest = 0;
    uint8_t *d_reads = nullptr, *d_plen = nullptr, *d_rlen = nullptr, *d_overf = nullptr, *d_ofirst = nullptr, *d_scan = nullptr, *d_raddr = nullptr,
            *d_req = nullptr, *d_rid = nullptr, *d_pkey = nullptr, *d_pidx = nullptr, *d_pkey2 = nullptr, *d_perm = nullptr, *d_ptmp = nullptr,
            *d_verdict = nullptr, *d_aligned = nullptr, *d_carriers = nullptr, *d_str = nullptr, *d_cp = nullptr, *d_ksw = nullptr, *d_wide = nullptr,
            *d_wplen = nullptr, *d_wlen = nullptr, *d_wrows = nullptr, *d_wseg = nullptr, *d_cflag = nullptr, *d_cfirst = nullptr, *d_gfirst = nullptr;
    size_t ksw_bytes = 0;
    for (int round = 0; round < 2; ++round) {
        const size_t W = (size_t)n_over;  // (0 in the first round)
        ksw_bytes = ksw_scratch_bytes(W ? (uint32_t)RSBWT_KSW_MAX_LEN : std::max<uint32_t>(SITE_STRIDE, rq.hi_w));
        const size_t a_reads = al256(R * (size_t)SITE_STRIDE), a_wide = al256(W * (size_t)SITE_WIDE_STRIDE), a_w4 = al256(W * 4), a_w8 = al256(W * 8);
        lc.drop();
        e = g->scratch.take(a_reads + 2 * a_r4 + 3 * a_r8 + al256(scan_tmp) + a_n8 + 5 * a_n4 + al256(perm_tmp) + a_n1 + 2 * a_q8 + a_str + a_cp +
                                al256(ksw_bytes) + a_wide + 2 * a_w4 + a_w8 + al256((size_t)(S + 1) * 8) + a_cls + a_first + 256,
                            st, &lc.l);
        if (e != hipSuccess)
            return fail(RSBWT_ENOMEM, "%zu reads, %llu items and %zu matrix cells do not fit the device's free memory: %s", R, (unsigned long long)n, mcells,
                        hipGetErrorString(e));
        d_reads = (uint8_t *)lc.l.p;
        d_plen = d_reads + a_reads;
        d_rlen = d_plen + a_r4;
        d_overf = d_rlen + a_r4;
        d_ofirst = d_overf + a_r8;
        d_raddr = d_ofirst + a_r8;
        d_scan = d_raddr + a_r8;
        d_req = d_scan + al256(scan_tmp);
        d_rid = d_req + a_n8;
        d_pkey = d_rid + a_n4;
        d_pidx = d_pkey + a_n4;
        d_pkey2 = d_pidx + a_n4;
        d_perm = d_pkey2 + a_n4;
        d_ptmp = d_perm + a_n4;
        d_verdict = d_ptmp + al256(perm_tmp);
        d_aligned = d_verdict + a_n1;
        d_carriers = d_aligned + a_q8;
        d_str = d_carriers + a_q8;
        d_cp = d_str + a_str;
        d_ksw = d_cp + a_cp;
        d_wide = d_ksw + al256(ksw_bytes);
        d_wplen = d_wide + a_wide;
        d_wlen = d_wplen + a_w4;
        d_wrows = d_wlen + a_w4;
        d_wseg = d_wrows + a_w8;
        d_cflag = d_wseg + al256((size_t)(S + 1) * 8);
        d_cfirst = d_cflag + a_r8;
        d_gfirst = d_cflag + a_cls;
        tm.begin(2);
        HIP_OK(hipMemsetAsync(d_sizes + 8, 0, 8, st));
        e = launch_extract_ragged(g->scratch, g->d_xviews, S, d_drows, R, d_seg, 1, d_reads, SITE_STRIDE, d_plen, d_rlen, g->num_cus, st);
        if (e == hipSuccess) e = launch_site_over(d_rlen, R, d_overf, d_ofirst, (unsigned long long *)(d_sizes + 8), d_scan, scan_tmp, st);
        if (e != hipSuccess) return fail_hip(e, "extraction of the candidate reads");
        tm.end(2);
        HIP_OK(hipMemcpyAsync(&n_over, d_ofirst + R * 8, 8, hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(&longest, d_sizes + 8, 8, hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        if (n_over > R) return fail(RSBWT_EHIP, "%llu of %zu reads over the stride", (unsigned long long)n_over, R);
        if (n_over == W) break;  // (none, or the room is there now)
        if (round == 1) return fail(RSBWT_EHIP, "the second extraction of the same rows counts other lengths");
    }
    tm.begin(2);
    if (n_over != 0) {
        e = launch_site_wide(d_drows, d_seg, S, R, d_overf, d_ofirst, d_wrows, d_wseg, st);
        if (e == hipSuccess)
            e = launch_extract_ragged(g->scratch, g->d_xviews, S, d_wrows, (size_t)n_over, d_wseg, 1, d_wide, SITE_WIDE_STRIDE, d_wplen, d_wlen, g->num_cus, st);
        if (e != hipSuccess) return fail_hip(e, "second extraction of the long candidate reads");
    }
    e = launch_site_addr(d_reads, SITE_STRIDE, n_over ? d_wide : nullptr, SITE_WIDE_STRIDE, d_overf, d_ofirst, d_wlen, R, d_raddr, d_rlen, st);
    if (e != hipSuccess) return fail_hip(e, "read address kernel launch");
    if (rd && (e = launch_site_classes(d_raddr, d_rlen, d_seg, S, R, d_cflag, d_cfirst, d_scan, scan_tmp, st)) != hipSuccess)
        return fail_hip(e, "string class kernel launch");
    tm.end(2);
    tm.begin(3);
    // ---- stage 4: the length rule, the alignment's batch and its order
    HIP_OK(hipMemsetAsync(d_aligned, 0, 2 * a_q8 + a_str + a_cp, st));  // (aligned, carriers and the matrices lie back to back)
    HIP_OK(hipMemsetAsync(d_verdict, 0, (size_t)n, st));                 // (0 is no verdict: nothing is kept that the alignment did not answer)
    e = launch_site_items(d_items, (size_t)n, d_rlen, d_off, Q, d_req, d_rid, d_pkey, d_pidx, (unsigned long long *)d_aligned, work, st);
    if (e == hipSuccess) e = launch_site_perm(d_pkey, d_pidx, (size_t)n, d_pkey2, d_perm, d_ptmp, perm_tmp, st);
    if (e != hipSuccess) return fail_hip(e, "length rule and ordering kernel launches");
    tm.end(3);
    tm.begin(4);
    gt_align_batch ab;
    ab.reads = nullptr;
    ab.text = f.bt.text;
    ab.alt = (const char *)d_alt;
    ab.roff = nullptr;
    ab.item = (const uint64_t *)d_req;
    ab.off = (const uint64_t *)d_off;
    ab.pos = f.bt.q_pos;
    ab.isalt = d_isalt;
    ab.n = (size_t)n;
    ab.Q = Q;
    ab.perm = (const uint32_t *)d_perm;
    ab.rid = (const uint32_t *)d_rid;
    ab.raddr = (const uint64_t *)d_raddr;
    ab.rlen = (const uint32_t *)d_rlen;
    const uint32_t hi_rows = n_over ? (uint32_t)RSBWT_KSW_MAX_LEN : std::max<uint32_t>((uint32_t)longest, rq.hi_w);
    e = launch_gt_align(ab, std::min(rq.lo_w, hi_rows), hi_rows, ksw_scratch_bytes(hi_rows) ? d_ksw : nullptr, d_verdict, nullptr, st);
    if (e != hipSuccess) return fail_hip(e, "gt alignment kernel launch");
    tm.end(4);
    tm.begin(5);
    if (rd) {
        const site_tail_args ta = {d_items,  d_verdict, d_cflag, d_cfirst, d_drows, d_seg,     d_sort_key, d_sort_idx, d_reads_tmp, d_pkey, d_req,
                                   d_gfirst, d_sizes,   d_raddr, d_rlen,   reads_tmp, Q,       R,          n,          S,           work};
        if ((rc = site_reads_tail(g, gc, ta, rd, &classes)) != RSBWT_OK) return rc;
        return finish();
    }
    // ---- stage 5: the kept reads' records
    site_tally ta;
    ta.items = (const site_item *)d_items;
    ta.n = (size_t)n;
    ta.req = (const uint64_t *)d_req;
    ta.verdict = d_verdict;
    ta.meta = g->d_meta;
    ta.S = S;
    ta.keys = (const uint64_t *)d_keys;
    ta.C = d.C;
    ta.size_of_sample = d.size_of_sample;
    ta.has_other = d.has_other;
    ta.strings = want_strings ? (uint32_t *)d_str : nullptr;
    ta.copies = want_copies ? (long long *)d_cp : nullptr;
    ta.carriers = (unsigned long long *)d_carriers;
    ta.work = work;
    if ((e = launch_site_tally(ta, st)) != hipSuccess) return fail_hip(e, "site tally kernel launch");
    tm.end(5);
    if (want_strings) HIP_OK(hipMemcpyAsync(out->strings.data(), d_str, mcells * 4, hipMemcpyDeviceToHost, st));
    if (want_copies) HIP_OK(hipMemcpyAsync(out->copies.data(), d_cp, mcells * 8, hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(out->aligned.data(), d_aligned, Q * 8, hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(out->carriers.data(), d_carriers, Q * 8, hipMemcpyDeviceToHost, st));
    return finish();
}

int set_site_counts_body(rsbwt_set_t *s, const char *text, const uint64_t *off, size_t Q, const uint64_t *pos, const char *alt, const uint8_t *isalt,
                         int32_t k, int32_t skip, uint64_t M, const uint8_t *codes, size_t C, uint32_t size_of_sample, int has_other, uint32_t *strings,
                         int64_t *copies, uint64_t *aligned, uint64_t *carriers) {
    for (uint64_t &w : site_last_work) w = 0;
    for (double &t : site_last_ms) t = 0;
    int rc = sample_set_ok(s);
    if (rc) return rc;
    sample_dict d;
    if ((rc = sample_dict_make(codes, C, size_of_sample, has_other, &d)) != RSBWT_OK) return rc;
    if (!strings && !copies && !aligned && !carriers) return fail(RSBWT_EINVAL, "null argument: no output array");
    if (Q == 0) return RSBWT_OK;
    if (!off || !pos || !alt || !isalt || (!text && off[Q] != off[0])) return fail(RSBWT_EINVAL, "null argument");
    for (size_t q = 0; q < Q; ++q) {
        if (off[q] > off[q + 1]) return fail(RSBWT_EINVAL, "query %zu: offsets not ascending", q);
        if (off[q + 1] - off[q] > (uint64_t)RSBWT_KSW_MAX_LEN)
            return fail(RSBWT_EINVAL, "query %zu: %llu symbols, at most %d", q, (unsigned long long)(off[q + 1] - off[q]), RSBWT_KSW_MAX_LEN);
    }
    const size_t S = s->shards.size(), G = s->groups.size(), width = C + 1;
    if (S > 65535) return fail(RSBWT_EINVAL, "%zu shards: at most 65535", S);
    uint32_t row_bits = 1;
    for (rsbwt_t *h : s->shards) {
        if (!rsbwt_opened_for_reads(h)) return fail(RSBWT_EINVAL, "site sample counts need shards opened with RSBWT_OPEN_READS");
        while (row_bits < 64 && (h->view.n >> row_bits) != 0) ++row_bits;
    }
    if (row_bits > 46) return fail(RSBWT_EINVAL, "a shard of 2^%u symbols: site sample counts take fewer than 2^46", row_bits);
    // slices: a request number of the set's keys has 24 bits, and a slice's matrices (12 bytes a cell) stay under 1.5 GiB of HBM
    const size_t SLICE = std::min<size_t>((size_t)1 << 24, std::max<size_t>(1, ((size_t)1 << 27) / width));
    const bool tight = sample_tight_set();
    uint64_t work10[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (size_t q0 = 0; q0 < Q; q0 += SLICE) {
        const size_t mq = std::min(SLICE, Q - q0), mcells = mq * width;
        uint32_t *st = strings ? strings + q0 * width : nullptr;
        int64_t *cp = copies ? copies + q0 * width : nullptr;
        uint64_t *al = aligned ? aligned + q0 : nullptr, *ca = carriers ? carriers + q0 : nullptr;
        gt_plan pl;
        if ((rc = gt_make_plan(text, off + q0, mq, pos + q0, k, skip, M, &pl)) != RSBWT_OK) return rc;
        if (st) memset(st, 0, mcells * 4);
        if (cp) memset(cp, 0, mcells * 8);
        if (al) memset(al, 0, mq * 8);
        if (ca) memset(ca, 0, mq * 8);
        if (pl.nitems == 0) continue;
        site_requests rq;
        rq.off.resize(mq + 1);
        rq.lo_w = (uint32_t)RSBWT_KSW_MAX_LEN;
        for (size_t q = 0; q <= mq; ++q) rq.off[q] = off[q0 + q] - off[q0];
        for (size_t q = 0; q < mq; ++q) {
            const uint32_t wl = (uint32_t)(rq.off[q + 1] - rq.off[q]);
            rq.hi_w = std::max(rq.hi_w, wl);
            if (wl) rq.lo_w = std::min(rq.lo_w, wl);
        }
#ifdef RSB_SITE_MUTANT_SLICE_ALT
        rq.alt = alt;
#else
        rq.alt = alt + q0;
#endif
        rq.isalt = isalt + q0;
        std::vector<site_group_out> outs(G);
        rc = for_each_group(s, [&](size_t gi) -> int {
            return site_group_run(s, s->groups[gi], pl, text + off[q0], rq, d, tight, row_bits, st != nullptr, cp != nullptr, &outs[gi]);
        });
        if (rc) return rc;
        for (const site_group_out &o : outs) {
            for (size_t i = 0; i < mcells; ++i) {
                if (st) st[i] += o.strings[i];
                if (cp) cp[i] += o.copies[i];
            }
            for (size_t q = 0; q < mq; ++q) {
                if (al) al[q] += o.aligned[q];
                if (ca) ca[q] += o.carriers[q];
            }
#ifdef RSB_SITE_MUTANT_SLICE_WORK
            for (int i = 0; i < 10; ++i) work10[i] = o.work[i];
#else
            for (int i = 0; i < 10; ++i) work10[i] += o.work[i];
#endif
            for (int i = 0; i < 6; ++i) site_last_ms[i] += o.ms[i];
        }
    }
    memcpy(site_last_work, work10, sizeof work10);
    return RSBWT_OK;
}

// ---- site reads (site_reads.hip): rsbwt_set_gt_aligned_reads' answer with the batch kept on the device ----
// the calling thread's last call: legs, LF steps spent lengthening, candidate rows, rows the span filter kept, distinct reads
// extracted, string classes among them, (request, read) items aligned, items kept, reads reported
thread_local uint64_t site_reads_last_work[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};

// reads = nullptr: first[] alone (want_bytes false), or the sizing call.  *total = the reads of the answer whatever the room.
int set_site_reads_body(rsbwt_set_t *s, const char *text, const uint64_t *off, size_t Q, const uint64_t *pos, const char *alt, const uint8_t *isalt,
                        int32_t k, int32_t skip, uint64_t M, uint64_t *first, bool want_bytes, char *reads, uint32_t read_stride, uint32_t *read_len,
                        uint64_t *read_row, size_t cap_reads, size_t *total) {
    for (uint64_t &w : site_reads_last_work) w = 0;
    *total = 0;
    if (!s) return fail(RSBWT_EINVAL, "null set");
    if (Q && (!off || !pos || !alt || !isalt || !first || (!text && off[Q] != off[0]))) return fail(RSBWT_EINVAL, "null argument");
    for (size_t q = 0; q < Q; ++q) {
        if (off[q] > off[q + 1]) return fail(RSBWT_EINVAL, "query %zu: offsets not ascending", q);
        if (off[q + 1] - off[q] > (uint64_t)RSBWT_KSW_MAX_LEN)
            return fail(RSBWT_EINVAL, "query %zu: %llu symbols, at most %d", q, (unsigned long long)(off[q + 1] - off[q]), RSBWT_KSW_MAX_LEN);
    }
    const size_t S = s->shards.size(), G = s->groups.size();
    if (S > 65535) return fail(RSBWT_EINVAL, "%zu shards: at most 65535", S);
    uint32_t row_bits = 1;
    for (rsbwt_t *h : s->shards) {
        if (h->view.n == 0) return fail(RSBWT_EINVAL, "empty index in the set");
        if (!rsbwt_opened_for_reads(h)) return fail(RSBWT_EINVAL, "site reads need shards opened with RSBWT_OPEN_READS");
        if (h->view.C[1] >= (1ull << 40)) return fail(RSBWT_EINVAL, "a shard of %llu strings: site reads take fewer than 2^40", (unsigned long long)h->view.C[1]);
        while (row_bits < 64 && (h->view.n >> row_bits) != 0) ++row_bits;
    }
    if (row_bits > 46) return fail(RSBWT_EINVAL, "a shard of 2^%u symbols: site reads take fewer than 2^46", row_bits);
    if (first) first[0] = 0;
    if (Q == 0) return RSBWT_OK;
    std::vector<std::pair<size_t, size_t>> where(S);  // shard of the set -> (group, shard of the group)
    for (size_t gi = 0; gi < G; ++gi)
        for (size_t j = 0; j < s->groups[gi]->idx.size(); ++j) where[s->groups[gi]->idx[j]] = {gi, j};
    const size_t SLICE = (size_t)1 << 24;  // a request number of the set's keys and of the layout's has 24 bits
    const sample_dict none;
    uint64_t work9[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    size_t at = 0;  // the reads of the slices before this one
    for (size_t q0 = 0; q0 < Q; q0 += SLICE) {
        const size_t mq = std::min(SLICE, Q - q0);
        gt_plan pl;
        int rc = gt_make_plan(text, off + q0, mq, pos + q0, k, skip, M, &pl);
        if (rc) return rc;
        if (pl.nitems == 0) {
            for (size_t c = q0 * S; c < (q0 + mq) * S; ++c) first[c + 1] = at;
            continue;
        }
        site_requests rq;
        rq.off.resize(mq + 1);
        rq.lo_w = (uint32_t)RSBWT_KSW_MAX_LEN;
        for (size_t q = 0; q <= mq; ++q) rq.off[q] = off[q0 + q] - off[q0];
        for (size_t q = 0; q < mq; ++q) {
            const uint32_t wl = (uint32_t)(rq.off[q + 1] - rq.off[q]);
            rq.hi_w = std::max(rq.hi_w, wl);
            if (wl) rq.lo_w = std::min(rq.lo_w, wl);
        }
        rq.alt = alt + q0;
        rq.isalt = isalt + q0;
        const size_t room = cap_reads > at ? cap_reads - at : 0;
        const bool direct = G == 1 && s->groups[0]->idx.size() == S && reads && read_len;  // (one group numbers the shards as the set does)
        std::vector<site_group_out> outs(G);
        std::vector<site_reads_out> rds(G);
        for (site_reads_out &rd : rds) {
            rd.want_bytes = want_bytes && reads && read_len;
            rd.stride = read_stride;
            rd.cap = room;
            if (direct) {
                rd.reads = reads + at * (size_t)read_stride;
                rd.len = read_len + at;
                rd.row = read_row ? read_row + at : nullptr;
            }
        }
        rc = for_each_group(s, [&](size_t gi) -> int {
            return site_group_run(s, s->groups[gi], pl, text + off[q0], rq, none, false, row_bits, false, false, &outs[gi], &rds[gi]);
        });
        if (rc) return rc;
        // ---- the groups' cells at their places: cell (q, p) is cell (q, j) of the group that holds shard p as its j-th
        size_t run = at;
        for (size_t q = 0; q < mq; ++q)
            for (size_t p = 0; p < S; ++p) {
                const site_reads_out &rd = rds[where[p].first];
                const size_t Sg = s->groups[where[p].first]->idx.size(), c = q * Sg + where[p].second;
                const size_t lo = (size_t)rd.first[c], cnt = (size_t)(rd.first[c + 1] - rd.first[c]);
                if (!direct && rd.stored && cnt && run + cnt <= cap_reads) {
                    memcpy(reads + run * (size_t)read_stride, rd.bytes_v.data() + lo * (size_t)read_stride, cnt * (size_t)read_stride);
                    memcpy(read_len + run, rd.len_v.data() + lo, cnt * 4);
                    if (read_row) memcpy(read_row + run, rd.row_v.data() + lo, cnt * 8);
                }
                run += cnt;
                first[(q0 + q) * S + p + 1] = run;
            }
        at = run;
        for (const site_group_out &o : outs)
            for (int i = 0; i < 9; ++i) work9[i] += o.work[i];
    }
    *total = at;
    memcpy(site_reads_last_work, work9, sizeof work9);
    return RSBWT_OK;
}

int read_file(const char *path, std::string *out) {
    FILE *f = fopen(path, "rb");
    if (!f) return fail(RSBWT_EIO, "cannot open %s", path);
    char buf[1 << 16];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, f)) > 0) out->append(buf, got);
    const bool bad = ferror(f) != 0;
    fclose(f);
    return bad ? fail(RSBWT_EIO, "cannot read %s", path) : RSBWT_OK;
}

}  // namespace

static void meta_free(rsbwt_set_t *s) {
    meta_free_tables(s, s->meta);
    s->meta_bytes = 0;
    s->meta_head_bytes = 0;
}

namespace {
// the service code's way in (service.h: service_slice.cpp is also linked into host harnesses without the engine)
struct register_meta_hooks {
    register_meta_hooks() {
        rsb::meta_engine_hooks.read_meta_var = rsbwt_set_read_meta_var;
        rsb::meta_engine_hooks.meta_bytes = rsbwt_set_meta_bytes;
    }
} register_meta_hooks_now;
// what service_slice.cpp reaches the site reads calls through (service.h)
struct register_site_hooks {
    register_site_hooks() {
        rsb::site_engine_hooks.reads = rsbwt_set_site_reads;
        rsb::site_engine_hooks.counts = rsbwt_set_site_read_counts;
    }
} register_site_hooks_now;
}  // namespace

extern "C" {

int rsbwt_set_meta_build(rsbwt_set_t *s, const char *text, const uint64_t *off, const uint8_t *values, const uint64_t *voff, size_t n,
                         uint64_t *stats4) {
    return guarded("rsbwt_set_meta_build", [&]() -> int { return set_meta_build_body(s, text, off, values, voff, n, stats4); });
}

// The whole file is parsed into pairs on the host (two copies of it at the peak) and built as rsbwt_set_meta_build builds:
// the higher index wins over the whole file because the pairs keep the file's order.
int rsbwt_set_meta_load(rsbwt_set_t *s, const char *path, uint64_t *stats4) {
    return guarded("rsbwt_set_meta_load", [&]() -> int {
        if (!s || !path) return fail(RSBWT_EINVAL, "null argument");
        meta_pairs pairs;
        {
            std::string data;
            const int rc = read_file(path, &data);
            if (rc) return rc;
            meta_parse_pairs(data.data(), data.size(), &pairs);
        }
        return set_meta_build_body(s, pairs.text.data(), pairs.off.data(), (const uint8_t *)pairs.values.data(), pairs.voff.data(), pairs.size(),
                                   stats4);
    });
}

int rsbwt_set_meta_clear(rsbwt_set_t *s) {
    return guarded("rsbwt_set_meta_clear", [&]() -> int {
        if (!s) return fail(RSBWT_EINVAL, "null set");
        meta_free(s);
        return meta_publish(s);
    });
}

uint64_t rsbwt_set_meta_bytes(const rsbwt_set_t *s) { return s ? s->meta_bytes : 0; }

int rsbwt_set_read_ordinals_var(rsbwt_set_t *s, const char *text, const uint64_t *off, size_t Q, uint64_t *ordinal, uint64_t *copies) {
    return guarded("rsbwt_set_read_ordinals_var", [&]() -> int {
        if (Q && (!ordinal || !copies)) return fail(RSBWT_EINVAL, "null argument");
        return rsbwt_set_read_copies_var_body(s, text, off, Q, copies, nullptr, ordinal);
    });
}

int rsbwt_set_meta_by_ordinal(rsbwt_set_t *s, const uint32_t *shard_of, const uint64_t *ordinal, size_t n, uint64_t *first, uint8_t *bytes,
                              size_t cap, size_t *nbytes) {
    return guarded("rsbwt_set_meta_by_ordinal", [&]() -> int {
        for (uint64_t &w : meta_last_work) w = 0;
        if (!s || !first || !nbytes || (n && (!shard_of || !ordinal))) return fail(RSBWT_EINVAL, "null argument");
        *nbytes = 0;
        first[0] = 0;
        const int rc = meta_required(s);
        if (rc || n == 0) return rc;
        return set_meta_by_ordinal_body(s, shard_of, ordinal, n, first, bytes, cap, nbytes);
    });
}

int rsbwt_set_meta_by_ordinal_dev(rsbwt_set_t *s, const void *d_shard, const void *d_ordinal, size_t n, void *d_first, void *d_bytes, size_t cap,
                                  void *stream) {
    return guarded("rsbwt_set_meta_by_ordinal_dev", [&]() -> int {
        dev_group *g = nullptr;
        int rc = one_device_group(s, &g);
        if (rc) return rc;
        if ((rc = meta_required(s)) != RSBWT_OK) return rc;
        if (!d_first || (n && (!d_shard || !d_ordinal))) return fail(RSBWT_EINVAL, "null argument");
        hipStream_t st = (hipStream_t)stream;
        if (n == 0) {
            HIP_OK(hipMemsetAsync(d_first, 0, 8, st));
            return RSBWT_OK;
        }
        const size_t a8 = al256((n + 1) * 8), a_tmp = meta_scan_bytes(n + 1);
        scratch_cache::lease mem;
        hipError_t e = g->scratch.take(2 * a8 + a_tmp, st, &mem);
        if (e != hipSuccess) return fail_hip(e, "scratch for a sample lookup");
        uint8_t *d_len = (uint8_t *)mem.p, *d_src = d_len + a8, *d_tmp = d_src + a8;
        const uint32_t S = (uint32_t)g->idx.size();
        e = launch_meta_sizes(g->d_meta, S, d_shard, d_ordinal, nullptr, 0, n, d_len, d_src, st);
        if (e == hipSuccess) e = launch_meta_scan(d_tmp, a_tmp, d_len, d_first, n + 1, st);
        if (e == hipSuccess && d_bytes && cap) e = launch_meta_copy(g->d_meta, S, d_shard, 0, nullptr, d_src, d_first, n, d_bytes, cap, st);
        g->scratch.give(mem, st);
        return e == hipSuccess ? RSBWT_OK : fail_hip(e, "sample lookup kernels");
    });
}

int rsbwt_set_read_meta_var(rsbwt_set_t *s, const char *text, const uint64_t *off, size_t Q, uint64_t *first, uint8_t *bytes, size_t cap,
                            size_t *nbytes, uint64_t *copies) {
    return guarded("rsbwt_set_read_meta_var", [&]() -> int {
        for (uint64_t &w : meta_last_work) w = 0;
        if (!s || !first || !nbytes) return fail(RSBWT_EINVAL, "null argument");
        *nbytes = 0;
        first[0] = 0;
        const int rc = meta_required(s);
        if (rc || Q == 0) return rc;
        if (!off || (!text && off[Q] != off[0])) return fail(RSBWT_EINVAL, "null argument");
        return set_read_meta_var_body(s, text, off, Q, first, bytes, cap, nbytes, copies);
    });
}

void rsbwt_set_meta_last_work(uint64_t *work4) {
    if (work4) memcpy(work4, meta_last_work, sizeof meta_last_work);
}

int rsbwt_set_sample_counts(rsbwt_set_t *s, const char *text, const uint64_t *off, size_t Q, const uint8_t *codes, size_t C, uint32_t size_of_sample,
                            int has_other_meta_data, uint64_t max_rows, uint32_t max_steps, uint32_t *strings, int64_t *copies, uint64_t *matches,
                            uint64_t *carriers) {
    return guarded("rsbwt_set_sample_counts", [&]() -> int {
        for (uint64_t &w : sample_last_work) w = 0;
        return set_sample_counts_body(s, text, off, Q, codes, C, size_of_sample, has_other_meta_data, max_rows, max_steps, strings, copies, matches,
                                      carriers);
    });
}

// one-device set, the caller's buffers and stream, nothing synchronised
int rsbwt_set_sample_counts_dev(rsbwt_set_t *s, const void *d_text, const void *d_off, size_t Q, uint32_t max_len, const void *d_keys, size_t C,
                                uint32_t size_of_sample, int has_other_meta_data, uint64_t max_rows, uint32_t max_steps, size_t cap_rows,
                                void *d_strings, void *d_copies, void *d_matches, void *d_carriers, void *d_status8, void *stream) {
    return guarded("rsbwt_set_sample_counts_dev", [&]() -> int {
        dev_group *g = nullptr;
        int rc = one_device_group(s, &g);
        if (rc) return rc;
        if ((rc = sample_set_ok(s)) != RSBWT_OK) return rc;
        if ((rc = sample_shape_ok(C, size_of_sample)) != RSBWT_OK) return rc;
        if (!d_keys || !d_status8) return fail(RSBWT_EINVAL, "null argument");
        if (!d_strings && !d_copies && !d_matches && !d_carriers) return fail(RSBWT_EINVAL, "null argument: no output array");
        hipStream_t st = (hipStream_t)stream;
        if (Q == 0) {
            HIP_OK(hipMemsetAsync(d_status8, 0, 64, st));
            return RSBWT_OK;
        }
        if (!d_text || !d_off) return fail(RSBWT_EINVAL, "null argument");
        if (Q > ((size_t)1 << 24)) return fail(RSBWT_EINVAL, "%zu queries: the device form takes at most 2^24 per call", Q);
        if (max_len == 0 || max_len > 65535u) return fail(RSBWT_EINVAL, "max_len %u: 1 to 65,535 symbols", max_len);
        if (cap_rows >= ((size_t)1 << 38)) return fail(RSBWT_ERANGE, "room for %zu rows: at most 2^38 per call", cap_rows);
        const uint32_t S = (uint32_t)g->idx.size(), wpq = words_per_kmer(max_len);
        if (S > 1024) return fail(RSBWT_EINVAL, "%u shards: the device form takes at most 1,024", S);
        sample_dict d;
        d.C = (uint32_t)C;
        d.size_of_sample = size_of_sample;
        d.has_other = has_other_meta_data ? 1u : 0u;
        const size_t a_pk = al256(Q * wpq * 8), a_ok = al256(Q), a_len = al256(Q * 4), a_rec = al256((size_t)S * Q * 16), a_q = al256((Q + 1) * 8),
                     tmp_bytes = interval_rows_scan_bytes(Q + 1), a8 = al256(cap_rows * 8), a4 = al256(cap_rows * 4);
        scratch_cache::lease mem;
        hipError_t e = g->scratch.take(a_pk + a_ok + a_len + 2 * a_rec + 3 * a_q + 512 + tmp_bytes + 256 + 2 * a8 + a4 + sample_tally_scratch(S, cap_rows),
                                       st, &mem);
        if (e != hipSuccess) return fail_hip(e, "scratch for sample counts");
        uint8_t *d_pk = (uint8_t *)mem.p, *d_ok = d_pk + a_pk, *d_len = d_ok + a_ok, *d_rec = d_len + a_len, *d_pairs = d_rec + a_rec,
                *d_mt = d_pairs + a_rec, *d_kept = d_mt + a_q, *d_first = d_kept + a_q, *d_over = d_first + a_q, *d_wk = d_over + 256,
                *d_tmp = d_wk + 256, *d_rows = d_tmp + tmp_bytes + 256, *d_od = d_rows + a8, *d_sh = d_od + a8, *d_scratch = d_sh + a4;
        void *matches = d_matches ? d_matches : (void *)d_mt;
        rc = [&]() -> int {
            if ((e = launch_pack_var(d_text, d_off, Q, wpq, d_pk, d_ok, d_len, st)) != hipSuccess) return fail_hip(e, "pack kernel launch");
            if ((e = launch_search_init_var(g->d_views, S, d_pk, d_ok, d_len, Q, wpq, d_rec, st)) != hipSuccess)
                return fail_hip(e, "start-record kernel launch");
            search_extra ex;
            ex.narrow = group_is_narrow(s, g, max_len);
            ex.d_init = d_rec;
            ex.pairs = true;
            const int rs = search_launch(*g, g->d_views, S, g->num_cus, d_pk, d_ok, Q, max_len, d_pairs, nullptr, false, st, &ex);
            if (rs) return rs;
            if ((e = launch_interval_totals(g->d_views, S, d_pairs, Q, max_rows, matches, d_kept, d_first, d_over, d_tmp, tmp_bytes, st)) != hipSuccess)
                return fail_hip(e, "interval-rows kernels");
            if (cap_rows) {
                // (rows past first[Q], and every row when first[Q] > cap_rows, name no shard: the walk leaves them alone)
                HIP_OK(hipMemsetAsync(d_sh, 0xFF, cap_rows * 4, st));
                HIP_OK(hipMemsetAsync(d_od, 0xFF, cap_rows * 8, st));
                if ((e = launch_interval_fill(g->d_views, S, d_pairs, Q, d_first, cap_rows, d_sh, d_rows, nullptr, nullptr, nullptr, st)) != hipSuccess)
                    return fail_hip(e, "row expansion");
                HIP_OK(hipMemsetAsync(d_wk, 0, 16, st));
                e = launch_locate(g->scratch, g->d_views, S, d_sh, d_rows, cap_rows, max_steps, nullptr, d_od, nullptr, (unsigned long long *)d_wk,
                                  g->num_cus, st);
                if (e != hipSuccess) return fail_hip(e, "locate kernel launch");
            } else {
                HIP_OK(hipMemsetAsync(d_wk, 0, 16, st));
            }
            return sample_tally_enqueue(g, st, d_scratch, d_first, Q, d_sh, d_od, cap_rows, d_keys, d, sample_tight_set(), d_wk, d_strings, d_copies,
                                        d_carriers, d_status8);
        }();
        g->scratch.give(mem, st);
        return rc;
    });
}

void rsbwt_set_sample_last_work(uint64_t *work6) {
    if (work6) memcpy(work6, sample_last_work, sizeof sample_last_work);
}

uint64_t rsbwt_set_meta_head_bytes(const rsbwt_set_t *s) { return s ? s->meta_head_bytes : 0; }

int rsbwt_sample_keys(const uint8_t *codes, size_t C, uint32_t size_of_sample, uint64_t *keys) {
    return guarded("rsbwt_sample_keys", [&]() -> int {
        sample_dict d;
        const int rc = sample_dict_make(codes, C, size_of_sample, 0, &d);
        if (rc) return rc;
        if (!keys) return fail(RSBWT_EINVAL, "null argument");
        memcpy(keys, d.keys.data(), C * 8);
        return RSBWT_OK;
    });
}

int rsbwt_set_site_sample_counts(rsbwt_set_t *s, const char *text, const uint64_t *off, size_t Q, const uint64_t *pos, const char *alt,
                                 const uint8_t *isalt, int32_t k, int32_t skip, uint64_t M, const uint8_t *codes, size_t C, uint32_t size_of_sample,
                                 int has_other_meta_data, uint32_t *strings, int64_t *copies, uint64_t *aligned, uint64_t *carriers) {
    return guarded("rsbwt_set_site_sample_counts", [&]() -> int {
        const int rc = set_site_counts_body(s, text, off, Q, pos, alt, isalt, k, skip, M, codes, C, size_of_sample, has_other_meta_data, strings, copies,
                                            aligned, carriers);
        if (rc)
            for (uint64_t &w : site_last_work) w = 0;
        return rc;
    });
}

void rsbwt_set_site_last_work(uint64_t *work10) {
    if (work10) memcpy(work10, site_last_work, sizeof site_last_work);
}

void rsbwt_set_site_last_times(double *ms6) {
    if (ms6) memcpy(ms6, site_last_ms, sizeof site_last_ms);
}

int rsbwt_set_site_reads(rsbwt_set_t *s, const char *text, const uint64_t *off, size_t Q, const uint64_t *pos, const char *alt, const uint8_t *isalt,
                         int32_t k, int32_t skip, uint64_t M, uint64_t *first, char *reads, uint32_t read_stride, uint32_t *read_len, uint64_t *read_row,
                         size_t cap_reads, size_t *nreads) {
    return guarded("rsbwt_set_site_reads", [&]() -> int {
        if (!nreads || (!first && Q)) return fail(RSBWT_EINVAL, "null argument");
        *nreads = 0;
        if (read_stride == 0) return fail(RSBWT_EINVAL, "read_stride must be positive");
        size_t total = 0;
        int rc = set_site_reads_body(s, text, off, Q, pos, alt, isalt, k, skip, M, first, true, reads, read_stride, read_len, read_row, cap_reads, &total);
        if (rc == RSBWT_OK) {
            *nreads = total;
            if (total > cap_reads) rc = fail(RSBWT_ERANGE, "%zu reads, room for %zu", total, cap_reads);
            else if (total != 0 && (!reads || !read_len)) rc = fail(RSBWT_EINVAL, "null argument");
        }
        if (rc != RSBWT_OK)
            for (uint64_t &w : site_reads_last_work) w = 0;
        return rc;
    });
}

int rsbwt_set_site_read_counts(rsbwt_set_t *s, const char *text, const uint64_t *off, size_t Q, const uint64_t *pos, const char *alt,
                               const uint8_t *isalt, int32_t k, int32_t skip, uint64_t M, uint64_t *counts) {
    return guarded("rsbwt_set_site_read_counts", [&]() -> int {
        if (!counts && Q) return fail(RSBWT_EINVAL, "null argument");
        const size_t cells = s ? Q * s->shards.size() : 0;
        std::vector<uint64_t> first(cells + 1, 0);
        size_t total = 0;
        const int rc = set_site_reads_body(s, text, off, Q, pos, alt, isalt, k, skip, M, first.data(), false, nullptr, 256, nullptr, nullptr, 0, &total);
        if (rc != RSBWT_OK) {
            for (uint64_t &w : site_reads_last_work) w = 0;
            return rc;
        }
        for (size_t c = 0; c < cells; ++c) counts[c] = first[c + 1] - first[c];
        return RSBWT_OK;
    });
}

void rsbwt_set_site_reads_last_work(uint64_t *work9) {
    if (work9) memcpy(work9, site_reads_last_work, sizeof site_reads_last_work);
}

int rsbwt_rccl_available(void) { return rccl().ok ? 1 : 0; }

// measurement hooks of the set's first device group (bench.py)
int rsbwt_set_set_counting(rsbwt_set_t *s, int on) {
    if (!s) return fail(RSBWT_EINVAL, "null set");
    for (dev_group *g : s->groups) {
        std::lock_guard<std::mutex> lock(g->mu);
        g->counting = on != 0;
    }
    return RSBWT_OK;
}

int rsbwt_set_search_history_ms(rsbwt_set_t *s, float *ms, size_t cap, size_t *count) {
    if (!s || (!ms && cap) || !count) return fail(RSBWT_EINVAL, "null argument");
    int rc = use_device(s->groups[0]->device);
    if (rc) return rc;
    return meter_history_ms(*s->groups[0], ms, cap, count);
}

int rsbwt_set_last_search_counters(rsbwt_set_t *s, uint64_t *words16) {
    if (!s || !words16) return fail(RSBWT_EINVAL, "null argument");
    int rc = use_device(s->groups[0]->device);
    if (rc) return rc;
    return meter_work(*s->groups[0], words16, WORK_WORDS);
}

}  // extern "C"
