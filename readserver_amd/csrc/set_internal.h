// set_internal.h -- what the translation units of the shard-set code (sets.hip, set_graph.hip) share: the set and its
// device groups behind include/rsbwt.h's rsbwt_set_t, the ways a call runs on one group or on all of them, and the checks
// of a sample dictionary.  The functions are inline: every translation unit that includes this shares one copy.
#ifndef RSBWT_SET_INTERNAL_H
#define RSBWT_SET_INTERNAL_H

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>
#include <stdint.h>

#include <atomic>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/rsbwt.h"
#include "capi_internal.h"
#include "sample_codes.h"

using namespace rsb;

#define HIP_OK(x)                                              \
    do {                                                       \
        hipError_t _e = (x);                                   \
        if (_e != hipSuccess) return fail_hip(_e, #x);         \
    } while (0)

// the shards of one device
struct dev_group : search_meter {
    int device = 0;   // the GPU
    int logical = 0;  // the device number its shards were opened with: what groups them (= device outside tests, capi.hip resolve_device)
    int num_cus = 256;
    std::vector<size_t> idx;         // positions in the set, ascending
    shard_view *d_views = nullptr;   // [idx.size()] in HBM: what the searches read (written by make_groups and when tables are attached, never else)
    shard_view *d_xviews = nullptr;  // the same WITH the shards' select samples, for the fused extraction: a second array, made once
    std::atomic<bool> xviews_ready{false};
    uint64_t *d_ktab = nullptr;      // the interleaved k-mer tables of the shards this set gave one
    meta_view *d_meta = nullptr;     // [idx.size()] in HBM: the shards' sample tables (rsbwt_set_meta_*), made with the first build
    ctx_pool pool;
    ncclComm_t comm = nullptr;
    // the gather without RCCL (peer copies issued on the root's stream): "the block is ready" on this group's stream,
    // "the block has been read" back onto it
    hipEvent_t peer_ready = nullptr, peer_done = nullptr;
    // side streams for calls that let the group's shards work side by side (small 1-mismatch batches: one shard's
    // launch does not fill the GPU), forked from and joined to the caller's stream with events; made on first use
    static constexpr int FORK = 8;
    hipStream_t fork_st[FORK] = {};
    hipEvent_t fork_ev = nullptr, join_ev[FORK] = {};
    std::mutex fork_mu;
    int ensure_fork() {
        if (fork_ev) return RSBWT_OK;  // (set last: everything below exists)
        // each stream / event is made once, whatever a previous, partly failed attempt left behind
        for (int i = 0; i < FORK; ++i) {
            if ((!fork_st[i] && hipStreamCreateWithFlags(&fork_st[i], hipStreamNonBlocking) != hipSuccess) ||
                (!join_ev[i] && hipEventCreateWithFlags(&join_ev[i], hipEventDisableTiming) != hipSuccess)) {
                (void)hipGetLastError();
                return fail(RSBWT_EHIP, "cannot create the side streams of a shard set");
            }
        }
        if (hipEventCreateWithFlags(&fork_ev, hipEventDisableTiming) != hipSuccess) {
            fork_ev = nullptr;
            return fail(RSBWT_EHIP, "cannot create an event");
        }
        return RSBWT_OK;
    }
};

struct rsbwt_set {
    std::vector<rsbwt_t *> shards;
    bool owns = false;
    std::vector<dev_group *> groups;
    bool comms_tried = false, comms_ok = false;
    std::mutex mu;
    // Collectives on the set's communicators are enqueued by one thread at a time: two callers
    // interleaving their group calls could reach the communicators in different orders.
    std::mutex comm_mu;
    // the per-read sample table (rsbwt_set_meta_*): shard i's off u64[num_strings + 1] / value bytes, on shard i's device;
    // empty = no table.  Written by build / load / clear only, which must not run beside a lookup.
    // d_heads: one bit per ordinal, set at the first ordinal of every string a pair named (rsbwt_set_sample_counts)
    struct meta_shard {
        uint64_t *d_off = nullptr;
        uint8_t *d_bytes = nullptr;
        uint32_t *d_heads = nullptr;
    };
    std::vector<meta_shard> meta;
    uint64_t meta_bytes = 0, meta_head_bytes = 0;
};

// runs fn(group index) for every device group, concurrently when there are several
template <class F>
int for_each_group(rsbwt_set_t *s, F &&fn) {
    const size_t G = s->groups.size();
    if (G == 1) return fn(0);
    std::vector<int> rcs(G, RSBWT_OK);
    std::vector<std::string> errs(G);
    std::vector<std::thread> th;
    for (size_t g = 0; g < G; ++g)
        th.emplace_back([&, g] {
            rcs[g] = fn(g);
            if (rcs[g]) errs[g] = rsbwt_last_error();  // the message is thread-local: carry it over
        });
    for (auto &t : th) t.join();
    for (size_t g = 0; g < G; ++g)
        if (rcs[g]) return fail(rcs[g], "%s", errs[g].c_str());
    return RSBWT_OK;
}

// What every device-resident call of a set starts with: they serve a set whose shards all sit on one device.
inline int one_device_group(rsbwt_set_t *s, dev_group **g) {
    if (!s) return fail(RSBWT_EINVAL, "null set");
    if (s->groups.size() != 1) return fail(RSBWT_EINVAL, "the set spans %zu devices: device-resident calls need one", s->groups.size());
    *g = s->groups[0];
    return use_device((*g)->device);
}

// A call context on g's device for the duration of one host-buffer call; rc says whether there is one.  The capped
// calls also lease their scratch through it (la, lb): their launches may still run when such a call leaves early, so
// the destructor waits for the stream before the leases go back.  A call without leases waits for nothing here.
struct group_call {
    dev_group *const g;
    const bool leases;
    int rc;
    call_ctx *c = nullptr;
    hipStream_t st = nullptr;
    scratch_cache::lease la, lb;
    explicit group_call(dev_group *grp, bool with_leases = false) : g(grp), leases(with_leases), rc(use_device(grp->device)) {
        if (rc == RSBWT_OK && !(c = g->pool.acquire())) rc = fail(RSBWT_EHIP, "cannot create a HIP stream");
        if (c) st = c->st[0];
    }
    group_call(const group_call &) = delete;
    ~group_call() {
        if (!c) return;
        if (leases) {
            (void)hipStreamSynchronize(st);
            g->scratch.give(la, st);
            g->scratch.give(lb, st);
        }
        g->pool.release(c);
    }
};

inline int meta_required(const rsbwt_set_t *s) {
    return s->meta.empty() ? fail(RSBWT_EINVAL, "the set has no sample table (rsbwt_set_meta_build / rsbwt_set_meta_load)") : RSBWT_OK;
}

struct sample_dict {
    std::vector<uint64_t> keys;  // (host form; the device form brings them in HBM)
    uint32_t C = 0, size_of_sample = 0, has_other = 0;
};

inline int sample_shape_ok(size_t C, uint32_t size_of_sample) {
    if (size_of_sample < 1u || size_of_sample > SAMPLE_CODE_MAX) return fail(RSBWT_EINVAL, "size_of_sample %u: 1 to 8 bytes", size_of_sample);
    if (C == 0) return fail(RSBWT_EINVAL, "an empty sample dictionary");
    if (C >= (1ull << 31)) return fail(RSBWT_EINVAL, "%zu sample codes: at most 2^31 - 1", C);
    return RSBWT_OK;
}

inline int sample_dict_make(const uint8_t *codes, size_t C, uint32_t size_of_sample, int has_other, sample_dict *d) {
    const int rc = sample_shape_ok(C, size_of_sample);
    if (rc) return rc;
    size_t bad = 0;
    switch (sample_codes_check(codes, C, size_of_sample, &d->keys, &bad)) {
    case SAMPLE_CODES_OK: break;
    case SAMPLE_CODES_ORDER: return fail(RSBWT_EINVAL, "sample code %zu is not above code %zu: the dictionary must be strictly ascending", bad, bad - 1);
    default: return fail(RSBWT_EINVAL, "null argument");
    }
    d->C = (uint32_t)C;
    d->size_of_sample = size_of_sample;
    d->has_other = has_other ? 1u : 0u;
    return RSBWT_OK;
}

inline int sample_set_ok(const rsbwt_set_t *s) {
    if (!s) return fail(RSBWT_EINVAL, "null set");
    const int rc = meta_required(s);
    if (rc) return rc;
    for (const rsbwt_t *h : s->shards) {
        if (h->view.n == 0) return fail(RSBWT_EINVAL, "empty index in the set");
        if (h->view.C[1] >= (1ull << 40)) return fail(RSBWT_EINVAL, "a shard of %llu strings: sample counts take fewer than 2^40", (unsigned long long)h->view.C[1]);
    }
    return RSBWT_OK;
}

#endif
