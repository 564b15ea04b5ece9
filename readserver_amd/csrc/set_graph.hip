// set_graph.hip -- the k-mer graph calls of a shard set (include/rsbwt.h: the definitions): extension counts, walks,
// unitigs and paths (walk.hip, paths.hip), and the same through one sample set's reads (sample_walk.hip).
//
// A set on one device group runs a whole call as one launch sequence there (*_host_views, sample_walk_group).  A set over
// several groups runs graph_steps.h's loop on the host: per step every group evaluates the contexts still in play -- their
// symbols alone are sent -- and the host adds the groups' answers and decides.  The device-resident forms serve a set on
// one device, on the caller's buffers and stream, and wait for nothing.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/rsbwt.h"
#include "capi_guard.h"
#include "capi_internal.h"
#include "graph_steps.h"
#include "set_internal.h"

namespace {
int walk_set_check(rsbwt_set_t *s) {
    // (no set can be had on a box without a GPU: the call says so instead of blaming the argument)
    if (!s && rsbwt_device_count() == 0) return fail(RSBWT_ENODEV, "no HIP device is visible: the popBWT engine has no CPU fallback");
    if (!s) return fail(RSBWT_EINVAL, "null set");
    for (rsbwt_t *h : s->shards)
        if (h->view.n == 0) return fail(RSBWT_EINVAL, "empty index in the set");
    return RSBWT_OK;
}

// One evaluation of every seed in every shard: each device group counts its shards' rows of counts[S][Q][4], side by
// side; the host only puts group gi's row j at row idx[j].  work6[2..5] += the launches' counters.
int extension_groups(rsbwt_set_t *s, const char *t0, const uint64_t *rel, size_t Q, size_t N, uint32_t ctx, uint32_t flags, uint64_t *counts,
                     uint64_t *work6) {
    struct group_out {
        std::vector<uint64_t> counts;
        uint64_t work[6] = {0, 0, 0, 0, 0, 0};
    };
    std::vector<group_out> outs(s->groups.size());
    const size_t row = Q * 4;
    int rc = for_each_group(s, [&](size_t gi) -> int {
        dev_group *g = s->groups[gi];
        group_call gc(g);
        if (gc.rc) return gc.rc;
        group_out &o = outs[gi];
        const size_t Sg = g->idx.size();
        // (a group whose shards sit next to each other in the set answers straight into the caller's rows)
        uint64_t *dst = counts + g->idx.front() * row;
        if (g->idx.back() - g->idx.front() + 1 != Sg) {
            o.counts.resize(Sg * row);
            dst = o.counts.data();
        }
        return extension_host_views(g->scratch, gc.st, g->d_views, (uint32_t)Sg, t0, rel, Q, N, ctx, flags, dst, o.work);
    });
    if (rc) return rc;
    for (size_t gi = 0; gi < outs.size(); ++gi) {
        const dev_group *g = s->groups[gi];
        const group_out &o = outs[gi];
        for (size_t j = 0; !o.counts.empty() && j < g->idx.size(); ++j) memcpy(counts + g->idx[j] * row, o.counts.data() + j * row, row * 8);
        for (int i = 2; i < 6; ++i) work6[i] += o.work[i];
    }
    return RSBWT_OK;
}

// ---- sample walks (sample_walk.hip): seeds extended through one sample set's reads ----
// the calling thread's last host-form call: seeds, appended symbols, candidate searches, their LF steps, rows located, rows
// on a head ordinal, distinct carriers, records read, LF steps of the rows' walks, wide evaluations
thread_local uint64_t sample_walk_last[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
// ... and, while RSBWT_SAMPLE_WALK_TIMES=1, the device time of its launches in ms by kind, from events round every launch on
// the call's stream, summed over steps, slices and device groups: {init, search, plan, rows, locate, tally, decide}
thread_local double sample_walk_ms[SAMPLE_WALK_KINDS] = {0, 0, 0, 0, 0, 0, 0};

// (null: zeros, as walk_set_last_work)
void sample_walk_set_last_work(const uint64_t *work10) {
    for (int i = 0; i < 10; ++i) sample_walk_last[i] = work10 ? work10[i] : 0;
}

// (read at every call: a probe turns it on and off inside one process)
bool sample_walk_times_on() {
    const char *e = getenv("RSBWT_SAMPLE_WALK_TIMES");
    return e && e[0] == '1' && e[1] == 0;
}

// the marks of one enqueue -> ms[kind] += ...; the events are destroyed.  After the stream has been waited for.
void sample_walk_read_marks(std::vector<hipEvent_t> &marks, double *ms) {
    for (size_t i = 1; i < marks.size(); ++i) {
        float dt = 0;
        if (hipEventElapsedTime(&dt, marks[i - 1], marks[i]) == hipSuccess) ms[i == 1 ? 0 : 1 + (i - 2) % 6] += dt;
        else (void)hipGetLastError();
    }
    for (hipEvent_t ev : marks) (void)hipEventDestroy(ev);
    marks.clear();
}

struct sample_walk_call {
    sample_dict d;
    std::vector<uint32_t> bits;  // the mask, a bit per column
    uint64_t max_rows = 0;
    uint32_t max_locate_steps = 0;
};

int sample_walk_shape_ok(const rsbwt_set_t *s, uint64_t max_rows) {
    if (!sample_walk_rows_ok(max_rows)) return fail(RSBWT_EINVAL, "max_rows = %llu: 1 to 2^20 for a sample walk", (unsigned long long)max_rows);
    for (const dev_group *g : s->groups)
        if (g->idx.size() > SAMPLE_WALK_MAX_SHARDS) return fail(RSBWT_EINVAL, "%zu shards on one device: a sample walk takes at most 1,024", g->idx.size());
    return RSBWT_OK;
}

int sample_walk_prepare(rsbwt_set_t *s, const uint8_t *codes, size_t C, uint32_t size_of_sample, int has_other, const uint8_t *mask, uint64_t max_rows,
                        uint32_t max_locate_steps, sample_walk_call *c) {
    int rc = sample_set_ok(s);
    if (rc) return rc;
    if ((rc = sample_dict_make(codes, C, size_of_sample, has_other, &c->d)) != RSBWT_OK) return rc;
    if (!mask) return fail(RSBWT_EINVAL, "null argument: mask");
    if ((rc = sample_walk_shape_ok(s, max_rows)) != RSBWT_OK) return rc;
    c->bits.resize(sample_walk_mask_words(C));
    sample_walk_mask_bits(mask, C, c->bits.data());
    c->max_rows = max_rows;
    c->max_locate_steps = max_locate_steps;
    return RSBWT_OK;
}

void sample_walk_add_work(uint64_t *work10, const unsigned long long *dev) {
    auto w = [&](int which) { return (uint64_t)dev[(size_t)which * TALLY_WORK_STRIDE]; };
    work10[1] += w(SW_WORK_APPENDED);
    work10[2] += w(SW_WORK_SEARCHES);
    work10[3] += w(SW_WORK_SEARCH_STEPS);
    work10[4] += w(SW_WORK_ROWS);
    work10[5] += w(SW_WORK_HEADS);
    work10[6] += w(SW_WORK_CARRIERS);
    work10[7] += w(SW_WORK_RECORDS);
    work10[8] += w(SW_WORK_LOCATE_STEPS);
    work10[9] += w(SW_WORK_WIDE);
}

// What sample_walk_enqueue takes for seeds q0 .. q0 + mq of a batch in HBM (bt: the whole batch; dict: C, size_of_sample,
// has_other), but for what differs between its callers: where the slice's outputs are, evaluate-only, the marks.
sample_walk_args sample_walk_slice(const dev_group *g, const walk_batch &bt, size_t q0, size_t mq, const void *d_keys, const void *d_bits,
                                   const sample_dict &dict, uint64_t max_rows, uint32_t max_locate_steps, void *d_work) {
    sample_walk_args a;
    a.views = g->d_views;
    a.meta = g->d_meta;
    a.S = (uint32_t)g->idx.size();
    a.num_cus = g->num_cus;
    a.bt = bt;
    a.bt.off = bt.off + q0;
    a.bt.Q = mq;
    a.keys = (const uint64_t *)d_keys;
    a.mask_bits = (const uint32_t *)d_bits;
    a.C = dict.C;
    a.size_of_sample = dict.size_of_sample;
    a.has_other = dict.has_other;
    a.max_rows = max_rows;
    a.max_locate_steps = max_locate_steps;
    a.ext = a.steps = a.stop = a.support = a.last = nullptr;
    a.evaluate_only = 0u;
    a.raw = a.matches8 = a.wide = nullptr;
    a.work = (unsigned long long *)d_work;
    return a;
}

// What a host-form call runs on one device group on `gc`'s stream: the batch, the dictionary and the mask go up once, then
// the seeds are walked (or evaluated once: evaluate) slice by slice -- sample_walk_slice_seeds -- each slice's launches
// enqueued blind and its answers copied back; the stream is waited for once per slice, never between steps.
// walk: ext, steps, stop, support (optional), last (optional).  evaluate: raw i64[Q][8], m8 u64[Q][8], wide u8[Q].
int sample_walk_group(dev_group *g, group_call &gc, const char *t0, const uint64_t *rel, size_t Q, size_t N, uint32_t ctx, uint64_t m,
                      uint32_t max_steps, uint32_t flags, const sample_walk_call &c, bool evaluate, char *ext, uint32_t *steps, uint8_t *stop,
                      uint32_t *support, uint64_t *last, int64_t *raw, uint64_t *m8, uint8_t *wide, uint64_t *work10, double *ms = nullptr) {
    if (Q == 0) return RSBWT_OK;
    std::vector<hipEvent_t> marks;
    struct drop_marks {  // (a call that leaves early: group_call's destructor has the stream waited for before the events go)
        std::vector<hipEvent_t> &m;
        ~drop_marks() {
            for (hipEvent_t ev : m) (void)hipEventDestroy(ev);
        }
    } drop{marks};
    hipStream_t st = gc.st;
    const uint32_t S = (uint32_t)g->idx.size(), steps_n = evaluate ? 1u : max_steps;
    const size_t per = std::min(Q, sample_walk_slice_seeds(c.max_rows, SAMPLE_WALK_BUDGET));
    const size_t cells = per * (size_t)steps_n;
    const size_t a_text = al256(N + 1), a_off = al256((Q + 1) * 8), a_keys = al256((size_t)c.d.C * 8), a_bits = al256(c.bits.size() * 4),
                 a_work = al256(SAMPLE_WALK_WORK * TALLY_WORK_STRIDE * 8), a_ext = evaluate ? 0 : al256(cells), a_steps = evaluate ? 0 : al256(per * 4),
                 a_stop = evaluate ? 0 : al256(per), a_sup = !evaluate && support ? al256(cells * 4) : 0, a_last = !evaluate && last ? al256(per * 32) : 0,
                 a_raw = evaluate ? al256(per * 64) : 0, a_m8 = evaluate ? al256(per * 64) : 0, a_wide = evaluate ? al256(per) : 0;
    hipError_t e = g->scratch.take(a_text + a_off + a_keys + a_bits + a_work + a_ext + a_steps + a_stop + a_sup + a_last + a_raw + a_m8 + a_wide +
                                       sample_walk_bytes(per, S, steps_n, c.max_rows),
                                   st, &gc.lb);
    if (e != hipSuccess)
        return fail(RSBWT_ENOMEM, "%zu seeds x %llu rows do not fit the device's free memory: %s", per, (unsigned long long)c.max_rows, hipGetErrorString(e));
    uint8_t *d_text = (uint8_t *)gc.lb.p, *d_off = d_text + a_text, *d_keys = d_off + a_off, *d_bits = d_keys + a_keys, *d_work = d_bits + a_bits,
            *d_ext = d_work + a_work, *d_steps = d_ext + a_ext, *d_stop = d_steps + a_steps, *d_sup = d_stop + a_stop, *d_last = d_sup + a_sup,
            *d_raw = d_last + a_last, *d_m8 = d_raw + a_raw, *d_wide = d_m8 + a_m8, *d_scratch = d_wide + a_wide;
    if (N) HIP_OK(hipMemcpyAsync(d_text, t0, N, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(d_off, rel, (Q + 1) * 8, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(d_keys, c.d.keys.data(), (size_t)c.d.C * 8, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(d_bits, c.bits.data(), c.bits.size() * 4, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemsetAsync(d_work, 0, a_work, st));
    const walk_batch bt = {(const char *)d_text, (const uint64_t *)d_off, Q, N, ctx, steps_n, m, flags};
    std::vector<unsigned long long> hwork(SAMPLE_WALK_WORK * TALLY_WORK_STRIDE);
    for (size_t q0 = 0; q0 < Q; q0 += per) {
        const size_t mq = std::min(per, Q - q0);
        sample_walk_args a = sample_walk_slice(g, bt, q0, mq, d_keys, d_bits, c.d, c.max_rows, c.max_locate_steps, d_work);
        a.ext = d_ext;
        a.steps = d_steps;
        a.stop = d_stop;
        a.support = a_sup ? d_sup : nullptr;
        a.last = a_last ? d_last : nullptr;
        a.evaluate_only = evaluate ? 1u : 0u;
        a.raw = d_raw;
        a.matches8 = d_m8;
        a.wide = d_wide;
        a.marks = ms ? &marks : nullptr;
        if ((e = sample_walk_enqueue(g->scratch, a, d_scratch, st)) != hipSuccess) return fail_hip(e, "sample walk launches");
        if (evaluate) {
            HIP_OK(hipMemcpyAsync(raw + q0 * 8, d_raw, mq * 64, hipMemcpyDeviceToHost, st));
            HIP_OK(hipMemcpyAsync(m8 + q0 * 8, d_m8, mq * 64, hipMemcpyDeviceToHost, st));
            HIP_OK(hipMemcpyAsync(wide + q0, d_wide, mq, hipMemcpyDeviceToHost, st));
        } else {
            HIP_OK(hipMemcpyAsync(ext + q0 * (size_t)max_steps, d_ext, mq * (size_t)max_steps, hipMemcpyDeviceToHost, st));
            HIP_OK(hipMemcpyAsync(steps + q0, d_steps, mq * 4, hipMemcpyDeviceToHost, st));
            HIP_OK(hipMemcpyAsync(stop + q0, d_stop, mq, hipMemcpyDeviceToHost, st));
            if (support) HIP_OK(hipMemcpyAsync(support + q0 * (size_t)max_steps, d_sup, mq * (size_t)max_steps * 4, hipMemcpyDeviceToHost, st));
            if (last) HIP_OK(hipMemcpyAsync(last + q0 * 4, d_last, mq * 32, hipMemcpyDeviceToHost, st));
        }
        HIP_OK(hipMemcpyAsync(hwork.data(), d_work, hwork.size() * 8, hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        if (ms) sample_walk_read_marks(marks, ms);
        if (hwork[(size_t)SW_WORK_LOST * TALLY_WORK_STRIDE] != 0)
            return fail(RSBWT_EINVAL, "%llu rows whose walk to their read's start does not end within max_locate_steps (a corrupt index, or a read longer than the limit)",
                        (unsigned long long)hwork[(size_t)SW_WORK_LOST * TALLY_WORK_STRIDE]);
    }
    sample_walk_add_work(work10, hwork.data());
    return RSBWT_OK;
}

// One evaluation of every seed over every device group: the groups' masked sums and rows added on the host, WIDE decided
// over the whole set's rows, the strands added.  msup u64[Q][4], wide u8[Q], matches u64[Q][4] (optional).
int extension_samples_groups(rsbwt_set_t *s, const char *t0, const uint64_t *rel, size_t Q, size_t N, uint32_t ctx, uint32_t flags,
                             const sample_walk_call &c, uint64_t *msup, uint8_t *wide, uint64_t *matches, uint64_t *work10) {
    struct group_out {
        std::vector<int64_t> raw;
        std::vector<uint64_t> m8;
        std::vector<uint8_t> wide;
        uint64_t work[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    };
    std::vector<group_out> outs(s->groups.size());
    int rc = for_each_group(s, [&](size_t gi) -> int {
        group_out &o = outs[gi];
        o.raw.assign(Q * 8, 0);
        o.m8.assign(Q * 8, 0);
        o.wide.assign(Q, 0);
        group_call gc(s->groups[gi], true);
        if (gc.rc) return gc.rc;
        return sample_walk_group(gc.g, gc, t0, rel, Q, N, ctx, 1ull, 1u, flags, c, true, nullptr, nullptr, nullptr, nullptr, nullptr, o.raw.data(),
                                 o.m8.data(), o.wide.data(), o.work);
    });
    if (rc) return rc;
    for (const group_out &o : outs)
        for (int i = 1; i < 10; ++i) work10[i] += o.work[i];
    for (size_t q = 0; q < Q; ++q) {
        uint64_t m8[8];
        int64_t raw[8];
        for (uint32_t l = 0; l < 8u; ++l) {
            m8[l] = 0;
            raw[l] = 0;
            for (const group_out &o : outs) {
                m8[l] += o.m8[q * 8 + l];
                raw[l] += o.raw[q * 8 + l];
            }
        }
        const bool w = sample_walk_wide(m8, c.max_rows);
        wide[q] = w ? 1u : 0u;
        for (uint32_t b = 0; b < 4u; ++b) {
            msup[q * 4 + b] = w ? 0ull : sample_walk_support(raw[2 * b], raw[2 * b + 1]);
            if (matches) matches[q * 4 + b] = m8[2 * b] + m8[2 * b + 1];
        }
    }
    return RSBWT_OK;
}

int sample_walk_flags_ok(uint32_t ctx, uint32_t flags, const uint32_t *max_steps, size_t Q) {
    // (the walk's own checks, with the one flag a sample walk adds)
    if (flags & ~(uint32_t)(RSBWT_WALK_LEFT | RSBWT_WALK_BOTH_STRANDS | RSBWT_WALK_SAMPLE_COPIES)) return fail(RSBWT_EINVAL, "unknown flag bits 0x%x", flags);
    return walk_check_args(ctx, flags & ~(uint32_t)RSBWT_WALK_SAMPLE_COPIES, max_steps, Q);
}

// ---- the set side of graph_steps.h ----
// The evaluator of a set over several device groups: the contexts go back to back into one batch, every group evaluates it
// in every shard it holds, and the host adds.  c null: the reads' own counts (extension_groups), summed over the shards;
// else the masked supports of a sample walk and its wide marks (extension_samples_groups: summed there).  work: the call's.
struct set_evaluator {
    rsbwt_set_t *s;
    uint32_t ctx, flags;  // (flags: the call's; the direction is each evaluation's own)
    const sample_walk_call *c;
    uint64_t *work;
    std::string t;
    std::vector<uint64_t> rel, counts;

    int operator()(const std::vector<std::string> &ctxs, bool left, uint64_t *sums, uint8_t *wide) {
        const size_t n = ctxs.size(), S = s->shards.size();
        if ((uint64_t)n * ctx >= (1ull << 31)) return fail(RSBWT_ERANGE, "%zu contexts x %u symbols: under 2^31 in one call", n, ctx);
        t.clear();
        rel.resize(n + 1);
        for (size_t i = 0; i < n; ++i) {
            rel[i] = (uint64_t)i * ctx;
            t += ctxs[i];
        }
        rel[n] = (uint64_t)n * ctx;
        const uint32_t f = (flags & ~(uint32_t)RSBWT_WALK_LEFT) | (left ? (uint32_t)RSBWT_WALK_LEFT : 0u);
        if (c) return extension_samples_groups(s, t.data(), rel.data(), n, (size_t)rel[n], ctx, f, *c, sums, wide, nullptr, work);
        counts.assign(S * n * 4, 0);
        const int rc = extension_groups(s, t.data(), rel.data(), n, (size_t)rel[n], ctx, f, counts.data(), work);
        if (rc) return rc;
        for (size_t p = 0; p < S; ++p)
            for (size_t i = 0; i < n * 4; ++i) sums[i] += counts[p * n * 4 + i];
        return RSBWT_OK;
    }
};

// ---- what the host forms share ----
struct graph_batch {
    std::vector<uint64_t> rel;  // the seeds' offsets from off[0]
    size_t N = 0;               // their symbols
    const char *t0 = nullptr;   // ... and where they begin
};
inline uint64_t at_least_one(uint64_t min_count) { return min_count ? min_count : 1ull; }

// A host form from its first check to its last-work block: the block cleared (publish(nullptr)), the set, the call's own
// arguments (check), the batch, nothing to do for no seeds, the outputs the call cannot do without -- then run(batch, work)
// with work[0] = Q, and the block written where all went well.
template <size_t W, class Check, class Run>
int graph_host_call(rsbwt_set_t *s, const char *text, const uint64_t *off, size_t Q, void (*publish)(const uint64_t *), Check &&check,
                    bool have_outputs, Run &&run) {
    publish(nullptr);
    int rc = walk_set_check(s);
    if (rc) return rc;
    if ((rc = check()) != RSBWT_OK) return rc;
    graph_batch b;
    if ((rc = match_check_batch(text, off, Q, &b.rel, &b.N)) != RSBWT_OK) return rc;
    if (Q == 0) return RSBWT_OK;
    if (!have_outputs) return fail(RSBWT_EINVAL, "null argument");
    b.t0 = b.N ? text + off[0] : nullptr;
    uint64_t work[W] = {Q};
    if ((rc = run(b, work)) != RSBWT_OK) return rc;
    publish(work);
    return RSBWT_OK;
}

// A set on one device group: the whole call is one(the group's call context); else by_steps(), graph_steps.h's loop.
template <class One, class Steps>
int one_group_or_steps(rsbwt_set_t *s, bool with_leases, One &&one, Steps &&by_steps) {
    if (s->groups.size() != 1) return by_steps();
    group_call gc(s->groups[0], with_leases);
    if (gc.rc) return gc.rc;
    return one(gc);
}

// ---- what the device-resident forms share ----
// The one device group, the call's own arguments (check: everything it refuses before it looks at Q), nothing more for no
// seeds (the caller tests Q too), the buffers it cannot do without, the targets (paths; else targets_ok = true, TN = 0), the
// range, the shards -- then the batch.
template <class Check>
int graph_dev_begin(rsbwt_set_t *s, Check &&check, const void *d_text, const void *d_off, size_t Q, size_t N, size_t TN, bool have_outputs,
                    bool targets_ok, uint32_t ctx, uint64_t min_count, uint32_t max_steps, uint32_t flags, dev_group **g, walk_batch *bt) {
    int rc = one_device_group(s, g);
    if (rc) return rc;
    if ((rc = check()) != RSBWT_OK || Q == 0) return rc;
    if (!d_text || !d_off || !have_outputs) return fail(RSBWT_EINVAL, "null argument");
    if (!targets_ok) return fail(RSBWT_EINVAL, "targets: d_ttext and d_toff come together or not at all");
    if (N >= (1ull << 31) || TN >= (1ull << 31)) return fail(RSBWT_ERANGE, "%zu positions in one call: at most 2^31 - 1", N > TN ? N : TN);
    for (rsbwt_t *h : s->shards)
        if (h->view.n == 0) return fail(RSBWT_EINVAL, "empty index in the set");
    *bt = {(const char *)d_text, (const uint64_t *)d_off, Q, N, ctx, max_steps, at_least_one(min_count), flags};
    return RSBWT_OK;
}

// rsbwt_set_walk_dev and rsbwt_set_unitigs_dev: launch = launch_walk or launch_unitigs
template <class Check, class Launch>
int walk_dev_call(rsbwt_set_t *s, Check &&check, Launch &&launch, const char *what, const void *d_text, const void *d_off, size_t Q, size_t N,
                  uint32_t ctx, uint64_t min_count, uint32_t max_steps, uint32_t flags, void *d_ext, void *d_steps, void *d_stop, void *d_support,
                  void *d_last, void *stream) {
    dev_group *g = nullptr;
    walk_batch bt;
    const int rc = graph_dev_begin(s, check, d_text, d_off, Q, N, 0, d_ext && d_steps && d_stop, true, ctx, min_count, max_steps, flags, &g, &bt);
    if (rc || Q == 0) return rc;
    const hipError_t e = launch(g->d_views, (uint32_t)g->idx.size(), bt, d_ext, d_steps, d_stop, d_support, d_last, nullptr, (hipStream_t)stream);
    return e == hipSuccess ? RSBWT_OK : fail_hip(e, what);
}
}  // namespace

extern "C" {

int rsbwt_set_extensions(rsbwt_set_t *s, const char *text, const uint64_t *off, size_t Q, uint32_t ctx, uint32_t flags, uint64_t *counts) {
    return guarded("rsbwt_set_extensions", [&]() -> int {
        return graph_host_call<6>(
            s, text, off, Q, walk_set_last_work, [&] { return walk_check_args(ctx, flags, nullptr, Q); }, counts != nullptr,
            [&](const graph_batch &b, uint64_t *work6) { return extension_groups(s, b.t0, b.rel.data(), Q, b.N, ctx, flags, counts, work6); });
    });
}

int rsbwt_set_walk(rsbwt_set_t *s, const char *text, const uint64_t *off, size_t Q, uint32_t ctx, uint64_t min_count, uint32_t max_steps,
                   uint32_t flags, char *ext, uint32_t *steps, uint8_t *stop, uint32_t *support, uint64_t *last) {
    return guarded("rsbwt_set_walk", [&]() -> int {
        return graph_host_call<6>(
            s, text, off, Q, walk_set_last_work, [&] { return walk_check_args(ctx, flags, &max_steps, Q); }, ext && steps && stop,
            [&](const graph_batch &b, uint64_t *work6) {
                const uint64_t m = at_least_one(min_count);
                return one_group_or_steps(
                    s, false,
                    [&](group_call &gc) {  // the whole walk in one launch
                        return walk_host_views(gc.g->scratch, gc.st, gc.g->d_views, (uint32_t)gc.g->idx.size(), b.t0, b.rel.data(), Q, b.N, ctx, m,
                                               max_steps, flags, ext, steps, stop, support, last, work6);
                    },
                    [&] {
                        return walk_steps(set_evaluator{s, ctx, flags, nullptr, work6}, b.t0, b.rel.data(), Q, ctx, m, max_steps,
                                          (flags & RSBWT_WALK_LEFT) != 0u, ext, steps, stop, support, last, work6);
                    });
            });
    });
}

int rsbwt_set_walk_dev(rsbwt_set_t *s, const void *d_text, const void *d_off, size_t Q, size_t N, uint32_t ctx, uint64_t min_count,
                       uint32_t max_steps, uint32_t flags, void *d_ext, void *d_steps, void *d_stop, void *d_support, void *d_last,
                       void *stream) {
    return walk_dev_call(s, [&] { return walk_check_args(ctx, flags, &max_steps, Q); }, launch_walk, "walk kernel launch", d_text, d_off, Q, N, ctx,
                         min_count, max_steps, flags, d_ext, d_steps, d_stop, d_support, d_last, stream);
}

void rsbwt_set_walk_last_work(uint64_t *work6) {
    if (work6) walk_get_last_work(work6);
}

int rsbwt_set_unitigs(rsbwt_set_t *s, const char *text, const uint64_t *off, size_t Q, uint32_t ctx, uint64_t min_count, uint32_t max_steps,
                      uint32_t flags, char *ext, uint32_t *steps, uint8_t *stop, uint32_t *support, uint64_t *last) {
    return guarded("rsbwt_set_unitigs", [&]() -> int {
        return graph_host_call<8>(
            s, text, off, Q, unitig_set_last_work, [&] { return unitig_check_args(ctx, flags, max_steps, Q); }, ext && steps && stop,
            [&](const graph_batch &b, uint64_t *work8) {
                const uint64_t m = at_least_one(min_count);
                return one_group_or_steps(
                    s, false,
                    [&](group_call &gc) {  // both sides of every seed in one launch
                        return unitig_host_views(gc.g->scratch, gc.st, gc.g->d_views, (uint32_t)gc.g->idx.size(), b.t0, b.rel.data(), Q, b.N, ctx, m,
                                                 max_steps, flags, ext, steps, stop, support, last, work8);
                    },
                    [&] {
                        return unitig_steps(set_evaluator{s, ctx, flags, nullptr, work8}, b.t0, b.rel.data(), Q, ctx, m, max_steps, ext, steps, stop,
                                            support, last, work8);
                    });
            });
    });
}

int rsbwt_set_unitigs_dev(rsbwt_set_t *s, const void *d_text, const void *d_off, size_t Q, size_t N, uint32_t ctx, uint64_t min_count,
                          uint32_t max_steps, uint32_t flags, void *d_ext, void *d_steps, void *d_stop, void *d_support, void *d_last,
                          void *stream) {
    return walk_dev_call(s, [&] { return unitig_check_args(ctx, flags, max_steps, Q); }, launch_unitigs, "unitig kernel launch", d_text, d_off, Q, N,
                         ctx, min_count, max_steps, flags, d_ext, d_steps, d_stop, d_support, d_last, stream);
}

void rsbwt_set_unitig_last_work(uint64_t *work8) {
    if (work8) unitig_get_last_work(work8);
}

int rsbwt_set_paths(rsbwt_set_t *s, const char *text, const uint64_t *off, size_t Q, const char *ttext, const uint64_t *toff, uint32_t ctx,
                    uint64_t min_count, uint32_t max_steps, uint32_t max_paths, uint32_t max_evals, uint32_t flags, char *ext, uint32_t *steps,
                    uint8_t *stop, uint32_t *min_support, uint32_t *npaths, uint8_t *state) {
    return guarded("rsbwt_set_paths", [&]() -> int {
        return graph_host_call<8>(
            s, text, off, Q, paths_set_last_work, [&] { return paths_check_args(ctx, flags, max_steps, max_paths, max_evals, Q); },
            ext && steps && stop && npaths && state, [&](const graph_batch &b, uint64_t *work8) {
                if ((ttext == nullptr) != (toff == nullptr)) return fail(RSBWT_EINVAL, "targets: ttext and toff come together or not at all");
                std::vector<uint64_t> trel;
                size_t TN = 0;
                if (toff) {
                    const int rc = match_check_batch(ttext, toff, Q, &trel, &TN);
                    if (rc) return rc;
                    for (size_t q = 0; q < Q; ++q)
                        if (trel[q + 1] - trel[q] > ctx)
                            return fail(RSBWT_EINVAL, "target %zu: %llu symbols, at most ctx = %u", q, (unsigned long long)(trel[q + 1] - trel[q]), ctx);
                }
                const uint64_t m = at_least_one(min_count), *tr = toff ? trel.data() : nullptr;
                const char *tt0 = toff ? ttext + toff[0] : nullptr;
                return one_group_or_steps(
                    s, false,
                    [&](group_call &gc) {  // every seed's whole search in one launch
                        return paths_host_views(gc.g->scratch, gc.st, gc.g->d_views, (uint32_t)gc.g->idx.size(), b.t0, b.rel.data(), Q, b.N, tt0, tr, TN,
                                                ctx, m, max_steps, max_paths, max_evals, flags, ext, steps, stop, min_support, npaths, state, work8);
                    },
                    [&] {
                        return paths_steps(set_evaluator{s, ctx, flags, nullptr, work8}, b.t0, b.rel.data(), Q, tt0, tr, ctx, m, max_steps, max_paths,
                                           max_evals, (flags & RSBWT_WALK_LEFT) != 0u, ext, steps, stop, min_support, npaths, state, work8);
                    });
            });
    });
}

int rsbwt_set_paths_dev(rsbwt_set_t *s, const void *d_text, const void *d_off, size_t Q, size_t N, const void *d_ttext, const void *d_toff,
                        size_t TN, uint32_t ctx, uint64_t min_count, uint32_t max_steps, uint32_t max_paths, uint32_t max_evals, uint32_t flags,
                        void *d_ext, void *d_steps, void *d_stop, void *d_min_support, void *d_npaths, void *d_state, void *stream) {
    dev_group *g = nullptr;
    paths_batch pb;
    const int rc = graph_dev_begin(
        s, [&] { return paths_check_args(ctx, flags, max_steps, max_paths, max_evals, Q); }, d_text, d_off, Q, N, TN,
        d_ext && d_steps && d_stop && d_npaths && d_state, (d_ttext == nullptr) == (d_toff == nullptr), ctx, min_count, max_steps, flags, &g, &pb.seeds);
    if (rc || Q == 0) return rc;
    pb.ttext = (const char *)d_ttext;
    pb.toff = (const uint64_t *)d_toff;
    pb.TN = d_toff ? TN : 0;
    pb.max_paths = max_paths;
    pb.max_evals = max_evals;
    // the frame store: leased for the launch and handed back in stream order, so nothing is waited for
    scratch_cache::lease mem;
    hipError_t e = g->scratch.take(paths_frame_bytes(Q, max_steps, max_evals) + 256, (hipStream_t)stream, &mem);
    if (e != hipSuccess) return fail(RSBWT_ENOMEM, "the frame store of %zu seeds does not fit the device's free memory: %s", Q, hipGetErrorString(e));
    e = launch_paths(g->d_views, (uint32_t)g->idx.size(), pb, mem.p, d_ext, d_steps, d_stop, d_min_support, d_npaths, d_state, nullptr,
                     (hipStream_t)stream);
    g->scratch.give(mem, (hipStream_t)stream);
    return e == hipSuccess ? RSBWT_OK : fail_hip(e, "paths kernel launch");
}

void rsbwt_set_paths_last_work(uint64_t *work8) {
    if (work8) paths_get_last_work(work8);
}

int rsbwt_set_extension_samples(rsbwt_set_t *s, const char *text, const uint64_t *off, size_t Q, uint32_t ctx, uint32_t flags, const uint8_t *codes,
                                size_t C, uint32_t size_of_sample, int has_other_meta_data, const uint8_t *mask, uint64_t max_rows,
                                uint32_t max_locate_steps, uint64_t *msup, uint8_t *wide, uint64_t *matches) {
    return guarded("rsbwt_set_extension_samples", [&]() -> int {
        sample_walk_call c;
        return graph_host_call<10>(
            s, text, off, Q, sample_walk_set_last_work,
            [&] {
                const int rc = sample_walk_flags_ok(ctx, flags, nullptr, Q);
                return rc ? rc : sample_walk_prepare(s, codes, C, size_of_sample, has_other_meta_data, mask, max_rows, max_locate_steps, &c);
            },
            msup && wide, [&](const graph_batch &b, uint64_t *work10) {
                return extension_samples_groups(s, b.t0, b.rel.data(), Q, b.N, ctx, flags, c, msup, wide, matches, work10);
            });
    });
}

int rsbwt_set_walk_samples(rsbwt_set_t *s, const char *text, const uint64_t *off, size_t Q, uint32_t ctx, uint64_t min_count, uint32_t max_steps,
                           uint32_t flags, const uint8_t *codes, size_t C, uint32_t size_of_sample, int has_other_meta_data, const uint8_t *mask,
                           uint64_t max_rows, uint32_t max_locate_steps, char *ext, uint32_t *steps, uint8_t *stop, uint32_t *support,
                           uint64_t *last) {
    return guarded("rsbwt_set_walk_samples", [&]() -> int {
        for (double &t : sample_walk_ms) t = 0;
        sample_walk_call c;
        return graph_host_call<10>(
            s, text, off, Q, sample_walk_set_last_work,
            [&] {
                const int rc = sample_walk_flags_ok(ctx, flags, &max_steps, Q);
                return rc ? rc : sample_walk_prepare(s, codes, C, size_of_sample, has_other_meta_data, mask, max_rows, max_locate_steps, &c);
            },
            ext && steps && stop, [&](const graph_batch &b, uint64_t *work10) {
                const uint64_t m = at_least_one(min_count);
                return one_group_or_steps(
                    s, true,
                    [&](group_call &gc) {  // the whole walk enqueued at once, slice by slice
                        return sample_walk_group(gc.g, gc, b.t0, b.rel.data(), Q, b.N, ctx, m, max_steps, flags, c, false, ext, steps, stop, support, last,
                                                 nullptr, nullptr, nullptr, work10, sample_walk_times_on() ? sample_walk_ms : nullptr);
                    },
                    [&] {
                        return walk_steps(set_evaluator{s, ctx, flags, &c, work10}, b.t0, b.rel.data(), Q, ctx, m, max_steps,
                                          (flags & RSBWT_WALK_LEFT) != 0u, ext, steps, stop, support, last, work10);
                    });
            });
    });
}

// one-device set, the caller's buffers and stream, nothing synchronised
int rsbwt_set_walk_samples_dev(rsbwt_set_t *s, const void *d_text, const void *d_off, size_t Q, size_t N, uint32_t ctx, uint64_t min_count,
                               uint32_t max_steps, uint32_t flags, const void *d_keys, size_t C, uint32_t size_of_sample, int has_other_meta_data,
                               const void *d_mask, uint64_t max_rows, uint32_t max_locate_steps, void *d_ext, void *d_steps, void *d_stop,
                               void *d_support, void *d_last, void *d_status8, void *stream) {
    return guarded("rsbwt_set_walk_samples_dev", [&]() -> int {
        dev_group *g = nullptr;
        walk_batch bt;
        int rc = graph_dev_begin(
            s,
            [&] {
                int ok = sample_walk_flags_ok(ctx, flags, &max_steps, Q);
                if (ok == RSBWT_OK) ok = sample_set_ok(s);
                if (ok == RSBWT_OK) ok = sample_shape_ok(C, size_of_sample);
                if (ok == RSBWT_OK) ok = sample_walk_shape_ok(s, max_rows);
                return ok != RSBWT_OK ? ok : !d_keys || !d_mask || !d_status8 ? fail(RSBWT_EINVAL, "null argument") : RSBWT_OK;
            },
            d_text, d_off, Q, N, 0, d_ext && d_steps && d_stop, true, ctx, min_count, max_steps, flags, &g, &bt);
        if (rc) return rc;
        hipStream_t st = (hipStream_t)stream;
        if (Q == 0) {
            HIP_OK(hipMemsetAsync(d_status8, 0, 64, st));
            return RSBWT_OK;
        }
        sample_dict dict;
        dict.C = (uint32_t)C;
        dict.size_of_sample = size_of_sample;
        dict.has_other = has_other_meta_data ? 1u : 0u;
        const uint32_t S = (uint32_t)g->idx.size();
        const size_t per = std::min(Q, sample_walk_slice_seeds(max_rows, SAMPLE_WALK_BUDGET));
        const size_t a_bits = al256(sample_walk_mask_words(C) * 4), a_work = al256(SAMPLE_WALK_WORK * TALLY_WORK_STRIDE * 8);
        scratch_cache::lease mem;
        hipError_t e = g->scratch.take(a_bits + a_work + sample_walk_bytes(per, S, max_steps, max_rows), st, &mem);
        if (e != hipSuccess) return fail_hip(e, "scratch for a sample walk");
        uint8_t *d_bits = (uint8_t *)mem.p, *d_work = d_bits + a_bits, *d_scratch = d_work + a_work;
        rc = [&]() -> int {
            if ((e = launch_sample_walk_mask(d_mask, C, d_bits, st)) != hipSuccess) return fail_hip(e, "mask kernel launch");
            HIP_OK(hipMemsetAsync(d_work, 0, a_work, st));
            for (size_t q0 = 0; q0 < Q; q0 += per) {  // (the slices share the scratch: stream order keeps them apart)
                sample_walk_args a = sample_walk_slice(g, bt, q0, std::min(per, Q - q0), d_keys, d_bits, dict, max_rows, max_locate_steps, d_work);
                a.ext = (char *)d_ext + q0 * (size_t)max_steps;
                a.steps = (uint32_t *)d_steps + q0;
                a.stop = (uint8_t *)d_stop + q0;
                a.support = d_support ? (uint32_t *)d_support + q0 * (size_t)max_steps : nullptr;
                a.last = d_last ? (uint64_t *)d_last + q0 * 4 : nullptr;
                if ((e = sample_walk_enqueue(g->scratch, a, d_scratch, st)) != hipSuccess) return fail_hip(e, "sample walk launches");
            }
            if ((e = launch_sample_walk_status((const unsigned long long *)d_work, d_status8, st)) != hipSuccess) return fail_hip(e, "status kernel launch");
            return RSBWT_OK;
        }();
        g->scratch.give(mem, st);
        return rc;
    });
}

void rsbwt_set_walk_samples_last_work(uint64_t *work10) {
    if (work10) memcpy(work10, sample_walk_last, sizeof sample_walk_last);
}

void rsbwt_set_walk_samples_last_times(double *ms7) {
    if (ms7) memcpy(ms7, sample_walk_ms, sizeof sample_walk_ms);
}

}  // extern "C"
