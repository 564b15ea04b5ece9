// capi_internal.h -- what the C-ABI translation units (capi.hip, sets.hip, set_graph.hip) share: the handle
// structs behind include/rsbwt.h's opaque types, per-call contexts, and the search launcher.
#ifndef RSBWT_CAPI_INTERNAL_H
#define RSBWT_CAPI_INTERNAL_H

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <atomic>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <vector>

#include "../../include/rsbwt.h"
#include "ctx_pool.h"
#include "kernels.h"
#include "line_format.h"

namespace rsb {

int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
int fail_hip(hipError_t e, const char *what);
int use_device(int device);
int resolve_device(int logical, int *physical);  // the device number of an rsbwt_open* call -> the GPU it names (capi.hip)

// A stream pair and a staging buffer for the duration of one host-buffer call.
struct call_ctx {
    hipStream_t st[2] = {nullptr, nullptr};
    void *d_stage = nullptr;
    size_t stage_bytes = 0;
    int stage(size_t bytes);  // grows the staging buffer; RSBWT_OK or RSBWT_ENOMEM
    // a small page-locked host buffer: the k-mers and answers of a SMALL call travel through it (a copy to
    // or from pageable memory costs the runtime a staging step and a wait of its own, three of them are
    // half of a lone request's latency); nullptr when it could not be had -- the call then goes the
    // ordinary way
    static constexpr size_t PIN_BYTES = 256u << 10;
    void *h_pin = nullptr;
};

// (the waiting logic: ctx_pool.h; 8 = the threads of the reference's query pool, service.cpp:88)
struct ctx_pool : bounded_pool<call_ctx, 8> {
    static constexpr int MAX_CTX = 8;
    call_ctx *acquire();  // blocks while MAX_CTX calls are in flight; nullptr = no stream could be made
    void destroy();       // with no call in flight
};

// HIP-event pairs of the most recent search launches + the counting mode's counters
struct search_meter {
    static constexpr int RING = 64;
    hipEvent_t ev_start[RING] = {}, ev_stop[RING] = {};
    uint64_t launches = 0;  // search launches so far; launch i uses pair i % RING
    bool counting = false;
    unsigned long long *d_work = nullptr;  // WORK_WORDS counters (search_lines.hip)
    scratch_cache scratch;                 // start records / row counters of the launches in flight
    std::mutex mu;
};

int search_launch(search_meter &m, const shard_view *d_views, uint32_t nshards, int num_cus, const void *d_packed,
                  const void *d_valid, size_t Q, uint32_t k, void *d_lower, void *d_upper, bool counts_only,
                  hipStream_t stream, const search_extra *extra);
int search_host_views(search_meter &m, ctx_pool &pool, const shard_view *d_views, uint32_t nshards, int num_cus,
                      const char *kmers, size_t Q, uint32_t k, size_t stride, uint64_t *lower, uint64_t *upper,
                      bool counts_only, bool narrow = false);
int search_host_views_var(search_meter &m, ctx_pool &pool, const shard_view *d_views, uint32_t nshards, int num_cus,
                          const char *text, const uint64_t *off, size_t Q, uint64_t *lower, uint64_t *upper, bool counts_only,
                          bool narrow = false);
inline uint32_t words_per_kmer(uint32_t k) { return k ? (k + 31u) / 32u : 1u; }
inline size_t al256(size_t b) { return (b + 255) & ~(size_t)255; }
// THE loop over a host batch of queries of lengths of their own (query q = text[off[q] .. off[q+1])), for every call
// that takes one (capi.hip).  The batch goes up in slices of 65,536 queries on `st`; per slice the loop refuses an
// off[] that runs backwards, sizes the slice by its longest query of at most 65,535 symbols (k), lays text, relative
// offsets, packed words, valid bytes and lengths out in c's staging buffer, each part 256-aligned, uploads, packs
// (launch_pack_var), hands the slice to run() and synchronises `st` before the staging buffer is used again.
//   extra_bytes(mq)  what the call wants behind d_len for a slice of mq queries: d_extra
//   empty(q0, mq)    the answers of a slice with nothing to search (k would be 0): nothing is uploaded or launched
//   run(slice)       the call's launches and copies back, enqueued on `st`
struct var_slice {
    size_t q0, mq;    // queries q0 .. q0 + mq of the batch
    uint32_t k, wpq;  // the longest query's symbols; packed words per query
    uint8_t *d_pk, *d_ok, *d_len, *d_extra;
};
int for_each_var_slice(call_ctx &c, hipStream_t st, const char *text, const uint64_t *off, size_t Q,
                       const std::function<size_t(size_t)> &extra_bytes, const std::function<int(size_t, size_t)> &empty,
                       const std::function<int(const var_slice &)> &run);
// search_extra::narrow for a launch on this shard: a T-mer's interval is ~ n / 4^T rows wide;
// a quarter of a window or less = the steps after the table find both positions in one line
inline bool view_is_narrow(const shard_view &v, uint32_t k) {
    return v.ktab && v.ktab_depth >= 2u && k >= v.ktab_depth && ((v.n >> (2u * v.ktab_depth)) << 2) <= v.sp.S;
}
// the worklist launch of a set's 1-mismatch search (kernels.h), metered like search_launch; the counters ACCUMULATE
// onto what the traced launch and the branch kernel left
int search_launch_worklist(search_meter &m, const shard_view *d_views, uint32_t nshards, int num_cus, const void *d_packed,
                           const void *d_valid, size_t nkmers, uint32_t tn, const void *d_worklists, const void *d_counts, size_t wl_cap,
                           uint32_t k, void *d_sparse, void *d_hit_bits, hipStream_t stream, const void *d_pre = nullptr);
// the walk that makes those worklists (kernels.h, launch_search_walk), metered like search_launch: a counting launch
// ZEROES the counters first (it is the first launch of the sequence)
int search_launch_walk(search_meter &m, const shard_view *d_views, uint32_t nshards, int num_cus, const void *d_packed,
                       const void *d_valid, size_t nkmers, uint32_t tn, void *d_worklists, void *d_counts, size_t wl_cap, uint32_t k,
                       void *d_sparse, void *d_hit_bits, hipStream_t stream);
int meter_history_ms(search_meter &m, float *ms, size_t cap, size_t *count);
// Whole-read matches by backward search from the terminator rows (read_lookup.hip): start records, the search launch,
// the '$' count -- copies / ending / ordinal [nshards][Q] (ending and ordinal may be null).  d_len: the queries' own lengths (u32[Q]), or
// nullptr when every query has k symbols; d_scratch: read_copies_scratch_bytes(nshards, Q) bytes the launches may use.
inline size_t read_copies_scratch_bytes(uint32_t nshards, size_t Q) { return (size_t)nshards * Q * 32; }
int read_copies_launch(search_meter &m, const shard_view *d_views, uint32_t nshards, int num_cus, const void *d_packed,
                       const void *d_valid, const void *d_len, size_t Q, uint32_t k, void *d_scratch, void *d_copies, void *d_ending,
                       hipStream_t stream, void *d_ordinal = nullptr);
int read_copies_host_views(search_meter &m, ctx_pool &pool, const shard_view *d_views, uint32_t nshards, int num_cus,
                           const char *kmers, size_t Q, uint32_t k, size_t stride, uint64_t *copies, uint64_t *ending);
int read_copies_host_views_var(search_meter &m, ctx_pool &pool, const shard_view *d_views, uint32_t nshards, int num_cus,
                               const char *text, const uint64_t *off, size_t Q, uint64_t *copies, uint64_t *ending,
                               uint64_t *ordinal = nullptr, uint64_t *lf_steps = nullptr);
// locate.hip: rows in host memory located through c's staging buffer (shard_of null: the one shard of d_views), the
// answers into the caller's arrays (each optional), work2[0..1] += {rows ended on '$', LF steps}; and what
// rsbwt_locate_last_work reports for the calling thread
int locate_host_views(scratch_cache &scratch, call_ctx &c, const shard_view *d_views, uint32_t nshards, int num_cus, const uint32_t *shard_of,
                      const uint64_t *rows, size_t n, uint32_t max_steps, uint64_t *read_row, uint64_t *ordinal, uint32_t *offset,
                      uint64_t *work2);
void locate_set_last_work(uint64_t walked, uint64_t steps);
// match_stats.hip: what the host-buffer matching-statistics calls share (capi.hip: one handle; sets.hip: a set).
//   match_check_batch  off[] ascending, no query over 2^31 - 1 symbols, under 2^31 positions: rel = offsets from off[0], *N
//   match_host_views   one device's share on `st` (synchronised before it returns): len u32[S][N], pairs {lower, upper}[S][N],
//                      smems (shard = d_views' number, unordered), each optional; work4 += the launch's counters
//   match_set / get_last_work: what rsbwt_set_match_last_work reports for the calling thread
int match_check_batch(const char *text, const uint64_t *off, size_t Q, std::vector<uint64_t> *rel, size_t *N);
int match_host_views(scratch_cache &scratch, hipStream_t st, const shard_view *d_views, uint32_t S, const char *t0, const uint64_t *rel, size_t Q,
                     size_t N, uint32_t cap, uint64_t m, uint32_t *len, uint64_t *pairs, std::vector<rsbwt_smem> *smems, uint64_t *work4);
void match_set_last_work(const uint64_t work6[6]);
void match_get_last_work(uint64_t work6[6]);
// overlaps.hip: what the host-buffer overlap calls share (capi.hip: one handle; sets.hip: a set); batches are checked by
// match_check_batch.
//   overlap_host_views  one device's share on `st` (synchronised before it returns): pairs {ordinal, count}[S][N] and recs
//                       (the entries with count > 0; shard = d_views' number, unordered), each optional; work5 += the
//                       launch's counters
//   overlap_set / get_last_work: what rsbwt_set_overlap_last_work reports for the calling thread
int overlap_host_views(scratch_cache &scratch, hipStream_t st, const shard_view *d_views, uint32_t S, const char *t0, const uint64_t *rel, size_t Q,
                       size_t N, uint32_t min_overlap, uint32_t max_overlap, uint64_t *pairs, std::vector<rsbwt_overlap> *recs, uint64_t *work5);
void overlap_set_last_work(const uint64_t work6[6]);
void overlap_get_last_work(uint64_t work6[6]);
// walk.hip: what the host-buffer extension and walk calls share (capi.hip: one handle; set_graph.hip: a set); batches are
// checked by match_check_batch and walk_check_args (ctx, flags and -- where max_steps is given -- max_steps and Q x max_steps).
//   extension_host_views  one device's share on `st` (synchronised before it returns): counts u64[S][Q][4]; work6[2..5] += the
//                         launch's counters
//   walk_host_views       a whole walk call on one device on `st` (synchronised before it returns): support and last are
//                         optional; work6[1..5] += the launch's counters
//   walk_set / get_last_work: what rsbwt_set_walk_last_work reports for the calling thread
int walk_check_args(uint32_t ctx, uint32_t flags, const uint32_t *max_steps, size_t Q);
int extension_host_views(scratch_cache &scratch, hipStream_t st, const shard_view *d_views, uint32_t S, const char *t0, const uint64_t *rel, size_t Q,
                         size_t N, uint32_t ctx, uint32_t flags, uint64_t *counts, uint64_t *work6);
int walk_host_views(scratch_cache &scratch, hipStream_t st, const shard_view *d_views, uint32_t S, const char *t0, const uint64_t *rel, size_t Q,
                    size_t N, uint32_t ctx, uint64_t min_count, uint32_t max_steps, uint32_t flags, char *ext, uint32_t *steps, uint8_t *stop,
                    uint32_t *support, uint64_t *last, uint64_t *work6);
void walk_set_last_work(const uint64_t work6[6]);
void walk_get_last_work(uint64_t work6[6]);
//   unitig_check_args     ctx, flags (RSBWT_WALK_BOTH_STRANDS only), max_steps and 2 x Q x max_steps
//   unitig_host_views     a whole unitig call on one device on `st` (synchronised before it returns): support and last
//                         are optional; work8[1..7] += the launch's counters
//   unitig_set / get_last_work: what rsbwt_set_unitig_last_work reports for the calling thread
int unitig_check_args(uint32_t ctx, uint32_t flags, uint32_t max_steps, size_t Q);
int unitig_host_views(scratch_cache &scratch, hipStream_t st, const shard_view *d_views, uint32_t S, const char *t0, const uint64_t *rel, size_t Q,
                      size_t N, uint32_t ctx, uint64_t min_count, uint32_t max_steps, uint32_t flags, char *ext, uint32_t *steps, uint8_t *stop,
                      uint32_t *support, uint64_t *last, uint64_t *work8);
void unitig_set_last_work(const uint64_t work8[8]);
void unitig_get_last_work(uint64_t work8[8]);
// paths.hip: what the path calls share (set_graph.hip).
//   paths_check_args      ctx, flags, max_steps, max_paths, max_evals and Q x max_paths x max_steps
//   paths_host_views      a whole paths call on one device on `st` (synchronised before it returns): trel (the targets'
//                         offsets from toff[0], TN symbols at tt0) may be null = no targets, min_support is optional;
//                         work8[1..7] += the launch's counters
//   paths_set / get_last_work: what rsbwt_set_paths_last_work reports for the calling thread
int paths_check_args(uint32_t ctx, uint32_t flags, uint32_t max_steps, uint32_t max_paths, uint32_t max_evals, size_t Q);
int paths_host_views(scratch_cache &scratch, hipStream_t st, const shard_view *d_views, uint32_t S, const char *t0, const uint64_t *rel, size_t Q,
                     size_t N, const char *tt0, const uint64_t *trel, size_t TN, uint32_t ctx, uint64_t min_count, uint32_t max_steps,
                     uint32_t max_paths, uint32_t max_evals, uint32_t flags, char *ext, uint32_t *steps, uint8_t *stop, uint32_t *min_support,
                     uint32_t *npaths, uint8_t *state, uint64_t *work8);
void paths_set_last_work(const uint64_t work8[8]);
void paths_get_last_work(uint64_t work8[8]);
// ksw_align.hip behind rsbwt_gt_align (capi.hip) and the aligned set calls (sets.hip): a host batch checked (null, item < Q,
// lengths 1..4096: RSBWT_EINVAL), ordered by length, aligned on `device` and waited for; work14 += {reads, reads by
// verdict 1..13}.  gt_align_set / get_last_work: what rsbwt_gt_align_last_work reports for the calling thread (null: zeros)
int gt_align_host(int device, const char *reads, const uint64_t *roff, const uint64_t *item, size_t n, const char *text, const uint64_t *off,
                  const uint64_t *pos, const char *alt, const uint8_t *isalt, size_t Q, uint8_t *verdict, uint64_t *work14);
void gt_align_set_last_work(const uint64_t *work14);
void gt_align_get_last_work(uint64_t *work14);
// 1-mismatch hit list of one shard from variants expanded once for the whole batch (sets.hip: every shard of a set
// searches the same variants)
size_t variants_bytes(size_t m, uint32_t k);
int variants_of_batch_dev(const void *d_packed, const void *d_valid, size_t m, uint32_t k, void *d_variants, hipStream_t stream);
int meter_work(search_meter &m, uint64_t *words, size_t nwords);

}  // namespace rsb

struct rsbwt : rsb::search_meter {
    int device = 0;          // the GPU (hipSetDevice)
    int logical_device = 0;  // the number the caller opened it with: what a shard set groups by (= device outside tests)
    int num_cus = 256;
    rsb::shard_view view;              // host copy
    rsb::shard_view *d_view = nullptr; // the same in HBM, for kernels that take views from memory
    uint64_t num_runs = 0, num_strings = 0, hbm_bytes = 0;
    uint64_t far_lines = 0, chunk_windows = 0, far_windows = 0, spilled_symbols = 0;
    rsb::ctx_pool pool;
    // What read extraction and getOccAt read: the view PLUS the sampled select table.  `view` / `d_view` -- what every
    // search reads -- are never written after the handle has been handed out (rsbwt_attach_ktab* apart: an explicit
    // step of the owner's).  A shard opened with RSBWT_OPEN_READS has its samples and psi hints before that, and
    // xview == view, d_xview == d_view.  Any other shard builds the samples on its first extraction INTO A SIDE TABLE
    // and publishes them here (x_ready, release / acquire): its lines are not touched, searches that run meanwhile
    // read what they always read.  psi hints go into such a shard's lines only by rsbwt_prepare_extraction, which the
    // owner calls before it shares the handle.
    rsb::shard_view xview;
    rsb::shard_view *d_xview = nullptr;
    std::atomic<bool> x_ready{false};
    uint64_t *d_sel = nullptr;  // sampled select table
    uint64_t psi_hint_lines = 0;  // window lines that carry a psi hint
    bool ktab_owned = true;     // false: view.ktab points into a shard set's interleaved table
    uint64_t ktab_untabulated = 0;  // grouped table: T-mers whose record leaves them to the search (empty, or a group too wide)
    std::atomic<int> exactmatch_by_search{0};  // rsbwt_exactmatch_by_search: rsbwt_query_exactmatch answers from rsbwt_read_copies
};

namespace rsb {
int hits_1mm_dev_shared(rsbwt *h, const void *d_packed, const void *d_valid, size_t m, uint32_t k, void *d_hits, size_t cap,
                        void *d_total, void *d_scratch, void *stream, const void *d_variants);
// Builds h's k-mer table of depth T into d_table[c * stride] (memory owned by the caller).
// (fmt: rsb::KTAB_PLAIN / KTAB_GROUPED; d_table = this shard's first entry / record inside an interleaved allocation)
int attach_ktab_into(rsbwt *h, uint32_t T, uint64_t *d_table, uint32_t stride, uint32_t fmt = 0);
// RSBWT_KTAB_FORMAT_* -> the format a table of depth T over n symbols gets (auto: the caller's plain / grouped choice)
uint32_t auto_ktab_depth_for(uint64_t budget, uint64_t n, uint32_t *fmt);
constexpr uint32_t KTAB_MAX_DEPTH_PLAIN = 16, KTAB_MAX_DEPTH_GROUPED = 17;
// Where the grouped records pay: a record holds a group of < 16383 rows (so: four siblings expected to hold an eighth of
// that at most), and a T-mer that does not occur is left to the search, T steps instead of none -- rare only while a
// T-mer's interval is still many runs wide (measured on the bench's 1.17e11-symbol run stream: 5.5e-5 of the 15-mers at
// 109 rows each, 0.46 of the 17-mers at 7 rows each: a context that narrow mostly has ONE preceding symbol).
inline bool ktab_grouped_sensible(uint64_t n, uint32_t T) {
    return T >= 2u && T <= 31u && (n >> (2u * (T - 1u))) <= 2048ull && (n >> (2u * T)) >= 64ull;
}
int detach_ktab(rsbwt *h);  // forgets a table it does not own
int ensure_samples(rsbwt *h, hipStream_t stream);  // the select samples of a shard (built once, into a side table): h->xview / d_xview then name them
}  // namespace rsb

#endif
