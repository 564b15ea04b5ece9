// kernels.h -- host-side launchers of every kernel of the library (the .hip files of this directory: each declaration
// names its own) and the scratch they lease.
#ifndef RSBWT_KERNELS_H
#define RSBWT_KERNELS_H

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <mutex>
#include <vector>

#include "launch_plan.h"
#include "line_format.h"

namespace rsb {

// Scratch in HBM for the duration of one launch sequence on a stream (the search's start records,
// a walk's row counters).  A few buffers are kept and handed out again: to the stream that used one
// last (stream order makes that safe at once), or to any stream once the event recorded at the last
// give() has completed.  Nothing here calls the runtime's stream-ordered allocator: on this stack a
// hipMallocAsync / hipFreeAsync pair per call stalls for seconds once in a few thousand calls
// (profiles/r02d_latency.md).
class scratch_cache {
  public:
    struct lease {
        void *p = nullptr;
        int slot = -1;
    };
    hipError_t take(size_t bytes, hipStream_t stream, lease *out);
    void give(const lease &l, hipStream_t stream);  // after the last launch that uses l.p was enqueued
    void destroy();                                 // with no launch in flight
    size_t held_bytes();

  private:
    static constexpr int SLOTS = 16;
    struct slot_t {
        void *p = nullptr;
        size_t bytes = 0;
        hipStream_t last = nullptr;
        hipEvent_t done = nullptr;
        bool recorded = false, busy = false;
    };
    slot_t slots_[SLOTS];
    std::mutex mu_;
};

// the search kernels' query pools (one counter per shard, drawn from by every wave of the launch) sit POOL_STRIDE u64
// apart, as the worklists' lengths do (WL_COUNT_STRIDE): eight adjacent counters are one line of one L2 channel, and a
// small batch -- 4,096 waves probing eight drained pools each -- then waits on that line longer than it searches (0.58
// against 0.32 ms for 4e4 31-mers x 8 shards with a quarter of the waves).  The walkers' row counters likewise: every
// wave of a small launch, and of any launch's tail, hits them with atomics.
constexpr uint32_t POOL_STRIDE = 32;

// The scratch of one persistent launch sequence on `stream`: front_bytes for the caller (a search's start records) and
// behind them npools x nshards counters POOL_STRIDE apart, zeroed.  error() says whether both steps went through; the
// lease goes back when this leaves scope -- after the sequence's last launch was enqueued, which is what give() asks.
class pool_lease {
  public:
    pool_lease(scratch_cache &scratch, hipStream_t stream, size_t front_bytes, uint32_t npools, uint32_t nshards)
        : scratch_(scratch), stream_(stream) {
        const size_t pool_bytes = (size_t)npools * nshards * POOL_STRIDE * sizeof(unsigned long long);
        err_ = scratch.take(front_bytes + pool_bytes, stream, &mem_);
        if (err_ != hipSuccess) return;
        pools_ = (unsigned long long *)((char *)mem_.p + front_bytes);
        err_ = hipMemsetAsync(pools_, 0, pool_bytes, stream);
    }
    ~pool_lease() { scratch_.give(mem_, stream_); }  // (nothing taken: slot -1, nothing given)
    pool_lease(const pool_lease &) = delete;
    pool_lease &operator=(const pool_lease &) = delete;
    hipError_t error() const { return err_; }
    void *front() const { return mem_.p; }
    unsigned long long *pool(uint32_t i, uint32_t nshards) const { return pools_ + (size_t)i * nshards * POOL_STRIDE; }

  private:
    scratch_cache &scratch_;
    hipStream_t stream_;
    scratch_cache::lease mem_;
    unsigned long long *pools_ = nullptr;
    hipError_t err_;
};

hipError_t launch_pack(const void *d_kmers, size_t Q, uint32_t k, size_t stride, void *d_packed,
                       void *d_valid, hipStream_t stream);

// words of the hit map of Q searches (one bit per search, a whole number of 16-byte units: the maps of a launch's
// shards lie back to back)
__host__ __device__ inline size_t hit_map_words(size_t Q) { return ((Q + 127) / 128) * 2; }

struct search_extra {
    // 1-mismatch search.  A traced search records, per (shard, k-mer), the interval
    // it holds when about to take each of its first trace_n symbols ([nshards][Q][trace_n] x {lower, upper});
    // the search of the k-mers' variants (`variants` per k-mer, variants_kernel's order) then starts
    // every variant whose substituted position is < trace_n from that interval (the shards of one launch
    // share trace_n: their k-mer tables have one depth).
    void *d_trace_out = nullptr;
    const void *d_trace_in = nullptr;
    uint32_t trace_n = 0, variants = 0;
    bool table_build = false;  // a k-mer table's own searches: same kernel under another name (profiles)
    bool pairs = false;        // results as {lower, upper}[nshards][Q] at d_lower (one 16-byte store per search)
    // sparse results: nothing is written for a search that ends empty; the others store
    // {lower, upper} at d_lower[s][search index] (16 B each, as with `pairs`) and set their bit in shard s's map
    // d_hit_bits[s][hit_map_words(Q)] (one bit per search, zeroed by the caller); launch_compact_hits turns the
    // two into a list per shard, ordered by search index
    void *d_hit_bits = nullptr;
    // the k-mer table leaves intervals well inside a window (n / 4^T << S): most steps of a search find
    // both positions in one line, which is what the one-lane-per-search kernel is for (search_solo.h)
    bool narrow = false;
    // start records computed ahead (launch_search_init, on any stream the caller orders before this launch):
    // [nshards][Q] x 16 B in the caller's HBM; the launch then takes no scratch and runs no start-record kernel
    const void *d_init = nullptr;
};
// the start-record kernel alone: d_init[s * Q + q] for every (query, shard) search of a batch
hipError_t launch_search_init(const shard_view *d_shards, uint32_t nshards, const void *d_packed, const void *d_valid, size_t Q,
                              uint32_t k, void *d_init, hipStream_t stream);
// queries of lengths of their own (search_lines.hip, search_init_var_kernel): the packing of `text` cut at off[0..Q] into wpq
// words per query + validity + lengths, and the start records [nshards][Q] a search launch then takes as search_extra::d_init
hipError_t launch_pack_var(const void *d_text, const void *d_off, size_t Q, uint32_t wpq, void *d_packed, void *d_valid, void *d_len,
                           hipStream_t stream);
hipError_t launch_search_init_var(const shard_view *d_shards, uint32_t nshards, const void *d_packed, const void *d_valid,
                                  const void *d_len, size_t Q, uint32_t wpq, void *d_init, hipStream_t stream);
// search_lines.hip: batched findInterval of Q packed k-mers in each of the nshards shards whose
// views are the device array d_shards (all on the current device).  d_lower/d_upper: [nshards][Q]
// (d_lower alone receives counts with counts_only).  ev0/ev1 (optional) are recorded on `stream`
// immediately around the search kernel itself.
hipError_t launch_search(scratch_cache &scratch, const shard_view *d_shards, uint32_t nshards, const void *d_packed,
                         const void *d_valid, size_t Q, uint32_t k, void *d_lower, void *d_upper, bool counts_only,
                         unsigned long long *d_work, int num_cus, hipStream_t stream, hipEvent_t ev0 = nullptr,
                         hipEvent_t ev1 = nullptr, const search_extra *extra = nullptr);
uint32_t trace_entries(const shard_view &ix, uint32_t k);
// read_lookup.hip: whole-read matches by backward search from the terminator rows.  launch_read_seed writes the start
// records [nshards][Q] of such a search (d_len: the queries' own lengths, u32[Q]; nullptr = every query has k symbols)
// for launch_search to take as search_extra::d_init; launch_dollar_count turns its {lower, upper} pairs [nshards][Q]
// into copies = Occ('$', upper) - Occ('$', lower - 1) and (d_ending, optional) upper - lower + 1, zeros for anything
// that is not a proper interval.  d_work (counting mode): words 13 results ranked, 14 positions that took a
// continuation, 15 results that needed a second line are ADDED to.
hipError_t launch_read_seed(const shard_view *d_shards, uint32_t nshards, const void *d_valid, const void *d_len, size_t Q, uint32_t k,
                            void *d_init, hipStream_t stream);
// d_ordinal (optional, u64[nshards][Q]): Occ('$', lower - 1) where copies > 0, else 0 -- the first of the dense read
// numbers (rsbwt_locate's ordinal) of the reads equal to the query; the rank is the one the count takes anyway.
hipError_t launch_dollar_count(const shard_view *d_shards, uint32_t nshards, const void *d_pairs, size_t Q, void *d_copies,
                               void *d_ending, unsigned long long *d_work, hipStream_t stream, void *d_ordinal = nullptr);
// read_meta.hip: the per-read sample table (rsbwt_set_meta_*).  A shard's table is off u64[num_strings + 1] and packed
// value bytes: the value of ordinal o is bytes[off[o] .. off[o+1]).  off == nullptr: no table.
struct meta_view {
    const uint64_t *off;
    const uint8_t *bytes;
    uint64_t num_strings;
    const uint32_t *heads;  // one bit per ordinal: the FIRST ordinal of a string some pair named (sample_counts.hip); bit o = heads[o / 32] >> (o % 32)
};
constexpr uint64_t META_NONE = ~0ull;  // src[] of an item that brings no bytes
size_t meta_scan_bytes(size_t n);      // temporary bytes of launch_meta_scan over n values
// d_first[n] = exclusive scan of d_len[n] (u64; the callers put a 0 behind the last length, so the last element is the total)
hipError_t launch_meta_scan(void *d_temp, size_t temp_bytes, const void *d_len, void *d_first, size_t n, hipStream_t stream);
// Sizes: one lane per item.  d_len u64[n + 1] (d_len[n] = 0) and d_src u64[n] (the item's first byte in its shard's
// table, META_NONE for an item without bytes).  Q == 0: item i is ordinal d_ordinal[i] of shard d_shard[i] (d_shard
// nullptr: shard 0).  Q > 0 (n = Q * S): item q * S + p is ordinal d_ordinal[p * Q + q] of shard p where
// d_copies[p * Q + q] > 0, else empty -- the [S][Q] arrays launch_dollar_count writes.  A shard >= S, an ordinal >=
// num_strings (UINT64_MAX included) and a shard without table give an empty value.
hipError_t launch_meta_sizes(const meta_view *d_meta, uint32_t S, const void *d_shard, const void *d_ordinal, const void *d_copies,
                             size_t Q, size_t n, void *d_len, void *d_src, hipStream_t stream);
// Copy: item i's bytes = base[d_src[i] ..) -> d_dst[d_first[i] .. d_first[i+1]); base = d_base if given, else its shard's
// table (shards as in launch_meta_sizes).  Nothing is written when d_first[n] > cap.
hipError_t launch_meta_copy(const meta_view *d_meta, uint32_t S, const void *d_shard, size_t Q, const void *d_base, const void *d_src,
                            const void *d_first, size_t n, void *d_dst, uint64_t cap, hipStream_t stream);
// Build: pairs [base, base + n) of a build with (ordinal, copies) in one shard: win[o] = max(win[o], index + 1) over every
// ordinal o of the pair (atomicMax: the pair with the higher index wins, whatever the order of the lanes)
hipError_t launch_meta_winners(const void *d_ordinal, const void *d_copies, size_t n, uint64_t base, void *d_win, uint64_t num_strings,
                               hipStream_t stream);
// for the ordinals won by a pair of [c0, c1): d_len[o] = that pair's value length, d_src[o] = its value's offset from the
// chunk's first value byte (d_voff = voff[c0 .. c1], c1 - c0 + 1 entries); either output may be nullptr; an ordinal won
// by another chunk keeps its d_len and gets d_src META_NONE.  *d_given (optional) += ordinals with a winner in the chunk.
hipError_t launch_meta_winner_values(const void *d_win, uint64_t num_strings, const void *d_voff, uint64_t c0, uint64_t c1, void *d_len,
                                     void *d_src, void *d_given, hipStream_t stream);
// sample_counts.hip: rsbwt_set_sample_counts' reduction of located rows to per-query sample matrices.
//   launch_meta_heads: the build's head bits: bit o of d_heads (u32 words, zeroed by the caller) is set for every pair with
//     copies > 0 and ordinal o < num_strings (atomicOr: two pairs that name one string set one bit)
//   launch_sample_regions: d_rows_of[p] (u64[S], zeroed by the caller) += the rows of d_shard u32[first[Q]] that name shard p,
//     then d_region u64[S][2] = every shard's first slot and slot count - 1: a power of two strictly above its rows, at least
//     twice its rows unless `tight` -- under 4 x rows + 1 slots, so 4 x cap + S slots hold all regions.  Nothing is counted
//     when first[Q] > cap (the rows were not made).
//   launch_sample_tally: one lane per row; see the struct.  keys_in_lds is set by the launcher.
//   launch_sample_status: d_status8 = {first[Q], rows on a head ordinal, carriers, records, records with an unknown code,
//     launch_locate's LF steps (d_locate_work2[1]; nullptr: 0), rows not located, 0}
constexpr size_t TALLY_LDS_BYTES = 32u << 10;  // the dictionary's keys live in LDS while 8 C fits this
enum { TALLY_WORK_HEADS = 0, TALLY_WORK_CARRIERS, TALLY_WORK_RECORDS, TALLY_WORK_UNKNOWN, TALLY_WORK_LOST, TALLY_WORK_COUNTERS };
constexpr size_t TALLY_WORK_STRIDE = 32;  // u64 words between two counters: 256 bytes
struct sample_tally {
    const meta_view *meta;  // [S]
    uint32_t S;
    const uint64_t *first;  // [Q + 1]: the rows of query q are first[q] .. first[q + 1] (launch_interval_totals)
    size_t Q;               // <= 2^24
    const uint32_t *shard;  // [total] (launch_interval_fill)
    const uint64_t *ordinal;  // [total] (launch_locate; UINT64_MAX: not located -> counted in TALLY_WORK_LOST)
    uint64_t total;           // room for rows: the rows are the first first[Q] of them, none when first[Q] > total
    unsigned long long *set;  // the regions' slots, all ones (empty) when the launch starts
    const uint64_t *region;   // [S][2]: a shard's first slot and its slot count - 1 (a power of two above its rows, minus 1)
    const uint64_t *keys;     // [C] ascending (sample_codes.h)
    uint32_t C, size_of_sample, has_other, keys_in_lds;
    uint32_t *strings;        // [Q][C + 1], zeroed by the caller; may be nullptr
    long long *copies;        // [Q][C + 1], zeroed by the caller; may be nullptr
    unsigned long long *carriers;  // [Q], zeroed by the caller; may be nullptr
    unsigned long long *work;      // TALLY_WORK_COUNTERS counters TALLY_WORK_STRIDE words apart, zeroed by the caller
};
hipError_t launch_meta_heads(const void *d_ordinal, const void *d_copies, size_t n, void *d_heads, uint64_t num_strings, hipStream_t stream);
hipError_t launch_sample_regions(const void *d_shard, const void *d_first, size_t Q, uint64_t cap, uint32_t S, bool tight, void *d_rows_of,
                                 void *d_region, hipStream_t stream);
hipError_t launch_sample_status(const void *d_first, size_t Q, const void *d_work, const void *d_locate_work2, void *d_status8, hipStream_t stream);
hipError_t launch_sample_tally(const sample_tally &a, hipStream_t stream);
// The 1-mismatch search of a set by worklist (mm1_worklist.hip; k <= 32, 0 < tn < k, one table depth k - tn for all
// shards).  launch_mm1_worklists takes the step of the three substitutions of every traced position (d_trace
// [nshards][m][tn], d_own [nshards][m] pairs: the traced search's output) and appends the variants that survive it to
// d_worklists [nshards][wl_cap] x 32 B, wl_cap >= m * 3 * tn; d_counts u64[nshards * WL_COUNT_STRIDE] their lengths (entry s
// at s * WL_COUNT_STRIDE); hits that need no further step go straight to d_sparse [nshards][mv] / d_hit_bits.  d_branch_work
// (optional): the search launches' counter words (WORK_*): steps += 3 per item, lookups += 2, lines fetched; word 13 =
// variants alive after the step, 14 = variants passed on unstepped.
// launch_search_worklist then runs, per shard, the m * 3 (k - tn) variants substituted inside the tables' reach -- no
// records: the kernel spells them out and reads their table entries itself (search_solo.h, WL) -- and the appended
// records: results at the variants' canonical indices.
// (the lists' lengths sit WL_COUNT_STRIDE u64 apart: appended to by every wave of the branch kernel, they must not share
// a cache line -- eight counters in one line serialised the kernel at one atomic at a time: 10 ms instead of 3)
constexpr uint32_t WL_COUNT_STRIDE = 32;
hipError_t launch_mm1_worklists(const shard_view *d_shards, uint32_t nshards, const void *d_packed, const void *d_valid, size_t m,
                                uint32_t k, uint32_t tn, const void *d_trace, const void *d_own, void *d_worklists, size_t wl_cap,
                                void *d_counts, void *d_sparse, void *d_hit_bits, int num_cus, hipStream_t stream,
                                unsigned long long *d_branch_work = nullptr);
// (d_pre, optional: the implicit items' table entries read ahead by launch_wl_table_entries, u64 [nshards][m * 3 (k - tn)])
hipError_t launch_search_worklist(scratch_cache &scratch, const shard_view *d_shards, uint32_t nshards, const void *d_packed,
                                  const void *d_valid, size_t m, uint32_t tn, const void *d_worklists, const void *d_counts, size_t wl_cap,
                                  uint32_t k, void *d_sparse, void *d_hit_bits, unsigned long long *d_work, int num_cus,
                                  hipStream_t stream, hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr, const void *d_pre = nullptr);
hipError_t launch_wl_table_entries(const shard_view *d_shards, uint32_t nshards, const void *d_packed, size_t m, uint32_t k, uint32_t tn,
                                   void *d_pre, hipStream_t stream);
// launch_search_walk replaces the traced launch and launch_mm1_worklists' branch kernel by ONE walk of the k-mers
// (search_solo.h, WALK): the k-mers' own intervals to d_sparse / d_hit_bits at their canonical indices, the variants
// that survive the step of their position appended to d_worklists (d_counts zeroed by the caller), no trace.
hipError_t launch_search_walk(scratch_cache &scratch, const shard_view *d_shards, uint32_t nshards, const void *d_packed,
                              const void *d_valid, size_t m, uint32_t tn, void *d_worklists, void *d_counts, size_t wl_cap, uint32_t k,
                              void *d_sparse, void *d_hit_bits, unsigned long long *d_work, int num_cus, hipStream_t stream,
                              hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr);
constexpr int WORK_WORDS = 16;  // counters of a counting launch (search_lines.hip, WORK_*)

// k-mer table: fills d_entries[c * stride], c < 4^T, by searching every T-mer (fmt = KTAB_GROUPED: the 12-byte
// records at d_entries + 12 * g * stride bytes, g < 4^(T-1); *untabulated = T-mers left to the search itself).
// `view` is the host copy of the shard's view (no table yet).
hipError_t build_ktable(const shard_view &view, uint32_t T, uint64_t *d_entries, uint32_t stride, int num_cus,
                        hipStream_t stream, uint32_t fmt = KTAB_PLAIN, uint64_t *untabulated = nullptr);

// class BWT mirrors, batched
hipError_t launch_occ_batch(const shard_view &ix, const void *d_syms, const void *d_index, size_t n,
                            void *d_out, hipStream_t stream);
hipError_t launch_char_batch(const shard_view &ix, const void *d_index, size_t n, void *d_out,
                             hipStream_t stream);
// (needs the sampled select table: shard_view::sel, launch_select_samples)
hipError_t launch_occ_at_batch(const shard_view &ix, const void *d_syms, const void *d_bc, size_t n, void *d_out,
                               hipStream_t stream);
// The list of the set bits of `bits` (n_searches bits), in order: record i = {lower, upper, search index, 0}
// (32 B) from sparse[index]; at most `cap` records are written, *d_total receives how many there are.
// d_block_counts: compact_hits_block_words(n_searches) u64 of scratch.
// nseg > 1: the same for nseg maps at once (the shards of one search launch): maps hit_map_words(n_searches) words
// apart, sparse results n_searches records apart, lists cap records apart, totals one u64 each, block scratch
// compact_hits_block_words(n_searches) apart.
size_t compact_hits_block_words(size_t n_searches);
hipError_t launch_compact_hits(const void *d_bits, const void *d_sparse, size_t n_searches, void *d_hits, size_t cap,
                               void *d_total, void *d_block_counts, hipStream_t stream, uint32_t nseg = 1);
// {lower, upper} pairs <-> 10-byte {lower:40, width:40} records (kernels.hip); d_unfit: optional u32 counter of
// pairs that do not fit the record (none does for an interval findInterval produced)
hipError_t launch_pack_pairs10(const void *d_pairs, size_t n, void *d_packed, void *d_unfit, hipStream_t stream);
hipError_t launch_unpack_pairs10(const void *d_packed, size_t n, void *d_pairs, hipStream_t stream);
// extracted reads <-> 2 bits per base ([n][stride] ASCII + lengths <-> [n][stride / 4] bytes; stride % 16 == 0)
hipError_t launch_pack_reads2(const void *d_reads, const void *d_len, size_t n, uint32_t stride, void *d_packed, hipStream_t stream);
hipError_t launch_unpack_reads2(const void *d_packed, const void *d_len, size_t n, uint32_t stride, void *d_reads, hipStream_t stream);
hipError_t launch_variants(const void *d_packed, const void *d_valid, size_t Q, uint32_t k, void *d_vpacked,
                           void *d_vvalid, hipStream_t stream);
// read extraction: sampled select table (5 x stride u64: for every 256th occurrence of each symbol its
// window and how the 256 occurrences from it on spread over the next windows -- kernels.hip) and the walk kernel
hipError_t launch_debug_fast_window(const void *d_p, size_t n, uint32_t S, void *d_w, void *d_r, hipStream_t stream);
uint64_t select_sample_stride(const shard_view &ix);
hipError_t launch_select_samples(const shard_view &ix, uint64_t *d_sel, hipStream_t stream);
// psi hints inside the window lines that have room for one (line_format.h); after the samples.  *d_made (optional,
// zeroed by the caller) counts the lines that got one
hipError_t launch_psi_hints(const shard_view &ix, unsigned long long *d_made, hipStream_t stream);
// extract_lines.hip: extractPrefix + extractPostfix of n rows of EACH of the nshards shards whose views (with their
// select samples: shard_view::sel) are the device array d_shards, wave-cooperative, one launch sequence for all of
// them: d_rows [nshards][n], d_out [nshards][n][stride], d_plen / d_len [nshards][n]
hipError_t launch_extract_wave(scratch_cache &scratch, const shard_view *d_shards, uint32_t nshards, const void *d_rows,
                               size_t n, void *d_out, uint32_t stride, void *d_plen, void *d_len, int num_cus,
                               hipStream_t stream, unsigned long long *d_work = nullptr);
// d_work (counting mode): WORK_WORDS counters, zeroed by the caller: words 0-7 the prefix walk, 8-15 the
// postfix walk (extract_lines.hip, XW_*)
// The same walks over RAGGED segments: shard i's rows are d_rows[seg(i) .. seg(i + 1)), seg(i) = d_seg[i * seg_stride] (u64, in
// HBM: interval_rows.hip's cell scan, seg_stride = Q) -- `total` rows in all (< 2^31), d_out [total][stride], d_plen / d_len
// [total], in the rows' order.  No padding: a set whose rows sit in one shard costs what they cost.
hipError_t launch_extract_ragged(scratch_cache &scratch, const shard_view *d_shards, uint32_t nshards, const void *d_rows, size_t total,
                                 const void *d_seg, size_t seg_stride, void *d_out, uint32_t stride, void *d_plen, void *d_len, int num_cus,
                                 hipStream_t stream);
// locate.hip: the LF walk of n (shard, row) entries to the row of their read's full suffix: d_shard_of u32[n] (nullptr:
// one shard, every entry a row of it), d_rows u64[n] in any order; d_read_row / d_ordinal u64[n], d_offset u32[n], each
// optional; max_steps 0 = 2^20.  d_work2 (optional, zeroed by the caller): [0] += rows that ended on '$', [1] += LF steps.
// One launch walks all the shards, a wave one shard at a time.  d_n (optional, u64 in HBM): the list ends at min(n, *d_n),
// for a caller that enqueues the launch before the device has counted its rows (sample_walk.hip); n sizes the grid.
hipError_t launch_locate(scratch_cache &scratch, const shard_view *d_shards, uint32_t nshards, const void *d_shard_of, const void *d_rows,
                         size_t n, uint32_t max_steps, void *d_read_row, void *d_ordinal, void *d_offset, unsigned long long *d_work2,
                         int num_cus, hipStream_t stream, const void *d_n = nullptr);
// interval_rows.hip: {lower, upper} pairs [S][Q] -> the rows of the batch, with a limit on the rows of one query.
//   launch_interval_totals: d_matches u64[Q] (every query's rows over the S shards), d_first u64[Q + 1] (exclusive scan of the
//     totals of the queries at or under max_rows; 0 = no limit), *d_over (u64) = queries over it; d_kept: u64[Q + 1] scratch
//   launch_interval_cells: d_cellpos u64[S * Q + 1] = where shard i's rows of query q start when the kept rows are laid
//     out shard by shard; d_cellw: u64[S * Q + 1] scratch
//   launch_interval_fill: a thread per output row t < cap: d_shard[t], d_rows[t] (optional) in the caller's order --
//     nothing at all when first[Q] > cap; with d_cellpos also d_cell_rows[cell row] and d_dest[t] = that cell row (u32)
// d_temp / temp_bytes: interval_rows_scan_bytes(number of elements scanned) bytes of scratch
size_t interval_rows_scan_bytes(size_t n);
hipError_t launch_interval_totals(const shard_view *d_views, uint32_t S, const void *d_pairs, size_t Q, uint64_t max_rows, void *d_matches,
                                  void *d_kept, void *d_first, void *d_over, void *d_temp, size_t temp_bytes, hipStream_t stream);
hipError_t launch_interval_cells(const shard_view *d_views, uint32_t S, const void *d_pairs, size_t Q, uint64_t max_rows, const void *d_matches,
                                 void *d_cellw, void *d_cellpos, void *d_temp, size_t temp_bytes, hipStream_t stream);
hipError_t launch_interval_fill(const shard_view *d_views, uint32_t S, const void *d_pairs, size_t Q, const void *d_first, size_t cap,
                                void *d_shard, void *d_rows, const void *d_cellpos, void *d_cell_rows, void *d_dest, hipStream_t stream);
// gt_narrow.hip: SiteMatch's candidate legs (find_gt_reads, src/service/service.cpp:507-711).  A batch is its queries'
// text back to back plus, per query, where it starts, its length and its site; a SLOT is one all-ACGT tile of one
// query, an ITEM one leg of a slot (item = 2 * slot + leg).  nprev[i] says where the last symbol outside ACGT at or
// before text position i lies: 1 + its index inside its query, 0 for none.
struct gt_batch {
    const char *text;
    const uint32_t *nprev;
    const uint64_t *q_off;
    const uint32_t *q_len;
    const uint64_t *q_pos;
    const uint32_t *slot_query, *slot_tile;
    size_t nitems;
    uint32_t k, step;  // tile length; skip + 1
    uint64_t M;        // max interval size
};
// a leg: the final string w[a:b) and its interval; label 0 = the tile itself (its interval is at or under the limit), 1 / 2 = the
// first / second lengthened leg; a == 0xFFFFFFFF: no leg -- reserved = 1 when one was owed and the string could not be lengthened
// any further (it would need a < 0 or b > L)
struct gt_leg {
    uint32_t a, b;
    uint64_t lower, upper;
    uint32_t label, reserved;
};
//   launch_gt_narrow: one lane per (item, shard): d_legs gt_leg[nshards][nitems], d_pairs {lower, upper}[nshards][nitems] as
//     the interval-rows kernels take them (all ones for no leg); d_work[0] += LF steps taken while lengthening
//   launch_gt_filter: the span filter over the legs' rows (launch_interval_fill's d_shard, launch_locate's d_offset and
//     d_read_row, d_first u64[nitems + 1]) and their compaction: d_kept_rows gt_kept_row[total] receives one record per row
//     kept, d_counters[0] of them in all, in no particular order (d_counters zeroed by the caller); d_counters[1] += rows
//     whose walk did not end (offset UINT32_MAX)
struct gt_kept_row {
    uint32_t item, shard, offset;  // shard: the launch's number
    uint32_t pending;              // 1: a LEFT row that stays unless its read is too short
    uint64_t read_row;
};
hipError_t launch_gt_narrow(const shard_view *d_shards, uint32_t nshards, const gt_batch &bt, void *d_legs, void *d_pairs,
                            unsigned long long *d_work, hipStream_t stream);
// (d_ordinal, launch_locate's: d_kept_rows is gt_site_row[total] instead, the record with the row's ordinal behind it)
struct gt_site_row {
    uint32_t item, shard, offset, pending;
    uint64_t read_row, ordinal;
};
hipError_t launch_gt_filter(const gt_batch &bt, const void *d_legs, const void *d_first, const void *d_shard_of, const void *d_offset,
                            const void *d_read_row, uint64_t total, void *d_kept_rows, unsigned long long *d_counters, hipStream_t stream,
                            const void *d_ordinal = nullptr);
// match_stats.hip: matching statistics (include/rsbwt.h: the definition).  A batch is its queries' text back to back and
// where each starts: position t < N = off[Q] belongs to the query with off[q] <= t < off[q + 1] (off[0] = 0), all in HBM.
struct match_batch {
    const char *text;
    const uint64_t *off;  // [Q + 1]
    size_t Q, N;
    uint32_t cap;  // max_len; 0 = none
    uint64_t m;    // rows a match must hold, >= 1
};
//   launch_match_stats: one lane per (position, shard): d_len u32[nshards][N], d_pairs {lower, upper}[nshards][N] (optional);
//     d_work (optional, zeroed by the caller) [0..3] += LF steps, lane-passes that fetched a line, starts from the k-mer
//     table, restarts from initInterval after a table entry was refused
//   launch_match_smems: the SMEMs of those answers, compacted: d_smems rsbwt_smem[cap_records] (shard = the launch's
//     number) receives one record per SMEM, *d_counter (zeroed by the caller) of them in all, in no particular order
hipError_t launch_match_stats(const shard_view *d_shards, uint32_t nshards, const match_batch &bt, void *d_len, void *d_pairs,
                              unsigned long long *d_work, hipStream_t stream);
hipError_t launch_match_smems(uint32_t nshards, const match_batch &bt, const void *d_len, const void *d_pairs, void *d_smems, uint64_t cap_records,
                              unsigned long long *d_counter, hipStream_t stream);
// overlaps.hip: the reads that begin with a suffix of a query (include/rsbwt.h: the definition).  A batch is laid out as
// a match_batch's; position t names the suffix of its query that starts there.
struct overlap_batch {
    const char *text;
    const uint64_t *off;  // [Q + 1]
    size_t Q, N;
    uint32_t min_overlap;  // >= 1
    uint32_t max_overlap;  // 0 = none
};
//   launch_overlaps: one lane per (query, shard): d_pairs {ordinal, count}[nshards][N] is zeroed on `stream` and the
//     entries with count > 0 written; d_ivals {lower, upper}[nshards][N] (optional) is written at those entries ONLY;
//     d_work (optional, zeroed by the caller) [0..4] += LF steps, lane-passes that fetched a line, starts from the k-mer
//     table, lane-passes fetched for '$' alone, entries with count > 0
//   launch_overlap_records: those entries compacted: d_out rsbwt_overlap[cap_records] (shard = the launch's number),
//     *d_counter (zeroed by the caller) of them in all, in no particular order
hipError_t launch_overlaps(const shard_view *d_shards, uint32_t nshards, const overlap_batch &bt, void *d_pairs, void *d_ivals,
                           unsigned long long *d_work, hipStream_t stream);
hipError_t launch_overlap_records(uint32_t nshards, const overlap_batch &bt, const void *d_pairs, const void *d_ivals, void *d_out,
                                  uint64_t cap_records, unsigned long long *d_counter, hipStream_t stream);
// walk.hip: extension counts and walks (include/rsbwt.h: the definition).  A batch is its seeds' text back to back and
// where each starts, as a match_batch's, all in HBM.
struct walk_batch {
    const char *text;
    const uint64_t *off;  // [Q + 1]
    size_t Q, N;
    uint32_t ctx;        // 1..255
    uint32_t max_steps;  // >= 1 (launch_extensions does not look at it)
    uint64_t min_count;  // >= 1 (launch_extensions does not look at it)
    uint32_t flags;      // RSBWT_WALK_LEFT | RSBWT_WALK_BOTH_STRANDS
};
//   launch_walk: a workgroup per 8 seeds walks them over all nshards shards: d_ext char[Q][max_steps] and d_support
//     u32[Q][max_steps] (optional) are zeroed on `stream` and the appended symbols written; d_steps u32[Q], d_stop u8[Q]
//     and d_last u64[Q][4] (optional) are written for every seed; d_work (optional, zeroed by the caller) [1..5] +=
//     appended symbols, candidate searches, LF steps, lane-passes that fetched a line, starts from the k-mer table
//   launch_extensions: a wave per (8 seeds, shard): d_counts u64[nshards][Q][4], every entry written; d_work [2..5] as above
hipError_t launch_walk(const shard_view *d_shards, uint32_t nshards, const walk_batch &bt, void *d_ext, void *d_steps, void *d_stop, void *d_support,
                       void *d_last, unsigned long long *d_work, hipStream_t stream);
hipError_t launch_extensions(const shard_view *d_shards, uint32_t nshards, const walk_batch &bt, void *d_counts, unsigned long long *d_work,
                             hipStream_t stream);
//   launch_unitigs: a workgroup per 8 items (4 seeds x 2 sides; item i = 2 * seed + side, side 1 walks left) walks them over
//     all nshards shards, stopping where another path joins; bt.flags holds RSBWT_WALK_BOTH_STRANDS at the most.  d_ext
//     char[2Q][max_steps] and d_support u32[2Q][max_steps] (optional) are zeroed on `stream`; d_steps u32[2Q], d_stop u8[2Q]
//     and d_last u64[2Q][8] (optional) are written for every item; d_work [1..5] as launch_walk's, [6..7] += onward and
//     return evaluations
hipError_t launch_unitigs(const shard_view *d_shards, uint32_t nshards, const walk_batch &bt, void *d_ext, void *d_steps, void *d_stop,
                          void *d_support, void *d_last, unsigned long long *d_work, hipStream_t stream);
// paths.hip: every path from a seed, depth first (include/rsbwt.h: the definition; paths_rule.h: the decisions).  The seeds
// are a walk_batch; the optional targets are their text back to back and where each starts, in HBM.
struct paths_batch {
    walk_batch seeds;
    const char *ttext;     // nullptr: no seed has a target
    const uint64_t *toff;  // [Q + 1], toff[0] = 0
    size_t TN;             // the targets' symbols: toff[Q]
    uint32_t max_paths;    // 1..256
    uint32_t max_evals;    // 1..2^20
};
//   paths_frame_bytes: the bytes of d_frames, the launch's frame store (a stack of paths_frame per seed)
//   launch_paths: a workgroup per 8 seeds searches them over all nshards shards.  d_ext char[Q][max_paths][max_steps],
//     d_steps u32[Q][max_paths], d_stop u8[Q][max_paths] and d_min_support u32[Q][max_paths] (optional) are zeroed on
//     `stream` and the paths written; d_npaths u32[Q] and d_state u8[Q] are written for every seed; d_work (optional,
//     zeroed by the caller) [1..5] as launch_walk's, [6..7] += evaluations and paths
size_t paths_frame_bytes(size_t Q, uint32_t max_steps, uint32_t max_evals);
hipError_t launch_paths(const shard_view *d_shards, uint32_t nshards, const paths_batch &pb, void *d_frames, void *d_ext, void *d_steps, void *d_stop,
                        void *d_min_support, void *d_npaths, void *d_state, unsigned long long *d_work, hipStream_t stream);
// sample_walk.hip: walks through one sample set's reads (include/rsbwt.h: the definition; sample_walk_rule.h: the host's
// share).  One slice of seeds on one device: sample_walk_bytes() of scratch, then sample_walk_enqueue() puts the whole
// walk on the stream -- init, then max_steps times {search, plan, rows, locate, tally, decide}, every launch leaving at
// once when no seed of the slice still walks -- and waits for nothing.
struct sample_walk_args {
    const shard_view *views;  // [S]
    const meta_view *meta;    // [S]
    uint32_t S;
    int num_cus;
    walk_batch bt;  // the slice's seeds; flags may hold RSBWT_WALK_SAMPLE_COPIES
    const uint64_t *keys;      // [C] ascending
    const uint32_t *mask_bits;  // [ceil(C / 32)]
    uint32_t C, size_of_sample, has_other;
    uint64_t max_rows;           // 1 .. 2^20
    uint32_t max_locate_steps;   // 0 = 2^20
    // outputs of a walk (evaluate_only == 0): as launch_walk's; every byte written
    void *ext, *steps, *stop, *support, *last;
    // outputs of one evaluation (evaluate_only != 0): raw i64[Q][8] the masked sums per (base, strand), matches u64[Q][8],
    // wide u8[Q] (this device's shards alone)
    uint32_t evaluate_only;
    void *raw, *matches8, *wide;
    unsigned long long *work;  // SAMPLE_WALK_WORK counters, zeroed by the caller, added to
    // measurement (optional, host side): an event is recorded on the stream when the enqueue starts and after every launch --
    // init, then per step search, plan, rows, locate, tally, decide -- and appended here; the caller reads and destroys them
    std::vector<hipEvent_t> *marks = nullptr;
};
constexpr int SAMPLE_WALK_KINDS = 7;  // init, search, plan, rows, locate, tally, decide
enum {
    SW_WORK_APPENDED = 0, SW_WORK_SEARCHES, SW_WORK_SEARCH_STEPS, SW_WORK_ROWS, SW_WORK_HEADS, SW_WORK_CARRIERS, SW_WORK_RECORDS,
    SW_WORK_LOST, SW_WORK_WIDE, SW_WORK_LOCATED, SW_WORK_LOCATE_STEPS, SAMPLE_WALK_WORK
};
size_t sample_walk_bytes(size_t Q, uint32_t S, uint32_t max_steps, uint64_t max_rows);
hipError_t sample_walk_enqueue(scratch_cache &scratch, const sample_walk_args &a, void *d_scratch, hipStream_t stream);
// d_status8 = {rows located, rows on a head ordinal, carriers, records read, appended symbols, LF steps of the rows' walks,
// rows not located, wide evaluations}
hipError_t launch_sample_walk_status(const unsigned long long *d_work, void *d_status8, hipStream_t stream);
// d_mask u8[C] -> d_bits u32[ceil(C / 32)], bit col of word col / 32 (sample_walk_rule.h, sample_walk_mask_bits)
hipError_t launch_sample_walk_mask(const void *d_mask, size_t C, void *d_bits, hipStream_t stream);
// ksw_align.hip: ksw_align of the reference's ksw.c and align_gt_read over it (ksw_pass.h), one lane per item.  A block is
// one wave of 64 items and belongs to the LENGTH CLASS of its longest pass: at most 32, 64, 104, 160 or KSW_LDS_ROWS rows
// -- the column lives in LDS, the launch's LDS sized for the class -- or more: the column lives in d_scratch
// (ksw_scratch_bytes(max_rows): KSW_HBM_BLOCKS resident blocks).  There is one launch per class; every launch goes over
// every block and takes the blocks that are its own, so none needs the lengths on the host.  min_rows / max_rows bound the
// items' longest passes (1 and 4096 when the host does not know): classes outside them are not launched.  d_perm
// (optional) names the item lane g works on -- the host orders items by length so that a wave's lanes finish together
// and a block's class fits it closely.  Everything in HBM.
//   ksw: pair i = qtext[qoff[i] .. qoff[i+1]) on the rows against ttext[toff[i] .. toff[i+1]) on the columns; out[i] =
//        {score, te, qe, tb, qb, 0}, all -1 for a pair with a length outside 1..4096 or match * min(qlen, tlen) >= 2^15
//   gt:  read i against request item[i]; verdict[i] = RSBWT_GT_*, RSBWT_GT_INVALID for a length outside 1..4096 or
//        item[i] >= Q; d_work14 (optional, zeroed by the caller): [0] += reads, [v] += reads with verdict v
constexpr uint32_t KSW_LDS_ROWS = 224;   // RSBWT_KSW_LDS_ROWS: 224 rows x 64 lanes x 4 B + their codes = 63 KiB of LDS
constexpr uint32_t KSW_HBM_BLOCKS = 128;
struct ksw_batch {
    const char *qtext, *ttext;
    const uint64_t *qoff, *toff;
    size_t n;
    const uint32_t *perm;
    int32_t match, mismatch, ambiguous, gapo, gape;
};
struct gt_align_batch {
    const char *reads, *text, *alt;
    const uint64_t *roff, *item, *off, *pos;
    const uint8_t *isalt;
    size_t n, Q;
    const uint32_t *perm;
    // optional indirection (nullptr: the packed roff form above): item i is read rid[i], which lies at address raddr[rid[i]]
    // (anywhere in HBM: reads extracted at two strides need not share a buffer) with rlen[rid[i]] symbols; reads / roff
    // are not looked at.  Requests that share a read then share its bytes.
    const uint32_t *rid = nullptr;
    const uint64_t *raddr = nullptr;
    const uint32_t *rlen = nullptr;
};
size_t ksw_scratch_bytes(uint32_t max_rows);  // 0 while max_rows <= KSW_LDS_ROWS: d_scratch may be null then
hipError_t launch_ksw_align(const ksw_batch &bt, uint32_t min_rows, uint32_t max_rows, void *d_scratch, void *d_out, hipStream_t stream);
hipError_t launch_gt_align(const gt_align_batch &bt, uint32_t min_rows, uint32_t max_rows, void *d_scratch, void *d_verdict,
                           unsigned long long *d_work14, hipStream_t stream);
// site_counts.hip: rsbwt_set_site_sample_counts -- the span filter's kept rows (gt_site_row) handed to the alignment and the
// kept reads' sample records tallied without a row, a read or a verdict leaving the device.  Everything in HBM; the stages
// are enqueued on one stream in this order (the host reads a size back where the next stage's launch needs one):
//   launch_site_legs     work[SITE_WORK_LEGS] += the leg records of d_legs gt_leg[cells] that hold a leg
//   launch_site_rows     STAGE 2, one lane per kept row (d_rows gt_site_row[*d_nrows], at most cap): rows_of[shard] (u64[S],
//                        zeroed) counted first and the regions made from it (launch_sample_regions' rule); then a row on a
//                        head ordinal inserts (request << 40 | ordinal) into its shard's region of `set` (all ones = empty,
//                        every access the 64-bit CAS), the winner stores set_row[slot] = read_row, and every row takes
//                        atomicMin(set_need[slot], the read length that lets it stay): gt_span_rule.h, 0 for a row that is
//                        not pending, capped at SITE_NEED_MAX; set_need starts all ones.  heads_only = false
//                        (site_reads.hip): no head test, d_meta is not read and every kept row of a shard inserts; heads_only
//                        with a null d_meta is hipErrorInvalidValue.
//   launch_site_compact  STAGE 3a, one lane per slot (nslots of them): the set's entries as site_item records in any order,
//                        work[SITE_WORK_ITEMS] of them; sort_key[i] = shard << row_bits | read_row and sort_idx[i] = i
//   launch_site_reads    STAGE 3b over n items: sort on (shard, read_row), unique: items[i].rid = the read's number among
//                        the distinct ones, d_rows[rid] its read_row, d_seg u64[S + 1] where each shard's reads start
//                        (launch_extract_ragged's segments, seg_stride 1), *d_nreads (u64) how many.  d_tmp: site_reads_tmp_bytes(n).
//   launch_site_over     after the extraction at the first stride: d_over u64[R + 1] = 1 for a read that did not fit (length
//                        UINT32_MAX), d_ofirst its exclusive scan (d_ofirst[R] = how many); *d_longest (zeroed) = the longest
//                        read that fit; d_tmp: meta_scan_bytes(R + 1)
//   launch_site_wide     those reads' rows compacted in order (d_wrows) and d_wseg u64[S + 1] for the second extraction
//   launch_site_addr     raddr[r] = where read r lies (narrow + r * stride, or wide + d_ofirst[r] * wide_stride) and rlen[r]
//                        from the second extraction for the reads that took it (wide = nullptr: none did)
//   launch_site_items    STAGE 4, one lane per item: the needed-length rule with the read's length; a survivor gets
//                        req[i] = its request, the others UINT64_MAX (launch_gt_align's RSBWT_GT_INVALID: not aligned);
//                        rid[i]; perm_key[i] = the item's longest pass (0: not aligned), perm_idx[i] = i; aligned[q] += 1 per
//                        survivor; work: SITE_WORK_ALIGNED, SITE_WORK_TOO_LONG (a read over 4,096 symbols)
//   launch_site_perm     perm = the items ordered by perm_key (launch_gt_align's d_perm); d_tmp: site_perm_tmp_bytes(n)
//   launch_site_tally    STAGE 5, one lane per item whose verdict is one of the three KEEPs: its value's records into row
//                        req[i] of the matrices (sample_records.h), carriers[q] += 1; work: SITE_WORK_KEPT, _RECORDS, _UNKNOWN
enum { SITE_WORK_LEGS = 0, SITE_WORK_HEADS, SITE_WORK_ITEMS, SITE_WORK_ALIGNED, SITE_WORK_KEPT, SITE_WORK_RECORDS, SITE_WORK_UNKNOWN,
       SITE_WORK_TOO_LONG, SITE_WORK_COUNTERS };
constexpr uint32_t SITE_NEED_MAX = 0xFFFFFFFEu;
struct site_item {
    uint64_t ordinal, read_row;
    uint32_t q, shard, need, rid;
};
struct site_set {
    unsigned long long *keys;  // [nslots]
    uint64_t *row;             // [nslots]
    uint32_t *need;            // [nslots]
    uint64_t *region;          // [S][2]: a shard's first slot and its slot count - 1
    uint64_t nslots;           // room: 4 x cap + S
};
struct site_tally {
    const site_item *items;
    size_t n;
    const uint64_t *req;     // [n]
    const uint8_t *verdict;  // [n]
    const meta_view *meta;   // [S]
    uint32_t S;
    const uint64_t *keys;  // [C] ascending
    uint32_t C, size_of_sample, has_other;
    uint32_t *strings;
    long long *copies;
    unsigned long long *carriers;
    unsigned long long *work;  // SITE_WORK_COUNTERS counters TALLY_WORK_STRIDE words apart
};
size_t site_reads_tmp_bytes(size_t n);
size_t site_perm_tmp_bytes(size_t n);
hipError_t launch_site_legs(const void *d_legs, size_t cells, unsigned long long *d_work, hipStream_t stream);
hipError_t launch_site_rows(const gt_batch &bt, const void *d_legs, const void *d_rows, const unsigned long long *d_nrows, uint64_t cap,
                            const meta_view *d_meta, bool heads_only, uint32_t S, bool tight, void *d_rows_of, const site_set &set,
                            unsigned long long *d_work, hipStream_t stream);
hipError_t launch_site_compact(const site_set &set, uint32_t S, uint32_t row_bits, void *d_items, void *d_sort_key, void *d_sort_idx, uint64_t cap,
                               unsigned long long *d_work, hipStream_t stream);
hipError_t launch_site_reads(void *d_items, size_t n, uint32_t S, uint32_t row_bits, void *d_sort_key, void *d_sort_idx, void *d_tmp, size_t tmp_bytes,
                             void *d_rows, void *d_seg, void *d_nreads, hipStream_t stream);
hipError_t launch_site_over(const void *d_rlen, size_t R, void *d_over, void *d_ofirst, unsigned long long *d_longest, void *d_tmp, size_t tmp_bytes,
                            hipStream_t stream);
hipError_t launch_site_wide(const void *d_rows, const void *d_seg, uint32_t S, size_t R, const void *d_over, const void *d_ofirst, void *d_wrows,
                            void *d_wseg, hipStream_t stream);
hipError_t launch_site_addr(const void *d_narrow, uint32_t stride, const void *d_wide, uint32_t wide_stride, const void *d_over, const void *d_ofirst,
                            const void *d_wlen, size_t R, void *d_raddr, void *d_rlen, hipStream_t stream);
hipError_t launch_site_items(const void *d_items, size_t n, const void *d_rlen, const void *d_off, size_t Q, void *d_req, void *d_rid,
                             void *d_perm_key, void *d_perm_idx, unsigned long long *d_aligned, unsigned long long *d_work, hipStream_t stream);
hipError_t launch_site_perm(void *d_perm_key, void *d_perm_idx, size_t n, void *d_key_out, void *d_perm, void *d_tmp, size_t tmp_bytes,
                            hipStream_t stream);
hipError_t launch_site_tally(const site_tally &a, hipStream_t stream);
// site_reads.hip: rsbwt_set_site_reads -- the same stages with launch_site_rows told heads_only = false (every kept row is
// an entry, not the head copies alone), and instead of the tally:
//   launch_site_classes  after launch_site_addr: d_cflag u64[R + 1] = 1 where read r begins a string class (its shard, length
//                        or bytes differ from read r - 1's), d_cfirst its exclusive scan (d_cfirst[R] = the classes);
//                        d_tmp: meta_scan_bytes(R + 1)
//   launch_site_layout   after the alignment, over n items of Q <= 2^24 requests: sorts them by (request, read number) into
//                        d_tmp (site_layout_tmp_bytes(n); d_key u64[n] and d_idx u32[n] are its unsorted input), reports an
//                        item iff its verdict is a KEEP and the item before it is no kept item of the same request and class:
//                        d_out_rid / d_out_row [*d_nout] in the answer's order, d_first u64[Q * S + 1] the cells' starts;
//                        work[SITE_WORK_KEPT] += the items with a KEEP verdict
//   launch_site_gather   16 lanes per reported read: its bytes into d_out + i * stride, the slot's rest zeroed, d_out_len[i] its
//                        length (UINT32_MAX and a zeroed slot when it is longer than the stride)
size_t site_layout_tmp_bytes(size_t n);
hipError_t launch_site_classes(const void *d_raddr, const void *d_rlen, const void *d_seg, uint32_t S, size_t R, void *d_cflag, void *d_cfirst,
                               void *d_tmp, size_t tmp_bytes, hipStream_t stream);
hipError_t launch_site_layout(const void *d_items, size_t n, size_t Q, uint32_t S, const void *d_verdict, const void *d_cflag, const void *d_cfirst,
                              const void *d_rows, const void *d_seg, void *d_key, void *d_idx, void *d_tmp, size_t tmp_bytes, void *d_out_rid,
                              void *d_out_row, void *d_first, void *d_nout, unsigned long long *d_work, hipStream_t stream);
hipError_t launch_site_gather(const void *d_out_rid, size_t n, const void *d_raddr, const void *d_rlen, void *d_out, uint32_t stride, void *d_out_len,
                              hipStream_t stream);
// (SEL_SHIFT, sample_window, window_samples, window_psi_hint: line_format.h -- shared with the host-side layout test)
// query / query_exactmatch (query.cpp:87-120) over extracted reads
hipError_t launch_match_reads(const void *d_reads, const void *d_len, size_t n, uint32_t stride, const void *d_owner,
                              const void *d_kmers, uint32_t k, size_t kstride, void *d_flags, hipStream_t stream);
hipError_t launch_synth_runs(void *d_runs, uint64_t num_runs, uint64_t seed, hipStream_t stream, uint64_t first = 0);
hipError_t launch_sample_present(const shard_view &ix, size_t Q, uint32_t k, size_t stride,
                                 uint64_t seed, void *d_kmers, hipStream_t stream);

// build_lines.hip: builds the window lines in HBM from run bytes in HBM.  On success fills `view`
// (lines are hipMalloc'ed and owned by the caller).  want_span 0 = choose S from the data.
// Synchronises `stream`.  build_error: 0 ok, BUILD_ERANGE, BUILD_EFORMAT.
enum { BUILD_OK = 0, BUILD_ERANGE = 1, BUILD_EFORMAT = 2 };
struct build_result {
    shard_view view;
    uint64_t num_runs;
    uint64_t hbm_bytes;
    uint64_t far_lines, chunk_windows, far_windows, spilled_symbols;
};
// hint_room: every window line keeps room for a psi hint (line_format.h; RSBWT_OPEN_READS).
hipError_t build_lines(const void *d_runs, uint64_t num_runs, uint32_t want_span, bool hint_room, hipStream_t stream,
                       build_result *out, int *build_error);

}  // namespace rsb
#endif
