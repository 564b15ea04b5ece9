/*
 * rsbwt.h -- C-ABI of the MI355X population-BWT engine (librsbwt.so).
 *
 * Drop-in boundary for ReadServer's src/bwt backward-search path.  Every entry point
 * names the reference interface it replaces (paths relative to the ReadServer tree).
 * Plain pointers and sizes only; no C++ or torch types.  All functions returning int
 * give RSBWT_OK (0) or a negative RSBWT_E* code and never call exit() (the reference
 * exits on a bad file: src/bwt/rlebwt_reader.cpp:31-34).
 *
 * Conventions kept from the reference:
 *   - symbols are ASCII '$','A','C','G','T' (include/bwt/alphabet.h:8-9);
 *   - intervals are inclusive SA-row ranges [lower, upper], empty <=> lower > upper
 *     (include/bwt/query.h:8-11, src/bwt/query.cpp:35);
 *   - a k-mer holding a symbol outside ACGT, or k == 0, yields lower = 1, upper = 0 and
 *     count 0 (callers filter these in the reference: src/service/service.cpp:299-301);
 *   - count = upper >= lower ? upper - lower + 1 : 0 (src/service/service.cpp:304).
 *
 * The engine is the HIP path only: there is no CPU fallback.  Every call that needs the
 * GPU fails with RSBWT_ENODEV when none is usable.
 *
 * Thread safety: a handle may be queried concurrently from several host threads (the
 * reference shares one BWT* across its pool threads, src/service/service.cpp:1513).
 * Host-buffer calls serialise on the handle's internal stream and staging buffers;
 * *_dev calls only enqueue work on the caller's stream.
 */
#ifndef RSBWT_H
#define RSBWT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RSBWT_OK 0
#define RSBWT_EINVAL (-1)  /* bad argument                                   */
#define RSBWT_EIO (-2)     /* file missing / short / unreadable              */
#define RSBWT_EFORMAT (-3) /* not an SGA RLE .bwt (magic 0xCACA) or corrupt  */
#define RSBWT_ENOMEM (-4)  /* host or HBM allocation failed                  */
#define RSBWT_ENODEV (-5)  /* no usable HIP device                           */
#define RSBWT_EHIP (-6)    /* a HIP runtime call failed (see rsbwt_last_error) */
#define RSBWT_ERANGE (-7)  /* shard exceeds format limits (2^40 symbols) / buffer too small */
#define RSBWT_ESYS (-8)    /* the host runtime failed (a thread could not be started, ...)   */

/* open flags */
/* bit 0: RSBWT_OPEN_READS -- the shard will serve read extraction (extractPrefix / extractPostfix, query(),
 * src/bwt/query.cpp:43-100: what the reference's find_reads does with every interval): every window line is laid
 * out with room for a psi hint (88 of its 96 piece bytes hold pieces, so ~9 % more lines), the hints and a sparse
 * select-sample table (n / 512 bytes) are built as part of the open, and the index is immutable from then on.
 * Extraction's select then finds its window in the line the walk already stands in: one HBM request per step.
 * Without the flag the layout is the denser one; the first extraction / getOccAt then builds a dense sample
 * table (n / 32 bytes) and writes hints into the lines that happen to have room (about 6 in 10) -- into the
 * resident lines, where no search reads them, but an index a search-only deployment never pays for.
 * bit 1: RSBWT_OPEN_KTAB_GROUPED -- the k-mer table in its grouped format (below, rsbwt_attach_ktab_format): 3 B per
 * T-mer instead of 8, so the same HBM holds a table one level deeper; with depth 0 the deepest grouped table that fits
 * the budget and is deeper than the plain one would be (else the plain one).
 * bits 2..4: reserved (0).
 * bits 5..9: depth T of the k-mer table (4^T entries of 8 B holding findInterval's answer for
 * every T-mer; searches of k >= T symbols start from one lookup).  0 = auto (the deepest table
 * no larger than the index itself nor than a quarter of the free HBM, with 4^T <= n; rsbwt_set_open
 * sizes the tables of one GPU's shards together, out of three quarters of what is free once they are all resident), 31 = no table, else T = 2..16 (T = 16: 34 GB). */
#define RSBWT_OPEN_READS 1u
#define RSBWT_OPEN_KTAB_GROUPED 2u
#define RSBWT_KTAB_SHIFT 5
#define RSBWT_KTAB_MASK (0x1Fu << RSBWT_KTAB_SHIFT)
#define RSBWT_KTAB_NONE (31u << RSBWT_KTAB_SHIFT)
#define RSBWT_KTAB_DEPTH(t) ((uint32_t)(t) << RSBWT_KTAB_SHIFT)
/* bits 12..23: symbols per window of the HBM layout (one 128-byte line per window, so that an Occ
 * lookup is a single request); 0 = chosen from the data: ~88 run pieces per window, shrunk while
 * more than 2.5 % of the positions would lie past their window's line.  2..2944. */
#define RSBWT_SPAN_SHIFT 12
#define RSBWT_SPAN_MASK (0xFFFu << RSBWT_SPAN_SHIFT)
#define RSBWT_SPAN(s) ((uint32_t)(s) << RSBWT_SPAN_SHIFT)

typedef struct rsbwt rsbwt_t;         /* one BWT shard resident in one GPU's HBM */
typedef struct rsbwt_set rsbwt_set_t; /* several shards on this process's GPU(s) */

/* Library / environment ------------------------------------------------------------ */
const char *rsbwt_version(void);
int rsbwt_device_count(void);           /* number of visible HIP devices, 0 if none */
const char *rsbwt_last_error(void);     /* thread-local message of the last failure */
const char *rsbwt_strerror(int code);

/* Index lifetime ---------------------------------------------------------------------
 * rsbwt_open replaces  RLEBWT::RLEBWT(const std::string& filename, int smallSampleRate)
 * (include/bwt/rlebwt.h:17, src/bwt/rlebwt.cpp:11-32): reads the SGA .bwt file
 * (src/bwt/rlebwt_reader.cpp:27-48), uploads the run bytes and builds the device index in
 * HBM.  A "<file>.bpi2" next to it is ignored: the device index is derived from the runs. */
int rsbwt_open(const char *bwt_path, int device, uint32_t flags, rsbwt_t **out);
/* Same from run bytes in host memory (RLUnit bytes, include/bwt/rlunit.h:8-11). */
int rsbwt_open_runs(const uint8_t *runs, uint64_t num_runs, uint64_t num_strings,
                    int device, uint32_t flags, rsbwt_t **out);
/* Same from run bytes already in HBM on `device` (not retained after the call). */
int rsbwt_open_device_runs(const void *d_runs, uint64_t num_runs, uint64_t num_strings,
                           int device, uint32_t flags, rsbwt_t **out);
/* Replaces the owner's unique_ptr<BWT> release (src/service/service.cpp:1513). */
void rsbwt_close(rsbwt_t *h);

/* class BWT mirrors (include/bwt/bwt.h:6-15), one value per call ---------------------- */
uint64_t rsbwt_bwlen(const rsbwt_t *h);               /* BWT::getBWLen, rlebwt.cpp:303-305 */
uint64_t rsbwt_pc(const rsbwt_t *h, char b);          /* BWT::getPC,    rlebwt.cpp:229-231 */
char rsbwt_f(const rsbwt_t *h, uint64_t index);       /* BWT::getF,     rlebwt.cpp:307-314 */
int rsbwt_occ(rsbwt_t *h, char b, uint64_t index, uint64_t *occ);   /* BWT::getOcc,  rlebwt.cpp:268-301 */
int rsbwt_char(rsbwt_t *h, uint64_t index, char *c);                /* BWT::getChar, rlebwt.cpp:202-227 */
int rsbwt_occ_at(rsbwt_t *h, char b, uint64_t bc, uint64_t *index); /* BWT::getOccAt, rlebwt.cpp:233-266 */

/* batched forms of the same (host buffers) */
int rsbwt_occ_batch(rsbwt_t *h, const char *b, const uint64_t *index, size_t n, uint64_t *occ);
int rsbwt_char_batch(rsbwt_t *h, const uint64_t *index, size_t n, char *c);
int rsbwt_occ_at_batch(rsbwt_t *h, const char *b, const uint64_t *bc, size_t n, uint64_t *index);

/* Shape of the resident index */
uint64_t rsbwt_num_runs(const rsbwt_t *h);
uint64_t rsbwt_num_strings(const rsbwt_t *h);
uint64_t rsbwt_num_lines(const rsbwt_t *h);       /* 128-byte lines of the index in HBM */
uint32_t rsbwt_ktab_depth(const rsbwt_t *h);      /* 0 = no k-mer table */
uint32_t rsbwt_window_span(const rsbwt_t *h);     /* symbols per window */
uint64_t rsbwt_far_lines(const rsbwt_t *h);       /* lines that continue windows of > 120 pieces */
uint64_t rsbwt_spilled_symbols(const rsbwt_t *h); /* positions one request past their window's line */
uint64_t rsbwt_hbm_bytes(const rsbwt_t *h);       /* lines + tables */
uint64_t rsbwt_psi_hint_lines(const rsbwt_t *h);  /* window lines carrying a psi hint (without RSBWT_OPEN_READS: 0 until rsbwt_prepare_extraction) */
int rsbwt_opened_for_reads(const rsbwt_t *h);     /* 1: laid out with RSBWT_OPEN_READS */
/* Read extraction and getOccAt need a sampled select table.  A shard opened with RSBWT_OPEN_READS has it (and a psi
 * hint in every window line) when rsbwt_open* returns.  Any other shard builds it on its first extraction / getOccAt
 * call INTO A SIDE TABLE: nothing a search reads -- the lines, the handle's view -- is written after the handle has
 * been handed out, so that first call may run beside searches on other threads (until round 5 it rewrote the
 * handle's view and wrote psi hints into the resident lines).  Such a shard then extracts WITHOUT hints (about 1.9
 * requests per psi step instead of 1.4).  rsbwt_prepare_extraction gives it the samples and the hints its lines have
 * room for (about two thirds of them) in one go; it WRITES INTO THE RESIDENT LINES, so the owner calls it before it
 * shares the handle with other threads, like rsbwt_attach_ktab.  No-op on a shard opened for reads. */
int rsbwt_prepare_extraction(rsbwt_t *h);
/* Builds the k-mer table of depth T (2..16) of an open handle that has none. */
int rsbwt_attach_ktab(rsbwt_t *h, uint32_t T);
/* The same with the table's format named.  The table holds what findInterval (src/bwt/query.cpp:24-41) returns for
 * every T-mer, so that a search of k >= T symbols starts T steps in (the reference has no such table: it takes every
 * step, query.cpp:33-38).  PLAIN: 8 bytes per T-mer {lower:40, width:24}.  GROUPED: the four T-mers that differ in
 * their LAST symbol only are neighbours in the BWT's rows; one 12-byte record holds the first row of the four and their
 * running widths (14 bits each) = 3 bytes per T-mer, T up to 17.  A T-mer the record cannot describe -- one that does
 * not occur (the reference's empty interval depends on the step the search died at), or a group of 16383 rows or more
 * -- is searched from initInterval like an untabulated one: same answers, T more steps; rsbwt_ktab_info counts them.
 * AUTO: grouped where 64 <= n / 4^T and n / 4^(T-1) <= 2048 -- the groups fit their records and a T-mer's interval is
 * still many runs wide, so nearly every T-mer occurs (5.5e-5 of the 15-mers of a 1.17e11-symbol shard do not; at 7 rows
 * per 17-mer 46 % do not, and a plain table answers those in no step at all) -- else plain. */
#define RSBWT_KTAB_FORMAT_PLAIN 0u
#define RSBWT_KTAB_FORMAT_GROUPED 1u
#define RSBWT_KTAB_FORMAT_AUTO 2u
int rsbwt_attach_ktab_format(rsbwt_t *h, uint32_t T, uint32_t format);
/* format (RSBWT_KTAB_FORMAT_PLAIN / _GROUPED), bytes in HBM and -- grouped -- the T-mers left to the search; any may be NULL */
int rsbwt_ktab_info(const rsbwt_t *h, uint32_t *format, uint64_t *bytes, uint64_t *untabulated);
/* Test hook (RSBWT_ENABLE_TEST_HOOKS): n bytes of the resident index (region 0: the lines, 1: an owned k-mer table,
 * 2: the select sample table, 5 * select stride words of 8 bytes -- RSBWT_ERANGE until it has been built: at open with
 * RSBWT_OPEN_READS, else by rsbwt_prepare_extraction or a first extraction) copied out, the reading twin of
 * rsbwt_debug_poke. */
int rsbwt_debug_peek(rsbwt_t *h, int region, uint64_t offset, void *bytes, size_t n);
/* Test hook (RSBWT_ENABLE_TEST_HOOKS=1): the '$' count of rsbwt_read_copies on {lower, upper} pairs given by hand,
 * u64[Q][2]: copies[q] = Occ('$', upper) - Occ('$', lower - 1) with Occ(., -1) = 0 and ending[q] = upper - lower + 1 (may
 * be NULL) for lower <= upper < BWLen, zeros otherwise.  Answers no query. */
int rsbwt_debug_dollar_count(rsbwt_t *h, const uint64_t *pairs, size_t Q, uint64_t *copies, uint64_t *ending);
int rsbwt_device(const rsbwt_t *h);          /* the GPU the shard is resident on */
/* The device number the shard was opened with.  Equal to rsbwt_device() except under the TEST HOOK
 * RSBWT_TEST_DEVICE_ALIASES=N (honoured only while RSBWT_ENABLE_TEST_HOOKS is set; read at every rsbwt_open*):
 * device numbers 0..N-1 then name N logical devices dealt round-robin over the physical ones, and a shard set groups
 * its shards by LOGICAL device -- so the several-device host code of a set (a thread, a context pool and a fused
 * launch per device group; the merge of the groups' counts, lists and reads) runs on a box with one GPU.  RCCL is
 * not used between groups that share a GPU (it refuses two ranks on one device): such a set takes the paths of a
 * box without librccl. */
int rsbwt_logical_device(const rsbwt_t *h);

/* query.h mirrors, batched (include/bwt/query.h:18-32) ---------------------------------
 * rsbwt_find_intervals replaces  BWTInterval findInterval(const BWT*, const std::string& w)
 * (src/bwt/query.cpp:24-41) for Q k-mers at once: k-mer q is the k ASCII bytes at
 * kmers + q*stride (stride >= k).  lower/upper receive Q values each. */
int rsbwt_find_intervals(rsbwt_t *h, const char *kmers, size_t Q, uint32_t k, size_t stride,
                         uint64_t *lower, uint64_t *upper);
/* Replaces the count in count_reads (src/service/service.cpp:303-304). */
int rsbwt_count(rsbwt_t *h, const char *kmers, size_t Q, uint32_t k, size_t stride,
                uint64_t *counts);

/* 1-mismatch search (BASELINE configs[3]; not in the reference, defined by composition): for each
 * k-mer, the exact findInterval of the k-mer itself and of each of its 3k single-substitution
 * variants.  Outputs are [Q][3k+1] in canonical order: column 0 = the k-mer, column 1 + 3i + d =
 * position i replaced by the d-th base of ACGT without the original one.  Empty variants have
 * lower > upper, exactly as findInterval leaves them; a k-mer holding a symbol outside ACGT is
 * invalid as a whole (every column lower = 1, upper = 0). */
int rsbwt_find_intervals_1mm(rsbwt_t *h, const char *kmers, size_t Q, uint32_t k, size_t stride,
                             uint64_t *lower, uint64_t *upper);

/* (device-resident searches need 1 <= k <= 65535) */

/* The same search with the output SURVEY 8 f3 defines: only the variants that occur, as a list
 * sorted by (query, pos, base).  The dense [Q][3k+1] matrices above are mostly empty intervals
 * (1.5 KB per 31-mer over PCIe); the list is compacted on the device.  `hits` receives at most
 * `cap` records, *nhits the number found; RSBWT_ERANGE (nothing written) when cap is too small. */
typedef struct rsbwt_hit_1mm {
    uint64_t lower, upper; /* lower <= upper */
    uint32_t query;        /* index of the k-mer in the batch */
    int16_t pos;           /* -1: the k-mer itself, else the substituted position (0 = leftmost) */
    char base;             /* the base put there ('\0' for the k-mer itself) */
    char reserved;
} rsbwt_hit_1mm;
int rsbwt_hits_1mm(rsbwt_t *h, const char *kmers, size_t Q, uint32_t k, size_t stride,
                   rsbwt_hit_1mm *hits, size_t cap, size_t *nhits);

/* Batched read extraction: replaces  extractPrefix(pBWT, row) + extractPostfix(pBWT, row)
 * (src/bwt/query.cpp:43-85; joined as query() does, :94-96) for n SA rows.  Row i's read is written
 * to out + i*stride (no NUL), its length to len[i] and the length of its prefix part to
 * prefix_len[i] (either may be NULL).  A read that does not fit `stride` bytes, or a row >= BWLen,
 * gets len = UINT32_MAX (the reference would loop forever / read out of bounds).
 * "Fits" is |prefix| + |postfix| <= stride, for any stride > 0: a read of exactly `stride` symbols comes back whole, at
 * every split point, one of stride + 1 never does.  Unspecified, and not to be relied on: the bytes of row i's own
 * `stride` bytes past len[i] (all of them for a read that does not fit), and prefix_len[i] of a read that does not fit.
 * Nothing outside out[0 .. n*stride) is written.  The stride and the alignment of the row block choose how the bytes
 * are stored (16 at a time for stride % 16 == 0 on a 16-byte aligned block, 4 at a time for stride % 4 == 0 on a 4-byte
 * aligned one, else byte by byte), never what is stored; the same holds for every form below that takes a stride. */
int rsbwt_extract(rsbwt_t *h, const uint64_t *rows, size_t n, char *out, uint32_t stride,
                  uint32_t *len, uint32_t *prefix_len);

/* query.cpp:102-120  bool query_exactmatch(const BWT*, const string& w), batched: found[q] = 1 when
 * k-mer q is itself one of the indexed reads (w == extractPrefix(i) + extractPostfix(i) for a row i
 * of its interval), else 0 -- also for a string holding a symbol outside ACGT (query.cpp:103-105). */
int rsbwt_query_exactmatch(rsbwt_t *h, const char *kmers, size_t Q, uint32_t k, size_t stride,
                           uint8_t *found);
/* Whole-read matches by backward search from the terminator rows (csrc/read_lookup.hip).  In SGA's multi-string BWT
 * the rows [0, num_strings) are the suffixes that begin with a terminator; stepping w backwards from that row range ends
 * on the rows whose suffix is w$ -- the reads that END with w -- and such a row holds '$' in the BWT exactly when its
 * read also begins there:
 *     copies[q] = Occ('$', upper) - Occ('$', lower - 1) = how many indexed reads EQUAL k-mer q,
 *     ending[q] = upper - lower + 1                     = how many END with it (may be NULL).
 * |w| LF steps and one line fetch, whatever the width of w's own interval; no read is extracted, so none of these calls
 * needs RSBWT_OPEN_READS, select samples or psi hints, and none causes them to be built.  A k-mer that is empty, holds
 * a symbol outside ACGT or is longer than 65,535 symbols gives 0 / 0; so does every k-mer on a shard without
 * terminator rows.  Null arguments, stride < k, an empty index and a box without GPU: as rsbwt_find_intervals.
 * The _dev form takes rsbwt_pack_kmers_dev's packing, writes u64[Q] arrays on `stream` and synchronises nothing. */
int rsbwt_read_copies(rsbwt_t *h, const char *kmers, size_t Q, uint32_t k, size_t stride, uint64_t *copies,
                      uint64_t *ending);
int rsbwt_read_copies_dev(rsbwt_t *h, const void *d_packed, const void *d_valid, size_t Q, uint32_t k, void *d_copies,
                          void *d_ending, void *stream);
/* on != 0: rsbwt_query_exactmatch on this handle answers found[q] = copies[q] > 0 through rsbwt_read_copies instead of
 * extracting and comparing the reads of w's interval (the same booleans; default 0). */
int rsbwt_exactmatch_by_search(rsbwt_t *h, int on);
int rsbwt_exactmatch_is_by_search(const rsbwt_t *h);
/* query.cpp:87-100  vector<string> query(const BWT*, const string& w), batched: every read that
 * contains k-mer q, in SA-row order (extractPrefix(i) + extractPostfix(i) for i = lower..upper).
 * first[Q+1] receives the offsets of each k-mer's reads in the output (first[Q] = their number, also
 * stored in *nreads); read r is the read_len[r] bytes at reads + r*read_stride (UINT32_MAX: longer
 * than read_stride).  RSBWT_ERANGE with *nreads set and nothing extracted when cap_reads is too
 * small: call once with cap_reads = 0 to size the buffers. */
int rsbwt_query(rsbwt_t *h, const char *kmers, size_t Q, uint32_t k, size_t stride, uint64_t *first,
                char *reads, uint32_t read_stride, uint32_t *read_len, size_t cap_reads, size_t *nreads);

/* Device-resident forms: all pointers are HBM addresses on the handle's device, `stream` is a
 * hipStream_t (NULL = the null stream).  Nothing is synchronised. ------------------------ */
/* ASCII k-mers -> 2-bit packed words (A,C,G,T = 0..3, symbol i at bits 2*(i%32) of word i/32,
 * ceil(k/32) words per k-mer) + one validity byte per k-mer (0 = holds a non-ACGT symbol). */
int rsbwt_pack_kmers_dev(const void *d_kmers, size_t Q, uint32_t k, size_t stride,
                         void *d_packed, void *d_valid, int device, void *stream);
int rsbwt_find_intervals_dev(rsbwt_t *h, const void *d_packed, const void *d_valid, size_t Q,
                             uint32_t k, void *d_lower, void *d_upper, void *stream);
int rsbwt_count_dev(rsbwt_t *h, const void *d_packed, const void *d_valid, size_t Q, uint32_t k,
                    void *d_counts, void *stream);
/* The same intervals as BWTInterval pairs (include/bwt/query.h:8-11): d_pairs[q] = {lower, upper}, 16
 * bytes per k-mer, written by one store per search (the separate arrays cost two scattered stores). */
int rsbwt_find_interval_pairs_dev(rsbwt_t *h, const void *d_packed, const void *d_valid, size_t Q, uint32_t k,
                                  void *d_pairs, void *stream);
/* Interval pairs for the wire.  Every interval findInterval leaves (empty ones, the (1, 0) of an invalid
 * k-mer and the reference's (0, 2^64-1) corner included) is {lower < 2^40, upper = lower + width - 1 mod 2^64,
 * width < 2^40}, so {lower:40, width:40} carries it exactly: n pairs (16 n bytes, as rsbwt_*_interval_pairs_dev
 * writes them) <-> rsbwt_packed_pairs_bytes(n) = 10 n bytes rounded up to 4.  What a rank sends to the root GPU
 * of a multi-GPU job (5/8 of the bytes over xGMI).  d_unfit (optional u32 in HBM, zeroed by the caller) counts
 * pairs that do not fit the record -- none does for an interval this library produced. */
size_t rsbwt_packed_pairs_bytes(size_t n);
int rsbwt_pack_interval_pairs_dev(const void *d_pairs, size_t n, void *d_packed, void *d_unfit, int device, void *stream);
int rsbwt_unpack_interval_pairs_dev(const void *d_packed, size_t n, void *d_pairs, int device, void *stream);
/* Extracted reads for the wire: [n][stride] ASCII bytes (rsbwt_extract_dev's d_out) + their lengths <-> [n][stride / 4]
 * bytes, 2 bits per base (A, C, G, T = 0..3, base i at bits 2 (i % 4) of byte i / 4; zeros past a read's end and for a
 * read marked UINT32_MAX).  stride % 16 == 0.  What a rank sends of an extraction batch at N > 1: a quarter of the
 * bytes over xGMI; the lengths travel beside it.  Unpacking restores the bytes up to each read's length (NUL beyond). */
int rsbwt_pack_reads_dev(const void *d_reads, const void *d_len, size_t n, uint32_t stride, void *d_packed, int device, void *stream);
int rsbwt_unpack_reads_dev(const void *d_packed, const void *d_len, size_t n, uint32_t stride, void *d_reads, int device, void *stream);
/* 1-mismatch search of m packed k-mers: d_lower/d_upper [m][3k+1] (rsbwt_find_intervals_1mm's layout);
 * d_scratch: rsbwt_1mm_scratch_bytes(h, m, k) bytes. */
size_t rsbwt_1mm_scratch_bytes(const rsbwt_t *h, size_t m, uint32_t k);
int rsbwt_find_intervals_1mm_dev(rsbwt_t *h, const void *d_packed, const void *d_valid, size_t m, uint32_t k,
                                 void *d_lower, void *d_upper, void *d_scratch, void *stream);
/* The same search leaving only the variants that occur, as a list ordered by search index: record i =
 * {u64 lower, u64 upper, u64 index, u64 0} (32 B), index = q * (3k+1) + v (v = 0: the k-mer itself, else
 * 1 + 3*pos + the rank of the substituted base among the three alternatives) -- the (k-mer, position, base)
 * order of rsbwt_hits_1mm.  At most `cap` records are written to d_hits; *d_total (a u64 in HBM) receives how
 * many there are.  Nothing is written for the variants that end empty -- no [m][3k+1] matrices.
 * d_scratch: rsbwt_hits_1mm_scratch_bytes(h, m, k) bytes.  Nothing is synchronised. */
size_t rsbwt_hits_1mm_scratch_bytes(const rsbwt_t *h, size_t m, uint32_t k);
int rsbwt_hits_1mm_dev(rsbwt_t *h, const void *d_packed, const void *d_valid, size_t m, uint32_t k, void *d_hits,
                       size_t cap, void *d_total, void *d_scratch, void *stream);
/* Read extraction of n rows (d_rows: u64): d_out [n][stride] bytes, d_len and d_prefix_len [n] u32. */
int rsbwt_extract_dev(rsbwt_t *h, const void *d_rows, size_t n, void *d_out, uint32_t stride, void *d_len,
                      void *d_prefix_len, void *stream);

/* Measurement hooks (bench.py): wall time of the last search kernel launched through this
 * handle, from HIP events recorded on the launch stream; synchronises on the stop event. */
int rsbwt_last_search_ms(rsbwt_t *h, float *ms);
/* The same for up to `cap` of the most recent launches (the handle keeps 64 event pairs), oldest
 * first; *count receives how many were written. */
int rsbwt_search_history_ms(rsbwt_t *h, float *ms, size_t cap, size_t *count);
/* Exact work counters of the last rsbwt_find_intervals_dev launch when the handle was put
 * in counting mode with rsbwt_set_counting(h, 1): LF steps taken, Occ lookups made, distinct
 * window lines those lookups read (one 128-byte request each; a lookup whose position lies past
 * its window's line costs one more request, counted apart: word 11 of the counters below).
 * Counting mode costs atomics; leave it off when timing. */
int rsbwt_set_counting(rsbwt_t *h, int on);
int rsbwt_last_search_work(rsbwt_t *h, uint64_t *lf_steps, uint64_t *occ_lookups,
                           uint64_t *line_reads);
/* all 16 counter words: 0 LF steps, 1 Occ lookups, 2 window lines read, 3 k-mer-table starts,
 * 4..9 phase cycles (lane-pair kernel only), 10 passes, 11 continuation (spill / far) lines read,
 * 12 = 1 when the launch ran one lane per search (a full batch on a single shard behind a deep k-mer
 * table; csrc/search_solo.h), 0 on lane pairs.
 * After an rsbwt_extract_dev in counting mode the words are the walk kernels' instead: 0..7 the LF
 * (prefix) walk, 8..15 the select (postfix) walk, each {passes, lanes holding a row over those
 * passes, steps completed, lanes on a continuation line, lines fetched, cycles, cycles from issuing
 * a pass's fetches until they landed, count-word probes}, summed over the waves. */
int rsbwt_last_search_counters(rsbwt_t *h, uint64_t *words16);
/* ... and the number of k-mer-table lookups of that launch. */
int rsbwt_last_search_ktab_lookups(rsbwt_t *h, uint64_t *lookups);
/* ... and, for the wave kernel, shader cycles (s_memtime, summed over waves) spent in the six
 * phases of a pass -- set-up, load issue, wait + LDS park, overflow hops, rank, update -- plus the
 * number of passes.  Shares only: the stamps fence the pipeline. */
int rsbwt_last_search_phases(rsbwt_t *h, uint64_t *cycles6, uint64_t *passes);

/* Synthetic data (bench / tests) ----------------------------------------------- */
/* Fill d_runs (HBM) with num_runs pseudo-random RLUnit bytes: the direct run-stream
 * synthesiser for throughput runs.  Same bytes as rsbwt_synth_runs_host for the same seed.
 * Seeds with bit 63 set (RSBWT_SYNTH_LONG_RUNS | seed) give the long-run stream: mostly 31-symbol
 * units of long runs, mean ~25 symbols per unit, as in a deep population BWT. */
#define RSBWT_SYNTH_LONG_RUNS (1ull << 63)
int rsbwt_synth_runs_dev(void *d_runs, uint64_t num_runs, uint64_t seed, int device, void *stream);
int rsbwt_synth_runs_host(uint8_t *runs, uint64_t num_runs, uint64_t seed);
/* A slice of the same stream: d_runs[i] = byte first + i (a 20 GB stream piece by piece, for a checker that has no
 * room for it in HBM). */
int rsbwt_synth_runs_dev_at(void *d_runs, uint64_t first, uint64_t num_runs, uint64_t seed, int device, void *stream);
/* Draw Q k-mers that are present in the index (LF walks from random rows, so every one of the
 * k-1 updateInterval steps keeps a non-empty interval) into d_kmers (ASCII, stride bytes). */
int rsbwt_sample_present_kmers_dev(rsbwt_t *h, size_t Q, uint32_t k, size_t stride, uint64_t seed,
                                   void *d_kmers, void *stream);
/* Build a valid multi-string BWT of a synthetic read population (a base genome, haplotypes with
 * SNPs, fixed-length reads, reverse-lexicographic sort + dedup) and write it as an SGA .bwt;
 * optionally also the sorted reads, one per line.  Host only. */
int rsbwt_synth_popbwt(const char *bwt_path, const char *reads_path, uint64_t seed,
                       uint64_t genome_len, uint32_t haplotypes, double snp_rate,
                       uint32_t read_len, double coverage, int shard, int num_shards);

/* The reference's FM-index file "<bwt>.bpi2"  -------------------------------------
 * Replaces src/util/index_rlebwt.cpp:19-22 (RLEBWT(path) + serialiseFMIndex(path + ".bpi2"),
 * src/bwt/rlebwt.cpp:150-161) for deployments that keep the CPU reference next to this engine:
 * the file written is byte-identical to the reference's for the same .bwt.  Host only; the
 * engine itself never reads a .bpi2 (its device index is derived from the run bytes). */
int rsbwt_bpi2_write(const char *bwt_path, const char *bpi2_path);
/* Validates a prebuilt .bpi2 (what deserialiseFMIndex would load, rlebwt.cpp:163-200) against the
 * resident index: level shapes, C[], vSum, and the absolute counts at the start of up to
 * max_samples evenly spaced 64-run buckets (0 = all) against Occ on the GPU.  *mismatches == 0
 * means the file describes this BWT; rsbwt_last_error() names the first difference. */
int rsbwt_bpi2_check(rsbwt_t *h, const char *bpi2_path, uint64_t max_samples, uint64_t *checked,
                     uint64_t *mismatches);
/* Host only: does the file parse as a .bpi2 (what deserialiseFMIndex reads, rlebwt.cpp:163-200)?
 * RSBWT_OK, RSBWT_EIO or RSBWT_EFORMAT (truncated, trailing bytes, sizes the file cannot back). */
int rsbwt_bpi2_validate_file(const char *bpi2_path);

/* Shard sets: the shards one process holds on its GPU(s), searched with one call ------
 * Every query goes to every shard (src/service/server.cpp:124,578).  The shards of one device are
 * searched by ONE fused launch -- the batch is uploaded and packed once per device -- and devices
 * are driven concurrently.  device_map[i] = HIP device of shard i (NULL: all on device 0); the
 * deployment SURVEY 8e describes is shard s -> GPU s / 8. */
int rsbwt_set_open(const char *const *bwt_paths, size_t num_shards, const int *device_map,
                   uint32_t flags, rsbwt_set_t **out);
int rsbwt_set_from_handles(rsbwt_t *const *handles, size_t num_shards, rsbwt_set_t **out);
void rsbwt_set_close(rsbwt_set_t *s); /* closes the shards it opened itself */
size_t rsbwt_set_size(const rsbwt_set_t *s);
size_t rsbwt_set_devices(const rsbwt_set_t *s);
rsbwt_t *rsbwt_set_shard(rsbwt_set_t *s, size_t i);
/* k-mer tables for the shards that have none; depth 0 = sized per device from its free HBM: the deepest tables that
 * fit three quarters of what is free with the shards resident, leave 8 GiB, and are no larger than 5/4 of a shard's
 * lines (the depth that gives, over all devices: rsbwt_set_auto_ktab_depth) */
int rsbwt_set_attach_ktabs(rsbwt_set_t *s, uint32_t depth);
uint32_t rsbwt_set_auto_ktab_depth(rsbwt_set_t *s);
/* THE sizing rule, with the format: the depth and format (RSBWT_KTAB_FORMAT_PLAIN / _GROUPED) the set's shards that
 * have no table yet would get -- one pair for the whole set, the shallowest over its devices -- when format_in
 * (PLAIN / GROUPED / AUTO) is asked for and keep_free_bytes of each device's free HBM are to stay free (0: the set's
 * own rule, a quarter of what is free and at least 8 GiB).  What rsbwt_set_open and rsbwt_set_attach_ktabs*(depth 0)
 * build, and what bench.py / onehost.py ask instead of restating the rule.  *depth 0 = no table. */
int rsbwt_set_auto_ktab(rsbwt_set_t *s, uint32_t format_in, uint64_t keep_free_bytes, uint32_t *depth, uint32_t *format_out);
/* The same rule as plain arithmetic (host only): the deepest table of at most budget_bytes over a shard of n_symbols --
 * plain: 8 B x 4^T <= budget, 4^T <= n, T <= 16; grouped (3 B x 4^T, T <= 17) only where it is deeper than the plain
 * one, a T-mer still has 64 rows and four siblings fit a record, else plain. */
int rsbwt_auto_ktab_for_budget(uint64_t budget_bytes, uint64_t n_symbols, uint32_t format_in, uint32_t *depth, uint32_t *format_out);
/* the same with the format named (rsbwt_attach_ktab_format; rsbwt_set_attach_ktabs = PLAIN); grouped tables are
 * interleaved like plain ones: a query's records for the S shards of a device are one stretch of 12 * S bytes */
int rsbwt_set_attach_ktabs_format(rsbwt_set_t *s, uint32_t depth, uint32_t format);
/* lower/upper: [num_shards][Q]; counts: [Q] summed over shards, the way the front-end sums
 * per-partition replies (src/service/server.cpp:184-197).  With several devices the per-device sums
 * are reduced onto the first device over RCCL (ncclReduce) and cross PCIe once. */
int rsbwt_set_find_intervals(rsbwt_set_t *s, const char *kmers, size_t Q, uint32_t k,
                             size_t stride, uint64_t *lower, uint64_t *upper);
int rsbwt_set_count(rsbwt_set_t *s, const char *kmers, size_t Q, uint32_t k, size_t stride,
                    uint64_t *counts);
/* Device-resident forms for a set on ONE device: one fused launch on `stream`, nothing synchronised.
 * d_lower/d_upper/d_counts: [num_shards][Q]. */
int rsbwt_set_find_intervals_dev(rsbwt_set_t *s, const void *d_packed, const void *d_valid, size_t Q,
                                 uint32_t k, void *d_lower, void *d_upper, void *stream);
int rsbwt_set_count_dev(rsbwt_set_t *s, const void *d_packed, const void *d_valid, size_t Q, uint32_t k,
                        void *d_counts, void *stream);
/* 1-mismatch search (SURVEY 8 f3 / BASELINE configs[3]) of m packed k-mers in every shard of a one-device
 * set: d_lower/d_upper [num_shards][m][3k+1]; d_scratch: rsbwt_set_1mm_scratch_bytes(s, m, k) bytes, shared
 * by the shards' searches, which run one after the other on `stream`. */
/* The pair search in two halves, for a pipelined caller: the start records of a batch ([num_shards][Q] x 16 B =
 * rsbwt_set_records_bytes) depend on its k-mers and the k-mer tables only, so batch i + 1's can be computed on a
 * second stream (rsbwt_set_prepare_dev) while batch i is searched; the caller orders the two (an event) and
 * rsbwt_set_find_interval_pairs_prepared_dev then runs the search kernel alone.  Same answers as
 * rsbwt_set_find_interval_pairs_dev (initInterval / the k-mer table: src/bwt/query.cpp:18-21). */
size_t rsbwt_set_records_bytes(const rsbwt_set_t *s, size_t Q);
int rsbwt_set_prepare_dev(rsbwt_set_t *s, const void *d_packed, const void *d_valid, size_t Q, uint32_t k, void *d_records,
                          void *stream);
int rsbwt_set_find_interval_pairs_prepared_dev(rsbwt_set_t *s, const void *d_packed, const void *d_valid, const void *d_records,
                                               size_t Q, uint32_t k, void *d_pairs, void *stream);
size_t rsbwt_set_1mm_scratch_bytes(const rsbwt_set_t *s, size_t m, uint32_t k);
int rsbwt_set_find_intervals_1mm_dev(rsbwt_set_t *s, const void *d_packed, const void *d_valid, size_t m, uint32_t k,
                                     void *d_lower, void *d_upper, void *d_scratch, void *stream);
/* d_pairs: [num_shards][Q] x {lower, upper} */
int rsbwt_set_find_interval_pairs_dev(rsbwt_set_t *s, const void *d_packed, const void *d_valid, size_t Q,
                                      uint32_t k, void *d_pairs, void *stream);
/* Gathers per-device result blocks onto the set's first device over RCCL / xGMI (ncclSend/ncclRecv in
 * one group): d_blocks[g], bytes[g], streams[g] belong to device g of the set; d_root (first device)
 * receives the blocks back to back.  For GPU-resident consumers of all shards' intervals. */
int rsbwt_set_gather_intervals_dev(rsbwt_set_t *s, const void *const *d_blocks, const size_t *bytes,
                                   void *d_root, void *const *streams);
/* BASELINE configs[3] / configs[4] over a set that may span devices.  The reference's front-end sends every
 * request to every partition and CONCATENATES the per-partition read lists (src/service/server.cpp:124,199-261):
 * the set-level forms are every shard's own result, side by side.  Devices work concurrently, a device's shards
 * take turns; each device's lists / reads cross its own PCIe link straight into the caller's buffers.
 *
 * rsbwt_set_hits_1mm: every shard's rsbwt_hits_1mm list: hits[first[i] .. first[i+1]) = shard i's (first has
 * num_shards + 1 entries; *nhits = first[num_shards]); RSBWT_ERANGE with *nhits and first[] set when cap is short. */
int rsbwt_set_hits_1mm(rsbwt_set_t *s, const char *kmers, size_t Q, uint32_t k, size_t stride, rsbwt_hit_1mm *hits,
                       size_t cap, uint64_t *first, size_t *nhits);
/* rsbwt_extract for rows of several shards: row i = SA row rows[i] of shard shard_of[i] (the ExtractTask chunks of
 * src/service/service.cpp:729-740 of all partitions in one call). */
int rsbwt_set_extract(rsbwt_set_t *s, const uint32_t *shard_of, const uint64_t *rows, size_t n, char *out, uint32_t stride,
                      uint32_t *len, uint32_t *prefix_len);
/* rsbwt_query over every shard = find_reads of a short query (service.cpp:714-743) in every partition, the lists
 * concatenated as the front-end does: k-mer q's reads are first[q] .. first[q+1], shard 0's first, each shard's in
 * SA-row order; read_shard[r] (optional) names the shard.  cap_reads = 0 sizes the buffers (RSBWT_ERANGE, *nreads set). */
int rsbwt_set_query(rsbwt_set_t *s, const char *kmers, size_t Q, uint32_t k, size_t stride, uint64_t *first,
                    uint32_t *read_shard, char *reads, uint32_t read_stride, uint32_t *read_len, size_t cap_reads,
                    size_t *nreads);
/* Queries of LENGTHS OF THEIR OWN in one call: query q = text[off[q] .. off[q+1]) (off has Q + 1 entries).  What a window of
 * the service loop holds -- the reference answers each request with its own findInterval (src/service/service.cpp:303,
 * src/bwt/query.cpp:24-41), whatever its length -- without a launch sequence per distinct length.  Results as
 * rsbwt_set_find_intervals / rsbwt_set_count / rsbwt_set_query give them for the queries of one length; an empty query,
 * one with a symbol outside ACGT or one longer than 65,535 symbols ends as the empty interval (1, 0) / count 0 / no reads. */
int rsbwt_set_find_intervals_var(rsbwt_set_t *s, const char *text, const uint64_t *off, size_t Q, uint64_t *lower, uint64_t *upper);
int rsbwt_set_count_var(rsbwt_set_t *s, const char *text, const uint64_t *off, size_t Q, uint64_t *counts);
/* rsbwt_read_copies for queries of lengths of their own, on every shard: copies / ending [num_shards][Q] in the set's shard
 * order (ending may be NULL); several device groups work as in rsbwt_set_count_var. */
int rsbwt_set_read_copies_var(rsbwt_set_t *s, const char *text, const uint64_t *off, size_t Q, uint64_t *copies,
                              uint64_t *ending);
/* rsbwt_exactmatch_by_search on every shard of the set (the service's Reads and KmerMatch paths ask
 * rsbwt_query_exactmatch of the shards). */
int rsbwt_set_exactmatch_by_search(rsbwt_set_t *s, int on);
int rsbwt_set_query_var(rsbwt_set_t *s, const char *text, const uint64_t *off, size_t Q, uint64_t *first, uint32_t *read_shard,
                        char *reads, uint32_t read_stride, uint32_t *read_len, size_t cap_reads, size_t *nreads);
/* rsbwt_set_query_var with a limit on the rows a query may bring: matches[q] (may be NULL) = rows of query q summed over
 * the shards; max_rows > 0 and matches[q] > max_rows: the query contributes no read (first[q+1] == first[q]), matches[q]
 * still says how many there are.  max_rows == 0: no limit -- the answers of rsbwt_set_query_var.  *nreads counts the kept
 * rows only, so cap_reads = Q * max_rows always suffices.  On a set whose shards share one device the intervals never
 * leave it: totals, limit, first[] and the rows are made there (csrc/interval_rows.hip) and the walks take the rows
 * where they are; a set over several devices applies the limit on the host.  Same answers either way. */
int rsbwt_set_query_var_capped(rsbwt_set_t *s, const char *text, const uint64_t *off, size_t Q, uint64_t max_rows,
                               uint64_t *first, uint32_t *read_shard, char *reads, uint32_t read_stride,
                               uint32_t *read_len, size_t cap_reads, size_t *nreads, uint64_t *matches);
/* the expansion alone, one-device set, nothing synchronised: d_pairs = {lower, upper} [num_shards][Q] x 16 B as
 * rsbwt_set_find_interval_pairs_dev writes them; d_first u64[Q+1] and d_matches u64[Q] always written; d_shard
 * u32[cap] / d_rows u64[cap] only when first[Q] <= cap (else left untouched).  Rows in rsbwt_set_query's order:
 * query by query, shard ascending inside a query, SA row ascending inside a shard. */
int rsbwt_set_interval_rows_dev(rsbwt_set_t *s, const void *d_pairs, size_t Q, uint64_t max_rows, void *d_first,
                                void *d_matches, void *d_shard, void *d_rows, size_t cap, void *stream);
/* calling thread's last rsbwt_set_query_var_capped: {rows expanded on the device, rows uploaded from the host,
 * queries over the limit, bytes copied to the host before the extraction was launched} */
void rsbwt_set_query_last_work(uint64_t *work4);
/* Locate: WHERE a row lies.  For SA row r the LF walk of extractPrefix (src/bwt/query.cpp:49-57: while BWT[r] != '$',
 * r = C[b] + Occ(b, r) - 1) gives
 *   read_row  the row the walk ends on: the row of the read's full suffix, whose BWT symbol is '$'
 *   offset    the LF steps taken = the length extractPrefix returns = where the row's suffix starts in its read
 *   ordinal   Occ('$', read_row) - 1, in [0, num_strings): a dense number of the read inside its shard
 * A row >= bwlen, or one whose walk needs more than max_steps steps (0 = 2^20), is not located: read_row = ordinal =
 * UINT64_MAX, offset = UINT32_MAX; the call still succeeds.  Any output may be NULL, not all of them.  No read is
 * extracted: the calls need neither RSBWT_OPEN_READS nor select samples or psi hints, and build none.  The _dev forms
 * take device pointers and a stream and synchronise nothing; rsbwt_set_locate takes rows as rsbwt_set_extract does (one
 * launch per device walks all of that device's shards); rsbwt_set_locate_dev serves a set on ONE device and takes
 * d_shard u32[n] / d_rows u64[n] as rsbwt_set_interval_rows_dev writes them. */
int rsbwt_locate(rsbwt_t *h, const uint64_t *rows, size_t n, uint32_t max_steps, uint64_t *read_row, uint64_t *ordinal,
                 uint32_t *offset);
int rsbwt_locate_dev(rsbwt_t *h, const void *d_rows, size_t n, uint32_t max_steps, void *d_read_row, void *d_ordinal,
                     void *d_offset, void *stream);
int rsbwt_set_locate(rsbwt_set_t *s, const uint32_t *shard_of, const uint64_t *rows, size_t n, uint32_t max_steps,
                     uint64_t *read_row, uint64_t *ordinal, uint32_t *offset);
int rsbwt_set_locate_dev(rsbwt_set_t *s, const void *d_shard, const void *d_rows, size_t n, uint32_t max_steps,
                         void *d_read_row, void *d_ordinal, void *d_offset, void *stream);
/* The matches of queries of lengths of their own as positions instead of strings: rsbwt_set_query_var_capped's first[] /
 * read_shard[] / matches[] / limit rules and row order (query by query, shard ascending, SA row ascending); rows[t] is
 * the SA row of match t in shard read_shard[t], read_row / ordinal / offset[t] its location.  Every array of `cap`
 * entries may be NULL.  cap = 0 sizes the buffers (RSBWT_ERANGE, *nrows set).  On a one-device set search, expansion
 * and walks stay on the device; a set over several devices expands on the host.  Same answers either way. */
int rsbwt_set_locate_var_capped(rsbwt_set_t *s, const char *text, const uint64_t *off, size_t Q, uint64_t max_rows,
                                uint32_t max_steps, uint64_t *first, uint32_t *read_shard, uint64_t *rows,
                                uint64_t *read_row, uint64_t *ordinal, uint32_t *offset, size_t cap, size_t *nrows,
                                uint64_t *matches);
/* calling thread's last host-buffer locate call: {rows that ended on '$', LF steps} */
void rsbwt_locate_last_work(uint64_t *work2);
/* KmerMatch (src/service/service.cpp:466-502, find_kmer_reads; KmerTask::run :871-960) over every shard: query q =
 * text[off[q] .. off[q+1]) is tiled as get_tiles(q, k, skip) does (:232-246), every all-ACGT tile goes through
 * find_reads with no suffix filter (:714-797, min / max_read_length: 0 = 73 / 100), and the reads are folded into a
 * std::unordered_set<std::string> in the reference's insertion order.  The reads of query q in shard p are
 * first[q*S+p] .. first[q*S+p+1] (first has Q*S + 1 entries), in that set's iteration order; read r is read_len[r]
 * bytes at reads + r*read_stride (UINT32_MAX: longer than read_stride).  cap_reads = 0 sizes the buffers (RSBWT_ERANGE,
 * *nreads set).  k <= 0, skip < 0 or a query shorter than k: no reads.  Every candidate row is mapped to its read on the
 * device first and each distinct read is extracted once; rsbwt_set_kmer_last_work tells the work of the calling
 * thread's last call: {candidate rows, rows walked to '$', LF steps of those walks, distinct read identities, reads
 * extracted}. */
int rsbwt_set_kmer_reads(rsbwt_set_t *s, const char *text, const uint64_t *off, size_t Q, int32_t k, int32_t skip,
                         uint32_t min_read_length, uint32_t max_read_length, uint64_t *first, char *reads, uint32_t read_stride,
                         uint32_t *read_len, size_t cap_reads, size_t *nreads);
/* counts[q*S+p] = the size of that set (KmerTask::run's Count, :889-897) */
int rsbwt_set_kmer_count(rsbwt_set_t *s, const char *text, const uint64_t *off, size_t Q, int32_t k, int32_t skip,
                         uint32_t min_read_length, uint32_t max_read_length, uint64_t *counts);
void rsbwt_set_kmer_last_work(uint64_t *work5);
/* the same call's wall time: {total, inside the calls that wait for the device (search, exact-match, identity walks,
 * extraction), the rest = host work} in ms */
void rsbwt_set_kmer_last_times(double *ms3);
/* SiteMatch candidates: find_gt_reads (src/service/service.cpp:507-711; GtTask::run calls it once per tile, :1048-1072)
 * over every shard -- the BWT half of a SiteMatch request; the alignment (align_gt_read) stays with the caller.  Query q =
 * text[off[q] .. off[q+1]) of L symbols with its site pos[q] (1-based, as find_gt_reads receives it); k, skip and M =
 * max_interval_size (0 = 10,000, :85) hold for the call.  k <= 0, skip < 0, L < k or pos > L: the query contributes
 * nothing.  Tile i = 0 .. (L-k)/(skip+1) is w[s0:e0), s0 = (skip+1) i, e0 = s0 + k; one holding a symbol outside ACGT
 * contributes nothing.  A tile whose interval holds at most M rows is ONE leg (leg = 0).  Any other tile is lengthened
 * one symbol at a time until the interval of w[a:b) holds at most M rows -- 0 for an absent string or one that took in a
 * symbol outside ACGT, then (lower, upper) = (1, 0) -- in two legs:
 *   tile LEFT of the site (pos > e0):   leg 1 grows right; leg 2 (only if s0 > 0) takes s0 - 1 and goes on left while
 *                                       a > 0, then right;
 *   tile RIGHT of it (pos <= s0):       leg 1 grows left; leg 2 (only if e0 < L) takes e0 and goes on right while b < L,
 *                                       then left;
 *   tile COVERING it:                   leg 1 grows right only, leg 2 left only.
 * A leg that would need a < 0 or b > L has no answer and is left out (the reference loops forever or throws
 * std::out_of_range there); the tile's other leg still counts.  An empty leg carries the (lower, upper) the reference's
 * search ends with: lower = upper + 1, or -- on a shard where no '$' row lies before the rows that begin with A -- the
 * reference's (0, 2^64 - 1), which does not end a search and from which the next symbol c gives (C[c], C[c] - 1); neither
 * holds a row.  Every row j of a leg's interval is a candidate; with the
 * reference's start = a + 1 and end = b the span filter keeps it iff
 *   LEFT:   pos - end <= (|extractPostfix(j)| - k) + 4        RIGHT:   start - pos <= |extractPrefix(j)| + 4
 * (the differences in unsigned 64-bit arithmetic as the reference takes them: a leg lengthened past pos keeps no row;
 * k is the tile's length, not the lengthened string's); COVERING keeps every row.
 *   rsbwt_set_gt_legs   the legs of query q are legs[first[q] .. first[q+1]) (first has Q + 1 entries), ordered by
 *                       (tile, leg, shard); cap = 0 sizes the buffer (RSBWT_ERANGE, *nlegs set).  Needs no
 *                       RSBWT_OPEN_READS.
 *   rsbwt_set_gt_reads  the distinct read strings over the kept rows: those of query q in shard p are first[q*S+p] ..
 *                       first[q*S+p+1] (first has Q*S + 1 entries), ascending read_row (rsbwt_locate's: the row of the
 *                       read's full suffix; read_row may be NULL); a string that occurs at several read_rows is reported
 *                       once, at the lowest.  reads / read_stride / read_len as rsbwt_set_kmer_reads; cap_reads = 0 sizes
 *                       the buffers (RSBWT_ERANGE, *nreads set).
 *   rsbwt_set_gt_count  counts[q*S+p] = how many reads that is.
 * The read calls need every shard opened with RSBWT_OPEN_READS (else RSBWT_EINVAL).  A query longer than 2^31 - 1
 * symbols is RSBWT_EINVAL, and so is a candidate row whose LF walk to its read's start does not end within 2^20 steps (a
 * corrupt index): no read is left out silently.  Each device group narrows, expands, walks, filters and compacts its
 * shards' rows where they are; the legs and one record per row the filter kept come back, and each distinct read is
 * extracted once.
 * rsbwt_set_gt_last_work: the calling thread's last call: {legs, legs with no answer, LF steps spent lengthening,
 * candidate rows, rows the device's filter kept (a LEFT row stays there until its read's length decides), distinct reads
 * extracted}; a legs call leaves the last three 0, a call that finds no tile leaves all six 0. */
typedef struct rsbwt_gt_leg {
    uint64_t query;
    uint32_t tile, leg, shard; /* leg: 0 = the tile itself, 1 / 2 = the lengthened legs */
    uint32_t a, b, reserved;   /* the final string is w[a:b): the reference's start = a + 1, end = b */
    uint64_t lower, upper;     /* findInterval(w[a:b)) in that shard */
} rsbwt_gt_leg;
int rsbwt_set_gt_legs(rsbwt_set_t *s, const char *text, const uint64_t *off, size_t Q, const uint64_t *pos, int32_t k, int32_t skip,
                      uint64_t M, uint64_t *first, rsbwt_gt_leg *legs, size_t cap, size_t *nlegs);
int rsbwt_set_gt_reads(rsbwt_set_t *s, const char *text, const uint64_t *off, size_t Q, const uint64_t *pos, int32_t k, int32_t skip,
                       uint64_t M, uint64_t *first, char *reads, uint32_t read_stride, uint32_t *read_len, uint64_t *read_row,
                       size_t cap_reads, size_t *nreads);
int rsbwt_set_gt_count(rsbwt_set_t *s, const char *text, const uint64_t *off, size_t Q, const uint64_t *pos, int32_t k, int32_t skip,
                       uint64_t M, uint64_t *counts);
void rsbwt_set_gt_last_work(uint64_t *work6);
/* SiteMatch alignment: ksw_align of the reference's src/service/ksw.c as align_gt_read calls it (src/service/service.cpp:134:
 * KSW_XSTART, no KSW_XBYTE, so the 16-bit striped path ksw_i16) and align_gt_read itself (:105-225), the second half of
 * GtTask::run (:1077-1108), one GPU lane per (read, target) item.  Symbols are ASCII, coded on the device by seq_nt4_table:
 * ACGTacgt -> 0..3, anything else 4.  s(a, b) = -ambiguous where either code is 4, else +match or -mismatch.
 * One PASS P(q, t, endsc) over columns i = 0 .. tlen-1 and rows j = 0 .. qlen-1, all values >= 0, borders 0:
 *   H[i][j]   = max(0, H[i-1][j-1] + s(t[i], q[j]), E[i][j], F[i][j])
 *   E[i+1][j] = max(E[i][j] - gape, H[i][j] - (gapo + gape))      F[i][j+1] = max(F[i][j] - gape, H[i][j] - (gapo + gape))
 * (subtractions floored at 0); te = the last column whose maximum rose above every earlier column's, score = that
 * maximum; the pass stops after the column at which it reaches endsc; qe = the row of the maximum in column te, ties to
 * the smallest (j mod slen, j div slen) with slen = (qlen + 7) / 8 -- the order ksw.c:307-308 scans its striped vectors
 * in.  Nothing scores: score 0, te -1, qe 0.  ksw_align is two passes: r = P(q, t, never); rr = P(reverse(q[0..qe]), t',
 * r.score) with t' = t, its first te + 1 symbols reversed (all tlen columns stay); tb = te - rr.te and qb = qe - rr.qe
 * when rr.score == r.score, else both -1.  score2 / te2 are not produced (the service never reads them).
 *   rsbwt_ksw_align      pair i = qtext[qoff[i] .. qoff[i+1]) on the rows against ttext[toff[i] .. toff[i+1]) on the columns;
 *                        out[i] = {score, te, qe, tb, qb, 0}.  p = NULL: the service's 1, 4, 1, 6, 1; each parameter in
 *                        1..127 and each length in 1..4,096, else RSBWT_EINVAL.  A pair with match * min(qlen, tlen) >= 2^15
 *                        is RSBWT_ERANGE: the reference's 16-bit lanes saturate there, this library's packed column would
 *                        overflow.  n = 0 succeeds and touches nothing.  The items are ordered by length on the host so
 *                        that a wave's lanes finish together; out is in the caller's order.
 *   rsbwt_ksw_align_dev  the same with every array in HBM (d_qoff / d_toff u64[n + 1]); writes every byte of d_out, enqueues
 *                        on `stream` and synchronises nothing, so it cannot refuse a length: a pair outside the rules above
 *                        gets all five fields -1.  Items are taken in the caller's order.
 * A lane's column lives in LDS while its longest pass has at most RSBWT_KSW_LDS_ROWS rows, else in a scratch buffer in HBM
 * (the host call sizes it by the batch; the _dev call takes it from the stream's memory pool and gives it back there).
 *   rsbwt_gt_align       read i = reads[roff[i] .. roff[i+1]) belongs to request item[i] < Q; request q = (w = text[off[q] ..
 *                        off[q+1]), pos[q] 1-based, alt[q], isalt[q]) as GtTask::run hands them to align_gt_read after its
 *                        reverse-complement and window fix-up (:1028-1040).  verdict[i] = the exit align_gt_read leaves by,
 *                        RSBWT_GT_* in source order; KEEP_PLAIN, KEEP_RIGHT and KEEP_LEFT are its `return true`.  The
 *                        conditions are the reference's as written, the unsigned arithmetic of :158 and :196 included.
 *                        0 is never written.
 *   rsbwt_gt_align_dev   the same in HBM, enqueued on `stream`, nothing synchronised; an item the host call would refuse
 *                        gets RSBWT_GT_INVALID.
 * Where the reference is undefined this library says what it does instead:
 *   (a) the reference stores the raw character alt[0] into the CODED target (:126), which indexes past ksw's query
 *       profile; here alt[q] is coded by the nt4 table like every other symbol;
 *   (b) pos = 0 or pos > |w| writes outside the array in the reference; here it is RSBWT_GT_OFF_SITE for every read of
 *       the request;
 *   (c) a read or w outside 1..4,096 symbols, or item[i] >= Q, is RSBWT_EINVAL.
 *   rsbwt_set_gt_aligned_reads  exactly rsbwt_set_gt_reads' reads for (q, p), in its order, cut down to those align_gt_read
 *                               keeps against request q = (w, pos[q], alt[q], isalt[q]); same layout, same sizing protocol
 *                               (cap_reads = 0: RSBWT_ERANGE, *nreads set).  The alignment runs on the device of the shard
 *                               that produced the read, device groups side by side.  A candidate read or a w longer than
 *                               4,096 symbols is RSBWT_EINVAL.  Known host trip: the distinct reads come back from the
 *                               extraction and go up again for the alignment.
 *   rsbwt_set_gt_aligned_count  counts[q*S+p] = how many reads that is.
 * rsbwt_gt_align_last_work: the calling thread's last host-buffer verdict call (rsbwt_gt_align or a set call above):
 * {reads aligned, reads by verdict 1..13}; a failed call leaves all 14 zero.  NULL is harmless. */
#define RSBWT_KSW_LDS_ROWS 224
#define RSBWT_KSW_MAX_LEN 4096
#define RSBWT_GT_ALT_NOT_BETTER 1 /* looking for alt, ra.score >= r.score   :138 */
#define RSBWT_GT_REF_WORSE 2      /* looking for ref, r.score < ra.score    :143 */
#define RSBWT_GT_OFF_SITE 3       /* site outside [tb, te]                  :150 */
#define RSBWT_GT_UNALIGNED 4      /* more than 4 read bases unaligned       :158 */
#define RSBWT_GT_FLOOR_PLAIN 5    /* score floor, no indel                  :163-183 */
#define RSBWT_GT_FLOOR_INS 6      /* score floor, insertion */
#define RSBWT_GT_FLOOR_DEL 7      /* score floor, deletion */
#define RSBWT_GT_SITE_MISMATCH 8  /* mismatch at the site                   :190 */
#define RSBWT_GT_KEEP_PLAIN 9     /* KEEP, no indel */
#define RSBWT_GT_RIGHT_QB 10      /* right sub-alignment, qb != 0           :203-207 */
#define RSBWT_GT_KEEP_RIGHT 11    /* KEEP, right sub-alignment */
#define RSBWT_GT_LEFT_QE 12       /* left sub-alignment, qe + 1 != len      :216-220 */
#define RSBWT_GT_KEEP_LEFT 13     /* KEEP, left sub-alignment */
#define RSBWT_GT_INVALID 255      /* (the _dev call only) */
typedef struct rsbwt_ksw_params {
    int32_t match, mismatch, ambiguous, gapo, gape; /* penalties as positive numbers */
} rsbwt_ksw_params;
typedef struct rsbwt_ksw_result {
    int32_t score, te, qe, tb, qb, reserved;
} rsbwt_ksw_result;
int rsbwt_ksw_align(int device, const rsbwt_ksw_params *p, const char *qtext, const uint64_t *qoff, const char *ttext, const uint64_t *toff,
                    size_t n, rsbwt_ksw_result *out);
int rsbwt_ksw_align_dev(const rsbwt_ksw_params *p, const void *d_qtext, const void *d_qoff, const void *d_ttext, const void *d_toff, size_t n,
                        void *d_out, int device, void *stream);
int rsbwt_gt_align(int device, const char *reads, const uint64_t *roff, const uint64_t *item, size_t n, const char *text, const uint64_t *off,
                   const uint64_t *pos, const char *alt, const uint8_t *isalt, size_t Q, uint8_t *verdict);
int rsbwt_gt_align_dev(const void *d_reads, const void *d_roff, const void *d_item, size_t n, const void *d_text, const void *d_off,
                       const void *d_pos, const void *d_alt, const void *d_isalt, size_t Q, void *d_verdict, int device, void *stream);
int rsbwt_set_gt_aligned_reads(rsbwt_set_t *s, const char *text, const uint64_t *off, size_t Q, const uint64_t *pos, const char *alt,
                               const uint8_t *isalt, int32_t k, int32_t skip, uint64_t M, uint64_t *first, char *reads, uint32_t read_stride,
                               uint32_t *read_len, uint64_t *read_row, size_t cap_reads, size_t *nreads);
int rsbwt_set_gt_aligned_count(rsbwt_set_t *s, const char *text, const uint64_t *off, size_t Q, const uint64_t *pos, const char *alt,
                               const uint8_t *isalt, int32_t k, int32_t skip, uint64_t M, uint64_t *counts);
void rsbwt_gt_align_last_work(uint64_t *work14);
/* Matching statistics: for every END position of a batch of queries and every shard, the longest string ending there
 * that the shard still supports, and its interval -- "how much of this sequence do the reads support, and where does the
 * support break".  Queries arrive as in the _var calls: text, off[Q + 1], N = off[Q] - off[0] positions; position t in
 * [0, N) belongs to query q with off[q] <= off[0] + t < off[q+1], and its end is e = off[0] + t - off[q] + 1.  W_p(x) is
 * the number of rows of findInterval(x) in shard p by this header's rule for an interval (lower <= upper && upper <
 * bwlen ? upper - lower + 1 : 0), and 0 for a string that holds a symbol outside ACGT.  m = max(min_rows, 1); cap =
 * max_len, 0 = no cap.
 *   len[p*N + t]            the largest l in [0, min(e, cap)] such that x = the l symbols ending at position t is all
 *                           ACGT and W_p(x) >= m
 *   lower / upper[p*N + t]  findInterval(x) in shard p; (1, 0) where l = 0
 *   SMEM                    position t is a super-maximal exact match of its shard iff len > 0 and either the query ends
 *                           at t or len[t+1] <= len[t].  The starts t - len[t] never decrease along a query, so a match
 *                           lies inside another exactly when the next position's match has the same start; a match that
 *                           stops at cap counts as maximal under the cap.
 * W cannot grow when a string grows to the left: Occ(c, upper) - Occ(c, lower - 1) <= upper - lower + 1 for any run
 * stream, a valid BWT or not.  So the largest l is where the first LF step fails; the search never looks past it, and
 * the definition holds on synthetic run streams too.  The search starts from the shard's k-mer table where the match is
 * at least that deep and from initInterval elsewhere: same answers with any table or none.
 *   rsbwt_set_match_lengths      len u32[S][N]; lower / upper u64[S][N] may be NULL, both or neither
 *   rsbwt_match_lengths          one handle = a set of one
 *   rsbwt_set_match_lengths_dev  a set on ONE device; d_text, d_off (u64[Q + 1], d_off[0] = 0, d_off[Q] = N) and the
 *                                outputs in HBM: d_len u32[S][N], d_pairs {lower, upper}[S][N] (16 bytes each; may be
 *                                NULL); enqueues on `stream`, synchronises nothing
 *   rsbwt_set_smems              the SMEMs of query q in shard p are out[first[q*S+p] .. first[q*S+p+1]) (first has Q*S + 1
 *                                entries), ascending end: the match is text[off[q]+start .. off[q]+end).  cap = 0 sizes
 *                                the buffer (RSBWT_ERANGE, *nsmems set).  Only the SMEMs' records leave the device.
 * Q = 0 or N = 0 succeeds and touches no output array (rsbwt_set_smems sets *nsmems = 0 and zeroes first[]).  A query longer
 * than 2^31 - 1 symbols is RSBWT_EINVAL, 2^31 positions or more in one call RSBWT_ERANGE.  No call needs RSBWT_OPEN_READS
 * or a k-mer table; they build nothing and write nothing a search reads, and are re-entrant like the other set calls.
 * rsbwt_set_match_last_work: the calling thread's last host-buffer call: {items = positions x shards, LF steps, lane-passes
 * that fetched a line, starts from a k-mer table entry, restarts from initInterval after a table entry was refused,
 * SMEMs}. */
typedef struct rsbwt_smem {
    uint64_t query;
    uint32_t shard, start, end, reserved; /* the match is query[start:end) */
    uint64_t lower, upper;                /* its interval in that shard */
} rsbwt_smem;
int rsbwt_set_match_lengths(rsbwt_set_t *s, const char *text, const uint64_t *off, size_t Q, uint32_t max_len, uint64_t min_rows,
                            uint32_t *len, uint64_t *lower, uint64_t *upper);
int rsbwt_set_match_lengths_dev(rsbwt_set_t *s, const void *d_text, const void *d_off, size_t Q, size_t N, uint32_t max_len,
                                uint64_t min_rows, void *d_len, void *d_pairs, void *stream);
int rsbwt_set_smems(rsbwt_set_t *s, const char *text, const uint64_t *off, size_t Q, uint32_t max_len, uint64_t min_rows,
                    uint64_t *first, rsbwt_smem *out, size_t cap, size_t *nsmems);
int rsbwt_match_lengths(rsbwt_t *h, const char *text, const uint64_t *off, size_t Q, uint32_t max_len, uint64_t min_rows,
                        uint32_t *len, uint64_t *lower, uint64_t *upper);
void rsbwt_set_match_last_work(uint64_t *work6);
/* Overlaps: the reads that BEGIN with a suffix of a query -- "which reads continue this sequence past its end", the
 * suffix-prefix overlaps an assembler walks.  Queries arrive as in the _var calls: text, off[Q + 1], N = off[Q] - off[0]
 * positions; position t in [0, N) belongs to query q as in rsbwt_set_match_lengths (off[q] <= off[0] + t < off[q+1]) and
 * names the suffix of its query that starts there: x = text[off[0]+t .. off[q+1]), of length l = off[q+1] - off[0] - t.
 * limit = max_overlap, 0 = no limit.  For shard p:
 *   count[p*N + t]    Occ('$', upper) - Occ('$', lower - 1) over (lower, upper) = findInterval(x), Occ(., -1) = 0, when
 *                     l >= max(min_overlap, 1), l <= limit (if one is set), x is all ACGT and the interval is proper by
 *                     this header's rule (lower <= upper && upper < bwlen); 0 in every other case.  In a multi-string
 *                     BWT a row of the interval holds '$' exactly when a read begins with x there, so this is the
 *                     number of reads of the shard that begin with x.
 *   ordinal[p*N + t]  Occ('$', lower - 1) where count > 0, else 0.  The reads are the ordinals [ordinal, ordinal + count),
 *                     the dense numbers rsbwt_locate reports: for each such o the row getOccAt('$', o + 1) lies in the
 *                     interval, has offset 0 and extracts as that read.
 * A read equal to x counts (it begins with x).  A shard without '$' rows gives 0 everywhere.  The definition goes through
 * Occ, so it holds on synthetic run streams too.  One backward search of a query from its right end passes through the
 * interval of every suffix, and the '$' ranks are taken at the positions the next LF step ranks its own symbol at: the
 * profile of a query costs one search.  The search ends at the first improper interval, at the limit or at a symbol
 * outside ACGT; it starts from the shard's k-mer table of depth T only when T >= 2, min_overlap >= T and
 * min(query length, limit) >= T, so no depth that could be reported is skipped: same answers with any table or none.
 *   rsbwt_set_overlaps         count u64[S][N]; ordinal u64[S][N] may be NULL
 *   rsbwt_overlaps             one handle = a set of one
 *   rsbwt_set_overlaps_dev     a set on ONE device; d_text, d_off (u64[Q + 1], d_off[0] = 0, d_off[Q] = N) and the output
 *                              in HBM: d_pairs {ordinal, count}[S][N] (16 bytes each, every entry written); enqueues on
 *                              `stream`, synchronises nothing
 *   rsbwt_set_overlap_records  the entries with count > 0 as records: those of query q in shard p are out[first[q*S+p] ..
 *                              first[q*S+p+1]) (first has Q*S + 1 entries), ascending start -- the longest overlap first.
 *                              cap = 0 sizes the buffer (RSBWT_ERANGE, *nrecords set).  Only the records leave the device.
 *   rsbwt_set_overlap_reads    the reads themselves: those of (q, p) are entries first[q*S+p] .. first[q*S+p+1) of reads
 *                              (read_stride bytes each), read_len, overlap (the length of the LONGEST suffix of the query
 *                              the read begins with) and ordinal.  A read is reported once per (query, shard) -- a
 *                              periodic query makes one read begin with several suffixes -- ordered by overlap descending,
 *                              then ordinal ascending.  matches[q*S+p] (may be NULL) = the number of distinct reads; a
 *                              (query, shard) with more than max_reads of them (0 = no limit) reports none and empties
 *                              nobody else (rsbwt_set_query_var_capped's rule).  cap_reads = 0 sizes the buffers
 *                              (RSBWT_ERANGE, *nreads set).  Every shard must be opened with RSBWT_OPEN_READS, else
 *                              RSBWT_EINVAL; no other call here needs that.
 * Q = 0 or N = 0 succeeds and touches no output array (the sizing calls set their count to 0 and zero first[]).  A query
 * longer than 2^31 - 1 symbols is RSBWT_EINVAL, 2^31 positions or more in one call RSBWT_ERANGE, no device RSBWT_ENODEV.
 * The calls build nothing and write nothing a search reads, and are re-entrant like the other set calls.
 * rsbwt_set_overlap_last_work: the calling thread's last host-buffer call: {items = queries x shards, LF steps,
 * lane-passes that fetched a line, starts from a k-mer table entry, lane-passes fetched for '$' alone, entries with
 * count > 0}. */
typedef struct rsbwt_overlap {
    uint64_t query;
    uint32_t shard, start, length, reserved; /* the suffix is query[start : start+length) */
    uint64_t ordinal, count;                 /* reads [ordinal, ordinal + count) of that shard begin with it */
    uint64_t lower, upper;                   /* its interval */
} rsbwt_overlap;                             /* 56 bytes */
int rsbwt_set_overlaps(rsbwt_set_t *s, const char *text, const uint64_t *off, size_t Q, uint32_t min_overlap, uint32_t max_overlap,
                       uint64_t *count, uint64_t *ordinal);
int rsbwt_overlaps(rsbwt_t *h, const char *text, const uint64_t *off, size_t Q, uint32_t min_overlap, uint32_t max_overlap, uint64_t *count,
                   uint64_t *ordinal);
int rsbwt_set_overlaps_dev(rsbwt_set_t *s, const void *d_text, const void *d_off, size_t Q, size_t N, uint32_t min_overlap,
                           uint32_t max_overlap, void *d_pairs, void *stream);
int rsbwt_set_overlap_records(rsbwt_set_t *s, const char *text, const uint64_t *off, size_t Q, uint32_t min_overlap, uint32_t max_overlap,
                              uint64_t *first, rsbwt_overlap *out, size_t cap, size_t *nrecords);
int rsbwt_set_overlap_reads(rsbwt_set_t *s, const char *text, const uint64_t *off, size_t Q, uint32_t min_overlap, uint32_t max_overlap,
                            uint64_t max_reads, uint64_t *first, char *reads, uint32_t read_stride, uint32_t *read_len, uint32_t *overlap,
                            uint64_t *ordinal, size_t cap_reads, size_t *nreads, uint64_t *matches);
void rsbwt_set_overlap_last_work(uint64_t *work6);
/* Extensions and walks: "what do the reads say comes next?" -- local assembly round a k-mer, the haplotypes either side of a
 * site, the gap between two anchors.  Queries (seeds) arrive as in the _var calls: text, off[Q + 1].
 *   ctx    the context length, 1 <= ctx <= 255
 *   flags  bit 0 RSBWT_WALK_LEFT: walk to the left; bit 1 RSBWT_WALK_BOTH_STRANDS: count the reverse complement too
 * W_p(x) = the rows of findInterval(x) in shard p by this header's rule (lower <= upper && upper < bwlen ? upper - lower + 1
 * : 0), so the wrapped (0, 2^64-1) counts 0; rc(x) = the reverse complement of x.  For a string s with |s| >= ctx whose
 * context is all ACGT the four CANDIDATES are
 *   x_c = s[-ctx:] + c   walking right
 *   x_c = c + s[:ctx]    walking left          c = A, C, G, T in that order
 * the EXTENSION COUNT is E_p(s, c) = W_p(x_c), plus W_p(rc(x_c)) with both strands, and the SUPPORT is sup(s, c) = the sum of
 * E_p(s, c) over every shard of the set.  A seed shorter than ctx, or with a symbol outside ACGT in its context (the ctx
 * symbols a candidate holds: an N elsewhere does not matter), is INVALID: its counts are all 0.
 *   rsbwt_set_extensions  counts u64[S][Q][4]: counts[(p*Q + q)*4 + c] = E_p(query q, c).  The one-step primitive; any set,
 *                         device groups side by side like the other set calls.
 *   rsbwt_extensions      one handle = a set of one: counts u64[Q][4]
 *   rsbwt_set_walk        walks every seed: m = max(min_count, 1); s = seed; repeat
 *                           1. max_steps symbols appended: stop with RSBWT_WALK_LIMIT
 *                           2. evaluate the four supports;  live = {c : sup(s, c) >= m}
 *                           3. live empty: stop with RSBWT_WALK_DEAD_END;  two or more: stop with RSBWT_WALK_BRANCH
 *                           4. else append the one live symbol to s on the walking side and note its support
 *                         An invalid seed stops with RSBWT_WALK_INVALID at 0 steps.
 *                           ext      char[Q][max_steps]: the appended symbols in the order they were appended (a left walk's
 *                                    sequence is reverse(ext) + seed); bytes past steps[q] are 0
 *                           steps    u32[Q]
 *                           stop     u8[Q], one of RSBWT_WALK_*; 0 is never written
 *                           support  u32[Q][max_steps], may be NULL: the support of each appended symbol, saturated at
 *                                    2^32 - 1; 0 past steps[q]
 *                           last     u64[Q][4], may be NULL: the four supports of the evaluation that stopped the walk,
 *                                    zeros for LIMIT and INVALID
 *                         On a set on one device the whole walk is ONE launch; over several device groups each group
 *                         evaluates one step of the seeds still walking (rsbwt_set_extensions' kernel), the host sums,
 *                         applies the rule and goes again: the same outputs, one round trip per step.
 *   rsbwt_set_walk_dev    a set on ONE device (several: RSBWT_EINVAL); d_text, d_off (u64[Q + 1], d_off[0] = 0, d_off[Q] = N)
 *                         and the outputs in HBM (d_support, d_last may be NULL); every byte of every output is written;
 *                         enqueues on `stream`, synchronises nothing
 * Q = 0 succeeds and touches nothing.  ctx outside 1..255, max_steps 0 or above 65,535 and unknown flag bits are RSBWT_EINVAL;
 * Q x max_steps >= 2^31 is RSBWT_ERANGE; no device RSBWT_ENODEV.  No call needs RSBWT_OPEN_READS or a k-mer table; they build
 * nothing and write nothing a search reads, and are re-entrant like the other set calls.  A candidate's search may start from
 * the shard's k-mer table entry of its last T symbols when T >= 2 and ctx + 1 >= T (a refused entry starts over from
 * initInterval): same answers with any table or none.  A search ends at the step that empties it and looks at nothing past
 * that step.
 * rsbwt_set_walk_last_work: the calling thread's last host-buffer walk or extensions call: {seeds, appended symbols,
 * candidate searches, LF steps, lane-passes that fetched a line, starts from a k-mer table entry}. */
#define RSBWT_WALK_LEFT 1u
#define RSBWT_WALK_BOTH_STRANDS 2u
#define RSBWT_WALK_DEAD_END 1
#define RSBWT_WALK_BRANCH 2
#define RSBWT_WALK_LIMIT 3
#define RSBWT_WALK_INVALID 4
int rsbwt_set_extensions(rsbwt_set_t *s, const char *text, const uint64_t *off, size_t Q, uint32_t ctx, uint32_t flags, uint64_t *counts);
int rsbwt_extensions(rsbwt_t *h, const char *text, const uint64_t *off, size_t Q, uint32_t ctx, uint32_t flags, uint64_t *counts);
int rsbwt_set_walk(rsbwt_set_t *s, const char *text, const uint64_t *off, size_t Q, uint32_t ctx, uint64_t min_count, uint32_t max_steps,
                   uint32_t flags, char *ext, uint32_t *steps, uint8_t *stop, uint32_t *support, uint64_t *last);
int rsbwt_set_walk_dev(rsbwt_set_t *s, const void *d_text, const void *d_off, size_t Q, size_t N, uint32_t ctx, uint64_t min_count,
                       uint32_t max_steps, uint32_t flags, void *d_ext, void *d_steps, void *d_stop, void *d_support, void *d_last,
                       void *stream);
void rsbwt_set_walk_last_work(uint64_t *work6);
/* Unitigs: the maximal unbranched stretch of the reads' k-mer graph through a seed.  A walk follows out-edges only and
 * runs through a node that two paths enter; a unitig stops on both sides where the graph forks onward, where another path
 * JOINS, or where the path ends.  W_p, rc, the candidates, E_p, sup, "invalid" and m = max(min_count, 1) are the walk
 * section's above.
 * Every seed s has two SIDES: side 0 walks right, side 1 walks left.  Each side is independent of the other and both start
 * from the seed as given: the right side looks at s[-ctx:] only, the left side at s[:ctx] only.  A side whose own context
 * is missing (|s| < ctx) or holds a symbol outside ACGT stops with RSBWT_WALK_INVALID at 0 steps; the other side may still
 * be valid.  One side, with t = s, repeats
 *   1. max_steps symbols appended on this side: stop with RSBWT_WALK_LIMIT; no evaluation is made
 *   2. the ONWARD evaluation: the four supports of t in the side's direction, exactly the walk's step;
 *      live = {c : sup(t, c) >= m}
 *   3. live empty: stop with RSBWT_WALK_DEAD_END;  two or more: stop with RSBWT_WALK_BRANCH
 *   4. else c = the one live symbol, t' = t + c walking right, c + t walking left, and v = the NODE entered: t'[-ctx:]
 *      walking right, t'[:ctx] walking left.  The RETURN evaluation: the four supports of the string v in the OPPOSITE
 *      direction -- walking right the candidates b + v, walking left v + b; all four are searched, the known one (b0 =
 *      t[-ctx] walking right, t[ctx-1] walking left: the same string as c's onward candidate, so its support is
 *      sup(t, c)) included.  Two or more return supports >= m: stop with RSBWT_WALK_JOIN; c is NOT appended, the
 *      unitig ends at the node before the join
 *   5. else append c, note its onward support saturated at 2^32 - 1, t = t', go to 1
 * A seed's interior is taken as given and is not checked; a cycle ends with LIMIT.  The unitig's sequence is
 * reverse(ext of side 1) + seed + (ext of side 0).
 *   rsbwt_set_unitigs      with i = 2 * q + side:
 *                            ext      char[Q][2][max_steps]: the symbols appended on that side in the order they were
 *                                     appended; 0 past steps[i]
 *                            steps    u32[Q][2]
 *                            stop     u8[Q][2], one of RSBWT_WALK_*; 0 is never written
 *                            support  u32[Q][2][max_steps], may be NULL; 0 past steps[i]
 *                            last     u64[Q][2][8], may be NULL: [0..3] the onward supports of the evaluation that stopped
 *                                     the side, [4..7] the return supports when the stop is JOIN, zeros otherwise; all eight
 *                                     zero for LIMIT and INVALID
 *                          On a set on one device both sides of every seed advance in ONE launch (the unit of work is the
 *                          item (seed, side), so a dependent chain is one side long); over several device groups each group
 *                          evaluates with rsbwt_set_extensions' kernel -- the onward contexts of the items still walking,
 *                          grouped by direction, then the nodes entered in the opposite direction -- and the host sums and
 *                          decides: the same outputs and counters, round trips per step.
 *   rsbwt_set_unitigs_dev  a set on ONE device (several: RSBWT_EINVAL); inputs and outputs in HBM as for
 *                          rsbwt_set_walk_dev; every byte of every output is written; enqueues on `stream`, synchronises
 *                          nothing
 * flags accepts RSBWT_WALK_BOTH_STRANDS only: RSBWT_WALK_LEFT and unknown bits are RSBWT_EINVAL.  ctx outside 1..255,
 * max_steps (per side) 0 or above 65,535, a NULL required pointer with Q > 0 and offsets that run backwards are
 * RSBWT_EINVAL; 2 x Q x max_steps >= 2^31 is RSBWT_ERANGE, refused before anything is read; Q = 0 succeeds and touches
 * nothing; no device RSBWT_ENODEV.  The calls need neither RSBWT_OPEN_READS nor a k-mer table (same answers with any table
 * or none), build nothing, write nothing a search reads and are re-entrant.  There is no single-handle form: a set of one
 * serves.
 * rsbwt_set_unitig_last_work: the calling thread's last host-buffer call: {seeds, appended symbols, candidate searches, LF
 * steps, lane-passes that fetched a line, starts from a k-mer table entry, onward evaluations, return evaluations}.
 * Measured on one MI355X (tools/unitig_probe.py, profiles/unitig_probe.json): 10^4 seeds of 31, ctx 30, 200 steps
 * a side, both strands, on a popBWT of 3.0e7 symbols: 116 ms as one shard, 1,069 ms dealt to eight (the call is its launch);
 * rsbwt_set_walk right plus left on the same seeds takes 100 and 481 ms, a host loop of rsbwt_set_extensions 637 and 1,364 ms. */
#define RSBWT_WALK_JOIN 5
int rsbwt_set_unitigs(rsbwt_set_t *s, const char *text, const uint64_t *off, size_t Q, uint32_t ctx, uint64_t min_count, uint32_t max_steps,
                      uint32_t flags, char *ext, uint32_t *steps, uint8_t *stop, uint32_t *support, uint64_t *last);
int rsbwt_set_unitigs_dev(rsbwt_set_t *s, const void *d_text, const void *d_off, size_t Q, size_t N, uint32_t ctx, uint64_t min_count,
                          uint32_t max_steps, uint32_t flags, void *d_ext, void *d_steps, void *d_stop, void *d_support, void *d_last,
                          void *stream);
void rsbwt_set_unitig_last_work(uint64_t *work8);
/* Paths: every path from a seed, through the forks, depth first -- the alleles between two anchors read off the reads (a SNP
 * is two paths of equal length, an indel two of different length).  W_p, rc, the candidates, E_p, sup, "invalid",
 * m = max(min_count, 1) and the flags RSBWT_WALK_LEFT / RSBWT_WALK_BOTH_STRANDS are the walk section's above.
 *   max_steps  the symbols a path may append, 1..65,535
 *   max_paths  the paths a seed may put out, 1..256
 *   max_evals  the evaluations (of four supports each) a seed may make, 1..2^20
 *   ttext, toff[Q + 1]  an optional TARGET per seed, both NULL = no targets: target q = ttext[toff[q] .. toff[q+1]); a target of
 *              no symbols = none for that seed; one longer than ctx is RSBWT_EINVAL; one holding a symbol outside ACGT never
 *              matches
 * Per seed, with seq = seed + path walking right and reverse(path) + seed walking left:
 *   an invalid seed: state RSBWT_PATHS_INVALID, 0 paths
 *   path = "", pend = {}, evals = 0, out = []
 *   loop:
 *     if target and len(path) >= 1 and the len(target) symbols at the walking end of seq == target:  stop = RSBWT_WALK_TARGET
 *     elif len(path) == max_steps:                                                                    stop = RSBWT_WALK_LIMIT
 *     elif evals == max_evals:                                                                        stop = RSBWT_WALK_BUDGET
 *     else:
 *        evals += 1; evaluate the four supports of seq; live = [c in A, C, G, T order : sup(seq, c) >= m]
 *        if live is empty: stop = RSBWT_WALK_DEAD_END
 *        else: pend[len(path)] = live[1:] (if any); path += live[0]; continue
 *     out.append((path, stop, the least support of the path's symbols saturated at 2^32 - 1; 0 for a path of no symbols))
 *     if stop == RSBWT_WALK_BUDGET:  state RSBWT_PATHS_BUDGET;    done
 *     if pend is empty:              state RSBWT_PATHS_COMPLETE;  done
 *     if len(out) == max_paths:      state RSBWT_PATHS_MORE;      done
 *     d = the deepest depth in pend; c = its first untried symbol (removed); path = path[:d] + c
 * The paths come depth first in pre-order with A < C < G < T at every fork: the output is a function of the supports alone.
 * A cycle ends with LIMIT; the target is not tested at 0 steps (the seed is the source anchor); the order of the three end
 * tests and of the three "done" tests is part of the definition (csrc/paths_rule.h states them once for device and host).
 *   rsbwt_set_paths      ext          char[Q][max_paths][max_steps]: path j of seed q in the order its symbols were appended
 *                                     (walking left the sequence is reverse(ext) + seed); 0 past a path's steps and in
 *                                     unused slots
 *                        steps        u32[Q][max_paths]; 0 in unused slots
 *                        stop         u8[Q][max_paths]: RSBWT_WALK_DEAD_END, _LIMIT, _TARGET or _BUDGET; 0 in unused slots
 *                        min_support  u32[Q][max_paths], may be NULL; 0 in unused slots
 *                        npaths       u32[Q]
 *                        state        u8[Q], one of RSBWT_PATHS_*; 0 is never written
 *                      On a set on one device the whole search of every seed is ONE launch: a workgroup per 8 seeds, a
 *                      seed's paths written into their own slots as they grow, its untried symbols in HBM scratch of
 *                      min(max_steps, max_evals) x 32 bytes per seed; over several device groups each group evaluates the
 *                      current node of the seeds still searching (rsbwt_set_extensions' kernel), the host sums, applies
 *                      csrc/paths_rule.h and goes again: the same outputs and counters, one round trip per evaluation.
 *   rsbwt_set_paths_dev  a set on ONE device (several: RSBWT_EINVAL); d_text, d_off (u64[Q + 1], d_off[0] = 0, d_off[Q] = N),
 *                        d_ttext, d_toff (both NULL, or u64[Q + 1] with d_toff[0] = 0, d_toff[Q] = TN) and the outputs in HBM
 *                        (d_min_support may be NULL); every byte of every output is written; enqueues on `stream`,
 *                        synchronises nothing.  The lengths are not on the host here: a target longer than ctx is not
 *                        refused, it never matches.
 * Unknown flag bits, ctx outside 1..255, max_steps, max_paths or max_evals outside their ranges, a NULL required pointer with
 * Q > 0 (one of ttext, toff without the other included) and offsets that run backwards are RSBWT_EINVAL;
 * Q x max_paths x max_steps >= 2^31 is RSBWT_ERANGE, refused before anything is read; Q = 0 succeeds and touches nothing; no
 * device RSBWT_ENODEV.  The calls need neither RSBWT_OPEN_READS nor a k-mer table (same answers with any table or none), build
 * nothing, write nothing a search reads and are re-entrant.  There is no single-handle form: a set of one serves.
 * rsbwt_set_paths_last_work: the calling thread's last host-buffer call: {seeds, symbols appended (every symbol put at the end
 * of a path: the first live symbol of an evaluation and the symbol a backtrack takes up), candidate searches, LF steps,
 * lane-passes that fetched a line, starts from a k-mer table entry, evaluations, paths}.
 * Measured on one MI355X (tools/paths_probe.py, profiles/paths_probe.json): 10^4 seeds of 31 walking right, ctx 30,
 * targets ending 60 symbols past the seed, max_steps 200, max_paths 8, max_evals 800, both strands, on a popBWT of 3.0e7
 * symbols: 50 ms as one shard, 204 ms dealt to eight; a depth-first host loop of rsbwt_set_extensions that gives the same
 * answers takes 409 and 528 ms (8.2 and 2.6 times the call). */
#define RSBWT_WALK_TARGET 6
#define RSBWT_WALK_BUDGET 7
#define RSBWT_PATHS_COMPLETE 1
#define RSBWT_PATHS_MORE 2
#define RSBWT_PATHS_BUDGET 3
#define RSBWT_PATHS_INVALID 4
int rsbwt_set_paths(rsbwt_set_t *s, const char *text, const uint64_t *off, size_t Q, const char *ttext, const uint64_t *toff, uint32_t ctx,
                    uint64_t min_count, uint32_t max_steps, uint32_t max_paths, uint32_t max_evals, uint32_t flags, char *ext, uint32_t *steps,
                    uint8_t *stop, uint32_t *min_support, uint32_t *npaths, uint8_t *state);
int rsbwt_set_paths_dev(rsbwt_set_t *s, const void *d_text, const void *d_off, size_t Q, size_t N, const void *d_ttext, const void *d_toff,
                        size_t TN, uint32_t ctx, uint64_t min_count, uint32_t max_steps, uint32_t max_paths, uint32_t max_evals, uint32_t flags,
                        void *d_ext, void *d_steps, void *d_stop, void *d_min_support, void *d_npaths, void *d_state, void *stream);
void rsbwt_set_paths_last_work(uint64_t *work8);
/* The per-read sample table: "which samples carry this read".  Replaces, for the return types All and Samples, the
 * RocksDB lookups of the reference -- sdb->Get(read, &value) in QueryTask::run (src/service/service.cpp:1292-1348), KmerTask::run
 * (:917-975) and DbTask::run (:816-845) -- by a table in HBM keyed by the read's ordinal: per shard off u64[num_strings + 1]
 * and the value bytes back to back, the value of ordinal o = bytes[off[o] .. off[o+1]).  The table holds raw bytes; what a
 * record is (size_of_sample, has_other_meta_data) only the Reply encoder below knows.  Each shard's table lives on that
 * shard's device.  The FM index is the hash from read string to ordinal: (ordinal, copies) of a string come from the
 * whole-read search of rsbwt_read_copies, ordinal = Occ('$', lower - 1) -- rsbwt_locate's and rsbwt_set_overlaps' number.
 *   rsbwt_set_meta_build       pair i = read text[off[i] .. off[i+1]) with value values[voff[i] .. voff[i+1]).  In every shard
 *                              every ordinal of [ordinal, ordinal + copies) takes the value (all copies of a string share one
 *                              RocksDB key).  A string given twice: the pair with the higher index wins (batch.Put overwrites,
 *                              src/util/load_data_into_rocksdb.cpp:50), whatever the order the GPU takes them in.  A string that
 *                              is empty, holds a symbol outside ACGT, is longer than 65,535 symbols or matches no shard is
 *                              counted and changes nothing; an ordinal no pair reaches has an empty value.  A second build
 *                              replaces the table.  stats4 (may be NULL) = {pairs that matched at least one shard, pairs that
 *                              matched none, ordinals given a value (an empty one included), value bytes stored}.
 *   rsbwt_set_meta_load        the same from the file load_data_into_rocksdb reads: line 1 a read, line 2 its value up to the
 *                              newline, repeated (:44); a last read without a value line is ignored, '\r' is a byte like any
 *                              other, "the higher index wins" holds over the whole file.  RSBWT_EIO: unreadable.
 *   rsbwt_set_meta_clear       frees the table.
 *   rsbwt_set_meta_bytes       its bytes in HBM over all shards (0: none).
 * BUILD, LOAD AND CLEAR MUST NOT RUN BESIDE A LOOKUP (or each other) ON THE SAME SET: they replace what the lookups read.
 * The lookups are re-entrant like the other set calls, need neither RSBWT_OPEN_READS nor a k-mer table, and use no atomics:
 *   rsbwt_set_read_ordinals_var   rsbwt_set_read_copies_var with one more output: ordinal / copies u64[S][Q] in the set's
 *                                 shard order; ordinal = Occ('$', lower - 1) where copies > 0, else 0.  The same search.
 *   rsbwt_set_meta_by_ordinal     item i = ordinal[i] of shard shard_of[i]; first has n + 1 entries, the value of item i is
 *                                 bytes[first[i] .. first[i+1]), in the order asked; an ordinal may be asked any number of
 *                                 times.  An ordinal >= num_strings or UINT64_MAX (locate's "not located"): empty.  A shard
 *                                 index out of range: RSBWT_EINVAL; a set without a table: RSBWT_EINVAL ("no sample table").
 *                                 cap too small (cap = 0 sizes the buffer): RSBWT_ERANGE with *nbytes and first[] set.
 *   rsbwt_set_meta_by_ordinal_dev a set on ONE device; d_shard u32[n] / d_ordinal u64[n] as rsbwt_set_interval_rows_dev and
 *                                 rsbwt_set_locate_dev write them; d_first u64[n + 1] is always written, d_bytes only when
 *                                 d_first[n] <= cap; a shard index out of range gives an empty value.  Enqueues on `stream`,
 *                                 synchronises nothing.
 *   rsbwt_set_read_meta_var       strings in, values out: the value of query q in shard p is item q * S + p (first has
 *                                 Q * S + 1 entries, the layout of the KmerMatch calls), taken at the read's FIRST ordinal,
 *                                 empty where copies == 0; copies u64[S][Q] may be NULL.  On a one-device set search, sizing,
 *                                 scan and copy stay on the device: first[] and the bytes come back.
 *   rsbwt_set_meta_last_work      the calling thread's last lookup call: {items, items with a value, value bytes copied, LF
 *                                 steps of the string searches (counted only while rsbwt_set_set_counting is on, else 0)}. */
int rsbwt_set_meta_build(rsbwt_set_t *s, const char *text, const uint64_t *off, const uint8_t *values, const uint64_t *voff, size_t n,
                         uint64_t *stats4);
int rsbwt_set_meta_load(rsbwt_set_t *s, const char *path, uint64_t *stats4);
int rsbwt_set_meta_clear(rsbwt_set_t *s);
uint64_t rsbwt_set_meta_bytes(const rsbwt_set_t *s);
int rsbwt_set_read_ordinals_var(rsbwt_set_t *s, const char *text, const uint64_t *off, size_t Q, uint64_t *ordinal, uint64_t *copies);
int rsbwt_set_meta_by_ordinal(rsbwt_set_t *s, const uint32_t *shard_of, const uint64_t *ordinal, size_t n, uint64_t *first, uint8_t *bytes,
                              size_t cap, size_t *nbytes);
int rsbwt_set_meta_by_ordinal_dev(rsbwt_set_t *s, const void *d_shard, const void *d_ordinal, size_t n, void *d_first, void *d_bytes,
                                  size_t cap, void *stream);
int rsbwt_set_read_meta_var(rsbwt_set_t *s, const char *text, const uint64_t *off, size_t Q, uint64_t *first, uint8_t *bytes, size_t cap,
                            size_t *nbytes, uint64_t *copies);
void rsbwt_set_meta_last_work(uint64_t *work4);
/* Sample counts: in which samples does each query occur, and how often -- the sum over the reads that ExactMatch + All |
 * Samples returns one by one, made on the device from the sample table above.  Queries arrive as in the _var calls.
 *   codes     the caller's sample dictionary: C codes of size_of_sample bytes each, back to back, strictly ascending in
 *             memcmp order.  RSBWT_EINVAL: codes not ascending or not distinct, size_of_sample outside 1..8, C == 0, a set
 *             without a sample table ("no sample table"), a shard with 2^40 or more strings.
 *   records   a value is cut into records of R = size_of_sample + (has_other_meta_data ? 2 : 0) bytes as
 *             rsbwt_proto_encode_all_reply cuts it: code, then the c byte and the l byte.  The tail that is no whole
 *             record is dropped.
 *   rows      query q is searched in every shard exactly as rsbwt_set_locate_var_capped searches it (a symbol outside
 *             ACGT or an empty string: the empty interval).  matches[q] = its rows summed over the shards.  If max_rows > 0
 *             and matches[q] > max_rows the query contributes nothing: its rows of the matrices and carriers[q] stay zero,
 *             matches[q] still reports the count.  Every row of a kept query is located (max_steps as in rsbwt_set_locate;
 *             0 = 2^20); a row that is not located fails the call with RSBWT_EINVAL, as the SiteMatch and KmerMatch paths
 *             fail an unfinished walk.
 *   carriers  the sum runs over distinct read STRINGS, not rows: a read that holds the query at three offsets is one read,
 *             and the 20 copies of a string share one RocksDB key and one value (find_reads returns an
 *             unordered_set<string>).  For that the table holds one more array per shard, `heads`, one bit per ordinal,
 *             built by rsbwt_set_meta_build / _load on the shard's device: bit `ordinal` is set for every pair whose string
 *             matched that shard with copies > 0 (two pairs that name one string set one bit); rsbwt_set_meta_clear and a
 *             second build free or replace it with the table.  rsbwt_set_meta_bytes keeps its meaning and its value;
 *             rsbwt_set_meta_head_bytes alone reports the bitmaps: 4 * ceil(num_strings / 32) bytes per shard (0: no
 *             table).  The carriers of (q, p) are the distinct ordinals o among the located rows of q in shard p with
 *             heads_p[o] = 1.  Dropping a row on a copy that is no head loses nothing: all copies of a string hold the query
 *             at the same offsets, so the head copy is among the rows whenever any copy is; and a query over the limit
 *             contributes nothing at all, so the limit never splits a group of copies.  carriers[q] = the carriers summed
 *             over the shards; a string present in two shards counts in each.
 *   the sum   for every carrier and every whole record i of its value: col = the index of the record's code in codes, C if
 *             it is absent; strings[q][col] += 1; copies[q][col] += c with c = (int)(signed char)value[i R + size_of_sample]
 *             - 33 when has_other_meta_data (the encoder's rule), else 1.  The l byte is not used.  A value that lists one
 *             code twice adds twice.  strings u32[Q][C + 1], copies i64[Q][C + 1], matches / carriers u64[Q]; any may be
 *             NULL, not all of them.  Summed over the shards: a per-partition answer is the same call on a set of one.  All
 *             arithmetic is in integers: the answers do not depend on the order the lanes run in and are bit-identical from
 *             run to run.
 * On a one-device set nothing but matches[], the row total and the answers leaves the device (csrc/sample_counts.hip); a
 * set over several devices expands the rows on the host, every device tallies its shards' rows into matrices of its own
 * and the host adds them: same answers either way.  A call of many queries runs in slices whose matrices stay under 1.5 GiB
 * of HBM (and under 2^24 queries: the query number is part of a 64-bit key).  Re-entrant like the other lookups; not
 * beside build / load / clear.
 *   rsbwt_set_sample_counts_dev   a set on ONE device, nothing synchronised, everything enqueued on `stream`: d_text, d_off
 *       (u64[Q + 1], d_off[0] = 0) as rsbwt_set_match_lengths_dev takes them, Q <= 2^24; max_len in 1..65,535 = the longest
 *       query (a longer one gives the empty interval); d_keys u64[C] = the dictionary's keys as rsbwt_sample_keys spells
 *       them, which the call cannot check; cap_rows = room for the kept rows of the batch.  d_strings / d_copies /
 *       d_matches / d_carriers (any may be NULL, not all) are OVERWRITTEN: zeroed on the stream, then added to.  d_status8
 *       u64[8] = {kept rows of the batch, rows on a head ordinal, carriers, records added, records with an unknown code, LF
 *       steps of the walks, rows not located, 0}.  When status[0] > cap_rows nothing was tallied (ask again with that
 *       much room); when status[6] > 0 the answers are not complete (the host form's RSBWT_EINVAL).
 *   rsbwt_sample_keys             checks a dictionary as the host form does and writes its keys: key = the code's bytes as a
 *       big-endian number (so ascending codes have ascending keys).  Host code, no device.
 *   rsbwt_set_sample_last_work    the calling thread's last host-form call: {candidate rows, rows on a head ordinal,
 *       distinct carriers, records added, records with an unknown code, LF steps of the rows' walks (counted only while
 *       rsbwt_set_set_counting is on, else 0)}. */
int rsbwt_set_sample_counts(rsbwt_set_t *s, const char *text, const uint64_t *off, size_t Q, const uint8_t *codes, size_t C,
                            uint32_t size_of_sample, int has_other_meta_data, uint64_t max_rows, uint32_t max_steps,
                            uint32_t *strings, int64_t *copies, uint64_t *matches, uint64_t *carriers);
int rsbwt_set_sample_counts_dev(rsbwt_set_t *s, const void *d_text, const void *d_off, size_t Q, uint32_t max_len, const void *d_keys,
                                size_t C, uint32_t size_of_sample, int has_other_meta_data, uint64_t max_rows, uint32_t max_steps,
                                size_t cap_rows, void *d_strings, void *d_copies, void *d_matches, void *d_carriers, void *d_status8,
                                void *stream);
int rsbwt_sample_keys(const uint8_t *codes, size_t C, uint32_t size_of_sample, uint64_t *keys);
void rsbwt_set_sample_last_work(uint64_t *work6);
uint64_t rsbwt_set_meta_head_bytes(const rsbwt_set_t *s);
/* Sample walks: "which way do THIS sample set's reads go?" -- the walk above with the support of a symbol counted over the
 * reads of the samples a mask names, so that a walk follows one individual, family or population through the forks that
 * every heterozygous site of anyone else puts into the all-sample graph.  Everything is composed of two definitions above.
 *   From rsbwt_set_walk, unchanged: the seeds, ctx, the candidates x_c, rc(x), "invalid", flags bits 0 and 1, m =
 *     max(min_count, 1), max_steps, and the outputs ext / steps / stop / support / last.
 *   From rsbwt_set_sample_counts, unchanged: codes, C, size_of_sample, has_other_meta_data and max_locate_steps (max_steps
 *     there: the limit of a row's walk to its read's start, 0 = 2^20), with the same RSBWT_EINVAL cases, "no sample table"
 *     included.
 *   mask      u8[C], one byte per code of the ascending dictionary; non-zero = the column counts.  The unknown-code column C
 *             never counts.  An all-zero mask is legal: every valid seed stops with RSBWT_WALK_DEAD_END at 0 steps.
 *   SC(x)     the row rsbwt_set_sample_counts gives for the one query x with the call's max_rows: strings[], copies[] and
 *             matches, summed over distinct carrier strings per shard and over the shards as that call defines it.
 *   msup      the MASKED SUPPORT of symbol c at string s: t(s, c) = the sum over the columns col with mask[col] != 0 of
 *             SC(x_c).strings[col]; with RSBWT_WALK_BOTH_STRANDS the same sum for rc(x_c) is added (a read holding both
 *             counts in each; a palindromic candidate counts twice, as the plain walk counts it).  With the flag
 *             RSBWT_WALK_SAMPLE_COPIES (bit 2) SC(.).copies[col] is summed instead.  msup(s, c) = max(t(s, c), 0): copies can
 *             be negative, and it is the total over the columns and both strands that is held at 0.
 *   WIDE      max_rows is 1 .. 2^20 for these calls (0 and more: RSBWT_EINVAL); it bounds the scratch of a step at seeds x 8 x
 *             max_rows rows.  If SC(.).matches of ANY of the (4, or 8 with both strands) candidate-strand queries of an
 *             evaluation exceeds max_rows the evaluation is WIDE: its four supports are reported as 0, and a walk stops
 *             there with RSBWT_WALK_WIDE and last = zeros.  A repeat is not walked through on a partial count.
 *   rsbwt_set_extension_samples  the one-step primitive, on any set: msup u64[Q][4]; wide u8[Q] (1 = wide); matches
 *             u64[Q][4], may be NULL: the unmasked rows of each candidate, both strands added (filled for a wide evaluation
 *             too).  An invalid seed: zeros everywhere.
 *   rsbwt_set_walk_samples       rsbwt_set_walk's loop with msup in place of sup and one more stop, looked at first:
 *                           1. max_steps symbols appended: stop with RSBWT_WALK_LIMIT
 *                           2. evaluate;  wide: stop with RSBWT_WALK_WIDE
 *                           3. live = {c : msup(s, c) >= m}; empty: RSBWT_WALK_DEAD_END; two or more: RSBWT_WALK_BRANCH
 *                           4. else append the one live symbol and note its masked support
 *             last: zeros for LIMIT, INVALID and WIDE.  On a set on one device the host enqueues the whole walk -- per step a
 *             fixed sequence of launches, max_steps times, each of which leaves at once when no seed still walks -- and
 *             waits once; nothing but the outputs and the counters leaves the device (csrc/sample_walk.hip).  The seeds of a
 *             call are walked in slices that keep a step's rows under 256 MiB of HBM (one seed at the least) and under 2,048
 *             seeds.  Over several device groups every group evaluates its shards with rsbwt_set_extension_samples' launches,
 *             the host adds, decides and goes again: the same outputs, one round trip per step.
 *   rsbwt_set_walk_samples_dev   a set on ONE device (several: RSBWT_EINVAL): d_text, d_off, N and the outputs as
 *             rsbwt_set_walk_dev takes them; d_keys u64[C] as rsbwt_sample_keys spells them and d_mask u8[C] in HBM, which the
 *             call cannot check.  Everything is enqueued on `stream`, nothing is synchronised, every byte of every output is
 *             written.  d_status8 u64[8] = {rows located, rows on a head ordinal, carriers, records read, appended symbols, LF
 *             steps of the rows' walks, rows not located, wide evaluations}; status[6] > 0: the answers are not complete (the
 *             host forms' RSBWT_EINVAL).  Q = 0 zeroes d_status8 and touches nothing else.
 * A row that is not located within max_locate_steps fails the host forms with RSBWT_EINVAL.  A shard without terminators, or
 * a set one of whose shards has no table entry for a read, is answered as rsbwt_set_sample_counts answers it: such reads
 * carry nothing.  Q = 0, the range errors (ctx, max_steps, unknown flag bits, Q x max_steps >= 2^31) and "no device" follow
 * rsbwt_set_walk; more than 1,024 shards on one device are RSBWT_EINVAL.  All arithmetic is in integers: the answers are
 * bit-identical from run to run.
 * rsbwt_set_walk_samples_last_work: the calling thread's last host-form call: {seeds, appended symbols, candidate searches,
 * their LF steps, rows located, rows on a head ordinal, distinct carriers, records read, LF steps of the rows' walks, wide
 * evaluations}.  rsbwt_set_walk_samples_last_times: while the environment holds RSBWT_SAMPLE_WALK_TIMES=1, the device time in
 * ms of that thread's last rsbwt_set_walk_samples on a one-device set by kind of launch, from events round every launch: {init,
 * search, plan, rows, locate, tally, decide}; zeros otherwise.  The events cost time of their own: a measurement aid. */
#define RSBWT_WALK_SAMPLE_COPIES 4u
#define RSBWT_WALK_WIDE 8
int rsbwt_set_extension_samples(rsbwt_set_t *s, const char *text, const uint64_t *off, size_t Q, uint32_t ctx, uint32_t flags,
                                const uint8_t *codes, size_t C, uint32_t size_of_sample, int has_other_meta_data, const uint8_t *mask,
                                uint64_t max_rows, uint32_t max_locate_steps, uint64_t *msup, uint8_t *wide, uint64_t *matches);
int rsbwt_set_walk_samples(rsbwt_set_t *s, const char *text, const uint64_t *off, size_t Q, uint32_t ctx, uint64_t min_count,
                           uint32_t max_steps, uint32_t flags, const uint8_t *codes, size_t C, uint32_t size_of_sample,
                           int has_other_meta_data, const uint8_t *mask, uint64_t max_rows, uint32_t max_locate_steps, char *ext,
                           uint32_t *steps, uint8_t *stop, uint32_t *support, uint64_t *last);
int rsbwt_set_walk_samples_dev(rsbwt_set_t *s, const void *d_text, const void *d_off, size_t Q, size_t N, uint32_t ctx,
                               uint64_t min_count, uint32_t max_steps, uint32_t flags, const void *d_keys, size_t C,
                               uint32_t size_of_sample, int has_other_meta_data, const void *d_mask, uint64_t max_rows,
                               uint32_t max_locate_steps, void *d_ext, void *d_steps, void *d_stop, void *d_support, void *d_last,
                               void *d_status8, void *stream);
void rsbwt_set_walk_samples_last_work(uint64_t *work10);
void rsbwt_set_walk_samples_last_times(double *ms7);
/* Site sample counts: which samples have reads supporting this allele, and how many -- the sum over the reads SiteMatch +
 * All returns one by one (the reference's /gt), made on the device.  Requests are exactly rsbwt_set_gt_aligned_reads' (w =
 * text[off[q] .. off[q+1]), pos, alt, isalt after GtTask::run's fix-up; k, skip, M); the dictionary and the record rules are
 * exactly rsbwt_set_sample_counts' (codes, C, size_of_sample, has_other_meta_data; column C for a code the dictionary lacks,
 * the stray tail dropped, a code listed twice adds twice, c = (signed char)byte - 33).  In terms of those calls:
 *   R(q, p)      the reads rsbwt_set_gt_reads reports for request q in shard p
 *   A(q, p)      those of R(q, p) that rsbwt_set_gt_aligned_reads keeps
 *   a head       a string has a head in shard p when its FIRST ordinal there has its bit set in heads_p, that is when a pair
 *                of the sample table named it with copies > 0
 *   aligned[q]   the sum over p of |{r in R(q, p) with a head in p}|
 *   carriers[q]  the sum over p of |{r in A(q, p) with a head in p}|
 *   the sum      every whole record of every carrier's value at its head ordinal is tallied into row q of strings u32[Q][C + 1]
 *                and copies i64[Q][C + 1], as rsbwt_set_sample_counts tallies a carrier.  A string present in two shards
 *                counts in each.  Any output may be NULL, not all of them.  Q = 0 succeeds and touches nothing.  All
 *                arithmetic is in integers: the answers are bit-identical from run to run.
 * A read no pair names is neither extracted nor aligned: it could add nothing.  That is the one place where this call is
 * cheaper than the composition by definition, and it loses nothing: every copy of a string lies in the same leg intervals at
 * the same offsets with the same prefix and postfix lengths, so the head copy is among the rows the span filter keeps
 * whenever any copy is.
 * align_gt_read is the reference's as written, the isalt branch included: isalt = 1 rejects when the alt scores at least as
 * well, so it keeps a subset of what isalt = 0 keeps.  A caller who wants the alt allele's support sends the alt window (w
 * with the alt base at pos, alt = the reference base).
 * RSBWT_EINVAL: shards not opened with RSBWT_OPEN_READS; a set without a sample table ("no sample table"); a dictionary
 * rsbwt_sample_keys refuses; a shard of 2^40 strings or 2^46 symbols; a candidate row whose walk does not end; a w, or a
 * candidate read with a head, longer than 4,096 symbols.  pos = 0 and pos > |w| behave as in rsbwt_set_gt_aligned_reads:
 * candidates may exist and are counted in aligned[], and none is a carrier.
 * From the narrowing to the matrices the batch stays on the device (csrc/site_counts.hip): the span filter's kept rows are
 * deduplicated to (request, head ordinal) items in a hash set in HBM, the distinct reads among them are extracted once into
 * a device buffer (requests that share a window share their reads), the items go to the alignment without a copy through the
 * host, and the kept ones are tallied there.  Per device group the host receives the matrices, the two count vectors, the
 * counters and five sizes of eight bytes (rows, items, distinct reads, reads over the first extraction's 256 bytes, the
 * longest read); the groups' matrices are added on the host.  A call of many requests runs in slices whose matrices stay
 * under 1.5 GiB of HBM (and under 2^24 requests: the request number is part of a 64-bit key).  Re-entrant like the other
 * lookups; not beside build / load / clear.
 *   rsbwt_set_site_last_work   the calling thread's last call: {legs, LF steps spent lengthening, candidate rows, rows the span
 *       filter kept (the first four as rsbwt_set_gt_last_work counts them), of those rows on a head ordinal, distinct reads
 *       extracted, (request, read) items aligned, items kept, records added, records with an unknown code}; a failed call
 *       leaves all ten zero.  NULL is harmless.
 *   rsbwt_set_site_last_times  a measurement hook: while the environment has RSBWT_SITE_TIMES=1 the call puts events around
 *       each stage's launches on its stream (and waits for them, which costs time: not for production) and this reports the
 *       calling thread's last call in ms, summed over device groups and slices: {narrowing + rows + walks + filter, head
 *       test + set + compaction, sort / unique + extraction, length rule + ordering, alignment, tally}; all zero otherwise. */
int rsbwt_set_site_sample_counts(rsbwt_set_t *s, const char *text, const uint64_t *off, size_t Q, const uint64_t *pos, const char *alt,
                                 const uint8_t *isalt, int32_t k, int32_t skip, uint64_t M, const uint8_t *codes, size_t C,
                                 uint32_t size_of_sample, int has_other_meta_data, uint32_t *strings, int64_t *copies, uint64_t *aligned,
                                 uint64_t *carriers);
void rsbwt_set_site_last_work(uint64_t *work10);
void rsbwt_set_site_last_times(double *ms6);
/* Site reads: rsbwt_set_gt_aligned_reads / rsbwt_set_gt_aligned_count answered without that call's host trip.  Same
 * arguments, same layout (first[Q*S + 1], reads at read_stride, read_len, read_row), same sizing protocol (cap_reads = 0:
 * RSBWT_ERANGE with *nreads set) and the same answer element for element: the reads of (q, p) in ascending read_row, a
 * string once per (q, p) under the smallest read_row it has, a string present in two shards reported in each, a read
 * longer than read_stride reported with read_len = UINT32_MAX.  No sample table is needed.
 * RSBWT_EINVAL: shards not opened with RSBWT_OPEN_READS; a shard of 2^40 strings or 2^46 symbols; a candidate row whose
 * walk does not end; a w or a surviving candidate read longer than 4,096 symbols.  pos = 0 or pos > |w| keeps nothing.
 * From the narrowing to the answer the batch stays on the device (csrc/site_reads.hip over csrc/site_counts.hip's stages):
 * every row the span filter keeps becomes a (request, ordinal) item, the distinct reads are extracted once into device
 * buffers, equal strings are found by comparing each distinct read with its predecessor in (shard, read_row) order (the
 * copies of a string stand on consecutive read_rows, and every copy is a candidate whenever one is), the items are aligned
 * where they lie, and the kept ones are counted, ordered and gathered at read_stride there.  Per device group the host
 * receives the group's first[], the reported reads' bytes, lengths and rows, the counters and seven sizes of eight bytes
 * (rows, items, distinct reads, reads over the first extraction's 256 bytes, the longest read, classes, reads reported);
 * with one device group the copies land in the caller's arrays, with several the host puts each group's cells at their
 * places.  Slices of 2^24 requests; memory is bounded by the candidate rows.  Re-entrant like the other lookups.
 *   rsbwt_set_site_read_counts     counts[q*S+p] = how many reads that is; nothing is gathered.
 *   rsbwt_set_site_reads_last_work the calling thread's last call of either: {legs, LF steps spent lengthening, candidate
 *       rows, rows the span filter kept, distinct reads extracted, string classes among them, (request, read) items
 *       aligned, items kept, reads reported}; a failed call leaves all nine zero.  NULL is harmless. */
int rsbwt_set_site_reads(rsbwt_set_t *s, const char *text, const uint64_t *off, size_t Q, const uint64_t *pos, const char *alt, const uint8_t *isalt,
                         int32_t k, int32_t skip, uint64_t M, uint64_t *first, char *reads, uint32_t read_stride, uint32_t *read_len,
                         uint64_t *read_row, size_t cap_reads, size_t *nreads);
int rsbwt_set_site_read_counts(rsbwt_set_t *s, const char *text, const uint64_t *off, size_t Q, const uint64_t *pos, const char *alt,
                               const uint8_t *isalt, int32_t k, int32_t skip, uint64_t M, uint64_t *counts);
void rsbwt_set_site_reads_last_work(uint64_t *work9);
/* Device-resident forms, for a set on ONE device (one process per GPU: bench.py --mode 1mm|extract).
 * d_hits [num_shards][cap_per_shard] x 32-byte records (rsbwt_hits_1mm_dev's), d_totals u64[num_shards];
 * d_rows [num_shards][n] (row numbers are per shard), d_out [num_shards][n][stride], d_len / d_prefix_len [num_shards][n]. */
/* (below 2^26 variant searches per shard the shards work side by side on streams of the set, forked from and joined to `stream`, each with a scratch of its
 * own -- rsbwt_set_hits_1mm_scratch_bytes accounts for that) */
size_t rsbwt_set_hits_1mm_scratch_bytes(const rsbwt_set_t *s, size_t m, uint32_t k);
/* 1 when a call of this size searches ALL the set's shards by two launches (one device, k-mer tables of one depth,
 * below the same 2^26 variant searches per shard) instead of shard by shard -- for k <= 32 a walk of the k-mers that
 * also takes the step of the three substitutions at every position left of the tables' reach, then one search of the
 * variants that survived it and of those inside the tables' reach (csrc/search_solo.h WALK / WL, csrc/mm1_worklist.hip);
 * else a traced and a resumed launch: the launches are
 * then metered by the set (rsbwt_set_search_history_ms, rsbwt_set_last_search_counters), not by the shards' handles */
int rsbwt_set_hits_1mm_is_fused(const rsbwt_set_t *s, size_t m, uint32_t k);
int rsbwt_set_hits_1mm_dev(rsbwt_set_t *s, const void *d_packed, const void *d_valid, size_t m, uint32_t k, void *d_hits,
                           size_t cap_per_shard, void *d_totals, void *d_scratch, void *stream);
int rsbwt_set_extract_dev(rsbwt_set_t *s, const void *d_rows, size_t n, void *d_out, uint32_t stride, void *d_len,
                          void *d_prefix_len, void *stream);
int rsbwt_rccl_available(void); /* 1 when librccl could be bound at run time */
/* measurement hooks of a set's fused launches (first device): as the per-handle ones */
int rsbwt_set_set_counting(rsbwt_set_t *s, int on);
int rsbwt_set_search_history_ms(rsbwt_set_t *s, float *ms, size_t cap, size_t *count);
int rsbwt_set_last_search_counters(rsbwt_set_t *s, uint64_t *words16);

/* Service slice: the CountReads / ExactMatch-Count path of the query service --------
 * rsbwt_service_counts replaces, for a batch of serialised `Request` messages
 * (src/service/readserver.proto:3-14; message i = requests[req_off[i] .. req_off[i+1]), offsets
 * ascending and inside requests_len), what the recv loop does per message
 * (src/service/service.cpp:1549-1554,1567-1570 -> count_reads :279-315): two serialised `Reply`
 * messages per request, forward strand then reverse complement, each carrying the original query and
 * an int32 count summed over the set's shards (the front-end only adds partition counts:
 * src/service/server.cpp:184-197; the narrowing to int32, readserver.proto:31-33, applies to the sum:
 * the per-partition form is what rsbwt_service_create(per_partition = 1) sends).  Reply j of request i
 * is replies[rep_off[2i+j] .. rep_off[2i+j+1]); requests of any other type get two empty replies and
 * stay with the caller.  *needed receives the bytes required; RSBWT_ERANGE if cap is too small. */
int rsbwt_service_counts(rsbwt_set_t *set, const uint8_t *requests, size_t requests_len, const uint64_t *req_off,
                         size_t n, uint8_t *replies, size_t cap, uint64_t *rep_off, size_t *needed);
/* The codec on its own (host only). */
int rsbwt_proto_decode_request(const uint8_t *msg, size_t len, int *t, int *rt, const char **q, size_t *qlen);
size_t rsbwt_proto_encode_count_reply(uint8_t *out, size_t cap, int request_type, const char *q, size_t qlen,
                                      int revcomp, int32_t c);
/* Reply{rt = request_type, t = ReplyReads, q, r = ReplyReads{forward_matches | revcomp_matches = ResultReads{r}}*}
 * (src/service/readserver.proto:35-37,39-49,61-64): what QueryTask::run sends for a Request whose return type is
 * Reads (src/service/service.cpp:1260-1291).  `r` is present even with no read (mutable_r(), :1278).  Returns the
 * bytes needed (written when out != NULL and they fit cap); 0 = bad arguments. */
size_t rsbwt_proto_encode_reads_reply(uint8_t *out, size_t cap, int request_type, const char *q, size_t qlen, int revcomp,
                                      const char *const *reads, const size_t *read_len, size_t nreads);

/* Reply{rt = KmerMatch (3), t = (ReplyType) return_type, q, ...} as KmerTask::run sends it (src/service/service.cpp:
 * 871-960): return_type Count (1): c = ReplyCount{forward_matches | revcomp_matches = ResultCount{c = nreads}} (the
 * reads are not used); Reads (2): r = ReplyReads{...: one ResultReads per read}, present even when empty; All (3):
 * a = ReplyAll{...: one ResultAll{r} per read}, present even when empty.  Returns the bytes needed; 0 = bad arguments. */
size_t rsbwt_proto_encode_kmer_reply(uint8_t *out, size_t cap, int return_type, const char *q, size_t qlen, int revcomp,
                                     const char *const *reads, const size_t *read_len, size_t nreads);
/* Request fields 4 and 5 (k, s: readserver.proto:9-10); *has_k / *has_s = 0 when absent (then 0) */
int rsbwt_proto_decode_request_ks(const uint8_t *msg, size_t len, int32_t *k, int *has_k, int32_t *s, int *has_s);
/* The Reply a reference service sends for a request it finds nothing for: for Request type t and return type rt,
 * strand revcomp -- what rsbwt_service_set_unserved answers with (0 = bad arguments / no such reply). */
size_t rsbwt_proto_encode_empty_reply(uint8_t *out, size_t cap, int t, int rt, const char *q, size_t qlen, int revcomp);

/* Reply{rt = request_type, t = (ReplyType) return_type, q, a = ReplyAll{forward_matches | revcomp_matches = ResultAll{r, s*}*}}
 * (readserver.proto:16-29,39-54): what QueryTask::run (src/service/service.cpp:1292-1348; request_type 2) and KmerTask::run
 * (:917-975; request_type 3) send for the return types All (3) and Samples (4) -- the reference sets t = 4 for Samples and
 * still fills `a` (:1263).  Read i carries the ReadInfo records spelled from its value values[i] (value_len[i] bytes; values
 * NULL: none) exactly as :1332-1347 spell them: per record g = hash[value.substr(pos, size_of_sample)] -- `hash` is the text
 * of the service's hash file, lines of `name \t code` (:1477-1488; the first line of a code wins, a code not in it gives
 * g = "", as std::map::operator[] does) -- and, with has_other_meta_data, c = (int)(signed char)value[pos] - 33 and l likewise
 * from the next byte (negative values are ten-byte varints), else c = l = 0; required fields are written even when 0.
 * THE ONE DIVERGENCE: a value whose length is not a multiple of the record size is cut at its last whole record (the
 * reference reads past the end of the string there).  Returns the bytes needed (written when out != NULL and they fit cap);
 * 0 = bad arguments (size_of_sample 0 without meta data among them: a record of no bytes). */
size_t rsbwt_proto_encode_all_reply(uint8_t *out, size_t cap, int request_type, int return_type, const char *q, size_t qlen, int revcomp,
                                    const char *const *reads, const size_t *read_len, const uint8_t *const *values, const size_t *value_len,
                                    size_t nreads, const char *hash, size_t hash_len, uint32_t size_of_sample, int has_other_meta_data);
/* Host only: the pairs rsbwt_set_meta_load would build from the file at `path` (the parser alone).  sizes3 = {pairs, read
 * bytes, value bytes} is always set; RSBWT_ERANGE when a buffer is too small or NULL (call once to size them), RSBWT_EIO when
 * the file cannot be read.  off / voff receive pairs + 1 entries. */
int rsbwt_meta_parse_file(const char *path, char *text, size_t text_cap, uint64_t *off, uint8_t *values, size_t values_cap, uint64_t *voff,
                          size_t cap_pairs, size_t *sizes3);

/* The service's configuration file: the libconfig subset the reference's service.cfg uses
 * (`key = "value";`, `key = [ "a", ... ];`, comments; demo/TEMPLATE.service.cfg).  Loading fails with
 * RSBWT_EFORMAT when a setting the reference looks up unconditionally is missing (prefix, suffix,
 * hashfile, pull, push, push_count, rocksdb_path, rocksdb_ext, rocksdb: service.cpp:1425-1442). */
typedef struct rsbwt_service_config rsbwt_service_config_t;
int rsbwt_service_config_load(const char *path, rsbwt_service_config_t **out);
void rsbwt_service_config_free(rsbwt_service_config_t *cfg);
const char *rsbwt_service_config_get(const rsbwt_service_config_t *cfg, const char *key); /* NULL: absent */
size_t rsbwt_service_config_array_len(const rsbwt_service_config_t *cfg, const char *key);
const char *rsbwt_service_config_array_item(const rsbwt_service_config_t *cfg, const char *key, size_t i);

/* Transports: what the loop needs of ZeroMQ -- a SUB socket connected to `pull` and subscribed to
 * everything, PUSH sockets connected to `push` (channel 0) and `push_count` (channel 1)
 * (service.cpp:1493-1502).  In-process: a queue pair for tests and embedding. */
typedef struct rsbwt_transport rsbwt_transport_t;
int rsbwt_transport_inproc(rsbwt_transport_t **out);
/* ZeroMQ (src/service/service.cpp:1493-1502: SUB connect(pull) + subscribe-all, PUSH connect(push), PUSH
 * connect(push_count)).  libzmq is bound at run time (dlopen of libzmq.so.5; RSBWT_LIBZMQ names another):
 * RSBWT_ENODEV on a box without it, no rebuild on one with it. */
int rsbwt_transport_zmq(const char *pull, const char *push, const char *push_count, rsbwt_transport_t **out);
int rsbwt_zmq_available(void); /* 1 when libzmq could be bound */
void rsbwt_transport_free(rsbwt_transport_t *t);
int rsbwt_transport_push_request(rsbwt_transport_t *t, const uint8_t *msg, size_t n); /* in-process only */
int rsbwt_transport_pop_reply(rsbwt_transport_t *t, int channel, uint8_t *buf, size_t cap, size_t *n, int64_t timeout_us);
/* The same in bulk (in-process only; one lock per call instead of one per message): `count` Requests, message j =
 * base[off[j] .. off[j + 1]); up to max_msgs Replies of a channel back to back into buf (message j at off[j] ..
 * off[j + 1], off has max_msgs + 1 entries; *count = how many, 0 after timeout_us without one; a Reply that does not
 * fit `cap` any more stays queued). */
int rsbwt_transport_push_requests(rsbwt_transport_t *t, const uint8_t *base, const uint64_t *off, size_t count);
int rsbwt_transport_pop_replies(rsbwt_transport_t *t, int channel, uint8_t *buf, size_t cap, uint64_t *off, size_t max_msgs,
                                size_t *count, int64_t timeout_us);
void rsbwt_transport_close(rsbwt_transport_t *t); /* the loop ends once what was pushed is answered */

/* The recv loop (service.cpp:1521-1577) with a micro-batch window: the first Request opens a window
 * that closes after window_us or at max_batch messages; all CountReads / ExactMatch-Count requests of
 * the window are answered by one batched search per query length over the set; replies go out in
 * arrival order, forward strand then reverse complement, CountReads on push_count and ExactMatch on
 * push.  per_partition = 1: two replies per request PER SHARD, each what a reference service holding
 * that partition sends (front-end `workers` = 2 x shards); 0: two replies with the counts summed
 * (`workers` = 2).  ExactMatch requests that ask for Reads are answered too (rsbwt_service_set_reads).  Requests of
 * other types go to the handler (may be NULL), which is called on the loop's SENDER thread, not on the thread that
 * called rsbwt_service_run; an exception it throws is caught there and becomes the run's error. */
typedef struct rsbwt_service rsbwt_service_t;
typedef void (*rsbwt_service_other_fn)(void *arg, const uint8_t *request, size_t len);
int rsbwt_service_create(rsbwt_set_t *set, rsbwt_transport_t *t, int64_t window_us, size_t max_batch,
                         int per_partition, rsbwt_service_t **out);
void rsbwt_service_set_other_handler(rsbwt_service_t *s, rsbwt_service_other_fn fn, void *arg);
/* ExactMatch requests whose return type is Reads (`GET /get?output=reads`: the front-end's count pre-flight is
 * followed by this request, and it waits for `workers` replies without a timeout, src/service/server.cpp:469,565-601).
 * The loop answers them itself (default on): find_reads (src/service/service.cpp:714-797) batched over the set --
 * a query shorter than min_read_length: the reads of every row of its interval (in find_reads' order: the tail of an
 * interval wider than 4,097 rows first, then its 2,048-row chunks, :724-751); up to max_read_length: the
 * min_read_length-long tiles of the query that are themselves reads (query_exactmatch, src/bwt/query.cpp:102-120), then
 * every read that contains it (query, :87-100); longer: its max_read_length-long tiles that are reads, then the
 * min_read_length-long ones -- and sends, per partition (or once, summed mode) and strand,
 * Reply{rt = ExactMatch, t = ReplyReads, q, r} on `push` (QueryTask::run, service.cpp:1260-1291), forward strand
 * first.  min / max_read_length: service.cfg's keys (service.cpp:1417-1420; 0 = keep: 73 / 100, :56-57).
 * Tiles are visited in the order of the reference's container (std::unordered_set<std::string>, filled the same
 * way): the same order on the same C++ standard library.  A query holding a symbol outside ACGT matches nothing
 * (find_reads' short-query branch would search it as it stands; count_reads, the pre-flight, answers 0 for it).
 * The return types All and Samples are answered once the set has a sample table (rsbwt_service_set_all), else they are the
 * `other` handler's.  enable = 0: Reads requests go to the
 * `other` handler too, as before round 5. */
void rsbwt_service_set_reads(rsbwt_service_t *s, int enable, uint32_t min_read_length, uint32_t max_read_length);
/* service.cfg's `suffix` of every shard of the set (demo/TEMPLATE.service.cfg:16-17), n = rsbwt_set_size (0: none):
 * a tile is looked up only in the partitions whose suffix it ends with (is_suffix_of, service.cpp:228-230,759). */
int rsbwt_service_set_suffixes(rsbwt_service_t *s, const char *const *suffix, size_t n);
uint64_t rsbwt_service_read_requests(const rsbwt_service_t *s); /* Reads requests answered so far */
uint64_t rsbwt_service_kmer_requests(const rsbwt_service_t *s); /* KmerMatch Count / Reads requests answered so far */
/* KmerMatch requests with return type Count or Reads (`/kmermatch`): answered in the window (rsbwt_set_kmer_reads'
 * path; service.cfg `kmermatch = "on"`), 2 replies per partition on `push`, woven into the window's replies in arrival
 * order.  Needs every shard opened with RSBWT_OPEN_READS: RSBWT_EINVAL otherwise.  Default off. */
int rsbwt_service_set_kmermatch(rsbwt_service_t *s, int enable);
/* SiteMatch requests (`/gt`): answered in the window when on (service.cfg `sitematch = "on"`; default off: they go to the
 * `other` handler or, under rsbwt_service_set_unserved, get empty Replies, as before).  Per request and strand the window
 * fix-up of GtTask::run (service.cpp:1028-1046) with L = max_read_length, in signed arithmetic: the reverse strand takes
 * rev_comp(q), pos = |q| - p + 1 and rev_comp(a); pos <= L gives w = query[0 : L + pos - 1], else w = query[pos - L :
 * pos + L - 1] and pos = L.  pos > |w| (the reference's "ERROR" line), pos < 0 or a substr start past the end: the Reply
 * carries rt, t and q and no sub-message.  pos = 0, an empty a, k <= 0, s < 0 or k > |w| run and keep nothing (zero
 * count / empty list, the sub-message present).  A window's requests make one rsbwt_set_site_reads call (or
 * _read_counts when all of them ask for Count) per distinct (k, s), both strands as items, M = 10,000.  Replies: 2 per
 * request and partition, or 2 with counts summed and lists joined in partition order; Reply.rt = SiteMatch, Reply.t = the
 * request's rt; Count sends ReplyCount (c = the kept reads), Reads ReplyReads, All and Samples ReplyAll (served only when
 * rsbwt_service_set_all is on; each read with the ReadInfo records of its value, a read no pair names with none).  The
 * reads come in ascending read_row per partition, a string once per partition -- not in the reference's unordered_set
 * order.  A failed batch is answered with zero counts / empty lists.  RSBWT_EINVAL: a shard not opened with
 * RSBWT_OPEN_READS; max_read_length over 2,048 (a window then passes the alignment's 4,096 symbols) -- set the lengths
 * (rsbwt_service_set_reads) before switching this on.
 * rsbwt_service_site_requests: the SiteMatch Count / Reads requests answered (All / Samples count in all_requests).
 * rsbwt_proto_decode_request_site: Request.p / a / isalt (fields 6, 7, 8) beside rsbwt_proto_decode_request_ks. */
int rsbwt_service_set_sitematch(rsbwt_service_t *s, int enable);
uint64_t rsbwt_service_site_requests(const rsbwt_service_t *s);
int rsbwt_proto_decode_request_site(const uint8_t *msg, size_t len, int32_t *p, int *has_p, const char **a, size_t *alen, int *has_a, int32_t *isalt,
                                    int *has_isalt);
/* A limit on the reads one ExactMatch-Reads query may bring (service.cfg `max_match_reads`; the reference's front-end
 * has a key of that name, src/service/server.cpp:129,413): each strand of a request is a query of its own, and a strand
 * whose rows, summed over the partitions, exceed n is answered -- in every partition's Reply, or in the one summed
 * Reply -- with rsbwt_proto_encode_empty_reply's bytes, neither tile matches nor reads; every other request of the
 * window is answered as if the wide one were not there.  The first such request is logged once.  n = 0 (the default):
 * no limit, the code path of the releases before the key.  RSBWT_ENODEV: a limit on a build without the engine. */
int rsbwt_service_set_max_match_reads(rsbwt_service_t *s, uint64_t n);
uint64_t rsbwt_service_capped_requests(const rsbwt_service_t *s); /* Reads requests with a strand over the limit so far */
/* Requests nothing in this loop answers and no `other` handler takes (ExactMatch / KmerMatch with All or Samples,
 * SiteMatch; service.cfg `unserved = "empty"`): 2 replies per partition on `push` carrying no matches, as the
 * reference sends for an empty result.  The first such request is logged once.  Default off. */
void rsbwt_service_set_unserved(rsbwt_service_t *s, int empty);
/* ExactMatch requests with return type All or Samples (`output=all`, what scripts/client.pl asks for by default), and KmerMatch
 * ones when rsbwt_service_set_kmermatch is on: answered in the window -- the reads of the Reads paths, in their order and
 * under their rules (tiles, suffix filter, min / max read length, max_match_reads: a strand over the limit gets empty lists),
 * each read with its `s` from the set's sample table (rsbwt_set_read_meta_var over the reads of each Reply, in their own
 * partition), one rsbwt_proto_encode_all_reply per partition and strand on `push`.  hashfile / size_of_sample /
 * has_other_meta_data: service.cfg's keys (service.cpp:1410-1415,1425; hashfile NULL or "": every g is "").  service.cfg:
 * `meta = "<pairs file>"`.  RSBWT_EINVAL: the set has no sample table, or a shard was not opened with RSBWT_OPEN_READS;
 * RSBWT_EIO: the hash file cannot be read.  Default off: such requests go to the `other` handler / rsbwt_service_set_unserved
 * as before.  Before rsbwt_service_run / _start. */
int rsbwt_service_set_all(rsbwt_service_t *s, int enable, const char *hashfile, uint32_t size_of_sample, int has_other_meta_data);
uint64_t rsbwt_service_all_requests(const rsbwt_service_t *s); /* All / Samples requests answered so far */
/* The loop is a pipeline: the thread that runs it receives and cuts the windows, `workers` threads answer a whole
 * window each (decode, one batched search per query length, Reply bytes -- the set's entry points are re-entrant),
 * a sender thread sends the windows' Replies in window order, so replies still leave in arrival order.  Default 8,
 * the threads of the reference's query pool (src/service/service.cpp:88,1505); before rsbwt_service_run / _start. */
void rsbwt_service_set_workers(rsbwt_service_t *s, int workers);
int rsbwt_service_run(rsbwt_service_t *s);   /* on the calling thread, until the transport closes */
int rsbwt_service_start(rsbwt_service_t *s); /* on a thread of its own */
int rsbwt_service_stop(rsbwt_service_t *s);  /* at once; after rsbwt_transport_close: once all that was pushed is answered */
void rsbwt_service_free(rsbwt_service_t *s);
/* {requests, count requests, windows, replies sent, malformed messages, largest window} */
void rsbwt_service_stats(const rsbwt_service_t *s, uint64_t *stats6);

/* Test hook (host only, answers no query): lays `runs` out as window lines with the code the GPU
 * builder runs and holds the layout's scalar readers to naive ranks at every position.  stats6 =
 * {S, lines, far lines, chunk windows, far windows, spilled symbols}; *first_bad = first position
 * that disagrees (RSBWT_EFORMAT) or UINT64_MAX.  Bit 31 of window_span (both hooks): the RSBWT_OPEN_READS
 * layout. */
int rsbwt_layout_selftest_host(const uint8_t *runs, uint64_t num_runs, uint32_t window_span,
                               uint64_t *stats6, uint64_t *first_bad);

/* Test hook (host only, answers no query): the select samples and psi hints of read extraction -- the code the
 * builder kernels and the walk kernels share with the host (csrc/line_format.h) -- built over a host-side layout of
 * `runs` and held to the naive select at EVERY occurrence and EVERY row, then every scalar reader again over the
 * lines that now carry hints.  stats4 = {sample words, occurrences whose sample is only a bound, lines with a
 * hint, rows a hint settles (the others it bounds)}; *first_bad as above. */
int rsbwt_layout_selftest_psi_host(const uint8_t *runs, uint64_t num_runs, uint32_t window_span, uint64_t *stats4,
                                   uint64_t *first_bad);

/* Test hook (host only, answers no query): the lines the two hooks above certify, handed out, so that a GPU test can
 * hold the device builder's lines and select sample table to them byte for byte.  `runs` is laid out by the very
 * passes of rsbwt_layout_selftest_host -- or, with RSBWT_LAYOUT_HINTS, of rsbwt_layout_selftest_psi_host, whose sample
 * table and psi hints are then built too, the hints written into the lines.  window_span as above (bit 31: the
 * RSBWT_OPEN_READS layout).  out_lines: lines * 128 bytes, cap_bytes of room (NULL: the count pass only); out_sel: the
 * sample table, stats10[7] words, cap_sel_words of room (NULL, or without the flag: not copied); group_stats4: {far
 * lines, chunk windows, far windows, spilled symbols} per group of 16 windows, cap_groups groups of room (NULL: not
 * wanted).  stats10 = the stats6 above, then {groups, words of the sample table, sample words written, lines with a
 * hint} (the last two 0 unless built).  RSBWT_ERANGE: a buffer is too small (stats10 is filled all the same);
 * RSBWT_EFORMAT: a symbol code above 4. */
#define RSBWT_LAYOUT_HINTS 1u
int rsbwt_layout_lines_host(const uint8_t *runs, uint64_t num_runs, uint32_t window_span, uint32_t flags,
                            uint32_t *out_lines, uint64_t cap_bytes, uint64_t *out_sel, uint64_t cap_sel_words,
                            uint64_t *group_stats4, uint64_t cap_groups, uint64_t *stats10);

/* Test hook (host only, answers no query): the grouped k-mer table's record code (rsbwt_attach_ktab_format) -- `groups`
 * x 4 sibling intervals in, the 4 entries each 12-byte record gives back out as {lower:40 | width:24} words, width
 * 0xFFFFFF = left to the search. */
int rsbwt_ktab_group_selftest_host(const uint64_t *lower, const uint64_t *upper, size_t groups, uint64_t *entries);

/* Test hook (answers no query): overwrites n bytes of the index in HBM -- region 0: the window lines,
 * 1: the handle's own k-mer table -- so that tests can hold the kernels to what they do with a DAMAGED
 * index: no read outside the index, every wave drains, a table entry that is not an interval of this BWT
 * is not believed.  RSBWT_ERANGE outside the region.  Refused (RSBWT_EINVAL) unless the environment has
 * RSBWT_ENABLE_TEST_HOOKS set: nothing in a deployment may write into a published index. */
int rsbwt_debug_poke(rsbwt_t *h, int region, uint64_t offset, const void *bytes, size_t n);

/* Test hook (answers no query): the kernels' position -> window division (an f64 multiply and one fix-up step
 * instead of a 64-bit divide) on n host positions: w[i] = p[i] / S, r[i] = p[i] % S, so that a test can hold
 * it to integer division up to the 2^40 symbols a shard may have, for every span S in 2..2944. */
int rsbwt_debug_fast_window(const uint64_t *p, size_t n, uint32_t S, uint32_t *w, uint32_t *r, int device);

/* Test hook (RSBWT_ENABLE_TEST_HOOKS, answers no query): the kernels' rank primitives (csrc/rank_device.h) on n cases given by
 * hand, one GPU thread each.  A case is 8 dwords: the 24 piece bytes of a quarter (six dwords, piece = symbol << 5 | length),
 * a symbol b (0..4) and one argument.  `op` names the primitive; out receives 6 dwords per case for
 * RSBWT_PRIM_DWORD_MATCHED, 2 per case for every other op (unused ones 0):
 *   DWORD_MATCHED     out[i] = dword_matched(dword i, b in every byte, acc = arg), i = 0..5
 *   MATCHED24         out[0] = matched24_tab
 *   RUNS_SCAN1 / 2    out[0] = runs_scan<1> on dword 0 / runs_scan<2> on dwords 0-1, rem = arg
 *   RANK24            out[0] = rank24, rem = arg
 *   RANK24_DOLLAR     out[0] = rank24_dollar, rem = arg (b is not looked at)
 *   CHAR_RANK24       out = {c, occ} of char_rank24(rem = arg, want = 0);  _WANT: want = b
 *   SELECT_IN24       out = {position, *left} of select_in24(b, t = arg)
 * const_b = 0: b reaches the primitive as a run-time value; 1: through the instance compiled for that symbol, b a
 * compile-time constant (a case whose b is above 4 then gets all-ones).  Host buffers. */
#define RSBWT_PRIM_DWORD_MATCHED 0u
#define RSBWT_PRIM_MATCHED24 1u
#define RSBWT_PRIM_RUNS_SCAN1 2u
#define RSBWT_PRIM_RUNS_SCAN2 3u
#define RSBWT_PRIM_RANK24 4u
#define RSBWT_PRIM_RANK24_DOLLAR 5u
#define RSBWT_PRIM_CHAR_RANK24 6u
#define RSBWT_PRIM_CHAR_RANK24_WANT 7u
#define RSBWT_PRIM_SELECT_IN24 8u
int rsbwt_debug_rank_primitives(uint32_t op, int const_b, const uint32_t *cases, size_t n, uint32_t *out, int device);

/* Test hook (RSBWT_ENABLE_TEST_HOOKS, answers no query): the staged-line readers (csrc/wave_lines.h) on n positions (< BWLen,
 * else RSBWT_ERANGE) of a resident shard, one lane per position: the lane fetches the position's window line into LDS as the
 * search kernels do and ranks off it.  out = u64[n][13]: Occ up to and including the position of the three bases other than
 * `orig` by staged_occ_alts, for orig = A, C, G, T in turn -- {C,G,T}, {A,G,T}, {A,C,T}, {A,C,G} -- then Occ('$') by
 * staged_dollars.  A position past its line's own pieces (spill chunk / far line): out[i][0] = all ones, out[i][1..12] = 0. */
int rsbwt_debug_staged_rank(rsbwt_t *h, const uint64_t *positions, size_t n, uint64_t *out);

#ifdef __cplusplus
}
#endif
#endif
