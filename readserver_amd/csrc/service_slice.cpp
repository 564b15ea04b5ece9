// service_slice.cpp -- the CountReads / ExactMatch-Count slice of ReadServer's query service
// (SURVEY 8 f1), host side: proto2 wire codec for the two messages involved and the batched
// count_reads (src/service/service.cpp:279-315) over a shard set; and, since round 5, the ExactMatch requests
// whose return type is Reads: find_reads (service.cpp:714-797) batched over the set, the replies of
// QueryTask::run (:1260-1291) -- what `GET /get?output=reads` waits for after its count pre-flight
// (server.cpp:565-601); BWT only (the `all` return type needs the RocksDB shards and stays with the caller).
//
// Wire schema followed: src/service/readserver.proto:3-14 (Request), :31-33 (ResultCount),
// :39-49 (Reply), :56-59 (ReplyCount).  protobuf is not in this image, so the codec is written
// against the proto2 encoding itself (varint keys, length-delimited strings/messages, fields
// emitted in field-number order as protobuf's C++ serialiser does); tests/test_service_slice.py
// compares it byte for byte with the Python protobuf runtime on a re-typed schema.
// Transport (ZeroMQ SUB/PUSH, service.cpp:1493-1502) stays with the caller: INTEGRATION.md.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <map>
#include <thread>
#include <new>
#include <string>
#include <unordered_set>
#include <vector>

#include "../../include/rsbwt.h"
#include "service.h"
#include "capi_guard.h"
#include "kmer_reads.h"

namespace {

struct request_view {
    int t = 0, rt = 0;      // Request.RequestType / ReturnType (readserver.proto:4-5)
    const char *q = nullptr;
    size_t qlen = 0;
    int32_t k = 0, s = 0;   // KmerMatch / SiteMatch: optional int32 k = 4, s = 5 (readserver.proto:9-10)
    bool has_t = false, has_rt = false, has_q = false, has_k = false, has_s = false;
    int32_t p = 0, isalt = 0;  // SiteMatch: optional int32 p = 6, string a = 7, int32 isalt = 8 (readserver.proto:11-13)
    const char *a = nullptr;
    size_t alen = 0;
    bool has_p = false, has_a = false, has_isalt = false;
};

bool get_varint(const uint8_t *&p, const uint8_t *end, uint64_t &v) {
    v = 0;
    for (int shift = 0; p < end && shift < 70; shift += 7) {
        const uint8_t b = *p++;
        v |= (uint64_t)(b & 0x7F) << shift;
        if (!(b & 0x80)) return true;
    }
    return false;
}

bool decode_request(const uint8_t *p, size_t n, request_view &r) {
    const uint8_t *end = p + n;
    while (p < end) {
        uint64_t key;
        if (!get_varint(p, end, key)) return false;
        const uint32_t field = (uint32_t)(key >> 3), wt = (uint32_t)(key & 7);
        if (wt == 0) {
            uint64_t v;
            if (!get_varint(p, end, v)) return false;
            if (field == 1) { r.t = (int)v; r.has_t = true; }
            else if (field == 2) { r.rt = (int)v; r.has_rt = true; }
            else if (field == 4) { r.k = (int32_t)(uint32_t)v; r.has_k = true; }  // (int32: a negative value arrives sign-extended)
            else if (field == 5) { r.s = (int32_t)(uint32_t)v; r.has_s = true; }
            else if (field == 6) { r.p = (int32_t)(uint32_t)v; r.has_p = true; }
            else if (field == 8) { r.isalt = (int32_t)(uint32_t)v; r.has_isalt = true; }
        } else if (wt == 2) {
            uint64_t len;
            if (!get_varint(p, end, len) || len > (uint64_t)(end - p)) return false;
            if (field == 3) { r.q = (const char *)p; r.qlen = (size_t)len; r.has_q = true; }
            else if (field == 7) { r.a = (const char *)p; r.alen = (size_t)len; r.has_a = true; }
            p += len;
        } else if (wt == 1) {
            if (end - p < 8) return false;
            p += 8;
        } else if (wt == 5) {
            if (end - p < 4) return false;
            p += 4;
        } else {
            return false;
        }
    }
    return r.has_t && r.has_rt && r.has_q;  // all three are `required`
}

inline size_t varint_len(uint64_t v) {
    size_t n = 1;
    while (v >= 0x80) { v >>= 7; ++n; }
    return n;
}

inline uint8_t *put_varint(uint8_t *p, uint64_t v) {
    while (v >= 0x80) { *p++ = (uint8_t)(v | 0x80); v >>= 7; }
    *p++ = (uint8_t)v;
    return p;
}

// Reply{rt, t = ReplyCount, q, c = ReplyCount{forward_matches | revcomp_matches = ResultCount{c}}}
size_t count_reply_len(int request_type, size_t qlen, int32_t c) {
    const size_t result_count = 1 + varint_len((uint64_t)(int64_t)c);  // int32: negative values are sign-extended to 10 bytes
    const size_t reply_count = 1 + varint_len(result_count) + result_count;
    return 1 + varint_len((uint64_t)request_type) + 2 + 1 + varint_len(qlen) + qlen + 1 + varint_len(reply_count) + reply_count;
}

uint8_t *encode_count_reply(uint8_t *p, int request_type, const char *q, size_t qlen, bool revcomp, int32_t c) {
    const size_t result_count = 1 + varint_len((uint64_t)(int64_t)c);
    const size_t reply_count = 1 + varint_len(result_count) + result_count;
    *p++ = 0x08; p = put_varint(p, (uint64_t)request_type);  // rt
    *p++ = 0x10; *p++ = 1;                                    // t = ReplyCount
    *p++ = 0x1A; p = put_varint(p, qlen);
    if (qlen) memcpy(p, q, qlen);
    p += qlen;
    *p++ = 0x22; p = put_varint(p, reply_count);
    *p++ = revcomp ? 0x12 : 0x0A; p = put_varint(p, result_count);
    *p++ = 0x08; p = put_varint(p, (uint64_t)(int64_t)c);
    return p;
}

std::string rev_comp(const char *q, size_t n) {  // service.cpp:251-276
    std::string s(n, 'N');
    for (size_t i = 0; i < n; ++i) {
        const char ch = q[n - 1 - i];
        s[i] = ch == 'A' ? 'T' : ch == 'T' ? 'A' : ch == 'C' ? 'G' : ch == 'G' ? 'C' : ch;
    }
    return s;
}

}  // namespace

extern "C" {

int rsbwt_proto_decode_request(const uint8_t *msg, size_t len, int *t, int *rt, const char **q, size_t *qlen) {
    request_view r;
    if (!msg || !decode_request(msg, len, r)) return RSBWT_EFORMAT;
    if (t) *t = r.t;
    if (rt) *rt = r.rt;
    if (q) *q = r.q;
    if (qlen) *qlen = r.qlen;
    return RSBWT_OK;
}

int rsbwt_proto_decode_request_ks(const uint8_t *msg, size_t len, int32_t *k, int *has_k, int32_t *s, int *has_s) {
    request_view r;
    if (!msg || !decode_request(msg, len, r)) return RSBWT_EFORMAT;
    if (k) *k = r.k;
    if (has_k) *has_k = r.has_k ? 1 : 0;
    if (s) *s = r.s;
    if (has_s) *has_s = r.has_s ? 1 : 0;
    return RSBWT_OK;
}

int rsbwt_proto_decode_request_site(const uint8_t *msg, size_t len, int32_t *p, int *has_p, const char **a, size_t *alen, int *has_a, int32_t *isalt,
                                    int *has_isalt) {
    request_view r;
    if (!msg || !decode_request(msg, len, r)) return RSBWT_EFORMAT;
    if (p) *p = r.p;
    if (has_p) *has_p = r.has_p ? 1 : 0;
    if (a) *a = r.a;
    if (alen) *alen = r.alen;
    if (has_a) *has_a = r.has_a ? 1 : 0;
    if (isalt) *isalt = r.isalt;
    if (has_isalt) *has_isalt = r.has_isalt ? 1 : 0;
    return RSBWT_OK;
}

size_t rsbwt_proto_encode_count_reply(uint8_t *out, size_t cap, int request_type, const char *q, size_t qlen,
                                      int revcomp, int32_t c) {
    if (!q && qlen) return 0;
    const size_t len = count_reply_len(request_type, qlen, c);
    if (out && len <= cap) encode_count_reply(out, request_type, q, qlen, revcomp != 0, c);
    return len;
}

}  // extern "C"

namespace rsb {

// count_reads (src/service/service.cpp:279-315) for a batch of decoded requests over a shard set.
// Every request of type CountReads, or ExactMatch with return type Count, gets its replies; the
// others are left to the caller (handled[i] = 0).  per_partition: one forward and one reverse-
// complement Reply PER SHARD, each carrying that shard's count narrowed to int32 exactly as a
// reference service process holding that partition would send it (readserver.proto:31-33,
// service.cpp:304) -- the front-end adds them up (server.cpp:184-197).  Otherwise two replies per
// request with the counts summed over the shards first (set the front-end's `workers` to 2): the
// narrowing then applies to the sum, which differs from the above only beyond 2^31 matches.
int service_count_batch(rsbwt_set_t *set, const std::vector<service_request> &rq, bool per_partition,
                        reply_arena *replies, std::vector<char> *handled) {
    const size_t n = rq.size();
    const size_t S = rsbwt_set_size(set);
    handled->assign(n, 0);
    replies->bytes.clear();
    replies->off.assign(1, 0);
    replies->first.assign(n + 1, 0);
    std::map<size_t, std::vector<size_t>> by_len;  // one batched search per query length
    for (size_t i = 0; i < n; ++i) {
        const bool count_reads = rq[i].t == 1;                   // Request::CountReads
        const bool exact_count = rq[i].t == 2 && rq[i].rt == 1;  // ExactMatch + Count
        if (!count_reads && !exact_count) continue;               // other paths stay with the caller
        (*handled)[i] = 1;
        by_len[rq[i].q.size()].push_back(i);
    }
    // per request: [strand][shard] counts (one row when summed)
    const size_t rows = per_partition ? S : 1;
    std::vector<std::vector<uint64_t>> cnt(n);
    // A window whose requests have lengths of their own (what a front-end sends: any length up to its limit): ONE search
    // of all of them, both strands -- forward queries, then their reverse complements (rsbwt_set_find_intervals_var /
    // rsbwt_set_count_var: a start record per search says where it goes on).  A window of one length keeps the
    // fixed-length call (its summed form reduces over RCCL on a set of several devices).
    if (by_len.size() > 1) {
        std::vector<size_t> who;
        for (size_t i = 0; i < n; ++i)
            if ((*handled)[i]) {
                cnt[i].assign(2 * rows, 0);
                if (!rq[i].q.empty()) who.push_back(i);  // (empty query: count 0, findInterval on "" is undefined in the reference)
            }
        const size_t m = who.size();
        std::string text;
        std::vector<uint64_t> off(2 * m + 1, 0);
        for (size_t j = 0; j < m; ++j) {
            text += rq[who[j]].q;
            off[j + 1] = text.size();
        }
        for (size_t j = 0; j < m; ++j) {
            text += rev_comp(rq[who[j]].q.data(), rq[who[j]].q.size());
            off[m + j + 1] = text.size();
        }
        if (m != 0 && per_partition) {
            std::vector<uint64_t> lo(S * 2 * m), up(S * 2 * m);
            const int rc = rsbwt_set_find_intervals_var(set, text.data(), off.data(), 2 * m, lo.data(), up.data());
            if (rc != RSBWT_OK) return rc;
            for (size_t s = 0; s < S; ++s)
                for (size_t j = 0; j < 2 * m; ++j) {
                    const uint64_t l = lo[s * 2 * m + j], u = up[s * 2 * m + j];
                    cnt[who[j % m]][(j / m) * rows + s] = u >= l ? u - l + 1 : 0;  // service.cpp:304
                }
        } else if (m != 0) {
            std::vector<uint64_t> c(2 * m);
            const int rc = rsbwt_set_count_var(set, text.data(), off.data(), 2 * m, c.data());
            if (rc != RSBWT_OK) return rc;
            for (size_t j = 0; j < 2 * m; ++j) cnt[who[j % m]][j / m] = c[j];
        }
        by_len.clear();
    }
    for (auto &g : by_len) {
        const size_t k = g.first, m = g.second.size();
        for (size_t j = 0; j < m; ++j) cnt[g.second[j]].assign(2 * rows, 0);
        if (k == 0) continue;  // empty query: count 0 (findInterval on "" is undefined in the reference)
        // both strands of the group in one batch: forward k-mers, then their reverse complements
        std::string flat(2 * m * k, 'N');
        for (size_t j = 0; j < m; ++j) {
            const std::string &q = rq[g.second[j]].q;
            memcpy(&flat[j * k], q.data(), k);
            const std::string rc = rev_comp(q.data(), k);
            memcpy(&flat[(m + j) * k], rc.data(), k);
        }
        int rc;
        if (per_partition) {
            std::vector<uint64_t> lo(S * 2 * m), up(S * 2 * m);
            rc = rsbwt_set_find_intervals(set, flat.data(), 2 * m, (uint32_t)k, k, lo.data(), up.data());
            if (rc != RSBWT_OK) return rc;
            for (size_t s = 0; s < S; ++s)
                for (size_t j = 0; j < 2 * m; ++j) {
                    const uint64_t l = lo[s * 2 * m + j], u = up[s * 2 * m + j];
                    const uint64_t c = u >= l ? u - l + 1 : 0;  // service.cpp:304
                    cnt[g.second[j % m]][(j / m) * rows + s] = c;
                }
        } else {
            std::vector<uint64_t> c(2 * m);
            rc = rsbwt_set_count(set, flat.data(), 2 * m, (uint32_t)k, k, c.data());
            if (rc != RSBWT_OK) return rc;
            for (size_t j = 0; j < 2 * m; ++j) cnt[g.second[j % m]][j / m] = c[j];
        }
    }
    // resultc->set_c(...) narrows the 64-bit count to int32 (readserver.proto:31-33)
    auto narrowed = [&](size_t i, size_t r, int strand) { return (int32_t)(uint32_t)cnt[i][strand * rows + r]; };
    size_t total = 0, messages = 0;
    for (size_t i = 0; i < n; ++i) {
        if (!(*handled)[i]) continue;
        for (size_t r = 0; r < rows; ++r)
            for (int strand = 0; strand < 2; ++strand) total += count_reply_len(rq[i].t, rq[i].q.size(), narrowed(i, r, strand));
        messages += 2 * rows;
    }
    replies->bytes.resize(total);
    replies->off.reserve(messages + 1);
    uint8_t *p = replies->bytes.data();
    for (size_t i = 0; i < n; ++i) {
        replies->first[i] = replies->off.size() - 1;
        if (!(*handled)[i]) continue;
        for (size_t r = 0; r < rows; ++r)
            for (int strand = 0; strand < 2; ++strand) {
                p = encode_count_reply(p, rq[i].t, rq[i].q.data(), rq[i].q.size(), strand == 1, narrowed(i, r, strand));
                replies->off.push_back((size_t)(p - replies->bytes.data()));
            }
    }
    replies->first[n] = replies->off.size() - 1;
    return RSBWT_OK;
}

// ---- ExactMatch + Reads: find_reads (service.cpp:714-797), batched ---------------------------------------------
namespace {

// Reply{rt, t = ReplyReads (2), q, r = ReplyReads{forward_matches | revcomp_matches = ResultReads{r}}*}
// (readserver.proto:35-37,39-49,61-64); `r` is present even when no read matched (QueryTask::run calls
// r.mutable_r() before the loop, service.cpp:1278: an empty sub-message, 2 bytes on the wire)
size_t reads_body_len(const std::vector<const std::string *> &reads) {
    size_t body = 0;
    for (const std::string *s : reads) {
        const size_t rr = 1 + varint_len(s->size()) + s->size();  // ResultReads{r}
        body += 1 + varint_len(rr) + rr;
    }
    return body;
}
size_t reads_reply_len(int request_type, size_t qlen, size_t body) {
    return 1 + varint_len((uint64_t)request_type) + 2 + 1 + varint_len(qlen) + qlen + 1 + varint_len(body) + body;
}
uint8_t *encode_reads_reply(uint8_t *p, int request_type, const std::string &q, bool revcomp, const std::vector<const std::string *> &reads, size_t body) {
    *p++ = 0x08; p = put_varint(p, (uint64_t)request_type);  // rt
    *p++ = 0x10; *p++ = 2;                                    // t = ReplyReads
    *p++ = 0x1A; p = put_varint(p, q.size());
    if (!q.empty()) memcpy(p, q.data(), q.size());
    p += q.size();
    *p++ = 0x2A; p = put_varint(p, body);                     // r
    for (const std::string *s : reads) {
        const size_t rr = 1 + varint_len(s->size()) + s->size();
        *p++ = revcomp ? 0x12 : 0x0A; p = put_varint(p, rr);
        *p++ = 0x0A; p = put_varint(p, s->size());
        if (!s->empty()) memcpy(p, s->data(), s->size());
        p += s->size();
    }
    return p;
}

// if w ends with s (service.cpp:228-230)
inline bool is_suffix_of(const std::string &s, const std::string &w) {
    return s.empty() || (w.size() >= s.size() && memcmp(s.data(), w.data() + (w.size() - s.size()), s.size()) == 0);
}

// get_tiles(w, kmer) (service.cpp:232-250, skip = 0): every kmer-long substring once -- into the SAME container the
// reference uses, filled in the same order, so that iterating it visits the tiles in the order the reference's
// loop does on the same standard library (the order of an unordered_set is the library's, not the standard's)
std::unordered_set<std::string> get_tiles(const std::string &w, size_t kmer) {
    std::unordered_set<std::string> vs;
    if (kmer == 0 || w.size() < kmer) return vs;
    for (size_t i = 0; i <= w.size() - kmer; ++i) vs.insert(w.substr(i, kmer));
    return vs;
}

// The order find_reads leaves the rows of a wide interval in (service.cpp:724-751): while more than 2 x 2,048 rows
// are left a chunk of 2,048 goes to the extraction pool; the rows that remain are extracted on the spot and come
// FIRST, the chunks' reads are appended after them in chunk order.  Returns the number of leading rows that move
// behind the tail (0 for intervals of up to 4,097 rows).
inline size_t chunked_head(size_t n) {
    const size_t large = 2048;  // service.cpp:86
    size_t start = 0;
    while (n != 0 && (n - 1) - start > 2 * large) start += large;
    return start;
}

}  // namespace

void service_reads_empty(const std::vector<service_request> &rq, size_t rows, reply_arena *replies, std::vector<char> *handled, const reads_config *cfg) {
    const size_t n = rq.size();
    handled->assign(n, 0);
    replies->bytes.clear();
    replies->off.assign(1, 0);
    replies->first.assign(n + 1, 0);
    const std::vector<const std::string *> none;
    for (size_t i = 0; i < n; ++i) {
        replies->first[i] = replies->off.size() - 1;
        if (cfg ? !service_takes_reads(rq[i], *cfg) : !service_is_reads_request(rq[i])) continue;
        if (service_is_all_return(rq[i])) {
            (*handled)[i] = 1;
            service_append_empty(rq[i], rows, replies);
            continue;
        }
        (*handled)[i] = 1;
        for (size_t r = 0; r < rows; ++r)
            for (int strand = 0; strand < 2; ++strand) {
                const size_t at = replies->bytes.size(), len = reads_reply_len(rq[i].t, rq[i].q.size(), 0);
                replies->bytes.resize(at + len);
                encode_reads_reply(replies->bytes.data() + at, rq[i].t, rq[i].q, strand == 1, none, 0);
                replies->off.push_back(replies->bytes.size());
            }
    }
    replies->first[n] = replies->off.size() - 1;
}

// fn(i) for i in [0, n), on up to 8 threads (the library's entry points are re-entrant: a stream per calling thread):
// a window's ExactMatch / Reads requests make one engine call per distinct query length -- dozens of small launch
// sequences, each waiting for its own copy back -- and one per (partition, tile length).  The first error wins.
template <class F>
static int for_each_parallel(size_t n, F &&fn) {
    if (n == 0) return RSBWT_OK;
    const size_t T = std::min<size_t>({n, (size_t)8, (size_t)std::max(1u, std::thread::hardware_concurrency())});
    if (T <= 1) {
        for (size_t i = 0; i < n; ++i) {
            const int rc = fn(i);
            if (rc != RSBWT_OK) return rc;
        }
        return RSBWT_OK;
    }
    std::atomic<size_t> next{0};
    std::atomic<int> err{RSBWT_OK};
    std::vector<std::string> msg(T);
    auto work = [&](size_t t) {
        for (size_t i = next.fetch_add(1); i < n && err.load(std::memory_order_relaxed) == RSBWT_OK; i = next.fetch_add(1)) {
            int rc;
            try {
                rc = fn(i);
            } catch (...) {
                rc = RSBWT_ENOMEM;
            }
            if (rc != RSBWT_OK) {
                int none = RSBWT_OK;
                if (err.compare_exchange_strong(none, rc)) msg[t] = rsbwt_last_error();  // (thread-local: carried over below)
            }
        }
    };
    std::vector<std::thread> th;
    try {
        for (size_t t = 1; t < T; ++t) th.emplace_back(work, t);
    } catch (...) {  // no more threads to be had: the ones that started and this one do the work
    }
    work(0);
    for (auto &t : th) t.join();
    const int rc = err.load();
    if (rc != RSBWT_OK)
        for (const std::string &m : msg)
            if (!m.empty()) return fail(rc, "%s", m.c_str());
    return rc;
}

query_engine query_engine_hooks = {nullptr};
meta_engine meta_engine_hooks = {nullptr, nullptr};

namespace {

sample_codec codec_of(const reads_config &cfg) {
    sample_codec c;
    c.hash = &cfg.hash;
    c.size_of_sample = cfg.size_of_sample;
    c.has_other = cfg.has_other_meta_data;
    return c;
}

// The sample values of the reads of a batch's All / Samples Replies: entry e of list li (a read of partition
// lshard[li][e]) has value bytes[first[at[li] + e] .. first[at[li] + e + 1]).  One rsbwt_set_read_meta_var call over
// all those reads: read x is query x, its value in ITS partition p is item x * S + p -- the other partitions' items of
// that query are answered and not used.
struct all_values {
    std::vector<size_t> at;      // first entry of list li among the looked-up reads (lists that are not All: unused)
    std::vector<uint32_t> shard;  // per looked-up read
    std::vector<uint64_t> first;
    std::vector<uint8_t> bytes;
    size_t S = 1;
    int lookup(rsbwt_set_t *set, const std::vector<std::vector<const std::string *>> &lists, const std::vector<std::vector<uint32_t>> &lshard,
               const std::vector<char> &is_all) {
        S = rsbwt_set_size(set);
        at.assign(lists.size(), 0);
        std::string text;
        std::vector<uint64_t> off(1, 0);
        for (size_t li = 0; li < lists.size(); ++li) {
            if (!is_all[li]) continue;
            at[li] = shard.size();
            for (size_t e = 0; e < lists[li].size(); ++e) {
                text += *lists[li][e];
                off.push_back(text.size());
                shard.push_back(lshard[li][e]);
            }
        }
        const size_t Q = shard.size();
        first.assign(Q * S + 1, 0);
        if (Q == 0) return RSBWT_OK;
        if (!meta_engine_hooks.read_meta_var) return fail(RSBWT_ENODEV, "the sample table is not part of this build");
        size_t need = 0;
        bytes.resize(64 * Q + 256);  // (a typical value is a few records; a call that does not fit says what does)
        int rc = meta_engine_hooks.read_meta_var(set, text.data(), off.data(), Q, first.data(), bytes.data(), bytes.size(), &need, nullptr);
        if (rc == RSBWT_ERANGE) {
            bytes.resize(need);
            rc = meta_engine_hooks.read_meta_var(set, text.data(), off.data(), Q, first.data(), bytes.data(), bytes.size(), &need, nullptr);
        }
        return rc;
    }
    // the Reply of list li (QueryTask::run / KmerTask::run with return type All or Samples); bytes needed, written when p
    size_t encode(uint8_t *p, size_t cap, size_t li, const std::vector<const std::string *> &l, int t, int rt, const std::string &q, bool revcomp,
                  const sample_codec &codec) const {
        const size_t m = l.size();
        std::vector<const char *> rp(m);
        std::vector<size_t> rl(m), vl(m);
        std::vector<const uint8_t *> vp(m);
        for (size_t e = 0; e < m; ++e) {
            const size_t x = at[li] + e, item = x * S + shard[x];
            rp[e] = l[e]->data();
            rl[e] = l[e]->size();
            vp[e] = bytes.data() + first[item];
            vl[e] = (size_t)(first[item + 1] - first[item]);
        }
        return meta_encode_all_reply(p, cap, t, rt, q.data(), q.size(), revcomp, rp.data(), rl.data(), vp.data(), vl.data(), m, codec);
    }
};

}  // namespace

int service_reads_batch(rsbwt_set_t *set, const std::vector<service_request> &rq, bool per_partition, const reads_config &cfg,
                        reply_arena *replies, std::vector<char> *handled, std::vector<char> *capped) {
    const size_t n = rq.size(), S = rsbwt_set_size(set);
    if (capped) capped->assign(n, 0);
    const uint64_t LIMIT = cfg.max_match_reads;
    if (LIMIT && !query_engine_hooks.query_var_capped) return fail(RSBWT_ENODEV, "max_match_reads needs the engine: it is not part of this build");
    const size_t MINL = cfg.min_read_length, MAXL = cfg.max_read_length;
    handled->assign(n, 0);
    replies->bytes.clear();
    replies->off.assign(1, 0);
    replies->first.assign(n + 1, 0);
    auto suffix_of = [&](size_t p) -> const std::string & {
        static const std::string none;
        return p < cfg.suffix.size() ? cfg.suffix[p] : none;
    };
    // a (request, strand) = one call of find_reads per partition; its result per partition: the tile matches, then the
    // reads of query() / of the interval
    struct job_t {
        size_t req;
        int strand;
        std::string w;
        std::vector<std::vector<std::string>> tiles;  // [shard]: tiles that are reads of that partition, in find_reads' order
        std::vector<std::vector<std::string>> reads;  // [shard]: query(w) / the interval's rows
        bool over = false;                            // its rows exceed cfg.max_match_reads: answered with no matches at all
    };
    std::vector<job_t> jobs;
    for (size_t i = 0; i < n; ++i) {
        if (!service_takes_reads(rq[i], cfg)) continue;
        (*handled)[i] = 1;
        for (int strand = 0; strand < 2; ++strand) {
            job_t j;
            j.req = i;
            j.strand = strand;
            j.w = strand ? rev_comp(rq[i].q.data(), rq[i].q.size()) : rq[i].q;  // QueryTask::run, service.cpp:1268-1272
            j.tiles.resize(S);
            j.reads.resize(S);
            jobs.push_back(std::move(j));
        }
    }
    if (jobs.empty()) {
        replies->first.assign(n + 1, 0);
        return RSBWT_OK;
    }
    // RSBWT_SERVICE_TIMING: a line per window on stderr with what its phases took (diagnosis, tools/README.md)
    static const bool timing = getenv("RSBWT_SERVICE_TIMING") != nullptr;
    auto now = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double t_begin = timing ? now() : 0.0;
    double t_tiles = 0, t_exact = 0, t_query = 0;
    // ---- the tiles (service.cpp:755-764,773-794): MAX-long ones of a query of MAX or more, then MIN-long ones (of any
    // query longer than MIN; not again when MIN == MAX).  A tile is looked up in the partitions whose suffix it ends
    // with; query_exactmatch (query.cpp:102-120) says whether it is a read there.  One batched call per (partition, length).
    struct cand_t {
        size_t job, seq;  // seq: the tile's place in find_reads' order within the job
        std::string tile;
    };
    std::map<std::pair<size_t, size_t>, std::vector<cand_t>> by_shard_len;  // (shard, tile length) -> candidates
    std::vector<size_t> nseq(jobs.size(), 0);
    for (size_t ji = 0; ji < jobs.size(); ++ji) {
        const std::string &w = jobs[ji].w;
        const size_t sz = w.size();
        std::vector<size_t> lens;
        if (sz >= MAXL) {
            lens.push_back(MAXL);
            if (MINL != MAXL) lens.push_back(MINL);
        } else if (sz >= MINL && sz != MINL) {
            lens.push_back(MINL);
        }
        for (size_t T : lens) {
            const std::unordered_set<std::string> vs = get_tiles(w, T);
            for (const std::string &tile : vs) {
                const size_t seq = nseq[ji]++;
                for (size_t p = 0; p < S; ++p)
                    if (is_suffix_of(suffix_of(p), tile)) by_shard_len[{p, T}].push_back(cand_t{ji, seq, tile});
            }
        }
    }
    if (timing) t_tiles = now();
    std::vector<std::vector<std::pair<size_t, std::pair<size_t, std::string>>>> hits(jobs.size());  // job -> (seq, (shard, tile))
    {
        // the (partition, tile length) groups side by side; what each found is merged afterwards (a job's tiles may
        // sit in several groups)
        std::vector<std::pair<const std::pair<size_t, size_t>, std::vector<cand_t>> *> groups;
        for (auto &g : by_shard_len) groups.push_back(&g);
        std::vector<std::vector<uint8_t>> found(groups.size());
        const int rc = for_each_parallel(groups.size(), [&](size_t gi) -> int {
            const size_t p = groups[gi]->first.first, T = groups[gi]->first.second, m = groups[gi]->second.size();
            if (T == 0 || m == 0) return RSBWT_OK;
            std::string flat(m * T, 'N');
            for (size_t j = 0; j < m; ++j) memcpy(&flat[j * T], groups[gi]->second[j].tile.data(), T);
            found[gi].assign(m, 0);
            return rsbwt_query_exactmatch(rsbwt_set_shard(set, p), flat.data(), m, (uint32_t)T, T, found[gi].data());
        });
        if (rc != RSBWT_OK) return rc;
        for (size_t gi = 0; gi < groups.size(); ++gi)
            for (size_t j = 0; j < found[gi].size(); ++j)
                if (found[gi][j]) hits[groups[gi]->second[j].job].push_back({groups[gi]->second[j].seq, {groups[gi]->first.first, groups[gi]->second[j].tile}});
    }
    for (size_t ji = 0; ji < jobs.size(); ++ji) {
        std::sort(hits[ji].begin(), hits[ji].end(), [](const auto &a, const auto &b) { return a.first < b.first; });
        for (auto &h : hits[ji]) jobs[ji].tiles[h.second.first].push_back(std::move(h.second.second));
    }
    if (timing) t_exact = now();
    // ---- the reads that CONTAIN w: query() for MIN <= |w| < MAX (service.cpp:767; query.cpp:87-100), the interval's
    // rows for |w| < MIN (service.cpp:718-753).
    // The jobs' queries have lengths of their own: rsbwt_set_query_var answers a slice of them in ONE search + ONE
    // extraction (until round 5: a call per distinct length, 75 of them in a window of 4,096 requests).  Slices of 2,048
    // jobs, side by side on the worker's threads.
    std::vector<std::vector<size_t>> slices;
    for (size_t ji = 0; ji < jobs.size(); ++ji) {
        const size_t sz = jobs[ji].w.size();
        if (sz == 0 || sz >= MAXL) continue;
        if (slices.empty() || slices.back().size() >= 2048) slices.emplace_back();
        slices.back().push_back(ji);
    }
    // (the slices write into jobs of their own)
    const int rc_len = for_each_parallel(slices.size(), [&](size_t gi) -> int {
        const std::vector<size_t> &members = slices[gi];
        const size_t m = members.size();
        std::string flat;
        std::vector<uint64_t> qoff(m + 1, 0);
        for (size_t j = 0; j < m; ++j) {
            flat += jobs[members[j]].w;
            qoff[j + 1] = flat.size();
        }
        std::vector<uint64_t> first(m + 1, 0);
        size_t nreads = 0;
        uint32_t stride = (uint32_t)std::max<size_t>(256, (2 * MAXL + 63) & ~(size_t)15);
        std::vector<char> reads;
        std::vector<uint32_t> rlen, rshard;
        size_t room = 16 * m + 256;  // reads the buffers hold: one call answers when they fit, else it says how many there are
        // (with a limit a query brings LIMIT rows at most: the call itself bounds what the buffers must hold)
        std::vector<uint64_t> matches(LIMIT ? m : 0);
        for (int attempt = 0;; ++attempt) {
            int rc = RSBWT_ERANGE;
            for (int sized = 0; sized < 2 && rc == RSBWT_ERANGE; ++sized) {
                reads.assign(room * (size_t)stride, 0);
                rlen.assign(room, 0);
                rshard.assign(room, 0);
                rc = LIMIT ? query_engine_hooks.query_var_capped(set, flat.data(), qoff.data(), m, LIMIT, first.data(), rshard.data(), reads.data(),
                                                                 stride, rlen.data(), room, &nreads, matches.data())
                           : rsbwt_set_query_var(set, flat.data(), qoff.data(), m, first.data(), rshard.data(), reads.data(), stride, rlen.data(), room, &nreads);
                if (rc == RSBWT_ERANGE && nreads > room) room = nreads;
            }
            if (rc != RSBWT_OK) return rc;
            for (size_t j = 0; j < matches.size(); ++j)
                if (matches[j] > LIMIT) jobs[members[j]].over = true;
            if (nreads == 0) break;
            bool over = false;
            for (size_t r = 0; r < nreads && !over; ++r) over = rlen[r] == 0xFFFFFFFFu;
            if (!over || attempt == 2) break;
            stride = attempt == 0 ? 4096u : 65536u;  // a read longer than the buffer (none in a collection built for these lengths): once more, wider
        }
        for (size_t j = 0; j < m && nreads; ++j) {
            job_t &jb = jobs[members[j]];
            const size_t k = jb.w.size();
            // this query's reads arrive shard by shard (shard 0's first), each shard's in SA-row order
            std::vector<size_t> begin_of(S + 1, 0);
            for (uint64_t r = first[j]; r < first[j + 1]; ++r) begin_of[rshard[r] + 1]++;
            for (size_t p = 0; p < S; ++p) begin_of[p + 1] += begin_of[p];
            for (size_t p = 0; p < S; ++p) {
                const size_t cnt = begin_of[p + 1] - begin_of[p], base = (size_t)first[j] + begin_of[p];
                const size_t head = k < MINL ? chunked_head(cnt) : 0;  // (find_reads' own extraction reorders wide intervals; query() does not)
                std::vector<std::string> &out = jb.reads[p];
                out.reserve(cnt);
                for (size_t t = 0; t < cnt; ++t) {
                    const size_t r = base + (t + head < cnt ? t + head : t + head - cnt);
                    if (rlen[r] == 0xFFFFFFFFu) continue;  // (longer than 64 KB: not a read of this service)
                    out.emplace_back(reads.data() + r * (size_t)stride, rlen[r]);
                }
            }
        }
        return RSBWT_OK;
    });
    if (rc_len != RSBWT_OK) return rc_len;
    // a strand over the limit: no tile matches either -- the Reply of an empty result (rsbwt_proto_encode_empty_reply)
    for (job_t &jb : jobs)
        if (jb.over) {
            for (auto &l : jb.tiles) l.clear();
            for (auto &l : jb.reads) l.clear();
            if (capped) (*capped)[jb.req] = 1;
        }
    if (timing) t_query = now();
    // ---- Reply bytes: request by request, partition by partition (or all partitions' lists joined, shard 0's first),
    // forward then reverse complement
    const size_t rows = per_partition ? S : 1;
    std::vector<std::vector<const std::string *>> lists(jobs.size() * rows);
    std::vector<std::vector<uint32_t>> lshard(lists.size());  // the partition each entry came from (its samples are that partition's)
    for (size_t ji = 0; ji < jobs.size(); ++ji)
        for (size_t p = 0; p < S; ++p) {
            std::vector<const std::string *> &l = lists[ji * rows + (per_partition ? p : 0)];
            // (a partition's list: its tile matches first, then the reads that contain w: service.cpp:757-769)
            for (const std::string &t : jobs[ji].tiles[p]) l.push_back(&t);
            for (const std::string &t : jobs[ji].reads[p]) l.push_back(&t);
            lshard[ji * rows + (per_partition ? p : 0)].resize(l.size(), (uint32_t)p);
        }
    // All / Samples: every read of those requests' lists is looked up in its partition's sample table, in one call
    std::vector<char> is_all(lists.size(), 0);
    for (size_t ji = 0; ji < jobs.size(); ++ji)
        if (service_is_all_return(rq[jobs[ji].req]))
            for (size_t r = 0; r < rows; ++r) is_all[ji * rows + r] = 1;
    all_values vals;
    {
        const int rc = vals.lookup(set, lists, lshard, is_all);
        if (rc != RSBWT_OK) return rc;
    }
    const sample_codec codec = codec_of(cfg);
    if (!per_partition) {
        // joined lists keep find_reads' order WITHIN a partition; across partitions the front-end concatenates in
        // arrival order (server.cpp:199-261): here shard order, tiles and reads of shard 0 first
    }
    std::vector<size_t> body(lists.size());
    size_t total = 0, messages = 0;
    for (size_t ji = 0; ji < jobs.size(); ++ji)
        for (size_t r = 0; r < rows; ++r) {
            const size_t li = ji * rows + r;
            const service_request &q = rq[jobs[ji].req];
            if (is_all[li]) {
                total += vals.encode(nullptr, 0, li, lists[li], q.t, q.rt, q.q, jobs[ji].strand == 1, codec);
            } else {
                body[li] = reads_body_len(lists[li]);
                total += reads_reply_len(q.t, q.q.size(), body[li]);
            }
            ++messages;
        }
    replies->bytes.resize(total);
    replies->off.reserve(messages + 1);
    uint8_t *p = replies->bytes.data();
    size_t ji = 0;
    for (size_t i = 0; i < n; ++i) {
        replies->first[i] = replies->off.size() - 1;
        if (!(*handled)[i]) continue;
        // jobs[ji] = forward, jobs[ji + 1] = reverse complement of request i; per partition: forward, then reverse
        // complement (the count path's order)
        for (size_t r = 0; r < rows; ++r)
            for (int strand = 0; strand < 2; ++strand) {
                const size_t li = (ji + strand) * rows + r;
                if (is_all[li]) p += vals.encode(p, (size_t)(replies->bytes.data() + total - p), li, lists[li], rq[i].t, rq[i].rt, rq[i].q, strand == 1, codec);
                else p = encode_reads_reply(p, rq[i].t, rq[i].q, strand == 1, lists[li], body[li]);
                replies->off.push_back((size_t)(p - replies->bytes.data()));
            }
        ji += 2;
    }
    replies->first[n] = replies->off.size() - 1;
    if (timing)
        fprintf(stderr, "rsbwt reads window: %zu requests, tiles %.1f ms, exact-match calls %.1f (%zu groups), query calls %.1f (%zu slices), replies %.1f ms (%zu bytes)\n",
                jobs.size() / 2, t_tiles - t_begin, t_exact - t_tiles, by_shard_len.size(), t_query - t_exact, slices.size(), now() - t_query, total);
    return RSBWT_OK;
}

// ---- KmerMatch Count / Reads: find_kmer_reads (service.cpp:466-502) batched, KmerTask::run's replies (:871-960) ------
kmer_engine kmer_engine_hooks = {nullptr, nullptr};

namespace {

// Reply{rt, t = 3 | 4, q, a = ReplyAll{forward_matches | revcomp_matches = ResultAll{r}}*} (readserver.proto:25-28,51-54)
size_t all_body_len(const std::vector<const std::string *> &reads) { return reads_body_len(reads); }  // ResultAll{r} = ResultReads{r} on the wire
uint8_t *encode_all_reply(uint8_t *p, int request_type, int reply_type, const std::string &q, bool revcomp,
                          const std::vector<const std::string *> &reads, size_t body) {
    *p++ = 0x08; p = put_varint(p, (uint64_t)request_type);
    *p++ = 0x10; p = put_varint(p, (uint64_t)reply_type);
    *p++ = 0x1A; p = put_varint(p, q.size());
    if (!q.empty()) memcpy(p, q.data(), q.size());
    p += q.size();
    *p++ = 0x32; p = put_varint(p, body);  // a
    for (const std::string *s : reads) {
        const size_t rr = 1 + varint_len(s->size()) + s->size();
        *p++ = revcomp ? 0x12 : 0x0A; p = put_varint(p, rr);
        *p++ = 0x0A; p = put_varint(p, s->size());
        if (!s->empty()) memcpy(p, s->data(), s->size());
        p += s->size();
    }
    return p;
}
size_t all_reply_len(int request_type, int reply_type, size_t qlen, size_t body) {
    return 1 + varint_len((uint64_t)request_type) + 1 + varint_len((uint64_t)reply_type) + 1 + varint_len(qlen) + qlen + 1 + varint_len(body) + body;
}

// KmerTask::run's Reply for return type rt (1 Count: c = the set's size; 2 Reads: r; else a) appended to *out
void append_kmer_reply(std::vector<uint8_t> *out, int request_type, int rt, const std::string &q, bool revcomp,
                       const std::vector<const std::string *> &reads, uint64_t count) {
    const size_t at = out->size();
    if (rt == 1) {
        const int32_t c = (int32_t)(uint32_t)count;  // set_c(vsize): narrowed to int32 (readserver.proto:31-33)
        out->resize(at + count_reply_len(request_type, q.size(), c));
        encode_count_reply(out->data() + at, request_type, q.data(), q.size(), revcomp, c);
    } else if (rt == 2) {
        const size_t body = reads_body_len(reads);
        out->resize(at + reads_reply_len(request_type, q.size(), body));
        encode_reads_reply(out->data() + at, request_type, q, revcomp, reads, body);
    } else {
        const size_t body = all_body_len(reads);
        out->resize(at + all_reply_len(request_type, rt, q.size(), body));
        encode_all_reply(out->data() + at, request_type, rt, q, revcomp, reads, body);
    }
}

}  // namespace

void service_append_empty(const service_request &r, size_t rows, reply_arena *replies) {
    const std::vector<const std::string *> none;
    for (size_t row = 0; row < rows; ++row)
        for (int strand = 0; strand < 2; ++strand) {
            append_kmer_reply(&replies->bytes, r.t, r.rt, r.q, strand == 1, none, 0);
            replies->off.push_back(replies->bytes.size());
        }
}

int service_kmer_batch(rsbwt_set_t *set, const std::vector<service_request> &rq, bool per_partition, const reads_config &cfg,
                       reply_arena *replies, std::vector<char> *handled) {
    const size_t n = rq.size(), S = rsbwt_set_size(set);
    handled->assign(n, 0);
    replies->bytes.clear();
    replies->off.assign(1, 0);
    replies->first.assign(n + 1, 0);
    std::vector<kmer_job> jobs;
    for (size_t i = 0; i < n; ++i) {
        if (!service_takes_kmer(rq[i], cfg)) continue;
        (*handled)[i] = 1;
        for (int strand = 0; strand < 2; ++strand) {
            kmer_job j;
            j.w = strand ? rev_comp(rq[i].q.data(), rq[i].q.size()) : rq[i].q;  // KmerTask::run, service.cpp:883-885
            j.k = rq[i].k;     // (size_t) request->k(): a negative k never tiles (get_tiles :236-239)
            j.skip = rq[i].s;  // a negative skip: answered empty
            jobs.push_back(std::move(j));
        }
    }
    if (jobs.empty()) return RSBWT_OK;
    static const bool timing = getenv("RSBWT_SERVICE_TIMING") != nullptr;
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<std::vector<std::vector<std::string>>> res;
    std::vector<char> failed;
    kmer_work wk;
    const uint32_t stride = (uint32_t)std::max<size_t>(256, (2 * cfg.max_read_length + 63) & ~(size_t)15);
    if (!kmer_engine_hooks.batch) return fail(RSBWT_ENODEV, "the k-mer path is not part of this build");
    const int rc = kmer_engine_hooks.batch(set, jobs, cfg.min_read_length, cfg.max_read_length, stride, &res, &failed, &wk);
    if (rc != RSBWT_OK) return rc;
    const size_t rows = per_partition ? S : 1;
    // the lists of the All / Samples requests (KmerTask::run, service.cpp:917-975: each read with its samples), looked up
    // in one call; list (job, row) as the loop below walks them
    std::vector<std::vector<const std::string *>> lists(jobs.size() * rows);
    std::vector<std::vector<uint32_t>> lshard(lists.size());
    std::vector<char> is_all(lists.size(), 0);
    {
        size_t ji = 0;
        for (size_t i = 0; i < n; ++i) {
            if (!(*handled)[i]) continue;
            for (int strand = 0; strand < 2; ++strand)
                for (size_t r = 0; r < rows; ++r) {
                    const size_t li = (ji + strand) * rows + r;
                    // per partition: that shard's set; summed: counts added up, lists joined in shard order
                    for (size_t p = per_partition ? r : 0; p < (per_partition ? r + 1 : S); ++p)
                        for (const std::string &x : res[ji + strand][p]) {
                            lists[li].push_back(&x);
                            lshard[li].push_back((uint32_t)p);
                        }
                    is_all[li] = service_is_all_return(rq[i]) ? 1 : 0;
                }
            ji += 2;
        }
    }
    all_values vals;
    {
        const int rv = vals.lookup(set, lists, lshard, is_all);
        if (rv != RSBWT_OK) return rv;
    }
    const sample_codec codec = codec_of(cfg);
    size_t ji = 0;
    for (size_t i = 0; i < n; ++i) {
        replies->first[i] = replies->off.size() - 1;
        if (!(*handled)[i]) continue;
        for (size_t r = 0; r < rows; ++r)
            for (int strand = 0; strand < 2; ++strand) {
                const size_t li = (ji + strand) * rows + r;
                if (is_all[li]) {
                    const size_t at = replies->bytes.size(), len = vals.encode(nullptr, 0, li, lists[li], rq[i].t, rq[i].rt, rq[i].q, strand == 1, codec);
                    replies->bytes.resize(at + len);
                    vals.encode(replies->bytes.data() + at, len, li, lists[li], rq[i].t, rq[i].rt, rq[i].q, strand == 1, codec);
                } else {
                    append_kmer_reply(&replies->bytes, rq[i].t, rq[i].rt, rq[i].q, strand == 1, lists[li], lists[li].size());
                }
                replies->off.push_back(replies->bytes.size());
            }
        ji += 2;
    }
    replies->first[n] = replies->off.size() - 1;
    if (timing)
        fprintf(stderr, "rsbwt kmer window: %zu requests, %.1f ms, %llu candidate rows, %llu walked to '$', %llu LF steps, %llu identities, %llu extracted\n",
                jobs.size() / 2, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(),
                (unsigned long long)wk.candidates, (unsigned long long)wk.walked, (unsigned long long)wk.lf_steps,
                (unsigned long long)wk.identities, (unsigned long long)wk.extracted);
    return RSBWT_OK;
}

// ---- SiteMatch: GtTask::run (service.cpp:1014-1210) over rsbwt_set_site_reads ----------------------------------------
site_engine site_engine_hooks = {nullptr, nullptr};

bool service_site_fixup(const std::string &q, int64_t p, const std::string &a, bool revcomp, size_t L, std::string *w, int64_t *pos, std::string *alt) {
    std::string query = q;
    int64_t at = p;
    *alt = a;
    if (revcomp) {  // :1028-1032
        query = rev_comp(q.data(), q.size());
        at = (int64_t)q.size() - p + 1;
        *alt = rev_comp(a.data(), a.size());
    }
    w->clear();
    *pos = at;
    if (at < 0) return false;  // (the reference takes pos as size_t: undefined from here on)
    const int64_t max_len = (int64_t)L;
    if (at <= max_len) {  // :1034-1036
        *w = query.substr(0, (size_t)(max_len + at - 1 > 0 ? max_len + at - 1 : 0));
    } else {  // :1037-1040
        if ((uint64_t)(at - max_len) > query.size()) return false;  // (substr throws there)
        *w = query.substr((size_t)(at - max_len), (size_t)(2 * max_len - 1));
        *pos = at = max_len;
    }
    return (uint64_t)at <= w->size();  // :1044
}

namespace {

// Reply{rt, t, q}: what GtTask::run sends after its "ERROR" line (no c / r / a sub-message)
void append_header_reply(std::vector<uint8_t> *out, int request_type, int reply_type, const std::string &q) {
    const size_t at = out->size();
    out->resize(at + 1 + varint_len((uint64_t)request_type) + 1 + varint_len((uint64_t)reply_type) + 1 + varint_len(q.size()) + q.size());
    uint8_t *p = out->data() + at;
    *p++ = 0x08; p = put_varint(p, (uint64_t)request_type);
    *p++ = 0x10; p = put_varint(p, (uint64_t)reply_type);
    *p++ = 0x1A; p = put_varint(p, q.size());
    if (!q.empty()) memcpy(p, q.data(), q.size());
}

struct site_strand {
    size_t req = 0;
    bool header = false, run = false;  // header: no sub-message; run: an item of an engine call (else nothing is kept)
    std::string w, alt;
    int64_t pos = 0;
    std::vector<std::vector<std::string>> reads;  // [shard], ascending read_row
    std::vector<uint64_t> count;                  // [shard]
};

}  // namespace

void service_site_empty(const std::vector<service_request> &rq, size_t rows, const reads_config &cfg, reply_arena *replies, std::vector<char> *handled) {
    const size_t n = rq.size();
    const std::vector<const std::string *> none;
    handled->assign(n, 0);
    replies->bytes.clear();
    replies->off.assign(1, 0);
    replies->first.assign(n + 1, 0);
    for (size_t i = 0; i < n; ++i) {
        replies->first[i] = replies->off.size() - 1;
        if (!service_takes_site(rq[i], cfg)) continue;
        (*handled)[i] = 1;
        bool header[2];
        for (int strand = 0; strand < 2; ++strand) {
            std::string w, alt;
            int64_t pos;
            header[strand] = !service_site_fixup(rq[i].q, rq[i].p, rq[i].a, strand == 1, cfg.max_read_length, &w, &pos, &alt);
        }
        for (size_t r = 0; r < rows; ++r)
            for (int strand = 0; strand < 2; ++strand) {
                if (header[strand]) append_header_reply(&replies->bytes, rq[i].t, rq[i].rt, rq[i].q);
                else append_kmer_reply(&replies->bytes, rq[i].t, rq[i].rt, rq[i].q, strand == 1, none, 0);
                replies->off.push_back(replies->bytes.size());
            }
    }
    replies->first[n] = replies->off.size() - 1;
}

int service_site_batch(rsbwt_set_t *set, const std::vector<service_request> &rq, bool per_partition, const reads_config &cfg, reply_arena *replies,
                       std::vector<char> *handled) {
    const size_t n = rq.size(), S = rsbwt_set_size(set), L = cfg.max_read_length;
    handled->assign(n, 0);
    replies->bytes.clear();
    replies->off.assign(1, 0);
    replies->first.assign(n + 1, 0);
    std::vector<site_strand> st;  // 2 per handled request: forward, reverse complement
    std::map<std::pair<int32_t, int32_t>, std::vector<size_t>> by_ks;  // one engine call per distinct (k, s)
    for (size_t i = 0; i < n; ++i) {
        if (!service_takes_site(rq[i], cfg)) continue;
        (*handled)[i] = 1;
        for (int strand = 0; strand < 2; ++strand) {
            site_strand x;
            x.req = i;
            x.header = !service_site_fixup(rq[i].q, rq[i].p, rq[i].a, strand == 1, L, &x.w, &x.pos, &x.alt);
            // (an empty a keeps nothing; pos = 0, k <= 0, s < 0 and k > |w| are the engine's own rule: gt_make_plan, rsbwt_gt_align)
            x.run = !x.header && !x.alt.empty();
            x.reads.resize(S);
            x.count.assign(S, 0);
            if (x.run) by_ks[{rq[i].k, rq[i].s}].push_back(st.size());
            st.push_back(std::move(x));
        }
    }
    if (st.empty()) return RSBWT_OK;
    if (!by_ks.empty() && (!site_engine_hooks.reads || !site_engine_hooks.counts)) return fail(RSBWT_ENODEV, "the SiteMatch path is not part of this build");
    const uint32_t stride = (uint32_t)std::max<size_t>(256, (2 * L + 63) & ~(size_t)15);
    for (auto &g : by_ks) {
        const std::vector<size_t> &members = g.second;
        const size_t m = members.size();
        std::string text, alt(m, 'N');
        std::vector<uint64_t> off(m + 1, 0), pos(m);
        std::vector<uint8_t> isalt(m);
        bool want_reads = false;
        for (size_t j = 0; j < m; ++j) {
            const site_strand &x = st[members[j]];
            text += x.w;
            off[j + 1] = text.size();
            pos[j] = (uint64_t)x.pos;
            alt[j] = x.alt[0];  // alt[q]: the first character
            isalt[j] = rq[x.req].isalt == 1 ? 1 : 0;  // :1018
            want_reads = want_reads || rq[x.req].rt != 1;
        }
        std::vector<uint64_t> first(m * S + 1, 0);
        if (!want_reads) {
            std::vector<uint64_t> counts(m * S, 0);
            const int rc = site_engine_hooks.counts(set, text.data(), off.data(), m, pos.data(), alt.data(), isalt.data(), g.first.first, g.first.second, 0,
                                                    counts.data());
            if (rc != RSBWT_OK) return rc;
            for (size_t j = 0; j < m; ++j)
                for (size_t p = 0; p < S; ++p) st[members[j]].count[p] = counts[j * S + p];
            continue;
        }
        size_t room = 64 * m + 256, nreads = 0;  // one call answers when the reads fit, else it says how many there are
        std::vector<char> reads;
        std::vector<uint32_t> rlen;
        int rc = RSBWT_ERANGE;
        for (int sized = 0; sized < 2 && rc == RSBWT_ERANGE; ++sized) {
            reads.assign(room * (size_t)stride, 0);
            rlen.assign(room, 0);
            rc = site_engine_hooks.reads(set, text.data(), off.data(), m, pos.data(), alt.data(), isalt.data(), g.first.first, g.first.second, 0, first.data(),
                                         reads.data(), stride, rlen.data(), nullptr, room, &nreads);
            if (rc == RSBWT_ERANGE && nreads > room) room = nreads;
        }
        if (rc != RSBWT_OK) return rc;
        for (size_t j = 0; j < m; ++j)
            for (size_t p = 0; p < S; ++p) {
                site_strand &x = st[members[j]];
                x.count[p] = first[j * S + p + 1] - first[j * S + p];
                for (uint64_t r = first[j * S + p]; r < first[j * S + p + 1]; ++r)
                    if (rlen[r] != 0xFFFFFFFFu) x.reads[p].emplace_back(reads.data() + r * (size_t)stride, rlen[r]);  // (longer: not a read of this service)
            }
    }
    // ---- the Replies: request by request, partition by partition (or the partitions' lists joined in partition order and
    // the counts summed), forward then reverse complement
    const size_t rows = per_partition ? S : 1;
    std::vector<std::vector<const std::string *>> lists(st.size() * rows);
    std::vector<std::vector<uint32_t>> lshard(lists.size());
    std::vector<uint64_t> counts(lists.size(), 0);
    std::vector<char> is_all(lists.size(), 0);
    for (size_t si = 0; si < st.size(); ++si)
        for (size_t r = 0; r < rows; ++r) {
            const size_t li = si * rows + r;
            for (size_t p = per_partition ? r : 0; p < (per_partition ? r + 1 : S); ++p) {
                counts[li] += st[si].count[p];
                for (const std::string &x : st[si].reads[p]) {
                    lists[li].push_back(&x);
                    lshard[li].push_back((uint32_t)p);
                }
            }
            is_all[li] = !st[si].header && service_is_all_return(rq[st[si].req]) ? 1 : 0;
        }
    all_values vals;
    {
        const int rv = vals.lookup(set, lists, lshard, is_all);
        if (rv != RSBWT_OK) return rv;
    }
    const sample_codec codec = codec_of(cfg);
    size_t si = 0;
    for (size_t i = 0; i < n; ++i) {
        replies->first[i] = replies->off.size() - 1;
        if (!(*handled)[i]) continue;
        for (size_t r = 0; r < rows; ++r)
            for (int strand = 0; strand < 2; ++strand) {
                const size_t li = (si + strand) * rows + r;
                if (st[si + strand].header) {
                    append_header_reply(&replies->bytes, rq[i].t, rq[i].rt, rq[i].q);
                } else if (is_all[li]) {
                    const size_t at = replies->bytes.size(), len = vals.encode(nullptr, 0, li, lists[li], rq[i].t, rq[i].rt, rq[i].q, strand == 1, codec);
                    replies->bytes.resize(at + len);
                    vals.encode(replies->bytes.data() + at, len, li, lists[li], rq[i].t, rq[i].rt, rq[i].q, strand == 1, codec);
                } else {
                    append_kmer_reply(&replies->bytes, rq[i].t, rq[i].rt, rq[i].q, strand == 1, lists[li], counts[li]);
                }
                replies->off.push_back(replies->bytes.size());
            }
        si += 2;
    }
    replies->first[n] = replies->off.size() - 1;
    return RSBWT_OK;
}

bool service_decode(const uint8_t *msg, size_t len, service_request *out) {
    request_view r;
    if (!decode_request(msg, len, r)) return false;
    out->t = r.t;
    out->rt = r.rt;
    out->q.assign(r.q ? r.q : "", r.qlen);
    out->k = r.k;
    out->s = r.s;
    out->has_k = r.has_k;
    out->has_s = r.has_s;
    out->p = r.p;
    out->isalt = r.isalt;
    out->a.assign(r.a ? r.a : "", r.alen);
    return true;
}

}  // namespace rsb

extern "C" {

static int rsbwt_service_counts_body(rsbwt_set_t *set, const uint8_t *requests, size_t requests_len, const uint64_t *req_off,
                         size_t n, uint8_t *replies, size_t cap, uint64_t *rep_off, size_t *needed) {
    if (!set || (!requests && n) || !req_off || !rep_off) return rsb::fail(RSBWT_EINVAL, "null argument");
    for (size_t i = 0; i < n; ++i)
        if (req_off[i] > req_off[i + 1] || req_off[i + 1] > requests_len)
            return rsb::fail(RSBWT_EINVAL, "request %zu: offsets %llu..%llu are not an ascending range inside the %zu-byte buffer",
                             i, (unsigned long long)req_off[i], (unsigned long long)req_off[i + 1], requests_len);
    try {
        std::vector<rsb::service_request> rq(n);
        std::vector<char> parsed(n, 0);
        for (size_t i = 0; i < n; ++i)
            parsed[i] = rsb::service_decode(requests + req_off[i], (size_t)(req_off[i + 1] - req_off[i]), &rq[i]) ? 1 : 0;
        for (size_t i = 0; i < n; ++i)
            if (!parsed[i]) rq[i].t = 0;  // not a Request: no reply
        rsb::reply_arena rep;
        std::vector<char> handled;
        const int rc = rsb::service_count_batch(set, rq, false, &rep, &handled);
        if (rc != RSBWT_OK) return rc;
        const size_t total = rep.bytes.size();
        rep_off[0] = 0;
        for (size_t i = 0; i < n; ++i)
            for (int strand = 0; strand < 2; ++strand)
                rep_off[2 * i + strand + 1] = handled[i] ? rep.off[rep.first[i] + strand + 1] : rep.off[rep.first[i]];
        if (replies && total <= cap && total) memcpy(replies, rep.bytes.data(), total);
        if (needed) *needed = total;
        if ((replies && total <= cap) || total == 0) return RSBWT_OK;
        return rsb::fail(RSBWT_ERANGE, "%zu reply bytes, room for %zu", total, cap);
    } catch (const std::bad_alloc &) {
        return rsb::fail(RSBWT_ENOMEM, "host allocation failed");
    }
}
int rsbwt_service_counts(rsbwt_set_t *set, const uint8_t *requests, size_t requests_len, const uint64_t *req_off,
                         size_t n, uint8_t *replies, size_t cap, uint64_t *rep_off, size_t *needed) {
    return rsb::guarded("rsbwt_service_counts", [&]() -> int { return rsbwt_service_counts_body(set, requests, requests_len, req_off, n, replies, cap, rep_off, needed); });
}


size_t rsbwt_proto_encode_kmer_reply(uint8_t *out, size_t cap, int return_type, const char *q, size_t qlen, int revcomp,
                                     const char *const *reads, const size_t *read_len, size_t nreads) {
    if ((!q && qlen) || ((!reads || !read_len) && nreads) || return_type < 1 || return_type > 4) return 0;
    try {
        std::vector<std::string> own(nreads);
        std::vector<const std::string *> l(nreads);
        for (size_t i = 0; i < nreads; ++i) {
            own[i].assign(reads[i] ? reads[i] : "", read_len[i]);
            l[i] = &own[i];
        }
        std::vector<uint8_t> b;
        rsb::append_kmer_reply(&b, 3, return_type, std::string(q ? q : "", qlen), revcomp != 0, l, nreads);
        if (out && b.size() <= cap) memcpy(out, b.data(), b.size());
        return b.size();
    } catch (const std::bad_alloc &) {
        return 0;
    }
}

size_t rsbwt_proto_encode_all_reply(uint8_t *out, size_t cap, int request_type, int return_type, const char *q, size_t qlen, int revcomp,
                                    const char *const *reads, const size_t *read_len, const uint8_t *const *values, const size_t *value_len,
                                    size_t nreads, const char *hash, size_t hash_len, uint32_t size_of_sample, int has_other_meta_data) {
    if ((!q && qlen) || ((!reads || !read_len) && nreads) || (values && !value_len) || (!hash && hash_len) || request_type < 1 ||
        request_type > 4 || return_type < 1 || return_type > 4 || (size_of_sample == 0 && !has_other_meta_data))
        return 0;
    try {
        std::map<std::string, std::string> h;
        rsb::meta_parse_hash(hash, hash_len, &h);
        rsb::sample_codec c;
        c.hash = &h;
        c.size_of_sample = size_of_sample;
        c.has_other = has_other_meta_data != 0;
        return rsb::meta_encode_all_reply(out, cap, request_type, return_type, q, qlen, revcomp != 0, reads, read_len, values, value_len, nreads, c);
    } catch (const std::bad_alloc &) {
        return 0;
    }
}

int rsbwt_meta_parse_file(const char *path, char *text, size_t text_cap, uint64_t *off, uint8_t *values, size_t values_cap, uint64_t *voff,
                          size_t cap_pairs, size_t *sizes3) {
    return rsb::guarded("rsbwt_meta_parse_file", [&]() -> int {
        if (!path || !sizes3) return rsb::fail(RSBWT_EINVAL, "null argument");
        FILE *f = fopen(path, "rb");
        if (!f) return rsb::fail(RSBWT_EIO, "cannot open %s", path);
        std::string data;
        char buf[1 << 16];
        size_t got;
        while ((got = fread(buf, 1, sizeof buf, f)) > 0) data.append(buf, got);
        const bool bad = ferror(f) != 0;
        fclose(f);
        if (bad) return rsb::fail(RSBWT_EIO, "cannot read %s", path);
        rsb::meta_pairs pairs;
        rsb::meta_parse_pairs(data.data(), data.size(), &pairs);
        const size_t n = pairs.size();
        sizes3[0] = n;
        sizes3[1] = pairs.text.size();
        sizes3[2] = pairs.values.size();
        if (!off || !voff || n > cap_pairs || (!text && sizes3[1]) || sizes3[1] > text_cap || (!values && sizes3[2]) || sizes3[2] > values_cap)
            return rsb::fail(RSBWT_ERANGE, "%zu pairs, %zu read bytes, %zu value bytes", n, sizes3[1], sizes3[2]);
        if (sizes3[1]) memcpy(text, pairs.text.data(), sizes3[1]);
        if (sizes3[2]) memcpy(values, pairs.values.data(), sizes3[2]);
        memcpy(off, pairs.off.data(), (n + 1) * sizeof(uint64_t));
        memcpy(voff, pairs.voff.data(), (n + 1) * sizeof(uint64_t));
        return RSBWT_OK;
    });
}

size_t rsbwt_proto_encode_empty_reply(uint8_t *out, size_t cap, int t, int rt, const char *q, size_t qlen, int revcomp) {
    if ((!q && qlen) || t < 1 || t > 4 || rt < 1 || rt > 4) return 0;
    try {
        std::vector<uint8_t> b;
        rsb::append_kmer_reply(&b, t, rt, std::string(q ? q : "", qlen), revcomp != 0, {}, 0);
        if (out && b.size() <= cap) memcpy(out, b.data(), b.size());
        return b.size();
    } catch (const std::bad_alloc &) {
        return 0;
    }
}

size_t rsbwt_proto_encode_reads_reply(uint8_t *out, size_t cap, int request_type, const char *q, size_t qlen, int revcomp,
                                      const char *const *reads, const size_t *read_len, size_t nreads) {
    if ((!q && qlen) || ((!reads || !read_len) && nreads)) return 0;
    try {
        std::vector<std::string> own(nreads);
        std::vector<const std::string *> l(nreads);
        for (size_t i = 0; i < nreads; ++i) {
            own[i].assign(reads[i] ? reads[i] : "", read_len[i]);
            l[i] = &own[i];
        }
        const std::string qs(q ? q : "", qlen);
        const size_t body = rsb::reads_body_len(l), len = rsb::reads_reply_len(request_type, qlen, body);
        if (out && len <= cap) rsb::encode_reads_reply(out, request_type, qs, revcomp != 0, l, body);
        return len;
    } catch (const std::bad_alloc &) {
        return 0;
    }
}


}  // extern "C"
