// service.h -- the query service's CountReads / ExactMatch-Count slice, host side:
// what service_slice.cpp (codec + batched count_reads) and service_loop.cpp (the recv loop with its
// micro-batch window, the service.cfg reader, the transport interface) share.
#ifndef RSBWT_SERVICE_H
#define RSBWT_SERVICE_H

#include <stddef.h>
#include <stdint.h>

#include <map>
#include <string>
#include <vector>

#include "../../include/rsbwt.h"
#include "meta_file.h"

namespace rsb {

int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));

struct service_request {
    int t = 0, rt = 0;  // Request.RequestType / ReturnType (readserver.proto:4-5)
    std::string q;
    int32_t k = 0, s = 0;  // optional int32 k = 4, s = 5 (readserver.proto:9-10); 0 when absent, as protobuf reads them
    bool has_k = false, has_s = false;
    // SiteMatch: optional int32 p = 6, string a = 7, int32 isalt = 8 (readserver.proto:11-13); 0 / "" when absent
    int32_t p = 0, isalt = 0;
    std::string a;
};

bool service_decode(const uint8_t *msg, size_t len, service_request *out);

// The serialised Reply messages of one batch, back to back: message j is bytes[off[j] .. off[j+1]);
// request i's messages are first[i] .. first[i+1], in sending order (forward, reverse complement; per
// shard first when per_partition).
struct reply_arena {
    std::vector<uint8_t> bytes;
    std::vector<size_t> off, first;
    size_t messages() const { return off.empty() ? 0 : off.size() - 1; }
};
// handled[i] = 0: not a count request, left to the caller (no messages)
int service_count_batch(rsbwt_set_t *set, const std::vector<service_request> &rq, bool per_partition,
                        reply_arena *replies, std::vector<char> *handled);

// find_reads (src/service/service.cpp:714-797) for the ExactMatch requests of a batch whose return type is Reads
// (QueryTask::run, :1260-1291): per request, partition and strand one Reply{rt = ExactMatch, t = ReplyReads, q, r =
// ReplyReads{forward_matches | revcomp_matches}} carrying the reads that partition holds for the query.
struct reads_config {
    size_t min_read_length = 73, max_read_length = 100;  // service.cpp:56-57; service.cfg min_read_length / max_read_length (:1417-1420)
    // service.cfg `max_match_reads` (the reference's front-end has the key, src/service/server.cpp:129,413): a (request,
    // strand) whose query brings more rows than this, summed over the partitions, is answered with no matches at all;
    // 0 = no limit, the path of every release before the key
    uint64_t max_match_reads = 0;
    std::vector<std::string> suffix;                      // service.cfg `suffix` of each shard of the set ("" where absent): a tile is looked
                                                          // up only in the partitions whose suffix it ends with (is_suffix_of, :228-230)
    // rsbwt_service_set_all (service.cfg `meta`): ExactMatch / KmerMatch requests whose return type is All or Samples are
    // answered too -- the reads of the Reads paths, each with its ReadInfo records from the set's sample table
    // (QueryTask::run's default branch, service.cpp:1292-1348; KmerTask::run, :917-975)
    bool serve_all = false;
    bool serve_reads = true;                  // rsbwt_service_set_reads' enable: off = Reads requests are not this batch's
    bool serve_site = false;                  // rsbwt_service_set_sitematch: SiteMatch requests are answered (service_site_batch)
    std::map<std::string, std::string> hash;  // sample code -> name (service.cfg `hashfile`)
    uint32_t size_of_sample = 2;              // service.cfg `size_of_sample` (service.cpp:59,1410-1412)
    bool has_other_meta_data = true;          // service.cfg `has_other_meta_data` (:60,1413-1415)
};
// What the All / Samples paths reach the sample table through (sets.hip fills it in, as query_engine_hooks)
struct meta_engine {
    int (*read_meta_var)(rsbwt_set_t *, const char *, const uint64_t *, size_t, uint64_t *, uint8_t *, size_t, size_t *, uint64_t *);
    uint64_t (*meta_bytes)(const rsbwt_set_t *);
};
extern meta_engine meta_engine_hooks;
inline bool service_is_all_return(const service_request &r) { return r.rt == 3 || r.rt == 4; }  // All, Samples
// capped (optional): capped[i] = 1 when a strand of request i was over cfg.max_match_reads
int service_reads_batch(rsbwt_set_t *set, const std::vector<service_request> &rq, bool per_partition, const reads_config &cfg,
                        reply_arena *replies, std::vector<char> *handled, std::vector<char> *capped = nullptr);
// What service_reads_batch reaches rsbwt_set_query_var_capped through (sets.hip fills it in when the engine is linked; the
// host harnesses under tests/native link this file against stub engines that know rsbwt_set_query_var only): null with
// a limit set = RSBWT_ENODEV.
struct query_engine {
    int (*query_var_capped)(rsbwt_set_t *, const char *, const uint64_t *, size_t, uint64_t, uint64_t *, uint32_t *, char *, uint32_t, uint32_t *,
                            size_t, size_t *, uint64_t *);
};
extern query_engine query_engine_hooks;
// the same requests answered with EMPTY read lists (a failed batch: the front-end has no timeout, server.cpp:469)
// (cfg given: the requests service_reads_batch takes under it -- All / Samples ones get an empty ReplyAll)
void service_reads_empty(const std::vector<service_request> &rq, size_t rows, reply_arena *replies, std::vector<char> *handled,
                         const reads_config *cfg = nullptr);
inline bool service_is_reads_request(const service_request &r) { return r.t == 2 && r.rt == 2; }  // ExactMatch + Reads
// the requests service_reads_batch answers under cfg: ExactMatch + Reads, and + All / Samples when cfg.serve_all
inline bool service_takes_reads(const service_request &r, const reads_config &cfg) {
    return r.t == 2 && ((cfg.serve_reads && r.rt == 2) || (cfg.serve_all && service_is_all_return(r)));
}

// KmerMatch with return type Count or Reads (KmerTask::run, service.cpp:871-960 around find_kmer_reads :466-502): per
// request, partition (or once, summed) and strand one Reply{rt = KmerMatch, t = (ReplyType) rt, q, c | r}.
inline bool service_is_kmer_request(const service_request &r) { return r.t == 3 && (r.rt == 1 || r.rt == 2); }
inline bool service_takes_kmer(const service_request &r, const reads_config &cfg) {
    return service_is_kmer_request(r) || (cfg.serve_all && r.t == 3 && service_is_all_return(r));
}
int service_kmer_batch(rsbwt_set_t *set, const std::vector<service_request> &rq, bool per_partition, const reads_config &cfg,
                       reply_arena *replies, std::vector<char> *handled);
// appends the 2 x rows Replies (per row: forward, reverse complement) a reference service sends for request r when it
// finds nothing: KmerTask / QueryTask / GtTask with an empty result (service.cpp:871-960, 1260-1360, 1023-1170)
void service_append_empty(const service_request &r, size_t rows, reply_arena *replies);

// SiteMatch (GtTask::run, service.cpp:1014-1210): per request, partition (or once, joined) and strand one Reply{rt =
// SiteMatch, t = (ReplyType) rt, q, c | r | a} with the reads align_gt_read keeps, from rsbwt_set_site_reads /
// rsbwt_set_site_read_counts -- one call per distinct (k, s) of the batch, both strands of every request as its items.
// The reads of a Reply come in ascending read_row per partition, not in the reference's unordered_set order.  Count and
// Reads are taken when cfg.serve_site, All / Samples when cfg.serve_all too.
inline bool service_takes_site(const service_request &r, const reads_config &cfg) {
    return cfg.serve_site && r.t == 4 && (r.rt == 1 || r.rt == 2 || (cfg.serve_all && service_is_all_return(r)));
}
// The window fix-up of one strand (service.cpp:1028-1046) with L = max_read_length, in signed arithmetic: false = the Reply
// carries rt, t and q and no sub-message (pos > |w|, the reference's "ERROR" line; and where the reference is undefined:
// pos < 0, or a substr start past the end).  alt: the (reverse-complemented) a, whole.
bool service_site_fixup(const std::string &q, int64_t p, const std::string &a, bool revcomp, size_t L, std::string *w, int64_t *pos, std::string *alt);
// What service_site_batch reaches the engine through (sets.hip fills it in; the host harnesses link a stub): the
// signatures of rsbwt_set_site_reads / rsbwt_set_site_read_counts
struct site_engine {
    int (*reads)(rsbwt_set_t *, const char *, const uint64_t *, size_t, const uint64_t *, const char *, const uint8_t *, int32_t, int32_t, uint64_t, uint64_t *,
                 char *, uint32_t, uint32_t *, uint64_t *, size_t, size_t *);
    int (*counts)(rsbwt_set_t *, const char *, const uint64_t *, size_t, const uint64_t *, const char *, const uint8_t *, int32_t, int32_t, uint64_t,
                  uint64_t *);
};
extern site_engine site_engine_hooks;
int service_site_batch(rsbwt_set_t *set, const std::vector<service_request> &rq, bool per_partition, const reads_config &cfg, reply_arena *replies,
                       std::vector<char> *handled);
// the same requests answered with zero counts / empty lists (a failed batch); header-only where the fix-up says so
void service_site_empty(const std::vector<service_request> &rq, size_t rows, const reads_config &cfg, reply_arena *replies, std::vector<char> *handled);

// What the loop needs of ZeroMQ: the SUB socket it receives Requests on (service.cpp:1495-1497) and
// the two PUSH sockets it answers on (push for ExactMatch, push_count for CountReads: :1499-1502,1568).
class transport {
  public:
    virtual ~transport() {}
    // next Request message; waits at most timeout_us (< 0: until one arrives or the transport
    // closes).  false = nothing arrived in time, or closed.
    virtual bool recv(std::vector<uint8_t> *msg, int64_t timeout_us) = 0;
    // up to `max` messages appended to *out: waits at most timeout_us for the first, takes whatever else is queued
    // already; the number taken (0: nothing arrived in time, or closed)
    virtual size_t recv_many(std::vector<std::vector<uint8_t>> *out, size_t max, int64_t timeout_us) {
        std::vector<uint8_t> m;
        if (max == 0 || !recv(&m, timeout_us)) return 0;
        out->push_back(std::move(m));
        return 1;
    }
    virtual bool closed() = 0;   // closed AND nothing left to receive
    virtual bool closing() = 0;  // close was asked for: what is queued is still answered
    enum channel { PUSH = 0, PUSH_COUNT = 1 };
    virtual void send(channel c, const uint8_t *data, size_t n) = 0;
    // messages [off[0], off[1]), ..., [off[count-1], off[count]) of `base`, in order
    virtual void send_many(channel c, const uint8_t *base, const size_t *off, size_t count) {
        for (size_t j = 0; j < count; ++j) send(c, base + off[j], off[j + 1] - off[j]);
    }
};

}  // namespace rsb
#endif
