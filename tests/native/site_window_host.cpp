// site_window_host.cpp -- the SiteMatch window fix-up and Reply code of csrc/service_slice.cpp without the engine (CPU only;
// built with -fsanitize=address,undefined and run by tests/test_site_window_host.py).  service_slice.cpp reaches
// rsbwt_set_site_reads / rsbwt_set_site_read_counts through rsb::site_engine_hooks and the sample table through
// rsb::meta_engine_hooks (csrc/service.h); here both are stubs that return canned answers made from their arguments:
//   cell (item j, partition p) holds (j + p) % 3 reads; read r of it is the item's window, its alt character, then r + 1
//   times the letter 'A' + p; the value of a read of odd length is "ab!#cd$%", of even length empty.
//   site_window_host fixup L          one line per (|q|, p, strand) for |q| <= 2L + 3 and -3 <= p <= |q| + L + 2: what
//                                     service_site_fixup answers for q = the first |q| symbols of SEQ and a = "AG"
//   site_window_host replies L MODE   MODE 1 = per partition, 0 = joined: the requests of requests() through
//                                     service_site_batch; one line of hex per Reply message, then "calls <reads> <counts>"
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "rsbwt.h"
#include "service.h"

namespace rsb {
int fail(int code, const char *, ...) { return code; }
}  // namespace rsb
static const size_t PARTS = 3;
static size_t reads_calls = 0, counts_calls = 0;
extern "C" {
size_t rsbwt_set_size(const rsbwt_set_t *) { return PARTS; }
int rsbwt_set_find_intervals(rsbwt_set_t *, const char *, size_t, uint32_t, size_t, uint64_t *, uint64_t *) { return RSBWT_EINVAL; }
int rsbwt_set_count(rsbwt_set_t *, const char *, size_t, uint32_t, size_t, uint64_t *) { return RSBWT_EINVAL; }
int rsbwt_set_find_intervals_var(rsbwt_set_t *, const char *, const uint64_t *, size_t, uint64_t *, uint64_t *) { return RSBWT_EINVAL; }
int rsbwt_set_count_var(rsbwt_set_t *, const char *, const uint64_t *, size_t, uint64_t *) { return RSBWT_EINVAL; }
const char *rsbwt_last_error(void) { return ""; }
rsbwt_t *rsbwt_set_shard(rsbwt_set_t *, size_t i) { return (rsbwt_t *)(uintptr_t)(i + 1); }
int rsbwt_query_exactmatch(rsbwt_t *, const char *, size_t, uint32_t, size_t, uint8_t *) { return RSBWT_EINVAL; }
int rsbwt_set_query(rsbwt_set_t *, const char *, size_t, uint32_t, size_t, uint64_t *, uint32_t *, char *, uint32_t, uint32_t *, size_t, size_t *) {
    return RSBWT_EINVAL;
}
int rsbwt_set_query_var(rsbwt_set_t *, const char *, const uint64_t *, size_t, uint64_t *, uint32_t *, char *, uint32_t, uint32_t *, size_t, size_t *) {
    return RSBWT_EINVAL;
}
}

static std::string canned(const char *text, const uint64_t *off, size_t j, char alt, size_t p, size_t r) {
    return std::string(text + off[j], (size_t)(off[j + 1] - off[j])) + alt + std::string(r + 1, (char)('A' + p));
}
static int stub_reads(rsbwt_set_t *, const char *text, const uint64_t *off, size_t Q, const uint64_t *, const char *alt, const uint8_t *, int32_t, int32_t,
                      uint64_t, uint64_t *first, char *reads, uint32_t stride, uint32_t *read_len, uint64_t *read_row, size_t cap, size_t *nreads) {
    ++reads_calls;
    size_t total = 0;
    for (size_t j = 0; j < Q; ++j)
        for (size_t p = 0; p < PARTS; ++p) {
            first[j * PARTS + p] = total;
            total += (j + p) % 3;
        }
    first[Q * PARTS] = total;
    *nreads = total;
    if (total > cap) return RSBWT_ERANGE;
    size_t at = 0;
    for (size_t j = 0; j < Q; ++j)
        for (size_t p = 0; p < PARTS; ++p)
            for (size_t r = 0; r < (j + p) % 3; ++r, ++at) {
                const std::string s = canned(text, off, j, alt[j], p, r);
                if (s.size() > stride) {
                    read_len[at] = 0xFFFFFFFFu;
                } else {
                    memcpy(reads + at * (size_t)stride, s.data(), s.size());
                    read_len[at] = (uint32_t)s.size();
                }
                if (read_row) read_row[at] = at;
            }
    return RSBWT_OK;
}
static int stub_counts(rsbwt_set_t *, const char *, const uint64_t *, size_t Q, const uint64_t *, const char *, const uint8_t *, int32_t, int32_t, uint64_t,
                       uint64_t *counts) {
    ++counts_calls;
    for (size_t j = 0; j < Q; ++j)
        for (size_t p = 0; p < PARTS; ++p) counts[j * PARTS + p] = (j + p) % 3;
    return RSBWT_OK;
}
static int stub_meta(rsbwt_set_t *, const char *, const uint64_t *off, size_t Q, uint64_t *first, uint8_t *bytes, size_t cap, size_t *need, uint64_t *) {
    size_t total = 0;
    for (size_t x = 0; x < Q * PARTS; ++x) {
        first[x] = total;
        if ((off[x / PARTS + 1] - off[x / PARTS]) % 2) total += 8;
    }
    first[Q * PARTS] = total;
    if (need) *need = total;
    if (total > cap) return RSBWT_ERANGE;
    for (size_t x = 0; x < Q * PARTS; ++x)
        if (first[x + 1] != first[x]) memcpy(bytes + first[x], "ab!#cd$%", 8);
    return RSBWT_OK;
}

static const char SEQ[] = "ACGTTGCAAGCTCAGGTACCATG";

static std::vector<rsb::service_request> requests(size_t L) {
    std::vector<rsb::service_request> rq;
    const std::string q(SEQ, 2 * L + 3);
    auto add = [&](int t, int rt, const std::string &s, int32_t k, int32_t sk, int32_t p, const char *a, int32_t isalt) {
        rsb::service_request r;
        r.t = t;
        r.rt = rt;
        r.q = s;
        r.k = k;
        r.s = sk;
        r.p = p;
        r.a = a;
        r.isalt = isalt;
        rq.push_back(r);
    };
    for (int rt = 1; rt <= 4; ++rt) {
        add(4, rt, q, 3, 0, (int32_t)L + 2, "G", 0);   // both strands past L
        add(4, rt, q, 3, 0, 2, "GT", 1);                // forward: the first branch
        add(4, rt, q, 4, 1, (int32_t)q.size() + 1, "C", 0);  // p > |q|: forward without sub-message
        add(4, rt, q, 4, 1, 3, "", 0);                  // an empty a: keeps nothing
        add(4, rt, q.substr(0, 3), 3, 0, 4, "T", 2);    // pos > |w| forward; isalt = 2 is not 1
    }
    add(2, 2, q, 0, 0, 0, "", 0);  // (ExactMatch + Reads: not this batch's)
    add(4, 1, q, 9, 9, 1, "A", 0);   // a (k, s) of its own whose requests all ask for Count: the counts call
    return rq;
}

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    const size_t L = (size_t)atoi(argv[2]);
    if (L == 0 || 2 * L + 3 >= sizeof SEQ) return 2;
    if (strcmp(argv[1], "fixup") == 0) {
        for (size_t n = 0; n <= 2 * L + 3; ++n)
            for (int64_t p = -3; p <= (int64_t)(n + L) + 2; ++p)
                for (int strand = 0; strand < 2; ++strand) {
                    std::string w, alt;
                    int64_t pos = 0;
                    const bool ok = rsb::service_site_fixup(std::string(SEQ, n), p, "AG", strand == 1, L, &w, &pos, &alt);
                    if (ok) printf("%zu %lld %d ok %s %lld %s\n", n, (long long)p, strand, w.c_str(), (long long)pos, alt.c_str());
                    else printf("%zu %lld %d header\n", n, (long long)p, strand);
                }
        return 0;
    }
    if (strcmp(argv[1], "replies") != 0 || argc < 4) return 2;
    const bool per_partition = atoi(argv[3]) != 0;
    rsbwt_set_t *set = (rsbwt_set_t *)0x1;
    rsb::reads_config cfg;
    cfg.min_read_length = 1;
    cfg.max_read_length = L;
    cfg.serve_site = true;
    cfg.serve_all = true;
    const std::vector<rsb::service_request> rq = requests(L);
    rsb::reply_arena rep;
    std::vector<char> handled;
    // no engine behind the hook: refused
    if (rsb::service_site_batch(set, rq, per_partition, cfg, &rep, &handled) != RSBWT_ENODEV) return 3;
    rsb::site_engine_hooks.reads = stub_reads;
    rsb::site_engine_hooks.counts = stub_counts;
    rsb::meta_engine_hooks.read_meta_var = stub_meta;
    if (rsb::service_site_batch(set, rq, per_partition, cfg, &rep, &handled) != RSBWT_OK) return 4;
    const size_t rows = per_partition ? PARTS : 1;
    for (size_t i = 0; i < rq.size(); ++i) {
        const size_t want = rq[i].t == 4 ? 2 * rows : 0;
        if ((handled[i] != 0) != (rq[i].t == 4) || rep.first[i + 1] - rep.first[i] != want) return 5;
        for (size_t j = rep.first[i]; j < rep.first[i + 1]; ++j) {
            for (size_t b = rep.off[j]; b < rep.off[j + 1]; ++b) printf("%02x", rep.bytes[b]);
            printf("\n");
        }
    }
    printf("calls %zu %zu\n", reads_calls, counts_calls);
    // All / Samples without serve_all, and everything with serve_site off: not this batch's
    cfg.serve_all = false;
    if (rsb::service_site_batch(set, rq, per_partition, cfg, &rep, &handled) != RSBWT_OK) return 6;
    for (size_t i = 0; i < rq.size(); ++i)
        if ((handled[i] != 0) != (rq[i].t == 4 && rq[i].rt <= 2)) return 7;
    cfg.serve_site = false;
    if (rsb::service_site_batch(set, rq, per_partition, cfg, &rep, &handled) != RSBWT_OK || rep.messages() != 0) return 8;
    return 0;
}
