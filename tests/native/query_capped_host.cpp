// query_capped_host.cpp -- the service's max_match_reads without the engine (CPU only; built and run by
// tests/test_query_capped_host.py).  service_slice.cpp reaches rsbwt_set_query_var_capped through
// rsb::query_engine_hooks (csrc/service.h), which only the engine fills in:
//   1. hook null: a limit is refused with RSBWT_ENODEV, by the setter and by service_reads_batch; 0 = no limit is taken;
//   2. hook set to a stub that finds 3 reads per query and partition, 10^9 rows for a query of one symbol: through the
//      loop, a Reads request whose strands are both over the limit gets 2 x partitions Replies equal to
//      rsbwt_proto_encode_empty_reply, its neighbours get their reads, rsbwt_service_capped_requests counts it.
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
static const size_t PARTS = 2;
static size_t plain_calls = 0, capped_calls = 0;
extern "C" {
size_t rsbwt_set_size(const rsbwt_set_t *) { return PARTS; }
int rsbwt_set_find_intervals(rsbwt_set_t *, const char *, size_t Q, uint32_t, size_t, uint64_t *lo, uint64_t *up) {
    for (size_t i = 0; i < PARTS * Q; ++i) { lo[i] = 1; up[i] = 0; }
    return RSBWT_OK;
}
int rsbwt_set_count(rsbwt_set_t *, const char *, size_t Q, uint32_t, size_t, uint64_t *c) {
    for (size_t i = 0; i < Q; ++i) c[i] = 0;
    return RSBWT_OK;
}
int rsbwt_set_find_intervals_var(rsbwt_set_t *, const char *, const uint64_t *, size_t Q, uint64_t *lo, uint64_t *up) {
    for (size_t i = 0; i < PARTS * Q; ++i) { lo[i] = 1; up[i] = 0; }
    return RSBWT_OK;
}
int rsbwt_set_count_var(rsbwt_set_t *, const char *, const uint64_t *, size_t Q, uint64_t *c) {
    for (size_t i = 0; i < Q; ++i) c[i] = 0;
    return RSBWT_OK;
}
const char *rsbwt_last_error(void) { return ""; }
rsbwt_t *rsbwt_set_shard(rsbwt_set_t *, size_t i) { return (rsbwt_t *)(uintptr_t)(i + 1); }
int rsbwt_query_exactmatch(rsbwt_t *, const char *, size_t Q, uint32_t, size_t, uint8_t *found) {
    for (size_t q = 0; q < Q; ++q) found[q] = 0;
    return RSBWT_OK;
}
int rsbwt_set_query(rsbwt_set_t *, const char *, size_t, uint32_t, size_t, uint64_t *, uint32_t *, char *, uint32_t, uint32_t *, size_t, size_t *) {
    return RSBWT_EINVAL;
}
int rsbwt_set_query_var(rsbwt_set_t *, const char *, const uint64_t *, size_t Q, uint64_t *first, uint32_t *, char *, uint32_t, uint32_t *, size_t,
                        size_t *nreads) {
    ++plain_calls;
    for (size_t q = 0; q <= Q; ++q) first[q] = 0;
    *nreads = 0;
    return RSBWT_OK;
}
}
// the stub engine's capped query: "ACGTAC" three times per partition; a query of one symbol has 10^9 rows
static int stub_capped(rsbwt_set_t *, const char *, const uint64_t *off, size_t Q, uint64_t max_rows, uint64_t *first, uint32_t *read_shard,
                       char *reads, uint32_t read_stride, uint32_t *read_len, size_t cap_reads, size_t *nreads, uint64_t *matches) {
    ++capped_calls;
    size_t total = 0;
    for (size_t q = 0; q < Q; ++q) {
        const uint64_t m = off[q + 1] - off[q] == 1 ? 1000000000ull : 3 * PARTS;
        if (matches) matches[q] = m;
        first[q] = total;
        if (!(max_rows && m > max_rows)) total += (size_t)m;
    }
    first[Q] = total;
    *nreads = total;
    if (total > cap_reads) return RSBWT_ERANGE;
    for (size_t r = 0; r < total; ++r) {
        memcpy(reads + r * (size_t)read_stride, "ACGTAC", 6);
        read_len[r] = 6;
        if (read_shard) read_shard[r] = (uint32_t)((r / 3) % PARTS);
    }
    return RSBWT_OK;
}

#define CHECK(x)                                                   \
    do {                                                           \
        if (!(x)) {                                                \
            fprintf(stderr, "line %d: %s\n", __LINE__, #x);        \
            return 1;                                              \
        }                                                          \
    } while (0)

static std::string reads_request(const std::string &q) {
    std::string m("\x08\x02\x10\x02\x1A", 5);
    m.push_back((char)q.size());
    return m + q;
}

int main() {
    rsbwt_set_t *set = (rsbwt_set_t *)0x1;
    rsbwt_transport_t *tr = nullptr;
    rsbwt_service_t *svc = nullptr;
    CHECK(rsbwt_transport_inproc(&tr) == RSBWT_OK && rsbwt_service_create(set, tr, 2000, 64, 1, &svc) == RSBWT_OK);
    // 1. no engine
    CHECK(rsb::query_engine_hooks.query_var_capped == nullptr);
    CHECK(rsbwt_service_set_max_match_reads(nullptr, 0) == RSBWT_EINVAL);
    CHECK(rsbwt_service_set_max_match_reads(svc, 0) == RSBWT_OK);
    CHECK(rsbwt_service_set_max_match_reads(svc, 100000) == RSBWT_ENODEV);
    CHECK(rsbwt_service_capped_requests(svc) == 0 && rsbwt_service_capped_requests(nullptr) == 0);
    {
        std::vector<rsb::service_request> rq(1);
        rq[0].t = 2; rq[0].rt = 2; rq[0].q = "ACGTA";
        rsb::reads_config cfg;
        rsb::reply_arena rep;
        std::vector<char> handled, capped;
        CHECK(rsb::service_reads_batch(set, rq, true, cfg, &rep, &handled, &capped) == RSBWT_OK);  // no limit: the plain entry point
        CHECK(plain_calls == 1 && rep.messages() == 2 * PARTS && capped.size() == 1 && !capped[0]);
        cfg.max_match_reads = 5;
        CHECK(rsb::service_reads_batch(set, rq, true, cfg, &rep, &handled, &capped) == RSBWT_ENODEV);
        CHECK(plain_calls == 1);
    }
    // 2. a stub engine behind the hook
    rsb::query_engine_hooks.query_var_capped = stub_capped;
    CHECK(rsbwt_service_set_max_match_reads(svc, 100) == RSBWT_OK);
    rsbwt_service_set_reads(svc, 1, 50, 70);
    CHECK(rsbwt_service_start(svc) == RSBWT_OK);
    const std::vector<std::string> qs = {"ACGTA", "A", "GGCAT", "C", "TTGCA"};
    for (const std::string &q : qs) {
        const std::string m = reads_request(q);
        CHECK(rsbwt_transport_push_request(tr, (const uint8_t *)m.data(), m.size()) == RSBWT_OK);
    }
    uint8_t buf[512], want[512];
    for (const std::string &q : qs)
        for (size_t p = 0; p < PARTS; ++p)
            for (int strand = 0; strand < 2; ++strand) {
                size_t n = 0;
                CHECK(rsbwt_transport_pop_reply(tr, 0, buf, sizeof buf, &n, 30000000) == RSBWT_OK);
                size_t nw;
                if (q.size() == 1) {
                    nw = rsbwt_proto_encode_empty_reply(want, sizeof want, 2, 2, q.data(), q.size(), strand);
                } else {
                    const char *r3[3] = {"ACGTAC", "ACGTAC", "ACGTAC"};
                    const size_t l3[3] = {6, 6, 6};
                    nw = rsbwt_proto_encode_reads_reply(want, sizeof want, 2, q.data(), q.size(), strand, r3, l3, 3);
                }
                CHECK(nw != 0 && nw == n && memcmp(buf, want, n) == 0);
            }
    rsbwt_transport_close(tr);
    CHECK(rsbwt_service_stop(svc) == RSBWT_OK);
    CHECK(rsbwt_service_capped_requests(svc) == 2 && rsbwt_service_read_requests(svc) == qs.size());
    CHECK(capped_calls >= 1 && plain_calls == 1);
    rsbwt_service_free(svc);
    rsbwt_transport_free(tr);
    printf("ok: %zu capped calls\n", capped_calls);
    return 0;
}
