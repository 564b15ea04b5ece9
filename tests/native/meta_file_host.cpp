// meta_file_host.cpp -- the host side of the sample table (readserver_amd/csrc/meta_file.h: the pairs-file parser, the hash
// file parser, the ReplyAll encoder) built for the CPU with -fsanitize=address,undefined by tests/test_meta_reference.py and
// run as a program of its own:
//
//     meta_file_host <pairs file> <hash file> <rounds>
//
//   1. the two files are parsed and one Reply holding every pair is encoded at the record sizes (1, no meta), (2, meta) and
//      (3, meta), forward and reverse complement, into a heap buffer of EXACTLY the size the sizing call named (one byte
//      more written = a report); "pairs ..." and one "reply ..." line per case carry the counts and an FNV-1a of the bytes,
//      which the test compares with what the library gives for the same files;
//   2. `rounds` mutations of the pairs file (bytes flipped, newlines inserted and removed, cut anywhere) go through the same
//      code: the offsets stay ascending and inside the text, every value's records decode inside the value.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <random>
#include <string>
#include <vector>

#include "../../readserver_amd/csrc/meta_file.h"

#define CHECK(x)                                                    \
    do {                                                            \
        if (!(x)) {                                                 \
            fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); \
            return 1;                                               \
        }                                                           \
    } while (0)

static std::string slurp(const char *path) {
    std::string s;
    FILE *f = fopen(path, "rb");
    if (!f) return s;
    char buf[1 << 14];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, f)) > 0) s.append(buf, got);
    fclose(f);
    return s;
}

static uint64_t fnv(const uint8_t *p, size_t n) {
    uint64_t h = 1469598103934665603ull;
    for (size_t i = 0; i < n; ++i) h = (h ^ p[i]) * 1099511628211ull;
    return h;
}

// every pair of `pairs` in one Reply; the bytes into a buffer of exactly the size asked for
static int encode_case(const rsb::meta_pairs &pairs, const std::map<std::string, std::string> &hash, uint32_t ss, bool other, bool revcomp,
                       uint64_t *digest, size_t *len) {
    const size_t n = pairs.size();
    std::vector<const char *> rp(n);
    std::vector<size_t> rl(n), vl(n);
    std::vector<const uint8_t *> vp(n);
    for (size_t i = 0; i < n; ++i) {
        rp[i] = pairs.text.data() + pairs.off[i];
        rl[i] = (size_t)(pairs.off[i + 1] - pairs.off[i]);
        vp[i] = (const uint8_t *)pairs.values.data() + pairs.voff[i];
        vl[i] = (size_t)(pairs.voff[i + 1] - pairs.voff[i]);
    }
    rsb::sample_codec c;
    c.hash = &hash;
    c.size_of_sample = ss;
    c.has_other = other;
    const char q[] = "ACGTNACGT";
    const size_t need = rsb::meta_encode_all_reply(nullptr, 0, 2, revcomp ? 4 : 3, q, sizeof q - 1, revcomp, rp.data(), rl.data(), vp.data(),
                                                   vl.data(), n, c);
    CHECK(need > 0);
    std::unique_ptr<uint8_t[]> buf(new uint8_t[need]);
    CHECK(rsb::meta_encode_all_reply(buf.get(), need, 2, revcomp ? 4 : 3, q, sizeof q - 1, revcomp, rp.data(), rl.data(), vp.data(), vl.data(), n,
                                     c) == need);
    if (need > 1) {  // a buffer one byte short: the size comes back, nothing is written
        std::unique_ptr<uint8_t[]> small(new uint8_t[need - 1]);
        CHECK(rsb::meta_encode_all_reply(small.get(), need - 1, 2, 3, q, sizeof q - 1, revcomp, rp.data(), rl.data(), vp.data(), vl.data(), n, c) == need);
    }
    // each read's records by themselves: the size the sizing pass names is the size written
    for (size_t i = 0; i < n; ++i) {
        const size_t s = rsb::meta_encode_samples(nullptr, c, vp[i], vl[i]);
        std::unique_ptr<uint8_t[]> one(new uint8_t[s ? s : 1]);
        CHECK(rsb::meta_encode_samples(one.get(), c, vp[i], vl[i]) == s);
    }
    *digest = fnv(buf.get(), need);
    *len = need;
    return 0;
}

static int check_pairs(const rsb::meta_pairs &p, size_t data_len) {
    CHECK(p.off.size() == p.voff.size() && !p.off.empty() && p.off[0] == 0 && p.voff[0] == 0);
    for (size_t i = 0; i + 1 < p.off.size(); ++i) CHECK(p.off[i] <= p.off[i + 1] && p.voff[i] <= p.voff[i + 1]);
    CHECK(p.off.back() == p.text.size() && p.voff.back() == p.values.size());
    CHECK(p.text.size() + p.values.size() <= data_len);
    CHECK(p.text.find('\n') == std::string::npos && p.values.find('\n') == std::string::npos);
    return 0;
}

int main(int argc, char **argv) {
    if (argc < 4) {
        fprintf(stderr, "usage: %s <pairs file> <hash file> <rounds>\n", argv[0]);
        return 2;
    }
    const std::string data = slurp(argv[1]), hdata = slurp(argv[2]);
    const int rounds = atoi(argv[3]);
    rsb::meta_pairs pairs;
    rsb::meta_parse_pairs(data.data(), data.size(), &pairs);
    if (check_pairs(pairs, data.size())) return 1;
    std::map<std::string, std::string> hash;
    rsb::meta_parse_hash(hdata.data(), hdata.size(), &hash);
    printf("pairs %zu %zu %zu hash %zu\n", pairs.size(), pairs.text.size(), pairs.values.size(), hash.size());
    const struct { uint32_t ss; bool other; } cases[] = {{1, false}, {2, true}, {3, true}};
    for (const auto &cs : cases)
        for (int revcomp = 0; revcomp < 2; ++revcomp) {
            uint64_t d = 0;
            size_t len = 0;
            if (encode_case(pairs, hash, cs.ss, cs.other, revcomp != 0, &d, &len)) return 1;
            printf("reply %u %d %d %zu %016llx\n", cs.ss, cs.other ? 1 : 0, revcomp, len, (unsigned long long)d);
        }
    // the empty inputs
    rsb::meta_pairs none;
    rsb::meta_parse_pairs(nullptr, 0, &none);
    CHECK(none.size() == 0);
    rsb::meta_parse_pairs("ACGT", 4, &none);  // a read without a value line
    CHECK(none.size() == 0);
    rsb::meta_parse_pairs("ACGT\n", 5, &none);
    CHECK(none.size() == 0);
    rsb::meta_parse_pairs("ACGT\n\n", 6, &none);  // an empty value line
    CHECK(none.size() == 1 && none.off[1] == 4 && none.voff[1] == 0);
    rsb::meta_parse_pairs("ACGT\r\nab\r\nTT\nxyz", 16, &none);  // CRLF is not special; a last line without a newline is a line
    CHECK(none.size() == 2 && none.text == "ACGT\rTT" && none.values == "ab\rxyz");
    // mutations
    std::mt19937_64 rng(20261019);
    for (int r = 0; r < rounds; ++r) {
        std::string m = data;
        const int edits = 1 + (int)(rng() % 8);
        for (int e = 0; e < edits && !m.empty(); ++e) {
            const size_t at = rng() % m.size();
            switch (rng() % 4) {
                case 0: m[at] = (char)(rng() & 0xFF); break;
                case 1: m.insert(at, 1, '\n'); break;
                case 2: m.erase(at, 1 + rng() % 3); break;
                default: m.resize(at); break;
            }
        }
        // (an exact-size heap copy: a read past the end of the data is a report)
        std::unique_ptr<char[]> exact(new char[m.size() ? m.size() : 1]);
        if (!m.empty()) memcpy(exact.get(), m.data(), m.size());
        rsb::meta_pairs mp;
        rsb::meta_parse_pairs(exact.get(), m.size(), &mp);
        if (check_pairs(mp, m.size())) return 1;
        std::map<std::string, std::string> mh;
        rsb::meta_parse_hash(exact.get(), m.size(), &mh);
        uint64_t d;
        size_t len;
        if (encode_case(mp, r % 2 ? mh : hash, 1 + (uint32_t)(r % 4), r % 3 != 0, r % 2 != 0, &d, &len)) return 1;
    }
    printf("meta_file ok: %d mutations\n", rounds);
    return 0;
}
