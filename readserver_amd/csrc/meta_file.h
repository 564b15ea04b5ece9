// meta_file.h -- the host side of the per-read sample table (rsbwt_set_meta_*): the pairs file the reference loads into
// RocksDB, the hash file that names the sample codes, and the ReplyAll encoder.  Host only (no HIP): what
// tests/native/meta_file_host.cpp runs under the sanitizers.  Header only: service_slice.cpp, which the host harnesses
// link without the engine, encodes with it.
#ifndef RSBWT_META_FILE_H
#define RSBWT_META_FILE_H

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <map>
#include <string>
#include <vector>

namespace rsb {

// The file load_data_into_rocksdb reads (src/util/load_data_into_rocksdb.cpp:44): line 1 a read, line 2 its value up to
// the newline, repeated -- `getline(read) && getline(value)`, so a last read without a value line is dropped, an empty
// value line is an empty value, and a '\r' is a byte like any other.  Pair i = text[off[i] .. off[i+1]) with
// values[voff[i] .. voff[i+1]).
struct meta_pairs {
    std::string text, values;
    std::vector<uint64_t> off{0}, voff{0};
    size_t size() const { return off.size() - 1; }
};

// One read's records: value -> ReadInfo{g, c, l}* as service.cpp:1332-1347 spells them.  record = size_of_sample (+ 2
// with has_other); a tail shorter than a record is cut (the reference reads past the string there).
struct sample_codec {
    const std::map<std::string, std::string> *hash = nullptr;  // nullptr: every g is ""
    uint32_t size_of_sample = 2;                                // service.cpp:59
    bool has_other = true;                                      // service.cpp:60
};

namespace meta_detail {

// std::getline over a buffer: false at the end of the data (nothing extracted); a last line without '\n' is a line
inline bool next_line(const char *data, size_t len, size_t *pos, size_t *b, size_t *e) {
    if (*pos >= len) return false;
    const void *nl = memchr(data + *pos, '\n', len - *pos);
    *b = *pos;
    *e = nl ? (size_t)((const char *)nl - data) : len;
    *pos = nl ? *e + 1 : len;
    return true;
}

inline size_t varint_len(uint64_t v) {
    size_t n = 1;
    while (v >= 0x80) {
        v >>= 7;
        ++n;
    }
    return n;
}
inline uint8_t *put_varint(uint8_t *p, uint64_t v) {
    while (v >= 0x80) {
        *p++ = (uint8_t)(v | 0x80);
        v >>= 7;
    }
    *p++ = (uint8_t)v;
    return p;
}
// an int32 field on the wire: sign-extended to 64 bits (a negative value is ten bytes)
inline uint64_t wire_int32(int32_t v) { return (uint64_t)(int64_t)v; }

// walks the whole records of a value; fn(g, c, l)
template <class F>
void for_each_record(const sample_codec &c, const uint8_t *value, size_t vlen, F &&fn) {
    static const std::string none;
    const size_t ss = c.size_of_sample, rec = ss + (c.has_other ? 2 : 0);
    if (rec == 0) return;  // (size_of_sample = 0 without meta data: the reference's loop would not end)
    std::string key;
    for (size_t pos = 0; pos + rec <= vlen; pos += rec) {
        const std::string *g = &none;
        if (c.hash) {
            key.assign((const char *)value + pos, ss);
            const auto it = c.hash->find(key);
            if (it != c.hash->end()) g = &it->second;  // (operator[] of a missing code: "")
        }
        int32_t cc = 0, ll = 0;
        if (c.has_other) {
            cc = (int32_t)(signed char)value[pos + ss] - 33;  // (int)(value[pos]) - 33 on a std::string: char is signed
            ll = (int32_t)(signed char)value[pos + ss + 1] - 33;
        }
        fn(*g, cc, ll);
    }
}

}  // namespace meta_detail

inline void meta_parse_pairs(const char *data, size_t len, meta_pairs *out) {
    using namespace meta_detail;
    out->text.clear();
    out->values.clear();
    out->off.assign(1, 0);
    out->voff.assign(1, 0);
    size_t pos = 0, rb, re, vb, ve;
    while (next_line(data, len, &pos, &rb, &re) && next_line(data, len, &pos, &vb, &ve)) {
        out->text.append(data + rb, re - rb);
        out->values.append(data + vb, ve - vb);
        out->off.push_back(out->text.size());
        out->voff.push_back(out->values.size());
    }
}

// The hash file (src/service/service.cpp:1477-1488): lines of `name \t code`; code -> name, the first line of a code
// wins (std::map::insert); empty lines and lines without a tab are skipped.
inline void meta_parse_hash(const char *data, size_t len, std::map<std::string, std::string> *out) {
    using namespace meta_detail;
    out->clear();
    size_t pos = 0, b, e;
    while (next_line(data, len, &pos, &b, &e)) {
        if (e == b) continue;
        const void *tab = memchr(data + b, '\t', e - b);
        if (!tab) continue;
        const size_t t = (size_t)((const char *)tab - data);
        out->insert(std::make_pair(std::string(data + t + 1, e - t - 1), std::string(data + b, t - b)));
    }
}

// bytes of the `s` fields of one ResultAll (tags and lengths included); p != nullptr: also written there
inline size_t meta_encode_samples(uint8_t *p, const sample_codec &c, const uint8_t *value, size_t vlen) {
    using namespace meta_detail;
    size_t total = 0;
    for_each_record(c, value, vlen, [&](const std::string &g, int32_t cc, int32_t ll) {
        const size_t info = 1 + varint_len(g.size()) + g.size() + 1 + varint_len(wire_int32(cc)) + 1 + varint_len(wire_int32(ll));
        total += 1 + varint_len(info) + info;
        if (!p) return;
        *p++ = 0x12;  // ResultAll.s
        p = put_varint(p, info);
        *p++ = 0x0A;  // ReadInfo.g
        p = put_varint(p, g.size());
        if (!g.empty()) memcpy(p, g.data(), g.size());
        p += g.size();
        *p++ = 0x10;  // c
        p = put_varint(p, wire_int32(cc));
        *p++ = 0x18;  // l
        p = put_varint(p, wire_int32(ll));
    });
    return total;
}

// Reply{rt = request_type, t = (ReplyType) return_type, q, a = ReplyAll{forward_matches | revcomp_matches =
// ResultAll{r, s*}*}} (readserver.proto:16-29,39-54).  Returns the bytes needed; written when out != nullptr and they fit.
inline size_t meta_encode_all_reply(uint8_t *out, size_t cap, int request_type, int return_type, const char *q, size_t qlen, bool revcomp,
                                    const char *const *reads, const size_t *read_len, const uint8_t *const *values, const size_t *value_len,
                                    size_t nreads, const sample_codec &c) {
    using namespace meta_detail;
    std::vector<size_t> slen(nreads);
    size_t body = 0;
    for (size_t i = 0; i < nreads; ++i) {
        slen[i] = meta_encode_samples(nullptr, c, values ? values[i] : nullptr, values ? value_len[i] : 0);
        const size_t ra = 1 + varint_len(read_len[i]) + read_len[i] + slen[i];
        body += 1 + varint_len(ra) + ra;
    }
    const size_t len = 1 + varint_len((uint64_t)request_type) + 1 + varint_len((uint64_t)return_type) + 1 + varint_len(qlen) + qlen + 1 +
                       varint_len(body) + body;
    if (!out || len > cap) return len;
    uint8_t *p = out;
    *p++ = 0x08; p = put_varint(p, (uint64_t)request_type);  // rt
    *p++ = 0x10; p = put_varint(p, (uint64_t)return_type);   // t = (ReplyType) request rt (service.cpp:1263)
    *p++ = 0x1A; p = put_varint(p, qlen);
    if (qlen) memcpy(p, q, qlen);
    p += qlen;
    *p++ = 0x32; p = put_varint(p, body);  // a: present even when empty (mutable_a(), :1293)
    for (size_t i = 0; i < nreads; ++i) {
        const size_t ra = 1 + varint_len(read_len[i]) + read_len[i] + slen[i];
        *p++ = revcomp ? 0x12 : 0x0A; p = put_varint(p, ra);
        *p++ = 0x0A; p = put_varint(p, read_len[i]);  // ResultAll.r
        if (read_len[i]) memcpy(p, reads[i], read_len[i]);
        p += read_len[i];
        p += meta_encode_samples(p, c, values ? values[i] : nullptr, values ? value_len[i] : 0);
    }
    return len;
}

}  // namespace rsb
#endif
