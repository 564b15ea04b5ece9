// sample_codes.h -- the caller's sample dictionary of rsbwt_set_sample_counts (include/rsbwt.h): how a code of
// size_of_sample bytes is spelt as a u64 key, and the check a dictionary must pass.  Host code with no HIP in it: the
// set code (sets.hip) and tests/native/sample_codes_host.cpp both build it; sample_counts.hip spells the same key from
// the bytes of a record (sample_key there and here must agree: the most significant byte first).
#ifndef RSBWT_SAMPLE_CODES_H
#define RSBWT_SAMPLE_CODES_H

#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace rsb {

constexpr uint32_t SAMPLE_CODE_MAX = 8;  // bytes of a code: what a u64 key holds

// The key of a code: its bytes as a big-endian number.  Codes of one length compare by memcmp exactly as their keys
// compare as numbers, so a dictionary ascending in memcmp order has ascending keys.
inline uint64_t sample_key(const uint8_t *code, uint32_t size_of_sample) {
    uint64_t k = 0;
    for (uint32_t i = 0; i < size_of_sample; ++i) k = (k << 8) | code[i];
    return k;
}

enum { SAMPLE_CODES_OK = 0, SAMPLE_CODES_SIZE = 1, SAMPLE_CODES_EMPTY = 2, SAMPLE_CODES_NULL = 3, SAMPLE_CODES_ORDER = 4 };

// C codes of size_of_sample bytes each, back to back: size_of_sample in 1..8, C > 0, strictly ascending in memcmp order
// (so: distinct).  On SAMPLE_CODES_OK keys holds the C keys; on SAMPLE_CODES_ORDER *bad (optional) is the index of the
// first code that is not above its predecessor.
inline int sample_codes_check(const uint8_t *codes, size_t C, uint32_t size_of_sample, std::vector<uint64_t> *keys, size_t *bad) {
    if (size_of_sample < 1u || size_of_sample > SAMPLE_CODE_MAX) return SAMPLE_CODES_SIZE;
    if (C == 0) return SAMPLE_CODES_EMPTY;
    if (!codes) return SAMPLE_CODES_NULL;
    keys->resize(C);
    for (size_t i = 0; i < C; ++i) {
        (*keys)[i] = sample_key(codes + i * (size_t)size_of_sample, size_of_sample);
        if (i && (*keys)[i] <= (*keys)[i - 1]) {
            if (bad) *bad = i;
            return SAMPLE_CODES_ORDER;
        }
    }
    return SAMPLE_CODES_OK;
}

// the column of a key: its index in the ascending keys, C when it is not among them (the binary search the kernel runs)
inline size_t sample_column(const uint64_t *keys, size_t C, uint64_t key) {
    size_t lo = 0, hi = C;
    while (lo < hi) {
        const size_t mid = lo + (hi - lo) / 2;
        if (keys[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo < C && keys[lo] == key ? lo : C;
}

}  // namespace rsb

#endif
