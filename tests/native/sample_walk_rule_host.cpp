// sample_walk_rule_host.cpp -- readserver_amd/csrc/sample_walk_rule.h as a program of its own (built by
// tests/test_sample_walk_reference.py with -fsanitize=address,undefined): the mask's bitmap, the slice sizing, the WIDE
// rule, the support's clamp, the set's key and the step's decision, printed for the test to hold against its own
// restatement.
//   sample_walk_rule_host C max_rows m
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <initializer_list>
#include <set>
#include <vector>

#include "../../readserver_amd/csrc/sample_walk_rule.h"

using namespace rsb;

static uint64_t rnd(uint64_t &s) {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return s >> 17;
}

int main(int argc, char **argv) {
    if (argc != 4) return 2;
    const size_t C = (size_t)strtoull(argv[1], nullptr, 10);
    const uint64_t max_rows = strtoull(argv[2], nullptr, 10), m = strtoull(argv[3], nullptr, 10);
    uint64_t seed = 12345 + C;
    // ---- the mask: exactly-sized heap arrays, so a byte or a word too far is the sanitizer's
    std::vector<uint8_t> mask(C);
    for (size_t c = 0; c < C; ++c) mask[c] = rnd(seed) % 3 == 0 ? (uint8_t)(1 + rnd(seed) % 255) : 0;
    std::vector<uint32_t> bits(sample_walk_mask_words(C), 0xFFFFFFFFu);
    const size_t on = sample_walk_mask_bits(mask.data(), C, bits.data());
    size_t seen = 0;
    for (size_t c = 0; c < C; ++c) {
        const bool b = sample_walk_counts(bits.data(), (uint32_t)C, (uint32_t)c);
        if (b != (mask[c] != 0)) return 3;
        seen += b;
    }
    if (seen != on || sample_walk_counts(bits.data(), (uint32_t)C, (uint32_t)C)) return 4;  // the unknown-code column never counts
    for (size_t w = 0; w < bits.size(); ++w)  // no bit past column C - 1
        for (uint32_t i = 0; i < 32; ++i)
            if (w * 32 + i >= C && ((bits[w] >> i) & 1u)) return 5;
    printf("mask %zu %zu %zu\n", C, sample_walk_mask_words(C), on);
    // ---- slices
    printf("rows_ok %d %d %d %d\n", (int)sample_walk_rows_ok(0), (int)sample_walk_rows_ok(1), (int)sample_walk_rows_ok(1ull << 20),
           (int)sample_walk_rows_ok((1ull << 20) + 1));
    const size_t per = sample_walk_slice_seeds(max_rows, SAMPLE_WALK_BUDGET);
    printf("slice %llu %zu %llu\n", (unsigned long long)max_rows, per, (unsigned long long)sample_walk_cap_rows(per, max_rows));
    if (per < 1 || per > SAMPLE_WALK_SLICE_SEEDS) return 6;
    if (per > 1 && sample_walk_cap_rows(per, max_rows) * SAMPLE_WALK_ROW_BYTES > SAMPLE_WALK_BUDGET) return 7;
    if (per < SAMPLE_WALK_SLICE_SEEDS && sample_walk_cap_rows(per + 1, max_rows) * SAMPLE_WALK_ROW_BYTES <= SAMPLE_WALK_BUDGET) return 8;
    for (uint64_t rows : std::initializer_list<uint64_t>{0, 1, 2, 3, 1000, max_rows * 8, sample_walk_cap_rows(per, max_rows)}) {
        const uint64_t slots = sample_walk_set_slots(rows);
        if ((slots & (slots - 1)) != 0 || slots < 2 * rows + 1 || slots >= 4 * rows + 2 + 1) return 9;
        if (slots * 8 > 32 * rows + 16) return 10;  // the set's share of SAMPLE_WALK_ROW_BYTES
        printf("slots %llu %llu\n", (unsigned long long)rows, (unsigned long long)slots);
    }
    // ---- keys: distinct over the corners of the three fields, never the empty slot
    std::set<uint64_t> keys;
    size_t made = 0;
    for (uint32_t sh : {0u, 1u, 1023u})
        for (uint32_t unit : {0u, 1u, 7u, 8u, 16383u})
            for (uint64_t o : std::initializer_list<uint64_t>{0, 1, (1ull << 40) - 1}) {
                const uint64_t k = sample_walk_key(sh, unit, o);
                if (k == ~0ull && !(sh == 1023u && unit == 16383u && o == (1ull << 40) - 1ull)) return 11;
                keys.insert(k);
                ++made;
            }
    if (keys.size() != made) return 12;
    // ---- WIDE, the support and the step, over every (sum >= m) pattern and sums round max_rows
    for (uint32_t pat = 0; pat < 16; ++pat)
        for (int wide = 0; wide < 2; ++wide) {
            uint64_t sup[4];
            for (uint32_t b = 0; b < 4; ++b) sup[b] = (pat >> b) & 1u ? m + rnd(seed) % 3 + (b == 3 ? (1ull << 33) : 0) : (m > 1 ? rnd(seed) % m : 0);
            uint32_t pick = 99;
            const uint32_t why = sample_walk_step(sup, wide != 0, m, &pick);
            printf("step %u %d %llu %llu %llu %llu %u %u\n", pat, wide, (unsigned long long)sup[0], (unsigned long long)sup[1], (unsigned long long)sup[2],
                   (unsigned long long)sup[3], why, why == SAMPLE_WALK_GO ? pick : 99u);
        }
    for (uint32_t at = 0; at < 9; ++at) {
        uint64_t m8[8];
        for (uint32_t i = 0; i < 8; ++i) m8[i] = i == at ? max_rows + 1 : (i % 2 ? max_rows : rnd(seed) % (max_rows + 1));
        printf("wide %u %d\n", at, (int)sample_walk_wide(m8, max_rows));
    }
    for (int64_t f : std::initializer_list<int64_t>{-5, 0, 3, (int64_t)1 << 40})
        for (int64_t r : std::initializer_list<int64_t>{-4, 0, 5}) printf("support %lld %lld %llu\n", (long long)f, (long long)r, (unsigned long long)sample_walk_support(f, r));
    printf("sample_walk_rule ok\n");
    return 0;
}
