// sample_walk_rule.h -- what the host decides about a sample walk (include/rsbwt.h: the definition), for the device
// (sample_walk.hip), the host (set_graph.hip, graph_steps.h) and, as a program of its own, tests/native/sample_walk_rule_host.cpp.
//
//   MASK    u8[C], one byte per code of the ascending dictionary -> one bit per column (bit col of word col / 32).  The
//           unknown-code column C has no bit: it never counts.
//   SLICE   a step's scratch is bounded by seeds x 8 x max_rows rows (8 = 4 bases x 2 strands) of SAMPLE_WALK_ROW_BYTES
//           each: row 8, ordinal 8, shard 4, and 32 for its share of the de-duplication set (under 4 slots of 8 bytes a
//           row).  A call walks its seeds in slices that keep this under SAMPLE_WALK_BUDGET (256 MiB) of HBM -- one seed at
//           the least, whatever it needs (448 MiB at max_rows = 2^20) -- and under SAMPLE_WALK_SLICE_SEEDS, so that
//           (shard, unit = seed x 8 + base x 2 + strand, ordinal) fit the set's 64-bit key: 10 + 14 + 40 bits.
//   WIDE    an evaluation is wide when any of its (up to 8) candidate-strand queries has more rows over the shards than
//           max_rows; the seed stops there and nothing of the evaluation is counted.
//   SUPPORT the masked support of a symbol: its two strands' sums added, a negative total (copies can be negative) = 0.
//   STEP    the walk's decision over the four masked supports: append *pick, or stop.
#ifndef RSBWT_SAMPLE_WALK_RULE_H
#define RSBWT_SAMPLE_WALK_RULE_H

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define SAMPLE_WALK_HD __host__ __device__ inline
#else
#define SAMPLE_WALK_HD inline
#endif

namespace rsb {

// (the values of RSBWT_WALK_* in include/rsbwt.h; sample_walk.hip asserts that they are)
constexpr uint32_t SAMPLE_WALK_GO = 0, SAMPLE_WALK_DEAD_END = 1, SAMPLE_WALK_BRANCH = 2, SAMPLE_WALK_LIMIT = 3, SAMPLE_WALK_INVALID = 4,
                   SAMPLE_WALK_WIDE = 8;
constexpr uint32_t SAMPLE_WALK_COPIES = 4u;  // RSBWT_WALK_SAMPLE_COPIES
constexpr uint64_t SAMPLE_WALK_MAX_ROWS = 1ull << 20;
constexpr size_t SAMPLE_WALK_ROW_BYTES = 52;
constexpr size_t SAMPLE_WALK_BUDGET = (size_t)256 << 20;
constexpr size_t SAMPLE_WALK_SLICE_SEEDS = 2048;
constexpr uint32_t SAMPLE_WALK_MAX_SHARDS = 1024;

SAMPLE_WALK_HD bool sample_walk_rows_ok(uint64_t max_rows) { return max_rows >= 1 && max_rows <= SAMPLE_WALK_MAX_ROWS; }

// the rows a slice of `seeds` seeds needs room for
SAMPLE_WALK_HD uint64_t sample_walk_cap_rows(size_t seeds, uint64_t max_rows) { return (uint64_t)seeds * 8ull * max_rows; }

// the seeds of a slice: as many as keep the rows' scratch under `budget`, 1 .. SAMPLE_WALK_SLICE_SEEDS
SAMPLE_WALK_HD size_t sample_walk_slice_seeds(uint64_t max_rows, size_t budget) {
    const uint64_t per_seed = 8ull * max_rows * SAMPLE_WALK_ROW_BYTES;
    const uint64_t n = per_seed ? (uint64_t)budget / per_seed : SAMPLE_WALK_SLICE_SEEDS;
    return n < 1 ? 1 : n > SAMPLE_WALK_SLICE_SEEDS ? SAMPLE_WALK_SLICE_SEEDS : (size_t)n;
}

// the slots of the set for `rows` rows: a power of two, at least 2 x rows + 1, under 4 x rows + 2
SAMPLE_WALK_HD uint64_t sample_walk_set_slots(uint64_t rows) {
    uint64_t slots = 2;
    while (slots < 2ull * rows + 1ull) slots <<= 1;
    return slots;
}

// words of the column bitmap
SAMPLE_WALK_HD size_t sample_walk_mask_words(size_t C) { return (C + 31) / 32; }

// mask u8[C] -> bits[sample_walk_mask_words(C)]; returns the columns that count
inline size_t sample_walk_mask_bits(const uint8_t *mask, size_t C, uint32_t *bits) {
    size_t on = 0;
    for (size_t w = 0; w < sample_walk_mask_words(C); ++w) bits[w] = 0u;
    for (size_t c = 0; c < C; ++c)
        if (mask[c]) {
            bits[c >> 5] |= 1u << (c & 31u);
            ++on;
        }
    return on;
}

SAMPLE_WALK_HD bool sample_walk_counts(const uint32_t *bits, uint32_t C, uint32_t col) { return col < C && ((bits[col >> 5] >> (col & 31u)) & 1u) != 0u; }

// matches8: the rows over the shards of the unit's queries, [base x 2 + strand]
SAMPLE_WALK_HD bool sample_walk_wide(const uint64_t matches8[8], uint64_t max_rows) {
    for (uint32_t i = 0; i < 8u; ++i)
        if (matches8[i] > max_rows) return true;
    return false;
}

SAMPLE_WALK_HD uint64_t sample_walk_support(int64_t forward, int64_t reverse) {
    const int64_t t = forward + reverse;
    return t < 0 ? 0ull : (uint64_t)t;
}

// (shard < 2^10, unit < 2^14, ordinal < 2^40: never all ones, the set's empty slot)
SAMPLE_WALK_HD uint64_t sample_walk_key(uint32_t shard, uint32_t unit, uint64_t ordinal) {
    return ((uint64_t)shard << 54) | ((uint64_t)unit << 40) | ordinal;
}

// One evaluation's decision: SAMPLE_WALK_GO with *pick = the one live symbol (0..3), or the stop.  m >= 1.  The caller
// appends and stops with LIMIT when that was the max_steps-th symbol.
SAMPLE_WALK_HD uint32_t sample_walk_step(const uint64_t msup[4], bool wide, uint64_t m, uint32_t *pick) {
    if (wide) return SAMPLE_WALK_WIDE;
    uint32_t nlive = 0;
    for (uint32_t b = 0; b < 4u; ++b)
        if (msup[b] >= m) {
            ++nlive;
            *pick = b;
        }
    return nlive == 1u ? SAMPLE_WALK_GO : nlive == 0u ? SAMPLE_WALK_DEAD_END : SAMPLE_WALK_BRANCH;
}

}  // namespace rsb
#endif
