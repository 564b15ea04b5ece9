// unitig_rule.h -- the decision of one step of a unitig side (include/rsbwt.h: the definition), for the device
// (walk.hip, unitig_kernel), the host (graph_steps.h, a set over several device groups) and, as a program of its own,
// tests/native/unitig_rule_host.cpp.
//
// A step has eight sums: the four ONWARD supports of the side's string in its own direction, and -- looked at only where
// exactly one onward support reaches m -- the four RETURN supports of the node that symbol enters, in the opposite
// direction.  The step either appends the one live symbol or stops the side:
//     steps == max_steps                 LIMIT      (no sum is looked at)
//     no onward support >= m             DEAD_END
//     two or more                        BRANCH
//     one, two or more return >= m       JOIN       (the symbol is not appended)
//     one, at most one return >= m       the symbol is appended
// The kernel takes the decision in two halves, because the return sums are searched only after the onward half has named
// the node: unitig_onward, then unitig_return.  unitig_rule is both in a row.
#ifndef RSBWT_UNITIG_RULE_H
#define RSBWT_UNITIG_RULE_H

#include <stdint.h>

#if defined(__HIPCC__)
#define UNITIG_RULE_HD __host__ __device__ inline
#else
#define UNITIG_RULE_HD inline
#endif

namespace rsb {

// (the values of RSBWT_WALK_* in include/rsbwt.h; walk.hip asserts that they are)
constexpr uint32_t UNITIG_GO = 0, UNITIG_DEAD_END = 1, UNITIG_BRANCH = 2, UNITIG_LIMIT = 3, UNITIG_JOIN = 5;

// The onward half: UNITIG_GO with *pick = the one live symbol (0..3 = A, C, G, T), or the stop.  m >= 1.
UNITIG_RULE_HD uint32_t unitig_onward(const uint64_t onward[4], uint64_t m, uint32_t steps, uint32_t max_steps, uint32_t *pick) {
    if (steps >= max_steps) return UNITIG_LIMIT;
    uint32_t nlive = 0;
    for (uint32_t b = 0; b < 4u; ++b)
        if (onward[b] >= m) {
            ++nlive;
            *pick = b;
        }
    return nlive == 1u ? UNITIG_GO : nlive == 0u ? UNITIG_DEAD_END : UNITIG_BRANCH;
}

// The return half, of the node the picked symbol enters: UNITIG_JOIN where another path enters it too.
UNITIG_RULE_HD uint32_t unitig_return(const uint64_t back[4], uint64_t m) {
    uint32_t nlive = 0;
    for (uint32_t b = 0; b < 4u; ++b) nlive += back[b] >= m ? 1u : 0u;
    return nlive >= 2u ? UNITIG_JOIN : UNITIG_GO;
}

// The whole step over sums[0..3] onward, sums[4..7] return: UNITIG_GO with *pick = the symbol to append, or the stop.
UNITIG_RULE_HD uint32_t unitig_rule(const uint64_t sums[8], uint64_t m, uint32_t steps, uint32_t max_steps, uint32_t *pick) {
    const uint32_t stop = unitig_onward(sums, m, steps, max_steps, pick);
    return stop != UNITIG_GO ? stop : unitig_return(sums + 4, m);
}

// the support noted for an appended symbol
UNITIG_RULE_HD uint32_t unitig_saturate(uint64_t support) { return support > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)support; }

}  // namespace rsb
#endif
