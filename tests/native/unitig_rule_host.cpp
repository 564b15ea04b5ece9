// unitig_rule_host.cpp -- readserver_amd/csrc/unitig_rule.h (the decision of one step of a unitig side, shared by
// csrc/walk.hip's unitig_kernel and csrc/graph_steps.h, the loop of a set over several device groups) as a program of its own, for
// tests/test_unitig_reference.py to build with -fsanitize=address,undefined and run.  Input: m and max_steps.  Output:
// one line "steps s0 .. s7 stop pick halves saturated" for every pattern of (sum >= m) over the eight sums -- a live sum
// is m + its index, a dead one m - 1 -- at steps 0, max_steps - 1 and max_steps; `stop` and `pick` are unitig_rule's (pick
// is -1 where nothing is appended), `halves` is 1 where unitig_onward followed by unitig_return says the same, `saturated`
// is unitig_saturate of the picked sum; then the same for sums beyond 32 bits.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../readserver_amd/csrc/unitig_rule.h"

static void line(const uint64_t sums[8], uint64_t m, uint32_t steps, uint32_t max_steps) {
    uint32_t pick = 99, pick2 = 99;
    const uint32_t stop = rsb::unitig_rule(sums, m, steps, max_steps, &pick);
    uint32_t stop2 = rsb::unitig_onward(sums, m, steps, max_steps, &pick2);
    if (stop2 == rsb::UNITIG_GO) stop2 = rsb::unitig_return(sums + 4, m);
    const bool go = stop == rsb::UNITIG_GO;
    printf("%u", steps);
    for (int i = 0; i < 8; ++i) printf(" %llu", (unsigned long long)sums[i]);
    printf(" %u %d %d %u\n", stop, go ? (int)pick : -1, stop == stop2 && (!go || pick == pick2) ? 1 : 0, go ? rsb::unitig_saturate(sums[pick]) : 0u);
}

int main(int argc, char **argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: %s m max_steps\n", argv[0]);
        return 2;
    }
    const uint64_t m = strtoull(argv[1], nullptr, 10);
    const uint32_t max_steps = (uint32_t)strtoul(argv[2], nullptr, 10);
    if (m < 1 || max_steps < 1) return 2;
    const uint32_t at[3] = {0u, max_steps - 1u, max_steps};
    for (int big = 0; big < 2; ++big)
        for (int a = 0; a < 3; ++a)
            for (uint32_t pattern = 0; pattern < 256u; ++pattern) {
                uint64_t sums[8];
                for (uint32_t i = 0; i < 8u; ++i) {
                    const bool live = (pattern >> i) & 1u;
                    sums[i] = live ? m + i + (big ? (1ull << 32) - 3ull : 0ull) : m - 1;
                }
                line(sums, m, at[a], max_steps);
            }
    puts("unitig_rule ok");
    return 0;
}
