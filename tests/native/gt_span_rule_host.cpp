// gt_span_rule_host.cpp -- readserver_amd/csrc/gt_span_rule.h (the length test of a row of a LEFT leg, as the reference
// writes it and solved for the read's length, shared by csrc/site_counts.hip and csrc/sets.hip) as a program of its own, for
// tests/test_site_reference.py to build with -fsanitize=address,undefined and run.  Input: the largest pos / end, offset,
// k and slack to walk.  Output: one line "pos end offset k len stays need" for every combination with len = offset + k +
// 0 .. slack (a read holds the k symbols of its tile), then the same at the far end of the 64-bit range, where the needed
// length saturates.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../readserver_amd/csrc/gt_span_rule.h"

static void line(uint64_t pos, uint64_t end, uint64_t offset, uint64_t k, uint64_t len) {
    printf("%llu %llu %llu %llu %llu %d %llu\n", (unsigned long long)pos, (unsigned long long)end, (unsigned long long)offset, (unsigned long long)k,
           (unsigned long long)len, rsb::gt_left_row_stays(pos, end, offset, k, len) ? 1 : 0,
           (unsigned long long)rsb::gt_left_needed_len(pos, end, offset, k));
}

int main(int argc, char **argv) {
    if (argc != 5) {
        fprintf(stderr, "usage: %s max_pos max_offset max_k slack\n", argv[0]);
        return 2;
    }
    const uint64_t P = strtoull(argv[1], nullptr, 10), O = strtoull(argv[2], nullptr, 10), K = strtoull(argv[3], nullptr, 10),
                   slack = strtoull(argv[4], nullptr, 10);
    for (uint64_t pos = 0; pos <= P; ++pos)
        for (uint64_t end = 0; end <= P; ++end)
            for (uint64_t offset = 0; offset <= O; ++offset)
                for (uint64_t k = 1; k <= K; ++k)
                    for (uint64_t extra = 0; extra <= slack; ++extra) line(pos, end, offset, k, offset + k + extra);
    const uint64_t top = ~0ull;
    line(top, 0, 0, 1, 4096);
    line(top, 0, top - 8, 4, top - 1);
    line(0, 1, 3, 8, 4096);  // pos < end: the left side wraps
    line(top - 2, top - 3, 5, 8, 13);
    puts("gt_span_rule ok");
    return 0;
}
