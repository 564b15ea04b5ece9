// gt_span_rule.h -- the length test of a row of a LEFT leg of SiteMatch (find_gt_reads, src/service/service.cpp:538), for
// the device (site_counts.hip), the host (sets.hip) and, as a program of its own, tests/native/gt_span_rule_host.cpp.
//
// A row of a leg whose tile lies left of the site (end < pos) is DROPPED iff
//     pos - end > (|postfix| - k) + indel_allowance,       |postfix| = |read| - offset, indel_allowance = 4,
// all in unsigned 64-bit as the reference takes it: pos < end wraps the left side to a number no read reaches.  offset is
// where the leg's string starts in the read, so the read holds at least the k symbols of the tile from there on:
// |read| >= offset + k, and the right side does not wrap.
#ifndef RSBWT_GT_SPAN_RULE_H
#define RSBWT_GT_SPAN_RULE_H

#include <stdint.h>

#if defined(__HIPCC__)
#define GT_RULE_HD __host__ __device__ inline
#else
#define GT_RULE_HD inline
#endif

namespace rsb {

constexpr uint64_t GT_INDEL_ALLOWANCE = 4;

// the reference's test as written
GT_RULE_HD bool gt_left_row_stays(uint64_t pos, uint64_t end, uint64_t offset, uint64_t k, uint64_t read_len) {
    return !(pos - end > (read_len - offset) - k + GT_INDEL_ALLOWANCE);
}

// The same test solved for the read's length: the row stays iff read_len >= gt_left_needed_len(...), for every read_len >=
// offset + k.  Saturates at 2^64 - 1 (no read is that long).  A read reached through several rows is a candidate iff one
// of them stays, that is iff its length reaches the SMALLEST of their needs; a row that is not pending needs 0.
GT_RULE_HD uint64_t gt_left_needed_len(uint64_t pos, uint64_t end, uint64_t offset, uint64_t k) {
    const uint64_t d = pos - end, base = offset + k;
    if (d <= GT_INDEL_ALLOWANCE) return base;
    const uint64_t extra = d - GT_INDEL_ALLOWANCE;
    return extra > ~0ull - base ? ~0ull : base + extra;
}

}  // namespace rsb
#endif
