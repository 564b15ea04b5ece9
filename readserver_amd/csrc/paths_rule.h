// paths_rule.h -- the decisions of rsbwt_set_paths' depth-first search from a seed (include/rsbwt.h: the definition), for the
// device (paths.hip, paths_kernel), the host (graph_steps.h, a set over several device groups) and, as a program of its own,
// tests/native/paths_rule_host.cpp.
//
// A seed's search holds the current path, the evaluations made so far and a FRAME STORE: a stack with one frame per depth
// at which live symbols are still untried, the deepest on top.  A frame keeps what a backtrack to it needs without looking
// at anything again: the untried symbols (4 bits), the four supports of that depth's evaluation (saturated) and the least
// support of the path below that depth.  In the order of the definition:
//     paths_end        the end test of the current path: TARGET, then LIMIT, then BUDGET, else the path is evaluated
//     paths_live       the live symbols of an evaluation, bit c = "ACGT"[c]
//     paths_advance    a non-empty live set: the first live symbol is appended, the others go into a new frame
//                      (an empty one ends the path with DEAD_END: the caller's)
//     paths_done       after a path has gone out: BUDGET, then COMPLETE (no frame), then MORE (max_paths paths), else
//     paths_backtrack  the deepest frame gives up its first untried symbol: the path is path[:depth] + that symbol
// The frame store has room for min(max_steps, max_evals) frames (paths_frames): frames sit at distinct depths below
// max_steps, and every frame was pushed by an evaluation of its own.
#ifndef RSBWT_PATHS_RULE_H
#define RSBWT_PATHS_RULE_H

#include <stdint.h>

#if defined(__HIPCC__)
#define PATHS_RULE_HD __host__ __device__ inline
#else
#define PATHS_RULE_HD inline
#endif

namespace rsb {

// (the values of RSBWT_WALK_* and RSBWT_PATHS_* in include/rsbwt.h; paths.hip asserts that they are)
constexpr uint32_t PATHS_GO = 0, PATHS_DEAD_END = 1, PATHS_LIMIT = 3, PATHS_TARGET = 6, PATHS_BUDGET = 7;
constexpr uint32_t PATHS_COMPLETE = 1, PATHS_MORE = 2, PATHS_OUT_OF_BUDGET = 3, PATHS_INVALID = 4;
constexpr uint32_t PATHS_NO_SUPPORT = 0xFFFFFFFFu;  // the least support of a path of no symbols, as the search keeps it

struct paths_frame {
    uint32_t depth;       // the length of the path the frame's evaluation was made at
    uint32_t untried;     // bit c: "ACGT"[c] is live at that depth and has not been taken
    uint32_t min_before;  // the least support of path[:depth] (PATHS_NO_SUPPORT at depth 0)
    uint32_t pad;
    uint32_t sup[4];      // the evaluation's supports, saturated
};

PATHS_RULE_HD uint32_t paths_saturate(uint64_t support) { return support > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)support; }
PATHS_RULE_HD uint32_t paths_min(uint32_t a, uint32_t b) { return a < b ? a : b; }
PATHS_RULE_HD uint32_t paths_first(uint32_t mask) { return (mask & 1u) ? 0u : (mask & 2u) ? 1u : (mask & 4u) ? 2u : 3u; }
// the frames a seed's store must hold
PATHS_RULE_HD uint32_t paths_frames(uint32_t max_steps, uint32_t max_evals) { return max_steps < max_evals ? max_steps : max_evals; }
// what goes out as a path's min_support
PATHS_RULE_HD uint32_t paths_min_out(uint32_t steps, uint32_t min_cur) { return steps == 0u ? 0u : min_cur; }

// The end test of a path of `steps` symbols after `evals` evaluations: PATHS_GO = evaluate it.  at_target: the seed has a
// target and the symbols at the walking end are the target's (looked at only where steps >= 1: the seed is the source anchor).
PATHS_RULE_HD uint32_t paths_end(bool at_target, uint32_t steps, uint32_t max_steps, uint32_t evals, uint32_t max_evals) {
    if (at_target && steps >= 1u) return PATHS_TARGET;
    if (steps >= max_steps) return PATHS_LIMIT;
    if (evals >= max_evals) return PATHS_BUDGET;
    return PATHS_GO;
}

PATHS_RULE_HD uint32_t paths_live(const uint64_t sup[4], uint64_t m) {
    uint32_t mask = 0;
    for (uint32_t c = 0; c < 4u; ++c)
        if (sup[c] >= m) mask |= 1u << c;
    return mask;
}

// An evaluation at `depth` found `live` != 0: returns the symbol to append (0..3), pushes a frame where others are live too,
// and takes the symbol's support into *min_cur.
PATHS_RULE_HD uint32_t paths_advance(paths_frame *stack, uint32_t *nframes, uint32_t depth, uint32_t live, const uint64_t sup[4], uint32_t *min_cur) {
    const uint32_t pick = paths_first(live), rest = live & ~(1u << pick);
    if (rest != 0u) {
        paths_frame f;
        f.depth = depth;
        f.untried = rest;
        f.min_before = *min_cur;
        f.pad = 0u;
        for (uint32_t c = 0; c < 4u; ++c) f.sup[c] = paths_saturate(sup[c]);
        stack[(*nframes)++] = f;
    }
    // (a chain of selects: an index that is not a constant would put the four sums into scratch memory on the device)
    const uint64_t mine = pick == 0u ? sup[0] : pick == 1u ? sup[1] : pick == 2u ? sup[2] : sup[3];
    *min_cur = paths_min(*min_cur, paths_saturate(mine));
    return pick;
}

// After a path has gone out with `stop` as number `npaths` (1-based): the seed's state, or PATHS_GO = backtrack.
PATHS_RULE_HD uint32_t paths_done(uint32_t stop, uint32_t nframes, uint32_t npaths, uint32_t max_paths) {
    if (stop == PATHS_BUDGET) return PATHS_OUT_OF_BUDGET;
    if (nframes == 0u) return PATHS_COMPLETE;
    if (npaths >= max_paths) return PATHS_MORE;
    return PATHS_GO;
}

// The backtrack (*nframes >= 1): returns the symbol c; the path becomes path[:*depth] + c and *min_cur its least support.
PATHS_RULE_HD uint32_t paths_backtrack(paths_frame *stack, uint32_t *nframes, uint32_t *depth, uint32_t *min_cur) {
    paths_frame *f = &stack[*nframes - 1u];  // (read where it lies: nothing of it is indexed in registers)
    const uint32_t untried = f->untried, c = paths_first(untried), rest = untried & ~(1u << c);
    *depth = f->depth;
    *min_cur = paths_min(f->min_before, f->sup[c]);
    if (rest == 0u) --*nframes;
    else f->untried = rest;
    return c;
}

}  // namespace rsb
#endif
