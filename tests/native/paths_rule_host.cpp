// paths_rule_host.cpp -- readserver_amd/csrc/paths_rule.h as a program of its own, for the address and undefined-behaviour
// sanitizers (tests/test_paths_reference.py builds and runs it, and restates the search in Python).
//
// The header's decisions drive the depth-first search exactly as the host loop of graph_steps.h and the writer lane of
// paths_kernel do, over a graph that is a function of the path alone: the supports of path p from seed s are FNV-1a hashes
// of "<s>:" + p + symbol, mapped onto a small table that holds zeros, small counts and counts at and past 32 bits.  The
// frame store is allocated at exactly paths_frames(max_steps, max_evals) frames, so a push past it is a heap overflow
// the address sanitizer reports.
//   paths_rule_host m max_steps max_paths max_evals seeds target
// prints per seed "state npaths evals", then per path "ext stop min_support" ('-' for a path of no symbols), then "paths_rule ok".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "../../readserver_amd/csrc/paths_rule.h"

using namespace rsb;

static const uint64_t TABLE[16] = {0, 0, 0, 0, 0, 0, 0, 1, 1, 2, 3, 5, 9, 0xFFFFFFFFull, 0x100000000ull, 0x200000005ull};

static uint64_t support(uint32_t seed, const std::string &path, uint32_t c) {
    const std::string key = std::to_string(seed) + ":" + path + "ACGT"[c];
    uint64_t h = 1469598103934665603ull;
    for (unsigned char ch : key) h = (h ^ ch) * 1099511628211ull;
    return TABLE[(h >> 20) & 15u];
}

int main(int argc, char **argv) {
    if (argc != 7) {
        fprintf(stderr, "usage: paths_rule_host m max_steps max_paths max_evals seeds target\n");
        return 2;
    }
    const uint64_t m = strtoull(argv[1], nullptr, 10);
    const uint32_t max_steps = (uint32_t)strtoul(argv[2], nullptr, 10), max_paths = (uint32_t)strtoul(argv[3], nullptr, 10),
                   max_evals = (uint32_t)strtoul(argv[4], nullptr, 10), seeds = (uint32_t)strtoul(argv[5], nullptr, 10);
    const std::string target = argv[6][0] == '-' ? "" : argv[6];
    for (uint32_t s = 0; s < seeds; ++s) {
        std::vector<paths_frame> frames(paths_frames(max_steps, max_evals));
        std::string path;
        std::vector<std::string> lines;
        uint32_t nframes = 0, evals = 0, npaths = 0, min_cur = PATHS_NO_SUPPORT, state = PATHS_GO;
        auto at_target = [&]() { return !target.empty() && path.size() >= target.size() && path.compare(path.size() - target.size(), target.size(), target) == 0; };
        uint32_t stop = paths_end(at_target(), 0u, max_steps, evals, max_evals);  // (never a stop at 0 steps: the limits are >= 1)
        if (stop != PATHS_GO) return 3;
        while (state == PATHS_GO) {
            uint64_t sup[4];
            for (uint32_t c = 0; c < 4u; ++c) sup[c] = support(s, path, c);
            ++evals;
            const uint32_t live = paths_live(sup, m);
            stop = PATHS_DEAD_END;
            if (live != 0u) {
                path += "ACGT"[paths_advance(frames.data(), &nframes, (uint32_t)path.size(), live, sup, &min_cur)];
                stop = paths_end(at_target(), (uint32_t)path.size(), max_steps, evals, max_evals);
            }
            while (stop != PATHS_GO) {
                lines.push_back((path.empty() ? std::string("-") : path) + " " + std::to_string(stop) + " " +
                                std::to_string(paths_min_out((uint32_t)path.size(), min_cur)));
                ++npaths;
                state = paths_done(stop, nframes, npaths, max_paths);
                if (state != PATHS_GO) break;
                uint32_t d = 0;
                const uint32_t c = paths_backtrack(frames.data(), &nframes, &d, &min_cur);
                path.resize(d);
                path += "ACGT"[c];
                stop = paths_end(at_target(), (uint32_t)path.size(), max_steps, evals, max_evals);
            }
        }
        printf("%u %u %u\n", state, npaths, evals);
        for (const std::string &ln : lines) printf("%s\n", ln.c_str());
    }
    printf("paths_rule ok\n");
    return 0;
}
