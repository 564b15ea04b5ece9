// graph_steps_host.cpp -- readserver_amd/csrc/graph_steps.h as a program of its own, for the address and undefined-behaviour
// sanitizers (tests/test_graph_steps_host.py builds and runs it and holds what it prints to walk_reference, unitig_reference
// and paths_reference).
//
// The loops a set over several device groups runs on the host, driven by an evaluator with no device and no BWT in it: the
// support of a candidate of ctx + 1 symbols is the number of times it occurs in the reads, overlapping occurrences
// included -- one hash map per shard, the reverse complement's count added under both strands, summed over the shards.
// With a row cap an evaluation is wide where a candidate (either strand's, on its own) occurs more often than the cap; its
// sums stay as counted, so a loop that let them into `last` would show.  Every output array is allocated at exactly the size the call states and filled with 0x77 first.
//   graph_steps_host walk    READS SEEDS ctx m max_steps left both optional cap      (cap 0: none)
//   graph_steps_host unitigs READS SEEDS ctx m max_steps both optional
//   graph_steps_host paths   READS SEEDS TARGETS|- ctx m max_steps max_paths max_evals left both optional
// READS: "S", then per shard "n" and n reads, a line each; SEEDS, TARGETS: "Q", then Q lines (an empty line: no symbols).
// optional 0: support / last / min_support are passed as null and printed as "-".
// walk, unitigs: a line per seed / item "ext steps stop support,.. last,..";  paths: per seed "state npaths", then per path
// "ext steps stop min_support";  ('-' for no symbols), then "work appended w6 w7" and "graph_steps ok".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <fstream>
#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../readserver_amd/csrc/graph_steps.h"

using namespace rsb;

static std::vector<std::string> read_lines(std::istream &in) {
    std::string ln;
    std::getline(in, ln);
    std::vector<std::string> out(strtoull(ln.c_str(), nullptr, 10));
    for (std::string &s : out) std::getline(in, s);
    return out;
}

static std::vector<std::string> lines_of(const char *path) {
    std::ifstream in(path);
    if (!in) {
        fprintf(stderr, "cannot open %s\n", path);
        exit(2);
    }
    return read_lines(in);
}

static std::string rc_of(const std::string &x) {
    std::string r(x.rbegin(), x.rend());
    for (char &ch : r) ch = ch == 'A' ? 'T' : ch == 'C' ? 'G' : ch == 'G' ? 'C' : 'A';
    return r;
}

struct counting_evaluator {
    std::vector<std::unordered_map<std::string, uint64_t>> shards;  // candidate -> occurrences, per shard
    uint32_t ctx;
    bool both;
    uint64_t cap;  // 0: nothing is wide

    counting_evaluator(const char *path, uint32_t ctx_, bool both_, uint64_t cap_) : ctx(ctx_), both(both_), cap(cap_) {
        std::ifstream in(path);
        if (!in) {
            fprintf(stderr, "cannot open %s\n", path);
            exit(2);
        }
        std::string ln;
        std::getline(in, ln);
        shards.resize(strtoull(ln.c_str(), nullptr, 10));
        for (auto &map : shards)
            for (const std::string &r : read_lines(in))
                for (size_t i = 0; i + ctx + 1 <= r.size(); ++i) ++map[r.substr(i, ctx + 1)];
    }
    uint64_t count(const std::string &x) const {
        uint64_t n = 0;
        for (const auto &map : shards) {
            const auto it = map.find(x);
            if (it != map.end()) n += it->second;
        }
        return n;
    }
    int operator()(const std::vector<std::string> &ctxs, bool left, uint64_t *sums, uint8_t *wide) const {
        for (size_t i = 0; i < ctxs.size(); ++i) {
            if (ctxs[i].size() != ctx) return RSBWT_EINVAL;
            for (uint32_t c = 0; c < 4u; ++c) {
                const std::string x = left ? std::string(1, "ACGT"[c]) + ctxs[i] : ctxs[i] + "ACGT"[c];
                const uint64_t fwd = count(x), rev = both ? count(rc_of(x)) : 0;
                sums[i * 4 + c] = fwd + rev;
                if (cap && (fwd > cap || rev > cap)) wide[i] = 1;
            }
        }
        return RSBWT_OK;
    }
};

// text back to back and offsets, as the calls take them
struct batch {
    std::string text;
    std::vector<uint64_t> off{0};
    explicit batch(const std::vector<std::string> &strs) {
        for (const std::string &s : strs) {
            text += s;
            off.push_back(text.size());
        }
    }
};

template <class T>
static std::unique_ptr<T[]> exactly(size_t n) {
    std::unique_ptr<T[]> p(new T[n]);
    memset(p.get(), 0x77, n * sizeof(T));
    return p;
}

// what a loop leaves past the symbols it wrote: zeros
template <class T>
static bool zero_past(const T *p, size_t from, size_t to) {
    for (size_t i = from; i < to; ++i)
        if (p[i] != 0) return false;
    return true;
}

static std::string symbols(const char *p, uint32_t n) { return n ? std::string(p, n) : std::string("-"); }

template <class T>
static std::string joined(const T *p, size_t n) {
    if (!p) return "-";
    std::string out;
    for (size_t i = 0; i < n; ++i) out += (i ? "," : "") + std::to_string(p[i]);
    return n ? out : std::string("-");
}

int main(int argc, char **argv) {
    auto u = [&](int i) { return strtoull(argv[i], nullptr, 10); };
    const std::string op = argc > 1 ? argv[1] : "";
    uint64_t work[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int rc = -100;
    if (op == "walk" && argc == 11) {
        const uint32_t ctx = (uint32_t)u(4), max_steps = (uint32_t)u(6);
        const bool left = u(7) != 0, optional = u(9) != 0;
        const counting_evaluator eval(argv[2], ctx, u(8) != 0, u(10));
        const batch b(lines_of(argv[3]));
        const size_t Q = b.off.size() - 1;
        auto ext = exactly<char>(Q * max_steps);
        auto steps = exactly<uint32_t>(Q);
        auto stop = exactly<uint8_t>(Q);
        auto support = exactly<uint32_t>(optional ? Q * max_steps : 0);
        auto last = exactly<uint64_t>(optional ? Q * 4 : 0);
        rc = walk_steps(eval, b.text.data(), b.off.data(), Q, ctx, u(5), max_steps, left, ext.get(), steps.get(), stop.get(),
                        optional ? support.get() : nullptr, optional ? last.get() : nullptr, work);
        for (size_t q = 0; rc == RSBWT_OK && q < Q; ++q) {
            if (!zero_past(&ext[q * max_steps], steps[q], max_steps) || (optional && !zero_past(&support[q * max_steps], steps[q], max_steps))) return 4;
            printf("%s %u %u %s %s\n", symbols(&ext[q * max_steps], steps[q]).c_str(), steps[q], stop[q],
                   joined(optional ? &support[q * max_steps] : nullptr, steps[q]).c_str(), joined(optional ? &last[q * 4] : nullptr, 4).c_str());
        }
    } else if (op == "unitigs" && argc == 9) {
        const uint32_t ctx = (uint32_t)u(4), max_steps = (uint32_t)u(6);
        const bool optional = u(8) != 0;
        const counting_evaluator eval(argv[2], ctx, u(7) != 0, 0);
        const batch b(lines_of(argv[3]));
        const size_t items = 2 * (b.off.size() - 1);
        auto ext = exactly<char>(items * max_steps);
        auto steps = exactly<uint32_t>(items);
        auto stop = exactly<uint8_t>(items);
        auto support = exactly<uint32_t>(optional ? items * max_steps : 0);
        auto last = exactly<uint64_t>(optional ? items * 8 : 0);
        rc = unitig_steps(eval, b.text.data(), b.off.data(), items / 2, ctx, u(5), max_steps, ext.get(), steps.get(), stop.get(),
                          optional ? support.get() : nullptr, optional ? last.get() : nullptr, work);
        for (size_t i = 0; rc == RSBWT_OK && i < items; ++i) {
            if (!zero_past(&ext[i * max_steps], steps[i], max_steps) || (optional && !zero_past(&support[i * max_steps], steps[i], max_steps))) return 4;
            printf("%s %u %u %s %s\n", symbols(&ext[i * max_steps], steps[i]).c_str(), steps[i], stop[i],
                   joined(optional ? &support[i * max_steps] : nullptr, steps[i]).c_str(), joined(optional ? &last[i * 8] : nullptr, 8).c_str());
        }
    } else if (op == "paths" && argc == 13) {
        const uint32_t ctx = (uint32_t)u(5), max_steps = (uint32_t)u(7), max_paths = (uint32_t)u(8), max_evals = (uint32_t)u(9);
        const bool left = u(10) != 0, optional = u(12) != 0, targets = strcmp(argv[4], "-") != 0;
        const counting_evaluator eval(argv[2], ctx, u(11) != 0, 0);
        const batch b(lines_of(argv[3])), t(targets ? lines_of(argv[4]) : std::vector<std::string>());
        const size_t Q = b.off.size() - 1, slots = Q * max_paths;
        if (targets && t.off.size() != Q + 1) return 2;
        auto ext = exactly<char>(slots * max_steps);
        auto steps = exactly<uint32_t>(slots);
        auto stop = exactly<uint8_t>(slots);
        auto least = exactly<uint32_t>(optional ? slots : 0);
        auto npaths = exactly<uint32_t>(Q);
        auto state = exactly<uint8_t>(Q);
        rc = paths_steps(eval, b.text.data(), b.off.data(), Q, targets ? t.text.data() : nullptr, targets ? t.off.data() : nullptr, ctx, u(6), max_steps,
                         max_paths, max_evals, left, ext.get(), steps.get(), stop.get(), optional ? least.get() : nullptr, npaths.get(), state.get(), work);
        for (size_t q = 0; rc == RSBWT_OK && q < Q; ++q) {
            const size_t used = (q * max_paths + npaths[q]) * max_steps;
            if (!zero_past(ext.get(), used, (q + 1) * max_paths * max_steps) || !zero_past(steps.get(), q * max_paths + npaths[q], (q + 1) * max_paths)) return 4;
            printf("%u %u\n", state[q], npaths[q]);
            for (size_t at = q * max_paths; at < q * max_paths + npaths[q]; ++at)
                printf("%s %u %u %s\n", symbols(&ext[at * max_steps], steps[at]).c_str(), steps[at], stop[at], joined(optional ? &least[at] : nullptr, 1).c_str());
        }
    } else {
        fprintf(stderr, "usage: graph_steps_host walk|unitigs|paths ... (see the head of graph_steps_host.cpp)\n");
        return 2;
    }
    if (rc != RSBWT_OK) {
        fprintf(stderr, "the loop returned %d\n", rc);
        return 3;
    }
    printf("work %llu %llu %llu\ngraph_steps ok\n", (unsigned long long)work[1], (unsigned long long)work[6], (unsigned long long)work[7]);
    return 0;
}
