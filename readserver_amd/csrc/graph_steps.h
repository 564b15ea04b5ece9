// graph_steps.h -- the k-mer graph calls of a set over several device groups, step by step on the host (include/rsbwt.h:
// the definitions): the walk (rsbwt_set_walk and rsbwt_set_walk_samples), the unitigs and the paths.  Plain C++ with no
// device in it, for set_graph.hip and, as a program of its own under the sanitizers, tests/native/graph_steps_host.cpp.
//
// Every loop is written over an EVALUATOR the caller passes in:
//     int eval(const std::vector<std::string> &ctxs, bool left, uint64_t *sums, uint8_t *wide)
// ctxs are n contexts of ctx symbols each, to be extended to the left or to the right; the evaluator fills sums[n][4], the
// supports of A, C, G, T already added over shards and strands, and -- where it has such a thing (a sample walk) -- sets
// wide[n]; both arrays come zeroed, so an evaluator may add into sums.  It returns an RSBWT code; anything but RSBWT_OK ends the loop, which hands it back.
// The loops decide with the rule headers the kernels decide with.  Of the work counters they add the appended symbols
// (work[1]) and the unitig and paths loops their evaluations and paths (work[6], work[7]); the rest is the evaluator's.
#ifndef RSBWT_GRAPH_STEPS_H
#define RSBWT_GRAPH_STEPS_H

#include <stdint.h>
#include <string.h>

#include <string>
#include <utility>
#include <vector>

#include "../../include/rsbwt.h"
#include "paths_rule.h"
#include "sample_walk_rule.h"
#include "unitig_rule.h"

namespace rsb {

// The context seed q is extended from: its first (left) or last ctx symbols.  False where it has fewer, or one outside ACGT.
inline bool seed_context(const char *text, const uint64_t *off, size_t q, uint32_t ctx, bool left, std::string *out) {
    if (off[q + 1] - off[q] < ctx) return false;
    out->assign(left ? text + off[q] : text + off[q + 1] - ctx, ctx);
    for (char ch : *out)
        if (ch != 'A' && ch != 'C' && ch != 'G' && ch != 'T') return false;
    return true;
}

// the context after "ACGT"[pick] has been put on the walking side
inline std::string context_advance(const std::string &c, uint32_t pick, bool left) {
    return left ? std::string(1, "ACGT"[pick]) + c.substr(0, c.size() - 1) : c.substr(1) + "ACGT"[pick];
}

// The walk: per step the seeds still walking are evaluated and sample_walk_step decides -- walk_kernel's decision and the
// sample walk's (a plain walk's evaluator never reports wide).  ext char[Q][max_steps], steps u32[Q], stop u8[Q], support
// u32[Q][max_steps] and last u64[Q][4] (both optional): last keeps the sums of the evaluation a seed stopped at, zeros at
// LIMIT and at WIDE.
template <class Eval>
int walk_steps(Eval &&eval, const char *text, const uint64_t *off, size_t Q, uint32_t ctx, uint64_t m, uint32_t max_steps, bool left, char *ext,
               uint32_t *steps, uint8_t *stop, uint32_t *support, uint64_t *last, uint64_t *work) {
    memset(ext, 0, Q * (size_t)max_steps);
    if (support) memset(support, 0, Q * (size_t)max_steps * 4);
    if (last) memset(last, 0, Q * 32);
    std::vector<size_t> live, next;  // the seeds still walking and, beside them, their contexts
    std::vector<std::string> ctxs, next_ctxs;
    for (size_t q = 0; q < Q; ++q) {
        std::string c;
        const bool valid = seed_context(text, off, q, ctx, left, &c);
        steps[q] = 0;
        stop[q] = valid ? 0 : (uint8_t)RSBWT_WALK_INVALID;
        if (!valid) continue;
        live.push_back(q);
        ctxs.push_back(std::move(c));
    }
    std::vector<uint64_t> sums;
    std::vector<uint8_t> wide;
    while (!live.empty()) {  // (every seed of `live` has fewer than max_steps symbols appended)
        const size_t nl = live.size();
        sums.assign(nl * 4, 0);
        wide.assign(nl, 0);
        const int rc = eval(ctxs, left, sums.data(), wide.data());
        if (rc) return rc;
        next.clear(), next_ctxs.clear();
        for (size_t i = 0; i < nl; ++i) {
            const size_t q = live[i];
            const uint64_t *sup = &sums[i * 4];
            uint32_t pick = 0;
            uint32_t why = sample_walk_step(sup, wide[i] != 0, m, &pick);
            if (why == SAMPLE_WALK_GO) {
                const size_t at = q * (size_t)max_steps + steps[q];
                ext[at] = "ACGT"[pick];
                if (support) support[at] = unitig_saturate(sup[pick]);
                work[1] += 1;
                if (++steps[q] < max_steps) {
                    next.push_back(q);
                    next_ctxs.push_back(context_advance(ctxs[i], pick, left));
                    continue;
                }
                why = SAMPLE_WALK_LIMIT;
            }
            stop[q] = (uint8_t)why;
            if (last && why != SAMPLE_WALK_LIMIT && why != SAMPLE_WALK_WIDE)
                for (int b = 0; b < 4; ++b) last[4 * q + b] = sup[b];
        }
        live.swap(next);
        ctxs.swap(next_ctxs);
    }
    return RSBWT_OK;
}

// The unitigs: item i = 2 * seed + side, side 1 walks left.  Per step the items still walking are evaluated ONWARD and
// unitig_rule.h's onward half decides; the nodes entered are then evaluated in RETURN, in the opposite direction, and the
// return half decides -- unitig_kernel's step.  An evaluation has one direction, so each of the two goes out as two calls,
// the right-walking items' and the left-walking ones'.  ext char[2Q][max_steps], steps u32[2Q], stop u8[2Q], support
// u32[2Q][max_steps] and last u64[2Q][8] (both optional).  work[6] += onward, work[7] += return evaluations.
template <class Eval>
int unitig_steps(Eval &&eval, const char *text, const uint64_t *off, size_t Q, uint32_t ctx, uint64_t m, uint32_t max_steps, char *ext,
                 uint32_t *steps, uint8_t *stop, uint32_t *support, uint64_t *last, uint64_t *work) {
    const size_t items = 2 * Q;
    memset(ext, 0, items * (size_t)max_steps);
    if (support) memset(support, 0, items * (size_t)max_steps * 4);
    if (last) memset(last, 0, items * 64);
    std::vector<std::string> cur(items);  // an item's context
    std::vector<size_t> live;
    for (size_t i = 0; i < items; ++i) {
        const bool valid = seed_context(text, off, i >> 1, ctx, (i & 1) != 0, &cur[i]);
        steps[i] = 0;
        stop[i] = valid ? 0 : (uint8_t)RSBWT_WALK_INVALID;
        if (valid) live.push_back(i);
    }
    // sums[k][0..3] of the strings str[k] of items `who`, in `who`'s own direction or the opposite one
    std::vector<std::string> part_str;
    std::vector<size_t> part;
    std::vector<uint64_t> part_sums;
    std::vector<uint8_t> wide;
    auto evaluate = [&](const std::vector<size_t> &who, const std::vector<std::string> &str, bool opposite, std::vector<uint64_t> &sums) -> int {
        sums.assign(who.size() * 4, 0);
        for (int side = 0; side < 2; ++side) {
            part.clear(), part_str.clear();
            for (size_t k = 0; k < who.size(); ++k)
                if ((int)(who[k] & 1) == side) {
                    part.push_back(k);
                    part_str.push_back(str[k]);
                }
            if (part.empty()) continue;
            part_sums.assign(part.size() * 4, 0);
            wide.assign(part.size(), 0);
            const int rc = eval(part_str, (side != 0) != opposite, part_sums.data(), wide.data());
            if (rc) return rc;
            for (size_t j = 0; j < part.size(); ++j) memcpy(&sums[part[j] * 4], &part_sums[j * 4], 32);
        }
        return RSBWT_OK;
    };
    std::vector<uint64_t> onward, back;
    std::vector<size_t> tent, tent_at, next;
    std::vector<std::string> ctxs, nodes;
    std::vector<uint32_t> picks;
    while (!live.empty()) {  // (every item of `live` has fewer than max_steps symbols appended)
        const size_t nl = live.size();
        ctxs.clear();
        for (size_t i : live) ctxs.push_back(cur[i]);
        int rc = evaluate(live, ctxs, false, onward);
        if (rc) return rc;
        work[6] += nl;
        tent.clear(), tent_at.clear(), nodes.clear(), picks.clear(), next.clear();
        for (size_t k = 0; k < nl; ++k) {
            const size_t i = live[k];
            uint32_t pick = 0;
            const uint32_t why = unitig_onward(&onward[k * 4], m, steps[i], max_steps, &pick);
            if (why != UNITIG_GO) {
                stop[i] = (uint8_t)why;
                if (last)
                    for (int c = 0; c < 4; ++c) last[8 * i + c] = onward[k * 4 + c];
                continue;
            }
            tent.push_back(i);
            tent_at.push_back(k);
            picks.push_back(pick);
            nodes.push_back(context_advance(cur[i], pick, (i & 1) != 0));
        }
        if (tent.empty()) break;  // (every item stopped)
        if ((rc = evaluate(tent, nodes, true, back)) != RSBWT_OK) return rc;
        work[7] += tent.size();
        for (size_t k = 0; k < tent.size(); ++k) {
            const size_t i = tent[k];
            const uint64_t *on = &onward[tent_at[k] * 4];
            if (unitig_return(&back[k * 4], m) != UNITIG_GO) {
                stop[i] = (uint8_t)RSBWT_WALK_JOIN;
                if (last)
                    for (int c = 0; c < 4; ++c) last[8 * i + c] = on[c], last[8 * i + 4 + c] = back[k * 4 + c];
                continue;
            }
            const size_t at = i * (size_t)max_steps + steps[i];
            ext[at] = "ACGT"[picks[k]];
            if (support) support[at] = unitig_saturate(on[picks[k]]);
            work[1] += 1;
            cur[i] = nodes[k];
            if (++steps[i] == max_steps) stop[i] = (uint8_t)RSBWT_WALK_LIMIT;
            else next.push_back(i);
        }
        live.swap(next);
    }
    return RSBWT_OK;
}

// The paths: per round the current node of every seed still searching is evaluated and the writer lane's decisions are
// taken with paths_rule.h -- paths_kernel's round.  tt / trel: the targets, trel null = none.  ext char[Q][max_paths]
// [max_steps], steps u32[Q][max_paths], stop u8[Q][max_paths], min_support u32[Q][max_paths] (optional), npaths u32[Q],
// state u8[Q].  work[6] += evaluations, work[7] += paths.
template <class Eval>
int paths_steps(Eval &&eval, const char *text, const uint64_t *off, size_t Q, const char *tt, const uint64_t *trel, uint32_t ctx, uint64_t m,
                uint32_t max_steps, uint32_t max_paths, uint32_t max_evals, bool left, char *ext, uint32_t *steps, uint8_t *stop, uint32_t *min_support,
                uint32_t *npaths, uint8_t *state, uint64_t *work) {
    const size_t slots = Q * (size_t)max_paths;
    memset(ext, 0, slots * max_steps);
    memset(steps, 0, slots * 4);
    memset(stop, 0, slots);
    if (min_support) memset(min_support, 0, slots * 4);
    struct search {
        std::string seed_ctx, path, target;
        std::vector<paths_frame> frames;
        uint32_t nframes = 0, evals = 0, min_cur = PATHS_NO_SUPPORT;
    };
    std::vector<search> st(Q);
    // the ctx symbols at the walking end of seed + path (reverse(path) + seed)
    auto context = [&](const search &a) {
        if (left) return (std::string(a.path.rbegin(), a.path.rend()) + a.seed_ctx).substr(0, ctx);
        const std::string all = a.seed_ctx + a.path;
        return all.substr(all.size() - ctx);
    };
    auto at_target = [&](const search &a) {
        if (a.target.empty()) return false;
        const std::string c = context(a);
        return left ? c.compare(0, a.target.size(), a.target) == 0 : c.compare(ctx - a.target.size(), a.target.size(), a.target) == 0;
    };
    std::vector<size_t> live, next;
    for (size_t q = 0; q < Q; ++q) {
        const bool valid = seed_context(text, off, q, ctx, left, &st[q].seed_ctx);
        npaths[q] = 0;
        state[q] = valid ? 0 : (uint8_t)PATHS_INVALID;
        if (!valid) continue;
        if (trel) st[q].target.assign(tt + trel[q], (size_t)(trel[q + 1] - trel[q]));
        st[q].frames.resize(paths_frames(max_steps, max_evals));
        live.push_back(q);
    }
    std::vector<std::string> ctxs;
    std::vector<uint64_t> sums;
    std::vector<uint8_t> wide;
    while (!live.empty()) {  // (every seed of `live` has a node to evaluate: its end test said so)
        const size_t nl = live.size();
        ctxs.clear();
        for (size_t q : live) ctxs.push_back(context(st[q]));
        sums.assign(nl * 4, 0);
        wide.assign(nl, 0);
        const int rc = eval(ctxs, left, sums.data(), wide.data());
        if (rc) return rc;
        next.clear();
        for (size_t i = 0; i < nl; ++i) {
            const size_t q = live[i];
            search &a = st[q];
            const uint64_t *sup = &sums[i * 4];
            ++a.evals;
            work[6] += 1;
            const uint32_t mask = paths_live(sup, m);
            uint32_t why = PATHS_DEAD_END;
            if (mask != 0u) {
                a.path += "ACGT"[paths_advance(a.frames.data(), &a.nframes, (uint32_t)a.path.size(), mask, sup, &a.min_cur)];
                work[1] += 1;
                why = paths_end(at_target(a), (uint32_t)a.path.size(), max_steps, a.evals, max_evals);
            }
            bool searching = true;
            while (why != PATHS_GO) {  // (max_paths times at the most: every turn puts a path out)
                const size_t at = q * (size_t)max_paths + npaths[q];
                memcpy(ext + at * max_steps, a.path.data(), a.path.size());
                steps[at] = (uint32_t)a.path.size();
                stop[at] = (uint8_t)why;
                if (min_support) min_support[at] = paths_min_out((uint32_t)a.path.size(), a.min_cur);
                ++npaths[q];
                work[7] += 1;
                const uint32_t done = paths_done(why, a.nframes, npaths[q], max_paths);
                if (done != PATHS_GO) {
                    state[q] = (uint8_t)done;
                    searching = false;
                    break;
                }
                uint32_t d = 0;
                const uint32_t c = paths_backtrack(a.frames.data(), &a.nframes, &d, &a.min_cur);
                a.path.resize(d);
                a.path += "ACGT"[c];
                work[1] += 1;
                why = paths_end(at_target(a), (uint32_t)a.path.size(), max_steps, a.evals, max_evals);
            }
            if (searching) next.push_back(q);
        }
        live.swap(next);
    }
    return RSBWT_OK;
}

}  // namespace rsb
#endif
