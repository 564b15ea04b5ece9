"""The paths reference the paths tests share -- TEST INFRASTRUCTURE, CPU only.  include/rsbwt.h's definition of
rsbwt_set_paths, its pseudocode line by line, over walk_reference's `extensions` for either side object (OracleSide over the
oracle's BWT, PlainSide with no BWT at all).

A seed's search goes depth first through the forks, A before C before G before T.  A path ends at its target (TARGET, not
looked at before the first symbol), at max_steps symbols (LIMIT), when the seed's evaluations have run out (BUDGET) or
where no symbol is live (DEAD_END); after a path the seed is done for BUDGET, then when no fork is pending (COMPLETE), then
at max_paths paths (MORE); else the deepest pending fork gives its first untried symbol.

The inputs are the walk tests' read sets and seeds.  The targets lie 30 symbols past the seed on haplotype 1, min(ctx, 12)
symbols long; the seeds after the windows have none, window 3's holds an N (it never matches) and window 5 has none.  The
expected work: the evaluations, the candidate searches = evaluations x shards x 4 x strands, the LF steps of those searches
without a k-mer table (walk_reference.search_steps), the appended symbols (the first live symbol of an evaluation and the
symbol a backtrack takes up) and the paths."""
from collections import namedtuple

import walk_reference as W
from kmer_reference import _rc

DEAD_END, LIMIT, TARGET, BUDGET = W.DEAD_END, W.LIMIT, 6, 7
COMPLETE, MORE, OUT_OF_BUDGET, INVALID = 1, 2, 3, 4
ACGT = W.ACGT
WIDE = (64, 8, 256)    # (max_steps, max_paths, max_evals)
TIGHT = (64, 3, 40)    # reaches MORE and BUDGET (tests/test_paths_reference.py counts them)
TARGET_PAST = 30
SAT = 2 ** 32 - 1

# a seed's search: state, [(ext, stop, min_support)], the strings evaluated in order, and per backtrack (the depth gone
# back to, the depth of the fork met last before it)
Search = namedtuple("Search", ["state", "paths", "evaluated", "backtracks"])


def targets(ctx, left):
    """one target per seed of W.seeds(ctx)"""
    g = W.G.fixture().haps[1]
    T = min(ctx, 12)
    out = []
    for i in range(W.N_PLAIN):
        at = i * W.SEED_STRIDE
        b = at - TARGET_PAST if left else at + W.SEED_LEN + TARGET_PAST - T
        out.append(g[b:b + T] if 0 <= b and b + T <= len(g) else "")
    out[3] = out[3][:2] + "N" + out[3][3:] if out[3] else ""
    out[5] = ""
    return out + [""] * (len(W.seeds(ctx)) - W.N_PLAIN)


def supports(side, c, left, both, shards=None):
    """the four supports of a string whose context is c; kept per side, because the searches of a side -- the limits, the
    targets, overlapping seeds -- come through the same nodes again and again"""
    memo = side.__dict__.setdefault("_paths_supports", {})
    key = (c, left, both, None if shards is None else tuple(shards))
    if key not in memo:
        memo[key] = tuple(sum(col) for col in zip(*W.extensions(side, c, len(c), left, both, shards)))
    return memo[key]


def _node_work(side, c, left, both):
    """(candidate searches, LF steps without a table) of one evaluation of context c over every shard; kept per side"""
    memo = side.__dict__.setdefault("_paths_work", {})
    if (c, left, both) not in memo:
        n = steps = 0
        for x in W.candidates(c, left):
            for y in ((x, _rc(x)) if both else (x,)):
                for p in range(side.S):
                    n += 1
                    steps += W.search_steps(side, p, y)
        memo[(c, left, both)] = (n, steps)
    return memo[(c, left, both)]


def search(side, seed, target, ctx, min_count, max_steps, max_paths, max_evals, left, both, shards=None):
    """the search of one seed over a side's supports"""
    g = search_by_rounds(seed, target, ctx, min_count, max_steps, max_paths, max_evals, left)
    try:
        c = next(g)
        while True:
            c = g.send(supports(side, c, left, both, shards))
    except StopIteration as done:
        return done.value


def search_by_rounds(seed, target, ctx, min_count, max_steps, max_paths, max_evals, left):
    """the definition as a generator: yields the context of every string it evaluates, is sent that string's four supports,
    and returns the Search -- so that whoever drives it decides where the supports come from"""
    m = max(min_count, 1)
    if W.context(seed, ctx, left) is None:
        return Search(INVALID, (), (), ())
    path, pend, evals, out = "", {}, 0, []
    sups, evaluated, backs, last_fork = [], [], [], None
    while True:
        seq = path[::-1] + seed if left else seed + path
        end = seq[:len(target)] if left else seq[len(seq) - len(target):]
        if target and len(path) >= 1 and end == target:
            stop = TARGET
        elif len(path) == max_steps:
            stop = LIMIT
        elif evals == max_evals:
            stop = BUDGET
        else:
            evals += 1
            evaluated.append(W.context(seq, ctx, left))
            tot = yield evaluated[-1]
            live = [c for c in range(4) if tot[c] >= m]
            if not live:
                stop = DEAD_END
            else:
                if live[1:]:
                    pend[len(path)] = (live[1:], tot, list(sups))
                    last_fork = len(path)
                path += ACGT[live[0]]
                sups.append(min(tot[live[0]], SAT))
                continue
        out.append((path, stop, min(sups) if sups else 0))
        if stop == BUDGET:
            return Search(OUT_OF_BUDGET, tuple(out), tuple(evaluated), tuple(backs))
        if not pend:
            return Search(COMPLETE, tuple(out), tuple(evaluated), tuple(backs))
        if len(out) == max_paths:
            return Search(MORE, tuple(out), tuple(evaluated), tuple(backs))
        d = max(pend)
        untried, tot, before = pend[d]
        c = untried.pop(0)
        if not untried:
            del pend[d]
        backs.append((d, last_fork))
        path = path[:d] + ACGT[c]
        sups = before + [min(tot[c], SAT)]


_SEARCHES = {}


def searches(side, key, sds, tgs, ctx, min_count, limits, left, both, shards=None):
    """the searches of every seed, computed once per (key, parameters); key names the side, the seeds and the targets;
    tgs None = no targets"""
    at = (key, ctx, min_count, limits, left, both, None if shards is None else tuple(shards))
    if at not in _SEARCHES:
        _SEARCHES[at] = [search(side, s, t, ctx, min_count, limits[0], limits[1], limits[2], left, both, shards)
                         for s, t in zip(sds, tgs or [""] * len(sds))]
    return _SEARCHES[at]


def expected_work(side, ss, left, both):
    """{evals, paths, appended, searches, lf_steps without a table} of searches `ss` over every shard of the side"""
    evals = paths = appended = n = steps = 0
    for s in ss:
        evals += len(s.evaluated)
        paths += len(s.paths)
        # every evaluation but those that found nothing live appended a symbol, and so did every backtrack
        appended += len(s.evaluated) - sum(p[1] == DEAD_END for p in s.paths) + len(s.backtracks)
        for c in s.evaluated:
            a, b = _node_work(side, c, left, both)
            n += a
            steps += b
    return dict(evals=evals, paths=paths, appended=appended, searches=n, lf_steps=steps)
