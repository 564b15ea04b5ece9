"""CPU suite: the inputs of tests/test_gpu_paths_streams.py and tests/test_gpu_graph_contexts.py (tests/graph_context_reference.py)
reach what those files rely on, shown with the references alone.  Walks, unitigs and paths over the oracle's BWT equal
those with no BWT at all at every context length the GPU file runs, candidates of 2 and of 256 symbols included; the
dense limits give the literal outcomes the GPU cases are named after and fill the reference's frame stack to exactly
min(max_steps, max_evals); the stream inputs reach every seed state and every stop, backtracks past the last fork, the
wrapped interval of the '$'-less stream and TARGET stops of the derived targets; at ctx 254 and 255 a walk crosses the
ring more than once, a search backtracks above depth 0 and both target lengths are met.  These are conditions on the
inputs, not measurements."""
from collections import Counter

import pytest

import graph_context_reference as X
import paths_reference as P
import stream_reference as R
import unitig_reference as U
import walk_reference as W
from kmer_reference import _rc

GT_CTXS = sorted(set(X.CTXS_AT_6) | {T - 1 for T in X.OTHER_DEPTHS} | set(X.DENSE_CTXS))
DIRECTIONS = [(left, both) for left in (False, True) for both in (False, True)]


@pytest.fixture(scope="module")
def sides(oracle):
    """{set name: (OracleSide, PlainSide)} over the two shards as they are"""
    return {name: (X.gt_side(oracle, name, 2), W.PlainSide(reads)) for name, reads in W.read_sets().items()}


def _three(side, key, sds, ctx, m, left, both, limits=P.WIDE, tgs=None, max_steps=W.MAX_STEPS):
    """walks, unitigs (once per strand setting: they walk both ways) and paths of the seeds over a side"""
    return (W.walks(side, key, sds, ctx, m, max_steps, left, both),
            U.unitigs(side, key, sds, ctx, m, max_steps, both) if not left else None,
            P.searches(side, key + (tgs is not None,), sds, tgs, ctx, m, limits, left, both))


@pytest.mark.parametrize("name,ctx", [(name, ctx) for name in ("plain", "stranded") for ctx in GT_CTXS] + [("plain", X.WHOLE_READ_CTX)])
def test_the_two_statements_agree_at_every_context(sides, name, ctx):
    sds = W.seeds(ctx)
    assert [len(s) for s in sds[W.N_PLAIN:]] == [ctx - 1, 60, 60, 0, ctx]
    for m in (1, 2):
        for left, both in DIRECTIONS:
            a = _three(sides[name][0], (name, "contexts", 0), sds, ctx, m, left, both)
            b = _three(sides[name][1], (name, "contexts", 1), sds, ctx, m, left, both)
            assert a == b, (name, ctx, m, left, both)


def _pending_most(side, seed, ctx, limits, left=False, both=False):
    """(the most entries the reference's frame stack `pend` ever holds, the Search): the stack grows only where an
    evaluation finds two or more live symbols, so its size is looked at as every evaluation's supports go in"""
    g = P.search_by_rounds(seed, "", ctx, 1, limits[0], limits[1], limits[2], left)
    most = 0
    try:
        c = next(g)
        while True:
            tot = P.supports(side, c, left, both)
            most = max(most, len(g.gi_frame.f_locals["pend"]) + (sum(t >= 1 for t in tot) >= 2))
            c = g.send(tot)
    except StopIteration as done:
        return most, done.value


@pytest.mark.parametrize("ctx", X.DENSE_CTXS)
def test_dense_forks_give_the_literal_outcomes(sides, ctx):
    """min_count 1, right, one strand: every node has four live successors, so the outcomes are those of a full 4-ary tree"""
    orc, plain = sides["plain"]
    sds = W.seeds(ctx)
    valid = [q for q, s in enumerate(sds) if W.context(s, ctx, False) is not None]
    assert len(valid) >= 55
    for limits, (state, npaths) in X.DENSE_LIMITS.items():
        a = P.searches(orc, ("plain", "dense", 0), sds, None, ctx, 1, limits, False, False)
        b = P.searches(plain, ("plain", "dense", 1), sds, None, ctx, 1, limits, False, False)
        assert a == b, (ctx, limits)
        for q in valid:
            s = a[q]
            assert s.state == state and (npaths is None or len(s.paths) == npaths), (ctx, limits, q, s.state, len(s.paths))
            stops = Counter(p[1] for p in s.paths)
            if limits == X.DENSE_FULL:
                assert stops == {P.LIMIT: 256} and len(s.evaluated) == 85 and len({p[0] for p in s.paths}) == 256
            if limits == (4, 256, 85):
                assert len(s.paths) == 256 and len(s.evaluated) == 85
            if limits == (4, 256, 84):
                assert stops == {P.LIMIT: 252, P.BUDGET: 1} and len(s.evaluated) == 84
            if limits == (64, 8, 3):
                assert len(s.evaluated) == 3 and [p[1] for p in s.paths] == [P.BUDGET]
    # the frame store is full in the first and the last row: min(max_steps, max_evals) frames
    for limits in (X.DENSE_FULL, (64, 8, 3)):
        for q in valid[:12] + valid[-2:]:
            most, s = _pending_most(plain, sds[q], ctx, limits)
            assert most == min(limits[0], limits[2]), (ctx, limits, q, most)
            assert s == P.searches(plain, ("plain", "dense", 1), sds, None, ctx, 1, limits, False, False)[q]
    # the other directions and strands are compared on the GPU whatever they give: here the two statements agree on them
    for left, both in DIRECTIONS[1:]:
        for limits in X.DENSE_LIMITS:
            a = P.searches(orc, ("plain", "dense", 0), sds, None, ctx, 1, limits, left, both)
            b = P.searches(plain, ("plain", "dense", 1), sds, None, ctx, 1, limits, left, both)
            assert a == b, (ctx, limits, left, both)


def test_the_oracle_counts_the_steps_of_a_search(sides, oracle):
    """graph_context_reference.oracle_steps is walk_reference.search_steps on shards that hold every base: on candidates
    that are there, that die early and that die at the last symbol, at lengths 2, 6, 8 and 40"""
    orc = sides["plain"][0]
    n = 0
    for ctx in (1, 5, 7, 39):
        for s in W.seeds(ctx)[:20]:
            c = W.context(s, ctx, False)
            for x in W.candidates(c, False) + W.candidates(c, True):
                for y in (x, _rc(x)):
                    for p in range(orc.S):
                        assert X.oracle_steps(orc, p, y) == W.search_steps(orc, p, y), (ctx, y, p)
                        n += 1
    assert n >= 2000


@pytest.fixture(scope="module")
def stream_runs(oracle, rsb):
    """per stream name: {(both, m, left, variant): searches}, variant one of "wide", "tight", "targets", and the targets"""
    out = {}
    for name in R.STREAMS + R.FIXTURES:
        src = R.source(name, oracle, rsb)
        sds = X.stream_seeds(src)
        runs, tgs = {}, {}
        for both, m, left in X.STREAM_SETTINGS:
            tgs[left] = X.stream_targets([src], sds, left)
            runs[(both, m, left, "wide")] = X.stream_searches([src], sds, None, m, X.STREAM_WIDE, left, both)
            runs[(both, m, left, "tight")] = X.stream_searches([src], sds, None, m, X.STREAM_TIGHT, left, both)
            runs[(both, m, left, "targets")] = X.stream_searches([src], sds, tgs[left], m, X.STREAM_WIDE, left, both)
        out[name] = (src, sds, runs, tgs)
    return out


def test_the_stream_inputs_reach_every_class(stream_runs):
    states, stops, tight = Counter(), Counter(), Counter()
    past_fork, with_target = Counter(), 0
    for name, (src, sds, runs, tgs) in stream_runs.items():
        assert len(sds) >= 9
        hits = 0
        for left in (False, True):
            made = [t for t in tgs[left] if t]
            assert all(len(t) == X.TARGET_LEN for t in made) and all(not t for t in tgs[left][::4])
            if len(made) >= 2:
                assert sum("N" in t for t in made) == 1
        for (both, m, left, variant), ss in runs.items():
            for s in ss:
                states[s.state] += 1
                stops.update(p[1] for p in s.paths)
                past_fork[name] += sum(d != f for d, f in s.backtracks)
                if variant == "tight":
                    tight[s.state] += 1
                if variant == "targets":
                    hits += sum(p[1] == P.TARGET for p in s.paths)
                else:
                    assert all(p[1] != P.TARGET for p in s.paths)
        with_target += hits >= 1
    print(dict(states), dict(stops), dict(tight), dict(past_fork), with_target)
    assert all(states[s] >= 20 for s in (P.COMPLETE, P.MORE, P.OUT_OF_BUDGET, P.INVALID)), states
    assert all(stops[s] >= 20 for s in (P.DEAD_END, P.LIMIT, P.TARGET, P.BUDGET)), stops
    assert tight[P.MORE] >= 20 and tight[P.OUT_OF_BUDGET] >= 20, tight
    assert sum(past_fork.values()) >= 20 and all(past_fork[name] >= 1 for name in R.FIXTURES), past_fork
    assert 2 * with_target >= len(stream_runs), with_target


def test_the_dollarless_stream_leaves_the_proper_rows(stream_runs):
    """evaluated candidates whose search leaves the proper rows: a step by A from rows that see no A before them ends the
    oracle's findInterval on the wrapped interval (0, 2^64 - 1), which counts 0 rows.  (The first step of a candidate of 9
    symbols starts from all the rows of its last symbol and cannot: here it is the last, after a table start would end.)"""
    src, sds, runs, _ = stream_runs["nodollar"]
    side = X.stream_side([src])
    wrapped = at_last = 0
    for (both, m, left, variant), ss in runs.items():
        if variant != "wide" or m != 1:
            continue
        for c in {c for s in ss for c in s.evaluated}:
            for x in W.candidates(c, left):
                for y in ((x, _rc(x)) if both else (x,)):
                    iv = src.orc.find(y)
                    if iv[0] == 0 and iv[1] == 2 ** 64 - 1:
                        wrapped += 1
                        at_last += X.oracle_steps(side, 0, y) == X.CTX
                        assert side.W(0, y) == 0
    print(wrapped, at_last)
    assert wrapped >= 10 and at_last >= 10


@pytest.fixture(scope="module")
def long_sides(oracle, rsb):
    return {S: (X.long_side(oracle, S, rsb), W.PlainSide(X.long_reads(S))) for S in (1, 2)}


def test_the_long_seeds_are_what_they_are_named():
    sds = X.long_seeds()
    lens = [len(s) for s in sds]
    assert len(sds) == 16 and all(300 <= n <= 400 for n in lens[:12]) and lens[12:14] == [255, 254]
    for ctx in X.LONG_CTXS:
        valid = [W.context(s, ctx, left) is not None for s in sds for left in (False, True)]
        # the seed of 254 symbols is INVALID at 255 alone; an N inside either context; an N outside both
        assert valid == [True] * 26 + [ctx == 254] * 2 + [False, False, True, True], (ctx, valid)
    assert X.long_target_lens(254) == (254, 12) and X.long_target_lens(255) == (255, 12)
    for tlen in (254,) + X.LONG_TARGETS:
        for left in (False, True):
            tgs = X.long_targets(tlen, left)
            assert len(tgs) == len(sds) and sum(len(t) == tlen for t in tgs) >= 12 and all(len(t) in (0, tlen) for t in tgs)
    assert len(X.long_reads(1)) == 1 and len(X.long_reads(2)) == 2
    assert sum(len(sh) for sh in X.long_reads(2)) == len(X.long_reads(1)[0]) + 2 * X.N_VARIANTS


@pytest.mark.parametrize("S", [1, 2])
@pytest.mark.parametrize("ctx", X.LONG_CTXS)
def test_the_largest_contexts(long_sides, ctx, S):
    """K = 255 and 256: the two statements agree, and the inputs reach a walk that crosses the ring more than once, a
    backtrack above depth 0 (two shards: the variants fork) and TARGET stops of both target lengths"""
    orc, plain = long_sides[S]
    sds = X.long_seeds()
    longest = deep_backtracks = 0
    targets = Counter()
    for left, both in DIRECTIONS:
        a = _three(orc, ("long", S, 0), sds, ctx, 1, left, both, X.LONG_LIMITS, None, X.LONG_MAX_STEPS)
        b = _three(plain, ("long", S, 1), sds, ctx, 1, left, both, X.LONG_LIMITS, None, X.LONG_MAX_STEPS)
        assert a == b, (ctx, S, left, both)
        longest = max(longest, max(len(w.ext) for w in a[0]))
        assert all(len(s.evaluated) < X.LONG_LIMITS[2] for s in a[2])
        for tlen in X.long_target_lens(ctx):
            tgs = X.long_targets(tlen, left)
            ta = P.searches(orc, ("long", S, 0, tlen), sds, tgs, ctx, 1, X.LONG_LIMITS, left, both)
            tb = P.searches(plain, ("long", S, 1, tlen), sds, tgs, ctx, 1, X.LONG_LIMITS, left, both)
            assert ta == tb, (ctx, S, left, both, tlen)
            targets[tlen] += sum(p[1] == P.TARGET for s in ta for p in s.paths)
            deep_backtracks += sum(any(d > 0 for d, _ in s.backtracks) for s in ta)
        deep_backtracks += sum(any(d > 0 for d, _ in s.backtracks) for s in a[2])
    print(ctx, S, longest, deep_backtracks, dict(targets))
    assert all(targets[tlen] >= 1 for tlen in X.long_target_lens(ctx)), targets
    if S == 1:
        assert longest > 255, longest
    else:
        assert deep_backtracks >= 1
