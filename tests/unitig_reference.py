"""The unitig reference the unitig tests share -- TEST INFRASTRUCTURE, CPU only.  include/rsbwt.h's definition of
rsbwt_set_unitigs stated over walk_reference's `extensions` and `context`, for either side object (OracleSide over the
oracle's BWT, PlainSide with no BWT at all).

Every seed has two SIDES, 0 walking right from s[-ctx:] and 1 walking left from s[:ctx].  A side repeats: LIMIT at
max_steps symbols; the ONWARD evaluation, the walk's own step (none live: DEAD_END, two or more: BRANCH); for the one
live symbol c the RETURN evaluation of the node entered, in the opposite direction (two or more live: JOIN, c is not
appended); else c is appended.  The expected work: the onward and the return evaluations, the candidate searches =
evaluations x shards x 4 x strands, and the LF steps of those searches without a k-mer table
(walk_reference.search_steps)."""
from collections import namedtuple

import walk_reference as W
from kmer_reference import _rc

DEAD_END, BRANCH, LIMIT, INVALID, JOIN = W.DEAD_END, W.BRANCH, W.LIMIT, W.INVALID, 5
ACGT = W.ACGT
ZERO8 = (0,) * 8

# ext, stop, support, last (8), the string the side ended with, the strings evaluated onward (in the side's direction)
# and the nodes evaluated in return (in the opposite one)
Side = namedtuple("Side", ["ext", "stop", "support", "last", "final", "onward", "back"])


def seeds(ctx):
    """walk_reference's seeds, plus one whose N lies in the left context only: side 1 is INVALID and side 0 walks"""
    w = W.G.fixture().haps[1][200:260]
    return W.seeds(ctx) + [w[:5] + "N" + w[6:]]


def side_walk(side, seed, ctx, min_count, max_steps, left, both, shards=None):
    """one side of the unitig through `seed`"""
    m = max(min_count, 1)
    t, ext, sup, onward, back = seed, "", [], [], []
    if W.context(t, ctx, left) is None:
        return Side("", INVALID, (), ZERO8, t, (), ())

    def sums(s, to_left):
        return tuple(sum(col) for col in zip(*W.extensions(side, s, ctx, to_left, both, shards)))

    while True:
        if len(ext) == max_steps:
            return Side(ext, LIMIT, tuple(sup), ZERO8, t, tuple(onward), tuple(back))
        onward.append(W.context(t, ctx, left))
        on = sums(t, left)
        live = [b for b in range(4) if on[b] >= m]
        if len(live) != 1:
            return Side(ext, BRANCH if live else DEAD_END, tuple(sup), on + (0, 0, 0, 0), t, tuple(onward), tuple(back))
        c = ACGT[live[0]]
        t2 = c + t if left else t + c
        v = W.context(t2, ctx, left)  # the node entered
        back.append(v)
        ret = sums(v, not left)
        if sum(r >= m for r in ret) >= 2:
            return Side(ext, JOIN, tuple(sup), on + ret, t, tuple(onward), tuple(back))
        ext += c
        sup.append(min(on[live[0]], 2 ** 32 - 1))
        t = t2


def known(s, ctx, left):
    """the index of the return candidate that is known: b0 = t[-ctx] walking right, t[ctx - 1] walking left, of the
    string t the side stopped with"""
    return ACGT.index(s.final[ctx - 1] if left else s.final[-ctx])


_UNITIGS = {}


def unitigs(side, key, sds, ctx, min_count, max_steps, both, shards=None):
    """[(right, left)] of every seed, computed once per (key, parameters); key names the side and the seeds"""
    at = (key, ctx, min_count, max_steps, both, None if shards is None else tuple(shards))
    if at not in _UNITIGS:
        _UNITIGS[at] = [tuple(side_walk(side, s, ctx, min_count, max_steps, left, both, shards) for left in (False, True)) for s in sds]
    return _UNITIGS[at]


def sequence(seed, right_ext, left_ext):
    return left_ext[::-1] + seed + right_ext


def expected_work(side, us, both):
    """{onward, back, searches, lf_steps without a table, appended} of unitigs `us` over every shard of the side"""
    onward = back = searches = steps = appended = 0
    for pair in us:
        for left, s in zip((False, True), pair):
            onward += len(s.onward)
            back += len(s.back)
            appended += len(s.ext)
            for strings, to_left in ((s.onward, left), (s.back, not left)):
                for c in strings:
                    for x in W.candidates(c, to_left):
                        for y in ((x, _rc(x)) if both else (x,)):
                            for p in range(side.S):
                                searches += 1
                                steps += W.search_steps(side, p, y)
    return dict(onward=onward, back=back, searches=searches, lf_steps=steps, appended=appended)
