"""Inputs of the k-mer graph tests at the context lengths where the search and the rings change behaviour, and of the
paths tests beyond the gt fixture -- TEST INFRASTRUCTURE, CPU only.  tests/test_graph_context_reference.py shows on the CPU
what these inputs reach; tests/test_gpu_paths_streams.py and tests/test_gpu_graph_contexts.py run them on the GPU.  Every
expected value comes from walk_reference, unitig_reference or paths_reference over the oracle.

  * PATHS ON STREAMS: stream_reference's run streams and read sets, context 8, a wide and a tight set of limits, and
    targets derived from the reference's own paths (a run stream has no haplotype to take them from).
  * AROUND THE TABLE DEPTH: the gt read sets at candidate lengths K = ctx + 1 below, at and above a table depth T.
  * THE LARGEST CONTEXT: the `ragged` read set (reads of up to 600 symbols) at ctx 254 and 255, as it is in one shard
    and -- with a few seeded variants of its long reads, which make 256-mers fork -- dealt to two.
  * DENSE FORKS: the gt `plain` set at ctx 1, 2 and 3, where every node has four live successors."""
import random

import numpy as np

import gt_reference as G
import paths_reference as P
import stream_reference as R
import test_kmer_fixtures as F
import walk_reference as W
from kmer_reference import _bwt_runs, _rc

ACGT = W.ACGT

# ---- paths on streams ------------------------------------------------------------------------------------------------

CTX = 8
STREAM_WIDE = (16, 8, 128)   # (max_steps, max_paths, max_evals)
STREAM_TIGHT = (16, 2, 20)  # reaches MORE and BUDGET (tests/test_graph_context_reference.py counts them)
TARGET_LEN = min(CTX, 5)
STREAM_SETTINGS = [(both, m, left) for both in (False, True) for m in (1, 2) for left in (False, True)]

_STREAM_SIDES = {}


def stream_seeds(src):
    """the small batch, cut to its queries of at least CTX symbols"""
    return [w for w in R.queries(src, "small") if len(w) >= CTX]


def stream_side(srcs):
    """one oracle side per tuple of sources: the supports of a side's nodes are kept with it"""
    key = tuple(s.name for s in srcs)
    if key not in _STREAM_SIDES:
        _STREAM_SIDES[key] = W.OracleSide([s.orc for s in srcs])
    return _STREAM_SIDES[key]


def stream_searches(srcs, sds, tgs, m, limits, left, both):
    """paths_reference.searches over the sources' oracle side; tgs None = no targets"""
    key = ("streams",) + tuple(s.name for s in srcs) + (tuple(sds), None if tgs is None else tuple(tgs))
    return P.searches(stream_side(srcs), key, sds, tgs, CTX, m, limits, left, both)


def stream_targets(srcs, sds, left):
    """targets from the reference's own paths (min_count 1, one strand, the wide limits, no targets): of the valid seeds
    whose first path has at least 4 symbols every third has one -- the TARGET_LEN symbols at the walking end of seed +
    the first half of that path -- but every fourth seed of the batch keeps none, and the second target made holds an N
    (it never matches)"""
    ref = stream_searches(srcs, sds, None, 1, STREAM_WIDE, left, False)
    out, eligible, made = [], 0, 0
    for q, (s, r) in enumerate(zip(sds, ref)):
        t = ""
        if r.state != P.INVALID and r.paths and len(r.paths[0][0]) >= 4:
            if eligible % 3 == 0 and q % 4 != 0:
                half = r.paths[0][0][:len(r.paths[0][0]) // 2]
                seq = half[::-1] + s if left else s + half
                t = seq[:TARGET_LEN] if left else seq[len(seq) - TARGET_LEN:]
                made += 1
                if made == 2:
                    t = t[:2] + "N" + t[3:]
            eligible += 1
        out.append(t)
    return out


# ---- the read sets around the table depth and at dense forks -----------------------------------------------------------

TABLE_DEPTH = 6
CTXS_AT_6 = (1, 2, 4, 5, 6, 7)        # K < T three times, K == T, K > T twice
OTHER_DEPTHS = (3, 9)                  # ... with ctx = T - 1 only
WHOLE_READ_CTX = 39                    # K = 40: the candidate is a whole read of the gt fixture
DENSE_CTXS = (1, 2, 3)
DENSE_FULL = (4, 256, 1 << 20)         # every path of 4 symbols: 256 LIMIT paths after 85 evaluations, COMPLETE
# limits -> (state, paths) of a valid seed at min_count 1, right, one strand (None: not stated)
DENSE_LIMITS = {
    DENSE_FULL: (P.COMPLETE, 256),
    (4, 255, 1 << 20): (P.MORE, 255),
    (4, 256, 85): (P.COMPLETE, None),
    (4, 256, 84): (P.OUT_OF_BUDGET, 253),
    (6, 256, 4096): (P.MORE, 256),
    (64, 8, 3): (P.OUT_OF_BUDGET, None),
}

_SIDES = {}


def gt_side(oracle, name, S):
    """the oracle side of gt read set `name` dealt to S shards"""
    if (name, S) not in _SIDES:
        shards = [G.OracleShard(oracle.from_runs(r, len(sh))) for sh, r in zip(W.dealt(name, S), W.runs(name, S))]
        _SIDES[(name, S)] = W.OracleSide(shards)
    return _SIDES[(name, S)]


def table_starts_expected(T, ctx):
    """the general rule: a search starts from the table exactly when there is one and the candidate is no shorter than its
    depth"""
    return T > 0 and ctx + 1 >= T


# ---- the largest context -----------------------------------------------------------------------------------------------

LONG_CTXS = (254, 255)
LONG_MAX_STEPS = 300
LONG_LIMITS = (LONG_MAX_STEPS, 8, 1024)  # the wide limits at this length: no seed runs out of evaluations
TARGET_ON = 40                           # a target ends (begins) this many symbols past the seed in its read
LONG_TARGETS = (255, 12)                 # (a target is no longer than ctx: the long one has 254 symbols at ctx 254)
N_VARIANTS = 4

_LONG = {}


def _long():
    """the seeds at ctx 254 / 255 with the read and the place each was cut from, and the variants: copies of a seed's read
    with one symbol substituted 20 symbols past the seed (on either side), so that the 255- and 256-mers of the reads fork
    there and join again -- the ragged set's own long reads come from one genome and never do"""
    if _LONG:
        return _LONG
    fx = F.fixture("ragged")
    rng = random.Random("graph contexts/ragged")
    longs = sorted((r for r in fx.longs if len(r) >= 400), key=len)
    cut = []  # (read, at, length)
    # a left walk of more than 255 symbols from the two longest reads: the ring is crossed more than once
    for r in longs[-2:]:
        cut.append((r, len(r) - 300 - TARGET_ON, 300))
    for i in range(10):
        r = longs[rng.randrange(len(longs))]
        ln = rng.randint(300, min(400, len(r) - 2 * TARGET_ON))
        cut.append((r, rng.randint(TARGET_ON, len(r) - ln - TARGET_ON), ln))
    r = longs[3]
    cut += [(r, 60, 255), (r, 61, 254)]
    seeds = [r[at:at + ln] for r, at, ln in cut]
    w = seeds[2]
    inside = w[:5] + "N" + w[6:len(w) - 6] + "N" + w[len(w) - 5:]   # an N in either direction's context
    wide = longs[-3]
    assert len(wide) >= 2 * 255 + 20
    outside = wide[:len(wide) // 2] + "N" + wide[len(wide) // 2 + 1:]  # an N outside both contexts (valid)
    seeds += [inside, outside]
    cut += [(None, 0, 0), (wide, 0, len(wide))]
    variants = []
    for r, at, ln in cut[:N_VARIANTS]:
        for p in (at + ln + 20, at - 21):
            variants.append(r[:p] + rng.choice([c for c in ACGT if c != r[p]]) + r[p + 1:])
    _LONG.update(seeds=seeds, cut=cut, variants=variants)
    return _LONG


def long_seeds():
    """about a dozen substrings of 300 to 400 symbols of reads of at least 400, one of exactly 255 symbols, one of 254
    (INVALID at ctx 255), one with an N inside the context and one with an N outside it"""
    return list(_long()["seeds"])


def long_target_lens(ctx):
    return tuple(min(t, ctx) for t in LONG_TARGETS)


def long_targets(tlen, left):
    """per seed the tlen symbols that end (walking left: begin) TARGET_ON symbols past the seed in its own read; none where
    the read does not reach that far"""
    out = []
    for r, at, ln in _long()["cut"]:
        t = ""
        if r is not None:
            b = at - TARGET_ON if left else at + ln + TARGET_ON - tlen
            if 0 <= b and b + tlen <= len(r):
                t = r[b:b + tlen]
        out.append(t)
    return out


def long_reads(S):
    """S = 1: the ragged set as it is; S = 2: its reads and the variants, dealt round-robin"""
    reads = list(F.fixture("ragged").shards[0])
    if S == 1:
        return [reads]
    every = reads + _long()["variants"]
    return [every[p::S] for p in range(S)]


_LONG_RUNS = {}


def long_runs(S):
    if S not in _LONG_RUNS:
        _LONG_RUNS[S] = F.fixture("ragged").runs() if S == 1 else [_bwt_runs(sh) for sh in long_reads(S)]
    return _LONG_RUNS[S]


def long_side(oracle, S, rsb=None):
    """S = 1 is stream_reference's `ragged` source"""
    if ("long", S) not in _SIDES:
        if S == 1:
            shards = [R.source("ragged", oracle, rsb).orc]
        else:
            shards = [G.OracleShard(oracle.from_runs(r, len(sh))) for sh, r in zip(long_reads(S), long_runs(S))]
        _SIDES[("long", S)] = W.OracleSide(shards)
    return _SIDES[("long", S)]


# ---- LF steps of long candidates -----------------------------------------------------------------------------------------

_STEPS = {}


def oracle_steps(side, p, x):
    """walk_reference.search_steps from the oracle's own count of updateInterval calls: the same number on a shard that
    holds every base (tests/test_graph_context_reference.py), without a search per suffix -- a candidate of 256 symbols has
    255 of them"""
    if (id(side), p, x) not in _STEPS:
        st = side.shards[p].oix.find_intervals(np.frombuffer(x.encode(), np.uint8).reshape(1, -1), want_steps=True)[2]
        _STEPS[(id(side), p, x)] = int(st[0])
    return _STEPS[(id(side), p, x)]


def lf_steps(side, contexts, to_left, both, steps=W.search_steps):
    """(candidate searches, LF steps without a table) of the evaluations of `contexts` over every shard of the side; a
    context's own are kept with the side: dense graphs come through the same few nodes thousands of times"""
    memo = side.__dict__.setdefault("_context_work", {})
    n = total = 0
    for c in contexts:
        at = (c, to_left, both, steps)
        if at not in memo:
            ys = [y for x in W.candidates(c, to_left) for y in ((x, _rc(x)) if both else (x,))]
            memo[at] = (len(ys) * side.S, sum(steps(side, p, y) for y in ys for p in range(side.S)))
        n, total = n + memo[at][0], total + memo[at][1]
    return n, total
