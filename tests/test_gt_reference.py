"""CPU guards for the SiteMatch tests: tests/gt_reference.py (find_gt_reads restated over the oracle's BWT) against a
second computation that uses NO BWT, and the coverage of the inputs tests/test_gpu_gt.py runs on the GPU.

The second computation takes the leg rules as the issue states them -- "the smallest c >= 1 with W <= M" -- not the
reference's loops: W(x) is the number of occurrences of x in the plain read list (str.find), the rows of x and their
prefix / postfix lengths come from the suffix sort of the reads (kmer_reference.suffix_rows).  An empty interval has no
rows there and its (lower, upper) depend on the step the BWT search died at, so empty legs are compared by (a, b) and
width only."""
import bisect
from collections import Counter

import pytest

import gt_reference as G
from kmer_reference import suffix_rows


class PlainShard:
    def __init__(self, reads):
        self.reads = reads
        self.table = suffix_rows(reads)
        tr = str.maketrans("ACGT", "BCDE")
        self.tr = tr
        self.keys = [reads[i][j:].translate(tr) + "$" for i, j in self.table]
        assert self.keys == sorted(self.keys)
        self.start = {i: r for r, (i, j) in enumerate(self.table) if j == 0}

    def W(self, x):
        if not x or set(x) - set("ACGT"):
            return 0
        n = 0
        for r in self.reads:
            j = r.find(x)
            while j >= 0:
                n += 1
                j = r.find(x, j + 1)
        return n

    def rows(self, x):
        t = x.translate(self.tr)
        lo, up = bisect.bisect_left(self.keys, t), bisect.bisect_left(self.keys, t + "\x7f")
        assert up - lo == self.W(x)
        return range(lo, up)


def legs_by_rule(sh, w, pos, k, skip, M):
    """[(tile, leg, a, b, width)] and {read string} of one query by the issue's rules"""
    legs, reads = [], set()
    L = len(w)
    if k <= 0 or skip < 0 or L < k or pos > L:
        return legs, reads
    W = lambda a, b: sh.W(w[a:b])
    for i in range((L - k) // (skip + 1) + 1):
        s0 = (skip + 1) * i
        e0 = s0 + k
        if set(w[s0:e0]) - set("ACGT"):
            continue
        side = "left" if pos > e0 else "right" if pos <= s0 else "cover"
        mine = []
        if W(s0, e0) <= M:
            mine.append((0, s0, e0))
        else:
            grow_right = next(((s0, b) for b in range(e0 + 1, L + 1) if W(s0, b) <= M), None)
            grow_left = next(((a, e0) for a in range(s0 - 1, -1, -1) if W(a, e0) <= M), None)
            if side == "left":
                second = None
                if s0 > 0:  # left while a > 0, then right
                    second = grow_left or next(((0, b) for b in range(e0 + 1, L + 1) if W(0, b) <= M), None)
                first = grow_right
            elif side == "right":
                second = None
                if e0 < L:  # right while b < L, then left
                    second = grow_right or next(((a, L) for a in range(s0 - 1, -1, -1) if W(a, L) <= M), None)
                first = grow_left
            else:
                first, second = grow_right, grow_left
            mine += [(lg, x[0], x[1]) for lg, x in ((1, first), (2, second)) if x is not None]
        for lg, a, b in mine:
            legs.append((i, lg, a, b, W(a, b)))
            for r in sh.rows(w[a:b]):
                ri, off = sh.table[r]
                read = sh.reads[ri]
                if side == "left" and ((pos - b) & G.U64) > (len(read) - off - k) + 4:
                    continue
                if side == "right" and ((a + 1 - pos) & G.U64) > off + 4:
                    continue
                reads.add(read)
    return legs, reads


@pytest.fixture(scope="module")
def sides(oracle):
    fx = G.fixture()
    orc = [G.OracleShard(oracle.from_runs(r, len(sh))) for sh, r in zip(fx.shards, fx.runs())]
    return fx, orc, [PlainShard(sh) for sh in fx.shards]


@pytest.mark.parametrize("M,k,skip", G.PARAMS)
def test_restatement_agrees_with_the_computation_without_a_bwt(sides, M, k, skip):
    fx, orc, plain = sides
    qs = fx.queries()
    exp = G.expected(orc, "fixture", qs, k, skip, M)
    some = 0
    for q, (w, pos) in enumerate(qs):
        for p in range(2):
            legs, reads = exp[q][p]
            rl, rr = legs_by_rule(plain[p], w, pos, k, skip, M)
            width = lambda lo, up: (up - lo + 1) & G.U64
            assert [(t, lg, a, b, width(lo, up)) for t, lg, a, b, lo, up in legs] == rl, (q, p, pos)
            for t, lg, a, b, lo, up in legs:
                if width(lo, up):
                    assert range(lo, up + 1) == plain[p].rows(w[a:b]), (q, p, t, lg)
            assert {s for _, s in reads} == rr, (q, p, pos)
            assert len({s for _, s in reads}) == len(reads)
            # a read's identity row is the row of its full suffix, the lowest among equal reads
            for ident, s in reads:
                assert plain[p].table[ident][1] == 0 and plain[p].reads[plain[p].table[ident][0]] == s
            some += len(reads)
    assert some > 0


def test_the_inputs_reach_every_branch(sides):
    """the coverage guard: every label of the restatement, over the parameter matrix the GPU test runs"""
    fx, orc, _ = sides
    c = Counter()
    for M, k, skip in G.PARAMS:
        G.expected(orc, "fixture", fx.queries(), k, skip, M, c)
    missing = [x for x in G.LABELS if c[x] == 0]
    assert not missing, (missing, dict(c))


def test_degenerate_queries_contribute_nothing(sides):
    fx, orc, _ = sides
    w = fx.haps[0][100:179]
    for k, skip, pos, q in ((0, 0, 1, w), (-3, 0, 1, w), (8, -1, 1, w), (8, 0, 80, w), (8, 0, 1, w[:7]), (8, 0, 0, "")):
        assert G.gt_query(orc[0], q, pos, k, skip, 3) == ([], [])
