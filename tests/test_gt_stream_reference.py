"""CPU guards for tests/test_gpu_gt_streams.py: what tests/stream_reference.py's SiteMatch batches (gt_queries, GT_PARAMS)
reach, shown with the restatement alone (tests/gt_reference.py over the oracle) before anything runs on a GPU -- every
branch label, the reference's (0, 2^64 - 1) corner in mid-search on the streams without '$' rows, legs at both ends of the
rows, right growth across the table depth, long lengthenings, reads of unlike lengths inside one LEFT leg, reads longer
than the internal extraction stride, nested and duplicate reads.  On the read sets the restatement is held to the
computation without a BWT (tests/test_gt_reference.py: legs_by_rule over PlainShard); a run stream that is no BWT of
reads has no string-level truth, and there the restatement is the definition."""
import time
from collections import Counter

import pytest

import gt_reference as G
import stream_reference as R
from test_gt_reference import PlainShard, legs_by_rule

T = 6  # the table depth the GPU cases use
U64 = G.U64
NO_ANSWER = ("noleg.end>L", "noleg.start<1", "noleg.cover.leftmost")


def _width(lo, up):
    return (up - lo + 1) & U64


def _all(src):
    """every parameter triple of the source: [(triple, expected [q] -> (legs, reads), Counter)]"""
    qs = R.gt_queries(src)
    out = []
    for M, k, skip in R.gt_params(src):
        c = Counter()
        exp = R.gt_expected([src], "small", qs, k, skip, M, c)
        out.append(((M, k, skip), [exp[q][0] for q in range(len(qs))], c))
    return qs, out


def test_the_expected_values_are_cheap(oracle, rsb):
    """every expected value of this module and of the GPU module's single-shard cases, computed here once: the GPU cases
    share them through the memo, so their share of this is the figure printed divided by the cases"""
    t = time.time()
    for name in R.STREAMS + R.FIXTURES:
        src = R.source(name, oracle, rsb)
        qs, per = _all(src)
        for M, k, skip in R.gt_params(src):
            R.gt_narrow_steps(src, qs, k, skip, M)
    spent = time.time() - t
    print(f"expected values of {len(R.STREAMS + R.FIXTURES)} sources: {spent:.1f} s")


@pytest.mark.parametrize("name", R.STREAMS + R.FIXTURES)
def test_the_batches_have_the_sizes_and_the_edges(oracle, rsb, name):
    src = R.source(name, oracle, rsb)
    qs = R.gt_queries(src)
    assert R.gt_queries(src) is qs and qs == R.gt_queries(src, "small")
    assert 30 <= len(qs) <= 60, len(qs)
    assert max(len(w) for w, _ in qs) <= (R.MAX_QUERY if src.reads is not None else 70)
    empty = ("", 0)
    assert qs[:3] == [empty] * 3 and qs[3] != empty and qs[-4:] == [empty] * 4 and qs[-5] != empty
    mid = [i for i in range(4, len(qs) - 7) if qs[i:i + 3] == [empty] * 3 and qs[i - 1] != empty and qs[i + 3] != empty]
    assert len(mid) == 1, mid
    ks = [k for _, k, _ in R.gt_params(src)]
    assert any(0 < len(w) < min(ks) for w, _ in qs)  # shorter than every k, between long queries
    _, kmin, skip = min(R.gt_params(src), key=lambda p: p[1])
    tiles = with_n = 0
    for w, pos in qs:
        if len(w) >= kmin and pos <= len(w):
            for i in range((len(w) - kmin) // (skip + 1) + 1):
                t = w[(skip + 1) * i:(skip + 1) * i + kmin]
                tiles += not set(t) - set("ACGT")
                with_n += "N" in t
    print(name, "queries", len(qs), "symbols", sum(len(w) for w, _ in qs), f"all-ACGT tiles at k = {kmin}, skip = {skip}:", tiles,
          "items", 2 * tiles, "workgroups of 256 lanes", -(-2 * tiles // 256))
    assert 2 * tiles > 3 * 256 and with_n > 0
    assert {p for w, p in qs if w} >= {0, 1} and any(p == len(w) for w, p in qs if w) and any(p == len(w) + 1 for w, p in qs if w)
    if src.reads is None:
        oix = src.orc.oix
        for x in (R.suffix_at(oix, oix.pc("A"), 7), R.suffix_at(oix, src.n - 1, 7)):
            for c1 in "ACGT":
                for c2 in "ACGT":
                    assert any(w == c2 + c1 + x and p in (1, len(w)) for w, p in qs), (name, c2 + c1 + x)
            assert sum(1 for w, _ in qs if len(w) > 40 and any(c2 + "A" + x in w[10:-10] for c2 in "ACGT")) >= 1
    if name == "single":
        assert {"CCCCCCCCA", "ACCCCCCCC", "CCCCACCCC"} <= {w for w, _ in qs}


def test_the_streams_reach_every_branch(oracle, rsb):
    """over the run streams together: every label of the restatement; a right lengthening that takes its string from under
    the table depth to it; a leg of more than 32 lengthenings; every cause of a leg without an answer"""
    total, cross, longest = Counter(), 0, 0
    for name in R.STREAMS:
        src = R.source(name, oracle, rsb)
        qs, per = _all(src)
        mine = Counter()
        for (M, k, skip), exp, c in per:
            mine.update(c)
            per_leg = Counter()
            for q, grown in enumerate(R.gt_grown(src, qs, k, skip, M)):
                for tile, leg, side, a, b in grown:
                    per_leg[(q, tile, leg)] += 1
                    cross += side == "R" and b - a - 1 < T <= b - a
            longest = max(longest, max(per_leg.values(), default=0))
        print(name, dict(mine))
        total.update(mine)
    print("right lengthenings that reach the table depth", cross, "most lengthenings of a leg", longest)
    missing = [x for x in G.LABELS if total[x] == 0]
    assert not missing, missing
    assert cross > 0 and longest > 32
    assert all(total[x] > 0 for x in NO_ANSWER)


class _Recorded:
    """a shard side whose find keeps every (string, interval) the restatement asked for"""

    def __init__(self, side):
        self.side, self.finds = side, {}
        self.extract, self.identity = side.extract, side.identity

    def find(self, w):
        iv = self.side.find(w)
        self.finds[w] = iv
        return iv


def test_the_stream_without_terminators_meets_the_corner_in_mid_search(oracle, rsb):
    """nodollar: finds of the restatement that return the reference's (0, 2^64 - 1), and finds of strings one or two symbols
    longer than such a string -- their search went on from the corner -- that return an empty interval"""
    src = R.source("nodollar", oracle, rsb)
    qs = R.gt_queries(src)
    rec = _Recorded(R.gt_side(src))
    for M, k, skip in R.gt_params(src):
        for w, pos in qs:
            G.gt_query(rec, w, pos, k, skip, M)
    corner = {w for w, iv in rec.finds.items() if iv[1] == U64}
    assert corner and all(rec.finds[w] == (0, U64) for w in corner)
    beyond = {w: iv for w, iv in rec.finds.items() for d in (1, 2) if len(w) > d and w[d:] in corner and set(w) <= set("ACGT")}
    print("nodollar: finds at the corner", len(corner), sorted(corner, key=len)[:4], "finds that went on from it", len(beyond),
          sorted(beyond.items())[:4])
    assert beyond and all(_width(*iv) == 0 for iv in beyond.values())
    assert any(iv[1] != U64 for iv in beyond.values())  # left the corner: (pc[c], pc[c] - 1)


def test_the_ends_of_the_rows(oracle, rsb):
    """single: an empty leg; the streams without '$': a leg of rows from row 0 on; every shaped stream: a leg that ends at
    the last row (or the figure printed)"""
    for name in R.STREAMS:
        src = R.source(name, oracle, rsb)
        _, per = _all(src)
        legs = [x for _, exp, _ in per for lg, _ in exp for x in lg]
        cls = {"legs": len(legs), "empty": sum(_width(lo, up) == 0 for *_, lo, up in legs),
               "corner": sum((lo, up) == (0, U64) for *_, lo, up in legs),
               "lower==0": sum(lo == 0 and _width(lo, up) > 0 for *_, lo, up in legs),
               "upper==n-1": sum(up == src.n - 1 and _width(lo, up) > 0 for *_, lo, up in legs)}
        print(name, cls)
        if name == "single":
            assert cls["empty"] > 0 and cls["corner"] > 0
        if name in ("single", "nodollar"):
            assert cls["lower==0"] > 0, cls
        if name in R.SHAPED and not cls["upper==n-1"]:
            print(name, "no leg ends at row n - 1")


class _ScannedShard(PlainShard):
    """PlainShard for thousands of reads: W(x) by scanning the reads laid end to end ('$' between them) for every
    (overlapping) occurrence, once per string"""

    def __init__(self, reads):
        PlainShard.__init__(self, reads)
        self.text, self.seen = "$".join(reads), {}

    def W(self, x):
        if not x or set(x) - set("ACGT"):
            return 0
        if x not in self.seen:
            n, at = 0, self.text.find(x)
            while at >= 0:
                n += 1
                at = self.text.find(x, at + 1)
            self.seen[x] = n
        return self.seen[x]


@pytest.mark.parametrize("name", R.FIXTURES)
def test_restatement_agrees_with_the_computation_without_a_bwt(oracle, rsb, name):
    """legs by (tile, leg, a, b, width), the rows of the non-empty legs, the read sets and the identity rows"""
    src = R.source(name, oracle, rsb)
    plain = _ScannedShard(src.reads)
    assert all(plain.W(x) == PlainShard.W(plain, x) for x in ("ACGT", "A" * 30, src.reads[0][:9], src.reads[-1]))
    qs, per = _all(src)
    lowest = {}
    for r, (i, j) in enumerate(plain.table):
        if j == 0:
            lowest.setdefault(plain.reads[i], r)
    some = 0
    for (M, k, skip), exp, _ in per:
        for q, (w, pos) in enumerate(qs):
            legs, reads = exp[q]
            rl, rr = legs_by_rule(plain, w, pos, k, skip, M)
            assert [(t, lg, a, b, _width(lo, up)) for t, lg, a, b, lo, up in legs] == rl, (q, pos, M, k, skip)
            for t, lg, a, b, lo, up in legs:
                if _width(lo, up):
                    assert range(lo, up + 1) == plain.rows(w[a:b]), (q, t, lg)
            assert {s for _, s in reads} == rr and len({s for _, s in reads}) == len(reads), (q, pos, M, k, skip)
            for ident, s in reads:
                i, j = plain.table[ident]
                assert j == 0 and plain.reads[i] == s
                assert ident == lowest[s]  # the lowest identity row among equal reads
            some += len(reads)
    assert some > 0


def test_ragged_read_lengths_decide_and_long_and_nested_reads_are_kept(oracle, rsb):
    src = R.source("ragged", oracle, rsb)
    qs, per = _all(src)
    decided = longer = nested = 0
    for (M, k, skip), exp, _ in per:
        for q, (w, pos) in enumerate(qs):
            legs, reads = exp[q]
            kept = [s for _, s in reads]
            longer += sum(len(s) > 256 for s in kept)
            nested += sum(1 for s in kept for o in kept if o != s and o.startswith(s))
            for t, lg, a, b, lo, up in legs:
                s0 = (skip + 1) * t
                if pos > s0 + k and _width(lo, up) > 1:  # a LEFT tile: pos - end <= |postfix| - k + 4 keeps the row
                    by_offset = {}
                    for r in range(lo, up + 1):
                        pre, post = src.orc.extract(r)
                        by_offset.setdefault(len(pre), set()).add(((pos - b) & U64) <= (len(post) - k) + G.INDEL)
                    decided += sum(len(v) == 2 for v in by_offset.values())
    print("ragged: offsets of a LEFT leg where the read's length decided", decided, "kept reads longer than 256 symbols", longer,
          "kept reads that are proper prefixes of other kept reads", nested)
    assert decided > 0 and longer > 0 and nested > 0


def test_repeat_reports_duplicate_reads_once(oracle, rsb):
    src = R.source("repeat", oracle, rsb)
    starts = Counter(src.reads)
    qs, per = _all(src)
    twice = 0
    for _, exp, _ in per:
        for legs, reads in exp:
            assert len({s for _, s in reads}) == len(reads)
            twice += sum(starts[s] >= 2 for _, s in reads)
    print("repeat: kept reads that occur at two identity rows or more, reported once", twice)
    assert twice >= 20
