"""The matching-statistics reference the match tests share -- TEST INFRASTRUCTURE.  include/rsbwt.h's definition restated
twice:

  * over the oracle's BWT (gt_reference.OracleShard.find): the string ending at a position grows one symbol to the left at
    a time and findInterval is asked again for each, until W drops under m -- where the GPU stops at the first failing LF
    step, this asks for whole searches;
  * with no BWT at all (PlainCounts): W(x) = the occurrences of x in the read list, the largest l taken over EVERY l in
    [0, min(e, cap)], not the first failure; the interval from the sorted suffixes.

W(x) by the C-ABI's rule for an interval: lower <= upper and upper < n ? upper - lower + 1 : 0, and 0 for a string holding
a symbol outside ACGT.  A position is a SMEM iff len > 0 and (the query ends there or the next position's len is not
larger).

The queries are the ones the issue lists, over gt_reference.fixture(): 15 strings, 800 positions, 1,600 (position, shard)
items."""
import bisect
import random
from collections import Counter

import gt_reference as G
from kmer_reference import suffix_rows

# (max_len, min_rows): no cap, a cap under most matches, and two row thresholds
PARAMS = [(0, 1), (16, 1), (0, 3), (0, 20)]


def queries():
    fx = G.fixture()
    g, (r0, r1) = fx.haps[1], fx.rep
    out = [g[at:at + 79] for at in (100, r0 - 45, r0 + 200, r1 - 30, 1500)]
    w = g[300:379]
    out.append(w[:30] + "N" + w[31:])
    rng = random.Random(8128)
    out += ["".join(rng.choice("ACGT") for _ in range(60)) for _ in range(3)]
    out.append(fx.shards[0][17])
    out.append(fx.shards[1][5] + fx.shards[0][101])
    out += ["", "A", "N", g[r0 + 6:r0 + 30]]
    return out


def width(iv, n):
    lo, up = iv
    return up - lo + 1 if lo <= up and up < n else 0


def longest(sh, n, w, e, cap, m):
    """(l, lower, upper) of the longest match ending at end e of w (1-based end, the match is w[e-l:e]) over a shard that
    answers find(x)"""
    limit = min(e, cap) if cap else e
    best = (0, 1, 0)
    for l in range(1, limit + 1):
        x = w[e - l:e]
        if x[0] not in "ACGT":
            break
        iv = sh.find(x)
        if width(iv, n) < m:
            break
        best = (l, iv[0], iv[1])
    return best


def smems_of(stats):
    """the SMEMs of one query in one shard from its per-position (l, lower, upper): [(start, end, lower, upper)]"""
    out = []
    for t, (l, lo, up) in enumerate(stats):
        if l > 0 and (t + 1 == len(stats) or stats[t + 1][0] <= l):
            out.append((t + 1 - l, t + 1, lo, up))
    return out


_EXPECTED = {}


def expected(shards, key, qs, max_len, min_rows):
    """per shard and query: the list over the query's positions of (l, lower, upper); computed once per (key, parameters)"""
    at = (key, max_len, min_rows)
    if at not in _EXPECTED:
        m = max(min_rows, 1)
        _EXPECTED[at] = [[[longest(sh, sh.oix.bwlen(), w, e, max_len, m) for e in range(1, len(w) + 1)] for w in qs] for sh in shards]
    return _EXPECTED[at]


def flat(exp):
    """expected() as the calls lay it out: (len, lower, upper) lists [shard][position]"""
    return tuple([[x[i] for per in sh for x in per] for sh in exp] for i in range(3))


def smem_records(exp):
    """rsbwt_set_smems' records (query, shard, start, end, lower, upper) in its order, and first[]"""
    S, Q = len(exp), len(exp[0])
    recs, first = [], [0]
    for q in range(Q):
        for p in range(S):
            recs += [(q, p) + r for r in smems_of(exp[p][q])]
            first.append(len(recs))
    return recs, first


class PlainCounts:
    """occurrences of every string in a read list, and its rows among the sorted suffixes -- no BWT"""

    def __init__(self, reads):
        self.count = Counter(r[i:j] for r in reads for i in range(len(r)) for j in range(i + 1, len(r) + 1))
        self.tr = str.maketrans("ACGT", "BCDE")
        self.keys = [reads[i][j:].translate(self.tr) + "$" for i, j in suffix_rows(reads)]
        self.n = len(self.keys)

    def W(self, x):
        return 0 if (not x or set(x) - set("ACGT")) else self.count.get(x, 0)

    def interval(self, x):
        t = x.translate(self.tr)
        return bisect.bisect_left(self.keys, t), bisect.bisect_left(self.keys, t + "\x7f") - 1

    def longest(self, w, e, cap, m):
        limit = min(e, cap) if cap else e
        ok = [l for l in range(1, limit + 1) if self.W(w[e - l:e]) >= m]
        if not ok:
            return (0, 1, 0)
        l = max(ok)
        return (l,) + self.interval(w[e - l:e])
