"""The overlap reference the overlap tests share -- TEST INFRASTRUCTURE.  include/rsbwt.h's definition restated twice over
gt_reference.fixture() and match_reference.queries() (15 strings, 800 positions, 2 shards, 1,600 items):

  * over the oracle's BWT (OracleSide): findInterval of every suffix asked for on its own (gt_reference.OracleShard.find)
    and Occ('$', .) at its two ends (oix.occ) -- where the GPU takes one backward search through all of them;
  * with no BWT at all (PlainSide): the number of reads that startswith the suffix, bisect_left(sorted(reads), x) as the
    first ordinal, sorted(reads)[o] as the read at ordinal o.

An entry is (ordinal, count) at the position where its suffix starts: count > 0 only for a suffix of l >= max(min_overlap,
1) symbols, l <= max_overlap where that is not 0, all ACGT, whose interval is proper by the C-ABI's rule (lower <= upper and
upper < n); ordinal is 0 where count is."""
import bisect

import gt_reference as G
import match_reference as M

# (min_overlap, max_overlap): every depth, the table depths the GPU tests use, one between them under a limit, none left
PARAMS = [(1, 0), (6, 0), (12, 0), (10, 30), (41, 0)]
ACGT = set("ACGT")


def queries():
    return M.queries()


def wanted(l, x, min_overlap, max_overlap):
    return l >= max(min_overlap, 1) and (max_overlap == 0 or l <= max_overlap) and not (set(x) - ACGT)


class OracleSide:
    """(ordinal, count, lower, upper) of a suffix from findInterval and Occ('$', .)"""
    ZERO = (0, 0, 1, 0)

    def __init__(self, sh):
        self.sh, self.n = sh, sh.oix.bwlen()

    def entry(self, x):
        lo, up = self.sh.find(x)
        if M.width((lo, up), self.n) == 0:
            return (0, 0, lo, up)
        before = self.sh.oix.occ("$", lo - 1) if lo else 0  # Occ(., -1) = 0
        cnt = self.sh.oix.occ("$", up) - before
        return (before if cnt else 0, cnt, lo, up)

    def proper(self, x):
        return M.width(self.sh.find(x), self.n) > 0


class PlainSide:
    """(ordinal, count) of a suffix from the read list alone"""
    ZERO = (0, 0)

    def __init__(self, reads):
        self.sorted = sorted(reads)

    def entry(self, x):
        cnt = sum(r.startswith(x) for r in self.sorted)
        return (bisect.bisect_left(self.sorted, x) if cnt else 0, cnt)

    def read(self, o):
        return self.sorted[o]


def profile(side, w, min_overlap, max_overlap):
    """per position t of query w: side.entry of the suffix w[t:], zeros where the suffix is not wanted"""
    out = []
    for t in range(len(w)):
        x = w[t:]
        e = side.entry(x) if wanted(len(x), x, min_overlap, max_overlap) else None
        out.append(e if e is not None and e[1] > 0 else side.ZERO)
    return out


_EXPECTED = {}


def expected(orc, key, qs, min_overlap, max_overlap):
    """per shard and query: the list over the query's positions of (ordinal, count, lower, upper) from the oracle; computed
    once per (key, parameters).  orc: a list of gt_reference.OracleShard"""
    at = (key, min_overlap, max_overlap)
    if at not in _EXPECTED:
        _EXPECTED[at] = [[profile(OracleSide(sh), w, min_overlap, max_overlap) for w in qs] for sh in orc]
    return _EXPECTED[at]


def flat(exp):
    """expected() as rsbwt_set_overlaps lays it out: (count, ordinal) lists [shard][position]"""
    return tuple([[x[i] for per in sh for x in per] for sh in exp] for i in (1, 0))


def records(exp, qs):
    """rsbwt_set_overlap_records' records (query, shard, start, length, ordinal, count, lower, upper) in its order, and
    first[]"""
    S, Q = len(exp), len(qs)
    recs, first = [], [0]
    for q in range(Q):
        for p in range(S):
            recs += [(q, p, t, len(qs[q]) - t) + e for t, e in enumerate(exp[p][q]) if e[1] > 0]
            first.append(len(recs))
    return recs, first


def reads_of(exp, qs, plain, max_reads=0):
    """rsbwt_set_overlap_reads' output: (first, [(overlap, ordinal, read)] in its order, matches[q*S+p]): a read once per
    (query, shard), at its longest overlap; overlap descending, then ordinal ascending; a (query, shard) over max_reads
    reports none.  plain: a list of PlainSide, the read at an ordinal"""
    S, Q = len(exp), len(qs)
    out, first, matches = [], [0], []
    for q in range(Q):
        for p in range(S):
            seen, mine = set(), []
            for t, (o, cnt, _, _) in enumerate(exp[p][q]):  # start ascending = overlap descending
                for x in range(o, o + cnt):
                    if x not in seen:
                        seen.add(x)
                        mine.append((len(qs[q]) - t, x, plain[p].read(x)))
            matches.append(len(mine))
            if not (max_reads and len(mine) > max_reads):
                out += mine
            first.append(len(out))
    return first, out, matches


def lf_steps(side, w, max_overlap):
    """the LF steps a walk of w without a k-mer table takes in one shard: initInterval of the last symbol, then one step
    per symbol up to and including the first that empties the interval; the walk stops at the limit or at a symbol outside
    ACGT"""
    L = len(w)
    limit = min(L, max_overlap) if max_overlap else L
    if limit == 0 or w[-1] not in ACGT or not side.proper(w[-1]):
        return 0
    steps = 0
    for j in range(1, limit):  # from depth j to depth j + 1
        if w[L - j - 1] not in ACGT:
            break
        steps += 1
        if not side.proper(w[L - j - 1:]):
            break
    return steps


def total_lf_steps(orc, qs, max_overlap):
    return sum(lf_steps(OracleSide(sh), w, max_overlap) for sh in orc for w in qs)


def fixture():
    return G.fixture()
