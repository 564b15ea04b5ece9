"""The sample-walk reference the sample-walk tests share -- TEST INFRASTRUCTURE, CPU only.  include/rsbwt.h's definition of
rsbwt_set_extension_samples / rsbwt_set_walk_samples restated twice, each time as a `side` of walk_reference's loop:

  * over sample_reference.counts_plain (plain_side): no BWT at all;
  * over sample_reference.counts_oracle (oracle_side): the oracle's BWT, every row's LF walk, the head ordinals.

A side has ONE shard (S = 1: SC(x) is already summed over the shards) and answers W(0, x) = the sum over the masked columns
of SC(x).strings (copies=True: SC(x).copies, which may be negative) and matches(x) = SC(x).matches.  walk_reference's
context / candidates / extensions turn that into the four sums of a string, both strands added; evaluate() holds a negative
total at 0 and looks for a candidate-strand query over max_rows (WIDE); walk() is walk_reference.walk with the WIDE stop
looked at first.

The fixture that shows the feature (haplotype_fixture): two haplotypes of 200 symbols that differ by one SNP and, further
on, by a deletion of two bases; reads of 40..60 symbols from every third offset of each, dealt round-robin to S shards.  A
read that only haplotype A spells lists samples a1 and a2, one that only B spells lists b1, one that both spell lists all
three."""
import hashlib
from collections import namedtuple

import sample_reference as SR
import walk_reference as WR
from kmer_reference import _bwt_runs, _rc

WIDE = 8
ACGT = "ACGT"


class Side:
    """SC(x) of one query at a time, remembered; count(x) -> sample_reference's answer for [x]"""
    S = 1

    def __init__(self, count, codes, mask_codes, copies=False, memo=None):
        self._count, self._sc = count, {} if memo is None else memo  # (memo: SC(x) shared by sides that differ in mask or copies)
        self.cols = [i for i, c in enumerate(codes) if c in set(mask_codes)]
        self.copies = copies

    def sc(self, x):
        if x not in self._sc:
            r = self._count(x)
            self._sc[x] = ([int(v) for v in r["strings"][0]], [int(v) for v in r["copies"][0]], int(r["matches"][0]))
        return self._sc[x]

    def W(self, p, x):
        assert p == 0
        strings, copies, _ = self.sc(x)
        return sum((copies if self.copies else strings)[i] for i in self.cols)

    def matches(self, x):
        return self.sc(x)[2]


def plain_side(shards, pairs, codes, size_of_sample, has_other, mask_codes, copies=False, memo=None):
    return Side(lambda x: SR.counts_plain(shards, pairs, [x], codes, size_of_sample, has_other), codes, mask_codes, copies, memo)


def oracle_side(osh, codes, size_of_sample, has_other, mask_codes, copies=False, memo=None):
    return Side(lambda x: SR.counts_oracle(osh, [x], codes, size_of_sample, has_other), codes, mask_codes, copies, memo)


def evaluate(side, s, ctx, left, both, max_rows):
    """(msup[4], wide, matches[4]) of one string; zeros for an invalid one"""
    c = WR.context(s, ctx, left)
    if c is None:
        return (0, 0, 0, 0), False, (0, 0, 0, 0)
    cands = WR.candidates(c, left)
    per = [[side.matches(y) for y in ((x, _rc(x)) if both else (x,))] for x in cands]
    matches = tuple(sum(m) for m in per)
    if any(m > max_rows for ms in per for m in ms):
        return (0, 0, 0, 0), True, matches
    tot = WR.extensions(side, s, ctx, left, both)[0]
    return tuple(max(t, 0) for t in tot), False, matches


def walk(side, seed, ctx, min_count, max_steps, left, both, max_rows):
    m = max(min_count, 1)
    s, ext, sup, seen = seed, "", [], []
    if WR.context(s, ctx, left) is None:
        return WR.Walk("", WR.INVALID, (), (0, 0, 0, 0), s, ())
    while True:
        if len(ext) == max_steps:
            return WR.Walk(ext, WR.LIMIT, tuple(sup), (0, 0, 0, 0), s, tuple(seen))
        seen.append(WR.context(s, ctx, left))
        tot, wide, _ = evaluate(side, s, ctx, left, both, max_rows)
        if wide:
            return WR.Walk(ext, WIDE, tuple(sup), (0, 0, 0, 0), s, tuple(seen))
        live = [b for b in range(4) if tot[b] >= m]
        if len(live) != 1:
            return WR.Walk(ext, WR.BRANCH if live else WR.DEAD_END, tuple(sup), tot, s, tuple(seen))
        b = live[0]
        ext += ACGT[b]
        sup.append(min(tot[b], 2 ** 32 - 1))
        s = ACGT[b] + s if left else s + ACGT[b]


# ---- the haplotype fixture -------------------------------------------------------------------------------------------

Haps = namedtuple("Haps", ["a", "b", "snp", "indel", "reads", "pairs", "codes", "size_of_sample", "has_other"])
A1, A2, B1 = b"a1", b"a2", b"b1"
HAP_LEN, SNP_AT, INDEL_AT = 200, 80, 140
_HAPS = {}


def _sequence(n, seed):
    out, i = [], 0
    while len(out) < n:
        for byte in hashlib.sha256(f"{seed}/{i}".encode()).digest():
            out.append(ACGT[byte & 3])
        i += 1
    return "".join(out[:n])


def haplotype_fixture():
    if not _HAPS:
        a = _sequence(HAP_LEN, "haplotype")
        snp = ACGT[(ACGT.index(a[SNP_AT]) + 1) % 4]
        b = a[:SNP_AT] + snp + a[SNP_AT + 1:INDEL_AT] + a[INDEL_AT + 2:]
        assert a[INDEL_AT] != a[INDEL_AT + 2], "the deletion must show at its first symbol"

        def reads_of(h):
            out = []
            for at in range(0, len(h) - 40 + 1, 3):
                ln = 40 + hashlib.sha256(f"len/{at}".encode()).digest()[0] % 21  # (the same on both: the shared flank gives equal reads)
                out.append(h[at:at + ln])
            return out
        ra, rb = reads_of(a), reads_of(b)
        sa, sb = set(ra), set(rb)
        rec = lambda code, c: code + bytes([33 + c, 33 + 7])  # noqa: E731
        pairs = []
        for r in sorted(sa | sb):
            who = ([A1, A2] if r in sa else []) + ([B1] if r in sb else [])
            pairs.append((r, b"".join(rec(code, 1 + i) for i, code in enumerate(who))))
        # the dictionary: the three samples among others, in an order that is not ascending
        codes = [b"zz", B1, b"c9", A2, A1, b"00"]
        _HAPS["fx"] = Haps(a, b, SNP_AT, INDEL_AT, [r for pair in zip(ra, rb) for r in pair] + ra[len(rb):] + rb[len(ra):], pairs, codes, 2, True)
    return _HAPS["fx"]


def dealt(reads, S):
    return [reads[p::S] for p in range(S)]


_RUNS = {}


def runs(reads, S):
    key = (hashlib.sha256("\n".join(reads).encode()).hexdigest(), S)
    if key not in _RUNS:
        _RUNS[key] = [_bwt_runs(sh) for sh in dealt(reads, S)]
    return _RUNS[key]


# ---- the gt fixture's reads under sample_reference.sample_pairs' values ----------------------------------------------

class GtCase:
    """walk_reference's `stranded` reads in `S` shards, values from sample_pairs (record counts 0 .. 2,000, stray tails, a code
    listed twice, negative c, unknown codes, every ninth read left out), a dictionary of 12 codes in an order that is not
    ascending of which 9 are masked; seeds: 7 windows, then walk_reference's five special seeds"""
    ctx, max_steps = 20, 12

    def __init__(self, oracle=None, S=2, size_of_sample=2, has_other=True):
        self.S, self.ss, self.other = S, size_of_sample, has_other
        self.shards = WR.dealt("stranded", S)
        self.uni, self.outside = SR.universe(size_of_sample)
        self.pairs, self.info = SR.sample_pairs(self.shards, self.uni, self.outside, size_of_sample, has_other)
        self.codes = self.uni[:30:3] + self.uni[40:42]
        self.mask = self.codes[:5] + self.codes[6:10]
        self.all_seeds = WR.seeds(self.ctx)
        self.seeds = self.all_seeds[:21:3] + self.all_seeds[WR.N_PLAIN:]
        self._oracle, self._osh, self._memo, self._walks = oracle, None, {"plain": {}, "oracle": {}}, {}

    def side(self, which, copies, mask=None):
        mask = self.mask if mask is None else mask
        if which == "plain":
            return plain_side(self.shards, self.pairs, self.codes, self.ss, self.other, mask, copies, self._memo["plain"])
        if self._osh is None:
            self._osh = SR.OracleShards(self._oracle, self.shards, WR.runs("stranded", self.S), self.pairs)
        return oracle_side(self._osh, self.codes, self.ss, self.other, mask, copies, self._memo["oracle"])


_GT = {}


def gt_case(oracle=None, S=2, size_of_sample=2, has_other=True):
    key = (S, size_of_sample, has_other)
    if key not in _GT:
        _GT[key] = GtCase(oracle, S, size_of_sample, has_other)
    if oracle is not None:
        _GT[key]._oracle = oracle
    return _GT[key]


def gt_walks(c, which, copies, left, both, max_rows, min_count=1, max_steps=None, seeds=None):
    """the walks of the case's seeds, computed once per parameter set"""
    max_steps = c.max_steps if max_steps is None else max_steps
    key = (which, copies, left, both, max_rows, min_count, max_steps, None if seeds is None else tuple(seeds))
    if key not in c._walks:
        side = c.side(which, copies)
        c._walks[key] = [walk(side, s, c.ctx, min_count, max_steps, left, both, max_rows) for s in (c.seeds if seeds is None else seeds)]
    return c._walks[key]
