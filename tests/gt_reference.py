"""The SiteMatch reference the gt tests share -- TEST INFRASTRUCTURE.  find_gt_reads (src/service/service.cpp:507-711)
restated branch by branch, with its linear lengthening loops, over any object that answers

    find(w)      -> (lower, upper) of findInterval(w); (1, 0) for a string holding a symbol outside ACGT (the C-ABI's rule)
    extract(row) -> (extractPrefix(row), extractPostfix(row))
    identity(row)-> the row of the read's full suffix (where extractPrefix's walk ends)

OracleShard answers from the oracle binding (the BWT); tests/test_gt_reference.py has a second one that uses no BWT.

Two guards are added to the reference, which loops forever or throws std::out_of_range there: a lengthening that would
need end > |w| or start < 1 ends its leg with no answer; the tile's other leg still counts.  Every branch taken is counted
in a Counter under a label (LABELS), so that a test can show its inputs reach all of them.

Legs are reported 0-based half-open: the final string is w[a:b), the reference's start = a + 1 and end = b; leg 0 = the
tile itself, 1 / 2 = the first / second lengthened leg."""
import random
from collections import Counter

from kmer_reference import Walks, _bwt_runs

U64 = (1 << 64) - 1
INDEL = 4            # indel_allowance, :509
M_DEFAULT = 10000    # max_interval_size, :85

LABELS = ("single.left", "single.right", "single.cover", "left.leg1", "left.leg2", "left.leg2.turn", "right.leg1", "right.leg2",
          "right.leg2.turn", "cover.leg1", "cover.leg2", "noleg.end>L", "noleg.start<1", "noleg.cover.leftmost", "wrap.left",
          "wrap.right", "tile.N", "grow.N", "leg.empty")


class OracleShard:
    def __init__(self, oix):
        self.oix = oix
        self.walks = Walks(oix)
        self._find, self._ext = {}, {}

    def find(self, w):
        if w not in self._find:
            self._find[w] = (1, 0) if (not w or set(w) - set("ACGT")) else self.oix.find_interval(w)
        return self._find[w]

    def extract(self, row):
        if row not in self._ext:
            self._ext[row] = self.oix.extract(row)
        return self._ext[row]

    def identity(self, row):
        return self.walks.identity(row)


def _wide(iv, M):
    return ((iv[1] - iv[0] + 1) & U64) > M


def find_gt_reads(sh, w, index, kmers, skip, pos, M=M_DEFAULT, count=None, grown=None):
    """one tile: (legs, kept) -- legs = [(leg, a, b, lower, upper)], kept = {read string: its lowest identity row};
    grown (a list) takes every lengthening as (leg, "L" or "R", a, b): the side the symbol was taken in on and the longer
    string w[a:b) that was searched"""
    C = count if count is not None else Counter()
    legs, kept = [], {}

    def longer(leg, side, start, size):
        if grown is not None:
            grown.append((leg, side, start - 1, start - 1 + size))
        return find(w[start - 1:start - 1 + size])
    length = len(w)
    kmer = w[(skip + 1) * index:(skip + 1) * index + kmers]
    if set(kmer) - set("ACGT"):  # don't bother with N (:513)
        C["tile.N"] += 1
        return legs, kept

    def find(s):
        if set(s) - set("ACGT"):
            C["grow.N"] += 1
        return sh.find(s)

    def rows(leg, start, end, iv, side):
        legs.append((leg, start - 1, end, iv[0], iv[1]))
        if ((iv[1] - iv[0] + 1) & U64) == 0:
            C["leg.empty"] += 1
            return
        for j in range(iv[0], iv[1] + 1):
            prefix, postfix = sh.extract(j)
            if side == "left":
                if pos < end:
                    C["wrap.left"] += 1
                if ((pos - end) & U64) > (len(postfix) - kmers) + INDEL:  # (:538)
                    continue
            elif side == "right":
                if start < pos:
                    C["wrap.right"] += 1
                if ((start - pos) & U64) > len(prefix) + INDEL:  # (:608)
                    continue
            s, ident = prefix + postfix, sh.identity(j)
            kept[s] = min(kept.get(s, ident), ident)

    interval = find(kmer)
    start = (skip + 1) * index + 1  # 1-based
    end = start + kmers - 1
    if pos > end:  # kmer on the left (:522)
        if _wide(interval, M):
            C["left.leg1"] += 1
            cnt, ok = 0, True
            while _wide(interval, M):  # extend it to the right first (:527)
                cnt += 1
                if end + 1 > length:
                    C["noleg.end>L"] += 1
                    ok = False
                    break
                interval = longer(1, "R", start, kmers + cnt)
                end += 1
            if ok:
                rows(1, start, end, interval, "left")
            if index != 0:  # not starting at left most (:546)
                C["left.leg2"] += 1
                start = (skip + 1) * index + 1
                end = start + kmers - 1
                cnt, ok = 1, True
                start -= 1
                interval = longer(2, "L", start, kmers + cnt)
                while _wide(interval, M):
                    cnt += 1
                    side = "L"
                    if start > 1:
                        start -= 1
                    else:  # reach left most, continue to extend to the right (:560)
                        side = "R"
                        C["left.leg2.turn"] += 1
                        if end + 1 > length:
                            C["noleg.end>L"] += 1
                            ok = False
                            break
                        end += 1
                    interval = longer(2, side, start, kmers + cnt)
                if ok:
                    rows(2, start, end, interval, "left")
        else:
            C["single.left"] += 1
            rows(0, start, end, interval, "left")
    elif pos < start:  # kmer on the right (:593)
        if _wide(interval, M):
            C["right.leg1"] += 1
            cnt, ok = 0, True
            while _wide(interval, M):  # extend it to the left first (:598)
                cnt += 1
                if start <= 1:
                    C["noleg.start<1"] += 1
                    ok = False
                    break
                start -= 1
                interval = longer(1, "L", start, kmers + cnt)
            if ok:
                rows(1, start, end, interval, "right")
            if end < length:  # not ending at the right most (:616)
                C["right.leg2"] += 1
                start = (skip + 1) * index + 1
                end = start + kmers - 1
                cnt, ok = 1, True
                end += 1
                interval = longer(2, "R", start, kmers + cnt)
                while _wide(interval, M):
                    cnt += 1
                    side = "R"
                    if end < length:
                        end += 1
                    else:  # reach right most, continue to extend to the left (:630)
                        side = "L"
                        C["right.leg2.turn"] += 1
                        if start <= 1:
                            C["noleg.start<1"] += 1
                            ok = False
                            break
                        start -= 1
                    interval = longer(2, side, start, kmers + cnt)
                if ok:
                    rows(2, start, end, interval, "right")
        else:
            C["single.right"] += 1
            rows(0, start, end, interval, "right")
    else:  # kmer at the position (:661)
        if _wide(interval, M):
            C["cover.leg1"] += 1
            cnt, ok = 0, True
            while _wide(interval, M):  # extend it to the right first (:666)
                cnt += 1
                if end + 1 > length:
                    C["noleg.end>L"] += 1
                    ok = False
                    break
                interval = longer(1, "R", start, kmers + cnt)
                end += 1
            if ok:
                rows(1, start, end, interval, "cover")
            C["cover.leg2"] += 1
            start = (skip + 1) * index + 1
            end = start + kmers - 1
            cnt, ok = 1, True
            if start <= 1:  # (the reference throws at once: w.substr(npos, ...))
                C["noleg.cover.leftmost"] += 1
                ok = False
            else:
                start -= 1
                interval = longer(2, "L", start, kmers + cnt)
                while _wide(interval, M):
                    cnt += 1
                    if start <= 1:
                        C["noleg.start<1"] += 1
                        ok = False
                        break
                    start -= 1
                    interval = longer(2, "L", start, kmers + cnt)
            if ok:
                rows(2, start, end, interval, "cover")
        else:
            C["single.cover"] += 1
            rows(0, start, end, interval, "cover")
    return legs, kept


def gt_query(sh, w, pos, k, skip, M=0, count=None, grown=None):
    """GtTask::run's loop over the tiles (:1048-1072) in one shard: (legs as (tile, leg, a, b, lower, upper), ordered by
    (tile, leg); reads as [(identity row, string)] ascending, a string once at its lowest row); grown (a list) takes the
    lengthenings as (tile, leg, side, a, b)"""
    M = M if M else M_DEFAULT
    legs, kept = [], {}
    if k <= 0 or skip < 0 or len(w) < k or pos > len(w):
        return legs, []
    for i in range((len(w) - k) // (skip + 1) + 1):
        mine = [] if grown is not None else None
        lg, kp = find_gt_reads(sh, w, i, k, skip, pos, M, count, mine)
        if grown is not None:
            grown += [(i,) + x for x in mine]
        legs += [(i,) + x for x in sorted(lg)]
        for s, ident in kp.items():
            kept[s] = min(kept.get(s, ident), ident)
    return legs, sorted((ident, s) for s, ident in kept.items())


# ---- the fixture the gt tests share: a genome of about 2,000 symbols, a third of it a short tandem repeat, 4 haplotypes,
# reads of 40 symbols, 2 shards -- explicit seeded read lists, their BWTs by suffix sort (kmer_reference._bwt_runs)
READ_LEN = 40
UNIT = "ACGTTG"


class GtFixture:
    def __init__(self):
        rng = random.Random(50711)
        rnd = lambda n: "".join(rng.choice("ACGT") for _ in range(n))
        self.genome = rnd(660) + UNIT * 110 + rnd(680)
        self.rep = (660, 660 + 110 * len(UNIT))
        self.haps = []
        for _ in range(4):
            s = list(self.genome)
            for i in range(len(s)):
                if rng.random() < 0.004:
                    s[i] = rng.choice([c for c in "ACGT" if c != s[i]])
            self.haps.append("".join(s))
        reads = []
        for _ in range(560):
            h = self.haps[rng.randrange(4)]
            s = rng.randrange(len(h) - READ_LEN + 1)
            reads.append(h[s:s + READ_LEN])
        self.shards = [reads[0::2], reads[1::2]]
        self._runs = None

    def runs(self):
        if self._runs is None:
            self._runs = [_bwt_runs(r) for r in self.shards]
        return self._runs

    def queries(self):
        """(w, pos): windows of 79 symbols of a haplotype -- outside the repeat, entering it, inside it, leaving it -- with
        the site at 1, in the middle and at L; one with an N in a tile, one whose lengthening runs into an N; and the
        degenerate inputs (shorter than k, pos > L, empty)"""
        g, (r0, r1) = self.haps[1], self.rep
        out = []
        for at in (100, r0 - 45, r0 + 200, r1 - 30, 1500):
            w = g[at:at + 79]
            out += [(w, 1), (w, 40), (w, 79)]
        w = g[300:379]
        out.append((w[:30] + "N" + w[31:], 40))
        w = g[r0 + 100:r0 + 179]
        out += [(w[:20] + "N" + w[21:60] + "N" + w[61:], 40), (w[:20] + "N" + w[21:60] + "N" + w[61:], 79), (w[:20] + "N" + w[21:60] + "N" + w[61:], 1)]
        out += [(g[100:107], 3), (g[100:179], 80), ("", 0), (g[r0 + 6:r0 + 30], 12), (g[r0 + 6:r0 + 30], 1), (g[r0 + 6:r0 + 30], 24)]
        return out


PARAMS = [(M, k, skip) for M in (1, 3, 8) for k in (8, 12) for skip in (0, 3)]
_FX = []


def fixture():
    if not _FX:
        _FX.append(GtFixture())
    return _FX[0]


_EXPECTED = {}


def expected(shards, key, queries, k, skip, M, count=None):
    """per query and shard: gt_query's (legs, reads), computed once per (key, k, skip, M)"""
    at = (key, k, skip, M)
    if at not in _EXPECTED:
        c = Counter()
        _EXPECTED[at] = ([[gt_query(sh, w, pos, k, skip, M, c) for sh in shards] for w, pos in queries], c)
    if count is not None:
        count.update(_EXPECTED[at][1])
    return _EXPECTED[at][0]
