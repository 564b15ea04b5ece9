"""The read sets the site-sample-counts tests run beyond the gt fixture -- TEST INFRASTRUCTURE, CPU only.  No restatement
of the definition is added here: the answers are tests/site_reference.py's (from gt_reference, sample_reference and
ksw_reference), computed once per key.  What is here is inputs:

  ragged-alleles  test_kmer_fixtures.fixture("ragged") -- read lengths 12 .. 600, 24 reads of 256 .. 600 symbols, prefixes
                  and suffixes of other reads, a genome with no variation -- plus variant reads at seven seeded sites: for
                  (up to a dozen of) the reads that cover a site a copy with another base there; at two sites also copies
                  with a one-base deletion or insertion 3 .. 10 symbols from the site; a few reads twice.  The first site is
                  where the most reads of fx.longs overlap, one site is covered by reads under 256 symbols only, one by a
                  read of the 12 .. 37 class.  Requests: both alleles of every site in a window of 79, a third base, isalt = 1,
                  pos = 0 and pos = L + 1, and three wide windows (600, 600 and 262 symbols) at the first site, so that reads of
                  256 .. 600 symbols are KEPT by the alignment (a read hanging more than 4 bases out of its window is not).
  repeat          fixture("repeat") as it is: windows through each tandem repeat and the random stretches between them,
                  both alleles at a site just outside a repeat, whole duplicated reads as windows.
  exact4096       one read of exactly 4,096 symbols on a head ordinal, in a small shard of its own beside a few short reads.

and dealings of them into shards: one shard, round-robin over 8, halves, and for ragged-alleles the dealing over 4 in which
every read over 256 symbols lies in shard 1 or 3, shard 2 is unrelated reads in which no tile of any request occurs (with
pairs in the table), and the pair list names no read of shard 0.

Input has the attributes of tests/test_gpu_site_counts.py's Ref, so that module's _check takes it."""
import random

import gt_reference as G
import sample_reference as SR
import site_reference as SITE
from kmer_reference import _bwt_runs
from test_kmer_fixtures import REPEATS, fixture

# (M, k, skip): gt_reference.PARAMS' and stream_reference.GT_PARAMS["reads"]' where they reach the guards of
# tests/test_site_sets_reference.py, and M = 0 (the default of 10,000: no leg is lengthened)
PARAMS = {"ragged-alleles": [(0, 12, 3), (8, 12, 3), (8, 8, 3)], "repeat": [(0, 12, 3), (3, 8, 0), (8, 20, 1)], "exact4096": [(0, 12, 3), (3, 12, 3)]}
WIDE = 256        # a read over this many symbols is extracted a second time (csrc/sets.hip, SITE_STRIDE)
K_MIN = 8         # the shortest tile of any parameter set: what "no tile occurs in shard 2" is about


class Input:
    """one read set dealt one way under one pair list: the pairs, the restatement's side, the batch, a dictionary of 12
    codes in an order that is not ascending, and the answers -- computed once, never changed"""

    def __init__(self, oracle, name, shards, reqs, alleles=(), ss=2, other=True, unnamed=(), pairs=None):
        self.name, self.shards, self.reqs, self.alleles = name, shards, list(reqs), list(alleles)
        self.runs = [_bwt_runs(sh) for sh in shards]
        self.ss, self.other = ss, other
        self.uni, self.outside = SR.universe(ss)
        self.info = None
        if pairs is None:
            pairs, self.info = SR.sample_pairs(shards, self.uni, self.outside, ss, other)
        unnamed = set(unnamed)
        self.pairs = [(w, v) for w, v in pairs if w not in unnamed]
        self.side = SITE.Side(oracle, shards, self.runs, self.pairs, (name, ss, other))
        self.codes = self.uni[:30:3] + self.uni[40:42]
        self._memo = {}

    def want(self, M, k, skip, reqs=None, codes=None):
        reqs = self.reqs if reqs is None else reqs
        codes = self.codes if codes is None else codes
        key = (M, k, skip, tuple(reqs), tuple(codes))
        if key not in self._memo:
            self._memo[key] = SITE.want(self.side, reqs, k, skip, M, codes, self.ss, self.other)
        return self._memo[key]


def _other(rng, c, also=""):
    return rng.choice([x for x in "ACGT" if x != c and x not in also])


# ---- ragged-alleles -------------------------------------------------------------------------------------------------
class RaggedAlleles:
    SITES, PER_SITE = 7, 12

    def __init__(self):
        fx = fixture("ragged")
        rng = random.Random(8128)
        g = self.genome = fx.sources[0]
        base = list(fx.shards[0])
        self.longs = list(fx.longs)
        at = {r: g.find(r) for r in set(base)}
        cover = lambda i: sorted(r for r, s in at.items() if s <= i < s + len(r))  # noqa: E731
        depth = [0] * len(g)
        for r in self.longs:
            for i in range(at[r], at[r] + len(r)):
                depth[i] += 1
        first = last = depth.index(max(depth))  # the middle of the first stretch the most long reads share
        while depth[last + 1] == depth[first]:
            last += 1
        self.long_site = (first + last) // 2
        tiny = [r for r in base if len(r) < 38]
        sites = [self.long_site]

        def far(i):
            return 400 < i < len(g) - 400 and all(abs(i - j) > 700 for j in sites)
        # a site only reads under 256 symbols cover; a site in the middle of a read of the 12 .. 37 class that others cover too
        self.short_site = next(i for i in (rng.randrange(len(g)) for _ in range(10 ** 5))
                               if far(i) and len(cover(i)) >= 5 and all(len(r) < WIDE for r in cover(i)) and not any(len(r) < 38 for r in cover(i)))
        sites.append(self.short_site)
        self.tiny_site = next(at[r] + len(r) // 2 for r in sorted(tiny, key=lambda r: rng.random())
                              if far(at[r] + len(r) // 2) and len(cover(at[r] + len(r) // 2)) >= 4)
        sites.append(self.tiny_site)
        while len(sites) < self.SITES:
            i = rng.randrange(len(g))
            if far(i) and len(cover(i)) >= 4:
                sites.append(i)
        self.sites = sites
        self.indel_sites = (sites[0], sites[3])
        self.alt = {i: _other(rng, g[i]) for i in sites}
        added = []
        for i in sites:
            cov = cover(i)
            some = [r for r in cov if len(r) > WIDE] + sorted((r for r in cov if len(r) <= WIDE), key=lambda r: rng.random())
            for n, r in enumerate(some[:self.PER_SITE]):
                j = i - at[r]
                copy = r[:j] + self.alt[i] + r[j + 1:]
                added.append(copy)
                if n < 6:  # nested reads: a prefix that ends 3 .. 10 symbols before the site, a suffix that begins 1 .. 6 after it
                    added += [x for x in ((r, copy)[n % 2][:max(j - 3 - (n * 3 + i) % 8, 0)], r[j + 1 + (n + i) % 6:]) if len(x) >= 12]
                if i not in self.indel_sites:
                    continue
                # a one-base deletion and a one-base insertion 3 .. 10 symbols from the site, on either allele and side
                for kind in ("del", "ins"):
                    s = list(r if (n + (kind == "ins")) % 2 else copy)
                    d = rng.randrange(3, 11) * rng.choice((-1, 1))
                    if not 2 <= j + d < len(s) - 2:
                        d = -d
                    if not 2 <= j + d < len(s) - 2:
                        continue
                    if kind == "del":
                        del s[j + d]
                    else:
                        s[j + d:j + d] = [_other(rng, s[j + d], s[j + d - 1])]
                    added.append("".join(s))
        added += self._made(rng, sites[3])
        reads = base + added
        reads += [added[0], added[5], self.longs[3], base[7], base[7], base[100]]  # a few reads twice (one three times)
        rng.shuffle(reads)
        self.reads = reads
        # ---- the requests
        reqs, alleles = [], []
        for i in sites:
            w, o = g[i - 39:i + 40], self.alt[i]
            alleles.append((len(reqs), len(reqs) + 1))
            reqs += [(w, 40, o, 0), (w[:39] + o + w[40:], 40, g[i], 0)]
        for i in sites[:2]:  # a third base as alt (site_reference.batch), and the alt allele asked with isalt = 1
            w, o = g[i - 39:i + 40], self.alt[i]
            reqs += [(w, 40, next(c for c in "ACGT" if c not in (g[i], o)), 0), (w, 40, o, 1), (w[:39] + o + w[40:], 40, g[i], 1)]
        w = g[sites[4] - 39:sites[4] + 40]
        reqs += [(w, 0, "A", 0), (w, 80, "A", 1)]
        self.narrow = len(reqs)  # the requests from here on have the wide windows
        i, o = self.long_site, self.alt[self.long_site]
        lo = min(at[r] for r in self.longs if at[r] <= i < at[r] + len(r))
        w = g[lo:lo + 600]
        alleles.append((len(reqs), len(reqs) + 1))
        reqs += [(w, i - lo + 1, o, 0), (w[:i - lo] + o + w[i - lo + 1:], i - lo + 1, g[i], 0)]
        r = min((r for r in self.longs if at[r] <= i < at[r] + len(r)), key=len)
        reqs.append((g[at[r] - 2:at[r] + len(r) + 3], i - at[r] + 3, o, 0))
        self.reqs, self.alleles = reqs, alleles

    def _made(self, rng, i):
        """reads of 50 symbols from the window of 79 around site i, made for the exits of align_gt_read that copies with one
        change hardly reach (as ksw_reference.verdict_batch makes them): four substitutions 9 apart (the score floor with no
        indel), two substitutions beside an insertion or a deletion (the floors with one), and an indel right of a site that
        lies in the read's left part, under the reference allele and under a third one (the second alignment from the site)"""
        w, out = self.genome[i - 39:i + 40], []
        third = next(c for c in "ACGT" if c not in (w[39], self.alt[i]))
        for a in (3, 9, 17):
            site = 39 - a
            for kind in ("subs", "ins", "del"):
                s = list(w[a:a + 50])
                for p in ((6, 15, 24, 33) if kind == "subs" else (8, 41)):
                    p += p == site
                    s[p] = _other(rng, s[p])
                if kind == "ins":
                    s[24:24] = [_other(rng, s[24], s[23])]
                elif kind == "del":
                    del s[24]
                out.append("".join(s))
        for a in (25, 26, 28):
            site = 39 - a
            for allele in (w[39], third):
                for kind in ("ins", "del"):
                    s = list(w[a:a + 50])
                    s[site] = allele
                    p = site + (9 if allele == w[39] else 5) + a % 3  # (9 matches or more are worth the gap's 7: exit 11)
                    if kind == "ins":
                        s[p:p] = [_other(rng, s[p], s[p - 1])]
                    else:
                        del s[p]
                    out.append("".join(s))
        # six symbols deleted left of the site: the rows of the tiles before the gap project the read's end six short of where
        # it is and fail the length rule, beside a row of a tile that covers the site (need 0 wins), or beside pending rows
        # of tiles behind the gap that stay
        for a in (0, 3):
            out += [w[a:20] + w[26:40], w[a:20] + w[26:41], w[a:20] + w[26:37], w[a:18] + w[24:38]]
        return out

    def unrelated(self, n=40):
        """reads in which no K_MIN-mer of any request occurs (so no tile and no lengthened leg of any parameter set)"""
        rng = random.Random(496)
        tiles = {w[j:j + K_MIN] for w, _, _, _ in self.reqs for j in range(len(w) - K_MIN + 1)}
        out = []
        while len(out) < n:
            r = "".join(rng.choice("ACGT") for _ in range(rng.randrange(30, 90)))
            if not any(r[j:j + K_MIN] in tiles for j in range(len(r) - K_MIN + 1)):
                out.append(r)
        return out + out[:3]


_RAGGED = []


def ragged_alleles():
    if not _RAGGED:
        _RAGGED.append(RaggedAlleles())
    return _RAGGED[0]


def deal_one(reads):
    return [list(reads)]


def deal_round_robin(reads, n=8):
    return [list(reads[i::n]) for i in range(n)]


def deal_halves(reads):
    return [list(reads[:len(reads) // 2]), list(reads[len(reads) // 2:])]


def deal_wide(ra):
    """four shards: the reads over 256 symbols in shards 1 and 3 by turns, the others over 0, 1 and 3, shard 2 unrelated"""
    shards = [[], [], ra.unrelated(), []]
    nl = ns = 0
    for r in ra.reads:
        if len(r) > WIDE:
            shards[(1, 3)[nl % 2]].append(r)
            nl += 1
        else:
            shards[(0, 1, 3)[ns % 3]].append(r)
            ns += 1
    return shards


DEALINGS = {"ragged-alleles": ("one", "wide4", "rr8"), "repeat": ("one", "halves"), "exact4096": ("with", "without")}
_INPUTS = {}


def get(oracle, name, dealing, ss=2, other=True):
    """the Input of a read set under a dealing (DEALINGS), built once"""
    key = (name, dealing, ss, other)
    if key in _INPUTS:
        return _INPUTS[key]
    unnamed, pairs = (), None
    if name == "ragged-alleles":
        ra = ragged_alleles()
        shards = {"one": deal_one, "rr8": deal_round_robin}[dealing](ra.reads) if dealing != "wide4" else deal_wide(ra)
        unnamed = shards[0] if dealing == "wide4" else ()
        reqs, alleles = ra.reqs, ra.alleles
    elif name == "repeat":
        rp = repeat()
        shards = {"one": deal_one, "halves": deal_halves}[dealing](rp.reads)
        reqs, alleles = rp.reqs, rp.alleles
    else:
        ex = exact4096()
        shards = ex.shards if dealing == "with" else [ex.shards[0], [r for r in ex.shards[1] if r != ex.big]]
        reqs, alleles = ex.reqs, []
        if dealing == "without":  # the same pair list: the pair that names `big` then finds no read
            pairs = get(oracle, name, "with", ss, other).pairs
    _INPUTS[key] = Input(oracle, f"{name}/{dealing}", shards, reqs, alleles, ss, other, unnamed, pairs)
    return _INPUTS[key]


# ---- repeat ---------------------------------------------------------------------------------------------------------
class Repeat:
    def __init__(self):
        fx = fixture("repeat")
        rng = random.Random(6)
        g = self.genome = fx.sources[0]
        self.reads = list(fx.shards[0])
        where = {}
        for name, rep in REPEATS.items():
            where[name] = (g.find(rep), g.find(rep) + len(rep))
        self.where = where
        reqs = []
        for n, (name, (a, b)) in enumerate(where.items()):  # through each repeat: the site inside it, and at an end of the window
            w = g[max(a - 10, 0):b + 10][:72]
            mid = len(w) // 2
            reqs.append((w, mid, _other(rng, w[mid - 1]), 0))
            if n % 2:
                reqs.append((w, len(w), _other(rng, w[-1]), 1) if n == 1 else (w, 1, _other(rng, w[0]), 1))
        ends = sorted(where.values())
        for (_, b), (a, _) in zip(ends, ends[1:]):  # the random stretches between them
            w = g[b + 5:a - 5][:90]
            reqs.append((w, len(w) // 2, _other(rng, w[len(w) // 2 - 1]), len(reqs) % 2))
        alleles = []
        for name in ("ACGT", "NINE"):  # both alleles at a site 3 symbols outside a repeat: most of the window lies inside
            i = where[name][1] + 3
            w, o = g[i - 60:i + 19], _other(rng, g[i])
            alleles.append((len(reqs), len(reqs) + 1))
            reqs += [(w, 61, o, 0), (w[:60] + o + w[61:], 61, g[i], 0)]
        twice = sorted({r for r in self.reads if self.reads.count(r) > 1}, key=lambda r: rng.random())
        inside = [r for r in twice if any(r in rep for rep in REPEATS.values())]
        for r in inside[:1] + [r for r in twice if r not in inside][:2]:  # whole duplicated reads as windows
            reqs.append((r, len(r) // 2, _other(rng, r[len(r) // 2 - 1]), 0))
        self.reqs, self.alleles = reqs, alleles


_REPEAT = []


def repeat():
    if not _REPEAT:
        _REPEAT.append(Repeat())
    return _REPEAT[0]


# ---- one read of exactly 4,096 symbols ------------------------------------------------------------------------------
class Exact4096:
    """a genome of 4,096 symbols that is itself a read (`big`), with a site at 2,040: shard 0 holds short reads over the
    site with both alleles, shard 1 -- the small shard of its own -- `big` and three more short reads.  Requests: both
    alleles in a window of 79 (big contains it and is a candidate; hanging 4,017 symbols out of it, it is no carrier), and
    the reference allele with all 4,096 symbols as the window: there big is a carrier"""

    def __init__(self):
        rng = random.Random(4096)
        g = self.big = "".join(rng.choice("ACGT") for _ in range(4096))
        i = self.site = 2040
        o = _other(rng, g[i])
        alt = g[:i] + o + g[i + 1:]
        short = []
        for n in range(9):
            ln = rng.randrange(40, 75)
            s = i - rng.randrange(5, ln - 5)
            short.append((alt if n % 3 == 2 else g)[s:s + ln])
        # (thirty reads that have nothing to do with it: sample_reference.sample_pairs wants a set with every kind of value)
        rest = ["".join(rng.choice("ACGT") for _ in range(rng.randrange(40, 75))) for _ in range(30)]
        self.shards = [short[:6] + short[:1] + rest, [short[6], self.big, short[7], short[8]]]
        w = g[i - 39:i + 40]
        self.reqs = [(w, 40, o, 0), (w[:39] + o + w[40:], 40, g[i], 0), (g, i + 1, o, 0)]
        assert len(self.big) == 4096 and w in self.big


_EXACT = []


def exact4096():
    if not _EXACT:
        _EXACT.append(Exact4096())
    return _EXACT[0]
