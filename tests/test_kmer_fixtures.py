"""CPU guards for the KmerMatch layout matrix (tests/test_gpu_kmer_layouts.py): the read sets, the window spans and the
query lists that module runs on the GPU are built here, where the CPU can see them, and held to what the GPU tests
rely on -- before anything runs on a GPU.

Every fixture is the run-byte array _bwt_runs(reads) of an explicit, seeded read list: a VALID BWT, so every LF walk
ends on a '$' row.  For every (fixture, shard, span) rsbwt_layout_selftest_host lays the runs out with the builder's
own code and gives {S, lines, far lines, chunk windows, far windows, spilled symbols}; LAYOUT_STATS below records them
(data measured once, asserted exactly here, and asserted against the GPU builder in the GPU module), and the layout's
kind is asserted from them:

    control   no continuation at all: far == chunk windows == spilled == 0
    chunk     spill chunks only: chunk windows > 0, far == 0
    chunk+    spill chunks in walked windows, far lines elsewhere allowed: chunk windows > 0
    far       far lines present: far > 0
    chain     far chains longer than one line: far > far windows > 0

The stats count windows of a kind but do not name them.  A group of 16 windows is laid out from its own symbols alone, so
the selftest of the run stream cut at every group boundary gives the counts per group (group_kinds below; the cut stream's
last figures are asserted to be the whole stream's).  "The walks really enter such windows" is then shown by counting: a
group of W windows, K of them of the kind and V of them visited, with V + K > W, holds a visited window of the kind.  The
guard asks for at least one such group, for the candidate rows and for the rows their LF walks visit.  (The rows of the
suffixes that begin with '$' -- the first num_strings rows -- are never visited by an LF walk, and their BWT symbols, the
reads' last symbols, have the shortest runs of the index: without this guard a "chunk" case could have every one of its
chunk windows there.)"""
import ctypes as C
import random

import numpy as np
import pytest

from kmer_reference import (Walks, _bwt_runs, _expected, _rc, _tiles, candidate_rows, expected_identities, identity, row_tiles)

MINL, MAXL = 73, 100                              # every (k, skip) of KS takes find_reads' row-walking branch
KS = [(8, 0), (12, 0), (15, 0), (15, 1), (20, 3), (12, 40), (31, 5)]
LONG_MINL, LONG_MAXL = 50, 70                     # ... and these the other branches (k >= min_read_length)
LONG_KS = [(50, 0), (60, 5), (70, 1)]
GROUP = 16                                        # windows per group of the line layout (line_format.h)


def _rand(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


class Fixture:
    def __init__(self, name, shards, sources, ks, extra=()):
        self.name, self.shards, self.sources, self.ks, self.extra = name, shards, sources, ks, list(extra)
        self._runs = None

    def runs(self):
        if self._runs is None:
            self._runs = [_bwt_runs(r) for r in self.shards]
        return self._runs

    def queries(self, k, skip):
        """one call's queries: cut from a read at every offset 0 .. skip + 1 from its start, cut from the middle of the
        sources, reverse complements, one query twice, an N in the middle, an N at position `skip`, the fixture's own"""
        rng = random.Random(f"{self.name}/{k}/{skip}")
        step = skip + 1
        reads = sorted({r for sh in self.shards for r in sh if len(r) >= min(k + 2 * step, 70)})
        r = reads[rng.randrange(len(reads))]
        out = [r[off:off + 60] for off in range(step + 1)]
        mids = []
        for _ in range(4):
            src = self.sources[rng.randrange(len(self.sources))]
            s = rng.randrange(len(src) - 100)
            mids.append(src[s:s + 100])
        out += mids + [_rc(mids[0]), _rc(mids[1]), mids[0]]
        out.append(mids[2][:50] + "N" + mids[2][51:])
        out.append(mids[3][:skip] + "N" + mids[3][skip + 1:])
        # a read that starts at the second tile: its row meets '$' inside the check steps
        first = rng.randrange(len(reads))
        src, at = next((s, s.find(r2)) for r2 in reads[first:] + reads[:first] for s in self.sources if s.find(r2) >= step)
        out.append(src[at - step:at - step + 60])
        return out + self.extra


def _pop():
    """reads of 70 drawn from 4 haplotypes (SNP rate 0.004) of a seeded genome, two shards"""
    rng = random.Random(1101)
    genome = _rand(rng, 12000)
    haps = []
    for _ in range(4):
        s = list(genome)
        for i in range(len(s)):
            if rng.random() < 0.004:
                s[i] = rng.choice([c for c in "ACGT" if c != s[i]])
        haps.append("".join(s))
    reads = []
    for _ in range(1300):
        h = haps[rng.randrange(4)]
        s = rng.randrange(len(h) - 70 + 1)
        reads.append(h[s:s + 70])
    return Fixture("pop", [reads[0::2], reads[1::2]], haps, KS)


REPEATS = {"ACGT": "ACGT" * 30, "A": "A" * 45, "AC": "AC" * 35, "NINE": "GATTCCAGT" * 8}


def _repeat():
    """a genome that embeds the tandem repeats between random stretches; reads of 50..70 from every start position, and
    every ninth read once more (exact duplicates)"""
    rng = random.Random(2202)
    genome, at = _rand(rng, 150), {}
    for name, rep in REPEATS.items():
        at[name] = (len(genome), len(genome) + len(rep))
        genome += rep + _rand(rng, 120)
    reads = []
    for s in range(len(genome) - 50):
        ln = 50 + (s * 5) % 21
        reads.append(genome[s:s + ln])
    reads += reads[::9]
    stretches = [genome[a - 10:b + 10] for a, b in at.values()]
    # (12, 8): skip + 1 = the 9-mer's period; (15, 1) and (20, 3) of KS are the periods 2 and 4; (10, 2): coprime to 2 and 4
    return Fixture("repeat", [reads], [genome], KS + [(12, 8), (10, 2)], stretches)


RAGGED_SHORT = list(range(12, 38)) + [53]
RAGGED_LONG = [256, 257, 258, 260, 270, 280, 300, 320, 350, 380, 400, 420, 450, 480, 500, 511, 512, 513, 520, 540, 560, 580, 599, 600]


def _ragged():
    """read lengths 12 .. 600: reads shorter than k, of exactly k, of k + 1 .. k + skip for the (k, skip) of KS, 24 reads of
    256 .. 600 symbols, and prefixes / suffixes of other reads"""
    rng = random.Random(3303)
    genome = _rand(rng, 12000)
    reads, short = [], []
    for ln in RAGGED_SHORT:
        for _ in range(6):
            s = rng.randrange(len(genome) - ln)
            reads.append(genome[s:s + ln])
        short.append(reads[-1])
    for _ in range(420):
        ln = rng.randrange(40, 121)
        s = rng.randrange(len(genome) - ln)
        reads.append(genome[s:s + ln])
    longs = []
    for ln in RAGGED_LONG:
        s = rng.randrange(len(genome) - ln)
        longs.append(genome[s:s + ln])
    reads += longs
    for r in reads[150:180] + longs[:4]:
        reads += [r[:len(r) // 2], r[len(r) // 3:]]
    rng.shuffle(reads)
    # the fixture's own queries: whole short reads, and two cut from inside reads longer than 256 / 512 symbols
    extra = short + [longs[6][100:200], longs[-1][350:450]]
    fx = Fixture("ragged", [reads], [genome], KS, extra)
    fx.longs = longs
    return fx


_BUILT = {}


def fixture(name):
    if name not in _BUILT:
        _BUILT[name] = {"pop": _pop, "repeat": _repeat, "ragged": _ragged}[name]()
    return _BUILT[name]


# ---- the layouts of the GPU matrix ----------------------------------------------------------------------------------
# (fixture, kind, window span, for_reads, ktab_depth); span 0 is the builder's choice, known only on the GPU: the GPU module
# runs the selftest at g.window_span()
LAYOUTS = []  # filled below from SPANS
SPANS = {
    "pop": {"control": 40, "chunk": 128, "far": 300, "chain": 600, "deep": 2944},
    "repeat": {"control": 40, "chunk": 270, "far": 320, "chain": 600, "deep": 2944},
    "ragged": {"control": 40, "chunk": 128, "far": 300, "chain": 600, "deep": 2944},
}
for _fx, _sp in SPANS.items():
    LAYOUTS.append((_fx, "auto", 0, True, 6))
    for _kind in ("control", "chunk", "far", "chain", "deep"):
        # (repeat and ragged have no span with spill chunks in walked windows and no far line anywhere: their '$' block
        # takes far lines first -- "chunk+": chunk windows proven walked, far lines allowed)
        LAYOUTS.append((_fx, "chunk+" if _kind == "chunk" and _fx != "pop" else _kind, _sp[_kind], True, 6))
    LAYOUTS.append((_fx, "far", _sp["far"], True, None))
    LAYOUTS.append((_fx, "deep", _sp["deep"], True, None))
    # rsbwt_set_kmer_reads accepts shards opened without RSBWT_OPEN_READS (the plain layout: 96 pieces a line, select
    # side table): two spans of it
    LAYOUTS.append((_fx, "far", _sp["far"], False, 6))
    LAYOUTS.append((_fx, "deep", _sp["deep"], False, 6))

# (fixture, shard, span, for_reads) -> [S, lines, far lines, chunk windows, far windows, spilled symbols]
LAYOUT_STATS = {
    ('pop', 0, 128, True): [128, 391, 0, 10, 0, 138],
    ('pop', 0, 2944, False): [2944, 157, 140, 0, 16, 41313],
    ('pop', 0, 2944, True): [2944, 158, 141, 0, 16, 41707],
    ('pop', 0, 300, False): [300, 181, 11, 17, 8, 1499],
    ('pop', 0, 300, True): [300, 185, 15, 44, 12, 2555],
    ('pop', 0, 40, True): [40, 1241, 0, 0, 0, 0],
    ('pop', 0, 600, True): [600, 187, 102, 0, 77, 23992],
    ('pop', 1, 128, True): [128, 391, 0, 8, 0, 86],
    ('pop', 1, 2944, False): [2944, 157, 140, 0, 16, 41420],
    ('pop', 1, 2944, True): [2944, 161, 144, 0, 16, 41934],
    ('pop', 1, 300, False): [300, 180, 10, 16, 7, 1480],
    ('pop', 1, 300, True): [300, 184, 14, 38, 10, 2283],
    ('pop', 1, 40, True): [40, 1241, 0, 0, 0, 0],
    ('pop', 1, 600, True): [600, 186, 101, 0, 77, 23843],
    ('ragged', 0, 128, True): [128, 443, 1, 9, 1, 93],
    ('ragged', 0, 2944, False): [2944, 167, 133, 0, 18, 44909],
    ('ragged', 0, 2944, True): [2944, 167, 133, 0, 18, 45482],
    ('ragged', 0, 300, False): [300, 197, 10, 5, 7, 1118],
    ('ragged', 0, 300, True): [300, 197, 10, 10, 7, 1479],
    ('ragged', 0, 40, True): [40, 1377, 0, 0, 0, 0],
    ('ragged', 0, 600, True): [600, 196, 94, 1, 85, 22342],
    ('repeat', 0, 270, True): [270, 244, 6, 4, 4, 695],
    ('repeat', 0, 2944, False): [2944, 84, 50, 0, 20, 32703],
    ('repeat', 0, 2944, True): [2944, 85, 51, 0, 20, 35221],
    ('repeat', 0, 320, False): [320, 212, 8, 1, 6, 870],
    ('repeat', 0, 320, True): [320, 212, 8, 2, 6, 1112],
    ('repeat', 0, 40, True): [40, 1598, 0, 0, 0, 0],
    ('repeat', 0, 600, True): [600, 130, 11, 2, 5, 2443],
}


def layout_id(lay):
    fx, kind, span, room, ktab = lay
    return f"{fx}-{kind}-S{span}-{'reads' if room else 'plain'}-ktab{ktab}"


def selftest(rsb, runs, span, room):
    st = (C.c_uint64 * 6)()
    bad = C.c_uint64()
    rc = rsb.lib().rsbwt_layout_selftest_host(runs.ctypes.data, runs.size, span | ((1 << 31) if room else 0), st, C.byref(bad))
    assert rc == 0, f"first disagreement at position {bad.value}"
    return [int(x) for x in st]


def group_kinds(rsb, runs, span, room, whole):
    """per group of 16 windows: (windows, chunk windows, far windows) -- the selftest's counts of the run stream cut at the
    group's end, less those of the stream cut at its start"""
    lens = (runs & 31).astype(np.int64)
    cum = np.cumsum(lens)
    n = int(cum[-1])
    out, prev = [], (0, 0)
    for end in range(GROUP * span, n + GROUP * span, GROUP * span):
        end = min(end, n)
        j = int(np.searchsorted(cum, end, side="right"))
        cut = runs[:j]
        rest = end - (int(cum[j - 1]) if j else 0)
        if rest:
            cut = np.append(cut, np.uint8((runs[j] & 0xE0) | rest))
        st = selftest(rsb, np.ascontiguousarray(cut), span, room)
        start = end - 1 - (end - 1) % (GROUP * span)
        out.append(((end - start + span - 1) // span, st[3] - prev[0], st[4] - prev[1]))
        assert st[3] >= prev[0] and st[4] >= prev[1]
        prev = (st[3], st[4])
    assert st == whole  # (the last cut is the whole stream)
    return out


def assert_kind(kind, st):
    S, nlines, far, chunkw, farw, spilled = st
    if kind == "control":
        assert far == chunkw == spilled == 0, st
    elif kind == "chunk":
        assert chunkw > 0 and far == 0, st
    elif kind == "chunk+":
        assert chunkw > 0, st
    elif kind == "far":
        assert far > 0 and farw > 0, st
    elif kind in ("chain", "deep"):
        assert far > farw > 0, st
        if kind == "deep":
            assert far > 2 * farw, st  # some chain has three lines or more: `tries` counts up


_CPU_LAYOUTS = sorted({(fx, kind, span, room) for fx, kind, span, room, _ in LAYOUTS if span})


@pytest.fixture(scope="module")
def walked(oracle):
    """per fixture and shard: the oracle index, the candidate rows of every query of every (k, skip) of the GPU matrix, and
    every row their LF walks visit"""
    out = {}

    def get(name):
        if name not in out:
            fx = fixture(name)
            per = []
            for sh, runs in zip(fx.shards, fx.runs()):
                oix = oracle.from_runs(runs, len(sh))
                wk = Walks(oix)
                cand = set()
                for k, skip in fx.ks:
                    for w in fx.queries(k, skip):
                        rows = candidate_rows(oix, w, k, skip, MAXL)
                        cand.update(rows)
                        for r in rows:
                            wk.rows(r)
                per.append((oix, wk, cand))
            out[name] = per
        return out[name]
    return get


@pytest.mark.parametrize("name,kind,span,room", _CPU_LAYOUTS, ids=[f"{a}-{b}-S{c}-{'reads' if d else 'plain'}" for a, b, c, d in _CPU_LAYOUTS])
def test_layout_is_the_kind_the_gpu_case_means(rsb, walked, name, kind, span, room):
    """the builder's own stats at this span are the recorded ones and of the case's kind, and the candidate rows and the rows
    their LF walks visit lie in windows of that kind (module docstring: by counting)"""
    fx = fixture(name)
    shown = {}
    for p, runs in enumerate(fx.runs()):
        st = selftest(rsb, runs, span, room)
        assert st == LAYOUT_STATS[(name, p, span, room)], (name, p, span, room, st)
        assert st[0] == span
        assert_kind(kind, st)
        if kind == "control":
            continue
        n = int((runs & 31).astype(np.int64).sum())
        _, wk, cand = walked(name)[p]
        groups = group_kinds(rsb, runs, span, room, st)
        for what, rows in (("candidate rows", cand), ("visited rows", wk.next.keys())):
            seen = {}
            for w in {r // span for r in rows}:
                seen[w // GROUP] = seen.get(w // GROUP, 0) + 1
            proven = [g for g, (W, chunkw, farw) in enumerate(groups)
                      if seen.get(g, 0) + (chunkw if kind.startswith("chunk") else farw) > W]
            shown[what] = shown.get(what, 0) + len(proven)
    if kind != "control":
        assert shown.get("candidate rows") and shown.get("visited rows"), (name, kind, span, shown)


def _all_ks(fx):
    return [(k, s, MINL, MAXL) for k, s in fx.ks] + [(k, s, LONG_MINL, LONG_MAXL) for k, s in LONG_KS]


@pytest.mark.parametrize("name", ["pop", "repeat", "ragged"])
def test_expected_identities_agree_with_the_string_reference(oracle, name):
    """the reads at expected_identities, as a set of strings, are _expected minus the sub-tile reads of long tiles -- for
    every fixture, request and query of the GPU matrix: the new reference is pinned to the trusted one"""
    fx = fixture(name)
    for sh, runs in zip(fx.shards, fx.runs()):
        oix = oracle.from_runs(runs, len(sh))
        wk = Walks(oix)
        for k, skip, minl, maxl in _all_ks(fx):
            for w in fx.queries(k, skip):
                ids = expected_identities(oix, [w], k, skip, minl, maxl, walks=wk)
                strings = {"".join(oix.extract(r, cap=1 << 12)) for r in ids}
                rows_only = set()
                for t in row_tiles(w, k, skip, maxl):
                    lo, up = oix.find_interval(t)
                    rows_only |= {"".join(oix.extract(r)) for r in range(lo, up + 1)}
                assert strings == rows_only, (name, k, skip, w)
                exp = _expected(oix, w, k, skip, minl, maxl)
                assert strings <= exp
                subtile = {x for t in _tiles(w, k, skip) if len(t) >= minl for ln in (minl, maxl) for x in _tiles(t, ln, 0)}
                assert exp - strings <= subtile, (name, k, skip, w)
                if k < minl:
                    assert strings == exp
                assert all(r in sh for r in strings)
        # the cached walk is the plain one
        some = sorted(wk.next)[::97]
        assert all(wk.identity(r) == identity(oix, r) for r in some)


def test_fixtures_hold_the_cases_the_issue_names(oracle):
    """computed from the read lists and the oracle alone: duplicates, the ragged lengths, over-long reads, '$' met inside
    the skip + 1 check steps, and -- on the repeats -- more than one candidate row per identity"""
    pop, rep, rag = fixture("pop"), fixture("repeat"), fixture("ragged")
    assert len(pop.shards) == 2 and all(len(r) == 70 for sh in pop.shards for r in sh)
    reads = rep.shards[0]
    assert len(reads) >= len(set(reads)) + 90 and all(50 <= len(r) <= 70 for r in reads)
    assert all(any(r in s or s in r for r in reads) for s in REPEATS.values())  # reads wholly inside a repeat (or, "A" * 45, around it)
    assert all(any(r in REPEATS[x] for r in reads) for x in ("ACGT", "AC", "NINE"))
    lens = {len(r) for r in rag.shards[0]}
    for k, skip in KS[1:]:
        assert k in lens and (k == min(lens) or any(x < k for x in lens)) and all(k + d in lens for d in range(1, min(skip, 6) + 1)), (k, skip)
    assert sum(1 for r in rag.shards[0] if len(r) > 256) >= 20 and sum(1 for r in rag.shards[0] if len(r) > 512) >= 5
    assert min(lens) == 12 and max(lens) == 600 and {256, 257} <= lens
    rs = set(rag.shards[0])
    assert sum(1 for r in rs if any(o != r and o.startswith(r) for o in rs)) >= 20
    assert sum(1 for r in rs if any(o != r and o.endswith(r) for o in rs)) >= 20
    for fx in (pop, rep, rag):
        ows = [(o, Walks(o)) for o in (oracle.from_runs(r, len(sh)) for sh, r in zip(fx.shards, fx.runs()))]
        for k, skip in fx.ks:
            step, early = skip + 1, 0
            for w in fx.queries(k, skip):
                if len(w) < k + step or not set(w[:k + step]) <= set("ACGT"):
                    continue
                for oix, wk in ows:
                    lo, up = oix.find_interval(w[step:step + k])  # the tile at p = skip + 1: its predecessor is the tile at 0
                    early += sum(1 for r in range(lo, up + 1) if wk.steps(r) < step)
            assert early > 0, (fx.name, k, skip, "no walk meets '$' inside the check steps")
    # a read that IS a tile, and reads shorter than k + skip + 1 among the matches
    oix = oracle.from_runs(rag.runs()[0], len(rag.shards[0]))
    for k, skip in KS[1:]:
        qs = rag.queries(k, skip)
        assert any(len(w) == k and w in rs for w in qs), (k, "no query is a whole read of k symbols")
        assert any(len(x) < k + skip + 1 for w in qs for x in _expected(oix, w, k, skip)), (k, skip)
    # the repeat stretches: chains inside one segment / cycles of tiles with real hits
    oix = oracle.from_runs(rep.runs()[0], len(reads))
    wk = Walks(oix)
    for k, skip in rep.ks:
        for w in rep.extra:
            rows = candidate_rows(oix, w, k, skip, MAXL)
            ids = {wk.identity(r) for r in rows}
            assert len(rows) > len(ids) > 0, (k, skip, w[:20])
    tiles = set(_tiles(REPEATS["ACGT"], 8, 0))
    assert len(tiles) == 4  # "ACGT" * n at skip = 0: T0 -> T3 -> T2 -> T1 -> T0
    for k, skip, rp in ((15, 1, "AC"), (20, 3, "ACGT"), (12, 8, "NINE"), (8, 0, "A")):
        assert REPEATS[rp][skip + 1:skip + 1 + k] == REPEATS[rp][:k]  # the predecessor tile is the tile itself
