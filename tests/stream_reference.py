"""Inputs beyond the gt fixture for the matching-statistics and overlap tests -- TEST INFRASTRUCTURE, CPU only.  Seeded run
streams in the shapes of tools/fuzz_parity.py:make_runs (symbols 0..4, about 6,000 run bytes), three degenerate streams,
the `repeat` and `ragged` read sets of tests/test_kmer_fixtures.py, seeded query batches for each of them in two sizes,
and the expected values of match_reference / overlap_reference over the oracle, computed once per key.

A run stream that is no BWT of reads has no string-level truth: there the restatement over the oracle IS the definition.
Half of a stream's queries are spelled from the stream itself (LF walks with the oracle's char and occ), so that their
backward searches stay alive for tens of steps on a stream where a random string dies after a few.

tests/test_stream_reference.py shows on the CPU what these inputs reach; tests/test_gpu_match_streams.py and
tests/test_gpu_overlap_streams.py run them on the GPU.  The SiteMatch batches of the same sources (gt_queries, GT_PARAMS,
gt_expected, gt_narrow_steps) are further down: tests/test_gt_stream_reference.py and tests/test_gpu_gt_streams.py."""
import random

import numpy as np

import gt_reference as G
import match_reference as M
import overlap_reference as O
import test_kmer_fixtures as F
from oracle_binding import expand_runs

RUN_BYTES = 6000
# (100,000 symbols at the most; runs of 1..2 make 1.5 symbols a byte: more bytes, or a random 7-mer is hardly ever there)
SIZES = {"all31": 3200, "synth-long": 3800, "short": 16000, "nodollar": 1500, "dollar-ends": 1500}
SYNTH_STYLES = {"synth-mixed": 0, "synth-long": 1 << 63, "synth-pop": 1 << 62}  # (tools/fuzz_parity.py: the library's own generators)
SHAPED = ("uniform", "all31", "short", "dollars", "stripes") + tuple(SYNTH_STYLES)
DEGENERATE = ("single", "nodollar", "dollar-ends")
STREAMS = SHAPED + DEGENERATE
FIXTURES = ("repeat", "ragged")
BATCHES = {"small": 12, "wide": 400}  # spelled queries = random queries of a batch
WIDE_POSITIONS = 20500
ACGT = "ACGT"
MAX_QUERY = 100                       # on the read sets: the reference asks for l^2 / 2 searches along a match of l symbols
MAX_READS = {"repeat": 20, "ragged": 2}  # cuts some (query, shard) pairs of the read set and leaves others whole
READ_PARAMS = [(1, 0), (6, 0), (10, 30)]  # the pairs the reads call runs at: every depth (a read met at two overlap lengths), two deeper ones
READ_STRIDE = {"repeat": 128, "ragged": 640}
SPILLING = ("short",)                 # the most run bytes per window: spill chunks at span 128, far lines from 300 on
FAR_AT_DEEP = ("short", "uniform", "dollars")  # (16 symbols a run byte: far lines only at span 2944)
LEAD = 40                             # the '$'-less stream begins with this many runs of T: its first rows see no A before them


def _seed(name):
    return [ord(c) for c in name]


def make_runs(name, rsb=None):
    """the run bytes of stream `name`; the synth-* streams come from the library's host generator"""
    rng = np.random.default_rng(_seed(name))
    R = SIZES.get(name, RUN_BYTES)
    if name in SYNTH_STYLES:
        runs = np.empty(R, np.uint8)
        assert rsb.lib().rsbwt_synth_runs_host(runs.ctypes.data, R, int(rng.integers(1, 1 << 30)) | SYNTH_STYLES[name]) == 0
        return runs
    if name == "single":
        return np.array([(2 << 5) | 17], np.uint8)
    sym = rng.integers(0, 5, R)
    ln = rng.integers(1, 32, R)
    if name == "all31":
        ln[:] = 31
    elif name == "short":
        ln = rng.integers(1, 3, R)
    elif name == "dollars":
        # 30 % of the runs are '$', but not evenly: three in four over the first 3/8 of the stream (neighbouring '$' runs
        # make stripes of '$' that cross quarters and lines), 3 in 100 after it.  Spread evenly, '$' would end every LF walk
        # within twenty steps and no suffix of overlap_reference.PARAMS' deeper pairs could open a read.
        sym = rng.integers(1, 5, R)
        sym[rng.random(R) < np.where(np.arange(R) < 3 * R // 8, 0.75, 0.03)] = 0
    elif name == "stripes":
        sym = np.where(rng.random(R) < 0.995, 1 + (np.arange(R) // 5000) % 4, sym)
    elif name == "nodollar":
        sym = rng.integers(1, 5, R)
        sym[:LEAD] = 4
    elif name == "dollar-ends":
        sym[0] = sym[-1] = 0
    else:
        assert name == "uniform", name
    return ((sym << 5) | ln).astype(np.uint8)


def _depths(runs, cap=70):
    """per row: min(cap, the LF steps a walk from it takes before it meets '$')"""
    bwt = expand_runs(runs).astype(np.int64)
    tot = np.bincount(bwt, minlength=5)
    first = np.concatenate([[0], np.cumsum(tot)[:-1]])
    rank = np.zeros(bwt.size, np.int64)
    for c in range(5):
        at = bwt == c
        rank[at] = np.arange(int(at.sum()))
    lf = first[bwt] + rank
    d = np.zeros(bwt.size, np.int64)
    for _ in range(cap):
        d = np.where(bwt != 0, 1 + d[lf], 0)
    return d


class Source:
    """one shard of the tests: its run bytes, its oracle side, and -- for a read set -- the reads"""

    def __init__(self, name, runs, reads, oracle):
        self.name, self.runs, self.reads = name, runs, reads
        self.num_strings = len(reads) if reads is not None else 0
        self.orc = G.OracleShard(oracle.from_runs(runs, self.num_strings))
        self.n = self.orc.oix.bwlen()
        self.plain = O.PlainSide(reads) if reads is not None else None
        self._depths = None

    def depths(self):
        if self._depths is None:
            self._depths = _depths(self.runs)
        return self._depths


_SOURCES = {}


def source(name, oracle, rsb=None):
    if name not in _SOURCES:
        if name in FIXTURES:
            fx = F.fixture(name)
            _SOURCES[name] = Source(name, fx.runs()[0], fx.shards[0], oracle)
        else:
            _SOURCES[name] = Source(name, make_runs(name, rsb), None, oracle)
    return _SOURCES[name]


def spell(oix, row, steps):
    """walk LF(r) = C[c] + Occ(c, r) - 1 from `row` for `steps` steps, stopping at '$'; the reversed spelling: a string
    whose backward search passes through every row of the walk"""
    out = []
    for _ in range(steps):
        c = oix.char(row)
        if c == "$":
            break
        out.append(c)
        row = oix.pc(c) + oix.occ(c, row) - 1
    return "".join(reversed(out))


def suffix_at(oix, row, m):
    """the first m symbols of the suffix at `row` (the walk against LF: getF and getOccAt), stopping at '$': a string whose
    interval holds `row`"""
    out = []
    for _ in range(m):
        f = oix.f(row)
        if f == "$":
            break
        out.append(f)
        row = oix.occ_at(f, row - oix.pc(f) + 1)
    return "".join(out)


def _rand(rng, n, alphabet=ACGT):
    return "".join(rng.choice(alphabet) for _ in range(n))


def _substituted(rng, w):
    at = rng.randrange(len(w))
    return w[:at] + rng.choice([c for c in ACGT if c != w[at]]) + w[at + 1:]


def _random_query(rng, i):
    # every fourth random string is half N: the positions of length 0, and the walks that end at a symbol outside ACGT
    return _rand(rng, rng.randint(1, 70), "ACGTNNNN" if i % 4 == 3 else ACGT)


def _with_empties(rng, body, positions=0):
    rng.shuffle(body)
    i = 0
    while sum(len(w) for w in body) < positions:
        body.append(_random_query(rng, i))
        i += 1
    mid = len(body) // 2
    return [""] * 3 + body[:mid] + [""] * 3 + body[mid:] + [""] * 4


def _stream_queries(src, batch):
    rng = random.Random(f"{src.name}/{batch}")
    half = BATCHES[batch]
    oix, n = src.orc.oix, src.n
    depth = src.depths()
    deep = np.flatnonzero(depth >= 20)
    if deep.size < half:  # (hardly a walk of 20 steps: the rows whose walks run deepest)
        deep = np.argsort(-depth, kind="stable")[:half]
    # walks that meet '$' after 42..69 steps: whole "reads" of the stream, longer than the deepest min_overlap of the tests
    ending = np.flatnonzero((depth >= 42) & (depth < 70))
    body = []
    for i in range(half):
        if i % 2 and ending.size >= half:
            w = spell(oix, int(ending[rng.randrange(len(ending))]), 70)
        else:
            w = spell(oix, int(deep[rng.randrange(len(deep))]), rng.randint(20, 70))
        if i % 3 == 0 and w:
            w = _substituted(rng, w)
        else:
            _SPELLED.setdefault((src.name, batch), []).append(w)
        body.append(w)
    body += [_random_query(rng, i) for i in range(half)]
    # the two ends of the rows that begin with a base: strings whose intervals touch them, and those one symbol longer
    for row in (oix.pc("A"), n - 1):
        x = suffix_at(oix, row, 8) if row < n else ""
        if x:
            body += [x] + [c + x for c in ACGT]
    w = spell(oix, int(deep[0]), 40) or "ACGT"
    body += ["", "A", "N", w[:len(w) // 2] + "N" + w[len(w) // 2 + 1:]]
    return _with_empties(rng, body, WIDE_POSITIONS if batch == "wide" else 0)


def _read_queries(src, batch):
    """cut from the sources, whole reads, and reads extended by random symbols on the left (where an overlap with a whole
    read appears)"""
    rng = random.Random(f"{src.name}/{batch}")
    third = {"small": 10, "wide": 230}[batch]
    fx = F.fixture(src.name)
    reads = sorted({r for r in src.reads if len(r) <= MAX_QUERY - 20})
    body = []
    for i in range(third):
        s = fx.sources[rng.randrange(len(fx.sources))]
        ln = rng.randint(20, 70)
        at = rng.randrange(len(s) - ln)
        body.append(_substituted(rng, s[at:at + ln]) if i % 5 == 0 else s[at:at + ln])
    body += [reads[rng.randrange(len(reads))] for _ in range(third)]
    body += [_rand(rng, rng.randint(1, 20)) + reads[rng.randrange(len(reads))] for _ in range(third)]
    body += [_random_query(rng, 3) for _ in range(third // 8)]
    w = reads[0]
    body += ["", "A", "N", w[:len(w) // 2] + "N" + w[len(w) // 2 + 1:]]
    return _with_empties(rng, body)


_QUERIES = {}
_SPELLED = {}


def spelled(src, batch):
    """the spelled queries of the batch that no substitution touched"""
    queries(src, batch)
    return _SPELLED[(src.name, batch)]


def queries(src, batch):
    if (src.name, batch) not in _QUERIES:
        _QUERIES[(src.name, batch)] = (_read_queries if src.reads is not None else _stream_queries)(src, batch)
    return _QUERIES[(src.name, batch)]


# ---- the expected values, once per (stream, batch, parameters): the oracle calls dominate the cost

def match_expected(srcs, batch_key, qs, max_len, min_rows):
    """(len [S][N] u32, lower, upper [S][N] u64, (SMEM records, first), exp) over the shards `srcs`"""
    exp = [M.expected([s.orc], (s.name, batch_key), qs, max_len, min_rows)[0] for s in srcs]
    ln, lo, up = M.flat(exp)
    return np.array(ln, np.uint32), np.array(lo, np.uint64), np.array(up, np.uint64), M.smem_records(exp), exp


def overlap_expected(srcs, batch_key, qs, min_overlap, max_overlap):
    """(count [S][N], ordinal [S][N] u64, (records, first), exp) over the shards `srcs`"""
    exp = [O.expected([s.orc], (s.name, batch_key), qs, min_overlap, max_overlap)[0] for s in srcs]
    cnt, od = O.flat(exp)
    return np.array(cnt, np.uint64), np.array(od, np.uint64), O.records(exp, qs), exp


_STEPS = {}


def overlap_lf_steps(srcs, batch_key, qs, max_overlap):
    """the LF steps of the walks without a table, per shard"""
    out = []
    for s in srcs:
        at = (s.name, batch_key, max_overlap)
        if at not in _STEPS:
            _STEPS[at] = O.total_lf_steps([s.orc], qs, max_overlap)
        out.append(_STEPS[at])
    return out


# ---- SiteMatch candidates (gt_reference) beyond the gt fixture: tests/test_gt_stream_reference.py shows on the CPU what
# these batches reach, tests/test_gpu_gt_streams.py runs them on the GPU

# (M, k, skip).  A run stream has 10^5 symbols at the most, where an 8-mer is nearly unique: lengthening needs k of 3 to 4,
# and k below the table depth of 6 makes right growth cross it.  A read set is a BWT of reads, where the gt fixture's k do.
# (k = 3 at skip = 1: at skip = 2 a batch of 60 queries of 70 symbols at the most has under 384 tiles, and the item grid of
# the smallest k would not reach a fourth workgroup of 256 lanes)
GT_PARAMS = {"stream": [(1, 8, 0), (8, 4, 0), (50, 3, 1), (3, 12, 3)], "reads": [(1, 8, 0), (3, 12, 3), (8, 20, 1)]}
GT_SHORT = "AC"  # shorter than every k used


def gt_params(src):
    return GT_PARAMS["reads" if src.reads is not None else "stream"]


def _gt_pos(rng, i, L):
    """the site cycles through 1, the middle, L, 0 (every tile on the right), L + 1 (past the end: no tiles), a random one"""
    return (1, L // 2, L, 0, L + 1, rng.randint(0, L))[i % 6]


def _gt_corner_queries(src, rng):
    """two symbols in front of a string whose interval touches an end of the rows that begin with a base, for all 16 pairs:
    where the first step leaves the reference's (0, 2^64 - 1), the search has symbols left; three of them inside a spelled
    query, where LEFT, RIGHT and COVERING tiles hold them"""
    oix, n = src.orc.oix, src.n
    xs = [suffix_at(oix, oix.pc("A"), 7), suffix_at(oix, n - 1, 7)]
    out = []
    for x in xs:
        for i, (c1, c2) in enumerate((c1, c2) for c1 in ACGT for c2 in ACGT):
            w = c2 + c1 + x
            out.append((w, 1 if i % 2 == 0 else len(w)))
    depth = src.depths()
    host = spell(oix, int(np.argmax(depth)), 60)
    host = (host + _rand(rng, 60))[:60]
    for c2, c1, x in (("C", "A", xs[0]), ("G", "A", xs[0]), ("T", "A", xs[1])):
        w = host[:26] + c2 + c1 + x + host[26:]
        out.append((w[:70], 30))
    return out


def _gt_stream_queries(src):
    rng = random.Random(f"gt/{src.name}/small")
    oix = src.orc.oix
    depth = src.depths()
    deep = np.argsort(-depth, kind="stable")[:64]
    body = []
    for i in range(6):  # spelled, every third with a substitution
        w = ""
        for _ in range(8):  # (where a walk meets '$' early: several spellings end to end, 70 symbols in all)
            w += spell(oix, int(deep[rng.randrange(len(deep))]), 70 - len(w))
        w = (w + _rand(rng, 70))[:70]
        body.append(_substituted(rng, w) if i % 3 == 0 else w)
    body += [_rand(rng, rng.randint(40, 70)) for _ in range(2)] + [_rand(rng, 70, "ACGTNNNN")]
    body = [(w, _gt_pos(rng, i, len(w))) for i, w in enumerate(body)]
    body += _gt_corner_queries(src, rng)
    if src.name == "single":
        body += [("CCCCCCCCA", 1), ("ACCCCCCCC", 9), ("CCCCACCCC", 5)]
    w = spell(oix, int(deep[0]), 70) or "ACGT" * 10
    w = (w + _rand(rng, 40))[:max(len(w), 40)]
    h = len(w) // 2
    # an N in a tile; a lengthening that runs into an N: a spelled (hence frequent) stretch with an N on either side of it
    body += [(GT_SHORT, 1), (w[:h] + "N" + w[h + 1:], h), (w[:4] + "N" + w[5:h] + "N" + w[h + 1:], 1)]
    return body


def _gt_read_queries(src):
    rng = random.Random(f"gt/{src.name}/small")
    fx = F.fixture(src.name)
    body = []
    for i in range(12):  # windows of the sources, every fifth with a substitution
        s = fx.sources[rng.randrange(len(fx.sources))]
        ln = rng.randint(30, MAX_QUERY)
        at = rng.randrange(len(s) - ln)
        body.append(_substituted(rng, s[at:at + ln]) if i % 5 == 0 else s[at:at + ln])
    for s in fx.extra[-6:] if src.name == "repeat" else ():  # the tandem repeats: intervals far above every M
        body.append(s[:MAX_QUERY])
    reads = sorted({r for r in src.reads if len(r) <= 80})
    body += [reads[rng.randrange(len(reads))] for _ in range(8)]
    if src.name == "repeat":  # whole reads that the shard holds twice
        twice = sorted({r for r in reads if src.reads.count(r) >= 2})
        body += [twice[rng.randrange(len(twice))] for _ in range(6)]
    if src.name == "ragged":  # from the inside of the reads of 256 to 600 symbols: the kept reads include those
        for r in sorted(fx.longs, key=len)[::4]:
            at = rng.randrange(20, len(r) - 90)
            body.append(r[at:at + rng.randint(40, 70)])
    body = [(w, _gt_pos(rng, i, len(w))) for i, w in enumerate(body)]
    w = fx.sources[0][200:280]
    body += [(GT_SHORT, 1), (w[:40] + "N" + w[41:], 40), (w[:10] + "N" + w[11:50] + "N" + w[51:], 1)]
    return body


_GT_QUERIES = {}


def gt_queries(src, batch="small"):
    """[(w, pos)]: the batch of SiteMatch queries of a source, runs of empty queries at its start, middle and end"""
    assert batch == "small", batch
    if src.name not in _GT_QUERIES:
        body = (_gt_read_queries if src.reads is not None else _gt_stream_queries)(src)
        random.Random(f"gt/{src.name}/{batch}/order").shuffle(body)
        mid = len(body) // 2
        _GT_QUERIES[src.name] = [("", 0)] * 3 + body[:mid] + [("", 0)] * 3 + body[mid:] + [("", 0)] * 4
    return _GT_QUERIES[src.name]


class LegsOnly:
    """a run stream's side of gt_reference: the oracle's intervals, and rows without reads -- a stream that is no BWT of
    reads has no read to extract (a walk need not meet '$'), and only its legs are compared"""

    def __init__(self, orc):
        self.orc = orc
        self.find = orc.find

    def extract(self, row):
        return "", ""

    def identity(self, row):
        return row


def gt_side(src, legs_only=False):
    return LegsOnly(src.orc) if legs_only or src.reads is None else src.orc


def gt_expected(srcs, key, qs, k, skip, M, count=None, legs_only=False):
    """[query][shard] -> gt_reference.gt_query's (legs, reads) over the sources' oracle sides, once per key and triple; a run
    stream's reads, and every shard's with legs_only, are meaningless (LegsOnly)"""
    per = [G.expected([gt_side(s, legs_only)], ("gt", s.name, key, legs_only or s.reads is None), qs, k, skip, M, count) for s in srcs]
    return [[per[p][q][0] for p in range(len(srcs))] for q in range(len(qs))]


_GT_GROWN, _FIND_STEPS = {}, {}


def gt_grown(src, qs, k, skip, M):
    """the lengthenings of every query in this shard: [q] -> [(tile, leg, "L" or "R", a, b)]"""
    at = (src.name, tuple(qs), k, skip, M)
    if at not in _GT_GROWN:
        out = []
        for w, pos in qs:
            grown = []
            G.gt_query(gt_side(src), w, pos, k, skip, M, None, grown)
            out.append(grown)
        _GT_GROWN[at] = out
    return _GT_GROWN[at]


def find_steps(src, x):
    """the LF steps findInterval(x) takes in the oracle"""
    if (src.name, x) not in _FIND_STEPS:
        st = src.orc.oix.find_intervals(np.frombuffer(x.encode(), np.uint8).reshape(1, -1), want_steps=True)[2]
        _FIND_STEPS[(src.name, x)] = int(st[0])
    return _FIND_STEPS[(src.name, x)]


def gt_narrow_steps(src, qs, k, skip, M):
    """the LF steps the lengthenings cost without a table, from the definition -- a left lengthening is one more step from
    an interval that is wide, hence proper (none if the symbol taken in is outside ACGT); a right lengthening is a fresh
    search of the longer string (none if it holds a symbol outside ACGT); the tile's own search is not counted"""
    steps = 0
    for (w, _), grown in zip(qs, gt_grown(src, qs, k, skip, M)):
        for _, _, side, a, b in grown:
            if side == "L":
                steps += int(w[a] in ACGT)
            elif not set(w[a:b]) - set(ACGT):
                steps += find_steps(src, w[a:b])
    return steps


def gt_right_lengthenings(src, qs, k, skip, M, depth):
    """the right lengthenings whose string has `depth` symbols or more, all of them ACGT: each may start from a table of
    that depth, which saves depth - 1 steps at the most"""
    return sum(1 for (w, _), grown in zip(qs, gt_grown(src, qs, k, skip, M)) for _, _, side, a, b in grown
               if side == "R" and b - a >= depth and not set(w[a:b]) - set(ACGT))


class ScanCounts(M.PlainCounts):
    """match_reference.PlainCounts for reads of hundreds of symbols, whose substrings do not fit a Counter: W(x) by scanning
    the reads laid end to end for every (overlapping) occurrence"""

    def __init__(self, reads):
        self.text = "$".join(reads)
        self.tr = str.maketrans("ACGT", "BCDE")
        self.keys = [reads[i][j:].translate(self.tr) + "$" for i, j in M.suffix_rows(reads)]
        self.n = len(self.keys)

    def W(self, x):
        if not x or set(x) - set(ACGT):
            return 0
        c, at = 0, self.text.find(x)
        while at >= 0:
            c += 1
            at = self.text.find(x, at + 1)
        return c
