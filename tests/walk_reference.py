"""The walk reference the walk tests share -- TEST INFRASTRUCTURE, CPU only.  include/rsbwt.h's definition of the extension
counts and of rsbwt_set_walk restated twice:

  * over the oracle's BWT (OracleSide): findInterval of every candidate on its own (gt_reference.OracleShard.find), its
    rows by the C-ABI's rule (match_reference.width) -- where the GPU keeps the loop over the steps inside one launch;
  * with no BWT at all (PlainSide): the occurrences of a candidate as a substring of the reads, overlapping ones included.

A side answers W(p, x), the rows of x in shard p.  The candidates of a string s are its context (s[-ctx:] walking right,
s[:ctx] walking left) with A, C, G, T put on the walking side; E_p(s, c) = W(p, x_c) (+ W(p, rc(x_c)) with both strands);
the support of c is the sum of E_p over the shards.  A walk appends the one symbol whose support is >= max(min_count, 1)
until none (DEAD_END), two or more (BRANCH) or max_steps symbols (LIMIT); a seed shorter than ctx or with a symbol outside
ACGT in its context is INVALID.

The inputs are gt_reference.fixture(): its 2 shards as they are (`plain`), the same with every odd-numbered read of each
shard reverse-complemented (`stranded`), and either read set dealt round-robin to 1, 2, 3, 5 and 9 shards (2 = the shards
as they are); BWTs by suffix sort (kmer_reference._bwt_runs).  The expected work counters: the candidate searches, and
the LF steps of a search without a k-mer table -- from initInterval of the last symbol, then one per symbol up to and
including the first that empties the interval; with a table of depth T they are T - 1 fewer per table start."""
from collections import Counter, namedtuple

import gt_reference as G
import match_reference as M
from kmer_reference import _bwt_runs, _rc

DEAD_END, BRANCH, LIMIT, INVALID = 1, 2, 3, 4
ACGT = "ACGT"
CTXS = (12, 20)
MIN_COUNTS = (1, 2, 3)
MAX_STEPS = 64
DEALS = (1, 2, 3, 5, 9)
SEED_LEN, SEED_STRIDE = 40, 37

Walk = namedtuple("Walk", ["ext", "stop", "support", "last", "final", "contexts"])


# ---- the inputs ------------------------------------------------------------------------------------------------------

_SETS = {}


def read_sets():
    """{name: [reads of shard 0, reads of shard 1]}"""
    if not _SETS:
        fx = G.fixture()
        _SETS["plain"] = [list(sh) for sh in fx.shards]
        _SETS["stranded"] = [[_rc(r) if i % 2 else r for i, r in enumerate(sh)] for sh in fx.shards]
    return _SETS


def dealt(name, S):
    """the reads of a set dealt round-robin to S shards; S = 2 gives the two shards as they are"""
    a, b = read_sets()[name]
    every = [r for pair in zip(a, b) for r in pair] + a[len(b):] + b[len(a):]
    return [every[p::S] for p in range(S)]


_RUNS = {}


def runs(name, S):
    if (name, S) not in _RUNS:
        _RUNS[(name, S)] = [_bwt_runs(sh) for sh in dealt(name, S)]
    return _RUNS[(name, S)]


def seeds(ctx):
    """the 53 windows of 40 symbols of haplotype 1, then: a seed of ctx - 1 symbols, one with an N in its context (either
    direction's), one with an N outside both contexts (valid), an empty one, one of exactly ctx symbols"""
    g = G.fixture().haps[1]
    out = [g[at:at + SEED_LEN] for at in range(0, len(g) - SEED_LEN, SEED_STRIDE)]
    assert len(out) == 53
    w = g[200:260]
    out += [g[900:900 + ctx - 1], w[:5] + "N" + w[6:54] + "N" + w[55:], w[:30] + "N" + w[31:], "", g[1300:1300 + ctx]]
    return out


N_PLAIN = 53   # seeds(ctx)[:N_PLAIN] are the windows; of the five after them the third and the fifth are valid
# (set, ctx, min_count, left, both strands) at which walks seeded inside the tandem repeat reach max_steps there
IN_REPEAT = ("stranded", 20, 2, True, False)


def seeds_inside_the_repeat():
    """the windows of seeds() that lie inside the tandem repeat"""
    r0, r1 = G.fixture().rep
    return [i for i in range(N_PLAIN) if r0 <= i * SEED_STRIDE and i * SEED_STRIDE + SEED_LEN <= r1]


# ---- the two sides ---------------------------------------------------------------------------------------------------

class OracleSide:
    """W(p, x) from findInterval over the oracle; shards: a list of gt_reference.OracleShard"""

    def __init__(self, shards):
        self.shards = shards
        self.n = [sh.oix.bwlen() for sh in shards]
        self.S = len(shards)

    def W(self, p, x):
        return M.width(self.shards[p].find(x), self.n[p])


class PlainSide:
    """W(p, x) = the occurrences of x in the reads of shard p, overlapping ones included -- no BWT"""

    def __init__(self, read_lists):
        self.reads = read_lists
        self.S = len(read_lists)
        self._by_len = {}

    def W(self, p, x):
        if not x or set(x) - set(ACGT):
            return 0
        k = len(x)
        if (p, k) not in self._by_len:
            self._by_len[(p, k)] = Counter(r[i:i + k] for r in self.reads[p] for i in range(len(r) - k + 1))
        return self._by_len[(p, k)].get(x, 0)


# ---- the definition --------------------------------------------------------------------------------------------------

def context(s, ctx, left):
    """the context of s, or None where s is invalid"""
    if len(s) < ctx:
        return None
    c = s[:ctx] if left else s[len(s) - ctx:]
    return None if set(c) - set(ACGT) else c


def candidates(c, left):
    return [b + c if left else c + b for b in ACGT]


def extensions(side, s, ctx, left, both, shards=None):
    """[shard][4] extension counts of s (zeros where s is invalid) over `shards` (default: all of the side's)"""
    ps = range(side.S) if shards is None else shards
    c = context(s, ctx, left)
    if c is None:
        return [[0] * 4 for _ in ps]
    return [[side.W(p, x) + (side.W(p, _rc(x)) if both else 0) for x in candidates(c, left)] for p in ps]


def walk(side, seed, ctx, min_count, max_steps, left, both, shards=None):
    m = max(min_count, 1)
    s, ext, sup, seen = seed, "", [], []
    if context(s, ctx, left) is None:
        return Walk("", INVALID, (), (0, 0, 0, 0), s, ())
    while True:
        if len(ext) == max_steps:
            return Walk(ext, LIMIT, tuple(sup), (0, 0, 0, 0), s, tuple(seen))
        seen.append(context(s, ctx, left))
        tot = tuple(sum(col) for col in zip(*extensions(side, s, ctx, left, both, shards)))
        live = [b for b in range(4) if tot[b] >= m]
        if len(live) != 1:
            return Walk(ext, BRANCH if live else DEAD_END, tuple(sup), tot, s, tuple(seen))
        b = live[0]
        ext += ACGT[b]
        sup.append(min(tot[b], 2 ** 32 - 1))
        s = ACGT[b] + s if left else s + ACGT[b]


_WALKS = {}


def walks(side, key, sds, ctx, min_count, max_steps, left, both, shards=None):
    """the walks of every seed, computed once per (key, parameters); key names the side and the seeds"""
    at = (key, ctx, min_count, max_steps, left, both, None if shards is None else tuple(shards))
    if at not in _WALKS:
        _WALKS[at] = [walk(side, s, ctx, min_count, max_steps, left, both, shards) for s in sds]
    return _WALKS[at]


# ---- the expected work -----------------------------------------------------------------------------------------------

def search_steps(side, p, x):
    """the LF steps of a search of x in shard p without a k-mer table"""
    if side.W(p, x[-1]) == 0:
        return 0
    steps = 0
    for j in range(1, len(x)):
        steps += 1
        if side.W(p, x[len(x) - j - 1:]) == 0:
            break
    return steps


def expected_work(side, ws, left, both):
    """(candidate searches, LF steps without a table) of walks `ws` over every shard of the side"""
    searches = steps = 0
    for w in ws:
        for c in w.contexts:
            for x in candidates(c, left):
                for y in ((x, _rc(x)) if both else (x,)):
                    for p in range(side.S):
                        searches += 1
                        steps += search_steps(side, p, y)
    return searches, steps
