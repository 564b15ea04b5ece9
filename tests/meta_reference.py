"""The sample-table reference the meta tests share -- TEST INFRASTRUCTURE.  include/rsbwt.h's definition of
rsbwt_set_meta_build / rsbwt_set_read_ordinals_var / rsbwt_set_meta_by_ordinal / rsbwt_set_read_meta_var restated twice:

  * over the oracle's BWT (OracleSide): the whole-read search from the terminator rows [0, num_strings) -- one
    updateInterval per symbol, right to left, until the interval empties -- and Occ('$', .) at its two ends;
  * with no BWT at all (PlainSide): the ordinal of a string is its place among the sorted reads (bisect_left, as
    tests/overlap_reference.py numbers reads), its copies the reads equal to it, and the table a dict from read string to
    value in which a later pair overwrites an earlier one.

Values are a deterministic function of the read string (SHA-256): the length is drawn from LADDER by the hash, the bytes
are the hash's stream; byte 10 is mapped to 11 so that every value can also stand on a line of the pairs file."""
import bisect
import hashlib

ACGT = set("ACGT")
# value lengths: empty, below / at / above a dword, a 16-byte granule, the 64-byte split between the lane copy and the
# wave copy, 256, one past 1 KiB (a wave pass) and a read of a common sequence
LADDER = [0, 1, 3, 4, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1028, 5000]
MAX_QUERY = 65535


def value_of(read, tag=0, ladder=None):
    """(ladder: the lengths to draw from, LADDER unless a test has a reason for another and says it)"""
    ladder = LADDER if ladder is None else ladder
    h = hashlib.sha256(f"{tag}/{read}".encode()).digest()
    n = ladder[int.from_bytes(h[:4], "little") % len(ladder)]
    out, i = b"", 0
    while len(out) < n:
        out += hashlib.sha256(h + i.to_bytes(4, "little")).digest()
        i += 1
    return out[:n].replace(b"\n", b"\x0b")


def searchable(w):
    return 0 < len(w) <= MAX_QUERY and not (set(w) - ACGT)


class OracleSide:
    """(ordinal, copies, LF steps) of a string from the whole-read search and Occ('$', .)"""

    def __init__(self, oix, num_strings):
        self.oix, self.ns = oix, num_strings
        self._memo = {}

    def lookup(self, w):
        if w not in self._memo:
            self._memo[w] = self._lookup(w)
        return self._memo[w]

    def _lookup(self, w):
        if not searchable(w) or self.ns == 0:
            return (0, 0, 0)
        occ = lambda b, i: self.oix.occ(b, i) if i >= 0 else 0  # noqa: E731  Occ(., -1) = 0
        lo, up, steps = 0, self.ns - 1, 0
        for c in reversed(w):
            lo, up = self.oix.pc(c) + occ(c, lo - 1), self.oix.pc(c) + occ(c, up) - 1
            steps += 1
            if lo > up:
                return (0, 0, steps)
        before = occ("$", lo - 1)
        copies = occ("$", up) - before
        return (before if copies else 0, copies, steps)


class PlainSide:
    """(ordinal, copies) of a string from the read list alone"""

    def __init__(self, reads):
        self.sorted = sorted(reads)
        self.ns = len(self.sorted)

    def lookup(self, w):
        if not searchable(w):
            return (0, 0, None)
        o = bisect.bisect_left(self.sorted, w)
        c = bisect.bisect_right(self.sorted, w) - o
        return (o if c else 0, c, None)


def build_tables(sides, pairs):
    """rsbwt_set_meta_build over oracle sides: (tables, stats4) -- tables[p][o] = the value of ordinal o of shard p (b""
    where no pair reaches it), the pair with the higher index winning; stats4 = {matched, unmatched, ordinals given a value,
    value bytes}"""
    tables = [[None] * s.ns for s in sides]
    matched = 0
    for read, value in pairs:  # in index order: a later pair overwrites
        hit = False
        for p, s in enumerate(sides):
            o, c, _ = s.lookup(read)
            for x in range(o, o + c):
                tables[p][x] = value
            hit = hit or c > 0
        matched += hit
    given = sum(v is not None for t in tables for v in t)
    out = [[v if v is not None else b"" for v in t] for t in tables]
    return out, (matched, len(pairs) - matched, given, sum(len(v) for t in out for v in t))


def build_tables_plain(shards, pairs):
    """the same with no BWT: a dict with later pairs overwriting, read out at every read of the sorted lists"""
    d = {}
    for read, value in pairs:
        if searchable(read):
            d[read] = value
    return [[d.get(r, b"") for r in sorted(sh)] for sh in shards]


def by_ordinal(tables, shard_of, ordinal):
    """rsbwt_set_meta_by_ordinal: the values in the order asked; empty for an ordinal >= num_strings"""
    return [tables[p][o] if o < len(tables[p]) else b"" for p, o in zip(shard_of, ordinal)]


def read_meta(sides, tables, queries):
    """rsbwt_set_read_meta_var: (values with query q in shard p at q * S + p, copies[p][q], LF steps): the value at the
    read's first ordinal, empty where copies == 0"""
    S = len(sides)
    vals, copies, steps = [], [[0] * len(queries) for _ in range(S)], 0
    for q, w in enumerate(queries):
        for p, s in enumerate(sides):
            o, c, st = s.lookup(w)
            copies[p][q] = c
            steps += st or 0
            vals.append(tables[p][o] if c else b"")
    return vals, copies, steps


def flat(values):
    """(first, bytes) as the calls lay values out"""
    first = [0]
    for v in values:
        first.append(first[-1] + len(v))
    return first, b"".join(values)


def pairs_for(shards, every=9, seed="meta"):
    """The pairs of a fixture: every distinct read of the shards except each `every`-th one (ordinals no pair reaches),
    in a seeded order, with value_of(read); then the classes a build must get right: two reads given a second time with
    another value (tag 1: the later pair wins), a proper prefix and a proper suffix of a read and an unrelated string
    (match nothing), a string with an N, the empty string.  Returns (pairs, info)"""
    distinct = sorted({r for sh in shards for r in sh})
    order = sorted(distinct, key=lambda r: hashlib.sha256(f"{seed}/{r}".encode()).digest())
    left_out = set(order[every - 1::every])
    pairs = [(r, value_of(r)) for r in order if r not in left_out]
    kept = [r for r in order if r not in left_out]
    differs = [r for r in kept if value_of(r, 1) != value_of(r)]
    twice = [differs[3], differs[len(differs) // 2]]
    pairs += [(r, value_of(r, 1)) for r in twice]
    longest = max(distinct, key=len)
    nothing = [longest[:len(longest) - 1], longest[1:], "ACGT" * 10 + "TTTTT"]
    nothing = [w for w in nothing if w not in set(distinct)]
    with_n = kept[0][:5] + "N" + kept[0][6:]
    pairs += [(w, value_of(w)) for w in nothing] + [(with_n, value_of(with_n)), ("", b"empty-string")]
    return pairs, dict(left_out=left_out, twice=twice, nothing=nothing, with_n=with_n)
