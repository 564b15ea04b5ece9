"""The KmerMatch reference the kmer tests share -- TEST INFRASTRUCTURE.  Everything here runs on the oracle alone
(oix.char, oix.occ, oix.pc, oix.find_interval, oix.extract): the reference's find_kmer_reads as a composition of
per-row extractions (service.cpp:466-502), and the read identity of a row as a plain LF walk (query.cpp:49-57) --
one walk per row, no chains, nothing deduplicated before the end."""
import numpy as np


def _rc(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def _tiles(w, k, skip):
    if k <= 0 or skip < 0 or len(w) < k:
        return []
    return sorted({w[i:i + k] for i in range(0, len(w) - k + 1, skip + 1)})


def _rows_reads(oix, t):
    lo, up = oix.find_interval(t)
    out = []
    for r in range(lo, up + 1):
        pre, post = oix.extract(r)
        out.append(pre + post)
    return out


def _find_reads(oix, t, minl, maxl):
    """find_reads(pBWT, t, "") (service.cpp:714-797) as a set of strings"""
    def is_read(x):  # query_exactmatch (query.cpp:102-120)
        return x in _rows_reads(oix, x)
    if len(t) < minl:
        return set(_rows_reads(oix, t))
    got = set()
    if len(t) < maxl:
        if len(t) != minl:
            got |= {x for x in _tiles(t, minl, 0) if is_read(x)}
        return got | set(_rows_reads(oix, t))
    got |= {x for x in _tiles(t, maxl, 0) if is_read(x)}
    if minl != maxl:
        got |= {x for x in _tiles(t, minl, 0) if is_read(x)}
    return got


def _expected(oix, w, k, skip, minl=73, maxl=100):
    got = set()
    for t in _tiles(w, k, skip):
        if set(t) <= set("ACGT"):
            got |= _find_reads(oix, t, minl, maxl)
    return got


def suffix_rows(reads):
    """what every row of the multi-string BWT of `reads` is: row -> (read index i, offset j), the row of the suffix
    reads[i][j:] + '$' -- suffixes ordered by their string, '$' lowest, equal ones by read index.  The read of the row is
    reads[i], the part of it left of the row (extractPrefix) has j symbols; j == len(reads[i]) on the terminator rows."""
    tr = str.maketrans("ACGT", "BCDE")  # (keeps '$' below every base)
    suf = sorted((r[j:].translate(tr) + "$", i, j) for i, r in enumerate(reads) for j in range(len(r) + 1))
    return [(i, j) for _, i, j in suf]


def _bwt_runs(reads):
    """the run bytes of the multi-string BWT of `reads` (RLUnit: symbol rank << 5 | length), duplicates kept: the symbol
    left of every row of suffix_rows"""
    rank = {"$": 0, "A": 1, "C": 2, "G": 3, "T": 4}
    runs = []
    for i, j in suffix_rows(reads):
        c = rank[reads[i][j - 1]] if j else 0
        if runs and runs[-1] >> 5 == c and runs[-1] & 31 < 31:
            runs[-1] += 1
        else:
            runs.append((c << 5) | 1)
    return np.array(runs, np.uint8)


# ---- read identities ------------------------------------------------------------------------------------------------

def identity(oix, row):
    """LF from `row` until the BWT symbol is '$'; that row: the row of the read's full suffix (query.cpp:49-57)"""
    while True:
        b = oix.char(row)
        if b == "$":
            return row
        row = oix.pc(b) + oix.occ(b, row) - 1


class Walks:
    """identity() of many rows of one index, each row's LF step asked of the oracle once: row -> (the next row or
    None at '$'), and from it the identity, the number of LF steps of the full walk, and the rows it visits.  A cache
    of single steps only -- every row's walk is still followed to its own '$'."""

    def __init__(self, oix):
        self.oix = oix
        self.next = {}
        self.pc = {b: oix.pc(b) for b in "ACGT"}

    def step(self, row):
        if row not in self.next:
            b = self.oix.char(row)
            self.next[row] = None if b == "$" else self.pc[b] + self.oix.occ(b, row) - 1
        return self.next[row]

    def rows(self, row):
        """the rows of the walk from `row`, `row` first, the '$' row last"""
        out = [row]
        while True:
            row = self.step(row)
            if row is None:
                return out
            out.append(row)

    def identity(self, row):
        return self.rows(row)[-1]

    def steps(self, row):
        return len(self.rows(row)) - 1


def row_tiles(w, k, skip, maxl):
    """the tiles of `w` whose interval's rows find_reads visits: all ACGT, shorter than max_read_length"""
    return [t for t in _tiles(w, k, skip) if set(t) <= set("ACGT") and len(t) < maxl]


def candidate_rows(oix, w, k, skip, maxl):
    """every row of the interval of every such tile of one query (a row once per tile that holds it)"""
    out = []
    for t in row_tiles(w, k, skip, maxl):
        lo, up = oix.find_interval(t)
        out.extend(range(lo, up + 1))
    return out


def expected_identities(oix, queries, k, skip, minl, maxl, walks=None):
    """the set of identity(row) over every row of the interval of every all-ACGT tile shorter than maxl, over all the
    queries of one call (one pass: identities are deduplicated per shard across the whole call)"""
    ident = walks.identity if walks is not None else (lambda r: identity(oix, r))
    return {ident(r) for w in queries for r in candidate_rows(oix, w, k, skip, maxl)}


def expected_over(oix, identities, stride):
    """how many of the reads at `identities` are longer than `stride`"""
    n = 0
    for r in identities:
        pre, post = oix.extract(r, cap=1 << 16)
        n += len(pre + post) > stride
    return n
