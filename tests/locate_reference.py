"""The locate reference the locate tests share -- TEST INFRASTRUCTURE.  The truth table is built from the read lists and
the suffix sort alone (kmer_reference.suffix_rows): no BWT, no LF walk, no rank.

For a shard's `reads`, row r of the multi-string BWT is the suffix reads[i][j:] + '$' with (i, j) = suffix_rows(reads)[r]:
    offset    j
    read_row  the row whose entry is (i, 0)
    ordinal   the rank of i when the reads are sorted by (string with '$' lowest, index)
The rows of the terminator block (j == len(reads[i])) are covered too: the table orders equal suffixes by read index."""
import numpy as np

from kmer_reference import suffix_rows

NONE64 = np.uint64(0xFFFFFFFFFFFFFFFF)
NONE32 = np.uint32(0xFFFFFFFF)


class Truth:
    """per row of one shard: read (index into the read list), offset, read_row, ordinal -- numpy arrays"""

    def __init__(self, reads):
        table = suffix_rows(reads)
        n = len(table)
        self.reads = reads
        self.n = n
        self.read = np.array([i for i, _ in table], np.int64)
        self.offset = np.array([j for _, j in table], np.uint32)
        start = np.zeros(len(reads), np.uint64)            # read i -> the row of (i, 0)
        for r, (i, j) in enumerate(table):
            if j == 0:
                start[i] = r
        tr = str.maketrans("ACGT", "BCDE")                  # (keeps '$' below every base)
        order = sorted(range(len(reads)), key=lambda i: (reads[i].translate(tr) + "$", i))
        rank = np.zeros(len(reads), np.uint64)
        rank[np.array(order, np.int64)] = np.arange(len(reads), dtype=np.uint64)
        self.read_row = start[self.read]
        self.ordinal = rank[self.read]
        self.row_of = {(int(i), int(j)): r for r, (i, j) in enumerate(table)}

    def identity_rows(self):
        """the rows whose BWT symbol is '$' (offset 0): where every walk ends"""
        return np.nonzero(self.offset == 0)[0]

    def expect(self, rows, max_steps=0):
        """(read_row, ordinal, offset) a locate call answers for `rows` (any integers below 2^64): markers for a row
        past the index and for one whose offset exceeds max_steps (0 = 2^20)"""
        rows = np.asarray(rows, np.uint64)
        cap = max_steps if max_steps else 1 << 20
        inside = rows < np.uint64(self.n)
        at = np.where(inside, rows, np.uint64(0)).astype(np.int64)
        ok = inside & (self.offset[at] <= cap)
        return (np.where(ok, self.read_row[at], NONE64), np.where(ok, self.ordinal[at], NONE64),
                np.where(ok, self.offset[at], NONE32).astype(np.uint32))


_TRUTH = {}


def truth(fx):
    """the truth tables of a fixture of tests/test_kmer_fixtures.py, one per shard, built once"""
    if fx.name not in _TRUTH:
        _TRUTH[fx.name] = [Truth(sh) for sh in fx.shards]
    return _TRUTH[fx.name]


def string_matches(shards, q):
    """{(shard, read index, offset)} of every occurrence of q in the reads, by str.find: no BWT"""
    out = set()
    if not q:
        return out
    for p, reads in enumerate(shards):
        for i, r in enumerate(reads):
            j = r.find(q)
            while j >= 0:
                out.add((p, i, j))
                j = r.find(q, j + 1)
    return out


# (fixture, kind, span, for_reads) of tests/test_kmer_fixtures.LAYOUTS on which no group of 16 windows PROVES an identity
# row in a window of the kind (tests/test_locate_reference.py, by counting): left out of the GPU matrix
# (every span with spill chunks among them: the identity rows lie where the BWT holds '$', next to the longest runs of the
# index, and no group both spills into chunks and is crowded with identity rows -- the terminal '$' count inside a spill
# chunk is therefore NOT shown to be exercised by these fixtures)
DROPPED = (
    ("pop", "chunk", 128, True),
    ("ragged", "chunk+", 128, True),
    ("repeat", "chunk+", 270, True),
    ("repeat", "far", 320, True),
    ("repeat", "far", 320, False),
    ("repeat", "chain", 600, True),
)


def gpu_layouts():
    import test_kmer_fixtures as F
    return [lay for lay in F.LAYOUTS if (lay[0], lay[1], lay[2], lay[3]) not in DROPPED]
