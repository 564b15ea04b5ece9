"""CPU guards for the extraction stride matrix (tests/test_gpu_extract_strides.py): the index, the plain reference and the
strides that module runs on the GPU are built here, where the CPU can see them, and held to what the GPU tests rely on.

The walk kernels of csrc/extract_lines.hip write a read's bytes in one of three ways, chosen per launch from the stride
and the address of the row block:

    "16"     stride % 16 == 0 and the block 16-byte aligned: 16 characters per store, move_prefix16_kernel
    "dword"  stride % 4 == 0 and the block 4-byte aligned:   4 characters per store, move_prefix_kernel
    "byte"   anything else:                                  a store per character,  move_prefix_kernel

The index is the `ragged` fixture's read list (test_kmer_fixtures.py; reads of 12 .. 600 symbols, prefixes and suffixes of
other reads among them) and three reads of 1, 2 and 3 symbols, added to a copy here so that the strides 1, 2 and 3 have
reads that fit.  The reference is the suffix sort that builds the BWT (kmer_reference.suffix_rows): row -> (read, offset),
so the read of a row and the length of its prefix part are known without any walk.  Every row 0 .. n-1 is extracted: every
read is met at every split point, the terminator rows give prefix = whole read with an empty postfix.

"Fits" is include/rsbwt.h's rule: |prefix| + |postfix| <= stride."""
import hashlib

import numpy as np
import pytest

from kmer_reference import _bwt_runs, suffix_rows
from test_kmer_fixtures import fixture

NOFIT = 0xFFFFFFFF

# the stride matrix by store class (the class a 16-byte aligned row block gets)
STRIDES = {
    "16": [32, 48, 112, 256, 512, 560],
    "dword": [20, 36, 100, 116, 260, 520, 580],  # (580, not 600: no read is longer than 600, nothing would overflow)
    "byte": [1, 2, 3, 21, 37, 101, 257, 513, 599],
}
# one stride per class where the full matrix is not needed (other line layouts, the set forms): each longer than the
# byte mover's 64-byte step, with reads of exactly that length, and with most of the long reads not fitting
ONE_PER_CLASS = {"16": 112, "dword": 100, "byte": 101}
# ... and one per class where the prefix is moved in several steps of the 16-byte mover too (reads of exactly that length)
LONG_PER_CLASS = {"16": 512, "dword": 260, "byte": 257}
TINY_READS = ["G", "TC", "CAG"]


def store_class(stride):
    return "16" if stride % 16 == 0 else "dword" if stride % 4 == 0 else "byte"


class Table:
    """the reads of one index and what each of its rows is: ri[row] the read's index, j[row] the length of the prefix part,
    len[row] the read's length; text[i] = read i's bytes (zeros past its end)"""

    def __init__(self, reads):
        self.reads = list(reads)
        rows = suffix_rows(self.reads)
        self.n = len(rows)
        self.ri = np.array([i for i, _ in rows], np.int64)
        self.j = np.array([j for _, j in rows], np.uint32)
        lens = np.array([len(r) for r in self.reads], np.uint32)
        self.len = lens[self.ri]
        self.width = int(lens.max())
        self.text = np.zeros((len(self.reads), self.width), np.uint8)
        for i, r in enumerate(self.reads):
            self.text[i, :len(r)] = np.frombuffer(r.encode(), np.uint8)
        self._row_of = None

    def runs(self):
        return _bwt_runs(self.reads)

    def row_of(self, i, j):
        if self._row_of is None:
            self._row_of = {(int(a), int(b)): r for r, (a, b) in enumerate(zip(self.ri, self.j))}
        return self._row_of[(i, j)]

    def interval(self, q):
        """the rows whose suffix starts with q, as (lower, upper) -- contiguous by the sort; (1, 0) when there is none"""
        rows = []
        for i, r in enumerate(self.reads):
            at = r.find(q)
            while at >= 0 and q:
                rows.append(self.row_of(i, at))
                at = r.find(q, at + 1)
        if not rows:
            return 1, 0
        rows.sort()
        assert rows == list(range(rows[0], rows[-1] + 1)), q
        return rows[0], rows[-1]


def assert_rows(tab, rows, stride, out, ln, pl, what=""):
    """the fit rule on the answers of one extraction: rows (SA rows of tab's index, any >= n allowed), out [m][stride] bytes,
    ln / pl [m] u32 (pl may be None).  A read that fits: its length, its prefix length and its bytes, exactly; one that does
    not, or a row past the index: UINT32_MAX.  Bytes past a read's length and the prefix length of a read that does not fit
    are not looked at (include/rsbwt.h: unspecified)."""
    rows = np.asarray(rows, np.uint64)
    m = rows.size
    out = np.asarray(out).reshape(m, stride)
    inside = rows < np.uint64(tab.n)
    at = np.where(inside, rows, 0).astype(np.int64)
    L = tab.len[at]
    fits = inside & (L <= stride)
    want = np.where(fits, L, NOFIT).astype(np.uint32)
    bad = np.flatnonzero(np.asarray(ln, np.uint32) != want)
    assert bad.size == 0, (what, stride, "len", [(int(rows[b]), int(ln[b]), int(want[b]), int(tab.j[at[b]])) for b in bad[:5]], bad.size)
    f = np.flatnonzero(fits)
    if pl is not None:
        bad = f[np.asarray(pl, np.uint32)[f] != tab.j[at[f]]]
        assert bad.size == 0, (what, stride, "prefix_len", [(int(rows[b]), int(pl[b]), int(tab.j[at[b]])) for b in bad[:5]], bad.size)
    w = min(stride, tab.width)
    exp = tab.text[tab.ri[at[f]], :w]
    live = np.arange(w, dtype=np.uint32)[None, :] < L[f][:, None]
    wrong = ((out[f, :w] != exp) & live).any(axis=1)
    bad = f[wrong]
    assert bad.size == 0, (what, stride, "bytes", [(int(rows[b]), int(L[b]), int(tab.j[at[b]]), out[b, :L[b]].tobytes(), tab.reads[tab.ri[at[b]]])
                                                   for b in bad[:2]], bad.size)
    return int(f.size)


def reads_of_the_index():
    return list(fixture("ragged").shards[0]) + TINY_READS


def table():
    """the table of the whole index (built anew by every call: the test modules keep it in a module-scoped fixture)"""
    return Table(reads_of_the_index())


def shard_reads():
    """the same reads cut into three shards of unequal size (the set forms): 60 %, 30 %, 10 %"""
    reads = reads_of_the_index()
    a, b = len(reads) * 6 // 10, len(reads) * 9 // 10
    return [reads[:a], reads[a:b], reads[b:]]


def shard_tables():
    return [Table(r) for r in shard_reads()]


@pytest.fixture(scope="module")
def tab():
    return table()


@pytest.fixture(scope="module")
def tabs():
    return shard_tables()


def set_queries():
    """a few dozen queries of lengths of their own, cut from the reads: whole short reads, pieces of 8 .. 40 symbols from
    every part of short and long reads, one from inside the longest read (its rows' reads fit no stride below 600), one that
    occurs nowhere, one with an N, and an empty one"""
    import random
    rng = random.Random(4404)
    reads = reads_of_the_index()
    longest = max(reads, key=len)
    qs = [longest[300:324], "", "ACGTN", "ACGTACGTACGTTTTTGGGGCCCCAAAA"]
    qs += [r for r in reads if len(r) in (12, 21, 37)][:6] + TINY_READS
    for _ in range(24):
        r = reads[rng.randrange(len(reads))]
        k = rng.randrange(8, 41)
        if len(r) < k:
            k = len(r)
        s = rng.randrange(len(r) - k + 1)
        qs.append(r[s:s + k])
    return qs


# ---- the reference -----------------------------------------------------------------------------------------------------

def _bwt_runs_as_it_was(reads):
    """_bwt_runs before suffix_rows was cut out of it, kept to show the cut changed nothing"""
    rank = {"$": 0, "A": 1, "C": 2, "G": 3, "T": 4}
    tr = str.maketrans("ACGT", "BCDE")
    suf = sorted((r[j:].translate(tr) + "$", i, j) for i, r in enumerate(reads) for j in range(len(r) + 1))
    runs = []
    for _, i, j in suf:
        c = rank[reads[i][j - 1]] if j else 0
        if runs and runs[-1] >> 5 == c and runs[-1] & 31 < 31:
            runs[-1] += 1
        else:
            runs.append((c << 5) | 1)
    return np.array(runs, np.uint8)


def test_bwt_runs_is_unchanged_by_the_cut(tab):
    rag = fixture("ragged")
    runs = _bwt_runs(rag.shards[0])
    assert runs.dtype == np.uint8 and np.array_equal(runs, _bwt_runs_as_it_was(rag.shards[0]))
    # (the digest of the run bytes as the code before the cut gave them)
    assert hashlib.sha256(runs.tobytes()).hexdigest() == "509546a51c40dde6717a855fa0f933c7ddfa730e23c7470f73660fb524996397"
    for fx in (fixture("pop"), fixture("repeat")):
        for sh in fx.shards:
            assert np.array_equal(_bwt_runs(sh), _bwt_runs_as_it_was(sh))
    assert np.array_equal(tab.runs(), _bwt_runs_as_it_was(reads_of_the_index()))


def test_suffix_rows_is_a_sorted_list_of_every_suffix(tab):
    """the table against its definition, on its own terms: every (read, offset) once, the suffixes in order, equal ones by
    read index; the first num_strings rows are the terminators in read order"""
    reads = tab.reads
    assert tab.n == sum(len(r) + 1 for r in reads)
    assert len({(int(i), int(j)) for i, j in zip(tab.ri, tab.j)}) == tab.n
    assert (tab.j <= tab.len).all()
    key = lambda r: [" ACGT".index(c) for c in reads[tab.ri[r]][tab.j[r]:]] + [0]  # ('$' = 0 ends every suffix)
    prev = key(0)
    for r in range(1, tab.n):
        cur = key(r)
        assert prev < cur or (prev == cur and tab.ri[r - 1] < tab.ri[r]), r
        prev = cur
    assert [int(i) for i in tab.ri[:len(reads)]] == list(range(len(reads))) and (tab.j[:len(reads)] == tab.len[:len(reads)]).all()


@pytest.mark.parametrize("which", ["whole", "shard0", "shard1", "shard2"])
def test_oracle_extracts_what_the_suffix_sort_says_on_every_row(oracle, tab, tabs, which):
    """oracle.extract(row) == (reads[i][:j], reads[i][j:]) for EVERY row: the oracle's two walks against a reference that
    shares no code with them"""
    tab = tab if which == "whole" else tabs[int(which[-1])]
    oix = oracle.from_runs(tab.runs(), len(tab.reads))
    assert oix.bwlen() == tab.n
    for row in range(tab.n):
        r = tab.reads[tab.ri[row]]
        j = int(tab.j[row])
        assert oix.extract(row) == (r[:j], r[j:]), row
    # ... and the batch form beside it (what the GPU tests of other modules compare with)
    out, ln, pl = oix.extract_batch(np.arange(tab.n, dtype=np.uint64), stride=tab.width)
    assert_rows(tab, np.arange(tab.n), tab.width, out, ln, pl, which)


@pytest.mark.parametrize("stride", [1, 3, 20, 37, 48, 100, 101, 112])
def test_the_fit_rule_of_the_checker_is_the_oracles(oracle, tab, stride):
    """assert_rows -- what the GPU tests judge with -- on the oracle's own batch extraction at short strides: the oracle
    cuts a walk at the stride as the header says (a read of exactly `stride` symbols fits, at every split point)"""
    oix = oracle.from_runs(tab.runs(), len(tab.reads))
    rows = np.concatenate([np.arange(tab.n), [tab.n, tab.n + 5]]).astype(np.uint64)
    out, ln, pl = oix.extract_batch(rows[:tab.n], stride=stride, nthreads=4)
    ln, pl = np.concatenate([ln, [NOFIT, NOFIT]]), np.concatenate([pl, [0, 0]])
    out = np.concatenate([out, np.zeros((2, stride), np.uint8)])
    fit = assert_rows(tab, rows, stride, out, ln, pl, "oracle")
    assert fit == int((tab.len <= stride).sum()) > 0
    # ... and it does notice: one wrong byte at the end of a read, one length, one prefix length
    f = int(np.flatnonzero(tab.len <= stride)[-1])
    for what in ("byte", "len", "pl"):
        o2, l2, p2 = out.copy(), ln.copy(), pl.copy()
        if what == "byte":
            o2[f, tab.len[f] - 1] ^= 1
        elif what == "len":
            l2[f] = NOFIT
        else:
            p2[f] += 1
        with pytest.raises(AssertionError):
            assert_rows(tab, rows, stride, o2, l2, p2, what)


# ---- what the strides of the matrix meet -------------------------------------------------------------------------------

def test_the_matrix_is_grouped_by_store_class():
    for cls, strides in STRIDES.items():
        assert strides and all(store_class(s) == cls for s in strides), cls
        assert store_class(ONE_PER_CLASS[cls]) == cls and store_class(LONG_PER_CLASS[cls]) == cls
        assert ONE_PER_CLASS[cls] in strides and LONG_PER_CLASS[cls] in strides
    all_s = [s for v in STRIDES.values() for s in v]
    assert len(set(all_s)) == len(all_s)


@pytest.mark.parametrize("cls", list(STRIDES))
def test_each_class_meets_the_fit_boundary_and_both_movers_steps(tab, cls):
    lens = {len(r) for r in tab.reads}
    strides = STRIDES[cls]
    # reads of s - 1, s and s + 1 symbols at a short stride
    assert any(s <= 120 and {s - 1, s, s + 1} <= lens for s in strides), cls
    # a read of exactly s symbols and a longer one at a long stride, and a prefix of more than 256 symbols of a read that
    # fits: move_prefix16_kernel's second step of 256 bytes, move_prefix_kernel's fifth of 64
    def long_case(s):
        fit = tab.len <= s
        return s >= 256 and s in lens and max(lens) > s and ((tab.j > 256) & (tab.j < s) & fit).any()
    assert any(long_case(s) for s in strides), cls
    # every phase of the prefix's and of the read's end against the store width, over the rows that fit
    fit = tab.len <= max(strides)
    mod = 4 if cls == "dword" else 16
    assert set((tab.j[fit] % mod).tolist()) == set(range(mod)) and set((tab.len[fit] % mod).tolist()) == set(range(mod)), cls
    if cls == "dword":  # (asked of the dword path modulo 4; the fixture gives it modulo 16 as well)
        assert set((tab.j[fit] % 16).tolist()) == set(range(16)) and set((tab.len[fit] % 16).tolist()) == set(range(16))
    # ... and every pair (prefix phase, end phase) of the store width where a postfix follows a prefix
    both = fit & (tab.j > 0) & (tab.j < tab.len)
    assert len(set(zip((tab.j[both] % mod).tolist(), (tab.len[both] % mod).tolist()))) == mod * mod, cls
    # the four kinds of row at every stride; the prefix that is exactly the stride with nothing after it at one or more
    full = 0
    for s in strides:
        L, j = tab.len, tab.j
        assert (L <= s).any(), (s, "no read fits")
        assert s in lens, (s, "no read of exactly the stride")
        assert ((L > s) & (j < s)).any(), (s, "no prefix fits of a read that does not")
        assert ((L > s) & (j == s)).any(), (s, "no prefix fills the stride with a postfix to come")
        assert ((L > s) & (j > s)).any(), (s, "no prefix overflows alone")
        assert ((L == s) & (j == s)).any() and ((L == s) & (j > 0) & (j < s)).any() or s == 1, (s, "a read of exactly the stride, split and unsplit")
        full += int(((L == s) & (j == s)).any())
        # a read that fits with a prefix the byte mover moves (shorter than the stride, not empty) and one it leaves
        assert ((L <= s) & (j > 0) & (j < s)).any() or s == 1, s
    assert full >= 1, cls
    if cls != "byte":  # (the strides 1, 2, 3 have no read of their length but the added ones)
        assert full >= 3, cls


def test_the_shards_and_the_queries_of_the_set_forms(tabs):
    """three shards of unequal size, each with reads that fit and reads that do not at the strides the set forms use; the
    queries: lengths of their own, one whose rows' reads do not fit, an empty one, one that is nowhere"""
    assert len(tabs) == 3 and tabs[0].n > 3 * tabs[1].n // 2 and tabs[1].n > 2 * tabs[2].n > 0
    assert sorted(r for t in tabs for r in t.reads) == sorted(reads_of_the_index())
    for s in list(ONE_PER_CLASS.values()) + [64]:
        for t in tabs:
            assert (t.len <= s).any() and ((t.len > s) & (t.j < s)).any() and ((t.len > s) & (t.j > s)).any(), s
            assert s == 64 or ((t.len <= s) & (t.j > 64)).any(), s  # (a second step of the byte mover in every shard)
    qs = set_queries()
    assert 30 <= len(qs) <= 48 and "" in qs and len({len(q) for q in qs}) >= 12
    width = [[(lambda lu: lu[1] - lu[0] + 1)(t.interval(q)) for t in tabs] for q in qs]
    assert sum(1 for w in width if sum(w) > 0) >= 25 and any(sum(w) == 0 for w in width[3:])
    assert sum(1 for w in width if sum(1 for x in w if x) >= 2) >= 5  # queries with rows in several shards
    p = max(range(3), key=lambda i: width[0][i])
    lo, up = tabs[p].interval(qs[0])
    assert up >= lo and (tabs[p].len[lo:up + 1] > max(ONE_PER_CLASS.values())).any()
    for s in ONE_PER_CLASS.values():  # fitting and non-fitting reads side by side in the answers of one call
        fit = [bool((t.len[lo:up + 1] <= s).any()) for q in qs for t in tabs for lo, up in [t.interval(q)] if up >= lo]
        nofit = [bool((t.len[lo:up + 1] > s).any()) for q in qs for t in tabs for lo, up in [t.interval(q)] if up >= lo]
        assert any(fit) and any(nofit), s
