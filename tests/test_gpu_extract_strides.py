"""GPU suite (-m gpu): read extraction at every stride class and row-block alignment, and on the fit boundary.

The walk kernels of csrc/extract_lines.hip write a read 16 bytes, 4 bytes or a byte at a time, by the stride and the
address of the row block (tests/test_extract_fixtures.py names the classes, builds the index and the reference, and proves
on the CPU that the strides below meet every case).  Every other extraction of the suite uses a stride that is a multiple of
16 on a fresh allocation: the first way only.

What is asserted, for EVERY row 0 .. n-1 of the index (every read at every split point) and rows past it, is the rule of
include/rsbwt.h: a read with |prefix| + |postfix| <= stride comes back whole -- its length, its prefix length, its bytes;
any other, and any row >= n, gets len = UINT32_MAX.  The expectation is the suffix sort's table, never a second GPU call.
Bytes past a read's length inside its own stride bytes and the prefix length of a read that does not fit are unspecified and
not looked at; nothing outside the row block may be written."""
import ctypes as C

import numpy as np
import pytest

from test_extract_fixtures import (LONG_PER_CLASS, NOFIT, ONE_PER_CLASS, STRIDES, assert_rows, set_queries, shard_tables, store_class,
                                   table)

pytestmark = pytest.mark.gpu

ALL_STRIDES = [s for cls in STRIDES.values() for s in cls]
CANARY = 64


def _sid(s):
    return f"{store_class(s)}-{s}"


@pytest.fixture(scope="module")
def index(rsb):
    """the index on the GPU, one handle per line layout asked for: get(span, for_reads)"""
    tab = table()
    runs = tab.runs()
    opened = {}

    def get(span=0, for_reads=False):
        if (span, for_reads) not in opened:
            opened[(span, for_reads)] = rsb.GpuBWT(runs=runs, num_strings=len(tab.reads), window_span=span, for_reads=for_reads)
            assert opened[(span, for_reads)].getBWLen() == tab.n
        return opened[(span, for_reads)]
    yield tab, get
    for g in opened.values():
        g.close()


def _host_extract(L, g, tab, rows, stride, what):
    """rsbwt_extract into arrays with canaries around them; the fit rule on every row"""
    m = rows.size
    buf = np.full(CANARY + m * stride + CANARY, 0xC7, np.uint8)
    ln = np.full(m + 2, 0x5A5A5A5A, np.uint32)
    pl = np.full(m + 2, 0x5A5A5A5A, np.uint32)
    out = buf[CANARY:CANARY + m * stride]
    assert L.rsbwt_extract(g.handle, rows.ctypes.data, m, out.ctypes.data, stride, ln[1:].ctypes.data, pl[1:].ctypes.data) == 0
    assert (buf[:CANARY] == 0xC7).all() and (buf[CANARY + m * stride:] == 0xC7).all(), (what, stride, "bytes written outside the output")
    assert ln[0] == ln[-1] == pl[0] == pl[-1] == 0x5A5A5A5A
    return assert_rows(tab, rows, stride, out, ln[1:-1], pl[1:-1], what)


# ---- a. the host form, one shard ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("stride", ALL_STRIDES, ids=_sid)
def test_gpu_extract_every_row_at_every_stride(rsb, index, stride):
    """rsbwt_extract over all rows and two rows past the index.  The call stages its rows in front of its row block (8 bytes
    a row): with an even and an odd number of rows the block lies 16-byte aligned and 8 bytes off, so a stride that is a
    multiple of 16 goes down the 16-byte path and the dword path; the second call takes the rows in a shuffled order."""
    tab, get = index
    g, n = get(), tab.n
    L = rsb.lib()
    rows = np.concatenate([np.arange(n), [n, n + 5]]).astype(np.uint64)
    fit = _host_extract(L, g, tab, rows, stride, "in order")
    assert 0 < fit < n
    rows = np.concatenate([np.random.default_rng(stride).permutation(n), [n + 5, n, 1 << 40]]).astype(np.uint64)
    assert rows.size % 2 != (n + 2) % 2
    assert _host_extract(L, g, tab, rows, stride, "shuffled") == fit


LAYOUTS = [("reads", 0, True), ("far", 600, False), ("reads-far", 600, True)]


@pytest.mark.parametrize("cls", list(STRIDES))
@pytest.mark.parametrize("lay", LAYOUTS, ids=[x[0] for x in LAYOUTS])
def test_gpu_extract_on_other_line_layouts(rsb, index, lay, cls):
    """the layout changes the walk, not the store path: one long stride per class with a psi hint in every line
    (RSBWT_OPEN_READS), and at a window span whose windows continue in far lines"""
    tab, get = index
    _, span, for_reads = lay
    g, n = get(span, for_reads), tab.n
    L = rsb.lib()
    assert bool(L.rsbwt_opened_for_reads(g.handle)) == for_reads
    if span:
        assert g.window_span() == span and g.far_lines() > 0
    rows = np.concatenate([np.arange(n), [n, n + 5]]).astype(np.uint64)
    for stride in (LONG_PER_CLASS[cls], ONE_PER_CLASS[cls]):
        assert 0 < _host_extract(L, g, tab, rows, stride, lay[0]) < n


# ---- b. the device form, the row block at any alignment -----------------------------------------------------------------------

# 64: the 16-byte path (delta 0), the byte path (1, 2, 3), the dword path (4, 8, 12); 36: dword / byte; 37: byte
DEV_CASES = [(64, d) for d in (0, 1, 2, 3, 4, 8, 12)] + [(36, d) for d in (0, 2, 4)] + [(37, 0), (37, 1)]


def _dev_extract(call, nrows, stride, delta, what):
    """call(d_out, d_len, d_pl) with d_out = base + 64 + delta inside a torch buffer of 0xAB: nothing outside the row block's
    nrows * stride bytes may change.  Gives the block and the two length arrays on the host."""
    import torch
    dev = torch.device("cuda", 0)
    at, size = CANARY + delta, nrows * stride
    base = torch.full((at + size + CANARY + 16,), 0xAB, dtype=torch.uint8, device=dev)
    assert base.data_ptr() % 16 == 0
    d_len = torch.full((nrows + 2,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    d_pl = torch.full((nrows + 2,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    call(C.c_void_p(base.data_ptr() + at), C.c_void_p(d_len.data_ptr() + 4), C.c_void_p(d_pl.data_ptr() + 4))
    torch.cuda.synchronize()
    host = base.cpu().numpy()
    ln, pl = d_len.cpu().numpy().view(np.uint32), d_pl.cpu().numpy().view(np.uint32)
    assert (host[:at] == 0xAB).all() and (host[at + size:] == 0xAB).all(), (what, stride, delta, "bytes written outside the row block")
    assert ln[0] == ln[-1] == pl[0] == pl[-1] == 0x5A5A5A5A
    return host[at:at + size], ln[1:-1], pl[1:-1]


@pytest.mark.parametrize("stride,delta", DEV_CASES, ids=[f"{s}+{d}" for s, d in DEV_CASES])
def test_gpu_extract_dev_misaligned_row_block(rsb, index, stride, delta):
    import torch
    tab, get = index
    g, n = get(), tab.n
    L = rsb.lib()
    d_rows = torch.arange(n, dtype=torch.int64, device=torch.device("cuda", 0))

    def call(d_out, d_len, d_pl):
        assert L.rsbwt_extract_dev(g.handle, C.c_void_p(d_rows.data_ptr()), n, d_out, stride, d_len, d_pl, None) == 0
    out, ln, pl = _dev_extract(call, n, stride, delta, "dev")
    assert 0 < assert_rows(tab, np.arange(n), stride, out, ln, pl, f"dev +{delta}") < n


# ---- c. sets: the padded launch (rsbwt_set_extract*, rsbwt_set_query_var) and the ragged one (rsbwt_set_query_var_capped) -----------------------------------------------------------------------------

@pytest.fixture(scope="module")
def shard_set(rsb):
    tabs = shard_tables()
    gs = [rsb.GpuBWT(runs=t.runs(), num_strings=len(t.reads), ktab_depth=6) for t in tabs]
    ss = rsb.ShardSet(gs)
    yield tabs, ss
    ss.close()
    for g in gs:
        g.close()


@pytest.mark.parametrize("cls", list(STRIDES))
def test_gpu_set_extract_padded_cells(rsb, shard_set, cls):
    """rsbwt_set_extract: one shard gives all its rows, one a single row, one none -- the [S][nmax] block of the one launch
    is mostly padding cells for two of the shards.  Which shard is which turns with the class."""
    tabs, ss = shard_set
    L = rsb.lib()
    stride = ONE_PER_CLASS[cls]
    turn = list(STRIDES).index(cls)
    big, one, none = turn % 3, (turn + 1) % 3, (turn + 2) % 3
    rng = np.random.default_rng(turn)
    rows_big = np.concatenate([rng.permutation(tabs[big].n), [tabs[big].n, 1 << 50]]).astype(np.uint64)
    # the single row: the terminator row of a read that fits (prefix = the whole read)
    row_one = int(np.flatnonzero((tabs[one].len <= stride) & (tabs[one].j == tabs[one].len) & (tabs[one].len > 8))[0])
    sh = np.concatenate([np.full(rows_big.size, big), [one]]).astype(np.uint32)
    rows = np.concatenate([rows_big, [row_one]]).astype(np.uint64)
    order = rng.permutation(rows.size)  # (the caller's order is its own: the single row somewhere in the middle)
    sh, rows = sh[order], rows[order]
    m = rows.size
    buf = np.full(CANARY + m * stride + CANARY, 0xC7, np.uint8)
    out = buf[CANARY:CANARY + m * stride]
    ln, pl = np.full(m, 7, np.uint32), np.full(m, 7, np.uint32)
    assert L.rsbwt_set_extract(ss._s, sh.ctypes.data, rows.ctypes.data, m, out.ctypes.data, stride, ln.ctypes.data, pl.ctypes.data) == 0
    assert (buf[:CANARY] == 0xC7).all() and (buf[CANARY + m * stride:] == 0xC7).all()
    out = out.reshape(m, stride)
    for p in (big, one):
        mine = np.flatnonzero(sh == p)
        assert assert_rows(tabs[p], rows[mine], stride, out[mine], ln[mine], pl[mine], f"shard {p}") > 0
    assert (sh == none).sum() == 0 and (sh == one).sum() == 1


SET_DEV_CASES = [(ONE_PER_CLASS[c], 0) for c in STRIDES] + [(64, 4)]


@pytest.mark.parametrize("stride,delta", SET_DEV_CASES, ids=[f"{s}+{d}" for s, d in SET_DEV_CASES])
def test_gpu_set_extract_dev_every_row_of_every_shard(rsb, shard_set, stride, delta):
    """rsbwt_set_extract_dev: [S][n] with n the largest shard's rows -- every row of every shard; the cells past a smaller
    shard's end name rows it does not have"""
    import torch
    tabs, ss = shard_set
    L = rsb.lib()
    S, n = len(tabs), max(t.n for t in tabs)
    d_rows = torch.arange(n, dtype=torch.int64, device=torch.device("cuda", 0)).repeat(S, 1).contiguous()

    def call(d_out, d_len, d_pl):
        assert L.rsbwt_set_extract_dev(ss._s, C.c_void_p(d_rows.data_ptr()), n, d_out, stride, d_len, d_pl, None) == 0
    out, ln, pl = _dev_extract(call, S * n, stride, delta, "set dev")
    out = out.reshape(S, n, stride)
    for p, t in enumerate(tabs):
        fit = assert_rows(t, np.arange(n), stride, out[p], ln[p * n:(p + 1) * n], pl[p * n:(p + 1) * n], f"shard {p} +{delta}")
        assert 0 < fit < t.n


def _query_var(L, ss, fn, queries, stride, cap_reads):
    bs = [q.encode() for q in queries]
    off = np.zeros(len(bs) + 1, np.uint64)
    off[1:] = np.cumsum([len(b) for b in bs], dtype=np.uint64)
    text = np.frombuffer(b"".join(bs) + b"\0", np.uint8).copy()
    Q = len(bs)
    first = np.full(Q + 1, 99, np.uint64)
    buf = np.full(CANARY + max(cap_reads, 1) * stride + CANARY, 0xC7, np.uint8)
    reads = buf[CANARY:CANARY + max(cap_reads, 1) * stride]
    ln = np.full(max(cap_reads, 1), 7, np.uint32)
    sh = np.full(max(cap_reads, 1), 7, np.uint32)
    matches = np.full(Q, 99, np.uint64)
    n = C.c_size_t()
    p = lambda a: C.c_void_p(a.ctypes.data)
    if fn == "rsbwt_set_query_var":
        rc = L.rsbwt_set_query_var(ss._s, p(text), p(off), Q, p(first), p(sh), p(reads), stride, p(ln), cap_reads, C.byref(n))
        matches = None
    else:
        rc = L.rsbwt_set_query_var_capped(ss._s, p(text), p(off), Q, 0, p(first), p(sh), p(reads), stride, p(ln), cap_reads, C.byref(n), p(matches))
    assert (buf[:CANARY] == 0xC7).all() and (buf[CANARY + max(cap_reads, 1) * stride:] == 0xC7).all()
    return rc, n.value, first, sh, ln, reads, matches


@pytest.fixture(scope="module")
def query_rows(shard_set):
    """per query: [(shard, lower, upper)] of the shards that hold it, from the tables"""
    tabs, qs = shard_set[0], set_queries()
    per = []
    for q in qs:
        ivs = [t.interval(q) if set(q) <= set("ACGT") else (1, 0) for t in tabs]
        per.append([(p, lo, up) for p, (lo, up) in enumerate(ivs) if up >= lo])
    return qs, per


@pytest.mark.parametrize("cls", list(STRIDES))
@pytest.mark.parametrize("fn", ["rsbwt_set_query_var_capped", "rsbwt_set_query_var"])
def test_gpu_set_query_var_reads_at_every_class(rsb, shard_set, query_rows, fn, cls):
    """the reads of queries of lengths of their own.  Of the two entry points only the capped one reaches
    launch_extract_ragged (csrc/sets.hip, query_capped_device: a segment of rows per shard, no padding; that it took this
    path is asserted through rsbwt_set_query_last_work).  rsbwt_set_query_var brings its intervals to the host and hands the
    rows to rsbwt_set_extract's code (set_query_rows -> rsbwt_set_extract_body): launch_extract_wave over a padded
    [S][nmax] block, here with every shard holding a share of the rows.  Query by query, shard ascending, SA row ascending:
    the rows whose suffix starts with the query; reads that do not fit the stride stand among those that do, marked
    UINT32_MAX."""
    tabs, ss = shard_set
    qs, per = query_rows
    L = rsb.lib()
    stride = ONE_PER_CLASS[cls]
    Q = len(qs)
    want_first = np.zeros(Q + 1, np.uint64)
    want_first[1:] = np.cumsum([sum(up - lo + 1 for _, lo, up in x) for x in per])
    total = int(want_first[-1])
    rc, n, first, _, _, _, matches = _query_var(L, ss, fn, qs, stride, 0)
    assert rc == -7 and n == total and np.array_equal(first, want_first)  # RSBWT_ERANGE: the sizes
    rc, n, first, sh, ln, reads, matches = _query_var(L, ss, fn, qs, stride, total)
    assert rc == 0 and n == total and np.array_equal(first, want_first)
    if matches is not None:
        assert np.array_equal(matches, np.diff(want_first))
        w = (C.c_uint64 * 4)()
        L.rsbwt_set_query_last_work(w)
        assert int(w[0]) == total and int(w[1]) == 0  # the rows were made on the device: the ragged launch took them
    want_sh = np.concatenate([np.full(up - lo + 1, p) for x in per for p, lo, up in x]).astype(np.uint32)
    want_rows = np.concatenate([np.arange(lo, up + 1) for x in per for p, lo, up in x]).astype(np.uint64)
    assert np.array_equal(sh, want_sh)
    reads = reads.reshape(total, stride)
    fit = nofit = 0
    for p, t in enumerate(tabs):
        mine = np.flatnonzero(want_sh == p)
        f = assert_rows(t, want_rows[mine], stride, reads[mine], ln[mine], None, f"{fn} shard {p}")
        fit, nofit = fit + f, nofit + mine.size - f
    assert fit > 100 and nofit > 10 and int((ln == NOFIT).sum()) == nofit
    e = qs.index("")
    assert first[e] == first[e + 1]
