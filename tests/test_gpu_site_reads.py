"""Site reads on the GPU (-m gpu): rsbwt_set_site_reads / rsbwt_set_site_read_counts / rsbwt_set_site_reads_last_work
(csrc/site_reads.hip, csrc/sets.hip) held element for element to the composed call they restate without its host trip,
rsbwt_set_gt_aligned_reads / rsbwt_set_gt_aligned_count -- which tests/test_gpu_gt_align.py holds to gt_reference and
ksw_reference.  Nothing is restated here.  The inputs are tests/site_sets_reference.py's (reads given twice and whole
duplicated reads as windows; reads of 256 to 600 symbols, so the second extraction and neighbours in two buffers; a read of
4,096 symbols; both alleles in one window; pos = 0 and pos = |w| + 1; a shard in which no tile occurs; one string in several
shards) and the gt fixture."""
import ctypes as C
import random

import numpy as np
import pytest

import gt_reference as G
import site_reference as SITE
import site_sets_reference as SS
from test_gpu_site_counts import _close, _cols, _open

pytestmark = pytest.mark.gpu

WORK = ("legs", "narrow_steps", "candidates", "kept", "extracted", "classes", "aligned", "items_kept", "reported")
CASES = [(n, d, p) for n in ("ragged-alleles", "repeat", "exact4096") for d in SS.DEALINGS[n] for p in SS.PARAMS[n]]
# a stride every read of the input fits: a multiple of 16 (slots written 16 bytes a lane) and one that is not (a byte a lane)
STRIDES = {"ragged-alleles": (640, 601), "repeat": (256, 250), "exact4096": (4096,)}
DUPLICATES = {("ragged-alleles", "one"), ("repeat", "one"), ("repeat", "halves")}  # a string twice in ONE shard, and a candidate


class GtSet:
    """the gt fixture's shards and site_reference's batch on it"""

    def __init__(self):
        fx = G.fixture()
        self.shards, self.runs = fx.shards, fx.runs()
        self.reqs, self.alleles = SITE.batch(fx)


@pytest.fixture(scope="module")
def gt():
    return GtSet()


def _both(ss, rsb, reqs, M, k, skip, stride=256):
    """the new call and the composed one on the same requests: (reads with rows, counts, work9) and (reads with rows, counts)"""
    ws, ps, al, ia = _cols(reqs)
    got = ss.site_reads(ws, ps, al, ia, k, skip, M, read_stride=stride, with_rows=True)
    work = rsb.ShardSet.site_reads_last_work()
    cnt = ss.site_read_counts(ws, ps, al, ia, k, skip, M)
    cwork = rsb.ShardSet.site_reads_last_work()
    want = ss.gt_aligned_reads(ws, ps, al, ia, k, skip, M, read_stride=stride, with_rows=True)
    wcnt = ss.gt_aligned_count(ws, ps, al, ia, k, skip, M)
    assert cwork == work, (cwork, work)
    return (got, cnt, work), (want, wcnt)


def _same(ss, rsb, reqs, M, k, skip, where, stride=256):
    (got, cnt, work), (want, wcnt) = _both(ss, rsb, reqs, M, k, skip, stride)
    print(where, work)
    assert tuple(work) == WORK
    assert got == want, (where, next((q, p, a, b) for q, (x, y) in enumerate(zip(got, want)) for p, (a, b) in enumerate(zip(x, y)) if a != b))
    assert cnt.dtype == np.uint64 and cnt.shape == wcnt.shape and (cnt == wcnt).all(), where
    assert [[len(c) for c in row] for row in got] == cnt.tolist()
    total = int(cnt.sum())
    assert work["reported"] == total and work["items_kept"] >= total and work["aligned"] >= work["items_kept"]
    assert work["candidates"] >= work["kept"] and work["extracted"] >= work["classes"] and (work["classes"] > 0) == (work["extracted"] > 0)
    ws, ps, _, _ = _cols(reqs)
    ss.gt_count(ws, ps, k, skip, M)
    gw = rsb.ShardSet.gt_last_work()
    assert [work[x] for x in ("legs", "narrow_steps", "candidates", "kept", "extracted")] == [gw[x] for x in ("legs", "narrow_steps", "candidates", "kept", "extracted")]
    return got, cnt, work


@pytest.mark.parametrize("name,dealing,params", CASES, ids=[f"{n}-{d}-M{p[0]}-k{p[1]}-skip{p[2]}" for n, d, p in CASES])
def test_gpu_site_reads_equal_the_composed_call(rsb, oracle, name, dealing, params):
    """every read set, dealing and parameter triple of site_sets_reference: first, strings, lengths and rows (first in the
    file: without the feature it fails for want of the symbol).  exact4096's third request, whose window is the 4,096
    symbols themselves, has a test of its own below (both calls, every triple): one alignment of 4,096 rows by 4,096
    columns takes seconds, and the comparison here makes seven calls"""
    r = SS.get(oracle, name, dealing)
    reqs = r.reqs[:2] if name == "exact4096" else r.reqs
    gs = _open(rsb, r)
    ss = rsb.ShardSet(gs)
    try:
        got, cnt, work = _same(ss, rsb, reqs, *params, (name, dealing, params), stride=STRIDES[name][0])
        ws, ps, al, ia = _cols(reqs)
        for stride in STRIDES[name][1:]:  # (the slots written a byte a lane)
            assert ss.site_reads(ws, ps, al, ia, params[1], params[2], params[0], read_stride=stride, with_rows=True) == got, stride
        assert cnt.sum() > 0
        if (name, dealing) in DUPLICATES:
            assert work["classes"] < work["extracted"], work
        if name == "ragged-alleles":  # the wide windows keep reads over 256 symbols: the second extraction's buffer is gathered from
            assert any(len(s) > SS.WIDE for q in range(SS.ragged_alleles().narrow, len(r.reqs)) for cell in got[q] for _, s in cell)
        if name == "exact4096":  # the read of 4,096 symbols is a candidate of both windows of 79 (extracted at the wide stride)
            assert work["extracted"] == _without_big(rsb, oracle, reqs, params) + (dealing == "with")
    finally:
        _close(ss, gs)


_LESS = {}


def _without_big(rsb, oracle, reqs, params):
    """`extracted` of the same requests on exact4096 dealt without its read of 4,096 symbols (computed once per triple)"""
    if params not in _LESS:
        r = SS.get(oracle, "exact4096", "without")
        gs = _open(rsb, r)
        ss = rsb.ShardSet(gs)
        try:
            ws, ps, al, ia = _cols(reqs)
            ss.site_read_counts(ws, ps, al, ia, params[1], params[2], params[0])
            _LESS[params] = rsb.ShardSet.site_reads_last_work()["extracted"]
        finally:
            _close(ss, gs)
    return _LESS[params]


@pytest.mark.parametrize("params", SS.PARAMS["exact4096"], ids=lambda p: f"M{p[0]}-k{p[1]}-skip{p[2]}")
def test_gpu_site_reads_a_window_of_4096_symbols(rsb, oracle, params):
    """exact4096's third request: the read of 4,096 symbols against a window that is its own 4,096 symbols, the one request
    it is kept by.  Each call runs that alignment once (seconds), so there are three: the new reads call and the composed
    one with room given up front -- first[], bytes, lengths and rows -- and the new count call, held to the composed
    call's cell sizes, which is what rsbwt_set_gt_aligned_count returns by construction"""
    L = rsb.lib()
    pv = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    ex = SS.exact4096()
    r = SS.get(oracle, "exact4096", "with")
    M, k, skip = params
    gs = _open(rsb, r)
    ss = rsb.ShardSet(gs)
    try:
        ws, ps, al, ia = _cols(ex.reqs[2:])
        text, off = ss._var_text(ws)
        pos, alt, isalt = ss._gt_requests(ws, ps, al, ia)
        out = []
        for fn in (L.rsbwt_set_site_reads, L.rsbwt_set_gt_aligned_reads):
            first, n = np.zeros(3, np.uint64), C.c_size_t()
            reads, ln, rr = np.zeros((16, 4096), np.uint8), np.zeros(16, np.uint32), np.zeros(16, np.uint64)
            assert fn(ss._s, pv(text), pv(off), 1, pv(pos), pv(alt), pv(isalt), k, skip, M, pv(first), pv(reads), 4096, pv(ln), pv(rr), 16, C.byref(n)) == 0
            out.append((n.value, first, ln[:n.value].copy(), rr[:n.value].copy(), [reads[i, :ln[i]].tobytes() for i in range(n.value)]))
        (n0, f0, l0, r0, s0), (n1, f1, l1, r1, s1) = out
        assert n0 == n1 > 0 and (f0 == f1).all() and (l0 == l1).all() and (r0 == r1).all() and s0 == s1
        assert ex.big.encode() in s0 and int(f0[2] - f0[1]) >= 1  # kept, in shard 1
        cnt = ss.site_read_counts(ws, ps, al, ia, k, skip, M)
        assert cnt.tolist() == [[int(f1[1] - f1[0]), int(f1[2] - f1[1])]] and rsb.ShardSet.site_reads_last_work()["reported"] == n0
    finally:
        _close(ss, gs)


def test_gpu_site_reads_report_a_duplicated_string_once(rsb, oracle):
    """a read given twice to one shard and kept by a request is reported once there, under the smaller read_row; the same
    string in another shard is reported there too"""
    r = SS.get(oracle, "repeat", "one")
    reads = r.shards[0]
    twice = {s for s in reads if reads.count(s) > 1}
    gs = _open(rsb, r)
    ss = rsb.ShardSet(gs)
    try:
        ws, ps, al, ia = _cols(r.reqs)
        M, k, skip = SS.PARAMS["repeat"][0]
        got = ss.site_reads(ws, ps, al, ia, k, skip, M, with_rows=True)
        cand = ss.gt_reads(ws, ps, k, skip, M)
        seen = 0
        for q in range(len(ws)):
            strings = [s for _, s in got[q][0]]
            rows = [row for row, _ in got[q][0]]
            assert len(set(strings)) == len(strings) and rows == sorted(rows) and set(strings) <= set(cand[q][0])
            seen += len(twice & set(strings))
        assert seen > 0
    finally:
        _close(ss, gs)
    r2 = SS.get(oracle, "repeat", "halves")
    both = set(r2.shards[0]) & set(r2.shards[1])
    gs = _open(rsb, r2)
    ss = rsb.ShardSet(gs)
    try:
        got = ss.site_reads(ws, ps, al, ia, k, skip, M)
        assert any(both & set(got[q][0]) & set(got[q][1]) for q in range(len(ws)))
    finally:
        _close(ss, gs)


def test_gpu_site_reads_on_the_gt_fixture(rsb, gt):
    """gt_reference's twelve parameter sets on the gt fixture, two shards behind 6-mer tables"""
    gs = _open(rsb, gt)
    ss = rsb.ShardSet(gs)
    try:
        kept = 0
        for M, k, skip in G.PARAMS:
            _, cnt, _ = _same(ss, rsb, gt.reqs, M, k, skip, ("gt", M, k, skip))
            kept += int(cnt.sum())
        assert kept > 0
    finally:
        _close(ss, gs)


@pytest.mark.parametrize("how", [dict(span=128), dict(span=2944), dict(ktab=None), dict(grouped=True)], ids=["S128", "S2944", "notable", "grouped"])
def test_gpu_site_reads_on_line_layouts(rsb, gt, how):
    gs = _open(rsb, gt, **how)
    ss = rsb.ShardSet(gs)
    try:
        _same(ss, rsb, gt.reqs, 3, 8, 3, tuple(how.items()))
    finally:
        _close(ss, gs)


def _two_groups(rsb, monkeypatch):
    if rsb.lib().rsbwt_device_count() < 2:
        monkeypatch.setenv("RSBWT_ENABLE_TEST_HOOKS", "1")
        monkeypatch.setenv("RSBWT_TEST_DEVICE_ALIASES", "2")


@pytest.mark.parametrize("dealing,devices", [("wide4", (0, 1, 1, 0)), ("rr8", (0, 1) * 4)], ids=["wide4", "rr8"])
def test_gpu_site_reads_two_device_groups(rsb, oracle, monkeypatch, dealing, devices):
    """two device groups (two logical devices on GPU 0 where the box has one) whose shards interleave in the set: each lays
    out its own cells and the host puts them at their places"""
    _two_groups(rsb, monkeypatch)
    r = SS.get(oracle, "ragged-alleles", dealing)
    gs = _open(rsb, r, devices=devices)
    ss = rsb.ShardSet(gs)
    try:
        assert rsb.lib().rsbwt_set_devices(ss._s) == 2
        M, k, skip = SS.PARAMS["ragged-alleles"][0]
        _same(ss, rsb, r.reqs, M, k, skip, ("two groups", dealing), stride=640)
    finally:
        _close(ss, gs)


def _raw(rsb, ss, reqs, M, k, skip, stride, cap, rows=True):
    """the C call with room for `cap` reads: (rc, nreads, first, reads, lengths, rows), the arrays marked where untouched"""
    L = rsb.lib()
    pv = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    ws, ps, al, ia = _cols(reqs)
    text, off = ss._var_text(ws)
    pos, alt, isalt = ss._gt_requests(ws, ps, al, ia)
    first = np.full(len(ws) * len(ss.shards) + 1, 0x7A7A, np.uint64)
    reads, ln, rr = np.full((max(cap, 1), stride), 0x7A, np.uint8), np.full(max(cap, 1), 0x7A7A, np.uint32), np.full(max(cap, 1), 0x7A7A, np.uint64)
    n = C.c_size_t(12345)
    rc = L.rsbwt_set_site_reads(ss._s, pv(text), pv(off), len(ws), pv(pos), pv(alt), pv(isalt), k, skip, M, pv(first), pv(reads) if cap else None, stride,
                                pv(ln) if cap else None, pv(rr) if cap and rows else None, cap, C.byref(n))
    return rc, n.value, first, reads, ln, rr


def test_gpu_site_reads_sizing_protocol_and_short_stride(rsb, oracle):
    """cap_reads = 0 is RSBWT_ERANGE with *nreads set, one read short still is, the exact size succeeds and writes every
    slot whole (the read, then zeros); read_row may be NULL; a stride below a kept read's length marks that read with
    UINT32_MAX and leaves the others as they are"""
    r = SS.get(oracle, "ragged-alleles", "one")
    M, k, skip = SS.PARAMS["ragged-alleles"][0]
    gs = _open(rsb, r)
    ss = rsb.ShardSet(gs)
    try:
        ws, ps, al, ia = _cols(r.reqs)
        want = ss.gt_aligned_reads(ws, ps, al, ia, k, skip, M, read_stride=640, with_rows=True)
        flat = [x for row in want for cell in row for x in cell]
        assert any(len(s) > 256 for _, s in flat) and any(len(s) <= 64 for _, s in flat)
        rc, n, first, _, _, _ = _raw(rsb, ss, r.reqs, M, k, skip, 640, 0)
        assert rc == -7 and n == len(flat) and int(first[-1]) == n and rsb.ShardSet.site_reads_last_work() == dict.fromkeys(WORK, 0)
        rc, n, _, _, _, _ = _raw(rsb, ss, r.reqs, M, k, skip, 640, len(flat) - 1)
        assert rc == -7 and n == len(flat)
        for stride in (640, 601):
            rc, n, first2, reads, ln, rr = _raw(rsb, ss, r.reqs, M, k, skip, stride, len(flat))
            assert rc == 0 and n == len(flat) and (first2 == first).all() and rsb.ShardSet.site_reads_last_work()["reported"] == n
            for i, (row, s) in enumerate(flat):
                assert ln[i] == len(s) and rr[i] == row and reads[i, :len(s)].tobytes() == s.encode() and not reads[i, len(s):].any(), (stride, i)
        rc, n, _, reads3, ln3, rr3 = _raw(rsb, ss, r.reqs, M, k, skip, 601, len(flat), rows=False)
        assert rc == 0 and (reads3 == reads).all() and (ln3 == ln).all() and (rr3 == 0x7A7A).all()
        for stride in (64, 61):  # the composed call's marker for the same reads
            rc, n, first4, reads4, ln4, rr4 = _raw(rsb, ss, r.reqs, M, k, skip, stride, len(flat))
            assert rc == 0 and n == len(flat) and (first4 == first).all()
            for i, (row, s) in enumerate(flat):
                if len(s) > stride:
                    assert ln4[i] == 0xFFFFFFFF and rr4[i] == row and not reads4[i].any(), (stride, i)
                else:
                    assert ln4[i] == len(s) and rr4[i] == row and reads4[i, :len(s)].tobytes() == s.encode(), (stride, i)
            assert (ln4 == 0xFFFFFFFF).any() and (ln4 != 0xFFFFFFFF).any()
            with pytest.raises(rsb.RsbwtError):
                ss.site_reads(ws, ps, al, ia, k, skip, M, read_stride=stride)
    finally:
        _close(ss, gs)


def test_gpu_site_reads_empty_batches(rsb, gt):
    """Q = 0; a batch whose tiles occur nowhere; requests that can keep nothing (pos = 0, pos = |w| + 1, k = 0, k > |w|)"""
    L = rsb.lib()
    gs = _open(rsb, gt)
    ss = rsb.ShardSet(gs)
    try:
        assert ss.site_reads([], [], [], [], 8, 3, 3) == [] and ss.site_read_counts([], [], [], [], 8, 3, 3).shape == (0, 2)
        n, first = C.c_size_t(7), np.full(1, 9, np.uint64)
        assert L.rsbwt_set_site_reads(ss._s, None, None, 0, None, None, None, 8, 3, 3, first.ctypes.data_as(C.c_void_p), None, 256, None, None, 0,
                                      C.byref(n)) == 0 and n.value == 0 and first[0] == 0
        rng = random.Random(11)
        have = {s[j:j + 8] for sh in gt.shards for s in sh for j in range(len(s) - 7)}
        none = []
        while len(none) < 5:
            w = "".join(rng.choice("ACGT") for _ in range(40))
            if not any(w[j:j + 8] in have for j in range(0, 33, 4)):  # (the tiles of k = 8, skip = 3)
                none.append((w, 20, "A", len(none) % 2))
        (got, cnt, work), (want, wcnt) = _both(ss, rsb, none, 3, 8, 3)
        assert got == want == [[[], []]] * 5 and not cnt.any() and work["reported"] == 0 and work["extracted"] == 0
        w, p, a, i = gt.reqs[0]
        for reqs, k in (([(w, 0, a, i), (w, len(w) + 1, a, i)], 8), ([(w, p, a, i)], 0), ([(w, p, a, i)], len(w) + 1)):
            (got, cnt, work), (want, wcnt) = _both(ss, rsb, reqs, 3, k, 3)
            assert got == want and not cnt.any() and not wcnt.any(), (reqs, k)
        _, cnt, _ = _same(ss, rsb, [gt.reqs[0], (w, 0, a, i), gt.reqs[1], (w, len(w) + 1, a, i)], 3, 8, 3, "mixed")
        assert cnt[0].sum() + cnt[2].sum() > 0 and not cnt[1].any() and not cnt[3].any()
    finally:
        _close(ss, gs)


def test_gpu_site_reads_permuted_batch_and_repeatability(rsb, oracle):
    """the requests permuted: the answers permute with them; the same batch twice: every output byte the same"""
    r = SS.get(oracle, "ragged-alleles", "wide4")
    M, k, skip = SS.PARAMS["ragged-alleles"][1]
    gs = _open(rsb, r)
    ss = rsb.ShardSet(gs)
    try:
        ws, ps, al, ia = _cols(r.reqs)
        base = ss.site_reads(ws, ps, al, ia, k, skip, M, read_stride=640, with_rows=True)
        order = list(range(len(r.reqs)))
        random.Random(3).shuffle(order)
        reqs = [r.reqs[i] for i in order]
        ws, ps, al, ia = _cols(reqs)
        assert ss.site_reads(ws, ps, al, ia, k, skip, M, read_stride=640, with_rows=True) == [base[i] for i in order]
        n = sum(len(c) for row in base for c in row)
        a, b = _raw(rsb, ss, reqs, M, k, skip, 640, n), _raw(rsb, ss, reqs, M, k, skip, 640, n)
        assert a[0] == b[0] == 0 and a[1] == b[1] == n > 0
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a[2:], b[2:]))
    finally:
        _close(ss, gs)


def test_gpu_site_reads_refusals(rsb, gt):
    """shards not opened for reads; a window of 4,097 symbols; NULL alt; a zero stride: RSBWT_EINVAL, the counters zero"""
    L = rsb.lib()
    pv = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    ws, ps, al, ia = _cols(gt.reqs[:4])
    gs = _open(rsb, gt)
    ss = rsb.ShardSet(gs)
    try:
        for call in (ss.site_reads, ss.site_read_counts):
            with pytest.raises(rsb.RsbwtError) as e:
                call(ws[:3] + ["ACGT" * 1024 + "A"], ps, al, ia, 8, 3, 3)
            assert e.value.code == -1 and "4096" in str(e.value), str(e.value)
            assert rsb.ShardSet.site_reads_last_work() == dict.fromkeys(WORK, 0)
        text, off = ss._var_text(ws)
        pos, alt, isalt = ss._gt_requests(ws, ps, al, ia)
        first, n = np.zeros(4 * 2 + 1, np.uint64), C.c_size_t()
        assert L.rsbwt_set_site_reads(ss._s, pv(text), pv(off), 4, pv(pos), None, pv(isalt), 8, 3, 3, pv(first), None, 256, None, None, 0, C.byref(n)) == -1
        assert L.rsbwt_set_site_reads(ss._s, pv(text), pv(off), 4, pv(pos), pv(alt), pv(isalt), 8, 3, 3, pv(first), None, 0, None, None, 0, C.byref(n)) == -1
        assert L.rsbwt_set_site_reads(ss._s, pv(text), pv(off), 4, pv(pos), pv(alt), pv(isalt), 8, 3, 3, pv(first), None, 256, None, None, 0, None) == -1
        assert L.rsbwt_set_site_reads(None, pv(text), pv(off), 4, pv(pos), pv(alt), pv(isalt), 8, 3, 3, pv(first), None, 256, None, None, 0, C.byref(n)) == -1
        assert L.rsbwt_set_site_read_counts(ss._s, pv(text), pv(off), 4, pv(pos), pv(alt), pv(isalt), 8, 3, 3, None) == -1
    finally:
        _close(ss, gs)
    gs = _open(rsb, gt, room=False)
    ss = rsb.ShardSet(gs)
    try:
        for call in (ss.site_reads, ss.site_read_counts):
            with pytest.raises(rsb.RsbwtError) as e:
                call(ws, ps, al, ia, 8, 3, 3)
            assert e.value.code == -1 and "RSBWT_OPEN_READS" in str(e.value)
    finally:
        _close(ss, gs)
