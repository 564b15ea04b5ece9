"""SiteMatch candidates on the GPU beyond the gt fixture (-m gpu): rsbwt_set_gt_legs / _reads / _count (csrc/gt_narrow.hip,
csrc/sets.hip) held bit-exactly to tests/gt_reference.py's restatement over the oracle on tests/stream_reference.py's
inputs: run streams in the shapes that broke other kernels on every line layout, with a plain and a grouped k-mer table and
without one (legs only: a stream that is no BWT of reads has no read to extract), sets of two unlike shards, the limits of
M, and the read calls on read sets with duplicate, nested and long reads.  tests/test_gt_stream_reference.py shows on the
CPU what these inputs reach -- among it the reference's (0, 2^64 - 1) corner in mid-search on the streams without '$'."""
import ctypes as C
from collections import Counter

import numpy as np
import pytest

import gt_reference as G
import stream_reference as R
from test_gpu_overlap_streams import GROUPED, PAIRS, SPANS, _assert_layout

pytestmark = pytest.mark.gpu

U32 = 0xFFFFFFFF
NO_ANSWER = ("noleg.end>L", "noleg.start<1", "noleg.cover.leftmost")


def _open(rsb, src, span=0, ktab=6, grouped=False, device=0):
    return rsb.GpuBWT(runs=src.runs, num_strings=src.num_strings, ktab_depth=ktab, window_span=span, for_reads=True, ktab_grouped=grouped,
                      device=device)


def _close(ss, gs):
    ss.close()
    for g in gs:
        g.close()


def _split(qs):
    return [w for w, _ in qs], [p for _, p in qs]


def _check_legs(ss, rsb, srcs, key, qs, M, k, skip, where, legs_only=True):
    """every (tile, leg, shard, a, b, lower, upper) in the set's order -- the wrapper cuts the legs by first[] -- and the
    counters of the call"""
    c = Counter()
    exp = R.gt_expected(srcs, key, qs, k, skip, M, c, legs_only=legs_only)
    got = ss.gt_legs(*_split(qs), k, skip, M)
    wk = rsb.ShardSet.gt_last_work()
    n = 0
    for q in range(len(qs)):
        want = sorted((t, lg, p, a, b, lo, up) for p in range(len(srcs)) for t, lg, a, b, lo, up in exp[q][p][0])
        assert got[q] == want, (where, M, k, skip, q, qs[q], [x for x in got[q] if x not in want][:3], [x for x in want if x not in got[q]][:3])
        n += len(want)
    assert wk["no_answer"] == sum(c[x] for x in NO_ANSWER), (where, M, k, skip, wk, {x: c[x] for x in NO_ANSWER})
    assert wk["legs"] == n and wk["candidates"] == wk["kept"] == wk["extracted"] == 0, (where, wk)
    return n, wk


def _check_reads(ss, rsb, srcs, key, qs, M, k, skip, where, stride=640):
    """reads in read_row order, counts and the candidates counter"""
    exp = R.gt_expected(srcs, key, qs, k, skip, M)
    got = ss.gt_reads(*_split(qs), k, skip, M, read_stride=stride, with_rows=True)
    wk = rsb.ShardSet.gt_last_work()
    cnt = ss.gt_count(*_split(qs), k, skip, M)
    cand = total = 0
    for q in range(len(qs)):
        for p in range(len(srcs)):
            legs, reads = exp[q][p]
            assert got[q][p] == reads, (where, M, k, skip, q, p, qs[q][1])
            assert int(cnt[q, p]) == len(reads), (where, M, k, skip, q, p)
            cand += sum((up - lo + 1) & G.U64 for _, _, _, _, lo, up in legs)
            total += len(reads)
    assert wk["candidates"] == cand, (where, wk, cand)
    assert wk["extracted"] <= wk["kept"] <= wk["candidates"], (where, wk)
    assert rsb.ShardSet.gt_last_work() == wk  # (the count call does the same work)
    return total


@pytest.mark.parametrize("ktab", [6, None])
@pytest.mark.parametrize("kind", list(SPANS))
@pytest.mark.parametrize("name", R.STREAMS)
def test_gpu_gt_legs_on_every_stream_and_layout(rsb, oracle, name, kind, ktab):
    """the first triple of GT_PARAMS and one that rotates with the span (every triple runs on every stream at some span);
    the LF steps spent lengthening are the definition's without a table, and with one at most T - 1 fewer per right
    lengthening whose string the table can start"""
    src = R.source(name, oracle, rsb)
    qs = R.gt_queries(src)
    grouped = ktab is not None and name in GROUPED
    g = _open(rsb, src, SPANS[kind], ktab, grouped)
    ss = rsb.ShardSet([g])
    try:
        _assert_layout(rsb, g, src, kind)
        if ktab is not None:
            assert g.ktab_info()[0] == (1 if grouped else 0)
        T = g.ktab_depth() if ktab is not None else 0
        params = R.gt_params(src)
        for M, k, skip in (params[0], params[1 + list(SPANS).index(kind) % (len(params) - 1)]):
            n, wk = _check_legs(ss, rsb, [src], "small", qs, M, k, skip, (name, kind, ktab))
            assert n > 0
            ref = R.gt_narrow_steps(src, qs, k, skip, M)
            if T < 2:
                assert wk["narrow_steps"] == ref, (name, kind, ktab, M, k, skip, wk, ref)
            else:
                started = R.gt_right_lengthenings(src, qs, k, skip, M, T)
                assert ref - (T - 1) * started <= wk["narrow_steps"] <= ref, (name, kind, ktab, M, k, skip, wk, ref, started)
    finally:
        _close(ss, [g])


@pytest.mark.parametrize("a,span_a,ktab_a,b,span_b,ktab_b", PAIRS, ids=[f"{p[0]}+{p[3]}" for p in PAIRS])
def test_gpu_gt_legs_sets_of_two_unlike_shards(rsb, oracle, a, span_a, ktab_a, b, span_b, ktab_b):
    """a run stream beside a read set's shard, different n, spans, table depths and formats in one launch (the grid's y is
    the shard): each shard's legs are that shard's restatement, in the set's (tile, leg, shard) order"""
    srcs = [R.source(a, oracle, rsb), R.source(b, oracle, rsb)]
    qs = R.gt_queries(srcs[0])
    gs = [_open(rsb, srcs[0], span_a, ktab_a, ktab_a is not None and a in GROUPED), _open(rsb, srcs[1], span_b, ktab_b, ktab_b is not None and b in GROUPED)]
    ss = rsb.ShardSet(gs)
    try:
        assert srcs[0].n != srcs[1].n
        for M, k, skip in R.gt_params(srcs[0]):
            n, _ = _check_legs(ss, rsb, srcs, f"small of {a}", qs, M, k, skip, (a, b))
            assert n > 0
    finally:
        _close(ss, gs)


@pytest.mark.parametrize("name", ["uniform", "nodollar"])
def test_gpu_gt_limits_of_M(rsb, oracle, name):
    """M = n and M = 2^64 - 1: no interval is wider, every all-ACGT tile is one leg 0 with findInterval of the tile;
    M = 0 is 10,000"""
    src = R.source(name, oracle, rsb)
    qs = R.gt_queries(src)
    g = _open(rsb, src, 300, 6)
    ss = rsb.ShardSet([g])
    try:
        for k, skip in ((1, 0), (4, 0), (12, 3)):
            want = []
            for w, pos in qs:
                per = []
                if len(w) >= k and pos <= len(w):
                    for i in range((len(w) - k) // (skip + 1) + 1):
                        s0 = (skip + 1) * i
                        if not set(w[s0:s0 + k]) - set("ACGT"):
                            per.append((i, 0, 0, s0, s0 + k) + src.orc.find(w[s0:s0 + k]))
                want.append(per)
            for M in (src.n, G.U64):
                assert ss.gt_legs(*_split(qs), k, skip, M) == want, (name, k, skip, M)
                wk = rsb.ShardSet.gt_last_work()
                assert wk["no_answer"] == 0 and wk["narrow_steps"] == 0 and wk["legs"] == sum(len(per) for per in want), wk
        for k, skip in ((1, 0), (3, 1)):
            one = ss.gt_legs(*_split(qs), k, skip, 0)
            assert one == ss.gt_legs(*_split(qs), k, skip, 10000), (name, k, skip)
            assert all(((up - lo + 1) & G.U64) <= 10000 for per in one for *_, lo, up in per) and sum(len(per) for per in one) > 0
        if src.n > 4 * 10000:  # a symbol's rows are more than 10,000: its tiles are lengthened
            assert any(lg > 0 for per in ss.gt_legs(*_split(qs), 1, 0, 0) for _, lg, *_ in per)
    finally:
        _close(ss, [g])


def _raw_reads(rsb, ss, qs, M, k, skip, stride):
    """rsbwt_set_gt_reads through the C entry point: (first, reads [n][stride], read_len, read_row)"""
    L = rsb.lib()
    pv = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    text, off = ss._var_text([w for w, _ in qs])
    pos = np.array([p for _, p in qs], np.uint64)
    Q, S = len(qs), len(ss.shards)
    first = np.zeros(Q * S + 1, np.uint64)
    n = C.c_size_t()
    assert L.rsbwt_set_gt_reads(ss._s, pv(text), pv(off), Q, pv(pos), k, skip, M, pv(first), None, stride, None, None, 0, C.byref(n)) == -7
    total = n.value
    reads = np.full((total, stride), 0xAB, np.uint8)
    ln = np.zeros(total, np.uint32)
    rr = np.zeros(total, np.uint64)
    assert L.rsbwt_set_gt_reads(ss._s, pv(text), pv(off), Q, pv(pos), k, skip, M, pv(first), pv(reads), stride, pv(ln), pv(rr), total, C.byref(n)) == 0
    assert n.value == total == int(first[-1])
    return first, reads, ln, rr


@pytest.mark.parametrize("span", [0, 300])
@pytest.mark.parametrize("name", R.FIXTURES)
def test_gpu_gt_reads_on_duplicate_nested_and_long_reads(rsb, oracle, name, span):
    """legs, reads, counts and counters on exact duplicates (repeat), on reads that are prefixes of other reads and reads of
    12 to 600 symbols inside one leg (ragged); on ragged through the C entry point: a stride the long reads do not fit
    (read_len = UINT32_MAX for exactly those) and one that they fit (longer than the internal stride of 256)"""
    src = R.source(name, oracle, rsb)
    qs = R.gt_queries(src)
    g = _open(rsb, src, span, 6)
    ss = rsb.ShardSet([g])
    try:
        for M, k, skip in R.gt_params(src):
            _check_legs(ss, rsb, [src], "small", qs, M, k, skip, (name, span), legs_only=False)
            assert _check_reads(ss, rsb, [src], "small", qs, M, k, skip, (name, span)) > 0
        if name == "ragged":
            M, k, skip = R.gt_params(src)[1]
            exp = R.gt_expected([src], "small", qs, k, skip, M)
            flat = [(q, ident, s) for q in range(len(qs)) for ident, s in exp[q][0][1]]
            assert sum(len(s) > 256 for _, _, s in flat) > 0
            for stride in (128, 640):
                first, reads, ln, rr = _raw_reads(rsb, ss, qs, M, k, skip, stride)
                assert [int(x) for x in first] == list(np.cumsum([0] + [len(exp[q][0][1]) for q in range(len(qs))]))
                assert [int(x) for x in rr] == [ident for _, ident, _ in flat]
                for q in range(len(qs)):
                    cell = rr[int(first[q]):int(first[q + 1])]
                    assert (np.diff(cell.astype(np.int64)) > 0).all(), (stride, q)
                over = [r for r, (_, _, s) in enumerate(flat) if len(s) > stride]
                assert [int(r) for r in np.flatnonzero(ln == U32)] == over and (len(over) > 0) == (stride == 128)
                for r, (_, _, s) in enumerate(flat):
                    if len(s) <= stride:
                        assert int(ln[r]) == len(s) and reads[r, :len(s)].tobytes().decode() == s, (stride, r)
    finally:
        _close(ss, [g])


def test_gpu_gt_reads_on_a_set_of_both_read_sets(rsb, oracle):
    """two shards of reads, different spans, one table: the reads of (query, shard) come from that shard"""
    srcs = [R.source("repeat", oracle, rsb), R.source("ragged", oracle, rsb)]
    qs = R.gt_queries(srcs[1])
    gs = [_open(rsb, srcs[0], 600, None), _open(rsb, srcs[1], 128, 6)]
    ss = rsb.ShardSet(gs)
    try:
        some = [0, 0]
        for M, k, skip in R.gt_params(srcs[1]):
            _check_legs(ss, rsb, srcs, "small of ragged", qs, M, k, skip, "both", legs_only=False)
            _check_reads(ss, rsb, srcs, "small of ragged", qs, M, k, skip, "both")
            exp = R.gt_expected(srcs, "small of ragged", qs, k, skip, M)
            for p in range(2):
                some[p] += sum(len(exp[q][p][1]) for q in range(len(qs)))
                assert all(s in srcs[p].reads for q in range(len(qs)) for _, s in exp[q][p][1])
        assert some[1] > 0
    finally:
        _close(ss, gs)


def test_gpu_gt_text_not_at_the_batch_start(rsb, oracle):
    """off[0] != 0: seven bytes in front of the text and every offset shifted by 7 -- the answers of the plain call"""
    src = R.source("ragged", oracle, rsb)
    qs = R.gt_queries(src)
    L = rsb.lib()
    pv = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    g = _open(rsb, src, 300, 6)
    ss = rsb.ShardSet([g])
    try:
        text, off = ss._var_text([w for w, _ in qs])
        pos = np.array([p for _, p in qs], np.uint64)
        lead = np.frombuffer(b"GATTACA", np.uint8)
        text2, off2 = np.concatenate([lead, text]), off + np.uint64(lead.size)
        Q = len(qs)
        for M, k, skip in R.gt_params(src):
            exp = R.gt_expected([src], "small", qs, k, skip, M)
            want = [(q, t, lg, 0, a, b, lo, up) for q in range(Q) for t, lg, a, b, lo, up in exp[q][0][0]]
            n = C.c_size_t()
            first = np.zeros(Q + 1, np.uint64)
            legs = np.zeros(max(len(want), 1), rsb.bwt.GT_LEG)
            assert L.rsbwt_set_gt_legs(ss._s, pv(text2), pv(off2), Q, pv(pos), k, skip, M, pv(first), pv(legs), len(want), C.byref(n)) == 0
            assert n.value == len(want) > 0
            got = [tuple(int(r[f]) for f in ("query", "tile", "leg", "shard", "a", "b", "lower", "upper")) for r in legs[:n.value]]
            assert got == want, (M, k, skip)
            assert [int(x) for x in first] == list(np.cumsum([0] + [len(exp[q][0][0]) for q in range(Q)]))
            cnt = np.zeros(Q, np.uint64)
            assert L.rsbwt_set_gt_count(ss._s, pv(text2), pv(off2), Q, pv(pos), k, skip, M, pv(cnt)) == 0
            assert [int(x) for x in cnt] == [len(exp[q][0][1]) for q in range(Q)] and cnt.sum() > 0, (M, k, skip)
    finally:
        _close(ss, [g])


def test_gpu_gt_legs_on_two_logical_devices(rsb, oracle, monkeypatch):
    """a read set's shard and the stream without '$' on two device groups (two logical devices on GPU 0 where the box has
    one): each group runs its shard, the host merges -- the one-device legs"""
    L = rsb.lib()
    if L.rsbwt_device_count() < 2:
        monkeypatch.setenv("RSBWT_ENABLE_TEST_HOOKS", "1")
        monkeypatch.setenv("RSBWT_TEST_DEVICE_ALIASES", "2")
    srcs = [R.source("ragged", oracle, rsb), R.source("nodollar", oracle, rsb)]
    qs = R.gt_queries(srcs[0])
    gs = [_open(rsb, srcs[0], 300, 6, device=0), _open(rsb, srcs[1], 128, None, device=1)]
    ss = rsb.ShardSet(gs)
    try:
        assert L.rsbwt_set_devices(ss._s) == 2
        for M, k, skip in R.gt_params(srcs[0]):
            _check_legs(ss, rsb, srcs, "small of ragged", qs, M, k, skip, "two devices")
    finally:
        _close(ss, gs)
