"""SiteMatch candidates on the GPU (-m gpu): rsbwt_set_gt_legs / _reads / _count (csrc/gt_narrow.hip, csrc/sets.hip) held
bit-exactly to tests/gt_reference.py, find_gt_reads restated over the oracle.  The fixture, the queries and the parameter
matrix are that module's; tests/test_gt_reference.py shows on the CPU that they reach every branch of the restatement
(single legs, both legs of LEFT / RIGHT / COVERING tiles, the turn-arounds, every "no leg" cause, the unsigned wraps, tiles
with N and lengthenings that run into one) and holds the restatement to a computation without a BWT."""
import ctypes as C
from collections import Counter

import numpy as np
import pytest

import gt_reference as G
import test_kmer_fixtures as F

pytestmark = pytest.mark.gpu

# window spans of the fixture: no continuation, spill chunks, far lines + chunks, far chains, chains of several lines
# (the kinds of tests/test_kmer_fixtures.py, asserted from the builder's own statistics below)
SPANS = {"control": 40, "chunk": 128, "far": 300, "chain": 600, "deep": 2944}


@pytest.fixture(scope="module")
def ref(oracle):
    fx = G.fixture()
    return fx, [G.OracleShard(oracle.from_runs(r, len(sh))) for sh, r in zip(fx.shards, fx.runs())]


def _open(rsb, fx, span=0, room=True, ktab=6, devices=(0, 0)):
    return [rsb.GpuBWT(runs=runs, num_strings=len(sh), ktab_depth=ktab, window_span=span, for_reads=room, device=d)
            for d, sh, runs in zip(devices, fx.shards, fx.runs())]


def _close(ss, gs):
    ss.close()
    for g in gs:
        g.close()


def _check_legs(ss, rsb, ref, M, k, skip, where):
    fx, orc = ref
    qs = fx.queries()
    c = Counter()
    exp = G.expected(orc, "fixture", qs, k, skip, M, c)
    got = ss.gt_legs([w for w, _ in qs], [p for _, p in qs], k, skip, M)
    wk = rsb.ShardSet.gt_last_work()
    assert wk["no_answer"] == c["noleg.end>L"] + c["noleg.start<1"] + c["noleg.cover.leftmost"], (where, wk, dict(c))
    n = 0
    for q in range(len(qs)):
        want = sorted((t, lg, p, a, b, lo, up) for p in range(2) for t, lg, a, b, lo, up in exp[q][p][0])
        assert got[q] == want, (where, M, k, skip, q, qs[q][1])
        n += len(want)
    assert wk["legs"] == n and wk["candidates"] == wk["kept"] == wk["extracted"] == 0, (where, wk)
    return n, wk


def _check_reads(ss, rsb, ref, M, k, skip, where):
    fx, orc = ref
    qs = fx.queries()
    exp = G.expected(orc, "fixture", qs, k, skip, M)
    got = ss.gt_reads([w for w, _ in qs], [p for _, p in qs], k, skip, M, with_rows=True)
    wk = rsb.ShardSet.gt_last_work()
    cnt = ss.gt_count([w for w, _ in qs], [p for _, p in qs], k, skip, M)
    cand = 0
    for q in range(len(qs)):
        for p in range(2):
            legs, reads = exp[q][p]
            assert got[q][p] == reads, (where, M, k, skip, q, p, qs[q][1])
            assert int(cnt[q, p]) == len(reads), (where, M, k, skip, q, p)
            cand += sum((up - lo + 1) & G.U64 for _, _, _, _, lo, up in legs)
    total = sum(len(exp[q][p][1]) for q in range(len(qs)) for p in range(2))
    assert wk["candidates"] == cand, (where, wk, cand)
    assert wk["extracted"] <= wk["kept"] <= wk["candidates"], (where, wk)
    assert rsb.ShardSet.gt_last_work() == wk  # (the count call does the same work)
    return total


@pytest.mark.parametrize("M,k,skip", G.PARAMS)
def test_gpu_gt_matches_the_restatement(rsb, ref, M, k, skip):
    """legs (every a, b, lower, upper), reads in read_row order, counts and the work counters, at the builder's own span"""
    gs = _open(rsb, ref[0])
    ss = rsb.ShardSet(gs)
    try:
        n, wk = _check_legs(ss, rsb, ref, M, k, skip, "auto")
        assert n > 0 and wk["narrow_steps"] > 0
        assert _check_reads(ss, rsb, ref, M, k, skip, "auto") > 0
    finally:
        _close(ss, gs)


@pytest.mark.parametrize("kind", list(SPANS))
@pytest.mark.parametrize("ktab", [6, None])
def test_gpu_gt_on_every_line_layout(rsb, ref, kind, ktab):
    """small spans, spill chunks, far lines and far chains, behind a k-mer table and without one"""
    fx = ref[0]
    span = SPANS[kind]
    gs = _open(rsb, fx, span=span, ktab=ktab)
    ss = rsb.ShardSet(gs)
    try:
        for g, runs in zip(gs, fx.runs()):
            st = F.selftest(rsb, runs, span, True)
            assert (g.window_span(), g.far_lines(), g.spilled_symbols()) == (span, st[2], st[5])
            F.assert_kind(kind, st)
        for M, k, skip in ((1, 8, 0), (8, 12, 3)):
            _check_legs(ss, rsb, ref, M, k, skip, (kind, ktab))
            _check_reads(ss, rsb, ref, M, k, skip, (kind, ktab))
    finally:
        _close(ss, gs)


def test_gpu_gt_strings_shorter_than_the_table_depth(rsb, ref):
    """a table of 10-mers under tiles of 8: the tile and its first lengthenings start from initInterval, the longer strings
    from the table -- the same legs and reads as without a table"""
    gs = _open(rsb, ref[0], ktab=10)
    ss = rsb.ShardSet(gs)
    try:
        assert all(g.ktab_depth() == 10 for g in gs)
        for M in (1, 3):
            _check_legs(ss, rsb, ref, M, 8, 0, "T=10")
            _check_reads(ss, rsb, ref, M, 8, 0, "T=10")
    finally:
        _close(ss, gs)


def test_gpu_gt_on_two_logical_devices(rsb, ref, monkeypatch):
    """a set split over two device groups (two logical devices on GPU 0 where the box has one): each group runs its
    shard, the host merges -- the one-device answers"""
    L = rsb.lib()
    if L.rsbwt_device_count() < 2:
        monkeypatch.setenv("RSBWT_ENABLE_TEST_HOOKS", "1")
        monkeypatch.setenv("RSBWT_TEST_DEVICE_ALIASES", "2")
    gs = _open(rsb, ref[0], span=SPANS["far"], devices=(0, 1))
    ss = rsb.ShardSet(gs)
    try:
        assert L.rsbwt_set_devices(ss._s) == 2
        for M, k, skip in ((3, 8, 3), (1, 12, 0)):
            _check_legs(ss, rsb, ref, M, k, skip, "two devices")
            _check_reads(ss, rsb, ref, M, k, skip, "two devices")
    finally:
        _close(ss, gs)


def test_gpu_gt_sizing_protocol_and_arguments(rsb, ref):
    """cap = 0 sizes the buffers (RSBWT_ERANGE with the count set), a buffer one short is refused, the exact one is
    filled; null arguments and a zero stride are RSBWT_EINVAL; an empty batch and the default M are answered"""
    fx, orc = ref
    L = rsb.lib()
    gs = _open(rsb, fx)
    ss = rsb.ShardSet(gs)
    pv = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    try:
        qs = fx.queries()
        text, off = ss._var_text([w for w, _ in qs])
        pos = np.array([p for _, p in qs], np.uint64)
        Q = len(qs)
        exp = G.expected(orc, "fixture", qs, 8, 3, 3)
        nlegs = sum(len(exp[q][p][0]) for q in range(Q) for p in range(2))
        nreads = sum(len(exp[q][p][1]) for q in range(Q) for p in range(2))
        n = C.c_size_t()
        first = np.zeros(Q + 1, np.uint64)
        assert L.rsbwt_set_gt_legs(ss._s, pv(text), pv(off), Q, pv(pos), 8, 3, 3, pv(first), None, 0, C.byref(n)) == -7 and n.value == nlegs
        assert int(first[Q]) == nlegs
        legs = np.zeros(nlegs, rsb.bwt.GT_LEG)
        assert L.rsbwt_set_gt_legs(ss._s, pv(text), pv(off), Q, pv(pos), 8, 3, 3, pv(first), pv(legs), nlegs - 1, C.byref(n)) == -7
        assert L.rsbwt_set_gt_legs(ss._s, pv(text), pv(off), Q, pv(pos), 8, 3, 3, pv(first), pv(legs), nlegs, C.byref(n)) == 0
        assert [int(x) for x in legs["query"]] == sorted(int(x) for x in legs["query"]) and (legs["reserved"] == 0).all()
        first2 = np.zeros(2 * Q + 1, np.uint64)
        assert L.rsbwt_set_gt_reads(ss._s, pv(text), pv(off), Q, pv(pos), 8, 3, 3, pv(first2), None, 64, None, None, 0, C.byref(n)) == -7
        assert n.value == nreads and int(first2[2 * Q]) == nreads
        reads = np.zeros((nreads, 64), np.uint8)
        ln = np.zeros(nreads, np.uint32)
        assert L.rsbwt_set_gt_reads(ss._s, pv(text), pv(off), Q, pv(pos), 8, 3, 3, pv(first2), pv(reads), 64, pv(ln), None, nreads - 1,
                                    C.byref(n)) == -7
        assert L.rsbwt_set_gt_reads(ss._s, pv(text), pv(off), Q, pv(pos), 8, 3, 3, pv(first2), pv(reads), 64, pv(ln), None, nreads, C.byref(n)) == 0
        assert (ln == G.READ_LEN).all()
        flat = [s for q in range(Q) for p in range(2) for _, s in exp[q][p][1]]
        assert [reads[r, :ln[r]].tobytes().decode() for r in range(nreads)] == flat
        # arguments
        assert L.rsbwt_set_gt_reads(ss._s, pv(text), pv(off), Q, pv(pos), 8, 3, 3, pv(first2), pv(reads), 0, pv(ln), None, nreads, C.byref(n)) == -1
        assert L.rsbwt_set_gt_reads(ss._s, pv(text), pv(off), Q, None, 8, 3, 3, pv(first2), pv(reads), 64, pv(ln), None, nreads, C.byref(n)) == -1
        assert L.rsbwt_set_gt_legs(None, pv(text), pv(off), Q, pv(pos), 8, 3, 3, pv(first), pv(legs), nlegs, C.byref(n)) == -1
        assert L.rsbwt_set_gt_legs(ss._s, pv(text), pv(off), Q, pv(pos), 8, 3, 3, pv(first), pv(legs), nlegs, None) == -1
        assert L.rsbwt_set_gt_count(ss._s, pv(text), pv(off), Q, pv(pos), 8, 3, 3, None) == -1
        assert L.rsbwt_set_gt_legs(ss._s, None, None, 0, None, 8, 3, 3, None, None, 0, C.byref(n)) == 0 and n.value == 0
        # M = 0 is 10,000: no interval of this fixture is that wide, so every ACGT tile is one leg
        one = ss.gt_legs([w for w, _ in qs], pos, 8, 3, 0)
        assert all(lg == 0 for per in one for _, lg, *_ in per) and sum(len(per) for per in one) > nlegs // 4
        assert one == ss.gt_legs([w for w, _ in qs], pos, 8, 3, 10000)
    finally:
        _close(ss, gs)


@pytest.mark.parametrize("k,skip", [(0, 0), (-3, 0), (8, -1), (0, -1)])
def test_gpu_gt_degenerate_parameters_contribute_nothing(rsb, ref, k, skip):
    """k <= 0 or skip < 0 through the C-ABI: every call succeeds, no legs, no reads, zero counts, first[] all zero and
    every work counter zero -- after a call that did work, so that nothing is left over from it"""
    fx = ref[0]
    L = rsb.lib()
    gs = _open(rsb, fx)
    ss = rsb.ShardSet(gs)
    pv = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    try:
        qs = fx.queries()
        text, off = ss._var_text([w for w, _ in qs])
        pos = np.array([p for _, p in qs], np.uint64)
        Q = len(qs)
        zero = dict(legs=0, no_answer=0, narrow_steps=0, candidates=0, kept=0, extracted=0)
        n = C.c_size_t(7)
        for call in ("legs", "reads", "count"):
            assert ss.gt_count([w for w, _ in qs], pos, 8, 3, 3).sum() > 0 and rsb.ShardSet.gt_last_work() != zero
            if call == "legs":
                first = np.full(Q + 1, 99, np.uint64)
                rc = L.rsbwt_set_gt_legs(ss._s, pv(text), pv(off), Q, pv(pos), k, skip, 3, pv(first), None, 0, C.byref(n))
            elif call == "reads":
                first = np.full(2 * Q + 1, 99, np.uint64)
                rc = L.rsbwt_set_gt_reads(ss._s, pv(text), pv(off), Q, pv(pos), k, skip, 3, pv(first), None, 64, None, None, 0, C.byref(n))
            else:
                first = np.full(2 * Q, 99, np.uint64)
                rc = L.rsbwt_set_gt_count(ss._s, pv(text), pv(off), Q, pv(pos), k, skip, 3, pv(first))
                n = C.c_size_t(0)
            assert rc == 0, (call, L.rsbwt_last_error())
            assert n.value == 0 and not first.any(), (call, first)
            assert rsb.ShardSet.gt_last_work() == zero, call
            n = C.c_size_t(7)
        assert ss.gt_legs([w for w, _ in qs], pos, k, skip, 3) == [[] for _ in qs]
        assert ss.gt_reads([w for w, _ in qs], pos, k, skip, 3) == [[[], []] for _ in qs]
    finally:
        _close(ss, gs)


def test_gpu_gt_shards_not_opened_for_reads(rsb, ref):
    """the legs need no RSBWT_OPEN_READS; the read calls refuse such a set with RSBWT_EINVAL"""
    fx = ref[0]
    gs = _open(rsb, fx, span=SPANS["far"], room=False)
    ss = rsb.ShardSet(gs)
    try:
        assert not any(rsb.lib().rsbwt_opened_for_reads(g.handle) for g in gs)
        _check_legs(ss, rsb, ref, 3, 8, 0, "plain")
        qs = fx.queries()
        for call in (ss.gt_reads, ss.gt_count):
            with pytest.raises(rsb.RsbwtError) as e:
                call([w for w, _ in qs], [p for _, p in qs], 8, 0, 3)
            assert e.value.code == -1
    finally:
        _close(ss, gs)
