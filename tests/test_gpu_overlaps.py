"""Overlaps on the GPU (-m gpu): rsbwt_set_overlaps / _dev / rsbwt_set_overlap_records / rsbwt_set_overlap_reads /
rsbwt_overlaps (csrc/overlaps.hip, csrc/sets.hip, csrc/capi.hip) held bit-exactly to tests/overlap_reference.py, the
definition restated over the oracle: count, ordinal, the records with their order and first[], the reads with overlap[],
ordinal[] and matches[].  The fixture is the gt tests'; the queries are the match tests'; tests/test_overlap_reference.py
shows on the CPU that they reach every class and holds the restatement to a computation without a BWT."""
import ctypes as C
import threading

import numpy as np
import pytest

import gt_reference as G
import overlap_reference as O
import test_kmer_fixtures as F

pytestmark = pytest.mark.gpu

# window spans of the fixture: no continuation, spill chunks, far lines + chunks, far chains, chains of several lines
# (the kinds of tests/test_kmer_fixtures.py, asserted from the builder's own statistics below)
SPANS = {"control": 40, "chunk": 128, "far": 300, "chain": 600, "deep": 2944}
ITEMS = 30     # 15 queries x 2 shards
MAX_READS = 20  # cuts the (query, shard) pairs inside the repeat, leaves their neighbours whole (test_overlap_reference.py)
REC = ("query", "shard", "start", "length", "ordinal", "count", "lower", "upper")


@pytest.fixture(scope="module")
def ref(oracle):
    fx = G.fixture()
    return fx, [G.OracleShard(oracle.from_runs(r, len(sh))) for sh, r in zip(fx.shards, fx.runs())], [O.PlainSide(sh) for sh in fx.shards]


def _open(rsb, fx, span=0, room=False, ktab=6, devices=(0, 0), grouped=False):
    return [rsb.GpuBWT(runs=runs, num_strings=len(sh), ktab_depth=ktab, window_span=span, for_reads=room, device=d, ktab_grouped=grouped)
            for d, sh, runs in zip(devices, fx.shards, fx.runs())]


def _close(ss, gs):
    ss.close()
    for g in gs:
        g.close()


_WANT = {}


def _expected(ref, mo, xo):
    """(count [S][N], ordinal [S][N], (records, first), exp) of the restatement, made once per pair"""
    if (mo, xo) not in _WANT:
        qs = O.queries()
        exp = O.expected(ref[1], "fixture", qs, mo, xo)
        cnt, od = O.flat(exp)
        _WANT[(mo, xo)] = (np.array(cnt, np.uint64), np.array(od, np.uint64), O.records(exp, qs), exp)
    return _WANT[(mo, xo)]


_READS = {}


def _expected_reads(ref, mo, xo, max_reads):
    if (mo, xo, max_reads) not in _READS:
        _READS[(mo, xo, max_reads)] = O.reads_of(_expected(ref, mo, xo)[3], O.queries(), ref[2], max_reads)
    return _READS[(mo, xo, max_reads)]


_STEPS = {}


def _ref_steps(ref, xo):
    if xo not in _STEPS:
        _STEPS[xo] = O.total_lf_steps(ref[1], O.queries(), xo)
    return _STEPS[xo]


def _check_reads(ss, ref, mo, xo, where):
    qs = O.queries()
    for max_reads in (0, MAX_READS):
        efirst, eout, ematches = _expected_reads(ref, mo, xo, max_reads)
        first, strs, ov, od, m = ss.overlap_reads(qs, mo, xo, max_reads, read_stride=64, raw=True)
        assert [int(x) for x in first] == efirst, (where, mo, xo, max_reads)
        assert [int(x) for x in m.ravel()] == ematches, (where, mo, xo, max_reads)
        assert [(int(a), int(b), s) for a, b, s in zip(ov, od, strs)] == eout, (where, mo, xo, max_reads)


def _check(ss, rsb, ref, mo, xo, where, reads=False, T=0):
    """every output of the host calls against the restatement; the work counters of the counting call"""
    qs = O.queries()
    ecnt, eod, (erecs, efirst), _ = _expected(ref, mo, xo)
    cnt, od = ss.overlaps(qs, mo, xo, ordinals=True)
    wk = rsb.ShardSet.overlap_last_work()
    assert cnt.dtype == np.uint64 and cnt.shape == ecnt.shape == (2, 800)
    bad = np.argwhere(cnt != ecnt)
    assert bad.size == 0, (where, mo, xo, bad[:5], cnt[tuple(bad[0])], ecnt[tuple(bad[0])])
    assert (od == eod).all(), (where, mo, xo, np.argwhere(od != eod)[:5])
    assert (ss.overlaps(qs, mo, xo) == ecnt).all(), where  # NULL ordinal
    print(where, mo, xo, wk)
    assert wk["items"] == ITEMS and wk["entries"] == len(erecs), (where, wk)
    assert wk["passes"] <= 2 * (wk["lf_steps"] + wk["items"]), (where, wk)
    assert wk["dollar_only_passes"] <= 2 * wk["items"], (where, wk)
    # a table start saves exactly the T - 1 steps of a T-mer that is there; nothing looks past the step that emptied an
    # item and nothing stops early
    assert wk["lf_steps"] == _ref_steps(ref, xo) - (T - 1) * wk["table_starts"], (where, mo, xo, wk, _ref_steps(ref, xo))
    if T == 0:
        assert wk["table_starts"] == 0, (where, wk)
    recs, first = ss.overlap_records(qs, mo, xo, raw=True)
    got = [tuple(int(r[f]) for f in REC) for r in recs]
    assert got == erecs, (where, mo, xo)
    assert [int(x) for x in first] == efirst and (recs["reserved"] == 0).all()
    assert rsb.ShardSet.overlap_last_work() == wk
    if reads:
        _check_reads(ss, ref, mo, xo, where)
    return wk


def _tabled(mo, xo, T):
    return mo >= T and (xo == 0 or xo >= T)


@pytest.mark.parametrize("min_overlap,max_overlap", O.PARAMS)
def test_gpu_overlaps_is_the_restatement(rsb, ref, min_overlap, max_overlap):
    """at the builder's own span behind 6-mer tables: starts come from the table exactly where no reported depth is
    skipped"""
    gs = _open(rsb, ref[0], room=True)
    ss = rsb.ShardSet(gs)
    try:
        assert all(g.ktab_depth() == 6 for g in gs)
        wk = _check(ss, rsb, ref, min_overlap, max_overlap, "auto", reads=True, T=6)
        assert (wk["table_starts"] > 0) == _tabled(min_overlap, max_overlap, 6), wk
        assert wk["lf_steps"] > 0
        # the nested form of the records
        nested = ss.overlap_records(O.queries(), min_overlap, max_overlap)
        erecs = _expected(ref, min_overlap, max_overlap)[2][0]
        assert [(q, p) + r for q, per in enumerate(nested) for p, cell in enumerate(per) for r in cell] == erecs
    finally:
        _close(ss, gs)


def test_gpu_overlaps_without_a_table_at_the_builders_span(rsb, ref):
    gs = _open(rsb, ref[0], ktab=None)
    ss = rsb.ShardSet(gs)
    try:
        for mo, xo in O.PARAMS:
            _check(ss, rsb, ref, mo, xo, "auto, no table")
    finally:
        _close(ss, gs)


@pytest.mark.parametrize("kind", list(SPANS))
@pytest.mark.parametrize("ktab", [6, None])
def test_gpu_overlaps_on_every_line_layout(rsb, ref, kind, ktab):
    """small spans, spill chunks, far lines and far chains (positions past a line's own pieces go through the scalar
    reader, for the step's symbol and for '$'), behind a k-mer table and without one; without one the LF steps are the
    reference walk's exactly"""
    fx = ref[0]
    span = SPANS[kind]
    gs = _open(rsb, fx, span=span, ktab=ktab, room=True)  # (the layout those kinds are asserted for: lines with room for a psi hint)
    ss = rsb.ShardSet(gs)
    try:
        for g, runs in zip(gs, fx.runs()):
            st = F.selftest(rsb, runs, span, True)
            assert (g.window_span(), g.far_lines(), g.spilled_symbols()) == (span, st[2], st[5])
            F.assert_kind(kind, st)
        for mo, xo in O.PARAMS:
            wk = _check(ss, rsb, ref, mo, xo, (kind, ktab), reads=(mo, xo) in ((1, 0), (10, 30)), T=ktab or 0)
            assert (wk["table_starts"] > 0) == (ktab is not None and _tabled(mo, xo, 6)), (kind, ktab, wk)
    finally:
        _close(ss, gs)


@pytest.mark.parametrize("ktab,grouped", [(6, False), (6, True), (10, False), (10, True)])
def test_gpu_overlaps_table_formats_and_depths(rsb, ref, ktab, grouped):
    """both table formats; (6, 0) on T = 10 may take no table start (depths 6..9 would be skipped), (10, 30) on T = 10
    starts at the first reported depth"""
    gs = _open(rsb, ref[0], ktab=ktab, grouped=grouped)
    ss = rsb.ShardSet(gs)
    try:
        assert all(g.ktab_depth() == ktab and g.ktab_info()[0] == (1 if grouped else 0) for g in gs)
        for mo, xo in O.PARAMS:
            wk = _check(ss, rsb, ref, mo, xo, (ktab, grouped), T=ktab)
            assert (wk["table_starts"] > 0) == _tabled(mo, xo, ktab), (mo, xo, wk)
    finally:
        _close(ss, gs)


def test_gpu_overlaps_single_handle_and_shards_not_opened_for_reads(rsb, ref):
    """only the reads call needs RSBWT_OPEN_READS; rsbwt_overlaps on a handle = the set of that one shard"""
    fx = ref[0]
    qs = O.queries()
    L = rsb.lib()
    gs = _open(rsb, fx, span=SPANS["far"], room=False)
    try:
        assert not any(L.rsbwt_opened_for_reads(g.handle) for g in gs)
        for mo, xo in O.PARAMS:
            ecnt, eod, _, _ = _expected(ref, mo, xo)
            for p, g in enumerate(gs):
                cnt, od = g.overlaps(qs, mo, xo, ordinals=True)
                wk = rsb.ShardSet.overlap_last_work()
                assert (cnt == ecnt[p]).all() and (od == eod[p]).all(), (p, mo, xo)
                assert (g.overlaps(qs, mo, xo) == ecnt[p]).all()
                assert wk["items"] == 15 and wk["entries"] == int((ecnt[p] > 0).sum())
                one = rsb.ShardSet([g])
                try:
                    cnt1, od1 = one.overlaps(qs, mo, xo, ordinals=True)
                    assert (cnt1[0] == cnt).all() and (od1[0] == od).all()
                    assert rsb.ShardSet.overlap_last_work() == wk
                finally:
                    one.close()
        ss = rsb.ShardSet(gs)
        try:
            _check(ss, rsb, ref, 6, 0, "not for reads", T=6)
            with pytest.raises(rsb.RsbwtError) as e:
                ss.overlap_reads(qs, 6)
            assert e.value.code == -1 and "RSBWT_OPEN_READS" in str(e.value)
        finally:
            ss.close()
    finally:
        for g in gs:
            g.close()


def test_gpu_overlaps_on_two_logical_devices(rsb, ref, monkeypatch):
    """a set split over two device groups (two logical devices on GPU 0 where the box has one): each group walks its
    shard's rows of the grid, the host puts them in place -- the one-device answers"""
    L = rsb.lib()
    if L.rsbwt_device_count() < 2:
        monkeypatch.setenv("RSBWT_ENABLE_TEST_HOOKS", "1")
        monkeypatch.setenv("RSBWT_TEST_DEVICE_ALIASES", "2")
    gs = _open(rsb, ref[0], span=SPANS["far"], devices=(0, 1), room=True)
    ss = rsb.ShardSet(gs)
    try:
        assert L.rsbwt_set_devices(ss._s) == 2
        for mo, xo in O.PARAMS:
            _check(ss, rsb, ref, mo, xo, "two devices", reads=True, T=6)
        # a group whose shards do NOT sit next to each other in the set: shard 0 a second time, behind device 1's shard
        fx = ref[0]
        g2 = rsb.GpuBWT(runs=fx.runs()[0], num_strings=len(fx.shards[0]), ktab_depth=6, window_span=SPANS["far"], device=0, for_reads=True)
        s3 = rsb.ShardSet(gs + [g2])
        try:
            assert L.rsbwt_set_devices(s3._s) == 2
            for mo, xo in ((1, 0), (10, 30)):
                ecnt, eod, _, _ = _expected(ref, mo, xo)
                cnt, od = s3.overlaps(O.queries(), mo, xo, ordinals=True)
                for row, p in enumerate((0, 1, 0)):
                    assert (cnt[row] == ecnt[p]).all() and (od[row] == eod[p]).all(), (row, mo, xo)
                assert rsb.ShardSet.overlap_last_work()["items"] == 45
                recs, first = s3.overlap_records(O.queries(), mo, xo, raw=True)
                key = [(int(r["query"]), int(r["shard"]), int(r["start"])) for r in recs]
                assert key == sorted(key) and int(first[-1]) == len(recs)
                cols = ("query", "start", "length", "ordinal", "count", "lower", "upper")
                of = lambda a: [tuple(int(r[f]) for f in cols) for r in recs[recs["shard"] == a]]  # noqa: E731
                assert of(0) == of(2) and (recs["shard"] == 1).any()
                first, strs, ov, od3, m = s3.overlap_reads(O.queries(), mo, xo, MAX_READS, read_stride=64, raw=True)
                assert (m[:, 0] == m[:, 2]).all() and int(first[-1]) == len(strs)
                for q in range(len(O.queries())):
                    a, b, c = (slice(int(first[q * 3 + p]), int(first[q * 3 + p + 1])) for p in range(3))
                    assert strs[a] == strs[c] and (ov[a] == ov[c]).all() and (od3[a] == od3[c]).all()
        finally:
            s3.close()
            g2.close()
    finally:
        _close(ss, gs)


def test_gpu_overlaps_device_resident_form(rsb, ref):
    """rsbwt_set_overlaps_dev: d_pairs inside a larger 0xAB buffer: every entry is defined, nothing outside the array
    changes"""
    import torch
    L = rsb.lib()
    qs = O.queries()
    gs = _open(rsb, ref[0], span=SPANS["far"])
    ss = rsb.ShardSet(gs)
    p = lambda t, byte=0: C.c_void_p(t.data_ptr() + byte)  # noqa: E731
    try:
        text, off = ss._var_text(qs)
        Q, N, S, PAD = len(qs), int(off[-1]), 2, 256
        d_text = torch.from_numpy(text).cuda()
        d_off = torch.from_numpy(off.view(np.int64)).cuda()
        for mo, xo in O.PARAMS:
            ecnt, eod, _, _ = _expected(ref, mo, xo)
            d_pairs = torch.full((PAD + S * N * 16 + PAD,), 0xAB, dtype=torch.uint8, device="cuda")
            rc = L.rsbwt_set_overlaps_dev(ss._s, p(d_text), p(d_off), Q, N, mo, xo, p(d_pairs, PAD), None)
            assert rc == 0, L.rsbwt_last_error()
            torch.cuda.synchronize()
            hp = d_pairs.cpu().numpy()
            assert (hp[:PAD] == 0xAB).all() and (hp[PAD + S * N * 16:] == 0xAB).all()
            pr = hp[PAD:PAD + S * N * 16].view(np.uint64).reshape(S, N, 2)
            assert (pr[:, :, 0] == eod).all() and (pr[:, :, 1] == ecnt).all(), (mo, xo)
        # min_overlap = 0 is 1
        d_pairs = torch.full((S * N * 16,), 0xAB, dtype=torch.uint8, device="cuda")
        assert L.rsbwt_set_overlaps_dev(ss._s, p(d_text), p(d_off), Q, N, 0, 0, p(d_pairs), None) == 0
        torch.cuda.synchronize()
        assert (d_pairs.cpu().numpy().view(np.uint64).reshape(S, N, 2)[:, :, 1] == _expected(ref, 1, 0)[0]).all()
        # nothing to do, nothing touched; null arguments
        d_pairs = torch.full((64,), 0xAB, dtype=torch.uint8, device="cuda")
        assert L.rsbwt_set_overlaps_dev(ss._s, p(d_text), p(d_off), 0, 0, 1, 0, p(d_pairs), None) == 0
        assert L.rsbwt_set_overlaps_dev(ss._s, p(d_text), p(d_off), Q, 0, 1, 0, p(d_pairs), None) == 0
        torch.cuda.synchronize()
        assert (d_pairs.cpu().numpy() == 0xAB).all()
        assert L.rsbwt_set_overlaps_dev(ss._s, p(d_text), p(d_off), Q, N, 1, 0, None, None) == -1
        assert L.rsbwt_set_overlaps_dev(ss._s, None, p(d_off), Q, N, 1, 0, p(d_pairs), None) == -1
    finally:
        _close(ss, gs)


def test_gpu_overlaps_sizing_protocol_and_arguments(rsb, ref):
    """cap = 0 sizes both capped calls' buffers (RSBWT_ERANGE with the count set), a buffer one short is refused with the
    count right, the exact one is filled; max_reads cuts some (query, shard) pairs and leaves their neighbours whole; Q = 0
    is answered; NULL ordinal is fine"""
    L = rsb.lib()
    qs = O.queries()
    gs = _open(rsb, ref[0], room=True)
    ss = rsb.ShardSet(gs)
    pv = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    try:
        text, off = ss._var_text(qs)
        Q, N, S = len(qs), int(off[-1]), 2
        mo, xo = 6, 0
        _, _, (erecs, efirst), _ = _expected(ref, mo, xo)
        # ---- the records
        n = C.c_size_t()
        first = np.zeros(Q * S + 1, np.uint64)
        assert L.rsbwt_set_overlap_records(ss._s, pv(text), pv(off), Q, mo, xo, pv(first), None, 0, C.byref(n)) == -7 and n.value == len(erecs)
        assert [int(x) for x in first] == efirst
        out = np.zeros(len(erecs) + 1, rsb.bwt.OVERLAP)
        out["reserved"][-1] = 0xABAB
        n = C.c_size_t()
        assert L.rsbwt_set_overlap_records(ss._s, pv(text), pv(off), Q, mo, xo, pv(first), pv(out), len(erecs) - 1, C.byref(n)) == -7
        assert n.value == len(erecs) and not out["length"].any()  # (refused: nothing written)
        assert L.rsbwt_set_overlap_records(ss._s, pv(text), pv(off), Q, mo, xo, pv(first), pv(out), len(erecs), C.byref(n)) == 0
        assert n.value == len(erecs) and [tuple(int(r[f]) for f in REC) for r in out[:-1]] == erecs
        assert out["reserved"][-1] == 0xABAB
        # ---- the reads, with a limit that cuts some pairs
        rfirst, rout, rmatches = _expected_reads(ref, mo, xo, MAX_READS)
        whole = _expected_reads(ref, mo, xo, 0)
        cut = [c for c, m in enumerate(rmatches) if m > MAX_READS]
        kept = [c for c, m in enumerate(rmatches) if 0 < m <= MAX_READS]
        assert cut and kept and any(abs(a - b) == 1 for a in cut for b in kept)  # a cut pair beside a whole one
        total = len(rout)
        assert 0 < total < len(whole[1])
        matches = np.zeros(Q * S, np.uint64)
        n = C.c_size_t()
        assert L.rsbwt_set_overlap_reads(ss._s, pv(text), pv(off), Q, mo, xo, MAX_READS, pv(first), None, 64, None, None, None, 0, C.byref(n),
                                         pv(matches)) == -7
        assert n.value == total and [int(x) for x in first] == rfirst and [int(x) for x in matches] == rmatches
        reads = np.zeros((total + 1, 64), np.uint8)
        ln, ov, od = np.zeros(total + 1, np.uint32), np.zeros(total + 1, np.uint32), np.zeros(total + 1, np.uint64)
        reads[-1], ln[-1], ov[-1], od[-1] = 0xAB, 0xABAB, 0xABAB, 0xABAB
        n = C.c_size_t()
        assert L.rsbwt_set_overlap_reads(ss._s, pv(text), pv(off), Q, mo, xo, MAX_READS, pv(first), pv(reads), 64, pv(ln), pv(ov), pv(od),
                                         total - 1, C.byref(n), pv(matches)) == -7
        assert n.value == total and not ln[:-1].any() and not reads[:-1].any()  # (refused: nothing written)
        assert L.rsbwt_set_overlap_reads(ss._s, pv(text), pv(off), Q, mo, xo, MAX_READS, pv(first), pv(reads), 64, pv(ln), pv(ov), pv(od), total,
                                         C.byref(n), None) == 0  # (matches may be NULL)
        got = [(int(ov[r]), int(od[r]), reads[r, :ln[r]].tobytes().decode()) for r in range(total)]
        assert got == rout and n.value == total
        assert (reads[-1] == 0xAB).all() and ln[-1] == ov[-1] == od[-1] == 0xABAB
        for c in cut:
            assert rfirst[c] == rfirst[c + 1]
        for c in kept:
            assert got[rfirst[c]:rfirst[c + 1]] == whole[1][whole[0][c]:whole[0][c + 1]]
        # the nested form
        nested, m = ss.overlap_reads(qs, mo, xo, MAX_READS, read_stride=64)
        assert [x for per in nested for cell in per for x in cell] == rout and [int(x) for x in m.ravel()] == rmatches
        # ---- min_overlap = 0 is 1
        cnt = np.zeros((S, N), np.uint64)
        assert L.rsbwt_set_overlaps(ss._s, pv(text), pv(off), Q, 0, 0, pv(cnt), None) == 0
        assert (cnt == _expected(ref, 1, 0)[0]).all()
        # ---- Q = 0 and N = 0: fine, nothing touched but the sizing calls' counts and first[]
        cnt[:] = 77
        n = C.c_size_t(5)
        f1 = np.full(3, 9, np.uint64)
        assert L.rsbwt_set_overlaps(ss._s, None, None, 0, 1, 0, pv(cnt), None) == 0
        assert L.rsbwt_set_overlap_records(ss._s, None, None, 0, 1, 0, None, None, 0, C.byref(n)) == 0 and n.value == 0
        n = C.c_size_t(5)
        assert L.rsbwt_set_overlap_reads(ss._s, None, None, 0, 1, 0, 0, None, None, 64, None, None, None, 0, C.byref(n), None) == 0 and n.value == 0
        e_off = np.zeros(2, np.uint64)
        assert L.rsbwt_set_overlaps(ss._s, pv(text), pv(e_off), 1, 1, 0, pv(cnt), None) == 0
        n = C.c_size_t(5)
        assert L.rsbwt_set_overlap_records(ss._s, pv(text), pv(e_off), 1, 1, 0, pv(f1), None, 0, C.byref(n)) == 0 and n.value == 0 and not f1.any()
        f1[:] = 9
        n = C.c_size_t(5)
        assert L.rsbwt_set_overlap_reads(ss._s, pv(text), pv(e_off), 1, 1, 0, 0, pv(f1), None, 64, None, None, None, 0, C.byref(n), None) == 0
        assert n.value == 0 and not f1.any()
        assert (cnt == 77).all()
        assert rsb.ShardSet.overlap_last_work() == dict(items=0, lf_steps=0, passes=0, table_starts=0, dollar_only_passes=0, entries=0)
        assert ss.overlaps([], 1).shape == (2, 0) and ss.overlap_records([], 1) == [] and ss.overlap_records([""], 1) == [[[], []]]
        assert ss.overlap_reads([""], 1)[0] == [[[], []]]
        # ---- arguments
        assert L.rsbwt_set_overlaps(ss._s, pv(text), pv(off), Q, 1, 0, None, None) == -1
        assert L.rsbwt_set_overlaps(ss._s, None, pv(off), Q, 1, 0, pv(cnt), None) == -1
        assert L.rsbwt_set_overlaps(ss._s, pv(text), None, Q, 1, 0, pv(cnt), None) == -1
        assert L.rsbwt_set_overlap_records(ss._s, pv(text), pv(off), Q, 1, 0, pv(first), None, 0, None) == -1
        assert L.rsbwt_set_overlap_records(ss._s, pv(text), pv(off), Q, 1, 0, None, None, 0, C.byref(n)) == -1
        assert L.rsbwt_set_overlap_reads(ss._s, pv(text), pv(off), Q, 1, 0, 0, pv(first), None, 0, None, None, None, 0, C.byref(n), None) == -1
        back = off.copy()
        back[3] = back[2] - 1
        assert L.rsbwt_set_overlaps(ss._s, pv(text), pv(back), Q, 1, 0, pv(cnt), None) == -1
        long = np.array([0, 2 ** 31], np.uint64)  # (refused before the text is looked at)
        assert L.rsbwt_set_overlaps(ss._s, pv(text), pv(long), 1, 1, 0, pv(cnt), None) == -1
        assert L.rsbwt_overlaps(gs[0].handle, pv(text), pv(long), 1, 1, 0, pv(cnt), None) == -1
        many = np.array([0, 2 ** 30, 2 ** 31], np.uint64)  # 2^31 positions in one call
        assert L.rsbwt_set_overlaps(ss._s, pv(text), pv(many), 2, 1, 0, pv(cnt), None) == -7
        assert (cnt == 77).all()
    finally:
        _close(ss, gs)


def test_gpu_overlaps_agree_with_locate(rsb, ref):
    """every reported ordinal o: the row getOccAt('$', o + 1) is located as (read_row = row, ordinal = o, offset = 0)"""
    qs = O.queries()
    gs = _open(rsb, ref[0], room=True)
    ss = rsb.ShardSet(gs)
    try:
        first, strs, ov, od, m = ss.overlap_reads(qs, 1, 0, 0, read_stride=64, raw=True)
        assert len(strs) == int(first[-1]) > 100
        shard_of = np.zeros(len(strs), np.uint32)
        for c in range(len(qs) * 2):
            shard_of[int(first[c]):int(first[c + 1])] = c % 2
        rows = np.zeros(len(strs), np.uint64)
        for p, g in enumerate(gs):
            at = np.flatnonzero(shard_of == p)
            rows[at] = g.occ_at_batch("$", od[at] + np.uint64(1))
        rr, lod, lof = ss.locate(shard_of, rows)
        assert (rr == rows).all() and (lod == od).all() and (lof == 0).all()
        # and each row lies in the interval of the record that reported it
        recs, rfirst = ss.overlap_records(qs, 1, 0, raw=True)
        for c in range(len(qs) * 2):
            mine = recs[int(rfirst[c]):int(rfirst[c + 1])]
            for r in range(int(first[c]), int(first[c + 1])):
                rec = mine[mine["length"] == ov[r]]
                assert len(rec) == 1 and rec["lower"][0] <= rows[r] <= rec["upper"][0]
                assert rec["ordinal"][0] <= od[r] < rec["ordinal"][0] + rec["count"][0]
    finally:
        _close(ss, gs)


@pytest.mark.parametrize("ktab", [None, 2])
def test_gpu_overlaps_on_a_shard_of_one_symbol_without_terminators(rsb, ktab):
    """7,037 x 'T' and no '$': no read begins with anything -- 0 everywhere, whatever the intervals hold"""
    runs = np.full(227, (4 << 5) | 31, np.uint8)
    qs = ["A", "T", "TTTT", "ATT"]
    with rsb.GpuBWT(runs=runs, num_strings=0, ktab_depth=ktab) as g:
        ss = rsb.ShardSet([g])
        try:
            for mo, xo in ((1, 0), (2, 0), (1, 2)):
                cnt, od = ss.overlaps(qs, mo, xo, ordinals=True)
                assert cnt.shape == (1, 9) and not cnt.any() and not od.any()
                recs, first = ss.overlap_records(qs, mo, xo, raw=True)
                assert len(recs) == 0 and not first.any()
            ss.overlaps(qs, 1)
            wk = rsb.ShardSet.overlap_last_work()
            assert wk["items"] == 4 and wk["entries"] == 0 and wk["lf_steps"] == 5  # TTTT: 3 steps; ATT: T, T, then A empties it
        finally:
            ss.close()


def test_gpu_overlaps_from_eight_threads(rsb, ref):
    """the calls are re-entrant: eight threads at once get the single-threaded answers and their own work counters"""
    qs = O.queries()
    gs = _open(rsb, ref[0], room=True)
    ss = rsb.ShardSet(gs)
    try:
        want = {pr: _expected(ref, *pr) for pr in O.PARAMS}
        rwant = {pr: _expected_reads(ref, *pr, MAX_READS) for pr in O.PARAMS}
        wk0 = {}
        for pr in O.PARAMS:
            ss.overlaps(qs, *pr, ordinals=True)
            wk0[pr] = rsb.ShardSet.overlap_last_work()
        errs = []

        def work(i):
            try:
                for r in range(5):
                    pr = O.PARAMS[(i + r) % len(O.PARAMS)]
                    cnt, od = ss.overlaps(qs, *pr, ordinals=True)
                    assert (cnt == want[pr][0]).all() and (od == want[pr][1]).all(), (i, r)
                    assert rsb.ShardSet.overlap_last_work() == wk0[pr], (i, r)
                    recs, first = ss.overlap_records(qs, *pr, raw=True)
                    assert [int(x) for x in first] == want[pr][2][1] and len(recs) == len(want[pr][2][0]), (i, r)
                    first, strs, ov, od, m = ss.overlap_reads(qs, *pr, MAX_READS, read_stride=64, raw=True)
                    assert [(int(a), int(b), s) for a, b, s in zip(ov, od, strs)] == rwant[pr][1], (i, r)
            except Exception as e:  # noqa: BLE001
                errs.append(repr(e))
        th = [threading.Thread(target=work, args=(i,)) for i in range(8)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert not errs, errs[:3]
    finally:
        _close(ss, gs)
