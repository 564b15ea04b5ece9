"""Matching statistics on the GPU (-m gpu): rsbwt_set_match_lengths / _dev / rsbwt_set_smems / rsbwt_match_lengths
(csrc/match_stats.hip, csrc/sets.hip, csrc/capi.hip) held bit-exactly to tests/match_reference.py, the definition restated
over the oracle: len, lower, upper, the SMEM records, their order and first[].  The fixture is the gt tests'; the queries
and parameter pairs are that module's; tests/test_match_reference.py shows on the CPU that they reach every class of
length (below, at and above both table depths used here, whole reads, zero, whole queries, capped) and holds the
restatement to a computation without a BWT."""
import ctypes as C
import threading

import numpy as np
import pytest

import gt_reference as G
import match_reference as M
import test_kmer_fixtures as F

pytestmark = pytest.mark.gpu

# window spans of the fixture: no continuation, spill chunks, far lines + chunks, far chains, chains of several lines
# (the kinds of tests/test_kmer_fixtures.py, asserted from the builder's own statistics below)
SPANS = {"control": 40, "chunk": 128, "far": 300, "chain": 600, "deep": 2944}
ITEMS = 1600


@pytest.fixture(scope="module")
def ref(oracle):
    fx = G.fixture()
    return fx, [G.OracleShard(oracle.from_runs(r, len(sh))) for sh, r in zip(fx.shards, fx.runs())]


def _open(rsb, fx, span=0, room=False, ktab=6, devices=(0, 0), grouped=False):
    return [rsb.GpuBWT(runs=runs, num_strings=len(sh), ktab_depth=ktab, window_span=span, for_reads=room, device=d, ktab_grouped=grouped)
            for d, sh, runs in zip(devices, fx.shards, fx.runs())]


def _close(ss, gs):
    ss.close()
    for g in gs:
        g.close()


def _expected(ref, max_len, min_rows):
    exp = M.expected(ref[1], "fixture", M.queries(), max_len, min_rows)
    ln, lo, up = M.flat(exp)
    return np.array(ln, np.uint32), np.array(lo, np.uint64), np.array(up, np.uint64), M.smem_records(exp)


def _check(ss, rsb, ref, max_len, min_rows, where):
    """every output of both host calls against the restatement; the work counters of the lengths call"""
    qs = M.queries()
    eln, elo, eup, (erecs, efirst) = _expected(ref, max_len, min_rows)
    ln, lo, up = ss.match_lengths(qs, max_len, min_rows, intervals=True)
    wk = rsb.ShardSet.match_last_work()
    assert ln.dtype == np.uint32 and ln.shape == eln.shape == (2, 800)
    bad = np.argwhere(ln != eln)
    assert bad.size == 0, (where, max_len, min_rows, bad[:5], ln[tuple(bad[0])], eln[tuple(bad[0])])
    assert (lo == elo).all() and (up == eup).all(), (where, max_len, min_rows, np.argwhere((lo != elo) | (up != eup))[:5])
    assert (ss.match_lengths(qs, max_len, min_rows) == eln).all(), where  # NULL lower / upper
    assert wk["items"] == ITEMS and wk["smems"] == 0, (where, wk)
    assert wk["lf_steps"] <= wk["passes"] <= 2 * wk["lf_steps"], (where, wk)
    recs, first = ss.smems(qs, max_len, min_rows, raw=True)
    got = [tuple(int(r[f]) for f in ("query", "shard", "start", "end", "lower", "upper")) for r in recs]
    assert got == erecs, (where, max_len, min_rows)
    assert [int(x) for x in first] == efirst and (recs["reserved"] == 0).all()
    wk2 = rsb.ShardSet.match_last_work()
    assert wk2["smems"] == len(erecs) and {k: v for k, v in wk2.items() if k != "smems"} == {k: v for k, v in wk.items() if k != "smems"}
    return wk


@pytest.mark.parametrize("max_len,min_rows", M.PARAMS)
def test_gpu_match_is_the_restatement(rsb, ref, max_len, min_rows):
    """at the builder's own span behind 6-mer tables: starts come from the table, and a step's two positions are ranked
    off one fetched line (passes < 2 x steps)"""
    gs = _open(rsb, ref[0])
    ss = rsb.ShardSet(gs)
    try:
        assert all(g.ktab_depth() == 6 for g in gs)
        wk = _check(ss, rsb, ref, max_len, min_rows, "auto")
        assert wk["table_starts"] > 0 and wk["lf_steps"] > 0
        assert wk["passes"] < 2 * wk["lf_steps"], wk
        assert wk["passes"] >= wk["lf_steps"], wk
        # the nested form of the SMEMs
        nested = ss.smems(M.queries(), max_len, min_rows)
        erecs = _expected(ref, max_len, min_rows)[3][0]
        assert [(q, p) + r for q, per in enumerate(nested) for p, cell in enumerate(per) for r in cell] == erecs
    finally:
        _close(ss, gs)


@pytest.mark.parametrize("kind", list(SPANS))
@pytest.mark.parametrize("ktab", [6, None])
def test_gpu_match_on_every_line_layout(rsb, ref, kind, ktab):
    """small spans, spill chunks, far lines and far chains (positions past a line's own pieces go through the scalar
    reader), behind a k-mer table and without one"""
    fx = ref[0]
    span = SPANS[kind]
    gs = _open(rsb, fx, span=span, ktab=ktab, room=True)  # (the layout those kinds are asserted for: lines with room for a psi hint)
    ss = rsb.ShardSet(gs)
    try:
        for g, runs in zip(gs, fx.runs()):
            st = F.selftest(rsb, runs, span, True)
            assert (g.window_span(), g.far_lines(), g.spilled_symbols()) == (span, st[2], st[5])
            F.assert_kind(kind, st)
        for max_len, min_rows in M.PARAMS:
            wk = _check(ss, rsb, ref, max_len, min_rows, (kind, ktab))
            assert (wk["table_starts"] == 0 and wk["restarts"] == 0) if ktab is None else wk["table_starts"] > 0, (kind, ktab, wk)
    finally:
        _close(ss, gs)


@pytest.mark.parametrize("ktab,grouped", [(6, False), (6, True), (10, False), (10, True)])
def test_gpu_match_table_formats_and_depths(rsb, ref, ktab, grouped):
    """both table formats, and a table deeper than most matches at min_rows = 20: those entries are refused and the
    lanes start over from initInterval -- the same answers"""
    gs = _open(rsb, ref[0], ktab=ktab, grouped=grouped)
    ss = rsb.ShardSet(gs)
    try:
        assert all(g.ktab_depth() == ktab and g.ktab_info()[0] == (1 if grouped else 0) for g in gs)
        for max_len, min_rows in M.PARAMS:
            wk = _check(ss, rsb, ref, max_len, min_rows, (ktab, grouped))
            assert wk["table_starts"] > 0, wk
            if min_rows == 20:
                assert wk["restarts"] > 0, wk
    finally:
        _close(ss, gs)


def test_gpu_match_single_handle_and_shards_not_opened_for_reads(rsb, ref):
    """no call needs RSBWT_OPEN_READS; rsbwt_match_lengths on a handle = the set of that one shard"""
    fx = ref[0]
    qs = M.queries()
    gs = _open(rsb, fx, span=SPANS["far"], room=False)
    try:
        assert not any(rsb.lib().rsbwt_opened_for_reads(g.handle) for g in gs)
        for max_len, min_rows in M.PARAMS:
            eln, elo, eup, _ = _expected(ref, max_len, min_rows)
            for p, g in enumerate(gs):
                ln, lo, up = g.match_lengths(qs, max_len, min_rows, intervals=True)
                wk = rsb.ShardSet.match_last_work()
                assert (ln == eln[p]).all() and (lo == elo[p]).all() and (up == eup[p]).all(), (p, max_len, min_rows)
                assert (g.match_lengths(qs, max_len, min_rows) == eln[p]).all()
                assert wk["items"] == 800 and wk["lf_steps"] <= wk["passes"] <= 2 * wk["lf_steps"]
                one = rsb.ShardSet([g])
                try:
                    ln1, lo1, up1 = one.match_lengths(qs, max_len, min_rows, intervals=True)
                    assert (ln1[0] == ln).all() and (lo1[0] == lo).all() and (up1[0] == up).all()
                    assert rsb.ShardSet.match_last_work() == wk
                finally:
                    one.close()
    finally:
        for g in gs:
            g.close()


def test_gpu_match_on_two_logical_devices(rsb, ref, monkeypatch):
    """a set split over two device groups (two logical devices on GPU 0 where the box has one): each group runs its
    shard's rows of the grid, the host concatenates -- the one-device answers"""
    L = rsb.lib()
    if L.rsbwt_device_count() < 2:
        monkeypatch.setenv("RSBWT_ENABLE_TEST_HOOKS", "1")
        monkeypatch.setenv("RSBWT_TEST_DEVICE_ALIASES", "2")
    gs = _open(rsb, ref[0], span=SPANS["far"], devices=(0, 1))
    ss = rsb.ShardSet(gs)
    try:
        assert L.rsbwt_set_devices(ss._s) == 2
        for max_len, min_rows in M.PARAMS:
            _check(ss, rsb, ref, max_len, min_rows, "two devices")
        # a group whose shards do NOT sit next to each other in the set: shard 0 a second time, behind device 1's shard
        fx = ref[0]
        g2 = rsb.GpuBWT(runs=fx.runs()[0], num_strings=len(fx.shards[0]), ktab_depth=6, window_span=SPANS["far"], device=0)
        s3 = rsb.ShardSet(gs + [g2])
        try:
            assert L.rsbwt_set_devices(s3._s) == 2
            for max_len, min_rows in ((0, 1), (0, 20)):
                eln, elo, eup, _ = _expected(ref, max_len, min_rows)
                ln, lo, up = s3.match_lengths(M.queries(), max_len, min_rows, intervals=True)
                for row, p in enumerate((0, 1, 0)):
                    assert (ln[row] == eln[p]).all() and (lo[row] == elo[p]).all() and (up[row] == eup[p]).all(), (row, max_len, min_rows)
                assert rsb.ShardSet.match_last_work()["items"] == 2400
                recs, first = s3.smems(M.queries(), max_len, min_rows, raw=True)
                key = [(int(r["query"]), int(r["shard"]), int(r["end"])) for r in recs]
                assert key == sorted(key) and int(first[-1]) == len(recs)
                same = lambda a, b: [tuple(int(r[f]) for f in ("query", "start", "end", "lower", "upper")) for r in recs[recs["shard"] == a]] == \
                    [tuple(int(r[f]) for f in ("query", "start", "end", "lower", "upper")) for r in recs[recs["shard"] == b]]  # noqa: E731
                assert same(0, 2) and (recs["shard"] == 1).any()
        finally:
            s3.close()
            g2.close()
    finally:
        _close(ss, gs)


def test_gpu_match_device_resident_form(rsb, ref):
    """rsbwt_set_match_lengths_dev: d_len and d_pairs inside larger 0xAB buffers, nothing outside them changes; d_pairs
    NULL writes the lengths alone"""
    import torch
    L = rsb.lib()
    qs = M.queries()
    gs = _open(rsb, ref[0], span=SPANS["far"])
    ss = rsb.ShardSet(gs)
    p = lambda t, byte=0: C.c_void_p(t.data_ptr() + byte)  # noqa: E731
    try:
        text, off = ss._var_text(qs)
        Q, N, S, PAD = len(qs), int(off[-1]), 2, 256
        d_text = torch.from_numpy(text).cuda()
        d_off = torch.from_numpy(off.view(np.int64)).cuda()
        for max_len, min_rows in ((0, 1), (16, 1), (0, 20)):
            eln, elo, eup, _ = _expected(ref, max_len, min_rows)
            for with_pairs in (True, False):
                d_len = torch.full((PAD + S * N * 4 + PAD,), 0xAB, dtype=torch.uint8, device="cuda")
                d_pairs = torch.full((PAD + S * N * 16 + PAD,), 0xAB, dtype=torch.uint8, device="cuda")
                rc = L.rsbwt_set_match_lengths_dev(ss._s, p(d_text), p(d_off), Q, N, max_len, min_rows, p(d_len, PAD),
                                                   p(d_pairs, PAD) if with_pairs else None, None)
                assert rc == 0, L.rsbwt_last_error()
                torch.cuda.synchronize()
                hl, hp = d_len.cpu().numpy(), d_pairs.cpu().numpy()
                assert (hl[:PAD] == 0xAB).all() and (hl[PAD + S * N * 4:] == 0xAB).all()
                assert (hp[:PAD] == 0xAB).all() and (hp[PAD + S * N * 16:] == 0xAB).all()
                assert (hl[PAD:PAD + S * N * 4].view(np.uint32).reshape(S, N) == eln).all(), (max_len, min_rows, with_pairs)
                if with_pairs:
                    pr = hp[PAD:PAD + S * N * 16].view(np.uint64).reshape(S, N, 2)
                    assert (pr[:, :, 0] == elo).all() and (pr[:, :, 1] == eup).all(), (max_len, min_rows)
                else:
                    assert (hp == 0xAB).all()
        # nothing to do, nothing touched; null arguments
        d_len = torch.full((64,), 0xAB, dtype=torch.uint8, device="cuda")
        assert L.rsbwt_set_match_lengths_dev(ss._s, p(d_text), p(d_off), 0, 0, 0, 1, p(d_len), None, None) == 0
        assert L.rsbwt_set_match_lengths_dev(ss._s, p(d_text), p(d_off), Q, 0, 0, 1, p(d_len), None, None) == 0
        torch.cuda.synchronize()
        assert (d_len.cpu().numpy() == 0xAB).all()
        assert L.rsbwt_set_match_lengths_dev(ss._s, p(d_text), p(d_off), Q, N, 0, 1, None, None, None) == -1
        assert L.rsbwt_set_match_lengths_dev(ss._s, None, p(d_off), Q, N, 0, 1, p(d_len), None, None) == -1
    finally:
        _close(ss, gs)


def test_gpu_match_sizing_protocol_and_arguments(rsb, ref):
    """cap = 0 sizes rsbwt_set_smems' buffer (RSBWT_ERANGE with the count set), a buffer one short is refused with the
    count right, the exact one is filled; Q = 0 is answered; NULL lower / upper is fine, one of the two is not"""
    L = rsb.lib()
    qs = M.queries()
    gs = _open(rsb, ref[0])
    ss = rsb.ShardSet(gs)
    pv = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    try:
        text, off = ss._var_text(qs)
        Q, N, S = len(qs), int(off[-1]), 2
        eln, elo, eup, (erecs, efirst) = _expected(ref, 0, 3)
        n = C.c_size_t()
        first = np.zeros(Q * S + 1, np.uint64)
        assert L.rsbwt_set_smems(ss._s, pv(text), pv(off), Q, 0, 3, pv(first), None, 0, C.byref(n)) == -7 and n.value == len(erecs)
        assert [int(x) for x in first] == efirst
        out = np.zeros(len(erecs) + 1, rsb.bwt.SMEM)
        out["reserved"][-1] = 0xABAB
        n = C.c_size_t()
        assert L.rsbwt_set_smems(ss._s, pv(text), pv(off), Q, 0, 3, pv(first), pv(out), len(erecs) - 1, C.byref(n)) == -7 and n.value == len(erecs)
        assert not out["end"].any()  # (refused: nothing written)
        assert L.rsbwt_set_smems(ss._s, pv(text), pv(off), Q, 0, 3, pv(first), pv(out), len(erecs), C.byref(n)) == 0 and n.value == len(erecs)
        assert [tuple(int(r[f]) for f in ("query", "shard", "start", "end", "lower", "upper")) for r in out[:-1]] == erecs
        assert out["reserved"][-1] == 0xABAB
        # min_rows = 0 is 1
        ln = np.zeros((S, N), np.uint32)
        assert L.rsbwt_set_match_lengths(ss._s, pv(text), pv(off), Q, 0, 0, pv(ln), None, None) == 0
        assert (ln == _expected(ref, 0, 1)[0]).all()
        # Q = 0 and N = 0: fine, nothing touched
        ln[:] = 77
        n = C.c_size_t(5)
        f1 = np.full(3, 9, np.uint64)
        assert L.rsbwt_set_match_lengths(ss._s, None, None, 0, 0, 1, pv(ln), None, None) == 0
        assert L.rsbwt_set_smems(ss._s, None, None, 0, 0, 1, None, None, 0, C.byref(n)) == 0 and n.value == 0
        e_off = np.zeros(2, np.uint64)
        assert L.rsbwt_set_match_lengths(ss._s, pv(text), pv(e_off), 1, 0, 1, pv(ln), None, None) == 0
        assert L.rsbwt_set_smems(ss._s, pv(text), pv(e_off), 1, 0, 1, pv(f1), None, 0, C.byref(n)) == 0 and n.value == 0 and not f1.any()
        assert (ln == 77).all()
        assert rsb.ShardSet.match_last_work() == dict(items=0, lf_steps=0, passes=0, table_starts=0, restarts=0, smems=0)
        assert ss.match_lengths([]).shape == (2, 0) and ss.smems([]) == [] and ss.smems([""]) == [[[], []]]
        # arguments
        lo = np.zeros((S, N), np.uint64)
        assert L.rsbwt_set_match_lengths(ss._s, pv(text), pv(off), Q, 0, 1, pv(ln), pv(lo), None) == -1
        assert L.rsbwt_set_match_lengths(ss._s, pv(text), pv(off), Q, 0, 1, None, None, None) == -1
        assert L.rsbwt_set_match_lengths(ss._s, None, pv(off), Q, 0, 1, pv(ln), None, None) == -1
        assert L.rsbwt_set_match_lengths(ss._s, pv(text), None, Q, 0, 1, pv(ln), None, None) == -1
        assert L.rsbwt_set_smems(ss._s, pv(text), pv(off), Q, 0, 1, pv(first), None, 0, None) == -1
        assert L.rsbwt_set_smems(ss._s, pv(text), pv(off), Q, 0, 1, None, None, 0, C.byref(n)) == -1
        back = off.copy()
        back[3] = back[2] - 1
        assert L.rsbwt_set_match_lengths(ss._s, pv(text), pv(back), Q, 0, 1, pv(ln), None, None) == -1
        long = np.array([0, 2 ** 31], np.uint64)  # (refused before the text is looked at)
        assert L.rsbwt_set_match_lengths(ss._s, pv(text), pv(long), 1, 0, 1, pv(ln), None, None) == -1
        assert L.rsbwt_match_lengths(gs[0].handle, pv(text), pv(long), 1, 0, 1, pv(ln), None, None) == -1
        assert (ln == 77).all()
    finally:
        _close(ss, gs)


@pytest.mark.parametrize("ktab", [None, 2])
def test_gpu_match_on_a_shard_of_one_symbol_without_terminators(rsb, oracle, ktab):
    """7,037 x 'T' and no '$': initInterval of A is the reference's (0, 2^64 - 1), which holds NO row by the C-ABI's rule
    -- length 0, not a live match; held to the oracle on the same runs"""
    runs = np.full(227, (4 << 5) | 31, np.uint8)
    sh = G.OracleShard(oracle.from_runs(runs, 0))
    assert sh.find("A") == (0, 2 ** 64 - 1) and sh.oix.bwlen() == 7037
    qs = ["A", "T", "TTTT", "ATT"]
    with rsb.GpuBWT(runs=runs, num_strings=0, ktab_depth=ktab) as g:
        ss = rsb.ShardSet([g])
        try:
            for max_len, min_rows in ((0, 1), (2, 1), (0, 7037), (0, 7038)):
                exp = M.expected([sh], ("allT",), qs, max_len, min_rows)
                eln, elo, eup = (np.array(x) for x in M.flat(exp))
                ln, lo, up = ss.match_lengths(qs, max_len, min_rows, intervals=True)
                assert [int(x) for x in ln[0]] == [int(x) for x in eln[0]], (max_len, min_rows)
                assert [int(x) for x in lo[0]] == [int(x) for x in elo[0]] and [int(x) for x in up[0]] == [int(x) for x in eup[0]]
                erecs, efirst = M.smem_records(exp)
                recs, first = ss.smems(qs, max_len, min_rows, raw=True)
                assert [tuple(int(r[f]) for f in ("query", "shard", "start", "end", "lower", "upper")) for r in recs] == erecs
            ln = ss.match_lengths(qs)[0]
            assert [int(x) for x in ln] == [0, 1, 1, 2, 3, 4, 0, 1, 2]
        finally:
            ss.close()


def test_gpu_match_from_eight_threads(rsb, ref):
    """the calls are re-entrant: eight threads at once get the single-threaded answers and their own work counters"""
    qs = M.queries()
    gs = _open(rsb, ref[0])
    ss = rsb.ShardSet(gs)
    try:
        want = {pr: _expected(ref, *pr) for pr in M.PARAMS}
        ss.match_lengths(qs)
        wk0 = {pr: None for pr in M.PARAMS}
        for pr in M.PARAMS:
            ss.match_lengths(qs, *pr, intervals=True)
            wk0[pr] = rsb.ShardSet.match_last_work()
        errs = []

        def work(i):
            try:
                for r in range(6):
                    pr = M.PARAMS[(i + r) % len(M.PARAMS)]
                    ln, lo, up = ss.match_lengths(qs, *pr, intervals=True)
                    assert (ln == want[pr][0]).all() and (lo == want[pr][1]).all() and (up == want[pr][2]).all(), (i, r)
                    assert rsb.ShardSet.match_last_work() == wk0[pr], (i, r)
                    recs, first = ss.smems(qs, *pr, raw=True)
                    assert [int(x) for x in first] == want[pr][3][1] and len(recs) == len(want[pr][3][0]), (i, r)
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
