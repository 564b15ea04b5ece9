"""Extension counts and walks on the GPU (-m gpu): rsbwt_set_extensions / rsbwt_extensions / rsbwt_set_walk / _dev
(csrc/walk.hip, csrc/set_graph.hip, csrc/capi.hip) held bit-exactly to tests/walk_reference.py, the definition restated over
the oracle: the per-shard counts on every seed and on every walk's last state; ext, steps, stop, support and last of the
walks; the work counters.  The fixture is the gt tests' read set as it is and with every other read reverse-complemented,
dealt to 1, 2, 3, 5 and 9 shards (workgroups of 1, 2 and 4 waves; one round, rounds, a last round that is not full);
tests/test_walk_reference.py shows on the CPU that the seeds reach every class of stop and holds the restatement to a
computation without a BWT."""
import ctypes as C
import threading

import numpy as np
import pytest

import gt_reference as G
import walk_reference as W
from kmer_reference import _rc

pytestmark = pytest.mark.gpu

SPANS = {"control": 40, "chunk": 128, "chain": 600}  # the builder's own spans of the line-layout tests
SETTINGS = [(ctx, m, left, both) for ctx in W.CTXS for m in W.MIN_COUNTS for left in (False, True) for both in (False, True)]

_SIDES = {}


def _side(oracle, name, S):
    """the oracle side of read set `name` dealt to S shards"""
    if (name, S) not in _SIDES:
        shards = [G.OracleShard(oracle.from_runs(r, len(sh))) for sh, r in zip(W.dealt(name, S), W.runs(name, S))]
        _SIDES[(name, S)] = W.OracleSide(shards)
    return _SIDES[(name, S)]


def _open(rsb, name, S, span=0, ktab=6, devices=None):
    gs = [rsb.GpuBWT(runs=r, num_strings=len(sh), ktab_depth=ktab, window_span=span, device=(devices[p] if devices else 0))
          for p, (sh, r) in enumerate(zip(W.dealt(name, S), W.runs(name, S)))]
    return rsb.ShardSet(gs), gs


def _close(ss, gs):
    ss.close()
    for g in gs:
        g.close()


def _ref_walks(oracle, name, ctx, m, left, both, max_steps=W.MAX_STEPS):
    """the reference walks: over the two shards as they are -- the support is a sum over the shards, so they are those of
    every dealing (tests/test_walk_reference.py)"""
    return W.walks(_side(oracle, name, 2), (name, "oracle"), W.seeds(ctx), ctx, m, max_steps, left, both)


def _arrays(ws, max_steps):
    """reference walks as rsbwt_set_walk lays them out"""
    Q = len(ws)
    ext, sup = np.zeros((Q, max_steps), np.uint8), np.zeros((Q, max_steps), np.uint32)
    for q, w in enumerate(ws):
        ext[q, :len(w.ext)] = np.frombuffer(w.ext.encode(), np.uint8)
        sup[q, :len(w.ext)] = w.support
    return (ext, np.array([len(w.ext) for w in ws], np.uint32), np.array([w.stop for w in ws], np.uint8), sup,
            np.array([w.last for w in ws], np.uint64).reshape(Q, 4))


def _check_walk(ss, ws, sds, ctx, m, left, both, where, max_steps=W.MAX_STEPS):
    got = ss.walk(sds, ctx, m, max_steps, left, both, supports=True)
    want = [(w.ext, w.stop, w.last, w.support) for w in ws]
    bad = [q for q in range(len(sds)) if got[q] != want[q]]
    assert not bad, (where, ctx, m, left, both, bad[:5], got[bad[0]], want[bad[0]])


def _check_extensions(ss, side, strings, ctx, left, both, where):
    """the per-shard counts of the set call against the reference; returns the reference's"""
    want = np.array([W.extensions(side, s, ctx, left, both) for s in strings], np.uint64).transpose(1, 0, 2)
    got = ss.extensions(strings, ctx, left, both)
    assert got.dtype == np.uint64 and got.shape == want.shape == (side.S, len(strings), 4)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (where, ctx, left, both, len(bad), bad[:5], got[tuple(bad[0])], want[tuple(bad[0])])
    return want


def _check_work(rsb, side, ws, sds, left, both, T, where):
    wk = rsb.ShardSet.walk_last_work()
    searches, steps = W.expected_work(side, ws, left, both)
    print(where, wk, searches, steps)
    assert wk["seeds"] == len(sds) and wk["appended"] == sum(len(w.ext) for w in ws), (where, wk)
    assert wk["searches"] == searches == sum(len(w.contexts) for w in ws) * side.S * 4 * (2 if both else 1), (where, wk, searches)
    # a table start saves exactly the T - 1 steps of a T-mer that is there; nothing looks past the step that emptied a
    # search and nothing stops early
    assert wk["lf_steps"] == steps - (max(T, 1) - 1) * wk["table_starts"], (where, wk, steps)
    assert wk["passes"] <= 2 * wk["lf_steps"] + wk["searches"], (where, wk)
    assert (wk["table_starts"] > 0) == (T > 0), (where, wk)
    return wk


@pytest.mark.parametrize("ktab", [6, None])
@pytest.mark.parametrize("name", ["plain", "stranded"])
def test_gpu_walk_is_the_reference(rsb, oracle, name, ktab):
    """the two shards as they are at the builder's own span, every setting; the work counters where min_count is 1"""
    ss, gs = _open(rsb, name, 2, ktab=ktab)
    side = _side(oracle, name, 2)
    try:
        for ctx, m, left, both in SETTINGS:
            sds = W.seeds(ctx)
            ws = _ref_walks(oracle, name, ctx, m, left, both)
            _check_walk(ss, ws, sds, ctx, m, left, both, (name, ktab))
            if m == 1 and (name == "plain" or both):
                _check_work(rsb, side, ws, sds, left, both, ktab or 0, (name, ktab, ctx, left, both))
            if m == 1:
                _check_extensions(ss, side, sds + [w.final for w in ws], ctx, left, both, (name, ktab))
    finally:
        _close(ss, gs)


@pytest.mark.parametrize("ktab", [6, None])
@pytest.mark.parametrize("kind", list(SPANS))
def test_gpu_walk_on_every_line_layout(rsb, oracle, kind, ktab):
    """small spans, spill chunks and far chains (positions past a line's own pieces go through the scalar reader)"""
    ss, gs = _open(rsb, "plain", 2, span=SPANS[kind], ktab=ktab)
    side = _side(oracle, "plain", 2)
    try:
        assert all(g.window_span() == SPANS[kind] for g in gs)
        for ctx, m, left, both in SETTINGS:
            if m == 3:
                continue
            sds = W.seeds(ctx)
            ws = _ref_walks(oracle, "plain", ctx, m, left, both)
            _check_walk(ss, ws, sds, ctx, m, left, both, (kind, ktab))
            if m == 1 and ctx == 12:
                _check_work(rsb, side, ws, sds, left, both, ktab or 0, (kind, ktab, left, both))
                _check_extensions(ss, side, sds + [w.final for w in ws], ctx, left, both, (kind, ktab))
    finally:
        _close(ss, gs)


@pytest.mark.parametrize("name,ktab", [("plain", 6), ("stranded", None)])
@pytest.mark.parametrize("S", [1, 3, 5, 9])
def test_gpu_walk_on_dealt_sets(rsb, oracle, S, name, ktab):
    """workgroups of 1, 2, 4 and 4 waves: one shard per wave, more (rounds), a last round that is not full (3, 5, 9): the
    walks of every dealing are the same, the per-shard counts are that dealing's; Q = 1, 8, 9 and all"""
    ss, gs = _open(rsb, name, S, ktab=ktab)
    side = _side(oracle, name, S)
    try:
        for ctx, m, left, both in SETTINGS:
            sds = W.seeds(ctx)
            ws = _ref_walks(oracle, name, ctx, m, left, both)
            _check_walk(ss, ws, sds, ctx, m, left, both, (name, S))
            if m == 1 and ctx == 12:
                _check_work(rsb, side, ws, sds, left, both, ktab or 0, (name, S, left, both))
                _check_extensions(ss, side, sds + [w.final for w in ws], ctx, left, both, (name, S))
                for Q in (1, 8, 9):
                    _check_walk(ss, ws[:Q], sds[:Q], ctx, m, left, both, (name, S, Q))
                    want = _check_extensions(ss, side, sds[:Q], ctx, left, both, (name, S, Q))
                    assert rsb.ShardSet.walk_last_work()["seeds"] == Q
                    if S == 1:  # the single handle = the set of that one shard
                        assert (gs[0].extensions(sds[:Q], ctx, left, both) == want[0]).all()
        # the single-handle call on every shard of the dealing
        sds = W.seeds(20)
        want = _check_extensions(ss, side, sds, 20, True, True, (name, S, "handles"))
        for p, g in enumerate(gs):
            got = g.extensions(sds, 20, left=True, both_strands=True)
            assert got.shape == (len(sds), 4) and (got == want[p]).all(), (name, S, p)
    finally:
        _close(ss, gs)


def test_gpu_walk_agrees_with_count_var_of_the_spelled_candidates(rsb, oracle):
    """the parent's way to one evaluation: rsbwt_set_count_var of the four (eight) one-symbol continuations"""
    ss, gs = _open(rsb, "stranded", 3)
    try:
        for ctx, left, both in ((12, False, False), (20, True, True)):
            sds = [s for s in W.seeds(ctx) if W.context(s, ctx, left) is not None]
            cands = [x for s in sds for x in W.candidates(W.context(s, ctx, left), left)]
            cnt = ss.count_var(cands).astype(np.uint64)
            if both:
                cnt = cnt + ss.count_var([_rc(x) for x in cands])
            sup = ss.extensions(sds, ctx, left, both).sum(axis=0)
            assert (sup == cnt.reshape(len(sds), 4)).all(), (ctx, left, both)
            # and a walk of one step decides by those sums
            for (ext, stop, last), row in zip(ss.walk(sds, ctx, 2, 1, left, both), cnt.reshape(len(sds), 4)):
                live = [b for b in range(4) if row[b] >= 2]
                assert (ext, stop) == (("ACGT"[live[0]], W.LIMIT) if len(live) == 1 else ("", W.BRANCH if live else W.DEAD_END))
                assert last == ((0, 0, 0, 0) if len(live) == 1 else tuple(int(x) for x in row))
    finally:
        _close(ss, gs)


def test_gpu_walk_max_steps_one_and_the_limit_inside_the_repeat(rsb, oracle):
    name, ctx, m, left, both = W.IN_REPEAT
    ss, gs = _open(rsb, name, 5)
    try:
        sds = W.seeds(ctx)
        ws = _ref_walks(oracle, name, ctx, m, left, both)
        got = ss.walk(sds, ctx, m, W.MAX_STEPS, left, both)
        inside = [q for q in W.seeds_inside_the_repeat() if ws[q].stop == W.LIMIT]
        assert len(inside) >= 2 and all(got[q] == (ws[q].ext, W.LIMIT, (0, 0, 0, 0)) and len(got[q][0]) == W.MAX_STEPS for q in inside)
        for mx in (1, 2, 63):
            w1 = _ref_walks(oracle, name, ctx, m, left, both, max_steps=mx)
            _check_walk(ss, w1, sds, ctx, m, left, both, ("max_steps", mx), max_steps=mx)
            assert all(w.stop == W.LIMIT for w, full in zip(w1, ws) if len(full.ext) >= mx)
    finally:
        _close(ss, gs)


def test_gpu_walk_device_resident_form(rsb, oracle):
    """rsbwt_set_walk_dev: every output inside 0xAB guard bytes, every byte of every output written, with and without the
    optional ones"""
    import torch
    L = rsb.lib()
    ss, gs = _open(rsb, "plain", 3)
    p = lambda t, byte=0: C.c_void_p(t.data_ptr() + byte) if t is not None else None  # noqa: E731
    PAD = 256
    try:
        for ctx, m, left, both, mx in ((12, 1, False, False, W.MAX_STEPS), (20, 2, True, True, 7)):
            sds = W.seeds(ctx)
            ws = _ref_walks(oracle, "plain", ctx, m, left, both, max_steps=mx)
            want = _arrays(ws, mx)
            text, off = ss._var_text(sds)
            Q, N = len(sds), int(off[-1])
            d_text = torch.from_numpy(text).cuda()
            d_off = torch.from_numpy(off.view(np.int64)).cuda()
            for optional in (True, False):
                sizes = [Q * mx, Q * 4, Q, Q * mx * 4, Q * 32]
                bufs = [torch.full((PAD + n + PAD,), 0xAB, dtype=torch.uint8, device="cuda") for n in sizes]
                ptrs = [p(b, PAD) for b in bufs]
                if not optional:
                    ptrs[3] = ptrs[4] = None
                rc = L.rsbwt_set_walk_dev(ss._s, p(d_text), p(d_off), Q, N, ctx, m, mx, (1 if left else 0) | (2 if both else 0), *ptrs, None)
                assert rc == 0, L.rsbwt_last_error()
                torch.cuda.synchronize()
                for i, (b, n, w) in enumerate(zip(bufs, sizes, want)):
                    hb = b.cpu().numpy()
                    assert (hb[:PAD] == 0xAB).all() and (hb[PAD + n:] == 0xAB).all(), i
                    if i >= 3 and not optional:
                        assert (hb == 0xAB).all(), i
                    else:
                        assert (hb[PAD:PAD + n].view(w.dtype).reshape(w.shape) == w).all(), (i, ctx, optional)
        # nothing to do, nothing touched; null arguments; bad arguments
        buf = torch.full((64,), 0xAB, dtype=torch.uint8, device="cuda")
        assert L.rsbwt_set_walk_dev(ss._s, p(d_text), p(d_off), 0, 0, 12, 1, 4, 0, p(buf), p(buf), p(buf), None, None, None) == 0
        torch.cuda.synchronize()
        assert (buf.cpu().numpy() == 0xAB).all()
        assert L.rsbwt_set_walk_dev(ss._s, p(d_text), p(d_off), 1, N, 12, 1, 4, 0, None, p(buf), p(buf), None, None, None) == -1
        assert L.rsbwt_set_walk_dev(ss._s, None, p(d_off), 1, N, 12, 1, 4, 0, p(buf), p(buf), p(buf), None, None, None) == -1
        assert L.rsbwt_set_walk_dev(ss._s, p(d_text), p(d_off), 1, N, 0, 1, 4, 0, p(buf), p(buf), p(buf), None, None, None) == -1
        assert L.rsbwt_set_walk_dev(ss._s, p(d_text), p(d_off), 1, N, 12, 1, 0, 0, p(buf), p(buf), p(buf), None, None, None) == -1
        assert L.rsbwt_set_walk_dev(ss._s, p(d_text), p(d_off), 1, N, 12, 1, 4, 4, p(buf), p(buf), p(buf), None, None, None) == -1
        assert L.rsbwt_set_walk_dev(ss._s, p(d_text), p(d_off), 1 << 20, N, 12, 1, 1 << 11, 0, p(buf), p(buf), p(buf), None, None, None) == -7
    finally:
        _close(ss, gs)


def test_gpu_walk_on_two_logical_devices(rsb, oracle, monkeypatch):
    """a set split over two device groups (two logical devices on GPU 0 where the box has one), one of them with shards
    that do not sit next to each other: the groups evaluate a step, the host sums and decides -- the one-device answers;
    the device-resident form refuses such a set"""
    L = rsb.lib()
    if L.rsbwt_device_count() < 2:
        monkeypatch.setenv("RSBWT_ENABLE_TEST_HOOKS", "1")
        monkeypatch.setenv("RSBWT_TEST_DEVICE_ALIASES", "2")
    ss, gs = _open(rsb, "stranded", 3, devices=(0, 1, 0))
    side = _side(oracle, "stranded", 3)
    try:
        assert L.rsbwt_set_devices(ss._s) == 2
        for ctx, m, left, both in SETTINGS:
            if m == 3:
                continue
            sds = W.seeds(ctx)
            ws = _ref_walks(oracle, "stranded", ctx, m, left, both)
            _check_walk(ss, ws, sds, ctx, m, left, both, "two devices")
            if m == 1 and ctx == 12:
                _check_work(rsb, side, ws, sds, left, both, 6, ("two devices", left, both))
                _check_extensions(ss, side, sds + [w.final for w in ws], ctx, left, both, "two devices")
        # support and last null: ext, steps and stop of the call that has them
        pv = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
        text, off = ss._var_text(W.seeds(12))
        Q, mx = len(W.seeds(12)), W.MAX_STEPS
        full = [np.full((Q, mx), 77, np.uint8), np.full(Q, 77, np.uint32), np.full(Q, 77, np.uint8)]
        bare = [a.copy() for a in full]
        sup, last = np.zeros((Q, mx), np.uint32), np.zeros((Q, 4), np.uint64)
        assert L.rsbwt_set_walk(ss._s, pv(text), pv(off), Q, 12, 1, mx, 0, *[pv(a) for a in full], pv(sup), pv(last)) == 0
        assert L.rsbwt_set_walk(ss._s, pv(text), pv(off), Q, 12, 1, mx, 0, *[pv(a) for a in bare], None, None) == 0
        assert all((a == b).all() for a, b in zip(full, bare)) and full[1].any() and sup.any() and last.any()
        assert L.rsbwt_set_walk_dev(ss._s, None, None, 0, 0, 12, 1, 4, 0, None, None, None, None, None, None) == -1
        assert b"devices" in L.rsbwt_last_error()
    finally:
        _close(ss, gs)


def test_gpu_walk_arguments(rsb, oracle):
    """the errors of the header, Q = 0, NULL support and last, min_count 0 = 1, off[0] != 0"""
    L = rsb.lib()
    ss, gs = _open(rsb, "plain", 2)
    pv = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    try:
        ctx, mx = 12, 16
        sds = W.seeds(ctx)
        ws = _ref_walks(oracle, "plain", ctx, 1, False, False, max_steps=mx)
        e_ext, e_steps, e_stop, e_sup, e_last = _arrays(ws, mx)
        text, off = ss._var_text(sds)
        Q = len(sds)
        ext, steps, stop = np.full((Q, mx), 77, np.uint8), np.full(Q, 77, np.uint32), np.full(Q, 77, np.uint8)
        sup, last = np.full((Q, mx), 77, np.uint32), np.full((Q, 4), 77, np.uint64)
        cnt = np.full((2, Q, 4), 77, np.uint64)

        def walk(Q=Q, ctx=ctx, m=1, mx=mx, flags=0, text=text, off=off, ext=ext, steps=steps, stop=stop, sup=sup, last=last):
            return L.rsbwt_set_walk(ss._s, pv(text) if text is not None else None, pv(off) if off is not None else None, Q, ctx, m, mx, flags,
                                    pv(ext) if ext is not None else None, pv(steps) if steps is not None else None,
                                    pv(stop) if stop is not None else None, pv(sup) if sup is not None else None,
                                    pv(last) if last is not None else None)
        # ---- refused, nothing written
        assert walk(ctx=0) == -1 and walk(ctx=256) == -1 and walk(mx=0) == -1 and walk(mx=65536) == -1 and walk(flags=4) == -1
        assert walk(flags=0x80000001) == -1
        assert walk(Q=1 << 20, mx=1 << 11) == -7  # Q x max_steps = 2^31 (refused before anything is read)
        assert walk(ext=None) == -1 and walk(steps=None) == -1 and walk(stop=None) == -1 and walk(off=None) == -1 and walk(text=None) == -1
        back = off.copy()
        back[3] = back[2] - 1
        assert walk(off=back) == -1
        for c, f in ((0, 0), (256, 0), (12, 4)):
            assert L.rsbwt_set_extensions(ss._s, pv(text), pv(off), Q, c, f, pv(cnt)) == -1
            assert L.rsbwt_extensions(gs[0].handle, pv(text), pv(off), Q, c, f, pv(cnt)) == -1
        assert L.rsbwt_set_extensions(ss._s, pv(text), pv(off), Q, ctx, 0, None) == -1
        assert L.rsbwt_extensions(None, pv(text), pv(off), Q, ctx, 0, pv(cnt)) == -1
        # ---- Q = 0: fine, nothing touched
        assert walk(Q=0) == 0 and walk(Q=0, text=None, off=None, ext=None, steps=None, stop=None) == 0
        assert L.rsbwt_set_extensions(ss._s, None, None, 0, ctx, 0, None) == 0 and L.rsbwt_extensions(gs[0].handle, None, None, 0, ctx, 0, None) == 0
        for a in (ext, steps, stop, sup, last, cnt):
            assert (a == 77).all()
        assert rsb.ShardSet.walk_last_work() == dict(seeds=0, appended=0, searches=0, lf_steps=0, passes=0, table_starts=0)
        assert ss.walk([], ctx) == [] and ss.extensions([], ctx).shape == (2, 0, 4)
        assert ss.walk(["", "ACGT"], ctx) == [("", W.INVALID, (0, 0, 0, 0))] * 2  # seeds of no symbols at all
        # ---- every output, then NULL support / last
        assert walk() == 0
        assert (ext == e_ext).all() and (steps == e_steps).all() and (stop == e_stop).all() and (sup == e_sup).all() and (last == e_last).all()
        assert stop.min() >= 1
        ext[:], steps[:], stop[:] = 77, 77, 77
        assert walk(sup=None, last=None) == 0
        assert (ext == e_ext).all() and (steps == e_steps).all() and (stop == e_stop).all()
        # ---- min_count = 0 is 1; off[0] != 0: the text pointer is not at the batch's start
        ext[:] = 77
        assert walk(m=0) == 0 and (ext == e_ext).all()
        lead = np.frombuffer(b"GATTACA", np.uint8)
        ext[:] = 77
        assert walk(text=np.concatenate([lead, text]), off=off + np.uint64(lead.size)) == 0 and (ext == e_ext).all() and (last == e_last).all()
    finally:
        _close(ss, gs)


def test_gpu_walk_from_eight_threads(rsb, oracle):
    """the calls are re-entrant: eight threads at once get the single-threaded answers and their own work counters"""
    ss, gs = _open(rsb, "plain", 3)
    side = _side(oracle, "plain", 3)
    try:
        settings = [(12, 1, False, False), (12, 2, True, True), (20, 1, True, False), (20, 3, False, True)]
        want, wk0, ext0 = {}, {}, {}
        for st in settings:
            ctx, m, left, both = st
            ws = _ref_walks(oracle, "plain", *st)
            want[st] = [(w.ext, w.stop, w.last, w.support) for w in ws]
            assert ss.walk(W.seeds(ctx), ctx, m, W.MAX_STEPS, left, both, supports=True) == want[st]
            wk0[st] = rsb.ShardSet.walk_last_work()
            ext0[st] = np.array([W.extensions(side, s, ctx, left, both) for s in W.seeds(ctx)], np.uint64).transpose(1, 0, 2)
        errs = []

        def work(i):
            try:
                for r in range(5):
                    st = settings[(i + r) % len(settings)]
                    ctx, m, left, both = st
                    assert ss.walk(W.seeds(ctx), ctx, m, W.MAX_STEPS, left, both, supports=True) == want[st], (i, r)
                    assert rsb.ShardSet.walk_last_work() == wk0[st], (i, r)
                    assert (ss.extensions(W.seeds(ctx), ctx, left, both) == ext0[st]).all(), (i, r)
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
