"""Unitigs on the GPU (-m gpu): rsbwt_set_unitigs / _dev (csrc/walk.hip's unitig_kernel, csrc/set_graph.hip) held bit-exactly to
tests/unitig_reference.py, the definition stated over the oracle: ext, steps, stop, support and last of both sides of every
seed, and all eight work counters.  The fixture is the walk tests': the gt read set as it is and with every other read
reverse-complemented, dealt to 1, 2, 3, 5 and 9 shards (workgroups of 1, 2 and 4 waves; one round, rounds, a last round
that is not full); tests/test_unitig_reference.py shows on the CPU that the seeds reach every class of stop, JOIN at 0
steps included, and holds the statement to a computation without a BWT."""
import ctypes as C
import threading

import numpy as np
import pytest

import gt_reference as G
import unitig_reference as U
import walk_reference as W

pytestmark = pytest.mark.gpu

SPANS = {"control": 40, "chunk": 128, "chain": 600}  # the builder's own spans of the line-layout tests
SETTINGS = [(ctx, m, both) for ctx in W.CTXS for m in W.MIN_COUNTS for both in (False, True)]
WORK = ("seeds", "appended", "searches", "lf_steps", "passes", "table_starts", "onward", "back")

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


def _ref(oracle, name, ctx, m, both, max_steps=W.MAX_STEPS):
    """the reference unitigs: over the two shards as they are -- the support is a sum over the shards, so they are those
    of every dealing (tests/test_unitig_reference.py)"""
    return U.unitigs(_side(oracle, name, 2), (name, "oracle"), U.seeds(ctx), ctx, m, max_steps, both)


def _want(us):
    return [tuple((s.ext, s.stop, s.last, s.support) for s in pair) for pair in us]


def _arrays(us, max_steps):
    """reference unitigs as rsbwt_set_unitigs lays them out"""
    Q = len(us)
    ext, sup = np.zeros((Q, 2, max_steps), np.uint8), np.zeros((Q, 2, max_steps), np.uint32)
    for q, pair in enumerate(us):
        for d, s in enumerate(pair):
            ext[q, d, :len(s.ext)] = np.frombuffer(s.ext.encode(), np.uint8)
            sup[q, d, :len(s.ext)] = s.support
    return (ext, np.array([[len(s.ext) for s in pair] for pair in us], np.uint32), np.array([[s.stop for s in pair] for pair in us], np.uint8),
            sup, np.array([[s.last for s in pair] for pair in us], np.uint64).reshape(Q, 2, 8))


def _check(ss, us, sds, ctx, m, both, where, max_steps=W.MAX_STEPS):
    got = ss.unitigs(sds, ctx, m, max_steps, both, supports=True)
    want = _want(us)
    bad = [q for q in range(len(sds)) if got[q] != want[q]]
    assert not bad, (where, ctx, m, both, bad[:5], got[bad[0]], want[bad[0]])


def _check_work(rsb, side, us, sds, both, T, where):
    wk = rsb.ShardSet.unitigs_last_work()
    ex = U.expected_work(side, us, both)
    print(where, wk, ex)
    assert tuple(wk) == WORK
    assert wk["seeds"] == len(sds) and wk["appended"] == ex["appended"], (where, wk, ex)
    assert wk["onward"] == ex["onward"] and wk["back"] == ex["back"], (where, wk, ex)
    assert wk["searches"] == ex["searches"] == (ex["onward"] + ex["back"]) * side.S * 4 * (2 if both else 1), (where, wk, ex)
    # a table start saves exactly the T - 1 steps of a T-mer that is there; nothing looks past the step that emptied a
    # search and nothing stops early
    assert wk["lf_steps"] == ex["lf_steps"] - (max(T, 1) - 1) * wk["table_starts"], (where, wk, ex)
    assert wk["passes"] <= 2 * wk["lf_steps"] + wk["searches"], (where, wk)
    assert (wk["table_starts"] > 0) == (T > 0), (where, wk)
    return wk


@pytest.mark.parametrize("ktab", [6, None])
@pytest.mark.parametrize("name", ["plain", "stranded"])
def test_gpu_unitigs_are_the_reference(rsb, oracle, name, ktab):
    """the two shards as they are at the builder's own span, every setting; the work counters where min_count is 1"""
    ss, gs = _open(rsb, name, 2, ktab=ktab)
    side = _side(oracle, name, 2)
    try:
        for ctx, m, both in SETTINGS:
            sds = U.seeds(ctx)
            us = _ref(oracle, name, ctx, m, both)
            _check(ss, us, sds, ctx, m, both, (name, ktab))
            if m == 1 and (name == "plain" or both):
                _check_work(rsb, side, us, sds, both, ktab or 0, (name, ktab, ctx, both))
    finally:
        _close(ss, gs)


@pytest.mark.parametrize("ktab", [6, None])
@pytest.mark.parametrize("kind", list(SPANS))
def test_gpu_unitigs_on_every_line_layout(rsb, oracle, kind, ktab):
    """small spans, spill chunks and far chains (positions past a line's own pieces go through the scalar reader)"""
    ss, gs = _open(rsb, "plain", 2, span=SPANS[kind], ktab=ktab)
    side = _side(oracle, "plain", 2)
    try:
        assert all(g.window_span() == SPANS[kind] for g in gs)
        for ctx, m, both in SETTINGS:
            if m == 3:
                continue
            sds = U.seeds(ctx)
            us = _ref(oracle, "plain", ctx, m, both)
            _check(ss, us, sds, ctx, m, both, (kind, ktab))
            if m == 1 and ctx == 12:
                _check_work(rsb, side, us, sds, both, ktab or 0, (kind, ktab, both))
    finally:
        _close(ss, gs)


@pytest.mark.parametrize("name,ktab", [("plain", 6), ("stranded", None)])
@pytest.mark.parametrize("S", [1, 3, 5, 9])
def test_gpu_unitigs_on_dealt_sets(rsb, oracle, S, name, ktab):
    """workgroups of 1, 2, 4 and 4 waves: one shard per wave, more (rounds), a last round that is not full (3, 5, 9): the
    unitigs of every dealing are the same; Q = 1 (two items of eight), 3, 4 (exactly one workgroup), 5 (a second workgroup
    with two items) and all"""
    ss, gs = _open(rsb, name, S, ktab=ktab)
    side = _side(oracle, name, S)
    try:
        for ctx, m, both in SETTINGS:
            sds = U.seeds(ctx)
            us = _ref(oracle, name, ctx, m, both)
            _check(ss, us, sds, ctx, m, both, (name, S))
            if m == 1 and ctx == 12:
                _check_work(rsb, side, us, sds, both, ktab or 0, (name, S, both))
                for Q in (1, 3, 4, 5):
                    _check(ss, us[:Q], sds[:Q], ctx, m, both, (name, S, Q))
                    _check_work(rsb, side, us[:Q], sds[:Q], both, ktab or 0, (name, S, both, Q))
    finally:
        _close(ss, gs)


def test_gpu_unitigs_agree_with_extensions_composed_by_the_rule(rsb, oracle):
    """the parent's way to the same answers: a host loop of rsbwt_set_extensions, two calls per step and direction"""
    ss, gs = _open(rsb, "stranded", 3)
    try:
        for ctx, m, both, mx in ((12, 1, False, 24), (20, 2, True, 24)):
            sds = U.seeds(ctx)
            got = ss.unitigs(sds, ctx, m, mx, both)
            for d, left in enumerate((False, True)):
                cur = {q: s for q, s in enumerate(sds) if W.context(s, ctx, left) is not None}
                done = {q: ("", U.INVALID, U.ZERO8) for q in range(len(sds)) if q not in cur}
                ext = {q: "" for q in cur}
                while cur:
                    qs = sorted(cur)
                    on = ss.extensions([cur[q] for q in qs], ctx, left, both).sum(axis=0)
                    tent = {}
                    for q, row in zip(qs, on):
                        live = [b for b in range(4) if row[b] >= m]
                        if len(live) != 1:
                            done[q] = (ext[q], U.BRANCH if live else U.DEAD_END, tuple(int(x) for x in row) + (0, 0, 0, 0))
                        else:
                            c = "ACGT"[live[0]]
                            tent[q] = (c, c + cur[q] if left else cur[q] + c, row)
                    ts = sorted(tent)
                    back = ss.extensions([W.context(tent[q][1], ctx, left) for q in ts], ctx, not left, both).sum(axis=0) if ts else []
                    nxt = {}
                    for q, ret in zip(ts, back):
                        c, t2, row = tent[q]
                        if sum(x >= m for x in ret) >= 2:
                            done[q] = (ext[q], U.JOIN, tuple(int(x) for x in row) + tuple(int(x) for x in ret))
                        else:
                            ext[q] += c
                            nxt[q] = t2
                    cur = nxt
                    for q in [q for q in cur if len(ext[q]) == mx]:
                        done[q] = (ext[q], U.LIMIT, U.ZERO8)
                        del cur[q]
                assert [done[q] for q in range(len(sds))] == [g[d] for g in got], (ctx, m, both, left)
    finally:
        _close(ss, gs)


@pytest.mark.parametrize("name,ctx,m,both,in_repeat", [W.IN_REPEAT[:3] + (W.IN_REPEAT[4], True), ("plain", 12, 1, False, False)],
                         ids=["in-repeat", "plain"])
def test_gpu_unitigs_max_steps_and_the_limit(rsb, oracle, name, ctx, m, both, in_repeat):
    """max_steps 1, 2, 63 and 64.  Inside the tandem repeat a walk goes round until max_steps; a unitig does not: every
    turn of the repeat enters a node that the turn before enters too (JOIN), and on this fixture no side seeded there
    passes 9 steps at any setting.  So LIMIT is reached inside the repeat at max_steps 1 and 2 (the setting at which the
    walks go round), and at every max_steps, 63 and 64 among them, by the windows of the plain setting"""
    ss, gs = _open(rsb, name, 5)
    try:
        sds = U.seeds(ctx)
        us = _ref(oracle, name, ctx, m, both)
        for mx in (1, 2, 63, 64):
            u1 = _ref(oracle, name, ctx, m, both, max_steps=mx)
            _check(ss, u1, sds, ctx, m, both, ("max_steps", mx), max_steps=mx)
            assert all(a[d].stop == U.LIMIT and len(a[d].ext) == mx for a, full in zip(u1, us) for d in (0, 1) if len(full[d].ext) >= mx)
            at = W.seeds_inside_the_repeat() if in_repeat else range(W.N_PLAIN)
            if not in_repeat or mx <= 2:
                assert all(sum(u1[q][d].stop == U.LIMIT for q in at) >= 2 for d in (0, 1)), (name, mx)
    finally:
        _close(ss, gs)


def test_gpu_unitigs_the_seed_with_one_invalid_side(rsb, oracle):
    ss, gs = _open(rsb, "plain", 2)
    try:
        for ctx in W.CTXS:
            sds = U.seeds(ctx)
            us = _ref(oracle, "plain", ctx, 1, False)
            one = [q for q, (r, l) in enumerate(us) if (r.stop == U.INVALID) != (l.stop == U.INVALID)]
            assert one == [len(sds) - 1]
            # alone (its sibling item idles from the start), beside walking seeds, and first of a second workgroup
            for batch in ([one[0]], [0, one[0], 1], [0, 1, 2, 3, one[0]]):
                _check(ss, [us[q] for q in batch], [sds[q] for q in batch], ctx, 1, False, ("one side", batch))
            right, left = ss.unitigs([sds[one[0]]], ctx)[0]
            assert left == ("", U.INVALID, U.ZERO8) and right[1] != U.INVALID and right == (us[one[0]][0].ext, us[one[0]][0].stop, us[one[0]][0].last)
            assert rsb.unitig_sequence(sds[one[0]], right[0], left[0]) == sds[one[0]] + right[0]
    finally:
        _close(ss, gs)


def test_gpu_unitigs_device_resident_form(rsb, oracle):
    """rsbwt_set_unitigs_dev: every output inside 0xAB guard bytes, every byte of every output written, with and without
    the optional ones"""
    import torch
    L = rsb.lib()
    ss, gs = _open(rsb, "plain", 3)
    p = lambda t, byte=0: C.c_void_p(t.data_ptr() + byte) if t is not None else None  # noqa: E731
    PAD = 256
    try:
        for ctx, m, both, mx in ((12, 1, False, W.MAX_STEPS), (20, 2, True, 7)):
            sds = U.seeds(ctx)
            us = _ref(oracle, "plain", ctx, m, both, max_steps=mx)
            want = _arrays(us, mx)
            text, off = ss._var_text(sds)
            Q, N = len(sds), int(off[-1])
            d_text = torch.from_numpy(text).cuda()
            d_off = torch.from_numpy(off.view(np.int64)).cuda()
            for optional in (True, False):
                sizes = [2 * Q * mx, 2 * Q * 4, 2 * Q, 2 * Q * mx * 4, 2 * Q * 64]
                bufs = [torch.full((PAD + n + PAD,), 0xAB, dtype=torch.uint8, device="cuda") for n in sizes]
                ptrs = [p(b, PAD) for b in bufs]
                if not optional:
                    ptrs[3] = ptrs[4] = None
                rc = L.rsbwt_set_unitigs_dev(ss._s, p(d_text), p(d_off), Q, N, ctx, m, mx, 2 if both else 0, *ptrs, None)
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
        assert L.rsbwt_set_unitigs_dev(ss._s, p(d_text), p(d_off), 0, 0, 12, 1, 4, 0, p(buf), p(buf), p(buf), None, None, None) == 0
        torch.cuda.synchronize()
        assert (buf.cpu().numpy() == 0xAB).all()
        assert L.rsbwt_set_unitigs_dev(ss._s, p(d_text), p(d_off), 1, N, 12, 1, 4, 0, None, p(buf), p(buf), None, None, None) == -1
        assert L.rsbwt_set_unitigs_dev(ss._s, None, p(d_off), 1, N, 12, 1, 4, 0, p(buf), p(buf), p(buf), None, None, None) == -1
        assert L.rsbwt_set_unitigs_dev(ss._s, p(d_text), p(d_off), 1, N, 0, 1, 4, 0, p(buf), p(buf), p(buf), None, None, None) == -1
        assert L.rsbwt_set_unitigs_dev(ss._s, p(d_text), p(d_off), 1, N, 12, 1, 0, 0, p(buf), p(buf), p(buf), None, None, None) == -1
        assert L.rsbwt_set_unitigs_dev(ss._s, p(d_text), p(d_off), 1, N, 12, 1, 4, 1, p(buf), p(buf), p(buf), None, None, None) == -1
        assert L.rsbwt_set_unitigs_dev(ss._s, p(d_text), p(d_off), 1, N, 12, 1, 4, 4, p(buf), p(buf), p(buf), None, None, None) == -1
        assert L.rsbwt_set_unitigs_dev(ss._s, p(d_text), p(d_off), 1 << 19, N, 12, 1, 1 << 11, 0, p(buf), p(buf), p(buf), None, None, None) == -7
        torch.cuda.synchronize()
        assert (buf.cpu().numpy() == 0xAB).all()
    finally:
        _close(ss, gs)


def test_gpu_unitigs_on_two_logical_devices(rsb, oracle, monkeypatch):
    """a set split over two device groups (two logical devices on GPU 0 where the box has one), one of them with shards
    that do not sit next to each other: the groups evaluate, the host sums and decides by the shared rule -- the
    one-device answers and counters; the device-resident form refuses such a set"""
    L = rsb.lib()
    one, gs1 = _open(rsb, "stranded", 3)
    counters = {}
    try:
        for ctx, m, both in SETTINGS:
            if m != 3:
                one.unitigs(U.seeds(ctx), ctx, m, W.MAX_STEPS, both)
                counters[(ctx, m, both)] = rsb.ShardSet.unitigs_last_work()
    finally:
        _close(one, gs1)
    if L.rsbwt_device_count() < 2:
        monkeypatch.setenv("RSBWT_ENABLE_TEST_HOOKS", "1")
        monkeypatch.setenv("RSBWT_TEST_DEVICE_ALIASES", "2")
    ss, gs = _open(rsb, "stranded", 3, devices=(0, 1, 0))
    side = _side(oracle, "stranded", 3)
    try:
        assert L.rsbwt_set_devices(ss._s) == 2
        for ctx, m, both in SETTINGS:
            if m == 3:
                continue
            sds = U.seeds(ctx)
            us = _ref(oracle, "stranded", ctx, m, both)
            _check(ss, us, sds, ctx, m, both, "two devices")
            assert rsb.ShardSet.unitigs_last_work() == counters[(ctx, m, both)], (ctx, m, both)
            if m == 1 and ctx == 12 and both:
                _check_work(rsb, side, us, sds, both, 6, ("two devices", both))
        # support and last null: ext, steps and stop of the call that has them
        pv = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
        text, off = ss._var_text(U.seeds(12))
        Q, mx = len(U.seeds(12)), W.MAX_STEPS
        full = [np.full((Q, 2, mx), 77, np.uint8), np.full((Q, 2), 77, np.uint32), np.full((Q, 2), 77, np.uint8)]
        bare = [a.copy() for a in full]
        sup, last = np.zeros((Q, 2, mx), np.uint32), np.zeros((Q, 2, 8), np.uint64)
        assert L.rsbwt_set_unitigs(ss._s, pv(text), pv(off), Q, 12, 1, mx, 0, *[pv(a) for a in full], pv(sup), pv(last)) == 0
        assert L.rsbwt_set_unitigs(ss._s, pv(text), pv(off), Q, 12, 1, mx, 0, *[pv(a) for a in bare], None, None) == 0
        assert all((a == b).all() for a, b in zip(full, bare)) and full[1].any() and sup.any() and last.any()
        assert L.rsbwt_set_unitigs_dev(ss._s, None, None, 0, 0, 12, 1, 4, 0, None, None, None, None, None, None) == -1
        assert b"devices" in L.rsbwt_last_error()
    finally:
        _close(ss, gs)


def test_gpu_unitigs_arguments(rsb, oracle):
    """the errors of the header, each leaving 77-filled buffers untouched; Q = 0; NULL support and last; min_count 0 = 1;
    off[0] != 0"""
    L = rsb.lib()
    ss, gs = _open(rsb, "plain", 2)
    pv = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    try:
        ctx, mx = 12, 16
        sds = U.seeds(ctx)
        us = _ref(oracle, "plain", ctx, 1, False, max_steps=mx)
        e_ext, e_steps, e_stop, e_sup, e_last = _arrays(us, mx)
        text, off = ss._var_text(sds)
        Q = len(sds)
        ext, steps, stop = np.full((Q, 2, mx), 77, np.uint8), np.full((Q, 2), 77, np.uint32), np.full((Q, 2), 77, np.uint8)
        sup, last = np.full((Q, 2, mx), 77, np.uint32), np.full((Q, 2, 8), 77, np.uint64)

        def call(Q=Q, ctx=ctx, m=1, mx=mx, flags=0, text=text, off=off, ext=ext, steps=steps, stop=stop, sup=sup, last=last):
            return L.rsbwt_set_unitigs(ss._s, pv(text) if text is not None else None, pv(off) if off is not None else None, Q, ctx, m, mx, flags,
                                       pv(ext) if ext is not None else None, pv(steps) if steps is not None else None,
                                       pv(stop) if stop is not None else None, pv(sup) if sup is not None else None,
                                       pv(last) if last is not None else None)
        # ---- refused, nothing written
        assert call(ctx=0) == -1 and call(ctx=256) == -1 and call(mx=0) == -1 and call(mx=65536) == -1
        assert call(flags=1) == -1 and call(flags=3) == -1 and call(flags=4) == -1 and call(flags=0x80000002) == -1
        assert call(Q=1 << 19, mx=1 << 11) == -7  # 2 x Q x max_steps = 2^31 (refused before anything is read)
        assert call(Q=1 << 19, mx=1 << 11, text=None, off=None) == -7
        assert call(ext=None) == -1 and call(steps=None) == -1 and call(stop=None) == -1 and call(off=None) == -1 and call(text=None) == -1
        back = off.copy()
        back[3] = back[2] - 1
        assert call(off=back) == -1
        # ---- Q = 0: fine, nothing touched
        assert call(Q=0) == 0 and call(Q=0, text=None, off=None, ext=None, steps=None, stop=None) == 0
        for a in (ext, steps, stop, sup, last):
            assert (a == 77).all()
        assert rsb.ShardSet.unitigs_last_work() == dict.fromkeys(WORK, 0)
        assert ss.unitigs([], ctx) == []
        assert ss.unitigs(["", "ACGT"], ctx) == [(("", U.INVALID, U.ZERO8),) * 2] * 2  # seeds of no symbols at all
        # ---- every output, then NULL support / last
        assert call() == 0
        assert (ext == e_ext).all() and (steps == e_steps).all() and (stop == e_stop).all() and (sup == e_sup).all() and (last == e_last).all()
        assert stop.min() >= 1
        ext[:], steps[:], stop[:] = 77, 77, 77
        assert call(sup=None, last=None) == 0
        assert (ext == e_ext).all() and (steps == e_steps).all() and (stop == e_stop).all()
        # ---- min_count = 0 is 1; off[0] != 0: the text pointer is not at the batch's start
        ext[:] = 77
        assert call(m=0) == 0 and (ext == e_ext).all()
        lead = np.frombuffer(b"GATTACA", np.uint8)
        ext[:] = 77
        assert call(text=np.concatenate([lead, text]), off=off + np.uint64(lead.size)) == 0 and (ext == e_ext).all() and (last == e_last).all()
    finally:
        _close(ss, gs)


def test_gpu_unitigs_from_eight_threads(rsb, oracle):
    """the calls are re-entrant: eight threads at once get the single-threaded answers and their own work counters"""
    ss, gs = _open(rsb, "plain", 3)
    try:
        settings = [(12, 1, False), (12, 2, True), (20, 1, False), (20, 3, True)]
        want, wk0 = {}, {}
        for st in settings:
            ctx, m, both = st
            want[st] = _want(_ref(oracle, "plain", *st))
            assert ss.unitigs(U.seeds(ctx), ctx, m, W.MAX_STEPS, both, supports=True) == want[st]
            wk0[st] = rsb.ShardSet.unitigs_last_work()
        errs = []

        def work(i):
            try:
                for r in range(5):
                    st = settings[(i + r) % len(settings)]
                    ctx, m, both = st
                    assert ss.unitigs(U.seeds(ctx), ctx, m, W.MAX_STEPS, both, supports=True) == want[st], (i, r)
                    assert rsb.ShardSet.unitigs_last_work() == wk0[st], (i, r)
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


def test_gpu_walk_is_unchanged_by_a_unitig_call(rsb, oracle):
    """rsbwt_set_walk on the same set before and after a unitig call: the same answers and the same work counters; and it
    goes on refusing flags = 4"""
    ss, gs = _open(rsb, "stranded", 5)
    try:
        for ctx, m, left, both in ((12, 1, False, False), (20, 2, True, True)):
            sds = U.seeds(ctx)
            before = ss.walk(sds, ctx, m, W.MAX_STEPS, left, both, supports=True)
            wk = rsb.ShardSet.walk_last_work()
            ss.unitigs(sds, ctx, m, W.MAX_STEPS, both)
            assert rsb.ShardSet.walk_last_work() == wk  # (the unitig call keeps counters of its own)
            assert ss.walk(sds, ctx, m, W.MAX_STEPS, left, both, supports=True) == before
            assert rsb.ShardSet.walk_last_work() == wk
        text, off = ss._var_text(["ACGTACGTACGTACGT"])
        z = np.full(8, 77, np.uint64)
        pz = C.c_void_p(z.ctypes.data)
        assert rsb.lib().rsbwt_set_walk(ss._s, C.c_void_p(text.ctypes.data), C.c_void_p(off.ctypes.data), 1, 12, 1, 4, 4, pz, pz, pz, None, None) == -1
        assert (z == 77).all()
    finally:
        _close(ss, gs)
