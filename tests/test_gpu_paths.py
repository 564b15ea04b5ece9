"""Paths on the GPU (-m gpu): rsbwt_set_paths / _dev (csrc/paths.hip's paths_kernel, csrc/set_graph.hip) held bit-exactly to
tests/paths_reference.py, the definition stated over the oracle: ext, steps, stop, min_support, npaths and state of every
seed, and all eight work counters.  The fixture is the walk tests': the gt read set as it is and with every other read
reverse-complemented, dealt to 1, 2, 3, 5 and 9 shards (workgroups of 1, 2 and 4 waves; one round, rounds, a last round
that is not full); tests/test_paths_reference.py shows on the CPU that the seeds reach every seed state and every stop,
backtracks past the last fork and bubbles that close at the target, and holds the statement to a computation without a BWT."""
import ctypes as C
import threading

import numpy as np
import pytest

import gt_reference as G
import paths_reference as P
import walk_reference as W

pytestmark = pytest.mark.gpu

SPANS = {"control": 40, "chunk": 128, "chain": 600}  # the builder's own spans of the line-layout tests
SETTINGS = [(ctx, m, left, both) for ctx in W.CTXS for m in W.MIN_COUNTS for left in (False, True) for both in (False, True)]
VARIANTS = ((P.WIDE, True), (P.WIDE, False), (P.TIGHT, True))  # (limits, with targets)
WORK = ("seeds", "appended", "searches", "lf_steps", "passes", "table_starts", "evals", "paths")

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


def _ref(oracle, name, ctx, m, left, both, limits=P.WIDE, targets=True):
    """the reference searches: over the two shards as they are -- the support is a sum over the shards, so they are those
    of every dealing (tests/test_paths_reference.py)"""
    return P.searches(_side(oracle, name, 2), (name, "oracle", targets), W.seeds(ctx), P.targets(ctx, left) if targets else None, ctx, m, limits,
                      left, both)


def _want(ss):
    return [(s.state, list(s.paths)) for s in ss]


def _arrays(ss, limits):
    """reference searches as rsbwt_set_paths lays them out"""
    mx, mp = limits[0], limits[1]
    Q = len(ss)
    ext, steps, stop, sup = np.zeros((Q, mp, mx), np.uint8), np.zeros((Q, mp), np.uint32), np.zeros((Q, mp), np.uint8), np.zeros((Q, mp), np.uint32)
    for q, s in enumerate(ss):
        for j, (e, why, least) in enumerate(s.paths):
            ext[q, j, :len(e)] = np.frombuffer(e.encode(), np.uint8)
            steps[q, j], stop[q, j], sup[q, j] = len(e), why, least
    return ext, steps, stop, sup, np.array([len(s.paths) for s in ss], np.uint32), np.array([s.state for s in ss], np.uint8)


def _check(ss, ref, sds, tgs, ctx, m, left, both, limits, where):
    got = ss.paths(sds, ctx, m, limits[0], limits[1], limits[2], left, both, tgs)
    want = _want(ref)
    bad = [q for q in range(len(sds)) if got[q] != want[q]]
    assert not bad, (where, ctx, m, left, both, limits, bad[:5], got[bad[0]], want[bad[0]])


def _check_work(rsb, side, ref, sds, left, both, T, where):
    wk = rsb.ShardSet.paths_last_work()
    ex = P.expected_work(side, ref, left, both)
    print(where, wk, ex)
    assert tuple(wk) == WORK
    assert wk["seeds"] == len(sds) and wk["appended"] == ex["appended"], (where, wk, ex)
    assert wk["evals"] == ex["evals"] and wk["paths"] == ex["paths"], (where, wk, ex)
    assert wk["searches"] == ex["searches"] == ex["evals"] * side.S * 4 * (2 if both else 1), (where, wk, ex)
    # a table start saves exactly the T - 1 steps of a T-mer that is there; nothing looks past the step that emptied a
    # search and nothing stops early
    assert wk["lf_steps"] == ex["lf_steps"] - (max(T, 1) - 1) * wk["table_starts"], (where, wk, ex)
    assert wk["passes"] <= 2 * wk["lf_steps"] + wk["searches"], (where, wk)
    assert (wk["table_starts"] > 0) == (T > 0), (where, wk)
    return wk


def _all_settings(rsb, oracle, ss, side, name, T, where, skip_m3=False, work_at=lambda ctx, m, left, both: m == 1):
    for ctx, m, left, both in SETTINGS:
        if skip_m3 and m == 3:
            continue
        sds = W.seeds(ctx)
        for limits, targets in VARIANTS:
            ref = _ref(oracle, name, ctx, m, left, both, limits, targets)
            _check(ss, ref, sds, P.targets(ctx, left) if targets else None, ctx, m, left, both, limits, where + (targets,))
            if work_at(ctx, m, left, both):
                _check_work(rsb, side, ref, sds, left, both, T, where + (ctx, left, both, limits, targets))


@pytest.mark.parametrize("ktab", [6, None])
@pytest.mark.parametrize("name", ["plain", "stranded"])
def test_gpu_paths_are_the_reference(rsb, oracle, name, ktab):
    """the two shards as they are at the builder's own span: every setting, with and without targets, the wide limits and
    the tight ones (MORE and BUDGET); the work counters where min_count is 1"""
    ss, gs = _open(rsb, name, 2, ktab=ktab)
    try:
        _all_settings(rsb, oracle, ss, _side(oracle, name, 2), name, ktab or 0, (name, ktab))
    finally:
        _close(ss, gs)


@pytest.mark.parametrize("ktab", [6, None])
@pytest.mark.parametrize("kind", list(SPANS))
def test_gpu_paths_on_every_line_layout(rsb, oracle, kind, ktab):
    """small spans, spill chunks and far chains (positions past a line's own pieces go through the scalar reader)"""
    ss, gs = _open(rsb, "plain", 2, span=SPANS[kind], ktab=ktab)
    try:
        assert all(g.window_span() == SPANS[kind] for g in gs)
        _all_settings(rsb, oracle, ss, _side(oracle, "plain", 2), "plain", ktab or 0, (kind, ktab), skip_m3=True,
                      work_at=lambda ctx, m, left, both: m == 1 and ctx == 12)
    finally:
        _close(ss, gs)


@pytest.mark.parametrize("name,ktab", [("plain", 6), ("stranded", None)])
@pytest.mark.parametrize("S", [1, 3, 5, 9])
def test_gpu_paths_on_dealt_sets(rsb, oracle, S, name, ktab):
    """workgroups of 1, 2, 4 and 4 waves: one shard per wave, more (rounds), a last round that is not full (3, 5, 9): the
    paths of every dealing are the same; Q = 1, 7, 8 (exactly one workgroup), 9 (a second workgroup with one seed) and all
    58 (the last workgroup has two)"""
    ss, gs = _open(rsb, name, S, ktab=ktab)
    side = _side(oracle, name, S)
    try:
        _all_settings(rsb, oracle, ss, side, name, ktab or 0, (name, S), work_at=lambda ctx, m, left, both: m == 1 and ctx == 12)
        for ctx, m, left, both in ((12, 1, False, False), (20, 2, True, True)):
            sds, tgs = W.seeds(ctx), P.targets(ctx, left)
            ref = _ref(oracle, name, ctx, m, left, both)
            for Q in (1, 7, 8, 9):
                _check(ss, ref[:Q], sds[:Q], tgs[:Q], ctx, m, left, both, P.WIDE, (name, S, Q))
                if m == 1:
                    _check_work(rsb, side, ref[:Q], sds[:Q], left, both, ktab or 0, (name, S, Q))
    finally:
        _close(ss, gs)


def test_gpu_paths_agree_with_extensions_composed_on_the_host(rsb, oracle):
    """the parent's way to the same answers: a depth-first host loop over rsbwt_set_extensions, one call per round for the
    seeds still searching"""
    ss, gs = _open(rsb, "stranded", 3)
    try:
        for ctx, m, left, both, limits in ((12, 1, False, False, P.WIDE), (20, 2, True, True, P.TIGHT)):
            sds, tgs = W.seeds(ctx), P.targets(ctx, left)
            got = ss.paths(sds, ctx, m, limits[0], limits[1], limits[2], left, both, tgs)
            runs = [P.search_by_rounds(s, t, ctx, m, limits[0], limits[1], limits[2], left) for s, t in zip(sds, tgs)]
            done, asks = {}, {}
            for q, g in enumerate(runs):
                try:
                    asks[q] = next(g)
                except StopIteration as end:
                    done[q] = end.value
            while asks:
                qs = sorted(asks)
                tot = ss.extensions([asks[q] for q in qs], ctx, left, both).sum(axis=0)
                for q, row in zip(qs, tot):
                    try:
                        asks[q] = runs[q].send(tuple(int(x) for x in row))
                    except StopIteration as end:
                        done[q] = end.value
                        del asks[q]
            assert [(done[q].state, list(done[q].paths)) for q in range(len(sds))] == got, (ctx, m, left, both)
    finally:
        _close(ss, gs)


def test_gpu_paths_limits_at_their_edges(rsb, oracle):
    """max_steps 1 and 2, max_paths 1, max_evals 1 and 2, and a ring that wraps: ctx 12 with paths past 12 symbols on both
    sides of a backtrack (the wide limits have them; shown here by counting)"""
    ss, gs = _open(rsb, "plain", 5)
    side = _side(oracle, "plain", 2)
    try:
        for ctx, m, left, both in ((12, 1, False, False), (12, 2, True, True), (20, 1, True, False)):
            sds, tgs = W.seeds(ctx), P.targets(ctx, left)
            for limits in ((1, 8, 256), (2, 8, 256), (64, 1, 256), (64, 8, 1), (64, 8, 2), (3, 256, 7)):
                ref = P.searches(side, ("plain", "oracle", True), sds, tgs, ctx, m, limits, left, both)
                _check(ss, ref, sds, tgs, ctx, m, left, both, limits, ("edges",))
        ref = _ref(oracle, "plain", 12, 1, False, False)
        assert sum(len(s.paths) >= 2 and len(s.paths[1][0]) > 12 and any(d > 12 for d, _ in s.backtracks) for s in ref) >= 2
    finally:
        _close(ss, gs)


def test_gpu_paths_device_resident_form(rsb, oracle):
    """rsbwt_set_paths_dev: every output inside 0xAB guard bytes, every byte of every output written, with and without
    targets and the optional min_support"""
    import torch
    L = rsb.lib()
    ss, gs = _open(rsb, "plain", 3)
    p = lambda t, byte=0: C.c_void_p(t.data_ptr() + byte) if t is not None else None  # noqa: E731
    PAD = 256
    try:
        for ctx, m, left, both, limits, targets in ((12, 1, False, False, P.WIDE, True), (20, 2, True, True, P.TIGHT, True),
                                                    (12, 2, True, False, (7, 5, 30), False)):
            sds = W.seeds(ctx)
            tgs = P.targets(ctx, left) if targets else None
            ref = P.searches(_side(oracle, "plain", 2), ("plain", "oracle", targets), sds, tgs, ctx, m, limits, left, both)
            want = _arrays(ref, limits)
            text, off = ss._var_text(sds)
            Q, N = len(sds), int(off[-1])
            d_text = torch.from_numpy(text).cuda()
            d_off = torch.from_numpy(off.view(np.int64)).cuda()
            d_tt = d_toff = None
            TN = 0
            if targets:
                ttext, toff = ss._var_text(tgs)
                TN = int(toff[-1])
                d_tt, d_toff = torch.from_numpy(ttext).cuda(), torch.from_numpy(toff.view(np.int64)).cuda()
            mx, mp, me = limits
            for optional in (True, False):
                sizes = [Q * mp * mx, Q * mp * 4, Q * mp, Q * mp * 4, Q * 4, Q]
                bufs = [torch.full((PAD + n + PAD,), 0xAB, dtype=torch.uint8, device="cuda") for n in sizes]
                ptrs = [p(b, PAD) for b in bufs]
                if not optional:
                    ptrs[3] = None
                rc = L.rsbwt_set_paths_dev(ss._s, p(d_text), p(d_off), Q, N, p(d_tt), p(d_toff), TN, ctx, m, mx, mp, me,
                                           (1 if left else 0) | (2 if both else 0), *ptrs, None)
                assert rc == 0, L.rsbwt_last_error()
                torch.cuda.synchronize()
                for i, (b, n, w) in enumerate(zip(bufs, sizes, want)):
                    hb = b.cpu().numpy()
                    assert (hb[:PAD] == 0xAB).all() and (hb[PAD + n:] == 0xAB).all(), i
                    if i == 3 and not optional:
                        assert (hb == 0xAB).all(), i
                    else:
                        assert (hb[PAD:PAD + n].view(w.dtype).reshape(w.shape) == w).all(), (i, ctx, optional)
        # nothing to do, nothing touched; null arguments; bad arguments
        buf = torch.full((4096,), 0xAB, dtype=torch.uint8, device="cuda")
        b = p(buf)

        def dev(Q=1, N=N, tt=None, toff=None, TN=0, ctx=12, mx=4, mp=2, me=16, flags=0, text=p(d_text), off=p(d_off), ext=b, steps=b, stop=b,
                npaths=b, state=b):
            return L.rsbwt_set_paths_dev(ss._s, text, off, Q, N, tt, toff, TN, ctx, 1, mx, mp, me, flags, ext, steps, stop, None, npaths, state, None)
        assert dev(Q=0, N=0) == 0
        assert dev(ext=None) == -1 and dev(steps=None) == -1 and dev(stop=None) == -1 and dev(npaths=None) == -1 and dev(state=None) == -1
        assert dev(text=None) == -1 and dev(off=None) == -1 and dev(tt=b) == -1 and dev(toff=b) == -1
        assert dev(ctx=0) == -1 and dev(ctx=256) == -1 and dev(mx=0) == -1 and dev(mx=65536) == -1 and dev(mp=0) == -1 and dev(mp=257) == -1
        assert dev(me=0) == -1 and dev(me=(1 << 20) + 1) == -1 and dev(flags=4) == -1
        assert dev(Q=1 << 15, mx=1 << 11, mp=32) == -7
        torch.cuda.synchronize()
        assert (buf.cpu().numpy() == 0xAB).all()
    finally:
        _close(ss, gs)


def test_gpu_paths_on_two_logical_devices(rsb, oracle, monkeypatch):
    """a set split over two device groups (two logical devices on GPU 0 where the box has one), one of them with shards
    that do not sit next to each other: the groups evaluate, the host sums and decides by the shared header -- the
    one-device answers and counters; the device-resident form refuses such a set"""
    L = rsb.lib()
    settings = [(ctx, m, left, both) for ctx, m, left, both in SETTINGS if m != 3 and left == both]
    one, gs1 = _open(rsb, "stranded", 3)
    counters = {}
    try:
        for ctx, m, left, both in settings:
            for limits, targets in VARIANTS:
                one.paths(W.seeds(ctx), ctx, m, limits[0], limits[1], limits[2], left, both, P.targets(ctx, left) if targets else None)
                counters[(ctx, m, left, both, limits, targets)] = rsb.ShardSet.paths_last_work()
    finally:
        _close(one, gs1)
    if L.rsbwt_device_count() < 2:
        monkeypatch.setenv("RSBWT_ENABLE_TEST_HOOKS", "1")
        monkeypatch.setenv("RSBWT_TEST_DEVICE_ALIASES", "2")
    ss, gs = _open(rsb, "stranded", 3, devices=(0, 1, 0))
    side = _side(oracle, "stranded", 3)
    try:
        assert L.rsbwt_set_devices(ss._s) == 2
        for ctx, m, left, both in settings:
            sds = W.seeds(ctx)
            for limits, targets in VARIANTS:
                ref = _ref(oracle, "stranded", ctx, m, left, both, limits, targets)
                _check(ss, ref, sds, P.targets(ctx, left) if targets else None, ctx, m, left, both, limits, ("two devices",))
                assert rsb.ShardSet.paths_last_work() == counters[(ctx, m, left, both, limits, targets)], (ctx, m, left, both, limits, targets)
                if m == 1 and ctx == 12:
                    _check_work(rsb, side, ref, sds, left, both, 6, ("two devices", left, both))
        # min_support null: ext, steps, stop, npaths and state of the call that has it
        pv = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
        text, off = ss._var_text(W.seeds(12))
        Q, (mx, mp, me) = len(W.seeds(12)), P.WIDE
        full = [np.full((Q, mp, mx), 77, np.uint8), np.full((Q, mp), 77, np.uint32), np.full((Q, mp), 77, np.uint8), np.zeros((Q, mp), np.uint32),
                np.full(Q, 77, np.uint32), np.full(Q, 77, np.uint8)]
        bare = [a.copy() for a in full]
        assert L.rsbwt_set_paths(ss._s, pv(text), pv(off), Q, None, None, 12, 1, mx, mp, me, 0, *[pv(a) for a in full]) == 0
        assert L.rsbwt_set_paths(ss._s, pv(text), pv(off), Q, None, None, 12, 1, mx, mp, me, 0, *[pv(a) if i != 3 else None for i, a in enumerate(bare)]) == 0
        assert all((a == b).all() for i, (a, b) in enumerate(zip(full, bare)) if i != 3) and full[3].any() and (full[4] >= 2).any()
        assert L.rsbwt_set_paths_dev(ss._s, None, None, 0, 0, None, None, 0, 12, 1, 4, 2, 16, 0, None, None, None, None, None, None, None) == -1
        assert b"devices" in L.rsbwt_last_error()
    finally:
        _close(ss, gs)


def test_gpu_paths_arguments(rsb, oracle):
    """the errors of the header, each leaving 77-filled buffers untouched; Q = 0; NULL min_support; min_count 0 = 1;
    off[0] != 0 and toff[0] != 0; a target longer than ctx"""
    L = rsb.lib()
    ss, gs = _open(rsb, "plain", 2)
    pv = lambda x: x.ctypes.data_as(C.c_void_p) if x is not None else None  # noqa: E731
    try:
        ctx, limits = 12, (16, 4, 48)
        mx, mp, me = limits
        sds, tgs = W.seeds(ctx), P.targets(ctx, False)
        ref = P.searches(_side(oracle, "plain", 2), ("plain", "oracle", True), sds, tgs, ctx, 1, limits, False, False)
        e_ext, e_steps, e_stop, e_sup, e_np, e_state = _arrays(ref, limits)
        text, off = ss._var_text(sds)
        ttext, toff = ss._var_text(tgs)
        Q = len(sds)
        ext, steps, stop = np.full((Q, mp, mx), 77, np.uint8), np.full((Q, mp), 77, np.uint32), np.full((Q, mp), 77, np.uint8)
        sup, npaths, state = np.full((Q, mp), 77, np.uint32), np.full(Q, 77, np.uint32), np.full(Q, 77, np.uint8)
        outs = (ext, steps, stop, sup, npaths, state)

        def call(Q=Q, ctx=ctx, m=1, mx=mx, mp=mp, me=me, flags=0, text=text, off=off, ttext=ttext, toff=toff, ext=ext, steps=steps, stop=stop,
                 sup=sup, npaths=npaths, state=state):
            return L.rsbwt_set_paths(ss._s, pv(text), pv(off), Q, pv(ttext), pv(toff), ctx, m, mx, mp, me, flags, pv(ext), pv(steps), pv(stop),
                                     pv(sup), pv(npaths), pv(state))
        # ---- refused, nothing written
        assert call(ctx=0) == -1 and call(ctx=256) == -1 and call(mx=0) == -1 and call(mx=65536) == -1
        assert call(mp=0) == -1 and call(mp=257) == -1 and call(me=0) == -1 and call(me=(1 << 20) + 1) == -1
        assert call(flags=4) == -1 and call(flags=0x80000002) == -1
        assert call(Q=1 << 15, mx=1 << 11, mp=32) == -7  # Q x max_paths x max_steps = 2^31 (refused before anything is read)
        assert call(Q=1 << 15, mx=1 << 11, mp=32, text=None, off=None, ttext=None, toff=None) == -7
        assert call(ext=None) == -1 and call(steps=None) == -1 and call(stop=None) == -1 and call(npaths=None) == -1 and call(state=None) == -1
        assert call(off=None) == -1 and call(text=None) == -1 and call(ttext=None) == -1 and call(toff=None) == -1
        back = off.copy()
        back[3] = back[2] - 1
        assert call(off=back) == -1
        tback = toff.copy()
        tback[2] = tback[1] - 1
        assert call(toff=tback) == -1
        long_t, long_off = ss._var_text([sds[0][:ctx + 1]] + [""] * (Q - 1))
        assert call(ttext=long_t, toff=long_off) == -1 and b"target 0" in L.rsbwt_last_error()
        for a in outs:
            assert (a == 77).all()
        # ---- Q = 0: fine, nothing touched
        assert call(Q=0) == 0 and call(Q=0, text=None, off=None, ttext=None, toff=None, ext=None, steps=None, stop=None, npaths=None, state=None) == 0
        for a in outs:
            assert (a == 77).all()
        assert rsb.ShardSet.paths_last_work() == dict.fromkeys(WORK, 0)
        assert ss.paths([], ctx) == []
        assert ss.paths(["", "ACGT"], ctx) == [(P.INVALID, [])] * 2  # seeds of no symbols at all
        # ---- every output, then NULL min_support
        assert call() == 0
        for got, want in zip(outs, (e_ext, e_steps, e_stop, e_sup, e_np, e_state)):
            assert (got == want).all()
        assert state.min() >= 1
        for a in outs:
            a[:] = 77
        assert call(sup=None) == 0
        assert (ext == e_ext).all() and (steps == e_steps).all() and (stop == e_stop).all() and (npaths == e_np).all() and (state == e_state).all()
        assert (sup == 77).all()
        # ---- a target of exactly ctx symbols is taken; min_count = 0 is 1; off[0] / toff[0] != 0
        full_t, full_off = ss._var_text([sds[1][:ctx]] + [""] * (Q - 1))
        assert call(ttext=full_t, toff=full_off) == 0
        ext[:] = 77
        assert call(m=0) == 0 and (ext == e_ext).all()
        lead = np.frombuffer(b"GATTACA", np.uint8)
        ext[:], stop[:] = 77, 77
        assert call(text=np.concatenate([lead, text]), off=off + np.uint64(lead.size), ttext=np.concatenate([lead, ttext]),
                    toff=toff + np.uint64(lead.size)) == 0
        assert (ext == e_ext).all() and (stop == e_stop).all()
    finally:
        _close(ss, gs)


def test_gpu_paths_from_two_threads(rsb, oracle):
    """the calls are re-entrant: two threads calling at once get the single-threaded answers and their own work counters"""
    ss, gs = _open(rsb, "plain", 3)
    try:
        settings = [(12, 1, False, False, P.WIDE), (20, 2, True, True, P.TIGHT)]
        want, wk0 = {}, {}

        def run(st):
            ctx, m, left, both, limits = st
            return ss.paths(W.seeds(ctx), ctx, m, limits[0], limits[1], limits[2], left, both, P.targets(ctx, left))
        for st in settings:
            want[st] = _want(_ref(oracle, "plain", *st))
            assert run(st) == want[st]
            wk0[st] = rsb.ShardSet.paths_last_work()
        assert wk0[settings[0]] != wk0[settings[1]]
        errs = []

        def work(i):
            try:
                for r in range(6):
                    st = settings[(i + r) % 2]
                    assert run(st) == want[st], (i, r)
                    assert rsb.ShardSet.paths_last_work() == wk0[st], (i, r)
            except Exception as e:  # noqa: BLE001
                errs.append(repr(e))
        th = [threading.Thread(target=work, args=(i,)) for i in range(2)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert not errs, errs[:3]
    finally:
        _close(ss, gs)


def test_gpu_walk_is_unchanged_by_a_paths_call(rsb, oracle):
    """rsbwt_set_walk on the same set before and after a paths call: the same answers and the same work counters (walk.hip's
    search moved into a header both files include)"""
    ss, gs = _open(rsb, "stranded", 5)
    try:
        for ctx, m, left, both in ((12, 1, False, False), (20, 2, True, True)):
            sds = W.seeds(ctx)
            ws = W.walks(_side(oracle, "stranded", 2), ("stranded", "oracle", "paths"), sds, ctx, m, W.MAX_STEPS, left, both)
            before = ss.walk(sds, ctx, m, W.MAX_STEPS, left, both, supports=True)
            assert before == [(w.ext, w.stop, w.last, w.support) for w in ws]
            wk = rsb.ShardSet.walk_last_work()
            ss.paths(sds, ctx, m, 64, 8, 256, left, both)
            assert rsb.ShardSet.walk_last_work() == wk  # (the paths call keeps counters of its own)
            assert ss.walk(sds, ctx, m, W.MAX_STEPS, left, both, supports=True) == before
            assert rsb.ShardSet.walk_last_work() == wk
    finally:
        _close(ss, gs)
