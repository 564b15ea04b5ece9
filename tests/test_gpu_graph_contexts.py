"""The k-mer graph kernels at the context lengths where the search and the rings change behaviour (-m gpu):
rsbwt_set_extensions / rsbwt_extensions / rsbwt_set_walk / rsbwt_set_unitigs / rsbwt_set_paths / _dev (csrc/walk_search.h,
csrc/walk.hip, csrc/paths.hip, csrc/set_graph.hip) held bit-exactly, work counters included, to walk_reference, unitig_reference
and paths_reference over the oracle:

  * AROUND THE TABLE DEPTH.  walk_search takes a table start only when the candidate, K = ctx + 1 symbols, is no shorter
    than the table's depth T.  With K == T the table entry is the whole candidate: rows without one LF step.  With K < T
    the search starts from initInterval though a table is open.  The counter rules, in their general form:
        table_starts > 0  exactly when  T > 0 and ctx + 1 >= T
        lf_steps == (the steps without a table) - (T - 1) * table_starts
    so at K == T a candidate that is there costs no step at all (the second rule against walk_reference.search_steps).
  * THE LARGEST CONTEXT.  ctx 254 and 255 on the `ragged` read set: the ring of 256 bytes wraps at ctx, a left walk of
    more than 255 symbols crosses it more than once, paths keep a target of up to ctx ranks beside it and rebuild it after
    a backtrack; ctx 1, where the ring is one byte and the head never moves, is among the lengths below the table depth.
  * DENSE FORKS.  At ctx 1, 2 and 3 every node of the gt reads' graph has four live successors: the frame store of
    min(max_steps, max_evals) frames per seed is full, max_paths = 256 is reached, and COMPLETE before MORE decides.  A
    frame written past a seed's store lands in its neighbour's: every seed's paths are compared.

tests/test_graph_context_reference.py shows on the CPU what these inputs reach."""
import ctypes as C

import numpy as np
import pytest

import graph_context_reference as X
import paths_reference as P
import unitig_reference as U
import walk_reference as W

pytestmark = pytest.mark.gpu

DIRECTIONS = [(left, both) for left in (False, True) for both in (False, True)]


def _open(rsb, runs, reads, ktab=6, devices=None):
    gs = [rsb.GpuBWT(runs=r, num_strings=len(sh), ktab_depth=ktab, device=(devices[p] if devices else 0)) for p, (sh, r) in enumerate(zip(reads, runs))]
    return rsb.ShardSet(gs), gs


def _open_gt(rsb, name, S, ktab=6, devices=None):
    return _open(rsb, W.runs(name, S), W.dealt(name, S), ktab, devices)


def _close(ss, gs):
    ss.close()
    for g in gs:
        g.close()


def _counters(wk, n, steps, T, ctx, where):
    """the rules of the header of this file; n and steps: the candidate searches and their LF steps without a table"""
    assert wk["searches"] == n, (where, wk, n)
    assert (wk["table_starts"] > 0) == X.table_starts_expected(T, ctx), (where, wk)
    assert wk["lf_steps"] == steps - (max(T, 1) - 1) * wk["table_starts"], (where, wk, steps)
    assert wk["passes"] <= 2 * wk["lf_steps"] + wk["searches"], (where, wk)


def _check_extensions(rsb, ss, gs, side, strings, ctx, left, both, T, where, steps=W.search_steps):
    want = np.array([W.extensions(side, s, ctx, left, both) for s in strings], np.uint64).transpose(1, 0, 2)
    got = ss.extensions(strings, ctx, left, both)
    assert got.dtype == np.uint64 and got.shape == want.shape == (side.S, len(strings), 4)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (where, "extensions", len(bad), bad[:5], got[tuple(bad[0])], want[tuple(bad[0])])
    contexts = [c for c in (W.context(s, ctx, left) for s in strings) if c is not None]
    wk = rsb.ShardSet.walk_last_work()
    assert wk["seeds"] == len(strings), (where, wk)
    _counters(wk, *X.lf_steps(side, contexts, left, both, steps), T, ctx, where + ("extensions",))
    for p, g in enumerate(gs):
        assert (g.extensions(strings, ctx, left, both) == want[p]).all(), (where, "handle", p)


def _check_walk(rsb, ss, side, key, sds, ctx, m, max_steps, left, both, T, where, steps=W.search_steps, answers=None):
    ws = W.walks(answers or side, key, sds, ctx, m, max_steps, left, both)
    got = ss.walk(sds, ctx, m, max_steps, left, both, supports=True)
    want = [(w.ext, w.stop, w.last, w.support) for w in ws]
    bad = [q for q in range(len(sds)) if got[q] != want[q]]
    assert not bad, (where, "walk", bad[:5], got[bad[0]], want[bad[0]])
    wk = rsb.ShardSet.walk_last_work()
    assert wk["seeds"] == len(sds) and wk["appended"] == sum(len(w.ext) for w in ws), (where, wk)
    if m == 1:
        _counters(wk, *X.lf_steps(side, [c for w in ws for c in w.contexts], left, both, steps), T, ctx, where + ("walk",))
    return ws


def _check_unitigs(rsb, ss, side, key, sds, ctx, m, max_steps, both, T, where, steps=W.search_steps, answers=None):
    us = U.unitigs(answers or side, key, sds, ctx, m, max_steps, both)
    got = ss.unitigs(sds, ctx, m, max_steps, both, supports=True)
    want = [tuple((s.ext, s.stop, s.last, s.support) for s in pair) for pair in us]
    bad = [q for q in range(len(sds)) if got[q] != want[q]]
    assert not bad, (where, "unitigs", bad[:5], got[bad[0]], want[bad[0]])
    wk = rsb.ShardSet.unitigs_last_work()
    onward = sum(len(s.onward) for pair in us for s in pair)
    back = sum(len(s.back) for pair in us for s in pair)
    assert wk["seeds"] == len(sds) and wk["appended"] == sum(len(s.ext) for pair in us for s in pair), (where, wk)
    assert wk["onward"] == onward and wk["back"] == back, (where, wk, onward, back)
    if m == 1:
        n = total = 0
        for d, left in enumerate((False, True)):
            for strings, to_left in (([c for pair in us for c in pair[d].onward], left), ([c for pair in us for c in pair[d].back], not left)):
                a, b = X.lf_steps(side, strings, to_left, both, steps)
                n, total = n + a, total + b
        assert n == (onward + back) * side.S * 4 * (2 if both else 1)
        _counters(wk, n, total, T, ctx, where + ("unitigs",))
    return wk


def _check_paths(rsb, ss, side, key, sds, tgs, ctx, m, limits, left, both, T, where, steps=W.search_steps, answers=None, batches=()):
    """the seeds' paths at every batch size of `batches` and then of all the seeds, whose work counters are checked"""
    ref = P.searches(answers or side, key + (None if tgs is None else tuple(tgs),), sds, tgs, ctx, m, limits, left, both)
    for Q in tuple(batches) + (len(sds),):
        got = ss.paths(sds[:Q], ctx, m, limits[0], limits[1], limits[2], left, both, tgs[:Q] if tgs is not None else None)
        want = [(s.state, list(s.paths)) for s in ref[:Q]]
        bad = [q for q in range(Q) if got[q] != want[q]]
        assert not bad, (where, "paths", Q, limits, bad[:5], got[bad[0]][0], want[bad[0]][0], len(got[bad[0]][1]), len(want[bad[0]][1]))
    wk = rsb.ShardSet.paths_last_work()
    evals = sum(len(s.evaluated) for s in ref)
    appended = sum(len(s.evaluated) - sum(p[1] == P.DEAD_END for p in s.paths) + len(s.backtracks) for s in ref)
    assert wk["seeds"] == len(sds) and wk["appended"] == appended, (where, wk, appended)
    assert wk["evals"] == evals and wk["paths"] == sum(len(s.paths) for s in ref), (where, wk, evals)
    assert wk["searches"] == evals * side.S * 4 * (2 if both else 1), (where, wk, evals)
    if m == 1:
        _counters(wk, *X.lf_steps(side, [c for s in ref for c in s.evaluated], left, both, steps), T, ctx, where + ("paths",))
    return ref, wk


def _targets(ctx, left):
    """the paths tests' targets, cut to ctx symbols (below 3 the one that holds an N would be longer)"""
    return [t[:ctx] for t in P.targets(ctx, left)]


# ---- around the table depth ---------------------------------------------------------------------------------------------

TABLES = [(6, X.CTXS_AT_6), (None, X.CTXS_AT_6)] + [(T, (T - 1,)) for T in X.OTHER_DEPTHS]


@pytest.mark.parametrize("ktab,ctxs", TABLES, ids=[f"T{t}" for t, _ in TABLES])
@pytest.mark.parametrize("S", [2, 3])
@pytest.mark.parametrize("name", ["plain", "stranded"])
def test_gpu_graph_calls_around_the_table_depth(rsb, oracle, name, S, ktab, ctxs):
    """K < T, K == T and K > T behind a table of depth 6, K == T behind tables of depth 3 and 9, and the same lengths
    without a table; the answers are those of the two shards as they are, the work is this dealing's"""
    T = ktab or 0
    ss, gs = _open_gt(rsb, name, S, ktab)
    side, answers = X.gt_side(oracle, name, S), X.gt_side(oracle, name, 2)
    try:
        assert all(g.ktab_depth() == T for g in gs)
        for ctx in ctxs:
            sds = W.seeds(ctx)
            for left, both in DIRECTIONS:
                where = (name, S, T, ctx, left, both)
                for m in (1, 2):
                    ws = _check_walk(rsb, ss, side, (name, "contexts"), sds, ctx, m, W.MAX_STEPS, left, both, T, where + (m,), answers=answers)
                    if m == 1:
                        _check_extensions(rsb, ss, gs, side, sds + [w.final for w in ws], ctx, left, both, T, where)
                    if not left:
                        _check_unitigs(rsb, ss, side, (name, "contexts"), sds, ctx, m, W.MAX_STEPS, both, T, where + (m,), answers=answers)
                    for limits, tgs in ((P.WIDE, None), (P.TIGHT, None), (P.WIDE, _targets(ctx, left))):
                        _check_paths(rsb, ss, side, (name, "contexts"), sds, tgs, ctx, m, limits, left, both, T, where + (m,), answers=answers)
    finally:
        _close(ss, gs)


@pytest.mark.parametrize("ktab", [6, None])
def test_gpu_graph_calls_where_the_candidate_is_a_whole_read(rsb, oracle, ktab):
    """ctx 39 on reads of 40 symbols: only a whole read holds a candidate, and the seed of ctx symbols is one symbol short
    of it"""
    ctx, T = X.WHOLE_READ_CTX, ktab or 0
    ss, gs = _open_gt(rsb, "plain", 2, ktab)
    side = X.gt_side(oracle, "plain", 2)
    try:
        sds = W.seeds(ctx)
        for left, both in DIRECTIONS:
            where = ("plain", 2, T, ctx, left, both)
            ws = _check_walk(rsb, ss, side, ("plain", "contexts"), sds, ctx, 1, W.MAX_STEPS, left, both, T, where)
            _check_extensions(rsb, ss, gs, side, sds + [w.final for w in ws], ctx, left, both, T, where)
            if not left:
                _check_unitigs(rsb, ss, side, ("plain", "contexts"), sds, ctx, 1, W.MAX_STEPS, both, T, where)
            for tgs in (None, _targets(ctx, left)):
                _check_paths(rsb, ss, side, ("plain", "contexts"), sds, tgs, ctx, 1, P.WIDE, left, both, T, where)
    finally:
        _close(ss, gs)


# ---- the largest context ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ktab", [6, None])
@pytest.mark.parametrize("ctx", X.LONG_CTXS)
@pytest.mark.parametrize("S", [1, 2])
def test_gpu_graph_calls_at_the_largest_contexts(rsb, oracle, S, ctx, ktab):
    """candidates of 255 and 256 symbols: one shard (the ragged set as it is; a left walk of more than 255 symbols) and two
    (with the variants that make these k-mers fork: backtracks above depth 0, the ring rebuilt from seed and path); max_steps
    300; targets of ctx and of 12 symbols"""
    T = ktab or 0
    ss, gs = _open(rsb, X.long_runs(S), X.long_reads(S), ktab)
    side = X.long_side(oracle, S, rsb)
    sds = X.long_seeds()
    try:
        assert all(g.ktab_depth() == T for g in gs)
        for left, both in DIRECTIONS:
            where = ("long", S, T, ctx, left, both)
            ws = _check_walk(rsb, ss, side, ("long", S, 0), sds, ctx, 1, X.LONG_MAX_STEPS, left, both, T, where, steps=X.oracle_steps)
            _check_extensions(rsb, ss, gs, side, sds + [w.final for w in ws], ctx, left, both, T, where, steps=X.oracle_steps)
            if not left:
                _check_unitigs(rsb, ss, side, ("long", S, 0), sds, ctx, 1, X.LONG_MAX_STEPS, both, T, where, steps=X.oracle_steps)
            _check_paths(rsb, ss, side, ("long", S, 0), sds, None, ctx, 1, X.LONG_LIMITS, left, both, T, where, steps=X.oracle_steps)
            for tlen in X.long_target_lens(ctx):
                _check_paths(rsb, ss, side, ("long", S, 0, tlen), sds, X.long_targets(tlen, left), ctx, 1, X.LONG_LIMITS, left, both, T, where,
                             steps=X.oracle_steps)
    finally:
        _close(ss, gs)


# ---- dense forks ----------------------------------------------------------------------------------------------------------

BATCHES = (1, 8, 9)  # and all the seeds: one workgroup's seeds, a second workgroup with one


@pytest.mark.parametrize("S", [2, 5])
@pytest.mark.parametrize("ctx", X.DENSE_CTXS)
def test_gpu_paths_at_dense_forks(rsb, oracle, ctx, S):
    """every node forks four ways: a full frame store, 256 paths, COMPLETE at the very path that MORE would take, BUDGET one
    evaluation before the end; every seed of every batch size"""
    ss, gs = _open_gt(rsb, "plain", S)
    side, answers = X.gt_side(oracle, "plain", S), X.gt_side(oracle, "plain", 2)
    sds = W.seeds(ctx)
    try:
        for left, both in DIRECTIONS:
            for limits in X.DENSE_LIMITS:
                _check_paths(rsb, ss, side, ("plain", "dense", 0), sds, None, ctx, 1, limits, left, both, 6, ("dense", S, ctx, left, both), answers=answers,
                             batches=BATCHES)
    finally:
        _close(ss, gs)


def test_gpu_paths_device_resident_form_at_dense_forks(rsb, oracle):
    """rsbwt_set_paths_dev with every slot of every seed taken: every output inside 0xAB guard bytes, every byte of every
    output written and nothing outside"""
    import torch
    L = rsb.lib()
    ctx, (mx, mp, me) = 2, X.DENSE_FULL
    ss, gs = _open_gt(rsb, "plain", 3)
    p = lambda t, byte=0: C.c_void_p(t.data_ptr() + byte) if t is not None else None  # noqa: E731
    PAD = 256
    try:
        sds = W.seeds(ctx)
        ref = P.searches(X.gt_side(oracle, "plain", 2), ("plain", "dense", 0, None), sds, None, ctx, 1, X.DENSE_FULL, False, False)
        Q = len(sds)
        ext, steps, stop, sup = np.zeros((Q, mp, mx), np.uint8), np.zeros((Q, mp), np.uint32), np.zeros((Q, mp), np.uint8), np.zeros((Q, mp), np.uint32)
        for q, s in enumerate(ref):
            for j, (e, why, least) in enumerate(s.paths):
                ext[q, j, :len(e)] = np.frombuffer(e.encode(), np.uint8)
                steps[q, j], stop[q, j], sup[q, j] = len(e), why, least
        want = (ext, steps, stop, sup, np.array([len(s.paths) for s in ref], np.uint32), np.array([s.state for s in ref], np.uint8))
        assert (want[4][want[5] != P.INVALID] == 256).all() and (want[5] == P.COMPLETE).sum() >= 55
        text, off = ss._var_text(sds)
        N = int(off[-1])
        d_text = torch.from_numpy(text).cuda()
        d_off = torch.from_numpy(off.view(np.int64)).cuda()
        sizes = [Q * mp * mx, Q * mp * 4, Q * mp, Q * mp * 4, Q * 4, Q]
        bufs = [torch.full((PAD + n + PAD,), 0xAB, dtype=torch.uint8, device="cuda") for n in sizes]
        rc = L.rsbwt_set_paths_dev(ss._s, p(d_text), p(d_off), Q, N, None, None, 0, ctx, 1, mx, mp, me, 0, *[p(b, PAD) for b in bufs], None)
        assert rc == 0, L.rsbwt_last_error()
        torch.cuda.synchronize()
        for i, (b, n, w) in enumerate(zip(bufs, sizes, want)):
            hb = b.cpu().numpy()
            assert (hb[:PAD] == 0xAB).all() and (hb[PAD + n:] == 0xAB).all(), i
            assert (hb[PAD:PAD + n].view(w.dtype).reshape(w.shape) == w).all(), i
    finally:
        _close(ss, gs)


def test_gpu_paths_and_unitigs_on_two_logical_devices_at_these_lengths(rsb, oracle, monkeypatch):
    """the host loop of a set over two device groups (csrc/graph_steps.h under csrc/set_graph.hip) at K == T and at
    dense forks: the answers and the counters of the one-device set"""
    L = rsb.lib()
    cases = [(5, P.WIDE), (5, P.TIGHT), (2, X.DENSE_FULL)]
    side, answers = X.gt_side(oracle, "stranded", 3), X.gt_side(oracle, "stranded", 2)
    one, gs1 = _open_gt(rsb, "stranded", 3)
    counters = {}
    try:
        for ctx, limits in cases:
            for left, both in DIRECTIONS:
                where = ("one device", ctx, left, both)
                _, wk = _check_paths(rsb, one, side, ("stranded", "contexts"), W.seeds(ctx), None, ctx, 1, limits, left, both, 6, where, answers=answers)
                counters[("paths", ctx, limits, left, both)] = wk
                if not left:
                    counters[("unitigs", ctx, both)] = _check_unitigs(rsb, one, side, ("stranded", "contexts"), W.seeds(ctx), ctx, 1, W.MAX_STEPS,
                                                                      both, 6, where, answers=answers)
    finally:
        _close(one, gs1)
    if L.rsbwt_device_count() < 2:
        monkeypatch.setenv("RSBWT_ENABLE_TEST_HOOKS", "1")
        monkeypatch.setenv("RSBWT_TEST_DEVICE_ALIASES", "2")
    ss, gs = _open_gt(rsb, "stranded", 3, devices=(0, 1, 0))
    try:
        assert L.rsbwt_set_devices(ss._s) == 2
        for ctx, limits in cases:
            for left, both in DIRECTIONS:
                where = ("two devices", ctx, left, both)
                _, wk = _check_paths(rsb, ss, side, ("stranded", "contexts"), W.seeds(ctx), None, ctx, 1, limits, left, both, 6, where, answers=answers)
                assert wk == counters[("paths", ctx, limits, left, both)], (where, limits, wk)
                if not left:
                    wk = _check_unitigs(rsb, ss, side, ("stranded", "contexts"), W.seeds(ctx), ctx, 1, W.MAX_STEPS, both, 6, where, answers=answers)
                    assert wk == counters[("unitigs", ctx, both)], (where, wk)
    finally:
        _close(ss, gs)
