"""Matching statistics on the GPU beyond the gt fixture (-m gpu): rsbwt_set_match_lengths / _dev / rsbwt_set_smems /
rsbwt_match_lengths (csrc/match_stats.hip, csrc/sets.hip, csrc/capi.hip) held bit-exactly to tests/match_reference.py's
restatement over the oracle on tests/stream_reference.py's inputs: run streams in the shapes that broke other kernels
(runs of 31 with continuation bytes, runs of 1..2, '$'-dense, stripes of one symbol, the library's own generators, three
degenerate streams) on every line layout with and without a k-mer table, batches of several hundred queries (the offset
search of ms_query_of over hundreds of entries with runs of empty queries in it), and sets of two unlike shards.
tests/test_stream_reference.py shows on the CPU what these inputs reach."""
import ctypes as C

import numpy as np
import pytest

import match_reference as M
import stream_reference as R
import test_kmer_fixtures as F

pytestmark = pytest.mark.gpu

# window spans: the builder's choice, no continuation, spill chunks, far lines + chunks, far chains, chains of several lines
SPANS = {"auto": 0, "control": 40, "chunk": 128, "far": 300, "chain": 600, "deep": 2944}
GROUPED = ("short", "dollars", "nodollar")  # the streams whose tabled cases take the grouped table format
WIDE = ("uniform", "short", "dollars") + R.FIXTURES
SMEM = ("query", "shard", "start", "end", "lower", "upper")


def _open(rsb, src, span=0, ktab=6, grouped=False):
    return rsb.GpuBWT(runs=src.runs, num_strings=src.num_strings, ktab_depth=ktab, window_span=span, for_reads=True, ktab_grouped=grouped)


def _check(ss, rsb, srcs, key, qs, max_len, min_rows, where):
    """every output of both host calls against the restatement; the work counters of the lengths call"""
    eln, elo, eup, (erecs, efirst), _ = R.match_expected(srcs, key, qs, max_len, min_rows)
    ln, lo, up = ss.match_lengths(qs, max_len, min_rows, intervals=True)
    wk = rsb.ShardSet.match_last_work()
    assert ln.dtype == np.uint32 and ln.shape == eln.shape
    bad = np.argwhere(ln != eln)
    assert bad.size == 0, (where, max_len, min_rows, len(bad), bad[:5], ln[tuple(bad[0])], eln[tuple(bad[0])])
    bad = np.argwhere((lo != elo) | (up != eup))
    assert bad.size == 0, (where, max_len, min_rows, len(bad), bad[:5], lo[tuple(bad[0])], elo[tuple(bad[0])], up[tuple(bad[0])], eup[tuple(bad[0])])
    assert (ss.match_lengths(qs, max_len, min_rows) == eln).all(), where  # NULL lower / upper
    assert wk["items"] == eln.size and wk["smems"] == 0, (where, wk)
    assert wk["lf_steps"] <= wk["passes"] <= 2 * wk["lf_steps"], (where, wk)
    recs, first = ss.smems(qs, max_len, min_rows, raw=True)
    got = [tuple(int(r[f]) for f in SMEM) for r in recs]
    assert got == erecs, (where, max_len, min_rows, len(got), len(erecs))
    assert [int(x) for x in first] == efirst and (recs["reserved"] == 0).all()
    wk2 = rsb.ShardSet.match_last_work()
    assert wk2["smems"] == len(erecs) and {k: v for k, v in wk2.items() if k != "smems"} == {k: v for k, v in wk.items() if k != "smems"}
    return wk


def _assert_layout(rsb, g, src, kind):
    """the builder's own statistics are the host layout's, and of the kind the case is named for where the stream has
    run bytes enough per window (tests/test_stream_reference.py shows the same on the CPU)"""
    span = SPANS[kind]
    if span:
        st = F.selftest(rsb, src.runs, span, True)
        assert (g.window_span(), g.far_lines(), g.spilled_symbols()) == (span, st[2], st[5]), (src.name, kind)
    beyond = False  # positions past a line's own pieces: the scalar reader
    if src.name in R.SPILLING and kind == "chunk":
        assert g.spilled_symbols() > 0, (src.name, kind)
        beyond = True
    if (src.name in R.SPILLING and kind in ("far", "chain", "deep")) or (src.name in R.FAR_AT_DEEP and kind == "deep"):
        assert g.far_lines() > 0, (src.name, kind)
        beyond = True
    return beyond


@pytest.mark.parametrize("ktab", [6, None])
@pytest.mark.parametrize("kind", list(SPANS))
@pytest.mark.parametrize("name", R.STREAMS)
def test_gpu_match_on_every_stream_and_layout(rsb, oracle, name, kind, ktab):
    """the small batch, all of match_reference.PARAMS: len, lower, upper and the SMEM records with first[]"""
    src = R.source(name, oracle, rsb)
    qs = R.queries(src, "small")
    grouped = ktab is not None and name in GROUPED
    g = _open(rsb, src, SPANS[kind], ktab, grouped)
    ss = rsb.ShardSet([g])
    try:
        beyond = _assert_layout(rsb, g, src, kind)
        if ktab is not None:
            assert g.ktab_info()[0] == (1 if grouped else 0)
        for max_len, min_rows in M.PARAMS:
            wk = _check(ss, rsb, [src], "small", qs, max_len, min_rows, (name, kind, ktab))
            if ktab is None:
                assert wk["table_starts"] == 0 and wk["restarts"] == 0, wk
            if beyond:
                assert wk["passes"] > wk["lf_steps"], (name, kind, wk)
    finally:
        ss.close()
        g.close()


@pytest.mark.parametrize("span", [0, 300])
@pytest.mark.parametrize("name", WIDE)
def test_gpu_match_wide_batch(rsb, oracle, name, span):
    """several hundred queries, some 80 workgroups of positions, behind a 6-mer table; and the same call with off[0] != 0:
    the text pointer is not at the batch's start"""
    src = R.source(name, oracle, rsb)
    qs = R.queries(src, "wide")
    L = rsb.lib()
    pv = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    g = _open(rsb, src, span, 6)
    ss = rsb.ShardSet([g])
    try:
        N = sum(len(w) for w in qs)
        assert len(qs) >= 600 and N >= 20000 and g.ktab_depth() == 6
        for max_len, min_rows in M.PARAMS:
            wk = _check(ss, rsb, [src], "wide", qs, max_len, min_rows, (name, span))
            # (every 6-mer of a small stream can have fewer than 20 rows: those entries are refused, the lanes start over)
            assert wk["items"] == N and wk["table_starts"] + wk["restarts"] > 0 and (min_rows > 1 or wk["table_starts"] > 0), wk
        text, off = ss._var_text(qs)
        lead = np.frombuffer(b"GATTACA", np.uint8)
        text2, off2 = np.concatenate([lead, text]), off + np.uint64(lead.size)
        for max_len, min_rows in ((0, 1), (16, 1)):
            eln, elo, eup, _, _ = R.match_expected([src], "wide", qs, max_len, min_rows)
            ln, lo, up = np.zeros((1, N), np.uint32), np.zeros((1, N), np.uint64), np.zeros((1, N), np.uint64)
            assert L.rsbwt_set_match_lengths(ss._s, pv(text2), pv(off2), len(qs), max_len, min_rows, pv(ln), pv(lo), pv(up)) == 0
            assert (ln == eln).all() and (lo == elo).all() and (up == eup).all(), (name, span, max_len)
            ln[:] = 0
            assert L.rsbwt_match_lengths(g.handle, pv(text2), pv(off2), len(qs), max_len, min_rows, pv(ln), None, None) == 0
            assert (ln == eln).all(), (name, span, max_len)
    finally:
        ss.close()
        g.close()


# (first shard: span, table), (second shard: span, table); the queries are the first shard's small batch
PAIRS = [("uniform", 128, 6, "repeat", 0, None), ("ragged", 300, 6, "short", 40, None), ("repeat", 600, None, "single", 0, 6),
         ("dollars", 2944, None, "ragged", 128, 6), ("ragged", 0, 6, "nodollar", 300, None), ("all31", 40, 6, "dollar-ends", 600, None),
         ("repeat", 300, None, "dollar-ends", 0, 6), ("stripes", 300, None, "nodollar", 128, 6)]


@pytest.mark.parametrize("a,span_a,ktab_a,b,span_b,ktab_b", PAIRS, ids=[f"{p[0]}+{p[3]}" for p in PAIRS])
def test_gpu_match_sets_of_two_unlike_shards(rsb, oracle, a, span_a, ktab_a, b, span_b, ktab_b):
    """a run stream beside a read set's shard, different spans, one behind a table and one not: each row is that shard's
    restatement and its single-handle answer"""
    srcs = [R.source(a, oracle, rsb), R.source(b, oracle, rsb)]
    qs = R.queries(srcs[0], "small")
    key = f"small of {a}"
    gs = [_open(rsb, srcs[0], span_a, ktab_a), _open(rsb, srcs[1], span_b, ktab_b)]
    ss = rsb.ShardSet(gs)
    try:
        for max_len, min_rows in M.PARAMS:
            _check(ss, rsb, srcs, key, qs, max_len, min_rows, (a, b))
            eln, elo, eup, _, _ = R.match_expected(srcs, key, qs, max_len, min_rows)
            for p, g in enumerate(gs):
                ln, lo, up = g.match_lengths(qs, max_len, min_rows, intervals=True)
                assert (ln == eln[p]).all() and (lo == elo[p]).all() and (up == eup[p]).all(), (a, b, p, max_len, min_rows)
    finally:
        ss.close()
        for g in gs:
            g.close()


def test_gpu_match_wide_batch_device_resident_form(rsb, oracle):
    """rsbwt_set_match_lengths_dev on the wide batch of the runs-of-1..2 stream: d_len and d_pairs inside larger 0xAB
    buffers, nothing outside them changes"""
    import torch
    L = rsb.lib()
    src = R.source("short", oracle, rsb)
    qs = R.queries(src, "wide")
    g = _open(rsb, src, 300, 6)
    ss = rsb.ShardSet([g])
    p = lambda t, byte=0: C.c_void_p(t.data_ptr() + byte)  # noqa: E731
    try:
        text, off = ss._var_text(qs)
        Q, N, PAD = len(qs), int(off[-1]), 256
        d_text = torch.from_numpy(text).cuda()
        d_off = torch.from_numpy(off.view(np.int64)).cuda()
        for max_len, min_rows in ((0, 1), (0, 20)):
            eln, elo, eup, _, _ = R.match_expected([src], "wide", qs, max_len, min_rows)
            d_len = torch.full((PAD + N * 4 + PAD,), 0xAB, dtype=torch.uint8, device="cuda")
            d_pairs = torch.full((PAD + N * 16 + PAD,), 0xAB, dtype=torch.uint8, device="cuda")
            rc = L.rsbwt_set_match_lengths_dev(ss._s, p(d_text), p(d_off), Q, N, max_len, min_rows, p(d_len, PAD), p(d_pairs, PAD), None)
            assert rc == 0, L.rsbwt_last_error()
            torch.cuda.synchronize()
            hl, hp = d_len.cpu().numpy(), d_pairs.cpu().numpy()
            assert (hl[:PAD] == 0xAB).all() and (hl[PAD + N * 4:] == 0xAB).all()
            assert (hp[:PAD] == 0xAB).all() and (hp[PAD + N * 16:] == 0xAB).all()
            assert (hl[PAD:PAD + N * 4].view(np.uint32) == eln[0]).all(), (max_len, min_rows)
            pr = hp[PAD:PAD + N * 16].view(np.uint64).reshape(N, 2)
            assert (pr[:, 0] == elo[0]).all() and (pr[:, 1] == eup[0]).all(), (max_len, min_rows)
    finally:
        ss.close()
        g.close()
