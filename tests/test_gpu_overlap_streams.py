"""Overlaps on the GPU beyond the gt fixture (-m gpu): rsbwt_set_overlaps / _dev / rsbwt_set_overlap_records /
rsbwt_set_overlap_reads / rsbwt_overlaps (csrc/overlaps.hip, csrc/sets.hip, csrc/capi.hip) held bit-exactly to
tests/overlap_reference.py's restatement over the oracle on tests/stream_reference.py's inputs: run streams in the shapes
that broke other kernels on every line layout with and without a k-mer table, batches of several hundred queries (more
than three workgroups of overlap_kernel lanes per shard: every lane of a wave, every wave's stage buffer, a second and a
third blockIdx.x), sets of two unlike shards, and the reads call on read sets with duplicate and nested reads.
tests/test_stream_reference.py shows on the CPU what these inputs reach."""
import ctypes as C

import numpy as np
import pytest

import overlap_reference as O
import stream_reference as R
import test_kmer_fixtures as F

pytestmark = pytest.mark.gpu

# window spans: the builder's choice, no continuation, spill chunks, far lines + chunks, far chains, chains of several lines
SPANS = {"auto": 0, "control": 40, "chunk": 128, "far": 300, "chain": 600, "deep": 2944}
GROUPED = ("short", "dollars", "nodollar")  # the streams whose tabled cases take the grouped table format
WIDE = ("uniform", "short", "dollars") + R.FIXTURES
REC = ("query", "shard", "start", "length", "ordinal", "count", "lower", "upper")


def _open(rsb, src, span=0, ktab=6, grouped=False):
    return rsb.GpuBWT(runs=src.runs, num_strings=src.num_strings, ktab_depth=ktab, window_span=span, for_reads=True, ktab_grouped=grouped)


def _check(ss, rsb, srcs, key, qs, mo, xo, where, T=None):
    """every output of the host calls against the restatement; the work counters of the counting call.  T: the table depth
    of a set of one shard (0 = none), where the LF steps are the reference walk's less what the table starts saved"""
    ecnt, eod, (erecs, efirst), _ = R.overlap_expected(srcs, key, qs, mo, xo)
    cnt, od = ss.overlaps(qs, mo, xo, ordinals=True)
    wk = rsb.ShardSet.overlap_last_work()
    assert cnt.dtype == np.uint64 and cnt.shape == ecnt.shape
    bad = np.argwhere(cnt != ecnt)
    assert bad.size == 0, (where, mo, xo, len(bad), bad[:5], cnt[tuple(bad[0])], ecnt[tuple(bad[0])])
    bad = np.argwhere(od != eod)
    assert bad.size == 0, (where, mo, xo, len(bad), bad[:5], od[tuple(bad[0])], eod[tuple(bad[0])])
    assert (ss.overlaps(qs, mo, xo) == ecnt).all(), where  # NULL ordinal
    assert wk["items"] == len(qs) * len(srcs) and wk["entries"] == len(erecs), (where, wk, len(erecs))
    assert wk["passes"] <= 2 * (wk["lf_steps"] + wk["items"]), (where, wk)
    assert wk["dollar_only_passes"] <= 2 * wk["items"], (where, wk)
    if T is not None:
        # a table start saves exactly the T - 1 steps of a T-mer that is there; nothing looks past the step that emptied an
        # item and nothing stops early
        ref = sum(R.overlap_lf_steps(srcs, key, qs, xo))
        assert wk["lf_steps"] == ref - (max(T, 1) - 1) * wk["table_starts"], (where, mo, xo, wk, ref)
        if T == 0:
            assert wk["table_starts"] == 0, (where, wk)
    recs, first = ss.overlap_records(qs, mo, xo, raw=True)
    got = [tuple(int(r[f]) for f in REC) for r in recs]
    assert got == erecs, (where, mo, xo, len(got), len(erecs))
    assert [int(x) for x in first] == efirst and (recs["reserved"] == 0).all()
    assert rsb.ShardSet.overlap_last_work() == wk
    return wk


def _check_reads(ss, srcs, key, qs, mo, xo, max_reads, stride, where):
    """first, the (overlap, ordinal, read) triples in order, and matches[] against reads_of with the read text from the read
    lists alone"""
    exp = R.overlap_expected(srcs, key, qs, mo, xo)[3]
    efirst, eout, ematches = O.reads_of(exp, qs, [s.plain for s in srcs], max_reads)
    first, strs, ov, od, m = ss.overlap_reads(qs, mo, xo, max_reads, read_stride=stride, raw=True)
    assert [int(x) for x in first] == efirst, (where, mo, xo, max_reads)
    assert [int(x) for x in m.ravel()] == ematches, (where, mo, xo, max_reads)
    assert [(int(a), int(b), s) for a, b, s in zip(ov, od, strs)] == eout, (where, mo, xo, max_reads)
    return ematches, eout


def _assert_layout(rsb, g, src, kind):
    """the builder's own statistics are the host layout's, and of the kind the case is named for where the stream has
    run bytes enough per window (tests/test_stream_reference.py shows the same on the CPU)"""
    span = SPANS[kind]
    if span:
        st = F.selftest(rsb, src.runs, span, True)
        assert (g.window_span(), g.far_lines(), g.spilled_symbols()) == (span, st[2], st[5]), (src.name, kind)
    if src.name in R.SPILLING and kind == "chunk":
        assert g.spilled_symbols() > 0, (src.name, kind)
    if (src.name in R.SPILLING and kind in ("far", "chain", "deep")) or (src.name in R.FAR_AT_DEEP and kind == "deep"):
        assert g.far_lines() > 0, (src.name, kind)


@pytest.mark.parametrize("ktab", [6, None])
@pytest.mark.parametrize("kind", list(SPANS))
@pytest.mark.parametrize("name", R.STREAMS)
def test_gpu_overlaps_on_every_stream_and_layout(rsb, oracle, name, kind, ktab):
    """the small batch, all of overlap_reference.PARAMS: count, ordinal and the records with first[]"""
    src = R.source(name, oracle, rsb)
    qs = R.queries(src, "small")
    grouped = ktab is not None and name in GROUPED
    g = _open(rsb, src, SPANS[kind], ktab, grouped)
    ss = rsb.ShardSet([g])
    try:
        _assert_layout(rsb, g, src, kind)
        if ktab is not None:
            assert g.ktab_info()[0] == (1 if grouped else 0)
        for mo, xo in O.PARAMS:
            _check(ss, rsb, [src], "small", qs, mo, xo, (name, kind, ktab), T=g.ktab_depth() if ktab is not None else 0)
    finally:
        ss.close()
        g.close()


@pytest.mark.parametrize("span", [0, 300])
@pytest.mark.parametrize("name", WIDE)
def test_gpu_overlaps_wide_batch(rsb, oracle, name, span):
    """more than three workgroups of 256 lanes, behind a 6-mer table: all five parameter pairs, the records in order; and
    the same call with off[0] != 0: the text pointer is not at the batch's start"""
    src = R.source(name, oracle, rsb)
    qs = R.queries(src, "wide")
    L = rsb.lib()
    pv = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    g = _open(rsb, src, span, 6)
    ss = rsb.ShardSet([g])
    try:
        N = sum(len(w) for w in qs)
        assert len(qs) > 3 * 256 - 64 and N >= 20000 and g.ktab_depth() == 6
        for mo, xo in O.PARAMS:
            wk = _check(ss, rsb, [src], "wide", qs, mo, xo, (name, span), T=6)
            assert wk["items"] == len(qs), wk
        text, off = ss._var_text(qs)
        lead = np.frombuffer(b"GATTACA", np.uint8)
        text2, off2 = np.concatenate([lead, text]), off + np.uint64(lead.size)
        for mo, xo in ((1, 0), (10, 30)):
            ecnt, eod, _, _ = R.overlap_expected([src], "wide", qs, mo, xo)
            cnt, od = np.zeros((1, N), np.uint64), np.zeros((1, N), np.uint64)
            assert L.rsbwt_set_overlaps(ss._s, pv(text2), pv(off2), len(qs), mo, xo, pv(cnt), pv(od)) == 0
            assert (cnt == ecnt).all() and (od == eod).all(), (name, span, mo, xo)
            cnt[:] = 0
            assert L.rsbwt_overlaps(g.handle, pv(text2), pv(off2), len(qs), mo, xo, pv(cnt), None) == 0
            assert (cnt == ecnt).all(), (name, span, mo, xo)
    finally:
        ss.close()
        g.close()


# (first shard: span, table), (second shard: span, table); the queries are the first shard's small batch
PAIRS = [("uniform", 128, 6, "repeat", 0, None), ("ragged", 300, 6, "short", 40, None), ("repeat", 600, None, "single", 0, 6),
         ("dollars", 2944, None, "ragged", 128, 6), ("ragged", 0, 6, "nodollar", 300, None), ("all31", 40, 6, "dollar-ends", 600, None),
         ("repeat", 300, None, "dollar-ends", 0, 6), ("stripes", 300, None, "nodollar", 128, 6)]


@pytest.mark.parametrize("a,span_a,ktab_a,b,span_b,ktab_b", PAIRS, ids=[f"{p[0]}+{p[3]}" for p in PAIRS])
def test_gpu_overlaps_sets_of_two_unlike_shards(rsb, oracle, a, span_a, ktab_a, b, span_b, ktab_b):
    """a run stream beside a read set's shard, different spans, one behind a table and one not: each row is that shard's
    restatement and its single-handle answer"""
    srcs = [R.source(a, oracle, rsb), R.source(b, oracle, rsb)]
    qs = R.queries(srcs[0], "small")
    key = f"small of {a}"
    gs = [_open(rsb, srcs[0], span_a, ktab_a), _open(rsb, srcs[1], span_b, ktab_b)]
    ss = rsb.ShardSet(gs)
    try:
        for mo, xo in O.PARAMS:
            _check(ss, rsb, srcs, key, qs, mo, xo, (a, b))
            ecnt, eod, _, _ = R.overlap_expected(srcs, key, qs, mo, xo)
            for p, g in enumerate(gs):
                cnt, od = g.overlaps(qs, mo, xo, ordinals=True)
                assert (cnt == ecnt[p]).all() and (od == eod[p]).all(), (a, b, p, mo, xo)
    finally:
        ss.close()
        for g in gs:
            g.close()


@pytest.mark.parametrize("span", [0, 300])
@pytest.mark.parametrize("name", R.FIXTURES)
def test_gpu_overlap_reads_on_duplicate_and_nested_reads(rsb, oracle, name, span):
    """each read once, at its longest overlap: exact duplicates (repeat) and reads that are prefixes of other reads
    (ragged), without a limit and with one that cuts some (query, shard) pairs and leaves others"""
    src = R.source(name, oracle, rsb)
    qs = R.queries(src, "small")
    cap, stride = R.MAX_READS[name], R.READ_STRIDE[name]
    g = _open(rsb, src, span, 6)
    ss = rsb.ShardSet([g])
    try:
        cut = kept = 0
        for mo, xo in R.READ_PARAMS:
            whole = _check_reads(ss, [src], "small", qs, mo, xo, 0, stride, (name, span))
            capped = _check_reads(ss, [src], "small", qs, mo, xo, cap, stride, (name, span))
            assert capped[0] == whole[0] and len(capped[1]) < len(whole[1])
            if mo > 1:
                cut += sum(m > cap for m in whole[0])
                kept += sum(0 < m <= cap for m in whole[0])
        assert cut > 0 and kept > 0, (name, cut, kept)
        # nested form
        nested, m = ss.overlap_reads(qs, 6, 0, cap, read_stride=stride)
        exp = R.overlap_expected([src], "small", qs, 6, 0)[3]
        efirst, eout, ematches = O.reads_of(exp, qs, [src.plain], cap)
        assert [x for per in nested for cell in per for x in cell] == eout and [int(x) for x in m.ravel()] == ematches
    finally:
        ss.close()
        g.close()


@pytest.mark.parametrize("name", R.FIXTURES)
def test_gpu_overlap_reads_wide_batch(rsb, oracle, name):
    """several hundred (query, shard) pairs in one reads call, under the limit"""
    src = R.source(name, oracle, rsb)
    qs = R.queries(src, "wide")
    g = _open(rsb, src, 300, 6)
    ss = rsb.ShardSet([g])
    try:
        matches, out = _check_reads(ss, [src], "wide", qs, 10, 30, R.MAX_READS[name], R.READ_STRIDE[name], (name, "wide"))
        assert sum(m > R.MAX_READS[name] for m in matches) > 20 and sum(0 < m <= R.MAX_READS[name] for m in matches) > 20 and len(out) > 100
    finally:
        ss.close()
        g.close()


def test_gpu_overlap_reads_on_a_set_of_both_read_sets(rsb, oracle):
    """two shards of reads, different spans, one table: the reads of (query, shard) come from that shard"""
    srcs = [R.source("repeat", oracle, rsb), R.source("ragged", oracle, rsb)]
    qs = R.queries(srcs[1], "small")
    gs = [_open(rsb, srcs[0], 600, None), _open(rsb, srcs[1], 128, 6)]
    ss = rsb.ShardSet(gs)
    try:
        for mo, xo in R.READ_PARAMS:
            for cap in (0, 2):
                _check_reads(ss, srcs, "small of ragged", qs, mo, xo, cap, 640, "both")
    finally:
        ss.close()
        for g in gs:
            g.close()


def test_gpu_overlaps_wide_batch_device_resident_form(rsb, oracle):
    """rsbwt_set_overlaps_dev on the wide batch of the '$'-dense stream: d_pairs inside a larger 0xAB buffer: every entry
    is defined, nothing outside the array changes"""
    import torch
    L = rsb.lib()
    src = R.source("dollars", oracle, rsb)
    qs = R.queries(src, "wide")
    g = _open(rsb, src, 300, 6)
    ss = rsb.ShardSet([g])
    p = lambda t, byte=0: C.c_void_p(t.data_ptr() + byte)  # noqa: E731
    try:
        text, off = ss._var_text(qs)
        Q, N, PAD = len(qs), int(off[-1]), 256
        d_text = torch.from_numpy(text).cuda()
        d_off = torch.from_numpy(off.view(np.int64)).cuda()
        for mo, xo in ((1, 0), (12, 0)):
            ecnt, eod, _, _ = R.overlap_expected([src], "wide", qs, mo, xo)
            d_pairs = torch.full((PAD + N * 16 + PAD,), 0xAB, dtype=torch.uint8, device="cuda")
            rc = L.rsbwt_set_overlaps_dev(ss._s, p(d_text), p(d_off), Q, N, mo, xo, p(d_pairs, PAD), None)
            assert rc == 0, L.rsbwt_last_error()
            torch.cuda.synchronize()
            hp = d_pairs.cpu().numpy()
            assert (hp[:PAD] == 0xAB).all() and (hp[PAD + N * 16:] == 0xAB).all()
            pr = hp[PAD:PAD + N * 16].view(np.uint64).reshape(N, 2)
            assert (pr[:, 0] == eod[0]).all() and (pr[:, 1] == ecnt[0]).all(), (mo, xo)
    finally:
        ss.close()
        g.close()
