"""Whole-read matches by backward search from the terminator rows on the GPU (-m gpu): rsbwt_read_copies, its _dev and set
forms, and rsbwt_query_exactmatch switched to it (rsbwt_exactmatch_by_search), held to the compiled reference's golden
booleans, to the read lists of the seeded fixtures (tests/test_read_copies.py pins the expected values to the lists
themselves), to the oracle composition of the definition on run streams that are no BWT of anything, and to the
extraction path it replaces -- on every line layout of tests/test_kmer_fixtures.py, and through the service loop."""
import collections
import ctypes as C
import json
import os
import random
import re
import subprocess
import time

import numpy as np
import pytest

import test_kmer_fixtures as F
import test_read_copies as RC
from test_gpu_sets import two_devices  # noqa: F401  (the fixture)
from kmer_reference import _expected

pytestmark = pytest.mark.gpu

W_RANKED, W_CONT, W_SECOND = 13, 14, 15  # counting-mode words of the '$' count (csrc/read_lookup.hip)


def _by_length(qs):
    by = {}
    for i, w in enumerate(qs):
        by.setdefault(len(w), []).append(i)
    return by


def _fixed(rsb, g, qs):
    """rsbwt_read_copies, one call per distinct length"""
    cp, en = np.zeros(len(qs), np.uint64), np.zeros(len(qs), np.uint64)
    for ln, idx in _by_length(qs).items():
        c, e = rsb.read_copies(g, [qs[i] for i in idx])
        cp[idx], en[idx] = c, e
    return cp, en


def _dev(rsb, g, qs, counters=None):
    """rsbwt_read_copies_dev on torch buffers, one call per distinct length (lengths 1 .. 65535)"""
    import torch
    L = rsb.lib()
    p = lambda t: C.c_void_p(t.data_ptr())
    dev = torch.device("cuda", 0)
    cp, en = np.zeros(len(qs), np.uint64), np.zeros(len(qs), np.uint64)
    words = (C.c_uint64 * 16)()
    for ln, idx in _by_length(qs).items():
        if ln == 0:
            continue
        m = len(idx)
        km = np.frombuffer("".join(qs[i] for i in idx).encode(), np.uint8).reshape(m, ln).copy()
        d_km = torch.from_numpy(km).to(dev)
        d_pk = torch.empty((m, (ln + 31) // 32), dtype=torch.int64, device=dev)
        d_ok = torch.empty(m, dtype=torch.uint8, device=dev)
        d_cp = torch.full((m,), -1, dtype=torch.int64, device=dev)
        d_en = torch.full((m,), -1, dtype=torch.int64, device=dev)
        assert L.rsbwt_pack_kmers_dev(p(d_km), m, ln, ln, p(d_pk), p(d_ok), 0, None) == 0
        assert L.rsbwt_read_copies_dev(g.handle, p(d_pk), p(d_ok), m, ln, p(d_cp), p(d_en), None) == 0
        torch.cuda.synchronize()
        cp[idx], en[idx] = d_cp.cpu().numpy().view(np.uint64), d_en.cpu().numpy().view(np.uint64)
        if counters is not None:
            assert L.rsbwt_last_search_counters(g.handle, words) == 0
            for i in (W_RANKED, W_CONT, W_SECOND):
                counters[i] = counters.get(i, 0) + int(words[i])
    return cp, en


def _check_fixture(rsb, oracle, name, span, room, ktab, kind=None):
    """every distinct read and the non-read sample (and, on the layouts of the matrix, every proper suffix of every read)
    through the fixed-k call, the _dev call and the set's _var call, against the read lists; the '$' count's counters of
    the _dev calls against what the layout and the oracle's intervals say they must be (tests/test_read_copies.py)"""
    fx = F.fixture(name)
    reads, others = RC.queries(name)
    main = reads + others
    qs = main + (RC.all_suffixes(name) if kind else [])
    gs = [rsb.GpuBWT(runs=runs, num_strings=len(sh), ktab_depth=ktab, window_span=span, for_reads=room) for sh, runs in zip(fx.shards, fx.runs())]
    ss = rsb.ShardSet(gs)
    L = rsb.lib()
    try:
        cp_v, en_v = ss.read_copies_var(qs)  # mixed lengths, every shard, one call
        total_conts = 0
        for p, (g, sh) in enumerate(zip(gs, fx.shards)):
            want_c, want_e = RC.from_reads(sh, qs)
            want_c, want_e = np.array(want_c, np.uint64), np.array(want_e, np.uint64)
            cnt = collections.Counter(sh)
            assert all(int(want_c[i]) == cnt[w] for i, w in enumerate(reads))
            counters = {}
            assert L.rsbwt_set_counting(g.handle, 1) == 0
            dev_main = _dev(rsb, g, main, counters)
            assert L.rsbwt_set_counting(g.handle, 0) == 0
            got = {"fixed": _fixed(rsb, g, qs), "var": (cp_v[p], en_v[p])}
            for how, (c, e) in got.items():
                bad = np.nonzero((c != want_c) | (e != want_e))[0]
                assert bad.size == 0, (name, span, room, ktab, p, how, qs[bad[0]][:40], int(c[bad[0]]), int(want_c[bad[0]]), int(e[bad[0]]), int(want_e[bad[0]]))
            assert np.array_equal(dev_main[0], want_c[:len(main)]) and np.array_equal(dev_main[1], want_e[:len(main)]), (name, span, p, "dev")
            assert int((want_e[:len(main)] > 0).sum()) > len(reads)
            assert not L.rsbwt_exactmatch_is_by_search(g.handle) and g.exactmatch_by_search is False
            # one result ranked per non-empty answer (empty ones fetch nothing), and exactly the continuations and second
            # lines the layout holds for these intervals
            S = g.window_span()
            runs = fx.runs()[p]
            st = F.selftest(rsb, runs, S, room)
            assert (g.far_lines(), g.spilled_symbols()) == (st[2], st[5]), (name, p, S, st)
            tails = RC.spilled_tails(rsb, runs, S, room) if st[5] else {}
            want = RC.expected_counters(oracle.from_runs(runs, len(sh)), tails, S, main)
            assert (counters[W_RANKED], counters[W_CONT], counters[W_SECOND]) == want, (name, kind, S, p)
            assert want[0] == int((want_e[:len(main)] > 0).sum())
            total_conts += want[1]
        if kind in ("chunk", "chunk+", "far", "chain", "deep"):
            # (fails, not skips.  RC.NONE_POSSIBLE is the one layout where NO string can reach a continuation: shown on the
            # CPU over every read and every proper suffix by tests/test_read_copies.py::test_ranked_positions_take_continuations,
            # which also shows the span added for that fixture, RC.EXTRA_LAYOUTS, does reach them)
            assert (total_conts > 0) == ((name, span, room) != RC.NONE_POSSIBLE), (name, kind, span, "no ranked position took a continuation")
        if kind == "control":
            assert total_conts == 0
    finally:
        ss.close()
        for g in gs:
            g.close()


# ---- 1. the compiled reference's booleans ----------------------------------------------------------------------------

def test_gpu_golden_booleans(rsb, fixture_bwt, golden_dir):
    gq = np.load(os.path.join(golden_dir, "query_v1.npz"))
    path, _ = fixture_bwt
    total = 0
    with rsb.GpuBWT(path) as g:
        for key in sorted(k for k in gq.files if k.startswith("em_w")):
            ws = gq[key]
            want = gq["em_ans" + key[4:]].astype(bool)  # the compiled reference's query_exactmatch
            copies, ending = rsb.read_copies(g, ws)
            assert np.array_equal(copies > 0, want), key
            assert (ending >= copies).all()
            g.exactmatch_by_search = True
            assert g.exactmatch_by_search is True
            assert np.array_equal(rsb.query_exactmatch_batch(g, ws).astype(bool), want), key
            g.exactmatch_by_search = False
            assert np.array_equal(rsb.query_exactmatch_batch(g, ws).astype(bool), want), key
            total += len(ws)
    assert total == 900


# ---- 2. / 3. the read lists, on every layout ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["pop", "repeat", "ragged"])
def test_gpu_read_lists(rsb, oracle, name):
    """copies == Counter[w] and ending == reads with that suffix for every distinct read, copies == Counter.get(w, 0) for
    the non-read sample -- fixed-k call, _dev call, the set's _var call -- on the builder's own span"""
    _check_fixture(rsb, oracle, name, 0, False, 6)


_LAYOUTS = F.LAYOUTS + RC.EXTRA_LAYOUTS


@pytest.mark.parametrize("lay", _LAYOUTS, ids=[F.layout_id(x) for x in _LAYOUTS])
def test_gpu_read_lists_on_every_layout(rsb, oracle, lay):
    """the same on span / control / chunk / far / chain / deep layouts, with and without a k-mer table, plain and
    RSBWT_OPEN_READS, and the span this module adds for `ragged`; the counting-mode counters are held to the exact number of
    continuations the layout holds for the queries' end positions, which on the kinds that have continuations is not zero"""
    name, kind, span, room, ktab = lay
    _check_fixture(rsb, oracle, name, span, room, ktab, kind if span else "auto")


# ---- 4. run streams that are BWTs of nothing ---------------------------------------------------------------------------

@pytest.mark.parametrize("with_dollar,span", [(True, 0), (True, 1400), (False, 0)])
def test_gpu_synthetic_run_streams(rsb, oracle, with_dollar, span):
    R = 150000
    runs = np.empty(R, np.uint8)
    assert rsb.lib().rsbwt_synth_runs_host(runs.ctypes.data, R, 4242) == 0
    if not with_dollar:
        runs = runs[(runs >> 5) != 0].copy()
    oix = oracle.from_runs(runs)
    rng = random.Random(99)
    # (half of them short: on a stream that is no BWT the interval of w$ dies within half a dozen steps)
    qs = ["".join(rng.choice("ACGT") for _ in range(rng.randrange(1, 71) if i % 2 else rng.randrange(1, 9))) for i in range(10000)]
    want = [RC.definition(oix, w)[:2] for w in qs]
    with rsb.GpuBWT(runs=runs, ktab_depth=None, window_span=span) as g:
        if span:
            assert g.spilled_symbols() > 0  # (a span that spills: positions past their line's own pieces)
        ss = rsb.ShardSet([g])
        cp, en = ss.read_copies_var(qs)
        ss.close()
        cf, ef = _fixed(rsb, g, qs[:2000])
    assert [(int(a), int(b)) for a, b in zip(cp[0], en[0])] == want
    assert [(int(a), int(b)) for a, b in zip(cf, ef)] == want[:2000]
    if with_dollar:
        assert oix.pc("A") > 0 and sum(1 for c, e in want if e) > 2000 and sum(1 for c, e in want if c) > 100
    else:
        assert oix.pc("A") == 0 and not any(c or e for c, e in want)


def test_gpu_hand_made_index(rsb):
    """three reads, two of them equal, spelled out.  (Row 0 itself: after a step lower = C[b] + Occ >= C['A'] >= 1 on any index
    with terminators, and an index without them is answered from the start record -- so no search leaves lower = 0; the
    kernel's Occ(., -1) = 0 rule is held to the oracle on pairs given by hand, below)"""
    from kmer_reference import _bwt_runs
    reads = ["ACGTACGGT", "ACGTACGGT", "TTGAC"]
    with rsb.GpuBWT(runs=_bwt_runs(reads), num_strings=3, ktab_depth=None) as g:
        c, e = rsb.read_copies(g, ["ACGTACGGT"])
        assert (int(c[0]), int(e[0])) == (2, 2)
        c, e = rsb.read_copies(g, ["TTGAC", "GGTAC", "CGGTN"])
        assert [int(x) for x in c] == [1, 0, 0] and [int(x) for x in e] == [1, 0, 0]
        c, e = rsb.read_copies(g, ["GGT", "GAC"])
        assert [int(x) for x in c] == [0, 0] and [int(x) for x in e] == [2, 1]


def test_gpu_dollar_count_on_intervals_given_by_hand(rsb, oracle, monkeypatch):
    """The '$' count itself (rsbwt_debug_dollar_count) on intervals no search from the terminator rows leaves: lower = 0
    (Occ(., -1) = 0), intervals that span windows and groups, single rows, the last row, and pairs that are no interval
    (lower > upper, upper >= n) -- against the oracle's occ, on a span that spills and on the builder's own."""
    monkeypatch.setenv("RSBWT_ENABLE_TEST_HOOKS", "1")
    L = rsb.lib()
    R = 150000
    runs = np.empty(R, np.uint8)
    assert L.rsbwt_synth_runs_host(runs.ctypes.data, R, 77) == 0
    oix = oracle.from_runs(runs)
    n = oix.bwlen()
    rng = np.random.default_rng(3)
    lo = rng.integers(0, n, 6000).astype(np.uint64)
    up = np.minimum(lo + rng.integers(0, 5000, 6000).astype(np.uint64) * (rng.integers(0, 3, 6000) > 0).astype(np.uint64), np.uint64(n - 1))
    lo[:400] = 0                                   # reaching row 0
    up[:4] = [0, 1, n - 1, 17]
    lo[400:420], up[400:420] = up[400:420] + np.uint64(1), lo[400:420]   # lower > upper
    up[420:440] = np.uint64(n) + rng.integers(0, 50, 20).astype(np.uint64)  # upper >= n
    up[440] = np.uint64(2**64 - 1)                 # the wrapped (0, 2^64 - 1) of query.cpp
    lo[440] = 0
    pairs = np.ascontiguousarray(np.stack([lo, up], axis=1))
    want_c, want_e = [], []
    for a, b in zip(lo.tolist(), up.tolist()):
        if a <= b < n:
            want_c.append(oix.occ("$", b) - (oix.occ("$", a - 1) if a else 0))
            want_e.append(b - a + 1)
        else:
            want_c.append(0)
            want_e.append(0)
    assert sum(1 for a, c in zip(lo.tolist(), want_c) if a == 0 and c) > 100
    for span in (0, 1400):
        with rsb.GpuBWT(runs=runs, ktab_depth=None, window_span=span) as g:
            cp, en = np.full(len(lo), 7, np.uint64), np.full(len(lo), 7, np.uint64)
            assert L.rsbwt_debug_dollar_count(g.handle, pairs.ctypes.data, len(lo), cp.ctypes.data, en.ctypes.data) == 0, L.rsbwt_last_error()
            assert cp.tolist() == want_c and en.tolist() == want_e, span
            assert L.rsbwt_debug_dollar_count(g.handle, pairs.ctypes.data, len(lo), cp.ctypes.data, None) == 0 and cp.tolist() == want_c
    monkeypatch.delenv("RSBWT_ENABLE_TEST_HOOKS")
    with rsb.GpuBWT(runs=runs[:1000].copy(), ktab_depth=None) as g:
        assert L.rsbwt_debug_dollar_count(g.handle, pairs.ctypes.data, 4, cp.ctypes.data, None) == -1  # a test hook: refused unless asked for


def test_gpu_argument_errors_on_a_real_handle(rsb):
    """stride < k and an empty index are RSBWT_EINVAL, k = 0 and k > 65535 give 0 / 0 -- as rsbwt_find_intervals treats them"""
    from kmer_reference import _bwt_runs
    L = rsb.lib()
    EINVAL = -1
    km = np.frombuffer(b"ACGTACGGTTTGAC", np.uint8).copy()
    out = np.full(4, 9, np.uint64)
    with rsb.GpuBWT(runs=_bwt_runs(["ACGTACGGT", "TTGAC"]), num_strings=2, ktab_depth=None) as g:
        assert L.rsbwt_read_copies(g.handle, km.ctypes.data, 2, 5, 4, out.ctypes.data, None) == EINVAL and b"stride" in L.rsbwt_last_error()
        assert L.rsbwt_find_intervals(g.handle, km.ctypes.data, 2, 5, 4, out.ctypes.data, out.ctypes.data) == EINVAL
        assert L.rsbwt_read_copies(g.handle, None, 2, 5, 5, out.ctypes.data, None) == EINVAL
        assert L.rsbwt_read_copies(g.handle, km.ctypes.data, 2, 5, 5, None, None) == EINVAL
        assert L.rsbwt_read_copies(g.handle, None, 0, 5, 5, None, None) == 0  # nothing asked
        assert L.rsbwt_read_copies(g.handle, km.ctypes.data, 2, 0, 5, out.ctypes.data, out[2:].ctypes.data) == 0 and out.tolist() == [0, 0, 0, 0]
        assert L.rsbwt_read_copies_dev(g.handle, None, km.ctypes.data, 2, 5, out.ctypes.data, None, None) == EINVAL
        ss = rsb.ShardSet([g])
        off = np.array([0, 9, 14], np.uint64)
        assert L.rsbwt_set_read_copies_var(ss._s, km.ctypes.data, None, 2, out.ctypes.data, None) == EINVAL
        assert L.rsbwt_set_read_copies_var(ss._s, km.ctypes.data, off.ctypes.data, 2, None, None) == EINVAL
        bad = np.array([0, 9, 5], np.uint64)  # a query that ends before it starts
        assert L.rsbwt_set_read_copies_var(ss._s, km.ctypes.data, bad.ctypes.data, 2, out.ctypes.data, None) == EINVAL
        assert L.rsbwt_set_read_copies_var(ss._s, km.ctypes.data, off.ctypes.data, 2, out.ctypes.data, out[2:].ctypes.data) == 0
        assert out.tolist() == [1, 1, 1, 1]
        ss.close()
    # an index of no symbols (one run unit of length 0), where the library opens one: every form refuses it
    try:
        g0 = rsb.GpuBWT(runs=np.array([1 << 5], np.uint8), num_strings=0, ktab_depth=None)
    except rsb.RsbwtError:
        g0 = None  # (an index of no symbols cannot be opened: there is no handle to refuse)
    if g0 is not None:
        assert g0.getBWLen() == 0
        assert L.rsbwt_read_copies(g0.handle, km.ctypes.data, 2, 5, 5, out.ctypes.data, None) == EINVAL and b"empty index" in L.rsbwt_last_error()
        assert L.rsbwt_read_copies_dev(g0.handle, km.ctypes.data, km.ctypes.data, 2, 5, out.ctypes.data, None, None) == EINVAL
        s0 = rsb.ShardSet([g0])
        assert L.rsbwt_set_read_copies_var(s0._s, km.ctypes.data, np.array([0, 9, 14], np.uint64).ctypes.data, 2, out.ctypes.data, None) == EINVAL
        s0.close()
        g0.close()


# ---- 5. two modes, one answer ---------------------------------------------------------------------------------------------

def test_gpu_two_modes_one_answer(rsb, fixture_bwt, tmp_path):
    path, meta = fixture_bwt
    rd = str(tmp_path / "fx.reads")
    rsb.synth_popbwt(str(tmp_path / "fx.bwt"), rd, **meta["synth"])
    reads = open(rd).read().split()
    rng = random.Random(5)
    rl = len(reads[0])
    by_len = {}
    lens = sorted({rl, min(73, rl), min(100, rl), 50, 60})  # the service's tile lengths 73 and 100, held to the fixture's read length
    for ln in lens:
        out = []
        for _ in range(20000 // len(lens) + 1):
            r = reads[rng.randrange(len(reads))]
            s = rng.randrange(len(r) - ln + 1)
            t = r[s:s + ln]
            if rng.random() < 0.3:
                i = rng.randrange(ln)
                t = t[:i] + rng.choice("ACGTN") + t[i + 1:]
            out.append(t)
        by_len[ln] = out
    by_len[rl] = by_len[rl][:len(by_len[rl]) // 2] + [reads[rng.randrange(len(reads))] for _ in range(len(by_len[rl]) // 2)]
    assert sum(map(len, by_len.values())) >= 20000
    # What the extraction path builds on a shard opened without RSBWT_OPEN_READS is its select samples, into a side table
    # (ensure_select_samples, csrc/capi.hip): rsbwt_hbm_bytes grows by that table on the first extraction.  (psi hints are
    # NOT it: on such a shard only rsbwt_prepare_extraction writes them, so rsbwt_psi_hint_lines stays 0 in either mode --
    # tests/test_gpu_sets.py says the same -- and could not tell the two modes apart.)
    with rsb.GpuBWT(path) as g:
        L = rsb.lib()
        assert L.rsbwt_psi_hint_lines(g.handle) == 0 and not L.rsbwt_opened_for_reads(g.handle)
        hbm0 = g.hbm_bytes()
        g.exactmatch_by_search = True
        by_search = {ln: rsb.query_exactmatch_batch(g, ws) for ln, ws in by_len.items()}
        assert g.hbm_bytes() == hbm0, "search mode built the select samples"
        rsb.read_copies(g, by_len[rl][:500])
        ss = rsb.ShardSet([g])
        ss.read_copies_var(by_len[rl][:300] + by_len[50][:300])
        ss.close()
        assert g.hbm_bytes() == hbm0 and L.rsbwt_psi_hint_lines(g.handle) == 0, "rsbwt_read_copies / rsbwt_set_read_copies_var built extraction state"
        g.exactmatch_by_search = False
        by_extract = {ln: rsb.query_exactmatch_batch(g, ws) for ln, ws in by_len.items()}
        assert g.hbm_bytes() > hbm0, "the control: the same call by extraction builds the select samples"
        hbm1 = g.hbm_bytes()
        g.exactmatch_by_search = True
        again = rsb.query_exactmatch_batch(g, by_len[rl])
        assert g.hbm_bytes() == hbm1 and np.array_equal(again, by_search[rl])
    for ln in by_len:
        assert np.array_equal(by_search[ln], by_extract[ln]), ln
    assert by_search[rl].sum() >= len(by_len[rl]) // 2


# ---- 6. callers -------------------------------------------------------------------------------------------------------------

def test_gpu_service_loop_golden_replies_in_search_mode(rsb, fixture_bwt, golden_dir):
    """Reads and KmerMatch goldens through the loop, in process, with every shard's query_exactmatch by search: byte-equal"""
    from test_service_slice import _same
    L = rsb.lib()
    path, _ = fixture_bwt
    gr = json.load(open(os.path.join(golden_dir, "service_reads_v1.json")))
    gk = json.load(open(os.path.join(golden_dir, "service_kmer_v1.json")))
    assert (gr["min_read_length"], gr["max_read_length"]) == (gk["min_read_length"], gk["max_read_length"])
    items = gr["items"] + gk["items"]
    g = rsb.GpuBWT(path, for_reads=True)
    ss = rsb.ShardSet([g])
    ss.exactmatch_by_search(True)
    assert g.exactmatch_by_search is True
    tr, svc = C.c_void_p(), C.c_void_p()
    assert L.rsbwt_transport_inproc(C.byref(tr)) == 0
    assert L.rsbwt_service_create(ss._s, tr, 2000, 64, 1, C.byref(svc)) == 0
    L.rsbwt_service_set_reads(svc, 1, gr["min_read_length"], gr["max_read_length"])
    assert L.rsbwt_service_set_kmermatch(svc, 1) == 0
    assert L.rsbwt_service_start(svc) == 0
    for x in items:
        w = bytes.fromhex(x["request"])
        buf = (C.c_uint8 * len(w)).from_buffer_copy(w)
        assert L.rsbwt_transport_push_request(tr, buf, len(w)) == 0
    BUF = 4 << 20
    buf = (C.c_uint8 * BUF)()
    n = C.c_size_t()
    for x in items:
        for j, want in enumerate(x["replies"]):
            assert L.rsbwt_transport_pop_reply(tr, 0, buf, BUF, C.byref(n), 60_000_000) == 0, (x["q"][:30], j)
            assert _same(bytes(buf[:n.value]), want), (x["t"], x["rt"], x["q"][:30], j)
    L.rsbwt_transport_close(tr)
    assert L.rsbwt_service_stop(svc) == 0
    L.rsbwt_service_free(svc)
    L.rsbwt_transport_free(tr)
    ss.close()
    g.close()


def test_gpu_kmer_reads_long_tiles_in_search_mode(rsb, oracle, tmp_path):
    """ShardSet.kmer_reads on tiles of min_read_length or more (find_kmer_reads asks query_exactmatch of every sub-tile):
    the cases of tests/test_gpu_kmer_match.py, the switch on"""
    kw = dict(seed=77, genome_len=12000, haplotypes=5, snp_rate=0.004, read_len=70, coverage=3.0)
    shards, oixs = [], []
    for s in range(4):
        p = str(tmp_path / f"s{s}.bwt")
        rsb.synth_popbwt(p, None, shard=s, num_shards=4, **kw)
        shards.append(rsb.GpuBWT(p, ktab_depth=6, for_reads=True))
        oixs.append(oracle.load(p))
    rd = str(tmp_path / "whole.reads")
    rsb.synth_popbwt(str(tmp_path / "whole.bwt"), rd, **kw)
    reads = open(rd).read().split()
    ss = rsb.ShardSet(shards)
    ss.exactmatch_by_search(True)
    rng = np.random.default_rng(9)
    qs = []
    for _ in range(4):
        r = reads[rng.integers(len(reads))]
        qs.append(r[:70])
    qs.append(reads[3] + reads[7][:20])
    hits = 0
    for k, skip in ((50, 0), (60, 5), (70, 1)):
        got = ss.kmer_reads(qs, k, skip, min_read_length=50, max_read_length=70)
        for q, w in enumerate(qs):
            for p, oix in enumerate(oixs):
                exp = _expected(oix, w, k, skip, 50, 70)
                assert set(got[q][p]) == exp, (k, skip, q, p)
                hits += len(exp)
    assert hits > 0
    ss.close()
    for g in shards:
        g.close()


def _cfg(golden_dir, tmp_path, prefix, eps, value):
    """the reference's template service.cfg plus the key; with `eps`, its BWT prefix, sockets and read lengths replaced"""
    text = open(os.path.join(golden_dir, "service_template.cfg")).read()
    if eps is not None:
        for key, val in (("prefix", prefix), ("pull", eps[0]), ("push", eps[1]), ("push_count", eps[2]), ("min_read_length", "50"), ("max_read_length", "70")):
            text, n = re.subn(r'(?m)^%s\s*=\s*"[^"]*"' % key, lambda m: '%s = "%s"' % (key, val), text)
            assert n == 1, key
    p = tmp_path / f"service_{value}.cfg"
    p.write_text(text + f'\nexactmatch = "{value}";\n')
    return str(p)


def test_gpu_service_binary_refuses_an_unknown_exactmatch_value(rsb, golden_dir, tmp_path):
    exe = os.path.join(os.path.dirname(rsb.lib_path()), "rsbwt_service")
    r = subprocess.run([exe, _cfg(golden_dir, tmp_path, "", None, "maybe")], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and 'exactmatch = "maybe"' in r.stderr and "loaded" not in r.stdout


def test_gpu_service_binary_answers_a_golden_request_in_search_mode(rsb, fixture_bwt, golden_dir, tmp_path):
    """rsbwt_service started with exactmatch = "search": one golden ExactMatch-Reads request over real sockets.  Skipped only
    where no libzmq exists."""
    from test_service_slice import _libzmq, _same
    z = _libzmq()
    if z is None or not rsb.lib().rsbwt_zmq_available():
        pytest.skip("no libzmq on this box")
    gr = json.load(open(os.path.join(golden_dir, "service_reads_v1.json")))
    item = next(x for x in gr["items"] if sum(x["reads"]) > 0 and len(x["q"]) >= gr["min_read_length"])
    ZMQ_PUB, ZMQ_PULL, ZMQ_LINGER, ZMQ_RCVTIMEO, ZMQ_LAST_ENDPOINT = 1, 7, 17, 27, 32
    ctx = z.zmq_ctx_new()
    socks, eps = [], []
    for typ in (ZMQ_PUB, ZMQ_PULL, ZMQ_PULL):
        so = z.zmq_socket(ctx, typ)
        zero, tmo = C.c_int(0), C.c_int(500)
        z.zmq_setsockopt(so, ZMQ_LINGER, C.byref(zero), 4)
        z.zmq_setsockopt(so, ZMQ_RCVTIMEO, C.byref(tmo), 4)
        assert z.zmq_bind(so, b"tcp://127.0.0.1:*") == 0
        ep = C.create_string_buffer(256)
        n = C.c_size_t(256)
        assert z.zmq_getsockopt(so, ZMQ_LAST_ENDPOINT, ep, C.byref(n)) == 0
        socks.append(so)
        eps.append(ep.value.decode())
    pub, pull, pull_count = socks
    path, _ = fixture_bwt
    exe = os.path.join(os.path.dirname(rsb.lib_path()), "rsbwt_service")
    cfg = _cfg(golden_dir, tmp_path, path[:-4], eps, "search")
    proc = subprocess.Popen([exe, cfg], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    try:
        req = bytes.fromhex(item["request"])
        BUF = 4 << 20
        buf = C.create_string_buffer(BUF)
        got, t0 = [], time.time()
        # PUB/SUB drops what is published before the subscription has arrived: publish until the first reply comes
        while not got and time.time() - t0 < 120 and proc.poll() is None:
            z.zmq_send(pub, req, len(req), 0)
            n = z.zmq_recv(pull, buf, BUF, 0)
            if n >= 0:
                got.append(buf.raw[:n])
        assert got, "rsbwt_service never answered: " + (proc.stderr.read() if proc.poll() is not None else "")
        tmo = C.c_int(20000)
        z.zmq_setsockopt(pull, ZMQ_RCVTIMEO, C.byref(tmo), 4)
        n = z.zmq_recv(pull, buf, BUF, 0)
        assert n >= 0
        got.append(buf.raw[:n])
        for j, want in enumerate(item["replies"]):
            assert _same(got[j], want), j
    finally:
        proc.terminate()
        try:
            proc.wait(timeout=30)
        except subprocess.TimeoutExpired:
            proc.kill()
            proc.wait()
        for so in socks:
            z.zmq_close(so)
        z.zmq_ctx_term(ctx)


# ---- 7. sets -------------------------------------------------------------------------------------------------------------------

def test_gpu_set_equals_the_per_shard_calls(rsb):
    fx = F.fixture("pop")
    reads, others = RC.queries("pop")
    qs = (reads + others)[::3] + ["A" * 65536]  # (one longer than a start record can say: 0 / 0)
    gs = [rsb.GpuBWT(runs=runs, num_strings=len(sh), ktab_depth=6) for sh, runs in zip(fx.shards, fx.runs())]
    ss = rsb.ShardSet(gs)
    cp, en = ss.read_copies_var(qs)
    for p, g in enumerate(gs):
        c, e = _fixed(rsb, g, qs[:-1])
        assert np.array_equal(cp[p][:-1], c) and np.array_equal(en[p][:-1], e)
        assert cp[p][-1] == 0 and en[p][-1] == 0
    assert not np.array_equal(cp[0], cp[1])
    ss.close()
    for g in gs:
        g.close()


def test_gpu_set_split_over_two_devices(rsb, two_devices):
    """shards on devices 0 and 1 (two logical devices on GPU 0 where the box has one: tests/test_gpu_sets.py, two_devices)
    form two groups; the answers are the one-device set's"""
    fx = F.fixture("pop")
    reads, others = RC.queries("pop")
    qs = (reads + others)[::2]

    def run(devs):
        gs = [rsb.GpuBWT(runs=runs, num_strings=len(sh), ktab_depth=6, device=d) for (sh, runs), d in zip(zip(fx.shards, fx.runs()), devs)]
        ss = rsb.ShardSet(gs)
        ndev = rsb.lib().rsbwt_set_devices(ss._s)
        out = ss.read_copies_var(qs)
        ss.close()
        for g in gs:
            g.close()
        return ndev, out
    n1, one = run([0, 0])
    n2, two = run([1, 0])
    assert (n1, n2) == (1, 2)
    assert np.array_equal(one[0], two[0]) and np.array_equal(one[1], two[1])
    assert int(one[0].sum()) > 500
