"""rsbwt_set_query_var_capped / rsbwt_set_interval_rows_dev (csrc/interval_rows.hip, csrc/sets.hip) and the service's
max_match_reads: the expansion against numpy on pairs given by hand, the reads against the oracle on the multi-shard
fixtures, the uncapped call against rsbwt_set_query_var byte for byte, the sizing protocol, the work counters (no row
visits the host on a one-device set), two device groups, and a window of the service loop that holds "A"."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import test_kmer_fixtures as F
from test_gpu_sets import two_devices  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

ERANGE = -7
U64MAX = 2**64 - 1
SENTINEL_U32, SENTINEL_U64 = 0xA5A5A5A5, 0x5A5A5A5A5A5A5A5A
WIDE = 70001


# ---- 1. the expansion against numpy ------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def tiny_shards(rsb):
    """three small run streams of different lengths (each longer than the 70,001-row interval of the test)"""
    L = rsb.lib()
    gs = []
    for seed, R in ((11, 60000), (12, 45000), (13, 52000)):
        runs = np.empty(R, np.uint8)
        assert L.rsbwt_synth_runs_host(runs.ctypes.data, R, seed) == 0
        gs.append(rsb.GpuBWT(runs=runs, ktab_depth=None))
    yield gs
    for g in gs:
        g.close()


def _hand_pairs(ns, Q):
    """[S][Q] pairs cycling through the kinds the width rule tells apart, one interval of 70,001 rows among them"""
    S = len(ns)
    lo = np.zeros((S, Q), np.uint64)
    up = np.zeros((S, Q), np.uint64)
    for i, n in enumerate(ns):
        kinds = [(1, 0), (0, U64MAX), (n - 5, n), (n - 3, n - 1), (5, 3), (7 + i, 7 + i), (10, 12), (n, n), (0, 0), (2, 9)]
        for q in range(Q):
            lo[i, q], up[i, q] = kinds[(q + 3 * i) % len(kinds)]
    lo[0, Q // 2], up[0, Q // 2] = 100, 100 + WIDE - 1
    return lo, up


def _expected_rows(lo, up, ns, max_rows):
    S, Q = lo.shape
    nn = np.array(ns, np.uint64)[:, None]
    ok = (lo <= up) & (up < nn)
    w = np.where(ok, up - lo + np.uint64(1), np.uint64(0)).astype(np.uint64)
    matches = w.sum(axis=0, dtype=np.uint64)
    keep = np.ones(Q, bool) if max_rows == 0 else matches <= np.uint64(max_rows)
    wk = np.where(keep[None, :], w, np.uint64(0)).astype(np.int64)
    first = np.zeros(Q + 1, np.uint64)
    first[1:] = np.cumsum(wk.sum(axis=0))
    flat_w = wk.T.reshape(-1)                                    # query-major, shard ascending inside a query
    shard = np.repeat(np.tile(np.arange(S, dtype=np.uint32), Q), flat_w)
    starts = np.repeat(lo.T.reshape(-1), flat_w)
    cell_first = np.repeat(np.cumsum(flat_w) - flat_w, flat_w)
    rows = starts + (np.arange(int(flat_w.sum()), dtype=np.int64) - cell_first).astype(np.uint64)
    return first, matches, shard, rows


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("Q", [1, 63, 64, 65, 1025])
def test_gpu_interval_rows_against_numpy(rsb, tiny_shards, S, Q):
    import torch
    L = rsb.lib()
    gs = tiny_shards[:S]
    ns = [g.getBWLen() for g in gs]
    assert min(ns) > 100 + WIDE
    ss = rsb.ShardSet(gs)
    try:
        lo, up = _hand_pairs(ns, Q)
        pairs = np.stack([lo, up], axis=-1).astype(np.uint64)   # [S][Q][2]
        d_pairs = torch.from_numpy(pairs.view(np.int64)).cuda()
        _, m_all, _, _ = _expected_rows(lo, up, ns, 0)
        biggest = int(m_all.max())
        assert biggest >= WIDE
        for max_rows in sorted({0, 1, WIDE - 1, WIDE, biggest, biggest - 1}):
            first, matches, shard, rows = _expected_rows(lo, up, ns, max_rows)
            total = int(first[Q])
            assert total == shard.size == rows.size
            for cap in sorted({total, total + 3, max(total - 1, 0)}):
                d_first = torch.full((Q + 1,), -1, dtype=torch.int64, device="cuda")
                d_matches = torch.full((Q,), -1, dtype=torch.int64, device="cuda")
                d_shard = torch.from_numpy(np.full(max(cap, 1), SENTINEL_U32, np.uint32).view(np.int32)).cuda()
                d_rows = torch.from_numpy(np.full(max(cap, 1), SENTINEL_U64, np.uint64).view(np.int64)).cuda()
                rc = L.rsbwt_set_interval_rows_dev(ss._s, d_pairs.data_ptr(), Q, max_rows, d_first.data_ptr(), d_matches.data_ptr(),
                                                   d_shard.data_ptr(), d_rows.data_ptr(), cap, None)
                assert rc == 0, L.rsbwt_last_error()
                torch.cuda.synchronize()
                got_first = d_first.cpu().numpy().view(np.uint64)
                got_matches = d_matches.cpu().numpy().view(np.uint64)
                got_shard = d_shard.cpu().numpy().view(np.uint32)
                got_rows = d_rows.cpu().numpy().view(np.uint64)
                what = (S, Q, max_rows, cap, total)
                assert np.array_equal(got_first, first), what
                assert np.array_equal(got_matches, matches), what
                if total <= cap:
                    assert np.array_equal(got_shard[:total], shard), what
                    assert np.array_equal(got_rows[:total], rows), what
                    assert (got_shard[total:] == SENTINEL_U32).all() and (got_rows[total:] == SENTINEL_U64).all(), what
                else:  # too little room: first and matches complete, the lists untouched
                    assert (got_shard == SENTINEL_U32).all() and (got_rows == SENTINEL_U64).all(), what
    finally:
        ss.close()


# ---- 2. the reads against the oracle -------------------------------------------------------------------------------------

_REF = {}


def _batch(fx):
    """1- and 2-symbol queries, k-mers cut from reads, absent ones, one with N, an empty one"""
    import random
    rng = random.Random("capped/" + fx.name)
    reads = sorted({r for sh in fx.shards for r in sh})
    qs = ["A", "C", "AC", "GT", ""]
    for k in (12, 20, 31, 45):
        for _ in range(6):
            r = rng.choice([x for x in reads if len(x) >= k])
            s = rng.randrange(len(r) - k + 1)
            qs.append(r[s:s + k])
    qs += ["".join(rng.choice("ACGT") for _ in range(25)) for _ in range(5)]
    qs.append(qs[6][:5] + "N" + qs[6][6:])
    qs.append("T")
    rng.shuffle(qs)
    return qs


def _reference(oracle, name):
    """per query and shard the reads of the interval's rows, from the oracle's find_interval and extract -- computed once"""
    if name not in _REF:
        fx = F.fixture(name)
        qs = _batch(fx)
        stride = 1024
        per = []
        for sh, runs in zip(fx.shards, fx.runs()):
            oix = oracle.from_runs(runs, len(sh))
            n = oix.bwlen()
            col = []
            for w in qs:
                if not w or set(w) - set("ACGT"):
                    col.append([])
                    continue
                lo, up = oix.find_interval(w)
                if not (lo <= up and up < n):
                    col.append([])
                    continue
                out, ln, _ = oix.extract_batch(np.arange(lo, up + 1, dtype=np.uint64), stride=stride)
                assert (ln != 0xFFFFFFFF).all()
                col.append([out[j, :ln[j]].tobytes().decode() for j in range(len(ln))])
            per.append(col)
        _REF[name] = (qs, per)
    return _REF[name]


def _open_set(rsb, name, devices=None):
    fx = F.fixture(name)
    devices = devices or [0] * len(fx.shards)
    gs = [rsb.GpuBWT(runs=runs, num_strings=len(sh), ktab_depth=6, device=d) for sh, runs, d in zip(fx.shards, fx.runs(), devices)]
    return gs, rsb.ShardSet(gs)


def _raw_call(L, ss, qs, max_rows, cap_reads, stride, fn="rsbwt_set_query_var_capped"):
    """the C call itself on buffers of the test's own: (rc, nreads, first, shard, len, reads, matches)"""
    text, off = ss._var_text(qs)
    Q = len(qs)
    first = np.full(Q + 1, SENTINEL_U64, np.uint64)
    matches = np.full(Q, SENTINEL_U64, np.uint64)
    sh = np.zeros(max(cap_reads, 1), np.uint32)
    ln = np.zeros(max(cap_reads, 1), np.uint32)
    reads = np.zeros((max(cap_reads, 1), stride), np.uint8)
    n = C.c_size_t(12345)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    if fn == "rsbwt_set_query_var":
        rc = L.rsbwt_set_query_var(ss._s, p(text), p(off), Q, p(first), p(sh), p(reads), stride, p(ln), cap_reads, C.byref(n))
    else:
        rc = L.rsbwt_set_query_var_capped(ss._s, p(text), p(off), Q, max_rows, p(first), p(sh), p(reads), stride, p(ln), cap_reads, C.byref(n),
                                          p(matches))
    return rc, n.value, first, sh, ln, reads, matches


def _last_work(L):
    w = (C.c_uint64 * 4)()
    L.rsbwt_set_query_last_work(w)
    return [int(x) for x in w]


@pytest.mark.parametrize("name", ["pop", "repeat", "ragged"])
def test_gpu_capped_reads_against_the_oracle(rsb, oracle, name):
    L = rsb.lib()
    qs, per = _reference(oracle, name)
    S, Q = len(per), len(qs)
    want_matches = np.array([sum(len(per[p][q]) for p in range(S)) for q in range(Q)], np.uint64)
    widest = int(want_matches.max())
    assert widest > 100 and (want_matches == 0).sum() >= 7 and len({len(w) for w in qs}) >= 7
    gs, ss = _open_set(rsb, name)
    try:
        for max_rows in (0, 1, 7, widest, widest - 1):
            keep = [max_rows == 0 or int(want_matches[q]) <= max_rows for q in range(Q)]
            want = [(p, r) for q in range(Q) if keep[q] for p in range(S) for r in per[p][q]]
            want_first = np.zeros(Q + 1, np.uint64)
            want_first[1:] = np.cumsum([int(want_matches[q]) if keep[q] else 0 for q in range(Q)])
            rc, n, first, sh, ln, reads, matches = _raw_call(L, ss, qs, max_rows, len(want) + 2, 1024)
            assert rc == 0, L.rsbwt_last_error()
            assert n == len(want) and np.array_equal(first, want_first), (name, max_rows)
            assert np.array_equal(matches, want_matches), (name, max_rows)
            assert np.array_equal(sh[:n], np.array([p for p, _ in want], np.uint32)), (name, max_rows)
            assert np.array_equal(ln[:n], np.array([len(r) for _, r in want], np.uint32)), (name, max_rows)
            bad = [t for t in range(n) if reads[t, :ln[t]].tobytes().decode() != want[t][1]]
            assert not bad, (name, max_rows, bad[:3])
            work = _last_work(L)
            assert work[:3] == [n, 0, keep.count(False)], (name, max_rows, work)
        # the Python mirror: reads per query and shard, and the totals
        got, m = ss.query_var_capped(qs, 7, read_stride=1024)
        assert np.array_equal(m, want_matches)
        for q in range(Q):
            for p in range(S):
                assert got[q][p] == (per[p][q] if int(want_matches[q]) <= 7 else []), (name, q, p)
    finally:
        ss.close()
        for g in gs:
            g.close()


# ---- 3. - 5. no limit = rsbwt_set_query_var; sizing; residency -----------------------------------------------------------

@pytest.fixture(scope="module")
def pop_set(rsb):
    gs, ss = _open_set(rsb, "pop")
    yield ss
    ss.close()
    for g in gs:
        g.close()


def test_gpu_no_limit_is_query_var_byte_for_byte(rsb, oracle, pop_set):
    L = rsb.lib()
    qs, _ = _reference(oracle, "pop")
    rc0, n0, *_ = _raw_call(L, pop_set, qs, 0, 0, 256, fn="rsbwt_set_query_var")
    assert rc0 == ERANGE and n0 > 1000
    a = _raw_call(L, pop_set, qs, 0, n0 + 5, 256, fn="rsbwt_set_query_var")
    b = _raw_call(L, pop_set, qs, 0, n0 + 5, 256)
    assert a[0] == 0 and b[0] == 0 and a[1] == b[1] == n0
    for x, y, what in zip(a[2:6], b[2:6], ("first", "read_shard", "read_len", "reads")):
        assert np.array_equal(x, y), what
    assert _last_work(L)[:2] == [n0, 0]


def test_gpu_sizing_protocol(rsb, oracle, pop_set):
    L = rsb.lib()
    qs, per = _reference(oracle, "pop")
    m = [sum(len(per[p][q]) for p in range(len(per))) for q in range(len(qs))]
    for max_rows in (0, 7, 40):
        kept = sum(x for x in m if max_rows == 0 or x <= max_rows)
        rc, n, first, _, _, _, matches = _raw_call(L, pop_set, qs, max_rows, 0, 256)
        assert rc == ERANGE and n == kept and int(first[-1]) == kept
        assert max_rows == 0 or kept <= len(qs) * max_rows
        assert [int(x) for x in matches] == m
        # null buffers size too, as rsbwt_set_query_var's do
        text, off = pop_set._var_text(qs)
        first2 = np.zeros(len(qs) + 1, np.uint64)
        nn = C.c_size_t()
        rc = L.rsbwt_set_query_var_capped(pop_set._s, text.ctypes.data_as(C.c_void_p), off.ctypes.data_as(C.c_void_p), len(qs), max_rows,
                                          first2.ctypes.data_as(C.c_void_p), None, None, 256, None, 0, C.byref(nn), None)
        assert rc == ERANGE and nn.value == kept and np.array_equal(first2, first)
    # the null-argument rules of rsbwt_set_query_var, on a real set
    text, off = pop_set._var_text(qs)
    pt, po, pf = (a.ctypes.data_as(C.c_void_p) for a in (text, off, first2))
    assert L.rsbwt_set_query_var_capped(pop_set._s, pt, po, len(qs), 7, pf, None, None, 256, None, 0, None, None) == -1
    assert L.rsbwt_set_query_var_capped(pop_set._s, pt, po, len(qs), 7, pf, None, None, 0, None, 0, C.byref(nn), None) == -1
    assert L.rsbwt_set_query_var_capped(pop_set._s, pt, po, len(qs), 7, None, None, None, 256, None, 0, C.byref(nn), None) == -1
    assert L.rsbwt_set_query_var_capped(pop_set._s, pt, po, len(qs), 7, pf, None, None, 256, None, 1 << 20, C.byref(nn), None) == -1  # rows, nowhere to put them
    assert L.rsbwt_set_query_var_capped(pop_set._s, pt, po, 0, 7, None, None, None, 256, None, 0, C.byref(nn), None) == 0 and nn.value == 0
    # a limit nothing passes: no rows, no room needed
    rc, n, first, *_ = _raw_call(L, pop_set, ["A", "C"], 1, 0, 256)
    assert rc == 0 and n == 0 and not first.any() and _last_work(L)[2] == 2


def test_gpu_rows_never_visit_the_host_on_one_device(rsb, oracle, pop_set):
    L = rsb.lib()
    qs, per = _reference(oracle, "pop")
    m = [sum(len(per[p][q]) for p in range(len(per))) for q in range(len(qs))]
    for max_rows in (0, 7):
        over = sum(1 for x in m if max_rows and x > max_rows)
        kept = sum(x for x in m if max_rows == 0 or x <= max_rows)
        rc, n, *_ = _raw_call(L, pop_set, qs, max_rows, kept, 256)
        assert rc == 0 and n == kept
        work = _last_work(L)
        assert work[0] == n and work[1] == 0 and work[2] == over, work
        # what crossed before the walks were launched: first[], matches[] and a counter -- nothing that grows with the rows
        assert work[3] <= 8 * (2 * len(qs) + 1) + 8, work


# ---- 6. two device groups -------------------------------------------------------------------------------------------------

def test_gpu_two_device_groups_give_the_one_device_answer(rsb, oracle, two_devices):
    L = rsb.lib()
    qs, _ = _reference(oracle, "pop")

    def run(devs):
        gs, ss = _open_set(rsb, "pop", devs)
        try:
            ndev = L.rsbwt_set_devices(ss._s)
            outs = []
            for max_rows in (0, 7):
                rc, n, *_ = _raw_call(L, ss, qs, max_rows, 0, 256)
                assert rc in (0, ERANGE)
                out = _raw_call(L, ss, qs, max_rows, n, 256)
                assert out[0] == 0
                outs.append((out, _last_work(L)))
            return ndev, outs
        finally:
            ss.close()
            for g in gs:
                g.close()
    n1, one = run([0, 0])
    n2, two = run([1, 0])
    assert (n1, n2) == (1, 2)
    for (a, wa), (b, wb) in zip(one, two):
        assert a[1] == b[1] and a[1] > 0
        for x, y in zip(a[2:], b[2:]):
            assert np.array_equal(x, y)
        assert wa[:3] == [a[1], 0, wa[2]] and wb[:3] == [0, b[1], wa[2]]


# ---- 6b. a batch of two slices ----------------------------------------------------------------------------------------------

SLICE = 65536  # where the variable-length loop cuts a batch (csrc/capi.hip, for_each_var_slice)


def _cut_queries(fx):
    """40 queries cut from reads, 9 to 45 symbols: between 1 and about ten rows each over the set"""
    import random
    rng = random.Random("slices/" + fx.name)
    reads = sorted({r for sh in fx.shards for r in sh})
    qs = []
    for k in (9, 12, 20, 45):
        for _ in range(10):
            r = rng.choice([x for x in reads if len(x) >= k])
            s = rng.randrange(len(r) - k + 1)
            qs.append(r[s:s + k])
    return qs


@pytest.mark.parametrize("tail", ["real", "empty"])
def test_gpu_capped_calls_over_two_slices(rsb, pop_set, tail):
    """65,536 + 40 queries: 40 real ones, empty strings up to the cut, and a second slice of the 40 real ones again
    ("real": its pairs are copied into the batch's [S][Q] block row by row) or of 40 empty strings ("empty": the block's
    columns are set, nothing is launched).  Reads and positions of each real segment are those of the 40-query call; the
    empty queries have no matches and zero-width first[]."""
    L = rsb.lib()
    real = _cut_queries(F.fixture("pop"))
    R = len(real)
    again = tail == "real"
    qs = real + [""] * (SLICE - R) + (real if again else [""] * R)
    assert len(qs) == SLICE + R and R == 40

    def check_first(first, matches, f40, m40, where):
        n40 = int(f40[R])
        assert np.array_equal(first[:R + 1], f40) and np.array_equal(matches[:R], m40), where
        assert (first[R:SLICE + 1] == n40).all() and not matches[R:SLICE].any(), where
        if again:
            assert np.array_equal(first[SLICE:] - np.uint64(n40), f40) and np.array_equal(matches[SLICE:], m40), where
        else:
            assert (first[SLICE:] == n40).all() and not matches[SLICE:].any(), where
        return n40

    for max_rows in (0, 7):
        rc, n40, *_ = _raw_call(L, pop_set, real, max_rows, 0, 256)
        assert rc == ERANGE and n40 > 0
        want = _raw_call(L, pop_set, real, max_rows, n40, 256)
        assert want[0] == 0 and want[1] == n40
        assert max_rows == 0 or ((want[6] > max_rows).any() and (want[6] <= max_rows).any())
        total = n40 * (2 if again else 1)
        got = _raw_call(L, pop_set, qs, max_rows, total, 256)
        assert got[0] == 0 and got[1] == total, L.rsbwt_last_error()
        assert check_first(got[2], got[6], want[2], want[6], ("reads", max_rows)) == n40
        for x, y, what in zip(got[3:6], want[3:6], ("read_shard", "read_len", "reads")):
            assert np.array_equal(x[:n40], y[:n40]), (what, max_rows)
            assert not again or np.array_equal(x[n40:total], y[:n40]), (what, max_rows, "second slice")
        assert _last_work(L)[:2] == [total, 0]
    for max_rows in (0, 5):
        want = pop_set.locate_queries(real, max_rows=max_rows)
        got = pop_set.locate_queries(qs, max_rows=max_rows)
        n40 = check_first(got["first"], got["matches"], want["first"], want["matches"], ("locate", max_rows))
        assert n40 > 0 and (max_rows == 0 or ((want["matches"] > max_rows).any() and (want["matches"] <= max_rows).any()))
        for key in ("shard", "row", "read_row", "ordinal", "offset"):
            assert got[key].size == n40 * (2 if again else 1), (key, max_rows)
            assert np.array_equal(got[key][:n40], want[key]), (key, max_rows)
            assert not again or np.array_equal(got[key][n40:], want[key]), (key, max_rows, "second slice")


# ---- 7. the service loop: a window that holds "A" ---------------------------------------------------------------------------

def _reads_request(q):
    assert len(q) < 128
    return bytes([0x08, 0x02, 0x10, 0x02, 0x1A, len(q)]) + q.encode()


def test_gpu_service_window_with_a_wide_query(rsb, oracle, fixture_bwt, golden_dir):
    """service_reads_v1.json's Requests with "A" and "AC" Reads requests woven in, max_match_reads between every golden
    request's row count and theirs: the golden Replies are byte-equal to the file, the wide ones get 2 x P empty Replies"""
    from test_service_slice import _same
    L = rsb.lib()
    path, _ = fixture_bwt
    gr = json.load(open(os.path.join(golden_dir, "service_reads_v1.json")))
    LIMIT = 10000
    # on the CPU first: every golden strand brings fewer reads than the limit, every strand of the wide ones more
    assert max(max(x["reads"]) for x in gr["items"]) < LIMIT
    oix = oracle.load(path)
    wide = ["A", "AC"]
    for w in wide + ["T", "GT"]:  # (their reverse complements are queries of their own)
        lo, up = oix.find_interval(w)
        assert up - lo + 1 > LIMIT, w
    items = []
    for i, x in enumerate(gr["items"]):
        if i in (3, 40, 41, 90):
            items.append(("wide", wide[len([y for y in items if y[0] == "wide"]) % 2]))
        items.append(("golden", x))
    g = rsb.GpuBWT(path, for_reads=True)
    ss = rsb.ShardSet([g])
    tr, svc = C.c_void_p(), C.c_void_p()
    try:
        assert L.rsbwt_transport_inproc(C.byref(tr)) == 0
        assert L.rsbwt_service_create(ss._s, tr, 2000, 64, 1, C.byref(svc)) == 0
        L.rsbwt_service_set_reads(svc, 1, gr["min_read_length"], gr["max_read_length"])
        assert L.rsbwt_service_set_max_match_reads(svc, LIMIT) == 0
        assert L.rsbwt_service_start(svc) == 0
        for kind, x in items:
            w = _reads_request(x) if kind == "wide" else bytes.fromhex(x["request"])
            buf = (C.c_uint8 * len(w)).from_buffer_copy(w)
            assert L.rsbwt_transport_push_request(tr, buf, len(w)) == 0
        BUF = 4 << 20
        buf = (C.c_uint8 * BUF)()
        small = (C.c_uint8 * 64)()
        n = C.c_size_t()
        P = 1
        for kind, x in items:
            if kind == "wide":
                for _ in range(P):
                    for strand in (0, 1):
                        ne = L.rsbwt_proto_encode_empty_reply(small, 64, 2, 2, x.encode(), len(x), strand)
                        assert 0 < ne <= 64
                        assert L.rsbwt_transport_pop_reply(tr, 0, buf, BUF, C.byref(n), 60_000_000) == 0, x
                        assert bytes(buf[:n.value]) == bytes(small[:ne]), (x, strand)
            else:
                for j, want in enumerate(x["replies"]):
                    assert L.rsbwt_transport_pop_reply(tr, 0, buf, BUF, C.byref(n), 60_000_000) == 0, (x["q"][:30], j)
                    assert _same(bytes(buf[:n.value]), want), (x["q"][:30], j)
        L.rsbwt_transport_close(tr)
        assert L.rsbwt_service_stop(svc) == 0
        assert L.rsbwt_service_capped_requests(svc) == 4
        assert L.rsbwt_service_read_requests(svc) == len(items)
    finally:
        L.rsbwt_service_free(svc)
        L.rsbwt_transport_free(tr)
        ss.close()
        g.close()


# ---- 8. the binary ------------------------------------------------------------------------------------------------------------

def test_gpu_service_binary_refuses_a_max_match_reads_that_is_no_number(rsb, golden_dir, tmp_path):
    exe = os.path.join(os.path.dirname(rsb.lib_path()), "rsbwt_service")
    text = open(os.path.join(golden_dir, "service_template.cfg")).read()
    assert not re.search(r"(?m)^max_match_reads", text)
    for value in ("lots", "-3", "1e5", ""):
        p = tmp_path / "service_bad.cfg"
        p.write_text(text + f'\nmax_match_reads = "{value}";\n')
        r = subprocess.run([exe, str(p)], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and f'max_match_reads = "{value}"' in r.stderr and "loaded" not in r.stdout, (value, r.stderr)
