"""KmerMatch Count / Reads on the GPU (-m gpu): rsbwt_set_kmer_reads against the oracle composition of the reference's
find_kmer_reads (src/service/service.cpp:466-502: every row of every tile's interval extracted, the strings folded into
a set), per shard; the work counters that show one extraction per distinct read; a shard with duplicate reads; a very
wide request beside ordinary ones; and the service loop with kmermatch on and unserved requests answered empty."""
import ctypes as C

import numpy as np
import pytest

import proto_schema
from kmer_reference import _bwt_runs, _expected, _rc

pytestmark = pytest.mark.gpu

MINL, MAXL = 50, 70


@pytest.fixture(scope="module")
def kshards(rsb, oracle, tmp_path_factory):
    d = tmp_path_factory.mktemp("kset")
    kw = dict(seed=77, genome_len=12000, haplotypes=5, snp_rate=0.004, read_len=70, coverage=3.0)
    shards, oixs = [], []
    for s in range(4):
        p = str(d / f"s{s}.bwt")
        rsb.synth_popbwt(p, None, shard=s, num_shards=4, **kw)
        shards.append(rsb.GpuBWT(p, ktab_depth=6, for_reads=True))
        oixs.append(oracle.load(p))
    rd = str(d / "whole.reads")
    rsb.synth_popbwt(str(d / "whole.bwt"), rd, **kw)
    reads = open(rd).read().split()
    ss = rsb.ShardSet(shards)
    yield ss, oixs, reads
    ss.close()
    for g in shards:
        g.close()


def _queries(reads, rng, n, length):
    out = []
    for _ in range(n):
        r = reads[rng.integers(len(reads))]
        s = int(rng.integers(0, len(r) - length + 1))
        out.append(r[s:s + length])
    return out


@pytest.mark.parametrize("k,skip", [(15, 0), (20, 1), (31, 5), (12, 40)])
def test_gpu_kmer_reads_are_the_oracle_composition(rsb, kshards, k, skip):
    """per shard, the distinct reads every ACGT tile's interval holds -- no read missing, none twice"""
    ss, oixs, reads = kshards
    rng = np.random.default_rng(k * 100 + skip)
    qs = _queries(reads, rng, 10, 60)
    qs += [_rc(q) for q in qs[:4]]
    qs += [qs[0][:30] + "N" + qs[0][31:], "ACGT" * 20, qs[1][:k - 1], "A" * 64]
    got = ss.kmer_reads(qs, k, skip)
    cnt = ss.kmer_count(qs, k, skip)
    nonempty = 0
    for q, w in enumerate(qs):
        for p, oix in enumerate(oixs):
            exp = _expected(oix, w, k, skip)
            assert len(got[q][p]) == len(set(got[q][p])), (q, p)
            assert set(got[q][p]) == exp, (q, p, w)
            assert int(cnt[q, p]) == len(exp)
            nonempty += bool(exp)
    assert nonempty > 10


def test_gpu_kmer_reads_long_tiles_take_find_reads_other_branches(rsb, kshards):
    """tiles of min_read_length or more: their sub-tiles that are reads, and below max_read_length the reads that
    contain them (service.cpp:755-797)"""
    ss, oixs, reads = kshards
    rng = np.random.default_rng(9)
    qs = _queries(reads, rng, 4, 70) + [reads[3] + reads[7][:20]]
    for k, skip in ((50, 0), (60, 5), (70, 1)):
        got = ss.kmer_reads(qs, k, skip, min_read_length=MINL, max_read_length=MAXL)
        for q, w in enumerate(qs):
            for p, oix in enumerate(oixs):
                assert set(got[q][p]) == _expected(oix, w, k, skip, MINL, MAXL), (k, skip, q, p)


def test_gpu_kmer_edge_cases_answer_nothing(rsb, kshards):
    """k <= 0, skip < 0, a query shorter than k: no reads (the edge-case table)"""
    ss, _, reads = kshards
    w = reads[0][:40]
    for k, skip in ((0, 0), (-3, 0), (15, -1), (41, 0)):
        assert all(x == [] for row in ss.kmer_reads([w, ""], k, skip) for x in row)
        assert int(ss.kmer_count([w], k, skip).sum()) == 0


def test_gpu_kmer_work_counters_show_one_extraction_per_read(rsb, kshards):
    """overlapping tiles: many candidate rows per read, each read extracted once, and most rows end on the chain"""
    ss, _, reads = kshards
    qs = [reads[5][:64], reads[9][:64]]
    ss.kmer_reads(qs, 15, 0)
    w = rsb.ShardSet.kmer_last_work()
    assert w["extracted"] == w["identities"]  # (rows handed to the extraction calls: no read twice, none over the stride)
    assert 0 < w["identities"] < w["candidates"]
    t = rsb.ShardSet.kmer_last_times()
    assert 0 < t["device_ms"] <= t["total_ms"]
    assert w["walked"] < w["candidates"]
    assert w["lf_steps"] > 0


def test_gpu_kmer_duplicate_reads_collapse_as_strings(rsb, oracle):
    """the same read string at several BWT identities: the set holds it once, skip > 0"""
    rng = np.random.default_rng(5)
    genome = "".join("ACGT"[x] for x in rng.integers(0, 4, 400))
    reads = [genome[s:s + 60] for s in rng.integers(0, 340, 150)]
    assert len(reads) > len(set(reads)), "the fixture must hold duplicate reads"
    runs = _bwt_runs(reads)
    oix = oracle.from_runs(runs, len(reads))
    with rsb.GpuBWT(runs=runs, num_strings=len(reads), ktab_depth=6, for_reads=True) as g:
        ss = rsb.ShardSet([g])
        try:
            qs = [genome[100:150], genome[37:90], _rc(genome[200:245])]
            for skip in (2, 7):
                got = ss.kmer_reads(qs, 17, skip)
                work = rsb.ShardSet.kmer_last_work()
                for q, w in enumerate(qs):
                    assert len(got[q][0]) == len(set(got[q][0]))
                    assert set(got[q][0]) == _expected(oix, w, 17, skip)
                assert work["identities"] > len(set(x for row in got for x in row[0]))  # duplicates: more identities than strings
        finally:
            ss.close()


@pytest.mark.parametrize("wide_rows", [None, "50"])
def test_gpu_kmer_wide_request_leaves_the_others_alone(rsb, kshards, monkeypatch, wide_rows):
    """a k = 8 request over a whole read beside ordinary ones: their answers are unchanged, whether it shares their pass
    or -- RSBWT_KMER_WIDE_ROWS below its candidate rows -- goes through the device in a pass of its own"""
    ss, oixs, reads = kshards
    rng = np.random.default_rng(3)
    qs = _queries(reads, rng, 6, 60)
    alone = ss.kmer_reads(qs, 8, 0)
    wide = reads[0]
    if wide_rows:
        monkeypatch.setenv("RSBWT_KMER_WIDE_ROWS", wide_rows)
    mixed = ss.kmer_reads(qs[:3] + [wide] + qs[3:], 8, 0)
    work = rsb.ShardSet.kmer_last_work()
    assert mixed[:3] + mixed[4:] == alone
    for p, oix in enumerate(oixs):
        assert set(mixed[3][p]) == _expected(oix, wide, 8, 0)
    if wide_rows:
        assert work["candidates"] > int(wide_rows)  # (the wide job had a pass of its own)


def _same(got, want):
    import hashlib
    if isinstance(want, dict):
        return len(got) == want["len"] and hashlib.sha256(got).hexdigest() == want["sha256"]
    return got == bytes.fromhex(want)


def _golden(golden_dir):
    import json
    import os
    return json.load(open(os.path.join(golden_dir, "service_kmer_v1.json")))


def test_gpu_service_kmer_golden_replies(rsb, fixture_bwt, golden_dir):
    """the golden KmerMatch Requests (tests/golden/service_kmer_v1.json: reads from the compiled reference, the
    unordered_set orders from the C++ library) and one Request of every unserved (t, rt) pair through the loop with
    kmermatch on and unserved = empty: every Reply byte for byte, in order, on push"""
    gold = _golden(golden_dir)
    L = rsb.lib()
    path, _ = fixture_bwt
    g = rsb.GpuBWT(path, for_reads=True)
    ss = rsb.ShardSet([g])
    items = gold["items"] + gold["unserved"]
    tr, svc = C.c_void_p(), C.c_void_p()
    assert L.rsbwt_transport_inproc(C.byref(tr)) == 0
    assert L.rsbwt_service_create(ss._s, tr, 2000, 64, 1, C.byref(svc)) == 0
    L.rsbwt_service_set_reads(svc, 1, gold["min_read_length"], gold["max_read_length"])
    assert L.rsbwt_service_set_kmermatch(svc, 1) == 0
    L.rsbwt_service_set_unserved(svc, 1)
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
            assert L.rsbwt_transport_pop_reply(tr, 0, buf, BUF, C.byref(n), 60_000_000) == 0, (x["q"], j)
            assert _same(bytes(buf[:n.value]), want), (x["t"], x["rt"], x.get("k"), x.get("s"), x["q"], j)
    L.rsbwt_transport_close(tr)
    assert L.rsbwt_service_stop(svc) == 0
    assert L.rsbwt_transport_pop_reply(tr, 0, buf, BUF, C.byref(n), 1000) != 0  # exactly two per request, no more
    assert L.rsbwt_transport_pop_reply(tr, 1, buf, BUF, C.byref(n), 1000) != 0
    assert L.rsbwt_service_kmer_requests(svc) == len(gold["items"])
    assert sum(1 for x in gold["items"] if sum(x["reads"]) > 1000) >= 1
    L.rsbwt_service_free(svc)
    L.rsbwt_transport_free(tr)
    ss.close()
    g.close()


def test_gpu_service_kmer_golden_over_real_zeromq_sockets(rsb, fixture_bwt, golden_dir):
    """the same golden Requests over real sockets (the front-end's PUB and two PULLs bound here, the service's SUB / PUSH /
    PUSH connected through libzmq bound at run time).  Skipped only where no libzmq exists."""
    import time
    from test_service_slice import _libzmq
    z = _libzmq()
    L = rsb.lib()
    if z is None or not L.rsbwt_zmq_available():
        pytest.skip("no libzmq on this box")
    gold = _golden(golden_dir)
    ZMQ_PUB, ZMQ_PULL, ZMQ_LINGER, ZMQ_RCVTIMEO, ZMQ_LAST_ENDPOINT = 1, 7, 17, 27, 32
    ctx = z.zmq_ctx_new()
    socks, eps = [], []
    for typ in (ZMQ_PUB, ZMQ_PULL, ZMQ_PULL):
        so = z.zmq_socket(ctx, typ)
        zero, tmo = C.c_int(0), C.c_int(60000)
        z.zmq_setsockopt(so, ZMQ_LINGER, C.byref(zero), 4)
        z.zmq_setsockopt(so, ZMQ_RCVTIMEO, C.byref(tmo), 4)
        assert z.zmq_bind(so, b"tcp://127.0.0.1:*") == 0
        ep = C.create_string_buffer(256)
        n = C.c_size_t(256)
        assert z.zmq_getsockopt(so, ZMQ_LAST_ENDPOINT, ep, C.byref(n)) == 0
        socks.append(so)
        eps.append(ep.value)
    pub, pull, pull_count = socks
    path, _ = fixture_bwt
    g = rsb.GpuBWT(path, for_reads=True)
    ss = rsb.ShardSet([g])
    tr, svc = C.c_void_p(), C.c_void_p()
    assert L.rsbwt_transport_zmq(eps[0], eps[1], eps[2], C.byref(tr)) == 0, L.rsbwt_last_error()
    assert L.rsbwt_service_create(ss._s, tr, 2000, 512, 1, C.byref(svc)) == 0
    L.rsbwt_service_set_reads(svc, 1, gold["min_read_length"], gold["max_read_length"])
    assert L.rsbwt_service_set_kmermatch(svc, 1) == 0
    L.rsbwt_service_set_unserved(svc, 1)
    assert L.rsbwt_service_start(svc) == 0
    BUF = 4 << 20
    buf = C.create_string_buffer(BUF)
    # PUB/SUB drops what is published before the subscription has arrived: wait for a probe to be answered
    probe = bytes.fromhex(gold["unserved"][0]["request"])
    t0, up = time.time(), False
    tmo = C.c_int(200)
    z.zmq_setsockopt(pull, ZMQ_RCVTIMEO, C.byref(tmo), 4)
    while not up and time.time() - t0 < 20:
        z.zmq_send(pub, probe, len(probe), 0)
        up = z.zmq_recv(pull, buf, BUF, 0) >= 0
    assert up, "the service never subscribed"
    time.sleep(0.3)
    tmo = C.c_int(300)
    z.zmq_setsockopt(pull, ZMQ_RCVTIMEO, C.byref(tmo), 4)
    while z.zmq_recv(pull, buf, BUF, 0) >= 0:
        pass
    tmo = C.c_int(60000)
    z.zmq_setsockopt(pull, ZMQ_RCVTIMEO, C.byref(tmo), 4)
    items = gold["items"][::2] + gold["unserved"]
    for x in items:
        w = bytes.fromhex(x["request"])
        assert z.zmq_send(pub, w, len(w), 0) == len(w)
    for x in items:
        for j, want in enumerate(x["replies"]):
            n = z.zmq_recv(pull, buf, BUF, 0)
            assert 0 <= n <= BUF, "a reply is missing"
            assert _same(buf.raw[:n], want), (x["t"], x["rt"], x["q"], j)
    tmo = C.c_int(300)
    z.zmq_setsockopt(pull, ZMQ_RCVTIMEO, C.byref(tmo), 4)
    assert z.zmq_recv(pull, buf, BUF, 0) < 0  # exactly two per request, no more
    assert z.zmq_recv(pull_count, buf, BUF, 0) < 0
    L.rsbwt_transport_close(tr)
    assert L.rsbwt_service_stop(svc) == 0
    L.rsbwt_service_free(svc)
    L.rsbwt_transport_free(tr)
    for so in socks:
        z.zmq_close(so)
    z.zmq_ctx_term(ctx)
    ss.close()
    g.close()


def _serve(rsb, ss, msgs, per_partition, kmermatch=True, unserved=True):
    L = rsb.lib()
    tr, svc = C.c_void_p(), C.c_void_p()
    assert L.rsbwt_transport_inproc(C.byref(tr)) == 0
    assert L.rsbwt_service_create(ss._s, tr, 2000, 64, per_partition, C.byref(svc)) == 0
    L.rsbwt_service_set_reads(svc, 1, MINL, MAXL)
    assert L.rsbwt_service_set_kmermatch(svc, 1 if kmermatch else 0) == 0
    L.rsbwt_service_set_unserved(svc, 1 if unserved else 0)
    assert L.rsbwt_service_start(svc) == 0
    for m in msgs:
        buf = (C.c_uint8 * len(m)).from_buffer_copy(m)
        assert L.rsbwt_transport_push_request(tr, buf, len(m)) == 0
    L.rsbwt_transport_close(tr)
    assert L.rsbwt_service_stop(svc) == 0
    out = {0: [], 1: []}
    buf = (C.c_uint8 * (1 << 20))()
    n = C.c_size_t()
    for ch in (0, 1):
        while L.rsbwt_transport_pop_reply(tr, ch, buf, len(buf), C.byref(n), 200_000) == 0:
            out[ch].append(bytes(buf[:n.value]))
    L.rsbwt_service_free(svc)
    L.rsbwt_transport_free(tr)
    return out


def test_gpu_service_answers_kmermatch_and_unserved(rsb, kshards):
    """the loop with kmermatch on: 2 replies per partition per KmerMatch Count / Reads request, in arrival order, each
    what rsbwt_set_kmer_reads finds for that strand and shard; with unserved = empty every other (t, rt) pair gets its
    2 x P empty replies on push"""
    ss, _, reads = kshards
    Request, Reply = proto_schema.build()
    L = rsb.lib()
    S = 4
    rng = np.random.default_rng(12)
    qs = _queries(reads, rng, 5, 60)
    reqs = []
    for i, q in enumerate(qs):
        for rt in (1, 2):
            r = Request()
            r.t, r.rt, r.q, r.k, r.s = 3, rt, q, (15, 31, 20, 50, 12)[i], (0, 1, 5, 0, 40)[i]
            reqs.append(r)
    for t, rt in ((2, 3), (2, 4), (3, 3), (3, 4), (4, 1), (4, 2), (4, 3), (4, 4)):
        r = Request()
        r.t, r.rt, r.q, r.k, r.s, r.p = t, rt, qs[0], 31, 0, 10
        reqs.append(r)
    for per_partition in (1, 0):
        out = _serve(rsb, ss, [r.SerializeToString() for r in reqs], per_partition)
        rows = S if per_partition else 1
        assert out[1] == []
        assert len(out[0]) == 2 * rows * len(reqs)
        at = 0
        for r in reqs:
            mine = out[0][at:at + 2 * rows]
            at += 2 * rows
            if r.t == 3 and r.rt in (1, 2):
                fwd = ss.kmer_reads([r.q], r.k, r.s, MINL, MAXL)[0]
                rev = ss.kmer_reads([_rc(r.q)], r.k, r.s, MINL, MAXL)[0]
                exp = []
                for p in range(rows):
                    for strand, lists in ((0, fwd), (1, rev)):
                        lst = lists[p] if per_partition else [x for y in lists for x in y]
                        arr = (C.c_char_p * max(len(lst), 1))(*[x.encode() for x in lst])
                        lens = (C.c_size_t * max(len(lst), 1))(*[len(x) for x in lst])
                        n = L.rsbwt_proto_encode_kmer_reply(None, 0, r.rt, r.q.encode(), len(r.q), strand, arr, lens, len(lst))
                        b = (C.c_uint8 * n)()
                        L.rsbwt_proto_encode_kmer_reply(b, n, r.rt, r.q.encode(), len(r.q), strand, arr, lens, len(lst))
                        exp.append(bytes(b))
                assert mine == exp, (r.k, r.s, r.rt, per_partition)
            else:
                exp = []
                for p in range(rows):
                    for strand in (0, 1):
                        n = L.rsbwt_proto_encode_empty_reply(None, 0, r.t, r.rt, r.q.encode(), len(r.q), strand)
                        b = (C.c_uint8 * n)()
                        L.rsbwt_proto_encode_empty_reply(b, n, r.t, r.rt, r.q.encode(), len(r.q), strand)
                        exp.append(bytes(b))
                assert mine == exp, (r.t, r.rt)
            if r.rt in (1, 2):  # (the re-typed schema parses what it knows)
                rep = Reply()
                rep.ParseFromString(mine[0])
                assert (rep.rt, rep.t, rep.q) == (r.t, r.rt, r.q)
    # off (the default): no reply for any of these requests, as before
    out = _serve(rsb, ss, [r.SerializeToString() for r in reqs], 1, kmermatch=False, unserved=False)
    assert out[0] == [] and out[1] == []


def test_gpu_kmermatch_needs_shards_opened_for_reads(rsb, kshards, tmp_path):
    ss, _, _ = kshards
    L = rsb.lib()
    p = str(tmp_path / "plain.bwt")
    rsb.synth_popbwt(p, None, seed=1, genome_len=3000, haplotypes=2, snp_rate=0.01, read_len=60, coverage=2.0)
    with rsb.GpuBWT(p, ktab_depth=6) as g:
        plain = rsb.ShardSet([g])
        tr, svc = C.c_void_p(), C.c_void_p()
        assert L.rsbwt_transport_inproc(C.byref(tr)) == 0
        assert L.rsbwt_service_create(plain._s, tr, 200, 16, 1, C.byref(svc)) == 0
        assert L.rsbwt_service_set_kmermatch(svc, 1) == -1
        assert b"RSBWT_OPEN_READS" in L.rsbwt_last_error()
        assert L.rsbwt_service_set_kmermatch(svc, 0) == 0
        L.rsbwt_service_free(svc)
        L.rsbwt_transport_free(tr)
        plain.close()
