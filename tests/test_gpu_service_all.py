"""All / Samples replies through the service loop (-m gpu): the Requests of tests/golden/service_reads_v1.json (ExactMatch)
and of the Reads items of service_kmer_v1.json (KmerMatch) with their return type rewritten to All and to Samples, answered
from the set's sample table.

The expected bytes are the golden Replies themselves -- reads and read order from the compiled reference -- decoded and
re-encoded by the protobuf runtime as ReplyAll, each read with the ReadInfo records of its value in the pairs: the read
order is the reference's, the `s` rule is tests/meta_proto.py's restatement of src/service/service.cpp:1332-1347.  The six
Reads goldens and the two KmerMatch goldens kept as length + SHA-256 cannot be decoded; for those the Reply received is
taken apart instead: its reads, re-encoded as the ReplyReads the golden is, must hash to the golden, and every read's `s`
must be the records of its value.

The pairs: the union of the reads in the goldens' Replies (those that can be decoded) with meta_reference.value_of, the
hash function of the table tests, over a ladder of SHORT lengths -- 0 to 4 records of 4 bytes, whole and ragged: 0, 1, 3, 4,
5, 8, 11, 12, 16, 17 -- because a window here brings 8,000 reads per Reply and 2 x 61,653 reads in all (the ladder to 5,000
bytes is tests/test_gpu_meta.py's); every 7th read is left out of the pairs (an empty `s`), one read is given twice (the
later value holds).  This module needs rsbwt_service_set_all: it fails on a library without it."""
import ctypes as C
import hashlib
import json
import os

import pytest

import meta_proto
import meta_reference as MR
import proto_schema
from test_gpu_kmer_match import _same

pytestmark = pytest.mark.gpu

SHORT = [0, 1, 3, 4, 5, 8, 11, 12, 16, 17]
SS, OTHER = 2, True  # size_of_sample, has_other_meta_data: the reference's defaults (service.cpp:59-60)
BUF = 8 << 20


class Gold:
    def __init__(self, golden_dir):
        self.Request, self.ReplyR = proto_schema.build()
        self.Reply, _, _ = meta_proto.build()
        gr = json.load(open(os.path.join(golden_dir, "service_reads_v1.json")))
        gk = json.load(open(os.path.join(golden_dir, "service_kmer_v1.json")))
        self.minl, self.maxl = gr["min_read_length"], gr["max_read_length"]
        assert (gk["min_read_length"], gk["max_read_length"]) == (self.minl, self.maxl)
        self.items = gr["items"] + [x for x in gk["items"] if x["rt"] == 2]
        self.unserved = gk["unserved"]
        # the reads of every Reply that can be decoded, in the Reply's order
        self.lists = []
        reads = set()
        for x in self.items:
            per = []
            for strand, rep in enumerate(x["replies"]):
                if isinstance(rep, dict):
                    per.append(None)
                    continue
                m = self.ReplyR()
                m.ParseFromString(bytes.fromhex(rep))
                lst = [y.r for y in (m.r.revcomp_matches if strand else m.r.forward_matches)]
                assert len(lst) == x["reads"][strand]
                per.append(lst)
                reads.update(lst)
            self.lists.append(per)
        order = sorted(reads, key=lambda r: hashlib.sha256(r.encode()).digest())
        self.left_out = set(order[6::7])
        kept = [r for r in order if r not in self.left_out]
        self.pairs = [(r, MR.value_of(r, 0, SHORT)) for r in kept]
        again = next(r for r in kept if MR.value_of(r, 1, SHORT) != MR.value_of(r, 0, SHORT))
        self.pairs.insert(0, (again, MR.value_of(again, 1, SHORT)))  # given twice: the later pair (tag 0) holds
        self.value = {}
        for r, v in self.pairs:
            self.value[r] = v
        assert self.value[again] == MR.value_of(again, 0, SHORT)
        # the hash file: names for the codes of some records, the others are not in it (g = "")
        codes = sorted({v[i:i + SS] for v in self.value.values() for i in range(0, len(v) - SS - 1, SS + 2)})[::3]
        codes = [c for c in codes if b"\n" not in c]
        self.hash_text = b"".join(b"sample-%d\t" % i + c + b"\n" for i, c in enumerate(codes)) + b"late\t" + codes[0] + b"\n"
        self.hash_map = {c: "sample-%d" % i for i, c in enumerate(codes)}
        self._want = {}

    def request(self, x, rt):
        r = self.Request()
        r.ParseFromString(bytes.fromhex(x["request"]))
        r.rt = rt
        return r.SerializeToString()

    def want(self, i, rt):
        """the two expected Replies of item i asked with return type rt; None where the golden is only a hash"""
        if (i, rt) not in self._want:
            x = self.items[i]
            self._want[(i, rt)] = [None if lst is None else
                                   meta_proto.all_reply(self.Reply, x["t"], rt, x["q"], strand == 1, lst, [self.value.get(r, b"") for r in lst],
                                                        self.hash_map, SS, OTHER)
                                   for strand, lst in enumerate(self.lists[i])]
        return self._want[(i, rt)]

    def check(self, i, rt, strand, got):
        x = self.items[i]
        want = self.want(i, rt)[strand]
        if want is not None:
            assert got == want, (x["t"], rt, x["q"][:30], strand, len(got), len(want))
            return
        m = self.Reply.FromString(got)
        assert (m.rt, m.t, m.q) == (x["t"], rt, x["q"]) and m.HasField("a")
        ms = m.a.revcomp_matches if strand else m.a.forward_matches
        assert len(m.a.forward_matches if strand else m.a.revcomp_matches) == 0
        as_reads = self.ReplyR()
        as_reads.rt, as_reads.t, as_reads.q = x["t"], 2, x["q"]
        as_reads.r.SetInParent()
        for y in ms:
            (as_reads.r.revcomp_matches if strand else as_reads.r.forward_matches).add().r = y.r
        assert _same(as_reads.SerializeToString(), x["replies"][strand]), (x["q"][:30], strand)  # the reference's reads, in its order
        for y in ms:
            assert [(s.g, s.c, s.l) for s in y.s] == meta_proto.records(self.value.get(y.r, b""), self.hash_map, SS, OTHER), y.r

    def empty(self, L, x, rt, strand):
        b = (C.c_uint8 * 512)()
        n = L.rsbwt_proto_encode_empty_reply(b, 512, x["t"], rt, x["q"].encode(), len(x["q"]), strand)
        assert 0 < n <= 512
        return bytes(b[:n])


@pytest.fixture(scope="module")
def gold(golden_dir):
    return Gold(golden_dir)


def test_the_pairs_leave_reads_out_and_hold_every_record_shape(gold):
    """(no GPU work: what the module's expectations rest on)"""
    assert len(gold.left_out) > 100 and len(gold.pairs) == len(gold.value) + 1
    lens = {len(v) for v in gold.value.values()}
    assert lens == set(SHORT)
    assert any(v[i] < 33 or v[i] > 127 for v in gold.value.values() for i in range(2, len(v) - 1, 4))
    recs = [r for v in list(gold.value.values())[:2000] for r in meta_proto.records(v, gold.hash_map, SS, OTHER)]
    assert any(g == "" for g, _, _ in recs) and any(g for g, _, _ in recs) and any(c < 0 for _, c, _ in recs)
    assert sum(lst is None for per in gold.lists for lst in per) == 16  # 8 items kept as hashes: checked by taking the Reply apart


def _open_service(rsb, gold, tmp_path, partitions=1, per_partition=1, limit=0, meta=True, unserved=False, transport=None):
    L = rsb.lib()
    gs = [rsb.GpuBWT(gold.path, for_reads=True) for _ in range(partitions)]
    ss = rsb.ShardSet(gs)
    tr, svc = C.c_void_p(), C.c_void_p()
    if transport is None:
        assert L.rsbwt_transport_inproc(C.byref(tr)) == 0
    else:
        assert L.rsbwt_transport_zmq(*transport, C.byref(tr)) == 0, L.rsbwt_last_error()
    assert L.rsbwt_service_create(ss._s, tr, 2000, 64, per_partition, C.byref(svc)) == 0
    L.rsbwt_service_set_reads(svc, 1, gold.minl, gold.maxl)
    assert L.rsbwt_service_set_kmermatch(svc, 1) == 0
    if limit:
        assert L.rsbwt_service_set_max_match_reads(svc, limit) == 0
    L.rsbwt_service_set_unserved(svc, 1 if unserved else 0)
    if meta:
        st = ss.meta_build([r for r, _ in gold.pairs], [v for _, v in gold.pairs])
        assert st["matched"] == len(gold.pairs) and st["unmatched"] == 0
        hf = tmp_path / "hash.txt"
        hf.write_bytes(gold.hash_text)
        assert L.rsbwt_service_set_all(svc, 1, str(hf).encode(), SS, 1 if OTHER else 0) == 0, L.rsbwt_last_error()
    return L, gs, ss, tr, svc


def _close_service(L, gs, ss, tr, svc):
    L.rsbwt_service_free(svc)
    L.rsbwt_transport_free(tr)
    ss.close()
    for g in gs:
        g.close()


@pytest.fixture(autouse=True)
def _path(gold, fixture_bwt):
    gold.path = fixture_bwt[0]


def _push(L, tr, msgs):
    for w in msgs:
        buf = (C.c_uint8 * len(w)).from_buffer_copy(w)
        assert L.rsbwt_transport_push_request(tr, buf, len(w)) == 0


@pytest.mark.parametrize("rt", [3, 4])
@pytest.mark.parametrize("partitions", [1, 2])
def test_gpu_service_all_golden_replies(rsb, gold, tmp_path, rt, partitions):
    """in process; one partition, and the same fixture held as two partitions (each partition sends what a reference service
    holding it sends: the golden Replies once per partition, forward then reverse complement); All and Samples"""
    L, gs, ss, tr, svc = _open_service(rsb, gold, tmp_path, partitions=partitions)
    try:
        assert L.rsbwt_service_start(svc) == 0
        _push(L, tr, [gold.request(x, rt) for x in gold.items])
        buf = (C.c_uint8 * BUF)()
        n = C.c_size_t()
        for i, x in enumerate(gold.items):
            for p in range(partitions):
                for strand in (0, 1):
                    assert L.rsbwt_transport_pop_reply(tr, 0, buf, BUF, C.byref(n), 120_000_000) == 0, (x["q"][:30], p, strand)
                    gold.check(i, rt, strand, bytes(buf[:n.value]))
        L.rsbwt_transport_close(tr)
        assert L.rsbwt_service_stop(svc) == 0
        assert L.rsbwt_transport_pop_reply(tr, 0, buf, BUF, C.byref(n), 1000) != 0  # exactly two per partition, no more
        assert L.rsbwt_transport_pop_reply(tr, 1, buf, BUF, C.byref(n), 1000) != 0
        assert L.rsbwt_service_all_requests(svc) == len(gold.items)
        assert L.rsbwt_service_read_requests(svc) == 0 and L.rsbwt_service_kmer_requests(svc) == 0
    finally:
        _close_service(L, gs, ss, tr, svc)


def test_gpu_service_all_summed_replies(rsb, gold, tmp_path):
    """replies = "summed" over two partitions: one Reply per strand, the partitions' lists joined in shard order -- every
    read twice in a row of partitions, each with its samples"""
    L, gs, ss, tr, svc = _open_service(rsb, gold, tmp_path, partitions=2, per_partition=0)
    try:
        assert L.rsbwt_service_start(svc) == 0
        pick = [i for i, x in enumerate(gold.items) if max(x["reads"]) < 300 and None not in gold.lists[i]][::3]
        _push(L, tr, [gold.request(gold.items[i], 3) for i in pick])
        buf = (C.c_uint8 * BUF)()
        n = C.c_size_t()
        for i in pick:
            x = gold.items[i]
            for strand, lst in enumerate(gold.lists[i]):
                assert L.rsbwt_transport_pop_reply(tr, 0, buf, BUF, C.byref(n), 120_000_000) == 0
                want = meta_proto.all_reply(gold.Reply, x["t"], 3, x["q"], strand == 1, lst + lst, [gold.value.get(r, b"") for r in lst + lst],
                                            gold.hash_map, SS, OTHER)
                assert bytes(buf[:n.value]) == want, (x["q"][:30], strand)
        L.rsbwt_transport_close(tr)
        assert L.rsbwt_service_stop(svc) == 0
    finally:
        _close_service(L, gs, ss, tr, svc)


def test_gpu_service_all_with_max_match_reads(rsb, gold, tmp_path):
    """max_match_reads = 5,000 cuts the strands of the three 5-symbol queries (7,428 to 8,484 rows each): those get the empty
    Reply, every other request of the window its golden one"""
    LIMIT = 5000
    cut = [(i, s) for i, x in enumerate(gold.items) for s in (0, 1) if x["t"] == 2 and x["reads"][s] > LIMIT]
    assert len(cut) >= 2 and all(len(gold.items[i]["q"]) < gold.minl for i, _ in cut)
    L, gs, ss, tr, svc = _open_service(rsb, gold, tmp_path, limit=LIMIT)
    try:
        assert L.rsbwt_service_start(svc) == 0
        mine = [i for i, x in enumerate(gold.items) if x["t"] == 2]
        _push(L, tr, [gold.request(gold.items[i], 3) for i in mine])
        buf = (C.c_uint8 * BUF)()
        n = C.c_size_t()
        for i in mine:
            for strand in (0, 1):
                assert L.rsbwt_transport_pop_reply(tr, 0, buf, BUF, C.byref(n), 120_000_000) == 0
                if (i, strand) in cut:
                    assert bytes(buf[:n.value]) == gold.empty(L, gold.items[i], 3, strand), (i, strand)
                else:
                    gold.check(i, 3, strand, bytes(buf[:n.value]))
        L.rsbwt_transport_close(tr)
        assert L.rsbwt_service_stop(svc) == 0
        assert L.rsbwt_service_capped_requests(svc) == len({i for i, _ in cut})
    finally:
        _close_service(L, gs, ss, tr, svc)


def test_gpu_service_without_meta_answers_as_before(rsb, gold, tmp_path):
    """no table configured: the golden file's `unserved` Requests get exactly the Replies recorded there (unserved = "empty"),
    the rewritten Requests the empty Reply of their type -- and with unserved off, no Reply at all"""
    for unserved in (True, False):
        L, gs, ss, tr, svc = _open_service(rsb, gold, tmp_path, meta=False, unserved=unserved)
        try:
            assert L.rsbwt_service_start(svc) == 0
            some = gold.items[::9]
            _push(L, tr, [bytes.fromhex(x["request"]) for x in gold.unserved] + [gold.request(x, rt) for x in some for rt in (3, 4)])
            L.rsbwt_transport_close(tr)
            assert L.rsbwt_service_stop(svc) == 0
            buf = (C.c_uint8 * BUF)()
            n = C.c_size_t()
            if unserved:
                for x in gold.unserved:
                    for j, want in enumerate(x["replies"]):
                        assert L.rsbwt_transport_pop_reply(tr, 0, buf, BUF, C.byref(n), 1_000_000) == 0
                        assert _same(bytes(buf[:n.value]), want), (x["t"], x["rt"], j)
                for x in some:
                    for rt in (3, 4):
                        for strand in (0, 1):
                            assert L.rsbwt_transport_pop_reply(tr, 0, buf, BUF, C.byref(n), 1_000_000) == 0
                            assert bytes(buf[:n.value]) == gold.empty(L, x, rt, strand)
            assert L.rsbwt_transport_pop_reply(tr, 0, buf, BUF, C.byref(n), 1000) != 0
            assert L.rsbwt_service_all_requests(svc) == 0
        finally:
            _close_service(L, gs, ss, tr, svc)


def test_gpu_service_set_all_refusals(rsb, gold, tmp_path):
    """a set without a table, a shard not opened for reads, a hash file that cannot be read"""
    L = rsb.lib()
    for for_reads, build in ((True, False), (False, True)):
        g = rsb.GpuBWT(gold.path, for_reads=for_reads)
        ss = rsb.ShardSet([g])
        tr, svc = C.c_void_p(), C.c_void_p()
        try:
            assert L.rsbwt_transport_inproc(C.byref(tr)) == 0
            assert L.rsbwt_service_create(ss._s, tr, 200, 16, 1, C.byref(svc)) == 0
            if build:
                ss.meta_build([r for r, _ in gold.pairs[:50]], [v for _, v in gold.pairs[:50]])
            assert L.rsbwt_service_set_all(svc, 1, None, SS, 1) == -1
            assert (b"RSBWT_OPEN_READS" if build else b"sample table") in L.rsbwt_last_error()
            assert L.rsbwt_service_set_all(svc, 0, None, SS, 1) == 0
        finally:
            _close_service(L, [g], ss, tr, svc)
    L, gs, ss, tr, svc = _open_service(rsb, gold, tmp_path)
    try:
        assert L.rsbwt_service_set_all(svc, 1, str(tmp_path / "missing").encode(), SS, 1) == -2
        assert L.rsbwt_service_set_all(svc, 1, None, 0, 0) == -1
        assert L.rsbwt_service_set_all(svc, 1, None, SS, 1) == 0  # no hash file: every g is ""
    finally:
        _close_service(L, gs, ss, tr, svc)


def test_gpu_service_all_over_real_zeromq_sockets(rsb, gold, tmp_path):
    """every fourth Request over real sockets (the front-end's PUB and two PULLs bound here, the service's SUB / PUSH / PUSH
    connected through libzmq bound at run time).  Skipped only where no libzmq exists."""
    import time
    from test_service_slice import _libzmq
    z = _libzmq()
    if z is None or not rsb.lib().rsbwt_zmq_available():
        pytest.skip("no libzmq on this box")
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
    L, gs, ss, tr, svc = _open_service(rsb, gold, tmp_path, transport=eps)
    try:
        assert L.rsbwt_service_start(svc) == 0
        buf = C.create_string_buffer(BUF)
        # PUB/SUB drops what is published before the subscription has arrived: wait for a probe to be answered
        probe = gold.request(gold.items[0], 3)
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
        pick = list(range(0, len(gold.items), 4))
        for i in pick:
            w = gold.request(gold.items[i], 3 + i % 2)
            assert z.zmq_send(pub, w, len(w), 0) == len(w)
        for i in pick:
            for strand in (0, 1):
                n = z.zmq_recv(pull, buf, BUF, 0)
                assert 0 <= n <= BUF, "a reply is missing"
                gold.check(i, 3 + i % 2, strand, buf.raw[:n])
        tmo = C.c_int(300)
        z.zmq_setsockopt(pull, ZMQ_RCVTIMEO, C.byref(tmo), 4)
        z.zmq_setsockopt(pull_count, ZMQ_RCVTIMEO, C.byref(tmo), 4)
        assert z.zmq_recv(pull, buf, BUF, 0) < 0  # exactly two per request, no more
        assert z.zmq_recv(pull_count, buf, BUF, 0) < 0
        L.rsbwt_transport_close(tr)
        assert L.rsbwt_service_stop(svc) == 0
    finally:
        _close_service(L, gs, ss, tr, svc)
        for so in socks:
            z.zmq_close(so)
        z.zmq_ctx_term(ctx)
