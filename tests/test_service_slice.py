"""f1, the service slice: the proto2 codec against the Python protobuf runtime (CPU), and the
batched count_reads against the oracle (GPU)."""
import ctypes as C
import os

import numpy as np
import pytest

import proto_schema


@pytest.fixture(scope="module")
def pb():
    return proto_schema.build()


def _rc(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def test_codec_matches_protobuf_runtime(rsb, pb):
    Request, Reply = pb
    L = rsb.lib()
    rng = np.random.default_rng(0)
    for _ in range(300):
        r = Request()
        r.t = int(rng.integers(1, 5))
        r.rt = int(rng.integers(1, 5))
        r.q = "".join("ACGTN"[x] for x in rng.integers(0, 5, int(rng.integers(0, 320))))
        if rng.random() < 0.5:
            r.k, r.s, r.p = 31, int(rng.integers(0, 9)), int(rng.integers(-5, 500))
            r.a, r.isalt = "ACGT", 1
        wire = r.SerializeToString()
        t, rt, q, ql = C.c_int(), C.c_int(), C.c_char_p(), C.c_size_t()
        buf = (C.c_uint8 * len(wire)).from_buffer_copy(wire)
        assert L.rsbwt_proto_decode_request(buf, len(wire), C.byref(t), C.byref(rt), C.byref(q), C.byref(ql)) == 0
        got_q = C.string_at(C.cast(q, C.c_void_p).value, ql.value).decode() if ql.value else ""
        assert (t.value, rt.value, got_q) == (r.t, r.rt, r.q)
        for revcomp in (0, 1):
            for c in (0, 1, 127, 128, 300000, 2 ** 31 - 1, -1, -(2 ** 31)):
                rep = Reply()
                rep.rt, rep.t, rep.q = r.t, 1, r.q
                (rep.c.revcomp_matches if revcomp else rep.c.forward_matches).c = c
                exp = rep.SerializeToString()
                out = (C.c_uint8 * (len(exp) + 16))()
                n = L.rsbwt_proto_encode_count_reply(out, len(out), r.t, r.q.encode(), len(r.q), revcomp, c)
                assert bytes(out[:n]) == exp
    # ReplyReads (readserver.proto:35-37,61-64): none, one, many reads, either strand; `r` present even when empty
    for nreads in (0, 1, 2, 300):
        reads = ["".join("ACGT"[x] for x in rng.integers(0, 4, int(rng.integers(0, 200)))) for _ in range(nreads)]
        for revcomp in (0, 1):
            q = "ACGTTGCA" * int(rng.integers(0, 20))
            rep = Reply()
            rep.rt, rep.t, rep.q = 2, 2, q
            rep.r.SetInParent()
            for x in reads:
                (rep.r.revcomp_matches if revcomp else rep.r.forward_matches).add().r = x
            exp = rep.SerializeToString()
            arr = (C.c_char_p * max(nreads, 1))(*[x.encode() for x in reads])
            lens = (C.c_size_t * max(nreads, 1))(*[len(x) for x in reads])
            need = L.rsbwt_proto_encode_reads_reply(None, 0, 2, q.encode(), len(q), revcomp, arr, lens, nreads)
            assert need == len(exp)
            out = (C.c_uint8 * need)()
            assert L.rsbwt_proto_encode_reads_reply(out, need, 2, q.encode(), len(q), revcomp, arr, lens, nreads) == need
            assert bytes(out) == exp
    # a message missing a required field, and a truncated one, are rejected
    bad = Request(); bad.t = 1; bad.rt = 1
    wire = bad.SerializePartialToString()
    buf = (C.c_uint8 * max(len(wire), 1)).from_buffer_copy(wire or b"\0")
    assert L.rsbwt_proto_decode_request(buf, len(wire), None, None, None, None) == -3
    ok = Request(); ok.t, ok.rt, ok.q = 1, 1, "ACGT"
    wire = ok.SerializeToString()[:-2]
    buf = (C.c_uint8 * len(wire)).from_buffer_copy(wire)
    assert L.rsbwt_proto_decode_request(buf, len(wire), None, None, None, None) == -3


@pytest.mark.gpu
def test_gpu_service_counts_batch(rsb, oracle, pb, tmp_path):
    Request, Reply = pb
    L = rsb.lib()
    kw = dict(seed=23, genome_len=20000, haplotypes=4, snp_rate=0.004, read_len=60, coverage=3.0)
    shards, oixs = [], []
    for s in range(2):
        p = str(tmp_path / f"s{s}.bwt")
        rsb.synth_popbwt(p, None, shard=s, num_shards=2, **kw)
        shards.append(rsb.GpuBWT(p))
        oixs.append(oracle.load(p))
    rd = str(tmp_path / "w.reads")
    rsb.synth_popbwt(str(tmp_path / "w.bwt"), rd, **kw)
    reads = open(rd).read().split()
    rng = np.random.default_rng(3)
    reqs = []
    for i in range(400):
        r = Request()
        kind = i % 5
        r.t, r.rt = (1, 1) if kind < 2 else (2, 1) if kind == 2 else (2, 2) if kind == 3 else (3, 1)
        rr = reads[rng.integers(len(reads))]
        k = int(rng.choice([20, 31, 31, 37, 60]))
        st = int(rng.integers(0, len(rr) - k + 1))
        q = rr[st:st + k]
        if i % 7 == 0:
            q = _rc(q)
        if i % 31 == 0:
            q = q[:5] + "N" + q[6:]
        if i == 13:
            q = ""
        r.q = q
        reqs.append(r)
    wires = [r.SerializeToString() for r in reqs]
    off = np.concatenate([[0], np.cumsum([len(w) for w in wires])]).astype(np.uint64)
    blob = np.frombuffer(b"".join(wires), np.uint8).copy()
    ss = rsb.ShardSet(shards)
    rep_off = np.zeros(2 * len(reqs) + 1, np.uint64)
    need = C.c_size_t()
    rc = L.rsbwt_service_counts(ss._s, blob.ctypes.data, blob.size, off.ctypes.data, len(reqs), None, 0,
                                rep_off.ctypes.data, C.byref(need))
    assert rc == -7 and need.value > 0
    out = np.zeros(need.value, np.uint8)
    assert L.rsbwt_service_counts(ss._s, blob.ctypes.data, blob.size, off.ctypes.data, len(reqs), out.ctypes.data,
                                  out.size, rep_off.ctypes.data, C.byref(need)) == 0
    # offsets that are not an ascending range inside the buffer are refused, with a message of their own
    bad_off = off.copy()
    bad_off[3], bad_off[4] = bad_off[4], bad_off[3]
    assert L.rsbwt_service_counts(ss._s, blob.ctypes.data, blob.size, bad_off.ctypes.data, len(reqs), out.ctypes.data,
                                  out.size, rep_off.ctypes.data, C.byref(need)) == -1
    assert b"ascending" in L.rsbwt_last_error()
    assert L.rsbwt_service_counts(ss._s, blob.ctypes.data, blob.size - 1, off.ctypes.data, len(reqs), out.ctypes.data,
                                  out.size, rep_off.ctypes.data, C.byref(need)) == -1
    for i, r in enumerate(reqs):
        f = out[int(rep_off[2 * i]):int(rep_off[2 * i + 1])].tobytes()
        v = out[int(rep_off[2 * i + 1]):int(rep_off[2 * i + 2])].tobytes()
        if not (r.t == 1 or (r.t == 2 and r.rt == 1)):
            assert f == b"" and v == b""
            continue
        fm, vm = Reply(), Reply()
        fm.ParseFromString(f); vm.ParseFromString(v)
        assert (fm.rt, fm.t, fm.q) == (r.t, 1, r.q) and (vm.rt, vm.t, vm.q) == (r.t, 1, r.q)
        assert fm.c.HasField("forward_matches") and not fm.c.HasField("revcomp_matches")
        assert vm.c.HasField("revcomp_matches") and not vm.c.HasField("forward_matches")

        def count(w):  # count_reads, service.cpp:299-304, summed over partitions
            if not w or any(ch not in "ACGT" for ch in w):
                return 0
            tot = 0
            for ox in oixs:
                lo, up = ox.find_interval(w)
                tot += up - lo + 1 if up >= lo else 0
            return tot
        assert fm.c.forward_matches.c == count(r.q)
        assert vm.c.revcomp_matches.c == count(_rc(r.q))
    ss.close()
    for g in shards:
        g.close()


# ---- service.cfg reader (CPU) -----------------------------------------------------------------------

CFG = '''// prefix for bwt file (path before .bwt extension)
prefix = "/data/SERVER/bwt/final"
# a hash comment
hashfile = "/data/SERVER/files/list_of_sample_hash";
pull = "tcp://10.0.0.1:5557";
push = "tcp://10.0.0.1:5558";
push_count = "tcp://10.0.0.1:5559";
/* the common suffix
   (read from backward) */
suffix = "";
size_of_sample = "1";
has_other_meta_data = "0";
max_read_length = "100"; min_read_length = "100";
rocksdb_path = "/data/SERVER/" "rocksdbs/"
rocksdb_ext = ".rocksdb";
rocksdb = [
    "CGA",
    "CGC", "AAA"
];
shards = [ "/data/s0", "/data/s1" ];
batch_window_us = "350";
'''


def test_service_config_reader(rsb, tmp_path):
    L = rsb.lib()
    p = tmp_path / "service.cfg"
    p.write_text(CFG)
    h = C.c_void_p()
    assert L.rsbwt_service_config_load(str(p).encode(), C.byref(h)) == 0
    get = lambda k: L.rsbwt_service_config_get(h, k.encode())
    assert get("prefix") == b"/data/SERVER/bwt/final" and get("suffix") == b"" and get("pull") == b"tcp://10.0.0.1:5557"
    assert get("push_count") == b"tcp://10.0.0.1:5559" and get("max_read_length") == b"100"
    assert get("rocksdb_path") == b"/data/SERVER/rocksdbs/"  # adjacent strings concatenate, as in libconfig
    assert get("batch_window_us") == b"350" and get("nope") is None
    assert L.rsbwt_service_config_array_len(h, b"rocksdb") == 3
    assert [L.rsbwt_service_config_array_item(h, b"rocksdb", i) for i in range(3)] == [b"CGA", b"CGC", b"AAA"]
    assert L.rsbwt_service_config_array_item(h, b"shards", 1) == b"/data/s1"
    assert L.rsbwt_service_config_array_item(h, b"rocksdb", 3) is None
    L.rsbwt_service_config_free(h)
    # a setting the reference looks up unconditionally is missing (SettingNotFoundException, service.cpp:1438-1442)
    q = tmp_path / "short.cfg"
    q.write_text(CFG.replace('push_count = "tcp://10.0.0.1:5559";', ""))
    assert L.rsbwt_service_config_load(str(q).encode(), C.byref(h)) == -3 and b"push_count" in L.rsbwt_last_error()
    q.write_text('prefix = "a"\nsuffix = nope;')
    assert L.rsbwt_service_config_load(str(q).encode(), C.byref(h)) == -3 and b"line 2" in L.rsbwt_last_error()
    assert L.rsbwt_service_config_load(str(tmp_path / "missing.cfg").encode(), C.byref(h)) == -2
    # the reference's own template parses (its demo/TEMPLATE.service.cfg, kept as a fixture)
    tpl = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "service_template.cfg")
    assert L.rsbwt_service_config_load(tpl.encode(), C.byref(h)) == 0
    assert L.rsbwt_service_config_array_len(h, b"rocksdb") == 64 and L.rsbwt_service_config_get(h, b"suffix") == b""
    L.rsbwt_service_config_free(h)


def _libzmq():
    """libzmq for the TEST's side of the sockets (the front-end's: PUB + two PULLs), by ctypes; None when the box
    has none.  The library binds its own copy at run time (rsbwt_zmq_available)."""
    import ctypes.util
    import glob
    cands = [os.environ.get("RSBWT_LIBZMQ"), ctypes.util.find_library("zmq"), "libzmq.so.5"]
    cands += sorted(glob.glob("/usr/local/lib/libzmq.so.5")) + sorted(glob.glob("/opt/conda/lib/libzmq.so.5"))
    for c in cands:
        if not c:
            continue
        try:
            z = C.CDLL(c)
        except OSError:
            continue
        z.zmq_ctx_new.restype = C.c_void_p
        z.zmq_socket.restype = C.c_void_p
        z.zmq_socket.argtypes = [C.c_void_p, C.c_int]
        for f in ("zmq_bind", "zmq_connect"):
            getattr(z, f).argtypes = [C.c_void_p, C.c_char_p]
        z.zmq_setsockopt.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]
        z.zmq_getsockopt.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_size_t)]
        z.zmq_send.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        z.zmq_recv.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        z.zmq_close.argtypes = [C.c_void_p]
        z.zmq_ctx_term.argtypes = [C.c_void_p]
        return z
    return None


def test_zmq_is_bound_at_run_time_or_reported_absent(rsb):
    """The ZeroMQ transport needs no rebuild: where a libzmq can be loaded the sockets are created and
    connected (connecting is asynchronous: no peer is needed), elsewhere the call says RSBWT_ENODEV and names
    libzmq -- never a stand-in."""
    L = rsb.lib()
    h = C.c_void_p()
    rc = L.rsbwt_transport_zmq(b"tcp://127.0.0.1:45001", b"tcp://127.0.0.1:45002", b"tcp://127.0.0.1:45003", C.byref(h))
    if L.rsbwt_zmq_available():
        assert rc == 0 and h.value
        L.rsbwt_transport_close(h)
        L.rsbwt_transport_free(h)
        assert L.rsbwt_transport_zmq(b"not-an-endpoint", b"tcp://127.0.0.1:2", b"tcp://127.0.0.1:3", C.byref(h)) == -2
        assert b"not-an-endpoint" in L.rsbwt_last_error()
    else:
        assert rc == -5 and b"libzmq" in L.rsbwt_last_error() and not h.value
    if _libzmq() is not None and not os.environ.get("RSBWT_LIBZMQ"):
        assert L.rsbwt_zmq_available() == 1, "a libzmq the test can load must be one the library can bind"


# ---- the recv loop with its micro-batch window (GPU) ------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("window_us,max_batch", [(5000, 4096), (0, 1), (300, 7)])
def test_gpu_service_loop_golden_replies(rsb, fixture_bwt, golden_dir, window_us, max_batch):
    """A mixed stream of serialised Requests pushed through the loop (in-process transport) with one
    partition = the golden fixture: the replies must be, byte for byte and in order, what a reference
    service process sends (tests/golden/service_v1.json: bytes from the protobuf runtime, counts from
    the compiled reference); CountReads on push_count, ExactMatch-Count on push; other request types
    go to the handler (here the ExactMatch-Reads requests too: rsbwt_service_set_reads(0), the loop as it was until
    round 5 -- test_gpu_service_loop_reads_golden_replies has them answered); a malformed message is dropped and counted."""
    import json
    import os
    import threading
    L = rsb.lib()
    gold = json.load(open(os.path.join(golden_dir, "service_v1.json")))["items"]
    path, _ = fixture_bwt
    g = rsb.GpuBWT(path)
    ss = rsb.ShardSet([g])
    tr, svc = C.c_void_p(), C.c_void_p()
    assert L.rsbwt_transport_inproc(C.byref(tr)) == 0
    assert L.rsbwt_service_create(ss._s, tr, window_us, max_batch, 1, C.byref(svc)) == 0
    L.rsbwt_service_set_reads(svc, 0, 0, 0)
    others = []
    CB = C.CFUNCTYPE(None, C.c_void_p, C.POINTER(C.c_uint8), C.c_size_t)
    cb = CB(lambda arg, p, n: others.append(bytes(p[:n])))
    L.rsbwt_service_set_other_handler(svc, C.cast(cb, C.c_void_p), None)
    assert L.rsbwt_service_start(svc) == 0
    wires = [bytes.fromhex(x["request"]) for x in gold]

    def feed():
        for i, w in enumerate(wires):
            buf = (C.c_uint8 * max(len(w), 1)).from_buffer_copy(w or b"\\0")
            assert L.rsbwt_transport_push_request(tr, buf, len(w)) == 0
            if i == 100:
                junk = (C.c_uint8 * 3)(0xFF, 0xFF, 0x01)
                L.rsbwt_transport_push_request(tr, junk, 3)
    th = threading.Thread(target=feed)
    th.start()
    want = {0: [], 1: []}
    for x in gold:
        if x["replies"]:
            want[x["channel"]] += [bytes.fromhex(r) for r in x["replies"]]
    got = {0: [], 1: []}
    buf = (C.c_uint8 * 4096)()
    n = C.c_size_t()
    for ch in (1, 0):
        for _ in want[ch]:
            assert L.rsbwt_transport_pop_reply(tr, ch, buf, 4096, C.byref(n), 20_000_000) == 0
            got[ch].append(bytes(buf[:n.value]))
    th.join()
    L.rsbwt_transport_close(tr)
    assert L.rsbwt_service_stop(svc) == 0
    assert got[1] == want[1] and got[0] == want[0]
    assert L.rsbwt_transport_pop_reply(tr, 0, buf, 4096, C.byref(n), 1000) == -2  # exactly two per request, no more
    st = (C.c_uint64 * 6)()
    L.rsbwt_service_stats(svc, st)
    assert st[0] == len(gold) + 1 and st[1] == sum(1 for x in gold if x["replies"]) and st[4] == 1
    assert st[3] == len(want[0]) + len(want[1]) and 1 <= st[5] <= max_batch
    if max_batch == 1:
        assert st[2] == st[0]
    assert sorted(others) == sorted(bytes.fromhex(x["request"]) for x in gold if not x["replies"])
    L.rsbwt_service_free(svc)
    L.rsbwt_transport_free(tr)
    ss.close()
    g.close()


@pytest.mark.gpu
def test_gpu_service_loop_many_partitions(rsb, oracle, pb, tmp_path):
    """One process impersonating P partitions: per_partition = 1 sends 2 x P replies per request, reply
    (s, strand) carrying shard s's own count; per_partition = 0 sends 2 with the counts summed."""
    Request, Reply = pb
    L = rsb.lib()
    kw = dict(seed=29, genome_len=20000, haplotypes=4, snp_rate=0.004, read_len=60, coverage=3.0)
    shards, oixs = [], []
    for s in range(4):
        p = str(tmp_path / f"s{s}.bwt")
        rsb.synth_popbwt(p, None, shard=s, num_shards=4, **kw)
        shards.append(rsb.GpuBWT(p))
        oixs.append(oracle.load(p))
    rd = str(tmp_path / "w.reads")
    rsb.synth_popbwt(str(tmp_path / "w.bwt"), rd, **kw)
    reads = open(rd).read().split()
    rng = np.random.default_rng(5)
    reqs = []
    for i in range(300):
        r = Request()
        r.t, r.rt = (1, 1) if i % 2 else (2, 1)
        rr = reads[rng.integers(len(reads))]
        k = int(rng.choice([25, 31, 40]))
        st = int(rng.integers(0, len(rr) - k + 1))
        r.q = rr[st:st + k]
        reqs.append(r)
    ss = rsb.ShardSet(shards)

    def count(ox, w):
        lo, up = ox.find_interval(w)
        return up - lo + 1 if up >= lo else 0
    for per_partition in (1, 0):
        tr, svc = C.c_void_p(), C.c_void_p()
        assert L.rsbwt_transport_inproc(C.byref(tr)) == 0
        assert L.rsbwt_service_create(ss._s, tr, 2000, 128, per_partition, C.byref(svc)) == 0
        for r in reqs:
            w = r.SerializeToString()
            buf = (C.c_uint8 * len(w)).from_buffer_copy(w)
            assert L.rsbwt_transport_push_request(tr, buf, len(w)) == 0
        L.rsbwt_transport_close(tr)
        assert L.rsbwt_service_run(svc) == 0  # returns once everything pushed is answered
        buf = (C.c_uint8 * 4096)()
        n = C.c_size_t()
        for r in reqs:
            ch = 1 if r.t == 1 else 0
            rows = len(shards) if per_partition else 1
            for s in range(rows):
                for strand in (0, 1):
                    assert L.rsbwt_transport_pop_reply(tr, ch, buf, 4096, C.byref(n), 1_000_000) == 0
                    m = Reply()
                    m.ParseFromString(bytes(buf[:n.value]))
                    assert (m.rt, m.t, m.q) == (r.t, 1, r.q)
                    w = _rc(r.q) if strand else r.q
                    exp = count(oixs[s], w) if per_partition else sum(count(ox, w) for ox in oixs)
                    c = m.c.revcomp_matches.c if strand else m.c.forward_matches.c
                    assert c == exp and m.c.HasField("revcomp_matches" if strand else "forward_matches")
        assert L.rsbwt_transport_pop_reply(tr, 0, buf, 4096, C.byref(n), 1000) == -2
        assert L.rsbwt_transport_pop_reply(tr, 1, buf, 4096, C.byref(n), 1000) == -2
        L.rsbwt_service_free(svc)
        L.rsbwt_transport_free(tr)
    ss.close()
    for g in shards:
        g.close()


@pytest.mark.gpu
def test_gpu_service_over_real_zeromq_sockets_golden_replies(rsb, pb, fixture_bwt, golden_dir):
    """The drop-in claim on real sockets (src/service/service.cpp:1493-1502,1521-1577): this test plays the
    front-end -- binds a PUB socket (server.cpp:124) and two PULL sockets (server.cpp:118-120) -- the service
    connects SUB / PUSH / PUSH to them through libzmq bound at run time, and the golden Request bytes must come
    back as the golden Reply bytes, in order per socket: the counts (service_v1.json) and, since round 5, the read
    lists of the ExactMatch-Reads requests (service_reads_v1.json), some of them hundreds of kilobytes long.
    Skipped only where no libzmq exists."""
    import json
    import time
    z = _libzmq()
    L = rsb.lib()
    if z is None or not L.rsbwt_zmq_available():
        pytest.skip("no libzmq on this box")
    ZMQ_PUB, ZMQ_PULL, ZMQ_LINGER, ZMQ_RCVTIMEO, ZMQ_LAST_ENDPOINT = 1, 7, 17, 27, 32
    ctx = z.zmq_ctx_new()
    socks, eps = [], []
    for typ in (ZMQ_PUB, ZMQ_PULL, ZMQ_PULL):
        so = z.zmq_socket(ctx, typ)
        zero, tmo = C.c_int(0), C.c_int(20000)
        z.zmq_setsockopt(so, ZMQ_LINGER, C.byref(zero), 4)
        z.zmq_setsockopt(so, ZMQ_RCVTIMEO, C.byref(tmo), 4)
        assert z.zmq_bind(so, b"tcp://127.0.0.1:*") == 0
        ep = C.create_string_buffer(256)
        n = C.c_size_t(256)
        assert z.zmq_getsockopt(so, ZMQ_LAST_ENDPOINT, ep, C.byref(n)) == 0
        socks.append(so)
        eps.append(ep.value)
    pub, pull, pull_count = socks
    gold = json.load(open(os.path.join(golden_dir, "service_v1.json")))["items"]
    gr = json.load(open(os.path.join(golden_dir, "service_reads_v1.json")))
    by_req = {x["request"]: x for x in gr["items"]}
    gold = gold + gr["items"][::3]  # (a third of the read requests: the rest run through the in-process transport)
    path, _ = fixture_bwt
    g = rsb.GpuBWT(path, for_reads=True)
    ss = rsb.ShardSet([g])
    tr, svc = C.c_void_p(), C.c_void_p()
    assert L.rsbwt_transport_zmq(eps[0], eps[1], eps[2], C.byref(tr)) == 0, L.rsbwt_last_error()
    assert L.rsbwt_service_create(ss._s, tr, 2000, 512, 1, C.byref(svc)) == 0
    L.rsbwt_service_set_reads(svc, 1, gr["min_read_length"], gr["max_read_length"])
    assert L.rsbwt_service_start(svc) == 0
    BUF = 4 << 20
    buf = C.create_string_buffer(BUF)
    # PUB/SUB drops what is published before the subscription has arrived: wait for a probe to be answered
    probe = bytes.fromhex(next(x for x in gold if x["replies"] and x["channel"] == 1)["request"])
    t0 = time.time()
    up = False
    while not up and time.time() - t0 < 20:
        z.zmq_send(pub, probe, len(probe), 0)
        tmo = C.c_int(200)
        z.zmq_setsockopt(pull_count, ZMQ_RCVTIMEO, C.byref(tmo), 4)
        up = z.zmq_recv(pull_count, buf, BUF, 0) >= 0
    assert up, "the service never subscribed"
    time.sleep(0.3)
    tmo = C.c_int(300)
    for so in (pull, pull_count):  # whatever other probes produced
        z.zmq_setsockopt(so, ZMQ_RCVTIMEO, C.byref(tmo), 4)
        while z.zmq_recv(so, buf, BUF, 0) >= 0:
            pass
    tmo = C.c_int(20000)
    for so in (pull, pull_count):
        z.zmq_setsockopt(so, ZMQ_RCVTIMEO, C.byref(tmo), 4)
    want = {0: [], 1: []}
    for x in gold:
        w = bytes.fromhex(x["request"])
        assert z.zmq_send(pub, w, len(w), 0) == len(w)
        if x["t"] == 2 and x["rt"] == 2:
            want[0] += by_req[x["request"]]["replies"] if x["request"] in by_req else _empty_reads_replies(pb, x["q"])
        elif x["replies"]:
            want[x["channel"]] += [bytes.fromhex(r) for r in x["replies"]]
    for ch, so in ((1, pull_count), (0, pull)):
        for j, w in enumerate(want[ch]):
            n = z.zmq_recv(so, buf, BUF, 0)
            assert 0 <= n <= BUF, "a reply is missing"
            assert _same(buf.raw[:n], w), (ch, j, n)
    assert any(isinstance(w, dict) and w["len"] > 100000 for w in want[0])  # (a read list of hundreds of kilobytes went over the socket)
    tmo = C.c_int(300)
    z.zmq_setsockopt(pull, ZMQ_RCVTIMEO, C.byref(tmo), 4)
    assert z.zmq_recv(pull, buf, BUF, 0) < 0  # exactly two per request, no more
    L.rsbwt_transport_close(tr)
    assert L.rsbwt_service_stop(svc) == 0
    L.rsbwt_service_free(svc)
    L.rsbwt_transport_free(tr)
    for so in socks:
        z.zmq_close(so)
    z.zmq_ctx_term(ctx)
    ss.close()
    g.close()


def _empty_reads_replies(pb, q):
    """What this service sends for a Reads request it answers with no read: both strands, `r` present and empty."""
    _, Reply = pb
    out = []
    for _strand in (0, 1):
        rep = Reply()
        rep.rt, rep.t, rep.q = 2, 2, q
        rep.r.SetInParent()
        out.append(rep.SerializeToString())
    return out


def _same(got, want):
    """a reply against its golden form: the bytes, or (long replies) their length and SHA-256"""
    import hashlib
    if isinstance(want, dict):
        return len(got) == want["len"] and hashlib.sha256(got).hexdigest() == want["sha256"]
    return got == (bytes.fromhex(want) if isinstance(want, str) else want)


@pytest.mark.gpu
@pytest.mark.parametrize("window_us,max_batch,for_reads,repeat", [(5000, 4096, True, 1), (0, 1, False, 1), (300, 7, True, 1), (200, 16, True, 12)])
def test_gpu_service_loop_reads_golden_replies(rsb, pb, fixture_bwt, golden_dir, window_us, max_batch, for_reads, repeat):
    """J1: ExactMatch Requests whose return type is Reads, answered by the loop itself.  The stream is
    service_v1.json's (counts, other types, malformed) with service_reads_v1.json's woven in; one partition = the golden
    fixture, min / max read length 50 / 70 as in the golden file.  Every Reads request must come back on `push` as the
    two Reply messages a reference service sends (QueryTask::run + find_reads, service.cpp:714-797,1260-1291; the reads
    out of the compiled reference, tests/golden/make_service_reads_golden.py) -- byte for byte, in arrival order,
    between the count replies of the same socket; intervals of more than 4,097 rows in find_reads' chunked order; the
    tiles in the reference's container order.  A Reads request with a symbol outside ACGT or an empty query gets two
    replies with an empty list (this service's rule: include/rsbwt.h).  Shards opened for reads or not: same bytes.
    repeat = 12: the stream twelve times over in windows of 16 -- hundreds of windows on the loop's eight workers at once,
    each answering its mixed-length queries in one search and its reads in one fused extraction from threads of its own:
    every reply still byte for byte, in order."""
    import json
    import threading
    L = rsb.lib()
    v1 = json.load(open(os.path.join(golden_dir, "service_v1.json")))["items"]
    gr = json.load(open(os.path.join(golden_dir, "service_reads_v1.json")))
    by_req = {x["request"]: x for x in gr["items"]}
    stream = []
    extra = [x for x in gr["items"]]
    for i, x in enumerate(v1):
        stream.append(x)
        if i % 2 == 0 and extra:
            stream.append(extra.pop(0))
    stream += extra
    stream = stream * repeat
    path, _ = fixture_bwt
    g = rsb.GpuBWT(path, for_reads=for_reads)
    ss = rsb.ShardSet([g])
    tr, svc = C.c_void_p(), C.c_void_p()
    assert L.rsbwt_transport_inproc(C.byref(tr)) == 0
    assert L.rsbwt_service_create(ss._s, tr, window_us, max_batch, 1, C.byref(svc)) == 0
    L.rsbwt_service_set_reads(svc, 1, gr["min_read_length"], gr["max_read_length"])
    suf = (C.c_char_p * 1)(gr["suffix"].encode())
    assert L.rsbwt_service_set_suffixes(svc, suf, 1) == 0
    assert L.rsbwt_service_set_suffixes(svc, suf, 2) == -1  # (one suffix per shard)
    others = []
    CB = C.CFUNCTYPE(None, C.c_void_p, C.POINTER(C.c_uint8), C.c_size_t)
    cb = CB(lambda arg, p, n: others.append(bytes(p[:n])))
    L.rsbwt_service_set_other_handler(svc, C.cast(cb, C.c_void_p), None)
    assert L.rsbwt_service_start(svc) == 0
    want = {0: [], 1: []}
    n_reads_req = 0
    for x in stream:
        if x["t"] == 2 and x["rt"] == 2:
            n_reads_req += 1
            want[0] += by_req[x["request"]]["replies"] if x["request"] in by_req else _empty_reads_replies(pb, x["q"])
        elif x["replies"]:
            want[x["channel"]] += [bytes.fromhex(r) for r in x["replies"]]

    def feed():
        for x in stream:
            w = bytes.fromhex(x["request"])
            buf = (C.c_uint8 * max(len(w), 1)).from_buffer_copy(w or b"\\0")
            assert L.rsbwt_transport_push_request(tr, buf, len(w)) == 0
    th = threading.Thread(target=feed)
    th.start()
    cap = 4 << 20
    buf = (C.c_uint8 * cap)()
    n = C.c_size_t()
    for ch in (1, 0):
        for j, w in enumerate(want[ch]):
            assert L.rsbwt_transport_pop_reply(tr, ch, buf, cap, C.byref(n), 60_000_000) == 0, (ch, j)
            assert _same(bytes(buf[:n.value]), w), (ch, j, n.value)
    th.join()
    L.rsbwt_transport_close(tr)
    assert L.rsbwt_service_stop(svc) == 0
    assert L.rsbwt_transport_pop_reply(tr, 0, buf, cap, C.byref(n), 1000) == -2  # exactly two per request and partition
    assert L.rsbwt_service_read_requests(svc) == n_reads_req
    # what is left to the embedder: KmerMatch, SiteMatch -- no ExactMatch request of either return type served here
    assert sorted(others) == sorted(bytes.fromhex(x["request"]) for x in stream if not x["replies"] and not (x["t"] == 2 and x["rt"] == 2))
    assert any(isinstance(r, dict) for r in want[0]) and sum(1 for x in gr["items"] if max(x["reads"]) > 4097) >= 2
    L.rsbwt_service_free(svc)
    L.rsbwt_transport_free(tr)
    ss.close()
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("per_partition", [1, 0])
def test_gpu_service_loop_reads_many_partitions(rsb, oracle, pb, tmp_path, per_partition):
    """The same over a set of four suffix partitions (reads that end in A, C, G, T: csrc/synth.cpp's shard rule) held by
    one process: per partition and strand a reply with what THAT partition holds (per_partition = 1; a tile is looked up
    only where it ends with the partition's suffix, service.cpp:228-230,759), or the four lists joined in shard order
    (= 0).  Expected lists composed from the oracle per shard: interval rows / reads containing the query in SA-row
    order after the tiles; the tile matches as a set (their order is pinned on one partition by the golden test)."""
    Request, Reply = pb
    L = rsb.lib()
    kw = dict(seed=31, genome_len=30000, haplotypes=4, snp_rate=0.004, read_len=60, coverage=4.0)
    MINL, MAXL = 40, 60
    shards, oixs, shard_reads = [], [], []
    for s in range(4):
        p = str(tmp_path / f"s{s}.bwt")
        rd = str(tmp_path / f"s{s}.reads")
        rsb.synth_popbwt(p, rd, shard=s, num_shards=4, **kw)
        shards.append(rsb.GpuBWT(p, for_reads=(s % 2 == 0)))
        oixs.append(oracle.load(p))
        shard_reads.append(set(open(rd).read().split()))
        assert all(r.endswith("ACGT"[s]) for r in shard_reads[-1])
    all_reads = sorted(set().union(*shard_reads))
    rng = np.random.default_rng(12)
    rnd = lambda k: "".join("ACGT"[x] for x in rng.integers(0, 4, k))
    qs = []
    for k in (8, 15, 31, 39, 40, 41, 50, 59):
        for _ in range(4):
            r = all_reads[rng.integers(len(all_reads))]
            st = int(rng.integers(0, len(r) - k + 1))
            qs.append(r[st:st + k])
    qs += [all_reads[rng.integers(len(all_reads))] for _ in range(4)]
    qs += [rnd(int(rng.integers(1, 20))) + all_reads[rng.integers(len(all_reads))] + rnd(int(rng.integers(0, 20))) for _ in range(4)]
    qs += [_rc(all_reads[rng.integers(len(all_reads))]), rnd(30), rnd(45), rnd(100), "ACGTN" * 5, ""]
    ss = rsb.ShardSet(shards)
    tr, svc = C.c_void_p(), C.c_void_p()
    assert L.rsbwt_transport_inproc(C.byref(tr)) == 0
    assert L.rsbwt_service_create(ss._s, tr, 2000, 64, per_partition, C.byref(svc)) == 0
    L.rsbwt_service_set_reads(svc, 1, MINL, MAXL)
    suf = (C.c_char_p * 4)(b"A", b"C", b"G", b"T")
    assert L.rsbwt_service_set_suffixes(svc, suf, 4) == 0
    for q in qs:
        r = Request()
        r.t, r.rt, r.q = 2, 2, q
        w = r.SerializeToString()
        buf = (C.c_uint8 * len(w)).from_buffer_copy(w)
        assert L.rsbwt_transport_push_request(tr, buf, len(w)) == 0
    L.rsbwt_transport_close(tr)
    assert L.rsbwt_service_run(svc) == 0

    def expect(s, w):
        """(tile matches as a set, the reads behind them in order) of find_reads in partition s"""
        ok = bool(w) and all(c in "ACGT" for c in w)
        tiles, seqs = set(), []
        if len(w) >= MINL:
            for T in ([MAXL, MINL] if len(w) >= MAXL else ([MINL] if len(w) != MINL else [])):
                for i in range(len(w) - T + 1):
                    t = w[i:i + T]
                    if t.endswith("ACGT"[s]) and t in shard_reads[s]:
                        tiles.add(t)
        if ok and len(w) < MAXL:
            lo, up = oixs[s].find_interval(w)
            for row in range(lo, up + 1) if up >= lo else []:
                pre, post = oixs[s].extract(row)
                seqs.append(pre + post)
        return tiles, seqs
    cap = 1 << 20
    buf = (C.c_uint8 * cap)()
    n = C.c_size_t()
    some_tiles = some_reads = 0
    for q in qs:
        for s in (range(4) if per_partition else [None]):
            for strand in (0, 1):
                assert L.rsbwt_transport_pop_reply(tr, 0, buf, cap, C.byref(n), 5_000_000) == 0
                m = Reply()
                m.ParseFromString(bytes(buf[:n.value]))
                assert (m.rt, m.t, m.q) == (2, 2, q) and m.HasField("r")
                got = [x.r for x in (m.r.revcomp_matches if strand else m.r.forward_matches)]
                assert not (m.r.forward_matches if strand else m.r.revcomp_matches)
                w = _rc(q) if strand else q
                parts = [expect(p, w) for p in (range(4) if s is None else [s])]
                at = 0
                for tiles, seqs in parts:  # a partition's list: its tile matches, then its reads (shard order when joined)
                    assert set(got[at:at + len(tiles)]) == tiles and len(set(got[at:at + len(tiles)])) == len(tiles), (q, s, strand)
                    at += len(tiles)
                    assert got[at:at + len(seqs)] == seqs, (q, s, strand)
                    at += len(seqs)
                    some_tiles += len(tiles)
                    some_reads += len(seqs)
                assert at == len(got)
    assert some_tiles > 5 and some_reads > 100
    assert L.rsbwt_transport_pop_reply(tr, 0, buf, cap, C.byref(n), 1000) == -2
    L.rsbwt_service_free(svc)
    L.rsbwt_transport_free(tr)
    ss.close()
    for g in shards:
        g.close()


def test_exceptions_do_not_cross_the_c_boundary(rsb):
    """extern "C" bodies that allocate run inside guarded() (csrc/capi_guard.h): an allocation that cannot be
    had comes back as RSBWT_ENOMEM instead of std::terminate.  No GPU is needed to get there."""
    L = rsb.lib()
    tr = C.c_void_p()
    assert L.rsbwt_transport_inproc(C.byref(tr)) == 0
    one = (C.c_uint8 * 1)(0)
    assert L.rsbwt_transport_push_request(tr, one, (1 << 62) + 5) == -4  # vector(first, first + 2^62): length_error
    assert b"allocation" in L.rsbwt_last_error()
    L.rsbwt_transport_free(tr)
    hs = (C.c_void_p * 1)(None)
    out = C.c_void_p()
    assert L.rsbwt_set_from_handles(hs, 1 << 61, C.byref(out)) == -7 and not out.value  # (2^61 x 8 bytes wraps to 0)
    assert L.rsbwt_strerror(-8) == b"host runtime error"


def test_decoder_and_config_reader_survive_garbage(rsb, tmp_path):
    """Hostile bytes: the Request decoder and the service.cfg reader are fed random and mutated inputs;
    they may refuse them, they may not crash, hang or read past the buffer (ASan-clean by construction:
    every length is checked against the bytes left before it is used)."""
    L = rsb.lib()
    rng = np.random.default_rng(12345)
    good = bytes([0x08, 0x01, 0x10, 0x01, 0x1A, 0x05]) + b"ACGTA"
    t, rt, q, ql = C.c_int(), C.c_int(), C.c_char_p(), C.c_size_t()
    assert L.rsbwt_proto_decode_request(good, len(good), C.byref(t), C.byref(rt), C.byref(q), C.byref(ql)) == 0
    assert (t.value, rt.value, ql.value) == (1, 1, 5)
    for i in range(20000):
        if i % 2:
            blob = rng.integers(0, 256, int(rng.integers(0, 64)), dtype=np.uint8).tobytes()
        else:  # a valid message with a few bytes flipped / cut short / lengths blown up
            b = bytearray(good)
            for _ in range(int(rng.integers(1, 4))):
                b[int(rng.integers(0, len(b)))] = int(rng.integers(0, 256))
            blob = bytes(b[: int(rng.integers(0, len(b) + 1))])
        rc = L.rsbwt_proto_decode_request(blob, len(blob), C.byref(t), C.byref(rt), C.byref(q), C.byref(ql))
        assert rc in (0, -6) or rc < 0
        if rc == 0:
            assert ql.value <= len(blob)
    base = 'prefix = "p"; suffix = "s"; hashfile = "h"; pull = "a"; push = "b"; push_count = "c";\n' \
           'rocksdb_path = "r"; rocksdb_ext = ".db"; rocksdb = [ "x", "y" ];\n'
    for i in range(300):
        b = bytearray(base.encode())
        for _ in range(int(rng.integers(1, 6))):
            b[int(rng.integers(0, len(b)))] = int(rng.integers(1, 256))
        p = tmp_path / f"g{i}.cfg"
        p.write_bytes(bytes(b[: int(rng.integers(1, len(b) + 1))]))
        h = C.c_void_p()
        rc = L.rsbwt_service_config_load(str(p).encode(), C.byref(h))
        if rc == 0:
            assert L.rsbwt_service_config_get(h, b"pull") is not None
            L.rsbwt_service_config_free(h)
        else:
            assert not h.value


def test_host_parsers_under_address_and_ub_sanitizers(tmp_path):
    """tests/native/fuzz_service_host.cpp: the Request decoder, the Reply encoder and the service.cfg
    reader built with -fsanitize=address,undefined (CPU build; the GPU engine's entry points they call
    are stubbed) and run on 3*10^5 random / mutated messages and 3,000 mutated config files."""
    import os
    import shutil
    import subprocess
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "fuzz_service_host")
    srcs = [os.path.join(root, "tests", "native", "fuzz_service_host.cpp"),
            os.path.join(root, "readserver_amd", "csrc", "service_slice.cpp"),
            os.path.join(root, "readserver_amd", "csrc", "service_loop.cpp")]
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        f"-I{os.path.join(root, 'include')}", *srcs, "-lpthread", "-o", exe], capture_output=True, text=True)
    if b.returncode != 0 and "sanitize" in b.stderr:
        pytest.skip("no sanitizer runtime here")
    assert b.returncode == 0, b.stderr
    r = subprocess.run([exe, "300000", str(tmp_path / "f.cfg")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "accepted" in r.stdout


def test_service_loop_under_thread_sanitizer(tmp_path):
    """tests/native/tsan_service_loop.cpp: producer, loop, consumer and a statistics poller on the
    in-process transport under -fsanitize=thread (the GPU engine behind the loop stubbed): no report, and
    exactly 2 x partitions Replies per count Request."""
    import os
    import shutil
    import subprocess
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "tsan_service_loop")
    srcs = [os.path.join(root, "tests", "native", "tsan_service_loop.cpp"),
            os.path.join(root, "readserver_amd", "csrc", "service_slice.cpp"),
            os.path.join(root, "readserver_amd", "csrc", "service_loop.cpp")]
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=thread", "-include",
                        os.path.join(root, "tests", "native", "tsan_prelude.h"), f"-I{os.path.join(root, 'include')}",
                        *srcs, "-lpthread", "-o", exe], capture_output=True, text=True)
    if b.returncode != 0 and "sanitize" in b.stderr:
        pytest.skip("no sanitizer runtime here")
    assert b.returncode == 0, b.stderr
    r = subprocess.run([exe, "50000"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ThreadSanitizer" not in r.stderr, r.stdout + r.stderr[-4000:]
