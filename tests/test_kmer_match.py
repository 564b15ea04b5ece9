"""KmerMatch Count / Reads and the empty replies of unserved requests, host side (CPU): Request fields k / s, the
KmerMatch Reply and every (request type, return type) empty Reply against the Python protobuf runtime on the re-typed
schema (tests/proto_schema.py = src/service/readserver.proto), and the two service.cfg keys."""
import ctypes as C
import os

import numpy as np
import pytest

import proto_schema


@pytest.fixture(scope="module")
def pb():
    return proto_schema.build()


def _decode_ks(L, wire):
    buf = (C.c_uint8 * max(len(wire), 1)).from_buffer_copy(wire + b"\0")
    k, hk, s, hs = C.c_int32(), C.c_int(), C.c_int32(), C.c_int()
    rc = L.rsbwt_proto_decode_request_ks(buf, len(wire), C.byref(k), C.byref(hk), C.byref(s), C.byref(hs))
    return rc, (k.value, hk.value, s.value, hs.value)


def test_request_k_and_s_are_decoded(rsb, pb):
    """fields 4 and 5 (optional int32 k, s: readserver.proto:9-10), negative values included (sign-extended varints);
    absent ones read as 0, as protobuf's getters give them"""
    Request, _ = pb
    L = rsb.lib()
    rng = np.random.default_rng(1)
    for _ in range(200):
        r = Request()
        r.t, r.rt, r.q = 3, int(rng.integers(1, 5)), "ACGT" * int(rng.integers(0, 40))
        has_k, has_s = rng.random() < 0.7, rng.random() < 0.7
        if has_k:
            r.k = int(rng.choice([0, 1, 15, 31, 70, -1, -(2 ** 31), 2 ** 31 - 1]))
        if has_s:
            r.s = int(rng.choice([0, 1, 5, 40, -1, -7, 2 ** 31 - 1]))
        rc, got = _decode_ks(L, r.SerializeToString())
        assert rc == 0
        assert got == (r.k if has_k else 0, int(has_k), r.s if has_s else 0, int(has_s))
    assert _decode_ks(L, b"\x08\x03")[0] != 0  # rt and q are required


def _kmer_reply(L, rt, q, revcomp, reads):
    arr = (C.c_char_p * max(len(reads), 1))(*[x.encode() for x in reads])
    lens = (C.c_size_t * max(len(reads), 1))(*[len(x) for x in reads])
    n = L.rsbwt_proto_encode_kmer_reply(None, 0, rt, q.encode(), len(q), revcomp, arr, lens, len(reads))
    out = (C.c_uint8 * max(n, 1))()
    assert L.rsbwt_proto_encode_kmer_reply(out, n, rt, q.encode(), len(q), revcomp, arr, lens, len(reads)) == n
    return bytes(out[:n])


def test_kmer_reply_matches_protobuf_runtime(rsb, pb):
    """KmerTask::run (src/service/service.cpp:871-960): rt = KmerMatch, t = (ReplyType) return type, the original q;
    Count: c = the set's size; Reads: r with one ResultReads per read, present even when empty"""
    _, Reply = pb
    L = rsb.lib()
    rng = np.random.default_rng(2)
    for nreads in (0, 1, 2, 17, 300):
        reads = ["".join("ACGT"[x] for x in rng.integers(0, 4, int(rng.integers(1, 120)))) for _ in range(nreads)]
        q = "".join("ACGTN"[x] for x in rng.integers(0, 5, int(rng.integers(0, 200))))
        for revcomp in (0, 1):
            rep = Reply()
            rep.rt, rep.t, rep.q = 3, 1, q
            (rep.c.revcomp_matches if revcomp else rep.c.forward_matches).c = nreads
            assert _kmer_reply(L, 1, q, revcomp, reads) == rep.SerializeToString()
            rep = Reply()
            rep.rt, rep.t, rep.q = 3, 2, q
            rep.r.SetInParent()
            for x in reads:
                (rep.r.revcomp_matches if revcomp else rep.r.forward_matches).add().r = x
            assert _kmer_reply(L, 2, q, revcomp, reads) == rep.SerializeToString()
    assert L.rsbwt_proto_encode_kmer_reply(None, 0, 5, b"A", 1, 0, None, None, 0) == 0


def test_empty_replies_match_protobuf_runtime(rsb, pb):
    """what the reference sends for an empty result, for every (request type, return type) a service process takes:
    Count -> c{ResultCount{0}}, Reads -> an empty r, All / Samples -> an empty a (KmerTask default branch :917-,
    QueryTask :1283-, GtTask :1136-: mutable_a() is called before the loop)"""
    _, Reply = pb
    L = rsb.lib()
    for t in (2, 3, 4):
        for rt in (1, 2, 3, 4):
            for q in ("", "ACGTNACGT", "A" * 300):
                for revcomp in (0, 1):
                    rep = Reply()
                    rep.rt, rep.t, rep.q = t, rt, q
                    if rt == 1:
                        (rep.c.revcomp_matches if revcomp else rep.c.forward_matches).c = 0
                    elif rt == 2:
                        rep.r.SetInParent()
                    exp = rep.SerializeToString()
                    if rt > 2:  # (the re-typed schema has no ReplyAll: an empty `a` = field 6, length 0, after q)
                        exp += b"\x32\x00"
                    n = L.rsbwt_proto_encode_empty_reply(None, 0, t, rt, q.encode(), len(q), revcomp)
                    out = (C.c_uint8 * n)()
                    assert L.rsbwt_proto_encode_empty_reply(out, n, t, rt, q.encode(), len(q), revcomp) == n
                    assert bytes(out) == exp, (t, rt, q, revcomp)
    assert L.rsbwt_proto_encode_empty_reply(None, 0, 5, 1, b"A", 1, 0) == 0
    assert L.rsbwt_proto_encode_empty_reply(None, 0, 3, 0, b"A", 1, 0) == 0


def test_service_cfg_keys(rsb, golden_dir, tmp_path):
    """kmermatch / unserved are read as the reference's libconfig file holds them (demo/TEMPLATE.service.cfg's form)"""
    L = rsb.lib()
    text = open(os.path.join(golden_dir, "service_template.cfg")).read()
    p = tmp_path / "service.cfg"
    p.write_text(text + '\nkmermatch = "on";\nunserved = "empty";\n')
    cfg = C.c_void_p()
    assert L.rsbwt_service_config_load(str(p).encode(), C.byref(cfg)) == 0
    try:
        assert L.rsbwt_service_config_get(cfg, b"kmermatch") == b"on"
        assert L.rsbwt_service_config_get(cfg, b"unserved") == b"empty"
    finally:
        L.rsbwt_service_config_free(cfg)
    p.write_text(text)
    assert L.rsbwt_service_config_load(str(p).encode(), C.byref(cfg)) == 0
    try:
        assert L.rsbwt_service_config_get(cfg, b"kmermatch") is None  # absent: today's behaviour
        assert L.rsbwt_service_config_get(cfg, b"unserved") is None
    finally:
        L.rsbwt_service_config_free(cfg)


def test_kmer_work_counters_start_at_zero(rsb):
    """the counters of a thread that has made no call"""
    w = rsb.ShardSet.kmer_last_work()
    assert w == dict(candidates=0, walked=0, lf_steps=0, identities=0, extracted=0)


@pytest.mark.parametrize("key,value", [("unserved", "none"), ("kmermatch", "yes")])
def test_service_rejects_unknown_values_of_the_new_keys(rsb, golden_dir, tmp_path, key, value):
    """rsbwt_service refuses a value it does not know for `unserved` / `kmermatch` before it connects or loads anything"""
    import subprocess
    exe = os.path.join(os.path.dirname(rsb.lib_path()), "rsbwt_service")
    text = open(os.path.join(golden_dir, "service_template.cfg")).read()
    p = tmp_path / "service.cfg"
    p.write_text(text + f'\n{key} = "{value}";\n')
    r = subprocess.run([exe, str(p)], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0
    assert f'{key} = "{value}"' in r.stderr
    assert "loaded" not in r.stdout
