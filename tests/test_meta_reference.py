"""CPU guards for the sample-table tests: tests/meta_reference.py's restatement over the oracle's BWT against its
computation with no BWT on the gt fixture and on the `ragged` fixture (reads of 12-600), the coverage of the pairs
tests/test_gpu_meta.py builds on the GPU, the ReplyAll encoder against the protobuf runtime, the pairs-file parser, the host
code under the address and undefined-behaviour sanitizers as a program of its own, and the boundary of the calls without a
GPU."""
import collections
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import gt_reference as G
import meta_proto
import meta_reference as MR
import test_kmer_fixtures as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = {"rsbwt_set_meta_build": 7, "rsbwt_set_meta_load": 3, "rsbwt_set_meta_clear": 1, "rsbwt_set_meta_bytes": 1,
         "rsbwt_set_read_ordinals_var": 6, "rsbwt_set_meta_by_ordinal": 8, "rsbwt_set_meta_by_ordinal_dev": 8,
         "rsbwt_set_read_meta_var": 9, "rsbwt_set_meta_last_work": 1, "rsbwt_proto_encode_all_reply": 16, "rsbwt_meta_parse_file": 9,
         "rsbwt_service_set_all": 5, "rsbwt_service_all_requests": 1}

HASH = {b"A": "one-byte-A", b"AB": "sample-AB", b"\x01\xfe": "low-high", b"ABC": "three", b"zz": "first-wins"}
HASH_TEXT = (b"sample-AB\tAB\n\nno tab on this line\none-byte-A\tA\nlow-high\t\x01\xfe\nthree\tABC\nfirst-wins\tzz\nsecond-loses\tzz\n"
             b"tab-in-code\tq\tq")


def _sides(oracle, shards, runs):
    return ([MR.OracleSide(oracle.from_runs(r, len(sh)), len(sh)) for sh, r in zip(shards, runs)], [MR.PlainSide(sh) for sh in shards])


@pytest.fixture(scope="module")
def gt(oracle):
    fx = G.fixture()
    return (fx,) + _sides(oracle, fx.shards, fx.runs())


def _strings(shards, pairs):
    """what both restatements are asked: the pairs' strings, every distinct read, and strings that are no read"""
    distinct = sorted({r for sh in shards for r in sh})
    return [w for w, _ in pairs] + distinct + [distinct[0][1:], distinct[-1][:-1], "A", "ACGTN", "", distinct[0] + "A"]


def test_the_gt_fixture_is_what_the_tests_count_on(gt):
    fx = gt[0]
    assert [len(sh) for sh in fx.shards] == [280, 280] and {len(r) for sh in fx.shards for r in sh} == {40}
    assert [len(set(sh)) for sh in fx.shards] == [180, 193]
    held = sorted(v for sh in fx.shards for v in collections.Counter(sh).values())
    assert held[-1] == 20 and held[-2] < 20  # one string held 20 times
    assert len(set(fx.shards[0]) & set(fx.shards[1])) == 24


def test_the_pairs_reach_every_class(gt):
    """fails if the pairs miss: a read with copies >= 2, a read in both shards, a string given twice with different values,
    a string that matches nothing, a string with N, an empty value, an ordinal no pair reaches -- or a value length of the
    ladder among the values the table ends up holding"""
    fx, orc, plain = gt
    pairs, info = MR.pairs_for(fx.shards)
    strings = [w for w, _ in pairs]
    look = {w: [s.lookup(w) for s in orc] for w in set(strings)}
    assert any(c >= 2 for w in strings for _, c, _ in look[w])
    assert any(all(c > 0 for _, c, _ in look[w]) for w in strings)
    seen = collections.defaultdict(set)
    for w, v in pairs:
        seen[w].add(v)
    assert sum(len(v) > 1 for v in seen.values()) >= 2 and all(len(seen[w]) == 2 for w in info["twice"])
    assert info["nothing"] and all(MR.searchable(w) and not any(c for _, c, _ in look[w]) for w in info["nothing"])
    assert "N" in info["with_n"] and "" in strings and look[""] == [(0, 0, 0)] * 2
    tables, stats = MR.build_tables(orc, pairs)
    assert any(v == b"" for w, v in pairs if any(c for _, c, _ in look[w]))  # an empty value given to a read
    reached = [[False] * s.ns for s in orc]
    for w in strings:
        for p, (o, c, _) in enumerate(look[w]):
            for x in range(o, o + c):
                reached[p][x] = True
    assert all(not all(r) and any(r) for r in reached)  # ordinals no pair reaches, in both shards
    assert stats[2] == sum(sum(r) for r in reached) and stats[0] + stats[1] == len(pairs) and stats[1] >= len(info["nothing"]) + 2
    assert {len(v) for t in tables for v in t} >= set(MR.LADDER), sorted(set(MR.LADDER) - {len(v) for t in tables for v in t})
    assert stats[3] == sum(len(v) for t in tables for v in t)


@pytest.mark.parametrize("name", ["gt", "ragged"])
def test_restatement_agrees_with_the_computation_without_a_bwt(oracle, gt, name):
    """ordinal and copies of every string, and the built tables, value for value"""
    if name == "gt":
        fx, orc, plain = gt
        shards = fx.shards
    else:
        fx = F.fixture("ragged")
        shards = fx.shards
        orc, plain = _sides(oracle, shards, fx.runs())
        assert min(len(r) for r in shards[0]) == 12 and max(len(r) for r in shards[0]) == 600
    pairs, _ = MR.pairs_for(shards)
    asked = _strings(shards, pairs)
    some = 0
    for w in asked:
        for p in range(len(shards)):
            assert orc[p].lookup(w)[:2] == plain[p].lookup(w)[:2], (name, p, w[:50])
            some += orc[p].lookup(w)[1] > 0
    assert some > 100
    tables, _ = MR.build_tables(orc, pairs)
    assert tables == MR.build_tables_plain(shards, pairs)
    # the two orders of the duplicate pairs give different tables: the order is what decides
    swapped = [pairs[len(pairs) - 1 - i] for i in range(len(pairs))]
    assert MR.build_tables(orc, swapped)[0] == MR.build_tables_plain(shards, swapped) != tables
    # lookups by string: the first ordinal's value where there is a read, nothing elsewhere
    vals, copies, steps = MR.read_meta(orc, tables, asked)
    S = len(shards)
    for q, w in enumerate(asked):
        for p in range(S):
            o, c, _ = plain[p].lookup(w)
            assert copies[p][q] == c and vals[q * S + p] == (tables[p][o] if c else b"")
    assert steps > sum(len(w) for w in asked if MR.searchable(w)) // 4


@pytest.mark.parametrize("size_of_sample,has_other", [(1, False), (2, True), (3, True)])
def test_encoder_is_the_protobuf_runtimes_bytes(rsb, size_of_sample, has_other):
    """rsbwt_proto_encode_all_reply against the protobuf runtime's serialisation of the same Reply: bytes below 33 and
    above 127 in c / l (negative int32: ten-byte varints), codes missing from the hash (g = ""), a ragged tail (cut at the
    last whole record), empty values, no reads at all; All and Samples, ExactMatch and KmerMatch, both strands"""
    Reply, _, _ = meta_proto.build()
    rec = size_of_sample + (2 if has_other else 0)
    code, missing = {1: b"A", 2: b"AB", 3: b"ABC"}[size_of_sample], b"?#%"[:size_of_sample]
    R = lambda g, c=0x21, l=0x21: g + (bytes([c, l]) if has_other else b"")  # noqa: E731  one record
    values = [b"", R(code), R(code, 0x05, 0xF0) * 3, R(missing, 0x00, 0xFF),  # (a code the hash does not have)
              R(code, 0x20, 0x80) * 2 + code[:1],                              # a ragged tail (none at a record of one byte)
              bytes(range(7, 7 + rec - 1)),                                    # shorter than one record
              R(code, 0x7F, 0x21), R(code, 0x0B, 0x0D)]
    reads = ["ACGT" * 10, "T" * 73, "G", "", "ACGTTGCA" * 12 + "A", "C" * 40, "AC" * 20, "GT" * 20]
    hash_map = {k: v for k, v in HASH.items()}
    for t, rt, revcomp in ((2, 3, False), (2, 4, True), (3, 3, True), (3, 4, False)):
        want = meta_proto.all_reply(Reply, t, rt, "ACGTNACGT", revcomp, reads, values, hash_map, size_of_sample, has_other)
        got = rsb.encode_all_reply(t, rt, "ACGTNACGT", revcomp, reads, values, HASH_TEXT, size_of_sample, has_other)
        assert got == want, (t, rt, revcomp)
        back = Reply.FromString(got)
        assert back.rt == t and back.t == rt and back.HasField("a") and not back.HasField("r")
        ms = back.a.revcomp_matches if revcomp else back.a.forward_matches
        assert [m.r for m in ms] == reads and [len(m.s) for m in ms] == [len(v) // rec for v in values]
        if has_other:
            cl = [(s.c, s.l) for m in ms for s in m.s]
            assert any(c < 0 for c, _ in cl) and any(l < -100 for _, l in cl) and any(c > 90 for c, _ in cl)
        assert any(s.g == "" for m in ms for s in m.s) and any(s.g != "" for m in ms for s in m.s)
        # no reads: `a` is there and empty, the bytes of rsbwt_proto_encode_empty_reply
        empty = rsb.encode_all_reply(t, rt, "ACGT", revcomp, [], [], HASH_TEXT, size_of_sample, has_other)
        assert empty == meta_proto.all_reply(Reply, t, rt, "ACGT", revcomp, [], [], hash_map, size_of_sample, has_other)
        buf = np.zeros(len(empty), np.uint8)
        assert rsb.lib().rsbwt_proto_encode_empty_reply(buf.ctypes.data_as(C.c_void_p), buf.size, t, rt, b"ACGT", 4, 1 if revcomp else 0) == len(empty)
        assert buf.tobytes() == empty
    # the first line of a code wins; a code holding a tab is a code
    got = Reply.FromString(rsb.encode_all_reply(2, 3, "A", False, ["A", "C"], [b"zz", b"q\tq"], HASH_TEXT, 2, False))
    assert [s.g for s in got.a.forward_matches[0].s] == ["first-wins"]
    got = Reply.FromString(rsb.encode_all_reply(2, 3, "A", False, ["C"], [b"q\tq"], HASH_TEXT, 3, False))
    assert [s.g for s in got.a.forward_matches[0].s] == ["tab-in-code"]
    # bad arguments: 0
    L = rsb.lib()
    assert L.rsbwt_proto_encode_all_reply(None, 0, 2, 3, b"A", 1, 0, None, None, None, None, 0, None, 0, 0, 0) == 0  # a record of no bytes
    assert L.rsbwt_proto_encode_all_reply(None, 0, 2, 5, b"A", 1, 0, None, None, None, None, 0, None, 0, 2, 1) == 0
    assert L.rsbwt_proto_encode_all_reply(None, 0, 2, 3, b"A", 1, 0, None, None, None, None, 1, None, 0, 2, 1) == 0


PAIRS_FILE = b"ACGT\r\nab\r\nTTTT\n\nGG\n\x01\xfe!!zz\x7f\x80\nCC\nlast value without newline"


def test_file_parser(rsb, tmp_path):
    """CRLF is not special, an empty value line is an empty value, a last value line needs no newline, an odd last line (a
    read without its value) is ignored as `getline && getline` ignores it; an unreadable file is RSBWT_EIO"""
    p = tmp_path / "pairs.txt"
    p.write_bytes(PAIRS_FILE)
    reads, values = rsb.parse_meta_file(p)
    assert reads == [b"ACGT\r", b"TTTT", b"GG", b"CC"]
    assert values == [b"ab\r", b"", b"\x01\xfe!!zz\x7f\x80", b"last value without newline"]
    for body, n in ((b"", 0), (b"ACGT", 0), (b"ACGT\n", 0), (b"ACGT\n\n", 1), (b"ACGT\nv\nTT", 1), (b"ACGT\nv\nTT\n", 1), (b"\n\n", 1),
                    (b"ACGT\nv\nTT\n\n", 2)):
        p.write_bytes(body)
        r, v = rsb.parse_meta_file(p)
        assert len(r) == len(v) == n, body
    assert rsb.parse_meta_file(p) == ([b"ACGT", b"TT"], [b"v", b""])
    sz = (C.c_size_t * 3)()
    assert rsb.lib().rsbwt_meta_parse_file(str(tmp_path / "missing").encode(), None, 0, None, None, 0, None, 0, sz) == -2
    assert rsb.lib().rsbwt_meta_parse_file(str(p).encode(), None, 0, None, None, 0, None, 0, sz) == -7 and list(sz) == [2, 6, 1]
    assert rsb.lib().rsbwt_meta_parse_file(None, None, 0, None, None, 0, None, 0, sz) == -1


def _fnv(b):
    h = 1469598103934665603
    for x in b:
        h = ((h ^ x) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def test_host_code_under_address_and_ub_sanitizers(rsb, gt, tmp_path):
    """tests/native/meta_file_host.cpp: the parser and the encoder (readserver_amd/csrc/meta_file.h) built with
    -fsanitize=address,undefined and run as a program of its own over the pairs file of the gt fixture's pairs and a hash
    file -- the same inputs the library is given here: the pair counts and an FNV-1a of every Reply must agree -- and over
    300 mutations of that file"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    pairs, _ = MR.pairs_for(gt[0].shards)
    body = b"".join(w.encode() + b"\n" + v + b"\n" for w, v in pairs) + b"ACGT"  # (and an odd last line)
    pf, hf = tmp_path / "pairs.txt", tmp_path / "hash.txt"
    pf.write_bytes(body)
    hf.write_bytes(HASH_TEXT)
    exe = str(tmp_path / "meta_file_host")
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(ROOT, "tests", "native", "meta_file_host.cpp"), "-o", exe], capture_output=True, text=True)
    if b.returncode != 0 and "sanitize" in b.stderr:
        pytest.skip("no sanitizer runtime here")
    assert b.returncode == 0, b.stderr
    r = subprocess.run([exe, str(pf), str(hf), "300"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "meta_file ok: 300 mutations" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
    reads, values = rsb.parse_meta_file(pf)
    assert [x.decode() for x in reads] == [w for w, _ in pairs] and values == [v for _, v in pairs]
    lines = r.stdout.splitlines()
    assert lines[0] == f"pairs {len(pairs)} {sum(len(x) for x in reads)} {sum(len(v) for v in values)} hash 6"
    got = [ln.split() for ln in lines if ln.startswith("reply ")]
    assert len(got) == 6
    for _, ss, other, revcomp, ln, digest in got:
        mine = rsb.encode_all_reply(2, 4 if revcomp == "1" else 3, "ACGTNACGT", revcomp == "1", reads, values, HASH_TEXT, int(ss), other == "1")
        assert (len(mine), "%016x" % _fnv(mine)) == (int(ln), digest), (ss, other, revcomp)


def test_entry_points_are_declared_exported_and_bound_and_no_gpu_is_enodev(rsb):
    from readserver_amd import _native
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rsbwt.h")).read(), flags=re.S)
    L = C.CDLL(rsb.lib_path())
    for n, nargs in ENTRY.items():
        assert re.search(r"\b%s\s*\(" % n, txt), f"{n} is not declared in include/rsbwt.h"
        assert n in _native.SIGNATURES and hasattr(L, n) and hasattr(rsb.lib(), n)
        assert len(_native.SIGNATURES[n][1]) == nargs, n
    for m in ("meta_build", "meta_load", "meta_clear", "meta_bytes", "read_ordinals", "meta_by_ordinal", "meta_by_ordinal_dev", "read_meta",
              "meta_last_work"):
        assert callable(getattr(rsb.ShardSet, m)), m
    assert callable(rsb.encode_all_reply) and callable(rsb.parse_meta_file)
    L = rsb.lib()
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    text = np.frombuffer(b"ACGTACGT", np.uint8).copy()
    off = np.array([0, 4, 8], np.uint64)
    first = np.full(5, 77, np.uint64)
    out = np.full(16, 77, np.uint8)
    n = C.c_size_t(77)
    # no set without a GPU: a null set is RSBWT_EINVAL everywhere, and nothing is written
    assert L.rsbwt_set_meta_build(None, p(text), p(off), p(out), p(off), 2, None) == -1
    assert L.rsbwt_set_meta_load(None, b"/nonexistent", None) == -1
    assert L.rsbwt_set_meta_clear(None) == -1 and L.rsbwt_set_meta_bytes(None) == 0
    assert L.rsbwt_set_read_ordinals_var(None, p(text), p(off), 2, p(first), p(first)) == -1
    assert L.rsbwt_set_meta_by_ordinal(None, p(first), p(first), 2, p(first), p(out), 16, C.byref(n)) == -1
    assert L.rsbwt_set_meta_by_ordinal_dev(None, None, None, 0, None, None, 0, None) == -1
    assert L.rsbwt_set_read_meta_var(None, p(text), p(off), 2, p(first), p(out), 16, C.byref(n), None) == -1
    assert L.rsbwt_service_set_all(None, 1, None, 2, 1) == -1 and L.rsbwt_service_all_requests(None) == 0
    assert (first == 77).all() and (out == 77).all() and n.value == 77
    w = (C.c_uint64 * 4)(*([9] * 4))
    L.rsbwt_set_meta_last_work(None)
    L.rsbwt_set_meta_last_work(w)
    assert list(w) == [0] * 4
