"""CPU guards for the sample-counts tests: tests/sample_reference.py's restatement over the oracle's BWT against its
computation with no BWT on the gt fixture and on the `repeat` and `ragged` read lists, the classes the inputs of
tests/test_gpu_sample_counts.py must reach, the dictionary header (readserver_amd/csrc/sample_codes.h) under the address
and undefined-behaviour sanitizers as a program of its own, and the boundary of the calls without a GPU."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import gt_reference as G
import meta_reference as MR
import sample_reference as SR
import test_kmer_fixtures as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = {"rsbwt_set_sample_counts": 14, "rsbwt_set_sample_counts_dev": 18, "rsbwt_sample_keys": 4, "rsbwt_set_sample_last_work": 1,
         "rsbwt_set_meta_head_bytes": 1}
SHAPES = [(1, True), (1, False), (2, True), (2, False), (3, True), (3, False), (4, True), (4, False), (8, True), (8, False)]


def _fixture(name):
    return G.fixture() if name == "gt" else F.fixture(name)


class Case:
    """one fixture under one record shape: pairs, both restatements' inputs, the queries, a dictionary of 12 of the
    universe's codes in an order that is not ascending"""

    def __init__(self, oracle, name, ss, other):
        fx = _fixture(name)
        self.shards, self.ss, self.other = fx.shards, ss, other
        self.uni, self.outside = SR.universe(ss)
        self.pairs, self.info = SR.sample_pairs(self.shards, self.uni, self.outside, ss, other)
        self.osh = SR.OracleShards(oracle, self.shards, fx.runs(), self.pairs)
        self.queries = SR.queries_for(self.shards)
        self.codes = self.uni[:30:3] + self.uni[40:42]


_CASES = {}


def case(oracle, name, ss, other):
    if (name, ss, other) not in _CASES:
        _CASES[(name, ss, other)] = Case(oracle, name, ss, other)
    return _CASES[(name, ss, other)]


# every record shape on the gt fixture; on the single-shard read lists the shapes at both ends and the usual one
AGREE = [("gt", ss, other) for ss, other in SHAPES] + [(n, ss, other) for n in ("repeat", "ragged") for ss, other in ((2, True), (1, False), (8, True))]


@pytest.mark.parametrize("name,ss,other", AGREE)
def test_restatement_agrees_with_the_computation_without_a_bwt(oracle, name, ss, other):
    """all four outputs and the six work numbers, with no limit and with one that some query is exactly at"""
    c = case(oracle, name, ss, other)
    a = SR.counts_oracle(c.osh, c.queries, c.codes, ss, other)
    b = SR.counts_plain(c.shards, c.pairs, c.queries, c.codes, ss, other)
    assert SR.same(a, b) is None, SR.same(a, b)
    assert a["work"]["carriers"] > 50 and a["work"]["records"] > 1000
    at = sorted(set(int(m) for m in a["matches"] if m > 0))
    limit = at[len(at) // 2]
    a2 = SR.counts_oracle(c.osh, c.queries, c.codes, ss, other, max_rows=limit)
    b2 = SR.counts_plain(c.shards, c.pairs, c.queries, c.codes, ss, other, max_rows=limit)
    assert SR.same(a2, b2) is None, SR.same(a2, b2)
    over = a["matches"] > limit
    assert over.any() and (a["matches"] == limit).any()  # a query over max_rows beside one exactly at it
    assert (a2["strings"][over] == 0).all() and (a2["carriers"][over] == 0).all() and (a2["matches"] == a["matches"]).all()
    assert (a2["strings"][~over] == a["strings"][~over]).all() and (a2["copies"][~over] == a["copies"][~over]).all()


@pytest.mark.parametrize("name", ["gt", "repeat", "ragged"])
def test_the_inputs_reach_every_class(oracle, name):
    """fails if the inputs miss a class the GPU tests count on (include/rsbwt.h's definition, case by case)"""
    ss, other = 2, True
    c = case(oracle, name, ss, other)
    a = SR.counts_oracle(c.osh, c.queries, c.codes, ss, other)
    R = SR.rec_size(ss, other)
    named = {w for w, _ in c.pairs if MR.searchable(w)}
    carried = lambda w: [r for sh in c.shards for r in set(sh) if w and w in r and r in named]  # noqa: E731
    # a carrier that holds its query at two or more offsets
    assert any(len(SR._offsets(r, w)) >= 2 for w in c.queries if MR.searchable(w) for r in carried(w)), name
    if name == "repeat":
        assert any(len(SR._offsets(r, "AAAA")) == 42 for r in carried("AAAA"))
    # a query whose carriers include a string with copies >= 2 (the ragged list holds every string once)
    if name == "ragged":
        assert all(len(set(sh)) == len(sh) for sh in c.shards)
    else:
        assert any(sh.count(r) >= 2 for w in c.queries if MR.searchable(w) for sh in c.shards for r in set(sh) if w in r and r in named), name
    if name == "gt":
        assert max(sh.count(r) for sh in c.shards for r in set(sh)) == 20
        both = set(c.shards[0]) & set(c.shards[1]) & named
        assert any(w in r for w in c.queries if MR.searchable(w) for r in both)  # a string carried in both shards
    # a row on a read no pair names
    assert any(w in r for w in c.queries if MR.searchable(w) for r in c.info["left_out"]), name
    assert a["work"]["rows"] > a["work"]["head_rows"] > a["work"]["carriers"] > 0
    # an unknown code, a stray tail, a negative c, a code listed twice, every rung of the ladder -- among the values carried
    vals = {v for t in c.osh.tables for v in t}
    assert a["work"]["unknown"] > 0 and (a["strings"][:, -1] > 0).any()
    assert any(len(v) % R for v in vals) and (a["copies"] < 0).any()
    assert {len(v) // R for v in vals} >= set(SR.LADDER), sorted(set(SR.LADDER) - {len(v) // R for v in vals})
    dv = dict(c.pairs)[c.info["doubled"]]
    assert dv[:R] == dv[R:2 * R] and dv in vals
    long_carried = {len(v) // R for p, t in enumerate(c.osh.tables) for o, v in enumerate(t) if o in c.osh.heads[p]}
    assert long_carried >= set(SR.LADDER)
    # an absent query, unsearchable ones, and the pairs' own classes
    assert any(MR.searchable(w) and m == 0 for w, m in zip(c.queries, a["matches"]))
    assert "" in c.queries and any("N" in w for w in c.queries)
    assert all(a["matches"][q] == 0 for q, w in enumerate(c.queries) if not MR.searchable(w))
    assert len(c.info["twice"]) == 2 and c.info["nothing"] and "N" in c.info["with_n"]
    assert {len(w) for w in c.queries} >= {0, 1, 4, 8, 12} and any(w in set(c.shards[0]) for w in c.queries)


def test_column_order_and_the_unknown_column(oracle):
    """the columns follow the caller's order; a dictionary of one code, and one that knows every code of the values"""
    c = case(oracle, "gt", 2, True)
    a = SR.counts_oracle(c.osh, c.queries, c.codes, 2, True)
    rev = SR.counts_oracle(c.osh, c.queries, c.codes[::-1], 2, True)
    assert (rev["strings"][:, :-1] == a["strings"][:, :-1][:, ::-1]).all() and (rev["strings"][:, -1] == a["strings"][:, -1]).all()
    one = SR.counts_oracle(c.osh, c.queries, c.codes[:1], 2, True)
    assert (one["strings"][:, 0] == a["strings"][:, 0]).all() and (one["strings"].sum(1) == a["strings"].sum(1)).all()
    full = SR.counts_oracle(c.osh, c.queries, c.uni + c.outside, 2, True)
    assert (full["strings"][:, -1] == 0).all() and full["work"]["unknown"] == 0 and (full["copies"].sum(1) == a["copies"].sum(1)).all()


def _run_host(exe, ss, codes):
    r = subprocess.run([exe, str(ss), b"".join(codes).hex()], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("sample_codes ok"), r.stdout[-2000:] + r.stderr[-3000:]
    return r.stdout.splitlines()


def test_dictionary_header_under_address_and_ub_sanitizers(rsb, tmp_path):
    """tests/native/sample_codes_host.cpp: sample_codes_check / sample_key / sample_column built with
    -fsanitize=address,undefined and run as a program of its own over ascending, duplicate, descending, 1-byte and 8-byte
    dictionaries; its keys are the library's (rsbwt_sample_keys) and Python's big-endian numbers"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "sample_codes_host")
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(ROOT, "tests", "native", "sample_codes_host.cpp"), "-o", exe], capture_output=True, text=True)
    if b.returncode != 0 and "sanitize" in b.stderr:
        pytest.skip("no sanitizer runtime here")
    assert b.returncode == 0, b.stderr
    L = rsb.lib()
    for ss in (1, 2, 3, 4, 8):
        codes = sorted(SR.universe(ss, 64)[0])
        if ss == 8:
            codes = [b"\0" * 8] + codes + [b"\xff" * 8]
        lines = _run_host(exe, ss, codes)
        assert lines[0] == "status 0 bad 0"
        keys = [int(ln.split()[1], 16) for ln in lines if ln.startswith("key ")]
        assert keys == [SR.key_of(c) for c in codes] == sorted(keys)
        cols = [int(ln.split()[1]) for ln in lines if ln.startswith("column ")]
        n = len(codes)
        changed = [codes.index(x) if x in codes else n for x in (c[:-1] + bytes([c[-1] ^ 1]) for c in codes)]
        ends = [codes.index(e) if e in codes else n for e in (b"\0" * ss, b"\xff" * ss)]
        assert cols == list(range(n)) + changed + ends
        flat = np.frombuffer(b"".join(codes), np.uint8).copy()
        out = np.zeros(n, np.uint64)
        assert L.rsbwt_sample_keys(flat.ctypes.data_as(C.c_void_p), n, ss, out.ctypes.data_as(C.c_void_p)) == 0
        assert [int(x) for x in out] == keys
        # a duplicate, a descending pair
        for bad_at, broken in ((5, codes[:5] + [codes[4]] + codes[5:]), (n - 1, codes[:-2] + [codes[-1], codes[-2]])):
            assert _run_host(exe, ss, broken)[0] == f"status 4 bad {bad_at}"
            fb = np.frombuffer(b"".join(broken), np.uint8).copy()
            assert L.rsbwt_sample_keys(fb.ctypes.data_as(C.c_void_p), len(broken), ss, out.ctypes.data_as(C.c_void_p) if len(broken) <= n else None) == -1
            assert b"ascending" in L.rsbwt_last_error()
    assert _run_host(exe, 0, [b"ab"])[0].startswith("status 1") and _run_host(exe, 9, [b"123456789"])[0].startswith("status 1")
    assert _run_host(exe, 2, [])[0].startswith("status 2")
    one = np.zeros(16, np.uint8)
    for ss, n in ((0, 1), (9, 1), (2, 0)):
        assert L.rsbwt_sample_keys(one.ctypes.data_as(C.c_void_p), n, ss, one.ctypes.data_as(C.c_void_p)) == -1
    assert L.rsbwt_sample_keys(None, 1, 2, one.ctypes.data_as(C.c_void_p)) == -1


def test_entry_points_are_declared_exported_and_bound_and_a_null_set_is_einval(rsb):
    from readserver_amd import _native
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rsbwt.h")).read(), flags=re.S)
    L = C.CDLL(rsb.lib_path())
    for n, nargs in ENTRY.items():
        assert re.search(r"\b%s\s*\(" % n, txt), f"{n} is not declared in include/rsbwt.h"
        assert n in _native.SIGNATURES and hasattr(L, n) and hasattr(rsb.lib(), n)
        assert len(_native.SIGNATURES[n][1]) == nargs, n
    for m in ("sample_counts", "sample_last_work", "meta_head_bytes"):
        assert callable(getattr(rsb.ShardSet, m)), m
    L = rsb.lib()
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    text = np.frombuffer(b"ACGTACGT", np.uint8).copy()
    off = np.array([0, 4, 8], np.uint64)
    codes = np.frombuffer(b"abcd", np.uint8).copy()
    out = np.full(16, 77, np.uint64)
    assert L.rsbwt_set_sample_counts(None, p(text), p(off), 2, p(codes), 2, 2, 1, 0, 0, p(out), p(out), p(out), p(out)) == -1
    assert L.rsbwt_set_sample_counts_dev(None, None, None, 0, 4, None, 2, 2, 1, 0, 0, 0, None, None, None, None, None, None) == -1
    assert L.rsbwt_set_meta_head_bytes(None) == 0
    assert (out == 77).all()
    w = (C.c_uint64 * 6)(*([9] * 6))
    L.rsbwt_set_sample_last_work(None)
    L.rsbwt_set_sample_last_work(w)
    assert list(w) == [0] * 6
