"""CPU guards for the overlap tests: tests/overlap_reference.py's restatement over the oracle's BWT against its computation
with no BWT, the coverage of the inputs tests/test_gpu_overlaps.py runs on the GPU, the round trip from an ordinal to its
row and its read on the oracle, the reads one (query, shard) meets under several overlap lengths, and the boundary of the
calls without a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import gt_reference as G
import overlap_reference as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = {"rsbwt_set_overlaps": 8, "rsbwt_overlaps": 8, "rsbwt_set_overlaps_dev": 9, "rsbwt_set_overlap_records": 10,
         "rsbwt_set_overlap_reads": 16, "rsbwt_set_overlap_last_work": 1}


@pytest.fixture(scope="module")
def sides(oracle):
    fx = G.fixture()
    orc = [G.OracleShard(oracle.from_runs(r, len(sh))) for sh, r in zip(fx.shards, fx.runs())]
    return fx, orc, [O.PlainSide(sh) for sh in fx.shards]


@pytest.mark.parametrize("min_overlap,max_overlap", O.PARAMS)
def test_restatement_agrees_with_the_computation_without_a_bwt(sides, min_overlap, max_overlap):
    """all 1,600 items: count and ordinal"""
    fx, orc, plain = sides
    qs = O.queries()
    exp = O.expected(orc, "fixture", qs, min_overlap, max_overlap)
    items = 0
    for p in range(2):
        for q, w in enumerate(qs):
            want = O.profile(plain[p], w, min_overlap, max_overlap)
            assert [e[:2] for e in exp[p][q]] == want, (p, q)
            items += len(w)
    assert items == 1600


def test_the_inputs_reach_every_class(sides):
    """the coverage guard: entries with one read, several, many; suffixes that are a whole read or a whole query; lengths
    below, at, between and above the table depths and limits the GPU tests use; the suffixes holding an N give 0; nothing is
    left at min_overlap 41"""
    fx, orc, _ = sides
    qs = O.queries()
    found = []
    for mo, xo in O.PARAMS:
        exp = O.expected(orc, "fixture", qs, mo, xo)
        found.append(sum(e[1] > 0 for p in range(2) for per in exp[p] for e in per))
    assert all(n > 0 for n in found[:4]) and found[0] > found[1] > found[2] > found[3] and found[4] == 0, found
    exp = O.expected(orc, "fixture", qs, 1, 0)
    ent = [(len(qs[q]) - t, e[1], t) for p in range(2) for q in range(len(qs)) for t, e in enumerate(exp[p][q]) if e[1] > 0]
    cls = {"count==1": sum(c == 1 for _, c, _ in ent), "count>1": sum(c > 1 for _, c, _ in ent), "count>50": sum(c > 50 for _, c, _ in ent),
           "l==40": sum(l == G.READ_LEN for l, _, _ in ent), "l==whole": sum(t == 0 for _, _, t in ent), "l<6": sum(l < 6 for l, _, _ in ent),
           "l==6": sum(l == 6 for l, _, _ in ent), "6<l<10": sum(6 < l < 10 for l, _, _ in ent), "l==10": sum(l == 10 for l, _, _ in ent),
           "l>10": sum(l > 10 for l, _, _ in ent)}
    assert all(v > 0 for v in cls.values()), cls
    # the two suffix families that hold an N: every suffix of query 5 from its N leftwards, and query 13
    assert qs[5][30] == "N" and qs[13] == "N"
    for p in range(2):
        assert all(e[1] == 0 for e in exp[p][5][:31]) and any(e[1] > 0 for e in exp[p][5][31:])
        assert [e[:2] for e in exp[p][13]] == [(0, 0)]


def test_ordinal_round_trip_on_the_oracle(sides):
    """for every record's first and last ordinal o: the row getOccAt('$', o + 1) lies in the suffix's interval, holds '$'
    in the BWT, and the read extracted there begins with the suffix (and is sorted(reads)[o])"""
    fx, orc, plain = sides
    qs = O.queries()
    recs, _ = O.records(O.expected(orc, "fixture", qs, 1, 0), qs)
    assert len(recs) > 100
    for q, p, start, length, o0, cnt, lo, up in recs:
        x = qs[q][start:]
        assert len(x) == length
        for o in {o0, o0 + cnt - 1}:
            row = orc[p].oix.occ_at("$", o + 1)
            assert lo <= row <= up and orc[p].oix.char(row) == "$", (q, p, start, o)
            pre, post = orc[p].extract(row)
            assert pre == "" and post.startswith(x) and post == plain[p].read(o), (q, p, start, o)


def test_a_read_is_met_under_two_overlap_lengths(sides):
    """the dedup guard: the repeat queries make one read begin with several suffixes, so the reads call has something to
    deduplicate -- and a max_reads exists that cuts some (query, shard) pairs and leaves others whole"""
    fx, orc, plain = sides
    qs = O.queries()
    exp = O.expected(orc, "fixture", qs, 6, 0)
    twice = 0
    for q in range(len(qs)):
        for p in range(2):
            seen = {}
            for t, (o, cnt, _, _) in enumerate(exp[p][q]):
                for x in range(o, o + cnt):
                    seen.setdefault(x, []).append(len(qs[q]) - t)
            twice += any(len(v) > 1 for v in seen.values())
    assert twice > 0
    first, out, matches = O.reads_of(exp, qs, plain)
    assert len(out) == sum(matches) == first[-1] < sum(e[1] for p in range(2) for per in exp[p] for e in per)
    first2, out2, matches2 = O.reads_of(exp, qs, plain, max_reads=20)
    assert matches2 == matches and 0 < len(out2) < len(out) and any(m > 20 for m in matches) and any(0 < m <= 20 for m in matches)


def test_entry_points_are_declared_exported_and_bound_and_no_gpu_is_enodev(rsb):
    from readserver_amd import _native
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rsbwt.h")).read(), flags=re.S)
    L = C.CDLL(rsb.lib_path())
    for n, nargs in ENTRY.items():
        assert re.search(r"\b%s\s*\(" % n, txt), f"{n} is not declared in include/rsbwt.h"
        assert n in _native.SIGNATURES and hasattr(L, n) and hasattr(rsb.lib(), n)
        assert len(_native.SIGNATURES[n][1]) == nargs, n
    assert "typedef struct rsbwt_overlap" in txt and rsb.bwt.OVERLAP.itemsize == 56
    assert callable(rsb.GpuBWT.overlaps) and callable(rsb.ShardSet.overlaps) and callable(rsb.ShardSet.overlap_records)
    assert callable(rsb.ShardSet.overlap_reads) and callable(rsb.ShardSet.overlap_last_work)
    L = rsb.lib()
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    text = np.frombuffer(b"ACGTACGT", np.uint8).copy()
    off = np.array([0, 4, 8], np.uint64)
    cnt = np.full(8, 77, np.uint64)
    od = np.full(8, 77, np.uint64)
    n = C.c_size_t(77)
    first = np.full(3, 77, np.uint64)
    none = L.rsbwt_device_count() == 0
    # a box without a GPU can have no set: RSBWT_ENODEV, no CPU fallback; where there is one a null set is RSBWT_EINVAL
    want = -5 if none else -1
    assert L.rsbwt_set_overlaps(None, p(text), p(off), 2, 1, 0, p(cnt), p(od)) == want
    assert (b"no CPU fallback" if none else b"null") in L.rsbwt_last_error()
    assert L.rsbwt_overlaps(None, p(text), p(off), 2, 1, 0, p(cnt), p(od)) == want
    assert L.rsbwt_set_overlap_records(None, p(text), p(off), 2, 1, 0, p(first), None, 0, C.byref(n)) == want and n.value == 0
    n = C.c_size_t(77)
    assert L.rsbwt_set_overlap_reads(None, p(text), p(off), 2, 1, 0, 0, p(first), None, 64, None, None, None, 0, C.byref(n), None) == want
    assert n.value == 0
    assert L.rsbwt_set_overlaps_dev(None, None, None, 0, 0, 1, 0, None, None) == -1
    assert (cnt == 77).all() and (od == 77).all() and (first == 77).all()
    w = (C.c_uint64 * 6)(*([9] * 6))
    L.rsbwt_set_overlap_last_work(None)  # (nothing to write to: no crash)
    L.rsbwt_set_overlap_last_work(w)
    assert list(w) == [0] * 6  # the failed calls above did no work
    if none:
        runs = np.array([(0 << 5) | 1, (1 << 5) | 3], np.uint8)
        with pytest.raises(rsb.RsbwtError) as e:
            with rsb.GpuBWT(runs=runs, num_strings=1) as g:
                g.overlaps(["ACGT"], 1)
        assert e.value.code == -5 and "no CPU fallback" in str(e.value)
