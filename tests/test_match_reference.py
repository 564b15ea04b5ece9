"""CPU guards for the matching-statistics tests: tests/match_reference.py's restatement over the oracle's BWT against its
computation with no BWT, the coverage of the inputs tests/test_gpu_match.py runs on the GPU, the two properties the kernel
leans on (W never grows with l; SMEM starts strictly increase), and the boundary of the calls without a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import gt_reference as G
import match_reference as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = {"rsbwt_set_match_lengths": 9, "rsbwt_set_match_lengths_dev": 10, "rsbwt_set_smems": 10, "rsbwt_match_lengths": 9,
         "rsbwt_set_match_last_work": 1}
DEPTHS = (6, 10)  # the k-mer table depths the GPU tests use


@pytest.fixture(scope="module")
def sides(oracle):
    fx = G.fixture()
    orc = [G.OracleShard(oracle.from_runs(r, len(sh))) for sh, r in zip(fx.shards, fx.runs())]
    return fx, orc, [M.PlainCounts(sh) for sh in fx.shards]


def test_the_queries_are_the_issues(sides):
    qs = M.queries()
    fx = sides[0]
    assert sum(len(w) for w in qs) == 800 and len(fx.shards) == 2
    assert [len(w) for w in qs] == [79] * 6 + [60] * 3 + [40, 80, 0, 1, 1, 24]
    assert qs[5][30] == "N" and qs[13] == "N" and sum(w.count("N") for w in qs) == 2


@pytest.mark.parametrize("max_len,min_rows", M.PARAMS)
def test_restatement_agrees_with_the_computation_without_a_bwt(sides, max_len, min_rows):
    """all 1,600 items: len, lower and upper"""
    fx, orc, plain = sides
    qs = M.queries()
    exp = M.expected(orc, "fixture", qs, max_len, min_rows)
    items = 0
    for p in range(2):
        assert orc[p].oix.bwlen() == plain[p].n
        for q, w in enumerate(qs):
            for e in range(1, len(w) + 1):
                assert exp[p][q][e - 1] == plain[p].longest(w, e, max_len, max(min_rows, 1)), (p, q, e)
                items += 1
    assert items == 1600


@pytest.mark.parametrize("max_len,min_rows", M.PARAMS)
def test_the_inputs_reach_every_class(sides, max_len, min_rows):
    """the coverage guard: lengths below, equal to and above both table depths, 40 (a whole read), 0, matches that reach
    the query's start, and matches the cap stops"""
    fx, orc, _ = sides
    qs = M.queries()
    exp = M.expected(orc, "fixture", qs, max_len, min_rows)
    ls = [(l, e + 1) for p in range(2) for per in exp[p] for e, (l, _, _) in enumerate(per)]
    assert len(ls) == 1600
    cls = {"zero": sum(l == 0 for l, _ in ls), "whole": sum(l == e for l, e in ls)}
    for T in DEPTHS:
        cls[f"0<l<{T}"] = sum(0 < l < T for l, _ in ls)
        cls[f"l=={T}"] = sum(l == T for l, _ in ls)
        cls[f"l>{T}"] = sum(l > T for l, _ in ls)
    cls["6<l<10"] = sum(6 < l < 10 for l, _ in ls)
    if max_len:
        cls["capped"] = sum(l == max_len < e for l, e in ls)
        assert max(l for l, _ in ls) == max_len
    else:
        cls["l==40"] = sum(l == G.READ_LEN for l, _ in ls)
    assert all(v > 0 for v in cls.values()), cls
    # the two positions that hold an N, in both shards -- and nothing else when one row is enough for a symbol
    assert cls["zero"] >= 4 and (min_rows > 1 or cls["zero"] == 4), cls
    recs, first = M.smem_records(exp)
    assert 0 < len(recs) < 1600 and first[-1] == len(recs)


def test_w_never_grows_with_l(sides):
    """W(text[t-l+1 .. t]) over EVERY l up to the end's position, not only up to the first failure: non-increasing, so the
    first failing step is where the longest match ends"""
    fx, orc, _ = sides
    seen = 0
    for sh in orc:
        n = sh.oix.bwlen()
        for w in M.queries():
            for e in range(1, len(w) + 1):
                prev = None
                for l in range(1, e + 1):
                    W = M.width(sh.find(w[e - l:e]), n)
                    assert prev is None or W <= prev, (w, e, l)
                    prev = W
                    seen += 1
    assert seen > 30000


@pytest.mark.parametrize("max_len,min_rows", M.PARAMS)
def test_smem_starts_strictly_increase(sides, max_len, min_rows):
    fx, orc, _ = sides
    exp = M.expected(orc, "fixture", M.queries(), max_len, min_rows)
    for p in range(2):
        for per in exp[p]:
            starts = [t + 1 - l for t, (l, _, _) in enumerate(per) if l > 0]
            assert starts == sorted(starts)  # the starts t - len never decrease along a query
            sm = M.smems_of(per)
            assert all(a[0] < b[0] and a[1] < b[1] for a, b in zip(sm, sm[1:]))
            # every match lies inside a SMEM of its query
            for t, (l, _, _) in enumerate(per):
                assert l == 0 or any(s <= t + 1 - l and t + 1 <= e for s, e, _, _ in sm)


def test_entry_points_are_declared_exported_and_bound_and_no_gpu_is_enodev(rsb):
    from readserver_amd import _native
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rsbwt.h")).read(), flags=re.S)
    L = C.CDLL(rsb.lib_path())
    for n, nargs in ENTRY.items():
        assert re.search(r"\b%s\s*\(" % n, txt), f"{n} is not declared in include/rsbwt.h"
        assert n in _native.SIGNATURES and hasattr(L, n) and hasattr(rsb.lib(), n)
        assert len(_native.SIGNATURES[n][1]) == nargs, n
    assert "typedef struct rsbwt_smem" in txt and rsb.bwt.SMEM.itemsize == 40
    assert callable(rsb.GpuBWT.match_lengths) and callable(rsb.ShardSet.match_lengths) and callable(rsb.ShardSet.smems)
    assert callable(rsb.ShardSet.match_last_work)
    L = rsb.lib()
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    text = np.frombuffer(b"ACGTACGT", np.uint8).copy()
    off = np.array([0, 4, 8], np.uint64)
    ln = np.full(8, 77, np.uint32)
    n = C.c_size_t(77)
    first = np.zeros(3, np.uint64)
    none = L.rsbwt_device_count() == 0
    # a box without a GPU can have no set: RSBWT_ENODEV, no CPU fallback; where there is one a null set is RSBWT_EINVAL
    want = -5 if none else -1
    assert L.rsbwt_set_match_lengths(None, p(text), p(off), 2, 0, 1, p(ln), None, None) == want
    assert (b"no CPU fallback" if none else b"null") in L.rsbwt_last_error()
    assert L.rsbwt_match_lengths(None, p(text), p(off), 2, 0, 1, p(ln), None, None) == want
    assert L.rsbwt_set_smems(None, p(text), p(off), 2, 0, 1, p(first), None, 0, C.byref(n)) == want and n.value == 0
    assert L.rsbwt_set_match_lengths_dev(None, None, None, 0, 0, 0, 1, None, None, None) == -1
    assert (ln == 77).all()
    w = (C.c_uint64 * 6)(*([9] * 6))
    L.rsbwt_set_match_last_work(None)  # (nothing to write to: no crash)
    L.rsbwt_set_match_last_work(w)
    assert list(w) == [0] * 6  # the failed calls above did no work
    if none:
        runs = np.array([(0 << 5) | 1, (1 << 5) | 3], np.uint8)
        with pytest.raises(rsb.RsbwtError) as e:
            with rsb.GpuBWT(runs=runs, num_strings=1) as g:
                g.match_lengths(["ACGT"])
        assert e.value.code == -5 and "no CPU fallback" in str(e.value)
