"""CPU guards for the site-sample-counts tests: tests/site_reference.py's restatement by head ordinal against its statement
by string, on the batch tests/test_gpu_site_counts.py asks; the classes that batch must reach; the shared length rule
(readserver_amd/csrc/gt_span_rule.h) as a program of its own under the address and undefined-behaviour sanitizers, held to
gt_reference's words; and the boundary of the call without a GPU."""
import ctypes as C
import os
import re
import shutil
import subprocess
from collections import Counter

import numpy as np
import pytest

import gt_reference as G
import ksw_reference as kr
import meta_reference as MR
import sample_reference as SR
import site_reference as SITE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, False), (2, True), (8, True)]
_CASES = {}


class Case:
    def __init__(self, oracle, ss, other):
        fx = G.fixture()
        self.fx, self.ss, self.other = fx, ss, other
        self.uni, self.outside = SR.universe(ss)
        self.pairs, self.info = SR.sample_pairs(fx.shards, self.uni, self.outside, ss, other)
        self.side = SITE.Side(oracle, fx.shards, fx.runs(), self.pairs, ("gt", ss, other))
        self.reqs, self.alleles = SITE.batch(fx)
        self.codes = self.uni[:30:3] + self.uni[40:42]


def case(oracle, ss=2, other=True):
    if (ss, other) not in _CASES:
        _CASES[(ss, other)] = Case(oracle, ss, other)
    return _CASES[(ss, other)]


@pytest.mark.parametrize("ss,other", SHAPES)
def test_by_head_ordinal_means_by_string(oracle, ss, other):
    """the two statements agree on all four outputs and the four work numbers they share, for the twelve parameter sets;
    and the walk over rows finds the same candidates with a head"""
    c = case(oracle, ss, other)
    for M, k, skip in G.PARAMS:
        a = SITE.counts_by_ordinal(c.side, c.reqs, k, skip, M, c.codes, ss, other)
        b = SITE.counts_by_string(c.side, c.reqs, k, skip, M, c.codes, ss, other)
        assert SITE.same(a, b) is None, (M, k, skip, SITE.same(a, b))
        assert a["work"]["carriers"] > 20 and a["work"]["aligned"] > a["work"]["carriers"]
        if ss == 2:
            work, items = SITE.rows_by_ordinal(c.side, c.reqs, k, skip, M)
            per = np.zeros(len(c.reqs), np.uint64)
            for (q, _, _), (_, rows) in items.items():
                per[q] += any(stays for _, stays in rows)
            assert (per == a["aligned"]).all(), (M, k, skip)
            assert work["candidates"] > work["kept"] > work["head_rows"] > work["extracted"] > 0


def test_the_batch_reaches_every_class(oracle):
    """fails if the inputs miss a class the GPU tests count on (include/rsbwt.h's definition, case by case)"""
    c = case(oracle)
    named = {w for w, _ in c.pairs if MR.searchable(w)}
    R = SR.rec_size(2, True)
    carried_rungs, hit = set(), Counter()
    for M, k, skip in ((3, 8, 3), (1, 12, 0)):
        a = SITE.counts_by_ordinal(c.side, c.reqs, k, skip, M, c.codes, 2, True)
        exp = c.side.expected(c.reqs, k, skip, M)
        work, items = SITE.rows_by_ordinal(c.side, c.reqs, k, skip, M)
        cand = [(q, p, s) for q in range(len(c.reqs)) for p in range(2) for _, s in exp[q][p][1]]
        # a candidate no pair names; a string with copies > 1; a carrier in both shards
        hit["no pair"] |= any(s not in named for _, _, s in cand)
        hit["copies > 1"] |= any(c.fx.shards[p].count(s) > 1 and s in named for _, p, s in cand)
        kept = {(q, p, s) for q, p, s in cand if s in named and SITE.keeps(s, *c.reqs[q])}
        hit["both shards"] |= any((q, 1 - p, s) in kept for q, p, s in kept)
        # a request with candidates and no carrier: pos = 0
        zero = [q for q, r in enumerate(c.reqs) if r[1] == 0 and r[0]]
        assert zero and all(a["aligned"][q] > 0 and a["carriers"][q] == 0 for q in zero)
        # a read reached through several rows; a pending row that fails beside a row of the same read that passes; a read all
        # of whose rows fail
        hit["several rows"] |= any(len(rows) > 1 for _, rows in items.values())
        hit["fails beside passes"] |= any(any(p and not st for p, st in rows) and any(st for _, st in rows) for _, rows in items.values())
        hit["all fail"] |= any(not any(st for _, st in rows) for _, rows in items.values())
        # ... and, for the min / max mutant: pending rows only, one failing and one passing
        hit["two needs"] |= any(any(not st for _, st in rows) and any(st for _, st in rows) and all(p for p, _ in rows) for _, rows in items.values())
        # a read shared by two requests
        hit["shared read"] |= work["extracted"] < len(items)
        # a candidate with a value that leaves align_gt_read by the mismatch at the site (the exit next to the KEEPs)
        hit["site mismatch"] |= any(s in named and kr.align_gt_read(s, *c.reqs[q]) == 8 for q, _, s in cand)
        # the allele pairs: at least 6 with both alleles carried, the two alleles' carriers disjoint in all 8
        assert len(c.alleles) == 8
        both = 0
        for qa, qb in c.alleles:
            ka, kb = ({(p, s) for q, p, s in kept if q == x} for x in (qa, qb))
            assert not ka & kb
            both += bool(ka) and bool(kb)
        assert both >= 6, both
        # a record with an unknown code; every rung of the ladder among the carried values
        assert a["work"]["unknown"] > 0 and (a["strings"][:, -1] > 0).any()
        vals = dict((w, v) for w, v in c.pairs if MR.searchable(w))
        carried_rungs |= {len(vals[s]) // R for _, _, s in kept}
    assert len(hit) == 9 and all(hit.values()), dict(hit)
    assert carried_rungs >= set(SR.LADDER), sorted(set(SR.LADDER) - carried_rungs)


def test_length_rule_header_under_address_and_ub_sanitizers(tmp_path):
    """tests/native/gt_span_rule_host.cpp: gt_left_row_stays is gt_reference's test of a LEFT row, and the row stays iff the
    read reaches gt_left_needed_len, on every small (pos, end, offset, k, len) with len >= offset + k -- pos < end, where the
    left side wraps, included -- and at the far end of the 64-bit range"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "gt_span_rule_host")
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(ROOT, "tests", "native", "gt_span_rule_host.cpp"), "-o", exe], capture_output=True, text=True)
    if b.returncode != 0 and "sanitize" in b.stderr:
        pytest.skip("no sanitizer runtime here")
    assert b.returncode == 0, b.stderr
    r = subprocess.run([exe, "14", "5", "4", "12"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("gt_span_rule ok"), r.stdout[-2000:] + r.stderr[-3000:]
    lines = r.stdout.splitlines()[:-1]
    assert len(lines) == 15 * 15 * 6 * 4 * 13 + 4
    seen = set()
    for ln in lines:
        pos, end, offset, k, n, stays, need = (int(x) for x in ln.split())
        assert bool(stays) == SITE.left_row_stays(pos, end, offset, k, n), ln
        assert bool(stays) == (n >= need), ln
        seen.add((bool(stays), pos < end))
    assert seen == {(True, False), (False, False), (False, True)}  # both answers, and the wrap (which keeps no read)


def test_the_call_is_declared_bound_and_refuses_without_a_gpu(rsb):
    from readserver_amd import _native
    txt = open(os.path.join(ROOT, "include", "rsbwt.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name, nargs in (("rsbwt_set_site_sample_counts", 18), ("rsbwt_set_site_last_work", 1), ("rsbwt_set_site_last_times", 1)):
        m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, txt, flags=re.S)
        assert m and len(m.group(1).split(",")) == nargs == len(_native.SIGNATURES[name][1]), name
    L = rsb.lib()
    w = np.full(10, 7, np.uint64)
    L.rsbwt_set_site_last_work(None)
    L.rsbwt_set_site_last_work(w.ctypes.data_as(C.POINTER(C.c_uint64)))
    assert not w.any()
    assert L.rsbwt_set_site_sample_counts(None, None, None, 0, None, None, None, 8, 0, 0, None, 0, 2, 1, None, None, None, None) == -1
    assert hasattr(rsb.ShardSet, "site_sample_counts") and hasattr(rsb.ShardSet, "site_last_work")
