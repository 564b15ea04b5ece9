"""Slices of rsbwt_set_site_sample_counts and rsbwt_set_sample_counts (-m gpu): both calls cut a batch where
Q x (C + 1) passes 2^27 cells (set_site_counts_body, set_sample_counts_body in csrc/sets.hip).  A dictionary of 131,071
three-byte codes makes the width 2^17 and a slice 1,024 requests; a batch of 1,024 + 65 is two slices, so the second runs
with q0 = 1,024: the rebased offsets, text + off[q0], pos / alt / isalt + q0, the output pointers + q0 * width, and the work
counters added over the slices.  Everything is on the gt fixture.

The expected values are the restatement's answer for the usual 12 codes, scattered to the columns those codes have in the
big dictionary; no value in the table holds any of the other 131,059 codes (asserted), so everything else is the last
column.  No dense (Q, 2^17) reference is built: the outputs are compared by their nonzero positions."""
import ctypes as C

import numpy as np
import pytest

import sample_reference as SR
import site_reference as SITE
import test_gpu_sample_counts as SAMPLE
import test_gpu_site_counts as SITES

pytestmark = pytest.mark.gpu

SS, OTHER = 3, True
BIG = 131071                 # codes: the width is 2^17, and a slice is 2^27 / 2^17 = 1,024 requests
SLICE, Q = 1024, 1024 + 65
M, K, SKIP = 3, 8, 3
pv = lambda x: x.ctypes.data_as(C.c_void_p) if x is not None else None  # noqa: E731


def _cycle(base):
    out = [base[i % len(base)] for i in range(Q)]
    assert all(out[i] != out[i + SLICE] for i in range(Q - SLICE))
    return out


class Big:
    """the 12 codes among 131,071, ascending as the C ABI takes them; col[j] = the column of the caller's j-th code"""

    def __init__(self, codes, pairs):
        held = {v[i:i + SS] for _, v in pairs for i in range(0, len(v) - len(v) % (SS + 2), SS + 2)}
        rng = np.random.default_rng(131071)
        mine = {SR.key_of(c) for c in codes}
        rest = [int(x) for x in rng.choice(1 << 24, BIG + 4096, replace=False) if int(x) not in mine and int(x).to_bytes(3, "big") not in held]
        keys = np.array(sorted(mine | set(rest[:BIG - len(mine)])), np.uint64)
        others = {int(x).to_bytes(3, "big") for x in keys} - set(codes)
        assert len(keys) == BIG and len(others) == BIG - len(codes) and not others & held  # no value of the table holds them
        self.flat = np.frombuffer(b"".join(int(x).to_bytes(3, "big") for x in keys) + b"\0", np.uint8).copy()
        self.col = np.append(np.searchsorted(keys, np.array([SR.key_of(c) for c in codes], np.uint64)), BIG).astype(np.int64)
        assert len(set(self.col.tolist())) == len(codes) + 1


def _same_cells(got, want13, col, what):
    """got (Q, 2^17) against want13 (Q, 13) scattered to the columns col: the nonzero cells, their places and values"""
    q, c = np.nonzero(want13)
    order = np.lexsort((col[c], q))
    wq, wc, wv = q[order], col[c][order], want13[q, c][order]
    gq, gc = np.nonzero(got)
    assert len(gq) == len(wq), (what, len(gq), len(wq))
    assert (gq == wq).all() and (gc == wc).all() and (got[gq, gc] == wv).all(), what
    assert (wq < SLICE).any() and (wq >= SLICE).any()


@pytest.fixture(scope="module")
def site_case(oracle):
    r = SITES.Ref(oracle, SS, OTHER)
    n = len(r.reqs)
    reqs = _cycle(r.reqs)
    base, head = r.want(M, K, SKIP), r.want(M, K, SKIP, reqs=r.reqs[:Q % n])
    want = {k: base[k][np.arange(Q) % n] for k in SITES.OUT}
    # every number but `extracted` is a sum over requests: Q // n whole rounds of the batch and its first Q % n requests;
    # `extracted` counts a slice's distinct reads, and both slices hold every request of the batch: twice the batch's
    assert SLICE >= n and Q - SLICE >= n
    want["work"] = {k: (Q // n) * base["work"][k] + head["work"][k] for k in base["work"]}
    want["work"]["extracted"] = 2 * base["work"]["extracted"]
    return r, reqs, want, Big(r.codes, r.pairs)


def _site_call(ss, rsb, reqs, flat, ncodes, strings=None, copies=None, aligned=None, carriers=None):
    ws, ps, al, ia = SITES._cols(reqs)
    text, off = ss._var_text(ws)
    pos, alt, isalt = ss._gt_requests(ws, ps, al, ia)
    rc = rsb.lib().rsbwt_set_site_sample_counts(ss._s, pv(text), pv(off), len(reqs), pv(pos), pv(alt), pv(isalt), K, SKIP, M, pv(flat), ncodes, SS,
                                                1 if OTHER else 0, pv(strings), pv(copies), pv(aligned), pv(carriers))
    assert rc == 0, rsb.lib().rsbwt_last_error()
    return rsb.ShardSet.site_last_work()


def _site_work(ss, rsb, reqs, work, want):
    assert SITE.same(dict(want, work=work), want) is None, SITE.same(dict(want, work=work), want)
    ws, ps, _, _ = SITES._cols(reqs)
    ss.gt_count(ws, ps, K, SKIP, M)
    gw = rsb.ShardSet.gt_last_work()
    assert [work[x] for x in ("legs", "narrow_steps", "candidates", "kept")] == [gw[x] for x in ("legs", "narrow_steps", "candidates", "kept")], gw


@pytest.fixture(scope="module")
def site_set(rsb, site_case):
    r = site_case[0]
    gs = SITES._open(rsb, r)
    ss = rsb.ShardSet(gs)
    SITES._build(ss, r.pairs)
    yield ss
    SITES._close(ss, gs)


def test_gpu_site_counts_two_slices_vectors(rsb, site_case, site_set):
    """aligned and carriers alone over two slices, the work counters their sums; the same batch under the 12 codes is one
    slice and gives the same vectors"""
    r, reqs, want, big = site_case
    al, ca = np.full(Q, 7, np.uint64), np.full(Q, 7, np.uint64)
    work = _site_call(site_set, rsb, reqs, big.flat, BIG, aligned=al, carriers=ca)
    assert (al == want["aligned"]).all() and (ca == want["carriers"]).all()
    assert (ca[:SLICE] > 0).any() and (ca[SLICE:] > 0).any() and (al[SLICE:] != al[:Q - SLICE]).any()
    _site_work(site_set, rsb, reqs, work, want)
    one = SITES._got(site_set, rsb, r, M, K, SKIP, reqs=reqs)
    assert (one["aligned"] == al).all() and (one["carriers"] == ca).all()
    assert (one["strings"] == want["strings"]).all() and (one["copies"] == want["copies"]).all()
    # ... whose `extracted` is one slice's: the batch's distinct reads once
    assert one["work"]["extracted"] * 2 == work["extracted"] and all(one["work"][k] == work[k] for k in SITES.KEYS if k != "extracted")


def test_gpu_site_counts_two_slices_strings(rsb, site_case, site_set):
    r, reqs, want, big = site_case
    st = np.zeros((Q, BIG + 1), np.uint32)
    work = _site_call(site_set, rsb, reqs, big.flat, BIG, strings=st)
    _same_cells(st, want["strings"], big.col, "strings")
    del st
    _site_work(site_set, rsb, reqs, work, want)


def test_gpu_site_counts_two_slices_copies(rsb, site_case, site_set):
    r, reqs, want, big = site_case
    cp = np.zeros((Q, BIG + 1), np.int64)
    work = _site_call(site_set, rsb, reqs, big.flat, BIG, copies=cp)
    _same_cells(cp, want["copies"], big.col, "copies")
    del cp
    _site_work(site_set, rsb, reqs, work, want)


# ---- rsbwt_set_sample_counts ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sample_case(oracle):
    r = SAMPLE.Ref(oracle, "gt", SS, OTHER)
    queries = _cycle(list(dict.fromkeys(r.queries)))  # (each of the batch's strings once)
    return r, queries, r.want(queries), Big(r.codes, r.pairs)  # (work6 is a sum over queries: the restatement's of the cycled batch)


@pytest.fixture(scope="module")
def sample_set(rsb, sample_case):
    r = sample_case[0]
    gs = SAMPLE._open(rsb, r.fx, room=True)
    ss = rsb.ShardSet(gs)
    SAMPLE._build(ss, r.pairs)
    yield ss
    SAMPLE._close(ss, gs)


def _sample_call(ss, rsb, queries, flat, ncodes, want, strings=None, copies=None, matches=None, carriers=None):
    L = rsb.lib()
    text, off = ss._var_text(queries)
    assert L.rsbwt_set_set_counting(ss._s, 1) == 0
    try:
        rc = L.rsbwt_set_sample_counts(ss._s, pv(text), pv(off), len(queries), pv(flat), ncodes, SS, 1 if OTHER else 0, 0, 0, pv(strings), pv(copies),
                                       pv(matches), pv(carriers))
    finally:
        assert L.rsbwt_set_set_counting(ss._s, 0) == 0
    assert rc == 0, L.rsbwt_last_error()
    work = rsb.ShardSet.sample_last_work()
    assert tuple(work) == SAMPLE.KEYS and work == want["work"], (work, want["work"])


def test_gpu_sample_counts_two_slices_vectors(rsb, sample_case, sample_set):
    """matches and carriers alone over two slices, work6 (LF steps included, in counting mode) the sums over both; the
    same batch under the 12 codes is one slice and gives the same vectors"""
    r, queries, want, big = sample_case
    mt, ca = np.full(Q, 7, np.uint64), np.full(Q, 7, np.uint64)
    _sample_call(sample_set, rsb, queries, big.flat, BIG, want, matches=mt, carriers=ca)
    assert (mt == want["matches"]).all() and (ca == want["carriers"]).all()
    assert (ca[:SLICE] > 0).any() and (ca[SLICE:] > 0).any() and (mt[SLICE:] != mt[:Q - SLICE]).any()
    one = SAMPLE._check(sample_set, rsb, r, "one slice", queries=queries)
    assert (one["matches"] == mt).all() and (one["carriers"] == ca).all()


def test_gpu_sample_counts_two_slices_strings(rsb, sample_case, sample_set):
    r, queries, want, big = sample_case
    st = np.zeros((Q, BIG + 1), np.uint32)
    _sample_call(sample_set, rsb, queries, big.flat, BIG, want, strings=st)
    _same_cells(st, want["strings"], big.col, "strings")


def test_gpu_sample_counts_two_slices_copies(rsb, sample_case, sample_set):
    r, queries, want, big = sample_case
    cp = np.zeros((Q, BIG + 1), np.int64)
    _sample_call(sample_set, rsb, queries, big.flat, BIG, want, copies=cp)
    _same_cells(cp, want["copies"], big.col, "copies")
