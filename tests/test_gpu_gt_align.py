"""align_gt_read on the GPU (-m gpu): rsbwt_gt_align / rsbwt_gt_align_dev and the composed rsbwt_set_gt_aligned_reads /
_count (csrc/ksw_align.hip, csrc/sets.hip) held to tests/ksw_reference.py: the verdict batch that
tests/test_ksw_reference.py shows to reach all thirteen exits, and the gt fixture's candidate reads (tests/gt_reference.py)
filtered by the restatement."""
import ctypes as C

import numpy as np
import pytest

import gt_reference as G
import ksw_reference as kr

pytestmark = pytest.mark.gpu


def test_verdicts_and_counters_equal_the_restatement(rsb):
    reads, item, requests, codes, cnt = kr.verdicts()
    got = rsb.gt_align(reads, item, requests)
    bad = [i for i in range(len(reads)) if int(got[i]) != codes[i]]
    assert not bad, (len(bad), bad[0], int(got[bad[0]]), codes[bad[0]], reads[bad[0]], requests[item[bad[0]]])
    wk = rsb.gt_align_last_work()
    assert wk["reads"] == len(reads) and wk["by_verdict"] == {v: cnt[v] for v in range(1, 14)}
    # in another order (the host orders by length anyway), and a lone read
    order = np.random.default_rng(3).permutation(len(reads))
    got2 = rsb.gt_align([reads[i] for i in order], [item[i] for i in order], requests)
    assert [int(x) for x in got2] == [codes[i] for i in order]
    assert int(rsb.gt_align(reads[:1], item[:1], requests)[0]) == codes[0] and rsb.gt_align_last_work()["reads"] == 1


def test_verdicts_through_the_device_call(rsb):
    """every array in HBM, the caller's order, the verdicts inside guard bytes; a read of a request that does not exist
    gets RSBWT_GT_INVALID"""
    import torch
    L = rsb.lib()
    reads, item, requests, codes, _ = kr.verdicts()
    reads, item, codes = reads + ["ACGTACGT"], item + [len(requests)], codes + [255]
    n, Q, PAD = len(reads), len(requests), 256
    rtext, roff = rsb.bwt._texts(reads)
    text, off = rsb.bwt._texts([r[0] for r in requests])
    pos = np.array([r[1] for r in requests], np.uint64)
    alt = np.frombuffer("".join(r[2] for r in requests).encode(), np.uint8).copy()
    isalt = np.array([r[3] for r in requests], np.uint8)
    d = [torch.from_numpy(np.ascontiguousarray(a).view(np.uint8)).cuda() for a in (rtext, roff, np.array(item, np.uint64), text, off, pos, alt, isalt)]
    out = torch.full((PAD + n + PAD,), 0xAB, dtype=torch.uint8, device="cuda")
    p = lambda t, byte=0: C.c_void_p(t.data_ptr() + byte)  # noqa: E731
    assert L.rsbwt_gt_align_dev(p(d[0]), p(d[1]), p(d[2]), n, p(d[3]), p(d[4]), p(d[5]), p(d[6]), p(d[7]), Q, p(out, PAD), 0, None) == 0, L.rsbwt_last_error()
    torch.cuda.synchronize()
    hb = out.cpu().numpy()
    assert (hb[:PAD] == 0xAB).all() and (hb[PAD + n:] == 0xAB).all()
    assert [int(x) for x in hb[PAD:PAD + n]] == codes


def test_windows_longer_than_the_lds_column(rsb):
    """a 300-symbol window puts the column in HBM (the sub-alignments lay a piece of the window on the rows); 224 and 225 are
    the two sides of the switch"""
    rng = np.random.default_rng(300)
    rnd = lambda n: "".join("ACGT"[c] for c in rng.integers(0, 4, n))  # noqa: E731
    requests, reads, item = [], [], []
    for L_ in (224, 225, 300):
        w = rnd(L_)
        for pos in (60, L_ - 50):
            requests.append((w, pos, "ACGT"[("ACGT".index(w[pos - 1]) + 1) % 4], 0))
            for site in (25, 45):  # more of the read right of the site, then left of it: both sub-alignments
                base = w[pos - 1 - site:pos - 1 - site + 70]
                for s in (base, base[:12] + base[14:], base[:58] + "T" + base[58:], base[:site] + "ACGT"[("ACGT".index(base[site]) + 1) % 4] + base[site + 1:],
                          base[:12] + "A" + base[12:]):
                    reads.append(s)
                    item.append(len(requests) - 1)
    want = [kr.align_gt_read(s, requests[r][0], requests[r][1], requests[r][2], requests[r][3]) for s, r in zip(reads, item)]
    assert {2, 9, 11, 13} <= set(want)
    assert [int(x) for x in rsb.gt_align(reads, item, requests)] == want


# ---- the composed call on the gt fixture: gt_reference's reads for (q, p), cut down by the restatement
_KEEP = {}


def _keeps(s, w, pos, alt, isalt):
    at = (s, w, pos, alt, isalt)
    if at not in _KEEP:
        _KEEP[at] = kr.align_gt_read(s, w, pos, alt, isalt) in kr.GT_KEEP
    return _KEEP[at]


@pytest.fixture(scope="module")
def ref(oracle):
    fx = G.fixture()
    g = fx.haps[1]
    qs = fx.queries() + [(g[100:179], 0), (g[1500:1579], 80)]  # pos = 0 and pos = L + 1
    alts = []
    for i, (w, pos) in enumerate(qs):
        c = w[pos - 1] if 1 <= pos <= len(w) else "A"
        # the alt allele: the next base for most, the reference base itself for some (then ra = r), an N for a few
        alts.append(("N" if i % 7 == 6 else c if i % 5 == 4 else "ACGT"[("ACGT".find(c) + 1) % 4], i % 2))
    return fx, [G.OracleShard(oracle.from_runs(r, len(sh))) for sh, r in zip(fx.shards, fx.runs())], qs, alts


def _open(rsb, fx, devices=(0, 0)):
    return [rsb.GpuBWT(runs=runs, num_strings=len(sh), ktab_depth=6, for_reads=True, device=d) for d, sh, runs in zip(devices, fx.shards, fx.runs())]


def _close(ss, gs):
    ss.close()
    for g in gs:
        g.close()


def _check(ss, rsb, ref, M, k, skip, where, stride=256):
    fx, orc, qs, alts = ref
    exp = G.expected(orc, "fixture+sites", qs, k, skip, M)
    ws, ps, al, ia = [w for w, _ in qs], [p for _, p in qs], [a for a, _ in alts], [i for _, i in alts]
    got = ss.gt_aligned_reads(ws, ps, al, ia, k, skip, M, read_stride=stride, with_rows=True)
    wk = rsb.gt_align_last_work()
    cnt = ss.gt_aligned_count(ws, ps, al, ia, k, skip, M)
    kept = aligned = 0
    for q, (w, pos) in enumerate(qs):
        for p in range(2):
            want = [(row, s) for row, s in exp[q][p][1] if _keeps(s, w, pos, al[q], ia[q])]
            assert got[q][p] == want, (where, M, k, skip, q, p, pos)
            assert int(cnt[q, p]) == len(want), (where, M, k, skip, q, p)
            kept += len(want)
            aligned += len(exp[q][p][1])
    assert wk["reads"] == aligned and sum(wk["by_verdict"][v] for v in kr.GT_KEEP) == kept, (where, wk)
    assert rsb.gt_align_last_work() == wk  # (the count call does the same work)
    return kept, aligned


@pytest.mark.parametrize("M,k,skip", G.PARAMS)
def test_aligned_reads_equal_the_filtered_candidates(rsb, ref, M, k, skip):
    gs = _open(rsb, ref[0])
    ss = rsb.ShardSet(gs)
    try:
        kept, aligned = _check(ss, rsb, ref, M, k, skip, "one group")
        assert 0 < kept < aligned
    finally:
        _close(ss, gs)


@pytest.mark.parametrize("stride", [128, 640])
def test_aligned_reads_on_two_device_groups_at_two_strides(rsb, ref, monkeypatch, stride):
    """each group aligns the reads of its own shard against the requests that have a read there; the one-group answers"""
    L = rsb.lib()
    if L.rsbwt_device_count() < 2:
        monkeypatch.setenv("RSBWT_ENABLE_TEST_HOOKS", "1")
        monkeypatch.setenv("RSBWT_TEST_DEVICE_ALIASES", "2")
    gs = _open(rsb, ref[0], devices=(0, 1))
    ss = rsb.ShardSet(gs)
    try:
        assert L.rsbwt_set_devices(ss._s) == 2
        for M, k, skip in ((3, 8, 3), (1, 12, 0)):
            _check(ss, rsb, ref, M, k, skip, "two groups", stride)
    finally:
        _close(ss, gs)
    gs = _open(rsb, ref[0])
    ss = rsb.ShardSet(gs)
    try:
        _check(ss, rsb, ref, 3, 8, 3, "one group", stride)
    finally:
        _close(ss, gs)


def test_sizing_protocol_and_off_site_requests(rsb, ref):
    """cap_reads = 0 sizes the buffers (RSBWT_ERANGE with the count set), one short is refused, the exact one is filled;
    the requests with pos = 0 and pos = L + 1 keep no read although pos = 0 has candidates"""
    fx, orc, qs, alts = ref
    L = rsb.lib()
    gs = _open(rsb, fx)
    ss = rsb.ShardSet(gs)
    pv = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    try:
        text, off = ss._var_text([w for w, _ in qs])
        pos, alt, isalt = ss._gt_requests([w for w, _ in qs], [p for _, p in qs], [a for a, _ in alts], [i for _, i in alts])
        Q = len(qs)
        exp = G.expected(orc, "fixture+sites", qs, 8, 3, 3)
        flat = [s for q, (w, ps) in enumerate(qs) for p in range(2) for _, s in exp[q][p][1] if _keeps(s, w, ps, alts[q][0], alts[q][1])]
        n = C.c_size_t()
        first = np.zeros(2 * Q + 1, np.uint64)
        args = (ss._s, pv(text), pv(off), Q, pv(pos), pv(alt), pv(isalt), 8, 3, 3, pv(first))
        assert L.rsbwt_set_gt_aligned_reads(*args, None, 64, None, None, 0, C.byref(n)) == -7 and n.value == len(flat) > 0
        assert int(first[2 * Q]) == len(flat)
        reads = np.zeros((len(flat), 64), np.uint8)
        ln = np.zeros(len(flat), np.uint32)
        assert L.rsbwt_set_gt_aligned_reads(*args, pv(reads), 64, pv(ln), None, len(flat) - 1, C.byref(n)) == -7
        assert L.rsbwt_set_gt_aligned_reads(*args, pv(reads), 64, pv(ln), None, len(flat), C.byref(n)) == 0
        assert [reads[r, :ln[r]].tobytes().decode() for r in range(len(flat))] == flat
        zero_q, past_q = Q - 2, Q - 1
        assert qs[zero_q][1] == 0 and qs[past_q][1] == len(qs[past_q][0]) + 1
        assert sum(len(exp[zero_q][p][1]) for p in range(2)) > 0, "pos = 0 has candidates: the alignment is what drops them"
        assert all(first[2 * q] == first[2 * q + 2] for q in (zero_q, past_q))
        cand = ss.gt_count([w for w, _ in qs], pos, 8, 3, 3)
        assert ss.gt_aligned_count([w for w, _ in qs], pos, [a for a, _ in alts], isalt, 8, 3, 3).sum() == len(flat) < cand.sum()
        assert rsb.gt_align_last_work()["by_verdict"][3] >= int(cand[zero_q].sum())
    finally:
        _close(ss, gs)
