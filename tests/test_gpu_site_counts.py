"""Site sample counts on the GPU (-m gpu): rsbwt_set_site_sample_counts / rsbwt_set_site_last_work (csrc/site_counts.hip,
csrc/sets.hip) held bit-exactly to tests/site_reference.py, the definition restated from the gt, sample and ksw
restatements.  tests/test_site_reference.py shows on the CPU that the inputs reach every class and that "by head ordinal"
means "by string".  Everything is on the gt fixture (560 reads of 40 symbols, 2 shards) unless said."""
import ctypes as C
import random
import threading

import numpy as np
import pytest

import gt_reference as G
import sample_reference as SR
import site_reference as SITE
from kmer_reference import _bwt_runs

pytestmark = pytest.mark.gpu

SPANS = {"control": 40, "chunk": 128, "far": 300, "chain": 600, "deep": 2944}  # tests/test_gpu_sample_counts.py's
KEYS = SITE.WORK_KEYS
OUT = ("strings", "copies", "aligned", "carriers")


class Ref:
    """one read set under one record shape: the pairs, the restatement's side, the batch, a dictionary of 12 codes in an
    order that is not ascending, and the answers -- computed once, never changed"""

    def __init__(self, oracle, ss=2, other=True, shards=None, runs=None, name="gt", reqs=None):
        fx = G.fixture()
        self.shards = fx.shards if shards is None else shards
        self.runs = fx.runs() if runs is None else runs
        self.ss, self.other = ss, other
        self.uni, self.outside = SR.universe(ss)
        self.pairs, self.info = SR.sample_pairs(self.shards, self.uni, self.outside, ss, other)
        self.side = SITE.Side(oracle, self.shards, self.runs, self.pairs, (name, ss, other))
        self.reqs, self.alleles = SITE.batch(fx) if reqs is None else (reqs, [])
        self.codes = self.uni[:30:3] + self.uni[40:42]
        self._memo = {}

    def want(self, M, k, skip, reqs=None, codes=None):
        reqs = self.reqs if reqs is None else reqs
        codes = self.codes if codes is None else codes
        key = (M, k, skip, tuple(reqs), tuple(codes))
        if key not in self._memo:
            self._memo[key] = SITE.want(self.side, reqs, k, skip, M, codes, self.ss, self.other)
        return self._memo[key]


@pytest.fixture(scope="module")
def refs(oracle):
    built = {}

    def get(ss=2, other=True):
        if (ss, other) not in built:
            built[(ss, other)] = Ref(oracle, ss, other)
        return built[(ss, other)]
    return get


@pytest.fixture(scope="module")
def ref(refs):
    return refs()


def _open(rsb, r, span=0, ktab=6, devices=None, grouped=False, room=True):
    devices = devices or [0] * len(r.shards)
    return [rsb.GpuBWT(runs=runs, num_strings=len(sh), ktab_depth=ktab, window_span=span, for_reads=room, device=d, ktab_grouped=grouped)
            for d, sh, runs in zip(devices, r.shards, r.runs)]


def _close(ss, gs):
    ss.close()
    for g in gs:
        g.close()


def _build(ss, pairs):
    return ss.meta_build([w for w, _ in pairs], [v for _, v in pairs])


def _cols(reqs):
    return [w for w, _, _, _ in reqs], [p for _, p, _, _ in reqs], [a for _, _, a, _ in reqs], [i for _, _, _, i in reqs]


def _got(ss, rsb, r, M, k, skip, reqs=None, codes=None):
    reqs = r.reqs if reqs is None else reqs
    ws, ps, al, ia = _cols(reqs)
    out = ss.site_sample_counts(ws, ps, al, ia, k, skip, M, codes=r.codes if codes is None else codes, size_of_sample=r.ss,
                                has_other_meta_data=r.other)
    out["work"] = rsb.ShardSet.site_last_work()
    return out


def _check(ss, rsb, r, M, k, skip, where, reqs=None, codes=None):
    """all four outputs and work10: nine numbers against the restatement, and the first four against what the candidate
    call counts on the same set (narrow_steps depends on the k-mer table: rsbwt_set_gt_last_work is its definition)"""
    want = r.want(M, k, skip, reqs, codes)
    got = _got(ss, rsb, r, M, k, skip, reqs, codes)
    assert tuple(got["work"]) == KEYS
    print(where, got["work"])
    assert SITE.same(got, want) is None, (where, SITE.same(got, want))
    ws, ps, _, _ = _cols(r.reqs if reqs is None else reqs)
    ss.gt_count(ws, ps, k, skip, M)
    gw = rsb.ShardSet.gt_last_work()
    assert [got["work"][x] for x in ("legs", "narrow_steps", "candidates", "kept")] == [gw[x] for x in ("legs", "narrow_steps", "candidates", "kept")], (where, gw)
    return got


@pytest.mark.parametrize("M,k,skip", G.PARAMS)
def test_gpu_site_counts_are_the_restatement(rsb, ref, M, k, skip):
    """the twelve parameter sets at 2-byte codes with meta bytes, shards behind 6-mer tables (first in the file: without the
    feature it fails at the binding)"""
    gs = _open(rsb, ref)
    ss = rsb.ShardSet(gs)
    try:
        _build(ss, ref.pairs)
        got = _check(ss, rsb, ref, M, k, skip, (M, k, skip))
        assert got["strings"].dtype == np.uint32 and got["copies"].dtype == np.int64 and got["strings"].shape == (len(ref.reqs), 13)
        wk = got["work"]
        assert wk["candidates"] > wk["kept"] > wk["head_rows"] > wk["aligned"] > wk["carriers"] > 0 and wk["extracted"] < wk["aligned"]
    finally:
        _close(ss, gs)


@pytest.mark.parametrize("ss,other", [(1, False), (4, True), (8, False)])
def test_gpu_site_counts_record_shapes(rsb, refs, ss, other):
    r = refs(ss, other)
    gs = _open(rsb, r)
    ss_ = rsb.ShardSet(gs)
    try:
        _build(ss_, r.pairs)
        _check(ss_, rsb, r, 3, 8, 3, (ss, other))
    finally:
        _close(ss_, gs)


def test_gpu_site_counts_equal_the_composed_calls(rsb, ref):
    """the same matrices from composing existing GPU calls: gt_aligned_reads, then the pairs by string, then a numpy tally"""
    gs = _open(rsb, ref)
    ss = rsb.ShardSet(gs)
    try:
        _build(ss, ref.pairs)
        named = {}
        for read, value in ref.pairs:
            if SITE.MR.searchable(read):
                named[read] = value
        t = SITE._Tally(ref.codes, ref.ss, ref.other)
        ws, ps, al, ia = _cols(ref.reqs)
        for M, k, skip in ((3, 8, 3), (1, 12, 0)):
            got = _got(ss, rsb, ref, M, k, skip)
            cand = ss.gt_reads(ws, ps, k, skip, M)
            kept = ss.gt_aligned_reads(ws, ps, al, ia, k, skip, M)
            Q = len(ws)
            strings, copies = np.zeros((Q, 13), np.uint32), np.zeros((Q, 13), np.int64)
            aligned, carriers = np.zeros(Q, np.uint64), np.zeros(Q, np.uint64)
            for q in range(Q):
                for p in range(2):
                    aligned[q] += sum(1 for s in cand[q][p] if s in named)
                    for s in kept[q][p]:
                        if s in named:
                            st, cp, _, _ = t.parse(named[s])
                            strings[q] += st
                            copies[q] += cp
                            carriers[q] += 1
            assert SITE.same(got, dict(strings=strings, copies=copies, aligned=aligned, carriers=carriers), work=False) is None, (M, k, skip)
    finally:
        _close(ss, gs)


def test_gpu_site_counts_on_two_device_groups(rsb, ref, monkeypatch):
    """two device groups (two logical devices on GPU 0 where the box has one): each group runs its own shard and tallies
    into matrices of its own, the host adds them -- the one-group answers and counters"""
    L = rsb.lib()
    if L.rsbwt_device_count() < 2:
        monkeypatch.setenv("RSBWT_ENABLE_TEST_HOOKS", "1")
        monkeypatch.setenv("RSBWT_TEST_DEVICE_ALIASES", "2")
    gs = _open(rsb, ref, devices=(0, 1))
    ss = rsb.ShardSet(gs)
    try:
        assert L.rsbwt_set_devices(ss._s) == 2
        _build(ss, ref.pairs)
        for M, k, skip in ((3, 8, 3), (1, 12, 0)):
            _check(ss, rsb, ref, M, k, skip, "two groups")
    finally:
        _close(ss, gs)


def test_gpu_site_counts_on_a_group_whose_shards_are_not_adjacent(rsb, oracle, monkeypatch):
    """the fixture's reads split into three shards, shards 0 and 2 on one device group and shard 1 on another"""
    L = rsb.lib()
    if L.rsbwt_device_count() < 2:
        monkeypatch.setenv("RSBWT_ENABLE_TEST_HOOKS", "1")
        monkeypatch.setenv("RSBWT_TEST_DEVICE_ALIASES", "2")
    fx = G.fixture()
    reads = [r for pair in zip(*fx.shards) for r in pair]
    shards = [reads[0::3], reads[1::3], reads[2::3]]
    r = Ref(oracle, shards=shards, runs=[_bwt_runs(sh) for sh in shards], name="gt3")
    gs = _open(rsb, r, devices=(0, 1, 0))
    ss = rsb.ShardSet(gs)
    try:
        assert L.rsbwt_set_devices(ss._s) == 2
        _build(ss, r.pairs)
        got = _check(ss, rsb, r, 3, 8, 3, "three shards, two groups")
        assert got["carriers"].sum() > 0
    finally:
        _close(ss, gs)


@pytest.mark.parametrize("kind", list(SPANS))
@pytest.mark.parametrize("ktab,grouped", [(6, False), (None, False), (6, True)])
def test_gpu_site_counts_on_every_line_layout(rsb, ref, kind, ktab, grouped):
    """window spans 40, 128, 300, 600 and 2,944, with a 6-mer table, with none and with a grouped one"""
    span = SPANS[kind]
    gs = _open(rsb, ref, span=span, ktab=ktab, grouped=grouped)
    ss = rsb.ShardSet(gs)
    try:
        assert all(g.window_span() == span for g in gs)
        _build(ss, ref.pairs)
        _check(ss, rsb, ref, 3, 8, 3, (kind, ktab, grouped))
    finally:
        _close(ss, gs)


def test_gpu_site_counts_batch_sizes_and_shared_reads(rsb, ref):
    """Q in {0, 1, 63, 64, 65} by repeating requests; one allele pair 200 times: 400 requests that share their reads, every
    row the single request's"""
    gs = _open(rsb, ref)
    ss = rsb.ShardSet(gs)
    try:
        _build(ss, ref.pairs)
        for cnt in (0, 1, 63, 64, 65):
            reqs = [ref.reqs[i % len(ref.reqs)] for i in range(cnt)]
            got = _check(ss, rsb, ref, 3, 8, 3, f"Q={cnt}", reqs=reqs)
            assert got["strings"].shape == (cnt, 13) and got["aligned"].shape == (cnt,)
        full = ref.want(3, 8, 3)
        a, b = max(ref.alleles, key=lambda ab: min(full["carriers"][ab[0]], full["carriers"][ab[1]]))
        assert full["carriers"][a] > 0 and full["carriers"][b] > 0
        got = _got(ss, rsb, ref, 3, 8, 3, reqs=[ref.reqs[a], ref.reqs[b]] * 200)
        for k in OUT:
            assert (got[k][0::2] == full[k][a]).all() and (got[k][1::2] == full[k][b]).all(), k
        wk = got["work"]
        assert 0 < wk["extracted"] < wk["aligned"] and wk["aligned"] == 200 * int(full["aligned"][a] + full["aligned"][b])
    finally:
        _close(ss, gs)


def test_gpu_site_counts_dictionary_sizes(rsb, ref):
    """C in {1, 64, 65} and 4,200 codes -- 33,600 bytes of keys, over the 32 KiB the kernel keeps in LDS -- in a shuffled
    order: the columns follow the caller's order, the rest lands in the unknown column"""
    gs = _open(rsb, ref)
    ss = rsb.ShardSet(gs)
    try:
        _build(ss, ref.pairs)
        big = SR.universe(ref.ss, 4200)[0]
        assert big[:70] == ref.uni and 8 * len(big) > 32 << 10
        rng = np.random.default_rng(5)
        base = ref.want(3, 8, 3)
        for n in (1, 64, 65, 4200):
            codes = [big[i] for i in rng.permutation(len(big))[:n]] if n > 65 else [big[i] for i in rng.permutation(70)[:n]]
            got = _check(ss, rsb, ref, 3, 8, 3, f"C={n}", codes=codes)
            assert got["strings"].shape == (len(ref.reqs), n + 1)
            assert (got["strings"].sum(1) == base["strings"].sum(1)).all() and (got["carriers"] == base["carriers"]).all()
    finally:
        _close(ss, gs)


# ---- long reads: a read set of this file's own --------------------------------------------------------------------
LONG_LENS = (200, 224, 225, 255, 256, 257, 300)


class LongSet:
    """about 60 reads of 200 to 300 symbols over a genome of 1,500 with three planted variants, one shard: for every variant,
    length and allele one read centred on the site, and 21 more laid at random over the sites.  align_gt_read keeps a read
    only if at most 4 of its bases hang out of the window, so the requests come with windows of 224 symbols (the alignment's
    last LDS class: the reads of 200, 224 and 225 fit it, and the read of 225 makes its item's longest pass 225), of 225
    (just over it) and of 599 (every read fits; the column lives in HBM), both alleles each"""

    def __init__(self):
        rng = random.Random(4096)
        rnd = lambda n: "".join(rng.choice("ACGT") for _ in range(n))  # noqa: E731
        self.genome = rnd(1500)
        self.sites = (400, 700, 1000)
        alt = list(self.genome)
        for i in self.sites:
            alt[i] = "ACGT"[("ACGT".index(alt[i]) + 1 + rng.randrange(3)) % 4]
        self.haps = [self.genome, "".join(alt)]
        reads = [h[at - n // 2:at - n // 2 + n] for at in self.sites for n in LONG_LENS for h in self.haps]
        for i in range(21):
            n = LONG_LENS[i % len(LONG_LENS)]
            h = self.haps[i % 2]
            s = self.sites[(i // 2) % 3] - rng.randrange(20, n - 20)
            reads.append(h[s:s + n])
        reads += reads[:4]  # copies > 1
        self.shards = [reads]

        def alleles(i, left, right):
            w, o = self.genome[i - left:i + right], self.haps[1][i]
            return [(w, left + 1, o, 0), (w[:left] + o + w[left + 1:], left + 1, self.genome[i], 0)]
        self.reqs = alleles(400, 111, 113) + alleles(400, 299, 300) + alleles(700, 112, 113) + alleles(1000, 299, 300)[:1]
        self.reqs.append((self.genome[701:1300], 599, "A", 1))


@pytest.fixture(scope="module")
def long_ref(oracle):
    ls = LongSet()
    return ls, Ref(oracle, shards=ls.shards, runs=[_bwt_runs(sh) for sh in ls.shards], name="long", reqs=ls.reqs)


def test_gpu_site_counts_long_reads(rsb, long_ref):
    """reads of 200, 224, 225, 255, 256, 257 and 300 symbols: the second extraction, the alignment's LDS class boundary and
    its HBM column, held to the restatement"""
    ls, r = long_ref
    gs = _open(rsb, r)
    ss = rsb.ShardSet(gs)
    try:
        _build(ss, r.pairs)
        for M, k, skip in ((0, 12, 3), (8, 16, 7)):
            got = _check(ss, rsb, r, M, k, skip, ("long", M, k, skip))
            assert (got["carriers"][:7] > 0).all() and got["work"]["extracted"] > 10
        items = SITE.rows_by_ordinal(r.side, r.reqs, 12, 3, 0)[1]
        assert {len(s) for s, _ in items.values()} >= set(LONG_LENS), sorted({len(s) for s, _ in items.values()})
        # the window of 224: reads of 200, 224 and 225 are carriers, the longer ones hang out of it
        kept = {len(s) for (q, _, _), (s, _) in items.items() if q < 2 and SITE.keeps(s, *r.reqs[q])}
        assert kept == {200, 224, 225}, kept
    finally:
        _close(ss, gs)


def test_gpu_site_counts_refuse_a_read_over_4096_symbols(rsb, long_ref):
    """one read of 4,097 symbols on a head ordinal is RSBWT_EINVAL, and the counters stay zero"""
    ls, _ = long_ref
    rng = random.Random(7)
    w = ls.reqs[0][0]
    huge = "".join(rng.choice("ACGT") for _ in range(2000)) + w + "".join(rng.choice("ACGT") for _ in range(4097 - 2000 - len(w)))
    assert len(huge) == 4097
    reads = ls.shards[0][:8] + [huge]
    with rsb.GpuBWT(runs=_bwt_runs(reads), num_strings=len(reads), ktab_depth=6, for_reads=True) as g:
        ss = rsb.ShardSet([g])
        try:
            ss.meta_build([huge], [b"ab!!"])
            ws, ps, al, ia = _cols(ls.reqs[:1])
            with pytest.raises(rsb.RsbwtError) as e:
                ss.site_sample_counts(ws, ps, al, ia, 16, 7, 0, codes=[b"ab"], size_of_sample=2)
            assert e.value.code == -1 and "4096" in str(e.value), str(e.value)
            assert rsb.ShardSet.site_last_work() == dict.fromkeys(KEYS, 0)
        finally:
            ss.close()


def test_gpu_site_counts_tight_set_repeatability_and_threads(rsb, ref, monkeypatch):
    """the set loaded to the brim (RSBWT_SAMPLE_TIGHT_SET=1: long probe chains) gives the same answers; two calls compared
    byte for byte; four host threads at once get the single-threaded answers and their own counters"""
    gs = _open(rsb, ref, span=SPANS["far"])
    ss = rsb.ShardSet(gs)
    try:
        _build(ss, ref.pairs)
        for tight in ("0", "1"):
            monkeypatch.setenv("RSBWT_SAMPLE_TIGHT_SET", tight)
            _check(ss, rsb, ref, 3, 8, 3, ("tight", tight))
            a, b = _got(ss, rsb, ref, 1, 12, 0), _got(ss, rsb, ref, 1, 12, 0)
            assert all(a[k].tobytes() == b[k].tobytes() for k in OUT) and a["work"] == b["work"]
        wants = {p: ref.want(*p) for p in ((3, 8, 3), (1, 12, 0))}
        errs = []

        def work(i):
            try:
                for rnd in range(3):
                    p = ((3, 8, 3), (1, 12, 0))[(i + rnd) % 2]
                    got = _got(ss, rsb, ref, *p)
                    got["work"].pop("narrow_steps")
                    assert SITE.same(got, wants[p]) is None, (i, rnd, SITE.same(got, wants[p]))
            except Exception as e:  # noqa: BLE001
                errs.append(repr(e))
        th = [threading.Thread(target=work, args=(i,)) for i in range(4)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert not errs, errs[:3]
    finally:
        _close(ss, gs)


def test_gpu_site_counts_second_build_clear_and_refusals(rsb, oracle, ref):
    """after a second build the answers follow the new table; after meta_clear the call is "no sample table"; and what the
    definition refuses: shards not opened for reads, a descending dictionary, all outputs NULL, NULL alt, a w of 4,097"""
    L = rsb.lib()
    gs = _open(rsb, ref)
    ss = rsb.ShardSet(gs)
    pv = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    try:
        ws, ps, al, ia = _cols(ref.reqs[:4])
        text, off = ss._var_text(ws)
        pos, alt, isalt = ss._gt_requests(ws, ps, al, ia)
        good = np.frombuffer(b"ab" b"ac" b"\xff\x00", np.uint8).copy()
        MARK = 0x7A7A7A7A
        st, ca = np.full((4, 4), MARK, np.uint32), np.full(4, MARK, np.uint64)
        call = lambda codes=good, alt_=alt, st_=st, ca_=ca, text_=text, off_=off: L.rsbwt_set_site_sample_counts(  # noqa: E731
            ss._s, pv(text_), pv(off_), 4, pv(pos), pv(alt_) if alt_ is not None else None, pv(isalt), 8, 3, 3, pv(codes), len(codes) // 2, 2, 1,
            pv(st_) if st_ is not None else None, None, None, pv(ca_) if ca_ is not None else None)
        assert call() == -1 and b"no sample table" in L.rsbwt_last_error()
        _build(ss, ref.pairs)
        first = _check(ss, rsb, ref, 3, 8, 3, "first build")
        assert call() == 0 and (st != MARK).all() and (ca != MARK).all()
        st[:] = MARK
        assert call(codes=np.frombuffer(b"ac" b"ab", np.uint8).copy()) == -1 and b"ascending" in L.rsbwt_last_error() and (st == MARK).all()
        assert call(st_=None, ca_=None) == -1 and b"no output" in L.rsbwt_last_error()
        assert call(alt_=None) == -1 and b"null" in L.rsbwt_last_error()
        long_text, long_off = ss._var_text(ws[:3] + ["ACGT" * 1024 + "A"])
        assert call(text_=long_text, off_=long_off) == -1 and b"4096" in L.rsbwt_last_error() and (st == MARK).all()
        assert rsb.ShardSet.site_last_work() == dict.fromkeys(KEYS, 0)
        assert L.rsbwt_set_site_sample_counts(ss._s, None, None, 0, None, None, None, 8, 3, 3, pv(good), 3, 2, 1, pv(st), None, None, None) == 0 and (st == MARK).all()
        pairs2, _ = SR.sample_pairs(ref.shards, ref.uni[5:40], ref.outside, ref.ss, ref.other, every=4, seed="second")
        side2 = SITE.Side(oracle, ref.shards, ref.runs, pairs2, "gt/second")
        assert side2.osh.heads != ref.side.osh.heads
        _build(ss, pairs2)
        want = SITE.want(side2, ref.reqs, 8, 3, 3, ref.codes, ref.ss, ref.other)
        got = _got(ss, rsb, ref, 3, 8, 3)
        assert SITE.same(got, want) is None, SITE.same(got, want)
        assert (got["carriers"] != first["carriers"]).any()
        ss.meta_clear()
        with pytest.raises(rsb.RsbwtError) as e:
            _got(ss, rsb, ref, 3, 8, 3)
        assert e.value.code == -1 and "no sample table" in str(e.value)
    finally:
        _close(ss, gs)
    gs = _open(rsb, ref, room=False)
    ss = rsb.ShardSet(gs)
    try:
        _build(ss, ref.pairs)
        with pytest.raises(rsb.RsbwtError) as e:
            _got(ss, rsb, ref, 3, 8, 3)
        assert e.value.code == -1 and "RSBWT_OPEN_READS" in str(e.value)
    finally:
        _close(ss, gs)
