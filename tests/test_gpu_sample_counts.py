"""Sample counts on the GPU (-m gpu): rsbwt_set_sample_counts / _dev, the head bitmaps of rsbwt_set_meta_build and
rsbwt_set_meta_head_bytes (csrc/sample_counts.hip, csrc/sets.hip) held bit-exactly to tests/sample_reference.py, the
definition restated over the oracle.  tests/test_sample_reference.py shows on the CPU that the inputs reach every class
and holds the restatement to a computation without a BWT."""
import ctypes as C
import threading

import numpy as np
import pytest

import gt_reference as G
import sample_reference as SR
import test_kmer_fixtures as F

pytestmark = pytest.mark.gpu

SPANS = {"control": 40, "chunk": 128, "far": 300, "chain": 600, "deep": 2944}
KEYS = ("rows", "head_rows", "carriers", "records", "unknown", "lf_steps")


class Ref:
    """one fixture under one record shape: the pairs, the restatement's side, the queries, a dictionary of 12 codes in an
    order that is not ascending, and the answers with no limit -- computed once, never changed"""

    def __init__(self, oracle, name="gt", ss=2, other=True):
        self.fx = G.fixture() if name == "gt" else F.fixture(name)
        self.ss, self.other = ss, other
        self.uni, self.outside = SR.universe(ss)
        self.pairs, self.info = SR.sample_pairs(self.fx.shards, self.uni, self.outside, ss, other)
        self.osh = SR.OracleShards(oracle, self.fx.shards, self.fx.runs(), self.pairs)
        self.queries = SR.queries_for(self.fx.shards)
        self.codes = self.uni[:30:3] + self.uni[40:42]
        self._memo = {}

    def want(self, queries=None, codes=None, max_rows=0):
        queries = self.queries if queries is None else queries
        codes = self.codes if codes is None else codes
        key = (tuple(queries), tuple(codes), max_rows)
        if key not in self._memo:
            self._memo[key] = SR.counts_oracle(self.osh, queries, codes, self.ss, self.other, max_rows)
        return self._memo[key]


@pytest.fixture(scope="module")
def refs(oracle):
    built = {}

    def get(name="gt", ss=2, other=True):
        if (name, ss, other) not in built:
            built[(name, ss, other)] = Ref(oracle, name, ss, other)
        return built[(name, ss, other)]
    return get


@pytest.fixture(scope="module")
def ref(refs):
    return refs()


def _open(rsb, fx, span=0, room=False, ktab=6, devices=None, grouped=False):
    devices = devices or [0] * len(fx.shards)
    return [rsb.GpuBWT(runs=runs, num_strings=len(sh), ktab_depth=ktab, window_span=span, for_reads=room, device=d, ktab_grouped=grouped)
            for d, sh, runs in zip(devices, fx.shards, fx.runs())]


def _close(ss, gs):
    ss.close()
    for g in gs:
        g.close()


def _build(ss, pairs):
    return ss.meta_build([w for w, _ in pairs], [v for _, v in pairs])


def _got(ss, rsb, r, queries=None, codes=None, max_rows=0, counting=True):
    queries = r.queries if queries is None else queries
    codes = r.codes if codes is None else codes
    L = rsb.lib()
    if counting:
        assert L.rsbwt_set_set_counting(ss._s, 1) == 0
    try:
        out = ss.sample_counts(queries, codes, r.ss, r.other, max_rows=max_rows)
    finally:
        if counting:
            assert L.rsbwt_set_set_counting(ss._s, 0) == 0
    out["work"] = rsb.ShardSet.sample_last_work()
    return out


def _check(ss, rsb, r, where, queries=None, codes=None, max_rows=0, counting=True):
    want = r.want(queries, codes, max_rows)
    got = _got(ss, rsb, r, queries, codes, max_rows, counting)
    if not counting:
        want = dict(want, work=dict(want["work"], lf_steps=0))
    assert tuple(got["work"]) == KEYS
    print(where, got["work"])
    assert SR.same(got, want) is None, (where, SR.same(got, want))
    return got


SHAPES = [("gt", ss, other) for ss in (1, 2, 3, 4, 8) for other in (True, False)] + [(n, ss, other) for n in ("repeat", "ragged")
                                                                                   for ss, other in ((2, True), (1, False), (8, True))]


@pytest.mark.parametrize("name,ss,other", SHAPES)
def test_gpu_sample_counts_is_the_restatement(rsb, refs, name, ss, other):
    """all four outputs and work6 (LF steps in counting mode) on the three fixtures, every size of sample with and without
    the meta bytes; shards opened for reads behind 6-mer tables; the bitmaps' size, and meta_bytes() unchanged by them"""
    r = refs(name, ss, other)
    gs = _open(rsb, r.fx, room=True)
    ss_ = rsb.ShardSet(gs)
    try:
        assert ss_.meta_head_bytes() == 0
        st = _build(ss_, r.pairs)
        assert tuple(st[k] for k in ("matched", "unmatched", "ordinals", "bytes")) == r.osh.stats
        assert ss_.meta_bytes() == sum((len(t) + 1) * 8 + sum(len(v) for v in t) for t in r.osh.tables)
        assert ss_.meta_head_bytes() == sum(4 * ((len(t) + 31) // 32) for t in r.osh.tables)
        got = _check(ss_, rsb, r, (name, ss, other))
        assert got["strings"].dtype == np.uint32 and got["copies"].dtype == np.int64 and got["strings"].shape == (len(r.queries), 13)
        _check(ss_, rsb, r, "not counting", counting=False)
    finally:
        _close(ss_, gs)


@pytest.mark.parametrize("kind", list(SPANS))
@pytest.mark.parametrize("ktab", [6, None])
def test_gpu_sample_counts_on_every_line_layout(rsb, ref, kind, ktab):
    """window spans 40, 128, 300, 600 and 2,944, with a 6-mer table and with none, shards NOT opened for reads"""
    span = SPANS[kind]
    gs = _open(rsb, ref.fx, span=span, ktab=ktab, room=False)
    ss = rsb.ShardSet(gs)
    try:
        assert all(g.window_span() == span and not rsb.lib().rsbwt_opened_for_reads(g.handle) for g in gs)
        _build(ss, ref.pairs)
        _check(ss, rsb, ref, (kind, ktab))
    finally:
        _close(ss, gs)


@pytest.mark.parametrize("ktab,grouped", [(6, True), (10, False), (10, True)])
def test_gpu_sample_counts_table_formats_and_depths(rsb, ref, ktab, grouped):
    gs = _open(rsb, ref.fx, ktab=ktab, grouped=grouped, room=True, span=SPANS["far"])
    ss = rsb.ShardSet(gs)
    try:
        assert all(g.ktab_depth() == ktab and g.ktab_info()[0] == (1 if grouped else 0) for g in gs)
        _build(ss, ref.pairs)
        _check(ss, rsb, ref, (ktab, grouped))
    finally:
        _close(ss, gs)


def test_gpu_sample_counts_single_handle_as_a_set_of_one(rsb, oracle, ref):
    """a per-partition answer is the same call on a set of one; the two partitions' answers add up to the set's"""
    gs = _open(rsb, ref.fx, span=SPANS["chunk"])
    try:
        parts = []
        for p, g in enumerate(gs):
            one = rsb.ShardSet([g])
            try:
                _build(one, ref.pairs)
                osh = SR.OracleShards(oracle, [ref.fx.shards[p]], [ref.fx.runs()[p]], ref.pairs)
                want = SR.counts_oracle(osh, ref.queries, ref.codes, ref.ss, ref.other)
                got = _got(one, rsb, ref)
                assert SR.same(got, want) is None, (p, SR.same(got, want))
                parts.append(got)
            finally:
                one.close()
        both = ref.want()
        for k in ("strings", "copies", "matches", "carriers"):
            assert (parts[0][k] + parts[1][k] == both[k]).all(), k
    finally:
        for g in gs:
            g.close()


def test_gpu_sample_counts_on_two_logical_devices(rsb, ref, monkeypatch):
    """a set split over two device groups (two logical devices on GPU 0 where the box has one): each group tallies its
    shards' rows, the host adds the matrices -- the one-device answers, with and without a limit; and a group whose
    shards do not sit next to each other in the set"""
    L = rsb.lib()
    if L.rsbwt_device_count() < 2:
        monkeypatch.setenv("RSBWT_ENABLE_TEST_HOOKS", "1")
        monkeypatch.setenv("RSBWT_TEST_DEVICE_ALIASES", "2")
    gs = _open(rsb, ref.fx, span=SPANS["far"], devices=(0, 1))
    ss = rsb.ShardSet(gs)
    try:
        assert L.rsbwt_set_devices(ss._s) == 2
        _build(ss, ref.pairs)
        _check(ss, rsb, ref, "two devices")
        m = ref.want()["matches"]
        limit = int(sorted(set(int(x) for x in m if x > 0))[2])
        _check(ss, rsb, ref, "two devices, limit", max_rows=limit)
        g2 = rsb.GpuBWT(runs=ref.fx.runs()[0], num_strings=len(ref.fx.shards[0]), ktab_depth=6, window_span=SPANS["far"], device=0)
        s3 = rsb.ShardSet(gs + [g2])
        try:
            assert L.rsbwt_set_devices(s3._s) == 2
            _build(s3, ref.pairs)
            one = rsb.ShardSet([g2])
            try:
                _build(one, ref.pairs)
                third = _got(one, rsb, ref)
            finally:
                one.close()
            got, both = _got(s3, rsb, ref), ref.want()
            for k in ("strings", "copies", "matches", "carriers"):
                assert (got[k] == both[k] + third[k]).all(), k
            assert all(got["work"][k] == both["work"][k] + third["work"][k] for k in KEYS)
        finally:
            s3.close()
            g2.close()
    finally:
        _close(ss, gs)


def test_gpu_sample_counts_batch_sizes_and_repeats(rsb, ref):
    """Q in {0, 1, 63, 64, 65, 4,097} by repeating queries; one query asked 1,000 times in one call"""
    gs = _open(rsb, ref.fx)
    ss = rsb.ShardSet(gs)
    try:
        _build(ss, ref.pairs)
        base = [w for w, m in zip(ref.queries, ref.want()["matches"]) if m < 400]  # (the 4,097 stay a few 10^4 rows)
        for cnt in (0, 1, 63, 64, 65, 4097):
            qs = [base[i % len(base)] for i in range(cnt)]
            got = _check(ss, rsb, ref, f"Q={cnt}", queries=qs)
            assert got["strings"].shape == (cnt, 13) and got["matches"].shape == (cnt,)
        w = max((w for w in base), key=lambda w: ref.want()["carriers"][ref.queries.index(w)])
        got = _check(ss, rsb, ref, "x1000", queries=[w] * 1000)
        assert got["carriers"][0] > 1 and (got["strings"] == got["strings"][0]).all()
    finally:
        _close(ss, gs)


def test_gpu_sample_counts_dictionary_sizes(rsb, ref):
    """C in {1, 2, 63, 64, 65} and 4,200 codes -- 33,600 bytes of keys, over the 32 KiB the kernel keeps in LDS -- in a
    shuffled order: the columns follow the caller's order, the rest lands in the unknown column"""
    gs = _open(rsb, ref.fx)
    ss = rsb.ShardSet(gs)
    try:
        _build(ss, ref.pairs)
        big = SR.universe(ref.ss, 4200)[0]
        assert big[:70] == ref.uni and 8 * len(big) > 32 << 10
        rng = np.random.default_rng(5)
        for n in (1, 2, 63, 64, 65, 4200):
            codes = [big[i] for i in rng.permutation(len(big))[:n]] if n > 65 else [big[i] for i in rng.permutation(70)[:n]]
            qs = ref.queries if n <= 65 else ref.queries[:20]
            got = _check(ss, rsb, ref, f"C={n}", queries=qs, codes=codes)
            assert got["strings"].shape == (len(qs), n + 1)
            assert (got["strings"].sum(1) == ref.want(qs)["strings"].sum(1)).all()
        full = _check(ss, rsb, ref, "every code known", codes=ref.uni + ref.outside)
        assert not full["strings"][:, -1].any() and full["work"]["unknown"] == 0
    finally:
        _close(ss, gs)


def test_gpu_sample_counts_tight_set_limits_and_repeatability(rsb, ref, monkeypatch):
    """max_rows 0, at and below a query's row count; the same answers with the set loaded to the brim
    (RSBWT_SAMPLE_TIGHT_SET=1: long probe chains); two calls in a row give identical bytes"""
    gs = _open(rsb, ref.fx, span=SPANS["far"])
    ss = rsb.ShardSet(gs)
    try:
        _build(ss, ref.pairs)
        m = ref.want()["matches"]
        at = int(sorted(set(int(x) for x in m if x > 0))[len(set(int(x) for x in m if x > 0)) // 2])
        for tight in ("0", "1"):
            monkeypatch.setenv("RSBWT_SAMPLE_TIGHT_SET", tight)
            for limit in (0, at, at - 1, 1):
                got = _check(ss, rsb, ref, (tight, limit), max_rows=limit)
                if limit:
                    over = m > limit
                    assert not got["strings"][over].any() and not got["carriers"][over].any() and (got["matches"] == m).all()
            a, b = _got(ss, rsb, ref), _got(ss, rsb, ref)
            assert all(a[k].tobytes() == b[k].tobytes() for k in ("strings", "copies", "matches", "carriers")) and a["work"] == b["work"]
            dup = [ref.queries[3]] * 777  # 777 x the same rows in a set with fewer than twice as many slots
            _check(ss, rsb, ref, ("dup", tight), queries=dup)
    finally:
        _close(ss, gs)


def test_gpu_sample_counts_device_resident_form(rsb, ref):
    """rsbwt_set_sample_counts_dev inside 0xAB guard bytes, against the host form: the exact row room, more room than rows,
    and one row short (nothing tallied, status[0] names the need)"""
    import torch
    L = rsb.lib()
    gs = _open(rsb, ref.fx, span=SPANS["far"])
    ss = rsb.ShardSet(gs)
    p = lambda t, byte=0: C.c_void_p(t.data_ptr() + byte)  # noqa: E731
    try:
        _build(ss, ref.pairs)
        text, off = rsb.ShardSet._var_text(ref.queries)
        Q, n, PAD = len(ref.queries), len(ref.codes), 256
        max_len = max(len(w) for w in ref.queries)
        order = sorted(range(n), key=lambda i: ref.codes[i])
        flat = np.frombuffer(b"".join(ref.codes[i] for i in order), np.uint8).copy()
        keys = np.zeros(n, np.uint64)
        assert L.rsbwt_sample_keys(flat.ctypes.data_as(C.c_void_p), n, ref.ss, keys.ctypes.data_as(C.c_void_p)) == 0
        d_text = torch.from_numpy(text).cuda()
        d_off = torch.from_numpy(off.view(np.int64)).cuda()
        d_keys = torch.from_numpy(keys.view(np.int64)).cuda()
        m = ref.want()["matches"]
        limit = int(sorted(set(int(x) for x in m if x > 0))[-2])
        want = ref.want(max_rows=limit)
        rows = want["work"]["rows"]
        sizes = dict(strings=Q * (n + 1) * 4, copies=Q * (n + 1) * 8, matches=Q * 8, carriers=Q * 8, status=64)
        for cap in (rows, rows + 1000, rows - 1):
            d = {k: torch.full((PAD + b + PAD,), 0xAB, dtype=torch.uint8, device="cuda") for k, b in sizes.items()}
            rc = L.rsbwt_set_sample_counts_dev(ss._s, p(d_text), p(d_off), Q, max_len, p(d_keys), n, ref.ss, 1 if ref.other else 0, limit, 0, cap,
                                               p(d["strings"], PAD), p(d["copies"], PAD), p(d["matches"], PAD), p(d["carriers"], PAD),
                                               p(d["status"], PAD), None)
            assert rc == 0, L.rsbwt_last_error()
            torch.cuda.synchronize()
            h = {k: t.cpu().numpy() for k, t in d.items()}
            for k, b in sizes.items():
                assert (h[k][:PAD] == 0xAB).all() and (h[k][PAD + b:] == 0xAB).all(), (cap, k)
            body = lambda k, dt: h[k][PAD:PAD + sizes[k]].view(dt)  # noqa: E731
            status = body("status", np.uint64).tolist()
            assert status[0] == rows and (body("matches", np.uint64) == want["matches"]).all()
            if cap < rows:
                assert status[1:] == [0] * 7 and not body("strings", np.uint32).any() and not body("carriers", np.uint64).any()
                continue
            back = np.empty(n + 1, np.int64)
            back[np.array(order, np.int64)] = np.arange(n)
            back[n] = n
            assert (body("strings", np.uint32).reshape(Q, n + 1)[:, back] == want["strings"]).all(), cap
            assert (body("copies", np.int64).reshape(Q, n + 1)[:, back] == want["copies"]).all(), cap
            assert (body("carriers", np.uint64) == want["carriers"]).all(), cap
            wk = want["work"]
            assert status == [rows, wk["head_rows"], wk["carriers"], wk["records"], wk["unknown"], wk["lf_steps"], 0, 0], (cap, status)
        # Q = 0: the status zeroed and nothing else; null arguments; max_len out of range
        d_st = torch.full((128,), 0xAB, dtype=torch.uint8, device="cuda")
        assert L.rsbwt_set_sample_counts_dev(ss._s, None, None, 0, 4, p(d_keys), n, ref.ss, 1, 0, 0, 0, p(d_st), None, None, None, p(d_st, 64), None) == 0
        torch.cuda.synchronize()
        hs = d_st.cpu().numpy()
        assert (hs[:64] == 0xAB).all() and not hs[64:].any()
        args = (p(d_text), p(d_off), Q, max_len, p(d_keys), n, ref.ss, 1, 0, 0, 16)
        assert L.rsbwt_set_sample_counts_dev(ss._s, *args, None, None, None, None, p(d_st), None) == -1
        assert L.rsbwt_set_sample_counts_dev(ss._s, *args, p(d_st), None, None, None, None, None) == -1
        assert L.rsbwt_set_sample_counts_dev(ss._s, p(d_text), p(d_off), Q, 0, p(d_keys), n, ref.ss, 1, 0, 0, 16, p(d_st), None, None, None, p(d_st), None) == -1
    finally:
        _close(ss, gs)


def test_gpu_sample_counts_second_build_and_clear(rsb, oracle, ref):
    """after a second build: new heads, new answers; after meta_clear: RSBWT_EINVAL and no bitmap bytes"""
    gs = _open(rsb, ref.fx)
    ss = rsb.ShardSet(gs)
    try:
        _build(ss, ref.pairs)
        first = _check(ss, rsb, ref, "first build")
        pairs2, _ = SR.sample_pairs(ref.fx.shards, ref.uni[5:40], ref.outside, ref.ss, ref.other, every=4, seed="second")
        osh2 = SR.OracleShards(oracle, ref.fx.shards, ref.fx.runs(), pairs2)
        assert osh2.heads != ref.osh.heads
        _build(ss, pairs2)
        want = SR.counts_oracle(osh2, ref.queries, ref.codes, ref.ss, ref.other)
        got = _got(ss, rsb, ref)
        assert SR.same(got, want) is None, SR.same(got, want)
        assert (got["carriers"] != first["carriers"]).any() and (got["matches"] == first["matches"]).all()
        head = ss.meta_head_bytes()
        assert head == sum(4 * ((len(sh) + 31) // 32) for sh in ref.fx.shards)
        ss.meta_clear()
        assert ss.meta_head_bytes() == 0 and ss.meta_bytes() == 0
        with pytest.raises(rsb.RsbwtError) as e:
            ss.sample_counts(ref.queries, ref.codes, ref.ss, ref.other)
        assert e.value.code == -1 and "no sample table" in str(e.value)
        _build(ss, ref.pairs)
        _check(ss, rsb, ref, "built again")
    finally:
        _close(ss, gs)


def test_gpu_sample_counts_refuses_what_the_definition_refuses(rsb, ref):
    L = rsb.lib()
    gs = _open(rsb, ref.fx)
    ss = rsb.ShardSet(gs)
    pv = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    try:
        text, off = rsb.ShardSet._var_text(["ACGT", "TTGA"])
        good = np.frombuffer(b"ab" b"ac" b"\xff\x00", np.uint8).copy()
        MARK = 0x7A7A7A7A
        st, cp = np.full((2, 4), MARK, np.uint32), np.full((2, 4), MARK, np.int64)
        mt, ca = np.full(2, MARK, np.uint64), np.full(2, MARK, np.uint64)
        call = lambda codes, n, size: L.rsbwt_set_sample_counts(  # noqa: E731
            ss._s, pv(text), pv(off), 2, pv(codes) if codes is not None else None, n, size, 1, 0, 0, pv(st), pv(cp), pv(mt), pv(ca))
        assert call(good, 3, 2) == -1 and b"no sample table" in L.rsbwt_last_error()
        _build(ss, ref.pairs)
        assert call(good, 3, 2) == 0 and (mt != MARK).all() and (st != MARK).all() and (ca != MARK).all()
        for codes, n, size, word in ((np.frombuffer(b"ab" b"ab" b"ac", np.uint8).copy(), 3, 2, b"ascending"),  # not distinct
                                     (np.frombuffer(b"ac" b"ab", np.uint8).copy(), 2, 2, b"ascending"),      # descending
                                     (np.frombuffer(b"a\x80" b"a\x7f", np.uint8).copy(), 2, 2, b"ascending"),  # bytes compare unsigned
                                     (good, 3, 0, b"size_of_sample"), (good, 1, 9, b"size_of_sample"), (good, 0, 2, b"empty"),
                                     (None, 3, 2, b"null")):
            st[:] = MARK
            assert call(codes, n, size) == -1 and word in L.rsbwt_last_error(), (n, size, L.rsbwt_last_error())
            assert (st == MARK).all()
        assert L.rsbwt_set_sample_counts(ss._s, pv(text), pv(off), 2, pv(good), 3, 2, 1, 0, 0, None, None, None, None) == -1
        assert L.rsbwt_set_sample_counts(ss._s, pv(text), None, 2, pv(good), 3, 2, 1, 0, 0, pv(st), None, None, None) == -1
        assert L.rsbwt_set_sample_counts(ss._s, pv(text), pv(off), 2, pv(good), 3, 2, 1, 0, 0, None, None, pv(mt), None) == 0  # one output is enough
        with pytest.raises(rsb.RsbwtError):
            ss.sample_counts(["ACGT"], [b"ab", b"ab"], 2)  # the same code twice
        with pytest.raises(ValueError):
            ss.sample_counts(["ACGT"], [b"ab", b"abc"], 2)
        # a walk that cannot end within max_steps fails the call: it is not left out silently
        deep = [w for w, m in zip(ref.queries, ref.want()["matches"]) if m > 0 and len(w) <= 12][0]
        with pytest.raises(rsb.RsbwtError) as e:
            ss.sample_counts([deep], ref.codes, ref.ss, ref.other, max_steps=1)
        assert e.value.code == -1 and "does not end" in str(e.value), str(e.value)
    finally:
        _close(ss, gs)


@pytest.mark.parametrize("ktab", [None, 2])
def test_gpu_sample_counts_on_a_shard_without_terminators(rsb, ktab):
    """7,037 x 'T' and no '$': no strings, no ordinals, no heads -- a query without rows answers zeros; one with rows cannot
    be located and fails the call"""
    runs = np.full(227, (4 << 5) | 31, np.uint8)
    with rsb.GpuBWT(runs=runs, num_strings=0, ktab_depth=ktab) as g:
        ss = rsb.ShardSet([g])
        try:
            st = ss.meta_build(["TTTT", "ACGT"], [b"ab!!", b"cd!!"])
            assert st["matched"] == 0 and ss.meta_head_bytes() == 0
            got = ss.sample_counts(["A", "ATT", ""], [b"ab", b"cd"], 2)
            assert not got["strings"].any() and not got["copies"].any() and not got["matches"].any() and not got["carriers"].any()
            assert rsb.ShardSet.sample_last_work() == dict.fromkeys(KEYS, 0)
            with pytest.raises(rsb.RsbwtError) as e:
                ss.sample_counts(["TTTT"], [b"ab", b"cd"], 2, max_steps=8)
            assert e.value.code == -1 and "does not end" in str(e.value)
        finally:
            ss.close()


def test_gpu_sample_counts_from_eight_threads(rsb, ref):
    """the call is re-entrant: eight threads on one set get the single-threaded answers and their own work counters"""
    gs = _open(rsb, ref.fx, room=True)
    ss = rsb.ShardSet(gs)
    try:
        _build(ss, ref.pairs)
        m = ref.want()["matches"]
        limits = [0, int(sorted(set(int(x) for x in m if x > 0))[3])]
        wants = {lim: ref.want(max_rows=lim) for lim in limits}
        errs = []

        def work(i):
            try:
                for rnd in range(4):
                    lim = limits[(i + rnd) % 2]
                    got = ss.sample_counts(ref.queries, ref.codes, ref.ss, ref.other, max_rows=lim)
                    got["work"] = dict(rsb.ShardSet.sample_last_work(), lf_steps=wants[lim]["work"]["lf_steps"])
                    assert SR.same(got, wants[lim]) is None, (i, rnd, SR.same(got, wants[lim]))
            except Exception as e:  # noqa: BLE001
                errs.append(repr(e))
        th = [threading.Thread(target=work, args=(i,)) for i in range(8)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert not errs, errs[:3]
    finally:
        _close(ss, gs)
