"""The per-read sample table on the GPU (-m gpu): rsbwt_set_meta_build / _load / _clear, rsbwt_set_read_ordinals_var,
rsbwt_set_meta_by_ordinal / _dev and rsbwt_set_read_meta_var (csrc/read_meta.hip, csrc/sets.hip) held bit-exactly to
tests/meta_reference.py, the definition restated over the oracle.  The fixture is the gt tests'; the pairs are
meta_reference.pairs_for's; tests/test_meta_reference.py shows on the CPU that they reach every class and holds the
restatement to a computation without a BWT."""
import ctypes as C
import threading

import numpy as np
import pytest

import gt_reference as G
import meta_reference as MR

pytestmark = pytest.mark.gpu

SPANS = {"control": 40, "chunk": 128, "far": 300, "chain": 600, "deep": 2944}
U64MAX = (1 << 64) - 1


class Ref:
    def __init__(self, oracle):
        self.fx = G.fixture()
        self.orc = [MR.OracleSide(oracle.from_runs(r, len(sh)), len(sh)) for sh, r in zip(self.fx.shards, self.fx.runs())]
        self.pairs, self.info = MR.pairs_for(self.fx.shards)
        self.tables, self.stats = MR.build_tables(self.orc, self.pairs)
        distinct = sorted({r for sh in self.fx.shards for r in sh})
        # the strings the lookups are asked: the pairs', every distinct read (those no pair names too), strings that are no read
        self.asked = [w for w, _ in self.pairs] + distinct + [distinct[0][1:], distinct[-1][:-1], "A", "ACGTN", "", distinct[0] + "A"]
        self.vals, self.copies, self.steps = MR.read_meta(self.orc, self.tables, self.asked)
        self.ordinals = [[s.lookup(w)[0] for w in self.asked] for s in self.orc]


@pytest.fixture(scope="module")
def ref(oracle):
    return Ref(oracle)


def _open(rsb, fx, span=0, room=False, ktab=6, devices=(0, 0), grouped=False):
    return [rsb.GpuBWT(runs=runs, num_strings=len(sh), ktab_depth=ktab, window_span=span, for_reads=room, device=d, ktab_grouped=grouped)
            for d, sh, runs in zip(devices, fx.shards, fx.runs())]


def _close(ss, gs):
    ss.close()
    for g in gs:
        g.close()


def _build(ss, pairs):
    return ss.meta_build([w for w, _ in pairs], [v for _, v in pairs])


def _all_items(tables, seed=7):
    """every ordinal of every shard once, in a seeded order"""
    items = [(p, o) for p, t in enumerate(tables) for o in range(len(t))]
    np.random.default_rng(seed).shuffle(items)
    return [p for p, _ in items], [o for _, o in items]


def _check(ss, rsb, ref, where, tables=None, counting=True):
    """every lookup against the restatement: ordinals, copies, values by string and by ordinal, the work counters"""
    tables = tables if tables is not None else ref.tables
    L = rsb.lib()
    S = len(tables)
    od, cp = ss.read_ordinals(ref.asked)
    assert od.dtype == np.uint64 and od.shape == cp.shape == (S, len(ref.asked))
    assert (cp == np.array(ref.copies, np.uint64)).all(), (where, np.argwhere(cp != np.array(ref.copies, np.uint64))[:5])
    assert (od == np.array(ref.ordinals, np.uint64)).all(), (where, np.argwhere(od != np.array(ref.ordinals, np.uint64))[:5])
    cp2, _ = ss.read_copies_var(ref.asked)  # the call this one adds an output to keeps its answers
    assert (cp2 == cp).all(), where
    vals, _, _ = MR.read_meta(ref.orc, tables, ref.asked) if tables is not ref.tables else (ref.vals, None, None)
    efirst, ebytes = MR.flat(vals)
    if counting:
        assert L.rsbwt_set_set_counting(ss._s, 1) == 0
    first, got, cpm = ss.read_meta(ref.asked, raw=True)
    wk = rsb.ShardSet.meta_last_work()
    if counting:
        assert L.rsbwt_set_set_counting(ss._s, 0) == 0
    assert [int(x) for x in first] == efirst, where
    assert got.tobytes() == ebytes, where
    assert (cpm == cp).all(), where
    print(where, wk, "reference steps", ref.steps)
    want = dict(items=len(ref.asked) * S, valued=sum(len(v) > 0 for v in vals), bytes=len(ebytes), lf_steps=ref.steps if counting else 0)
    assert wk == want, (where, wk, want)
    sh, ods = _all_items(tables)
    efirst2, ebytes2 = MR.flat(MR.by_ordinal(tables, sh, ods))
    first2, got2 = ss.meta_by_ordinal(sh, ods, raw=True)
    assert [int(x) for x in first2] == efirst2 and got2.tobytes() == ebytes2, where
    wk2 = rsb.ShardSet.meta_last_work()
    assert wk2 == dict(items=len(sh), valued=sum(len(tables[p][o]) > 0 for p, o in zip(sh, ods)), bytes=len(ebytes2), lf_steps=0), (where, wk2)


def test_gpu_meta_is_the_restatement(rsb, ref):
    """at the builder's own span behind 6-mer tables, shards opened for reads: the build's stats4, every lookup, the size"""
    gs = _open(rsb, ref.fx, room=True)
    ss = rsb.ShardSet(gs)
    try:
        assert ss.meta_bytes() == 0
        st = _build(ss, ref.pairs)
        assert tuple(st[k] for k in ("matched", "unmatched", "ordinals", "bytes")) == ref.stats, (st, ref.stats)
        assert ss.meta_bytes() == sum((len(t) + 1) * 8 + sum(len(v) for v in t) for t in ref.tables)
        _check(ss, rsb, ref, "auto")
        # the nested forms
        nested, cp = ss.read_meta(ref.asked[:50])
        assert [v for per in nested for v in per] == ref.vals[:100]
        assert ss.meta_by_ordinal([0, 1, 0], [0, 5, 3]) == [ref.tables[0][0], ref.tables[1][5], ref.tables[0][3]]
    finally:
        _close(ss, gs)


@pytest.mark.parametrize("kind", list(SPANS))
@pytest.mark.parametrize("ktab", [6, None])
def test_gpu_meta_on_every_line_layout(rsb, ref, kind, ktab):
    """window spans 40, 128, 300, 600 and 2,944 (no continuation, spill chunks, far lines, far chains), with a 6-mer table and
    with none, shards NOT opened for reads: no lookup needs that"""
    span = SPANS[kind]
    gs = _open(rsb, ref.fx, span=span, ktab=ktab, room=False)
    ss = rsb.ShardSet(gs)
    try:
        assert all(g.window_span() == span and not rsb.lib().rsbwt_opened_for_reads(g.handle) for g in gs)
        assert all(g.ktab_depth() == (ktab or 0) for g in gs)
        _build(ss, ref.pairs)
        _check(ss, rsb, ref, (kind, ktab))
        assert all(rsb.lib().rsbwt_psi_hint_lines(g.handle) == 0 for g in gs)  # nothing for extraction was built on the way
    finally:
        _close(ss, gs)


@pytest.mark.parametrize("ktab,grouped", [(6, True), (10, False), (10, True)])
def test_gpu_meta_table_formats_and_depths(rsb, ref, ktab, grouped):
    gs = _open(rsb, ref.fx, ktab=ktab, grouped=grouped, room=True, span=SPANS["far"])
    ss = rsb.ShardSet(gs)
    try:
        assert all(g.ktab_depth() == ktab and g.ktab_info()[0] == (1 if grouped else 0) for g in gs)
        _build(ss, ref.pairs)
        _check(ss, rsb, ref, (ktab, grouped))
    finally:
        _close(ss, gs)


def test_gpu_meta_single_handle_as_a_set_of_one(rsb, ref):
    gs = _open(rsb, ref.fx, span=SPANS["chunk"])
    try:
        for p, g in enumerate(gs):
            one = rsb.ShardSet([g])
            try:
                st = _build(one, ref.pairs)
                tables, stats = MR.build_tables([ref.orc[p]], ref.pairs)
                assert tables == [ref.tables[p]] and tuple(st.values()) == stats
                first, got, cp = one.read_meta(ref.asked, raw=True)
                efirst, ebytes = MR.flat(ref.vals[p::2])
                assert [int(x) for x in first] == efirst and got.tobytes() == ebytes and (cp[0] == np.array(ref.copies[p], np.uint64)).all()
                ods = list(range(len(tables[0]))) + [len(tables[0]), U64MAX]
                assert one.meta_by_ordinal([0] * len(ods), ods) == tables[0] + [b"", b""]
            finally:
                one.close()
    finally:
        for g in gs:
            g.close()


def test_gpu_meta_on_two_logical_devices(rsb, ref, monkeypatch):
    """a set split over two device groups (two logical devices on GPU 0 where the box has one): each shard's table lives
    with its shard, the host lays the values out in the order asked -- the one-device answers; and a group whose shards do
    not sit next to each other in the set"""
    L = rsb.lib()
    if L.rsbwt_device_count() < 2:
        monkeypatch.setenv("RSBWT_ENABLE_TEST_HOOKS", "1")
        monkeypatch.setenv("RSBWT_TEST_DEVICE_ALIASES", "2")
    gs = _open(rsb, ref.fx, span=SPANS["far"], devices=(0, 1))
    ss = rsb.ShardSet(gs)
    try:
        assert L.rsbwt_set_devices(ss._s) == 2
        st = _build(ss, ref.pairs)
        assert tuple(st.values()) == ref.stats
        _check(ss, rsb, ref, "two devices")
        g2 = rsb.GpuBWT(runs=ref.fx.runs()[0], num_strings=len(ref.fx.shards[0]), ktab_depth=6, window_span=SPANS["far"], device=0)
        s3 = rsb.ShardSet(gs + [g2])
        try:
            assert L.rsbwt_set_devices(s3._s) == 2
            _build(s3, ref.pairs)
            t3 = ref.tables + [ref.tables[0]]
            sh, ods = _all_items(t3, seed=11)
            assert s3.meta_by_ordinal(sh, ods) == MR.by_ordinal(t3, sh, ods)
            first, got, cp = s3.read_meta(ref.asked, raw=True)
            v3 = [v for q in range(len(ref.asked)) for v in (ref.vals[2 * q], ref.vals[2 * q + 1], ref.vals[2 * q])]
            efirst, ebytes = MR.flat(v3)
            assert [int(x) for x in first] == efirst and got.tobytes() == ebytes
            assert (cp[2] == cp[0]).all() and (cp[:2] == np.array(ref.copies, np.uint64)).all()
        finally:
            s3.close()
            g2.close()
    finally:
        _close(ss, gs)


def test_gpu_meta_by_ordinal_counts_repeats_and_edges(rsb, ref):
    """n in {0, 1, 63, 64, 65, 4,097}; one ordinal 1,000 times; ordinals num_strings - 1, num_strings and UINT64_MAX; a bad
    shard index; a set without a table"""
    L = rsb.lib()
    gs = _open(rsb, ref.fx)
    ss = rsb.ShardSet(gs)
    pv = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    try:
        n = C.c_size_t(5)
        first = np.full(4, 9, np.uint64)
        sh1, od1 = np.zeros(2, np.uint32), np.zeros(2, np.uint64)
        assert L.rsbwt_set_meta_by_ordinal(ss._s, pv(sh1), pv(od1), 2, pv(first), None, 0, C.byref(n)) == -1
        assert b"no sample table" in L.rsbwt_last_error()
        with pytest.raises(rsb.RsbwtError) as e:
            ss.read_meta(["ACGT"])
        assert e.value.code == -1 and "no sample table" in str(e.value)
        _build(ss, ref.pairs)
        ns = [len(t) for t in ref.tables]
        rng = np.random.default_rng(3)
        for cnt in (0, 1, 63, 64, 65, 4097):
            sh = rng.integers(0, 2, cnt).tolist()
            ods = [int(rng.integers(0, ns[p])) for p in sh]
            assert ss.meta_by_ordinal(sh, ods) == MR.by_ordinal(ref.tables, sh, ods), cnt
            assert rsb.ShardSet.meta_last_work()["items"] == cnt
        long_o = next(o for o, v in enumerate(ref.tables[1]) if len(v) == 5000)
        short_o = next(o for o, v in enumerate(ref.tables[1]) if len(v) == 3)
        for o in (long_o, short_o):
            got = ss.meta_by_ordinal([1] * 1000, [o] * 1000)
            assert got == [ref.tables[1][o]] * 1000
        sh = [0, 0, 0, 1, 1, 1, 0]
        ods = [ns[0] - 1, ns[0], U64MAX, ns[1] - 1, ns[1], U64MAX, 0]
        assert ss.meta_by_ordinal(sh, ods) == [ref.tables[0][-1], b"", b"", ref.tables[1][-1], b"", b"", ref.tables[0][0]]
        # a shard index out of range
        bad_sh, bad_od = np.array([0, 2], np.uint32), np.array([0, 0], np.uint64)
        first[:] = 9
        assert L.rsbwt_set_meta_by_ordinal(ss._s, pv(bad_sh), pv(bad_od), 2, pv(first), None, 0, C.byref(n)) == -1
        assert b"shard 2" in L.rsbwt_last_error()
        # null arguments
        assert L.rsbwt_set_meta_by_ordinal(ss._s, pv(sh1), pv(od1), 2, None, None, 0, C.byref(n)) == -1
        assert L.rsbwt_set_meta_by_ordinal(ss._s, pv(sh1), pv(od1), 2, pv(first), None, 0, None) == -1
        assert L.rsbwt_set_meta_by_ordinal(ss._s, None, pv(od1), 2, pv(first), None, 0, C.byref(n)) == -1
    finally:
        _close(ss, gs)


def test_gpu_meta_sizing_protocol(rsb, ref):
    """cap = 0 sizes the buffer (RSBWT_ERANGE with *nbytes and first[] set), one byte short is refused with nothing written,
    the exact size is filled and nothing behind it is touched -- by ordinal and by string"""
    L = rsb.lib()
    gs = _open(rsb, ref.fx)
    ss = rsb.ShardSet(gs)
    pv = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    try:
        _build(ss, ref.pairs)
        sh, ods = _all_items(ref.tables, seed=5)
        efirst, ebytes = MR.flat(MR.by_ordinal(ref.tables, sh, ods))
        a_sh, a_od = np.array(sh, np.uint32), np.array(ods, np.uint64)
        text, off = ss._var_text(ref.asked)
        sfirst, sbytes = MR.flat(ref.vals)
        calls = [(lambda f, b, cap, n: L.rsbwt_set_meta_by_ordinal(ss._s, pv(a_sh), pv(a_od), len(sh), pv(f), b, cap, C.byref(n)), efirst, ebytes),
                 (lambda f, b, cap, n: L.rsbwt_set_read_meta_var(ss._s, pv(text), pv(off), len(ref.asked), pv(f), b, cap, C.byref(n), None),
                  sfirst, sbytes)]
        for call, wfirst, wbytes in calls:
            total = len(wbytes)
            for buf_cap in (0, total - 1):
                first = np.zeros(len(wfirst), np.uint64)
                out = np.full(total + 16, 0xAB, np.uint8)
                n = C.c_size_t()
                assert call(first, pv(out) if buf_cap else None, buf_cap, n) == -7
                assert n.value == total and [int(x) for x in first] == wfirst and (out == 0xAB).all()
            first = np.zeros(len(wfirst), np.uint64)
            out = np.full(total + 16, 0xAB, np.uint8)
            n = C.c_size_t()
            assert call(first, pv(out), total, n) == 0
            assert n.value == total and out[:total].tobytes() == wbytes and (out[total:] == 0xAB).all()
        # nothing asked: fine, nothing but first[0] and *nbytes touched
        first = np.full(3, 9, np.uint64)
        n = C.c_size_t(5)
        assert L.rsbwt_set_meta_by_ordinal(ss._s, None, None, 0, pv(first), None, 0, C.byref(n)) == 0 and n.value == 0 and first[0] == 0
        n = C.c_size_t(5)
        assert L.rsbwt_set_read_meta_var(ss._s, None, None, 0, pv(first), None, 0, C.byref(n), None) == 0 and n.value == 0
        assert ss.read_meta([""], raw=True)[0].tolist() == [0, 0, 0] and ss.meta_by_ordinal([], []) == []
        # items whose values are all empty need no buffer
        n = C.c_size_t(5)
        e_sh, e_od = np.zeros(2, np.uint32), np.full(2, U64MAX, np.uint64)
        assert L.rsbwt_set_meta_by_ordinal(ss._s, pv(e_sh), pv(e_od), 2, pv(first), None, 0, C.byref(n)) == 0 and n.value == 0 and not first.any()
    finally:
        _close(ss, gs)


def test_gpu_meta_device_resident_form(rsb, ref):
    """rsbwt_set_meta_by_ordinal_dev inside 0xAB guard bytes: with cap one byte short only d_first is written; with the
    exact cap the bytes are the restatement's and nothing outside the two arrays changes"""
    import torch
    L = rsb.lib()
    gs = _open(rsb, ref.fx, span=SPANS["far"])
    ss = rsb.ShardSet(gs)
    p = lambda t, byte=0: C.c_void_p(t.data_ptr() + byte)  # noqa: E731
    try:
        _build(ss, ref.pairs)
        sh, ods = _all_items(ref.tables, seed=9)
        sh += [0, 1, 5]
        ods += [len(ref.tables[0]), U64MAX, 0]  # (a shard index out of range: an empty value in this form)
        efirst, ebytes = MR.flat([ref.tables[p_][o] if p_ < 2 and o < len(ref.tables[p_]) else b"" for p_, o in zip(sh, ods)])
        n, total, PAD = len(sh), len(ebytes), 256
        d_sh = torch.from_numpy(np.array(sh, np.uint32).view(np.int32)).cuda()
        d_od = torch.from_numpy(np.array(ods, np.uint64).view(np.int64)).cuda()
        for cap in (total - 1, total):
            d_first = torch.full((PAD + (n + 1) * 8 + PAD,), 0xAB, dtype=torch.uint8, device="cuda")
            d_bytes = torch.full((PAD + total + PAD,), 0xAB, dtype=torch.uint8, device="cuda")
            rc = L.rsbwt_set_meta_by_ordinal_dev(ss._s, p(d_sh), p(d_od), n, p(d_first, PAD), p(d_bytes, PAD), cap, None)
            assert rc == 0, L.rsbwt_last_error()
            torch.cuda.synchronize()
            hf, hb = d_first.cpu().numpy(), d_bytes.cpu().numpy()
            assert (hf[:PAD] == 0xAB).all() and (hf[PAD + (n + 1) * 8:] == 0xAB).all()
            assert hf[PAD:PAD + (n + 1) * 8].view(np.uint64).tolist() == efirst
            assert (hb[:PAD] == 0xAB).all() and (hb[PAD + total:] == 0xAB).all()
            if cap < total:
                assert (hb == 0xAB).all()
            else:
                assert hb[PAD:PAD + total].tobytes() == ebytes
        # n = 0: d_first[0] = 0 and nothing else; null arguments
        d_first = torch.full((64,), 0xAB, dtype=torch.uint8, device="cuda")
        assert L.rsbwt_set_meta_by_ordinal_dev(ss._s, None, None, 0, p(d_first), None, 0, None) == 0
        torch.cuda.synchronize()
        hf = d_first.cpu().numpy()
        assert not hf[:8].any() and (hf[8:] == 0xAB).all()
        assert L.rsbwt_set_meta_by_ordinal_dev(ss._s, p(d_sh), p(d_od), n, None, None, 0, None) == -1
        assert L.rsbwt_set_meta_by_ordinal_dev(ss._s, None, p(d_od), n, p(d_first), None, 0, None) == -1
    finally:
        _close(ss, gs)


def test_gpu_meta_length_ladder_at_every_residue(rsb, ref):
    """every value length of the ladder, and values longer than the lane / wave split copied from every source residue mod
    16 to every destination residue mod 16 (asserted from the offsets): a one-byte value is asked as often as it takes to
    move the next long value's destination on by one"""
    gs = _open(rsb, ref.fx)
    ss = rsb.ShardSet(gs)
    try:
        _build(ss, ref.pairs)
        t = ref.tables[1]
        off = MR.flat(t)[0]  # the table's own offsets: where each value's bytes start
        assert {len(v) for v in t} >= set(MR.LADDER)
        longs = {}
        for o, v in enumerate(t):
            if len(v) > 64:
                longs.setdefault(off[o] % 16, o)
        assert sorted(longs) == list(range(16)), sorted(longs)
        one = next(o for o, v in enumerate(t) if len(v) == 1)
        ods, at, pairs_seen = [], 0, set()
        for s_res, o in sorted(longs.items()):
            for d_res in range(16):
                while at % 16 != d_res:
                    ods.append(one)
                    at += 1
                ods.append(o)
                pairs_seen.add((s_res, at % 16))
                at += len(t[o])
        assert len(pairs_seen) == 256
        shorts = {}
        for o, v in enumerate(t):
            if 0 < len(v) <= 64:
                shorts.setdefault((off[o] % 16, len(v)), o)
        ods += [o for _, o in sorted(shorts.items())] * 17  # (17 = 1 mod 16: the block's residues move on with every repeat)
        efirst, ebytes = MR.flat([t[o] for o in ods])
        assert {(off[o] % 16, efirst[i] % 16) for i, o in enumerate(ods) if len(t[o]) > 64} >= {(a, b) for a in range(16) for b in range(16)}
        assert {efirst[i] % 4 == off[o] % 4 for i, o in enumerate(ods) if 0 < len(t[o]) <= 64} == {True, False}
        first, got = ss.meta_by_ordinal([1] * len(ods), ods, raw=True)
        assert [int(x) for x in first] == efirst
        bad = np.flatnonzero(np.frombuffer(ebytes, np.uint8) != got)
        assert bad.size == 0, (bad[:5], len(ebytes))
    finally:
        _close(ss, gs)


def test_gpu_meta_build_replace_clear_and_load(rsb, ref, tmp_path):
    """the duplicate-string pairs in both orders (the pair with the higher index wins either way); a second build replaces
    the first; clear, then a lookup is RSBWT_EINVAL; rsbwt_set_meta_load of a file = rsbwt_set_meta_build of its pairs"""
    L = rsb.lib()
    gs = _open(rsb, ref.fx)
    ss = rsb.ShardSet(gs)
    try:
        _build(ss, ref.pairs)
        sh, ods = _all_items(ref.tables)
        assert ss.meta_by_ordinal(sh, ods) == MR.by_ordinal(ref.tables, sh, ods)
        bytes_a = ss.meta_bytes()
        # the other order: the earlier values of the strings given twice win now; the stats count the same pairs
        swapped = ref.pairs[::-1]
        t2, s2 = MR.build_tables(ref.orc, swapped)
        assert t2 != ref.tables
        st = _build(ss, swapped)
        assert tuple(st.values()) == s2
        assert ss.meta_by_ordinal(sh, ods) == MR.by_ordinal(t2, sh, ods)
        _check(ss, rsb, ref, "swapped", tables=t2)
        # a second build replaces the first: a few pairs only, everything else becomes empty
        few = ref.pairs[:7]
        t3, s3 = MR.build_tables(ref.orc, few)
        st = _build(ss, few)
        assert tuple(st.values()) == s3 and ss.meta_by_ordinal(sh, ods) == MR.by_ordinal(t3, sh, ods)
        assert ss.meta_bytes() < bytes_a
        # no pairs at all: a table of empty values
        st = _build(ss, [])
        assert tuple(st.values()) == (0, 0, 0, 0) and ss.meta_by_ordinal(sh[:10], ods[:10]) == [b""] * 10
        assert ss.meta_bytes() == sum((len(t) + 1) * 8 for t in ref.tables)
        # the file
        f = tmp_path / "pairs.txt"
        f.write_bytes(b"".join(w.encode() + b"\n" + v + b"\n" for w, v in ref.pairs) + b"ACGTACGT")
        st = ss.meta_load(f)
        assert tuple(st.values()) == ref.stats and ss.meta_bytes() == bytes_a
        assert ss.meta_by_ordinal(sh, ods) == MR.by_ordinal(ref.tables, sh, ods)
        with pytest.raises(rsb.RsbwtError) as e:
            ss.meta_load(tmp_path / "missing.txt")
        assert e.value.code == -2
        assert ss.meta_by_ordinal(sh, ods) == MR.by_ordinal(ref.tables, sh, ods)  # (a failed load leaves the table)
        # a string longer than 65,535 symbols is counted and changes nothing
        st = _build(ss, ref.pairs + [("AC" * 40000, b"too long")])
        assert tuple(st.values()) == (ref.stats[0], ref.stats[1] + 1) + ref.stats[2:]
        assert ss.meta_by_ordinal(sh, ods) == MR.by_ordinal(ref.tables, sh, ods)
        # clear
        ss.meta_clear()
        assert ss.meta_bytes() == 0
        with pytest.raises(rsb.RsbwtError) as e:
            ss.meta_by_ordinal(sh, ods)
        assert e.value.code == -1 and "no sample table" in str(e.value)
        with pytest.raises(rsb.RsbwtError) as e:
            ss.read_meta(ref.asked[:3])
        assert e.value.code == -1
        od, cp = ss.read_ordinals(ref.asked)  # (needs no table)
        assert (cp == np.array(ref.copies, np.uint64)).all()
        # arguments
        assert L.rsbwt_set_meta_build(ss._s, None, None, None, None, 3, None) == -1
        voff = np.array([0, 5, 3], np.uint64)
        off = np.array([0, 4, 8], np.uint64)
        text = np.frombuffer(b"ACGTACGT", np.uint8).copy()
        pv = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
        assert L.rsbwt_set_meta_build(ss._s, pv(text), pv(off), pv(text), pv(voff), 2, None) == -1
        assert ss.meta_bytes() == 0
    finally:
        _close(ss, gs)


@pytest.mark.parametrize("ktab", [None, 2])
def test_gpu_meta_on_a_shard_without_terminators(rsb, ktab):
    """7,037 x 'T' and no '$': nothing is matched, every value is empty"""
    runs = np.full(227, (4 << 5) | 31, np.uint8)
    with rsb.GpuBWT(runs=runs, num_strings=0, ktab_depth=ktab) as g:
        ss = rsb.ShardSet([g])
        try:
            st = ss.meta_build(["TTTT", "T", "A"], [b"abc", b"d", b""])
            assert tuple(st.values()) == (0, 3, 0, 0)
            od, cp = ss.read_ordinals(["TTTT", "A", ""])
            assert not od.any() and not cp.any()
            first, got, cp = ss.read_meta(["TTTT", "A", "", "T"], raw=True)
            assert not first.any() and got.size == 0 and not cp.any()
            assert ss.meta_by_ordinal([0, 0, 0], [0, 1, U64MAX]) == [b"", b"", b""]
            assert rsb.ShardSet.meta_last_work() == dict(items=3, valued=0, bytes=0, lf_steps=0)
        finally:
            ss.close()


def test_gpu_meta_from_eight_threads(rsb, ref):
    """the lookups are re-entrant: eight threads at once get the single-threaded answers and their own work counters"""
    gs = _open(rsb, ref.fx)
    ss = rsb.ShardSet(gs)
    try:
        _build(ss, ref.pairs)
        sfirst, sbytes = MR.flat(ref.vals)
        errs = []

        def work(i):
            try:
                for r in range(4):
                    sh, ods = _all_items(ref.tables, seed=100 + i * 10 + r)
                    sh, ods = sh[:200 + 37 * i], ods[:200 + 37 * i]
                    want = MR.by_ordinal(ref.tables, sh, ods)
                    assert ss.meta_by_ordinal(sh, ods) == want, (i, r)
                    wk = rsb.ShardSet.meta_last_work()
                    assert wk["items"] == len(sh) and wk["bytes"] == sum(len(v) for v in want), (i, r, wk)
                    first, got, cp = ss.read_meta(ref.asked, raw=True)
                    assert [int(x) for x in first] == sfirst and got.tobytes() == sbytes, (i, r)
                    assert rsb.ShardSet.meta_last_work()["bytes"] == len(sbytes), (i, r)
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
