"""Locate (csrc/locate.hip; the set forms in csrc/sets.hip) on the GPU (-m gpu): SA row -> (read_row, ordinal, offset), held
to tests/locate_reference.py -- a truth table made from the read lists and the suffix sort alone, which
tests/test_locate_reference.py pins to the oracle's LF walks and '$' ranks on the CPU.

The layout matrix is tests/test_kmer_fixtures.LAYOUTS less locate_reference.DROPPED: the (fixture, span) pairs on which
the CPU guard cannot show an identity row in a window of the layout's kind (all of them spans with spill chunks) are not
run here.  Only valid BWTs are walked; rows past the index and the step cap are the only ways to "not located"."""
import ctypes as C

import numpy as np
import pytest

import locate_reference as R
import test_kmer_fixtures as F
from test_gpu_kmer_layouts import Ref, _check_layout, _open

pytestmark = pytest.mark.gpu

LAYOUTS = R.gpu_layouts()
NONE64, NONE32 = R.NONE64, R.NONE32


@pytest.fixture(scope="module")
def refs(oracle):
    built = {}

    def get(name):
        if name not in built:
            built[name] = Ref(oracle, name)
        return built[name]
    return get


def _close(ss, gs):
    if ss is not None:
        ss.close()
    for g in gs:
        g.close()


def _same(got, want, where):
    for name, g, w in zip(("read_row", "ordinal", "offset"), got, want):
        bad = np.nonzero(np.asarray(g) != np.asarray(w))[0]
        assert bad.size == 0, (where, name, int(bad[0]), int(np.asarray(g)[bad[0]]), int(np.asarray(w)[bad[0]]), bad.size)


# ---- 4. every row on every layout ------------------------------------------------------------------------------------

@pytest.mark.parametrize("lay", LAYOUTS, ids=[F.layout_id(x) for x in LAYOUTS])
def test_gpu_locate_every_row_on_every_layout(rsb, refs, lay):
    """all rows of each shard in ONE call: the three outputs equal the truth table, and the work counters are exactly
    {rows, sum of offsets} -- no row walked twice, none dropped"""
    name, kind, span, room, ktab = lay
    ref = refs(name)
    gs = _open(rsb, ref, span, room, ktab)
    try:
        _check_layout(rsb, ref, gs, kind, span, room)
        for p, (g, t) in enumerate(zip(gs, R.truth(ref.fx))):
            assert g.getBWLen() == t.n and g.num_strings() == len(ref.fx.shards[p])
            got = g.locate(np.arange(t.n, dtype=np.uint64))
            _same(got, (t.read_row, t.ordinal, t.offset), (F.layout_id(lay), p))
            work = rsb.ShardSet.locate_last_work()
            assert work == dict(located=t.n, lf_steps=int(t.offset.astype(np.int64).sum())), (F.layout_id(lay), p, work)
    finally:
        _close(None, gs)


# ---- 5. hand-out edges -----------------------------------------------------------------------------------------------

def test_gpu_locate_hand_out_edges(rsb, refs):
    """batches of 1, 63, 64, 65 and 4,099 rows -- unsorted, with duplicates -- one row 200 times, and the device form with
    only d_offset and with only d_ordinal"""
    import torch
    L = rsb.lib()
    ref = refs("pop")
    span = F.SPANS["pop"]["chain"]
    g = _open(rsb, ref, span, True, 6, shards=(0,))[0]
    t = R.truth(ref.fx)[0]
    rng = np.random.default_rng(505)
    try:
        for n in (1, 63, 64, 65, 4099):
            rows = rng.integers(0, t.n, n).astype(np.uint64)
            rows[n // 2:] = rows[:n - n // 2]  # every row of the first half once more
            rng.shuffle(rows)
            _same(g.locate(rows), t.expect(rows), ("host", n))
            assert rsb.ShardSet.locate_last_work() == dict(located=n, lf_steps=int(t.offset[rows.astype(np.int64)].astype(np.int64).sum()))
            d_rows = torch.from_numpy(rows.view(np.int64)).cuda()
            d_of = torch.full((n + 1,), 0x55555555, dtype=torch.int32, device="cuda")
            d_od = torch.full((n + 1,), 0x5555555555555555, dtype=torch.int64, device="cuda")
            assert L.rsbwt_locate_dev(g.handle, d_rows.data_ptr(), n, 0, None, None, d_of.data_ptr(), None) == 0, L.rsbwt_last_error()
            assert L.rsbwt_locate_dev(g.handle, d_rows.data_ptr(), n, 0, None, d_od.data_ptr(), None, None) == 0, L.rsbwt_last_error()
            torch.cuda.synchronize()
            want = t.expect(rows)
            of, od = d_of.cpu().numpy().view(np.uint32), d_od.cpu().numpy().view(np.uint64)
            assert np.array_equal(of[:n], want[2]) and of[n] == 0x55555555, ("dev offset", n)
            assert np.array_equal(od[:n], want[1]) and od[n] == 0x5555555555555555, ("dev ordinal", n)
        deep = int(np.argmax(t.offset))  # the longest walk of the shard, 200 times
        rows = np.full(200, deep, np.uint64)
        _same(g.locate(rows), t.expect(rows), "one row 200 times")
        assert rsb.ShardSet.locate_last_work() == dict(located=200, lf_steps=200 * int(t.offset[deep]))
    finally:
        g.close()


# ---- 6. the step cap and rows past the index -------------------------------------------------------------------------

def test_gpu_locate_step_cap_and_bad_rows(rsb, refs):
    ref = refs("ragged")
    g = _open(rsb, ref, F.SPANS["ragged"]["far"], True, None)[0]
    t = R.truth(ref.fx)[0]
    try:
        rows = np.arange(t.n, dtype=np.uint64)
        # max_steps = 50: exactly the rows with offset <= 50 are located
        got = g.locate(rows, max_steps=50)
        _same(got, t.expect(rows, 50), "cap 50")
        located = t.offset <= 50
        assert 0 < located.sum() < t.n and np.array_equal(got[2] != NONE32, located)
        assert (got[0][~located] == NONE64).all() and (got[1][~located] == NONE64).all()
        # max_steps = 1: the '$'-symbol rows and the rows one step from them
        got = g.locate(rows, max_steps=1)
        _same(got, t.expect(rows, 1), "cap 1")
        assert np.array_equal(got[2] != NONE32, t.offset <= 1) and (t.offset == 0).sum() == len(ref.fx.shards[0]) and (t.offset == 1).sum() > 0
        # rows past the index among good ones
        rng = np.random.default_rng(606)
        mix = rng.integers(0, t.n, 300).astype(np.uint64)
        mix[[0, 7, 64, 65, 150, 299]] = np.array([t.n, t.n + 1, 2 ** 64 - 1, t.n, 2 ** 64 - 1, t.n + 1], np.uint64)
        got = g.locate(mix)
        _same(got, t.expect(mix), "bad rows")
        assert (got[2] == NONE32).sum() == 6
        assert rsb.ShardSet.locate_last_work()["located"] == 294
    finally:
        g.close()


# ---- 7. sets ---------------------------------------------------------------------------------------------------------

def _interleaved(ts, rng, n):
    sh = rng.integers(0, len(ts), n).astype(np.uint32)
    rows = np.array([rng.integers(0, ts[s].n) for s in sh], np.uint64)
    return sh, rows


def _expect_set(ts, sh, rows, max_steps=0):
    out = [np.empty(rows.size, np.uint64), np.empty(rows.size, np.uint64), np.empty(rows.size, np.uint32)]
    for s, t in enumerate(ts):
        m = sh == s
        for o, e in zip(out, t.expect(rows[m], max_steps)):
            o[m] = e
    return out


def test_gpu_set_locate_host_and_device_forms(rsb, refs):
    """the two pop shards as one set: rows of both shards interleaved through rsbwt_set_locate, and rsbwt_set_locate_dev
    fed by rsbwt_set_interval_rows_dev where it left its rows"""
    import torch
    L = rsb.lib()
    ref = refs("pop")
    ts = R.truth(ref.fx)
    gs = _open(rsb, ref, F.SPANS["pop"]["far"], True, 6)
    ss = rsb.ShardSet(gs)
    p = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    try:
        rng = np.random.default_rng(707)
        sh, rows = _interleaved(ts, rng, 5000)
        rows[[3, 4000]] = np.array([ts[sh[3]].n, 2 ** 64 - 1], np.uint64)
        _same(ss.locate(sh, rows), _expect_set(ts, sh, rows), "set host")
        assert rsb.ShardSet.locate_last_work()["located"] == 4998
        _same(ss.locate(sh, rows, max_steps=20), _expect_set(ts, sh, rows, 20), "set host, cap 20")
        # intervals -> rows on the device -> locate on the device
        qs = ref.fx.queries(12, 0) + ["ACG", "T"]
        lo, up = ss.find_intervals_var(qs)
        Q = len(qs)
        pairs = np.stack([lo, up], axis=-1).astype(np.uint64)
        d_pairs = torch.from_numpy(pairs.view(np.int64)).cuda()
        width = np.where((lo <= up) & (up < np.array([[t.n] for t in ts], np.uint64)), up - lo + np.uint64(1), np.uint64(0)).astype(np.int64)
        total = int(width.sum())
        assert total > 5000
        d_first = torch.zeros(Q + 1, dtype=torch.int64, device="cuda")
        d_matches = torch.zeros(Q, dtype=torch.int64, device="cuda")
        d_shard = torch.zeros(total, dtype=torch.int32, device="cuda")
        d_rows = torch.zeros(total, dtype=torch.int64, device="cuda")
        d_rr, d_od = torch.zeros(total, dtype=torch.int64, device="cuda"), torch.zeros(total, dtype=torch.int64, device="cuda")
        d_of = torch.zeros(total, dtype=torch.int32, device="cuda")
        assert L.rsbwt_set_interval_rows_dev(ss._s, p(d_pairs), Q, 0, p(d_first), p(d_matches), p(d_shard), p(d_rows), total, None) == 0
        assert L.rsbwt_set_locate_dev(ss._s, p(d_shard), p(d_rows), total, 0, p(d_rr), p(d_od), p(d_of), None) == 0, L.rsbwt_last_error()
        torch.cuda.synchronize()
        got_sh, got_rows = d_shard.cpu().numpy().view(np.uint32), d_rows.cpu().numpy().view(np.uint64)
        assert int(d_first.cpu().numpy()[Q]) == total
        got = (d_rr.cpu().numpy().view(np.uint64), d_od.cpu().numpy().view(np.uint64), d_of.cpu().numpy().view(np.uint32))
        _same(got, _expect_set(ts, got_sh, got_rows), "set dev")
        assert (got[2] != NONE32).all()
    finally:
        _close(ss, gs)


def test_gpu_set_locate_shards_of_different_layouts(rsb, refs):
    """shard 0 at the builder's span, shard 1 at the far-chain span, in ONE set and one launch"""
    ref = refs("pop")
    ts = R.truth(ref.fx)
    far = F.SPANS["pop"]["chain"]
    gs = [_open(rsb, ref, sp, True, 6, shards=(p,))[0] for p, sp in enumerate((0, far))]
    ss = rsb.ShardSet(gs)
    try:
        st = F.LAYOUT_STATS[("pop", 1, far, True)]
        assert (gs[1].window_span(), gs[1].far_lines(), gs[1].spilled_symbols()) == (far, st[2], st[5])
        sh = np.concatenate([np.full(t.n, s, np.uint32) for s, t in enumerate(ts)])
        rows = np.concatenate([np.arange(t.n, dtype=np.uint64) for t in ts])
        perm = np.random.default_rng(808).permutation(rows.size)
        sh, rows = sh[perm], rows[perm]
        _same(ss.locate(sh, rows), _expect_set(ts, sh, rows), "mixed layouts")
        assert rsb.ShardSet.locate_last_work() == dict(located=rows.size, lf_steps=sum(int(t.offset.astype(np.int64).sum()) for t in ts))
    finally:
        _close(ss, gs)


def test_gpu_set_locate_on_two_logical_devices(rsb, refs, monkeypatch):
    """the same host calls on a set split over two devices (two logical devices on GPU 0 through the library's test hook
    where the box has one GPU, set the way tests/test_gpu_sets.py sets it): a launch per device group, side by side"""
    L = rsb.lib()
    if L.rsbwt_device_count() < 2:
        monkeypatch.setenv("RSBWT_ENABLE_TEST_HOOKS", "1")
        monkeypatch.setenv("RSBWT_TEST_DEVICE_ALIASES", "2")
    ref = refs("pop")
    ts = R.truth(ref.fx)
    span = F.SPANS["pop"]["far"]
    gs = [rsb.GpuBWT(runs=runs, num_strings=len(sh), ktab_depth=6, window_span=span, for_reads=True, device=p)
          for p, (sh, runs) in enumerate(zip(ref.fx.shards, ref.fx.runs()))]
    ss = rsb.ShardSet(gs)
    try:
        assert L.rsbwt_set_devices(ss._s) == 2
        rng = np.random.default_rng(909)
        sh, rows = _interleaved(ts, rng, 3000)
        rows[5] = np.uint64(2 ** 64 - 1)
        _same(ss.locate(sh, rows), _expect_set(ts, sh, rows), "two devices")
        assert rsb.ShardSet.locate_last_work()["located"] == 2999
        qs = ref.fx.queries(15, 1) + ["A", "ACNT"]
        two = ss.locate_queries(qs, max_rows=40)
    finally:
        _close(ss, gs)
    gs = _open(rsb, ref, span, True, 6)
    ss = rsb.ShardSet(gs)
    try:
        one = ss.locate_queries(qs, max_rows=40)
    finally:
        _close(ss, gs)
    assert int(one["first"][-1]) > 0 and (one["matches"] > 40).any()
    for key in one:
        assert np.array_equal(one[key], two[key]), key


def test_gpu_locate_queries_host_path_at_every_limit(rsb, refs, monkeypatch):
    """rsbwt_set_locate_var_capped on two device groups (limit and expansion on the host) against the one-group set (both
    on the GPU), at limits 0, 1 and 5, in the two forms that walk nothing: every output null (the sizing call), and
    shard / row wanted with read_row / ordinal / offset null"""
    L = rsb.lib()
    if L.rsbwt_device_count() < 2:
        monkeypatch.setenv("RSBWT_ENABLE_TEST_HOOKS", "1")
        monkeypatch.setenv("RSBWT_TEST_DEVICE_ALIASES", "2")
    ref = refs("pop")
    span = F.SPANS["pop"]["far"]
    cut = [ref.fx.shards[p][i][o:o + k] for p in (0, 1) for i, o, k in ((0, 3, 9), (7, 17, 12), (11, 30, 10))]  # 4 to 12 rows each
    qs = ref.fx.queries(15, 1) + cut + ["A", "ACNT", ""]
    Q = len(qs)
    pv = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731

    def run(devices):
        gs = [rsb.GpuBWT(runs=runs, num_strings=len(sh), ktab_depth=6, window_span=span, for_reads=True, device=d)
              for d, sh, runs in zip(devices, ref.fx.shards, ref.fx.runs())]
        ss = rsb.ShardSet(gs)
        try:
            assert L.rsbwt_set_devices(ss._s) == len(set(devices))
            text, off = ss._var_text(qs)
            out = []
            for max_rows in (0, 1, 5):
                first, matches = np.full(Q + 1, 77, np.uint64), np.full(Q, 77, np.uint64)
                n = C.c_size_t(12345)
                rc = L.rsbwt_set_locate_var_capped(ss._s, pv(text), pv(off), Q, max_rows, 0, pv(first), None, None, None, None, None, 0,
                                                   C.byref(n), pv(matches))
                total = n.value
                assert rc == (-7 if total else 0) and total == int(first[Q]), (devices, max_rows, rc)
                first2, matches2 = np.full(Q + 1, 77, np.uint64), np.full(Q, 77, np.uint64)
                sh, rows = np.full(total + 1, 0xA5A5A5A5, np.uint32), np.full(total + 1, 2 ** 64 - 1, np.uint64)
                n2 = C.c_size_t(12345)
                rc = L.rsbwt_set_locate_var_capped(ss._s, pv(text), pv(off), Q, max_rows, 0, pv(first2), pv(sh), pv(rows), None, None, None,
                                                   total, C.byref(n2), pv(matches2))
                assert rc == 0, L.rsbwt_last_error()
                assert sh[total] == 0xA5A5A5A5 and rows[total] == 2 ** 64 - 1
                assert rsb.ShardSet.locate_last_work() == dict(located=0, lf_steps=0)
                out.append(dict(nrows=np.array([total, n2.value]), first=first, matches=matches, first2=first2, matches2=matches2, shard=sh, row=rows))
            return out
        finally:
            _close(ss, gs)
    one, two = run([0, 0]), run([0, 1])
    assert int(one[0]["nrows"][0]) > int(one[2]["nrows"][0]) > int(one[1]["nrows"][0]) > 0  # (each limit cuts: "A" alone is thousands of rows)
    for max_rows, a, b in zip((0, 1, 5), one, two):
        assert a["nrows"][0] == a["nrows"][1]
        for key in a:
            assert np.array_equal(a[key], b[key]), (max_rows, key)


# ---- 8. the query form against plain string search -------------------------------------------------------------------

def _check_queries(ss, ref, ts, qs, where):
    shards = ref.fx.shards
    S, Q = len(shards), len(qs)
    res = ss.locate_queries(qs)
    first, matches = res["first"], res["matches"]
    reads_q, m_q = ss.query_var_capped(qs, 0, read_stride=1024)  # (ragged holds reads of 600 symbols)
    # first[] / matches[] of the string form on the same input
    assert np.array_equal(matches, m_q), where
    assert [int(first[q + 1] - first[q]) for q in range(Q)] == [sum(len(x) for x in reads_q[q]) for q in range(Q)], where
    nonempty = 0
    for q, w in enumerate(qs):
        a, b = int(first[q]), int(first[q + 1])
        sh, rows = res["shard"][a:b], res["row"][a:b]
        # the documented order: shard ascending, SA row ascending inside a shard
        key = sh.astype(np.int64) * (1 << 40) + rows.astype(np.int64)
        assert (np.diff(key) > 0).all(), (where, q, w)
        got = set()
        for s, r, rr, od, of in zip(sh, rows, res["read_row"][a:b], res["ordinal"][a:b], res["offset"][a:b]):
            t = ts[int(s)]
            r = int(r)
            assert (int(rr), int(od), int(of)) == (int(t.read_row[r]), int(t.ordinal[r]), int(t.offset[r])), (where, q, w, r)
            got.add((int(s), int(t.read[r]), int(of)))
        want = R.string_matches(shards, w) if set(w) <= set("ACGT") else set()
        assert got == want and len(got) == b - a == int(matches[q]), (where, q, w, len(got), len(want))
        nonempty += bool(want)
    assert nonempty >= 3, where  # (str.find: the queries cut from reads occur, the 1-symbol query everywhere)
    return res


@pytest.mark.parametrize("name,pairs", [("pop", ((12, 0), (20, 3))), ("repeat", ((15, 1), (12, 8))), ("ragged", ((8, 0), (31, 5)))])
def test_gpu_locate_queries_against_string_search(rsb, refs, name, pairs):
    L = rsb.lib()
    ref = refs(name)
    ts = R.truth(ref.fx)
    span = F.SPANS[name]["far" if name != "repeat" else "deep"]
    gs = _open(rsb, ref, span, True, 6)
    ss = rsb.ShardSet(gs)
    try:
        for k, skip in pairs:
            qs = ref.fx.queries(k, skip)
            qs = qs + ["G", qs[0][:5] + "N" + qs[0][6:12]]
            res = _check_queries(ss, ref, ts, qs, (name, k, skip))
            # a limit of 5 rows: queries over it bring nothing, matches[] still counts them, the others are unchanged
            cap = ss.locate_queries(qs, max_rows=5)
            assert np.array_equal(cap["matches"], res["matches"]) and (res["matches"] > 5).any() and (res["matches"] <= 5).any()
            for q in range(len(qs)):
                a, b = int(res["first"][q]), int(res["first"][q + 1])
                ca, cb = int(cap["first"][q]), int(cap["first"][q + 1])
                if res["matches"][q] > 5:
                    assert ca == cb, (name, k, skip, q)
                else:
                    assert cb - ca == b - a
                    for key in ("shard", "row", "read_row", "ordinal", "offset"):
                        assert np.array_equal(cap[key][ca:cb], res[key][a:b]), (name, k, skip, q, key)
            # the sizing call
            text, off = ss._var_text(qs)
            first = np.zeros(len(qs) + 1, np.uint64)
            n = C.c_size_t()
            pv = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
            rc = L.rsbwt_set_locate_var_capped(ss._s, pv(text), pv(off), len(qs), 0, 0, pv(first), None, None, None, None, None, 0, C.byref(n), None)
            assert rc == -7 and n.value == int(res["first"][-1]) and np.array_equal(first, res["first"])
    finally:
        _close(ss, gs)


# ---- 9. consistency with extraction on the golden fixture ------------------------------------------------------------

def test_gpu_locate_agrees_with_extraction_on_the_golden_index(rsb, fixture_bwt):
    path, _ = fixture_bwt
    with rsb.GpuBWT(path) as g:
        n = g.getBWLen()
        rows = np.random.default_rng(1001).integers(0, n, 1000).astype(np.uint64)
        rr, od, of = g.locate(rows)
        assert (of != NONE32).all() and (od < np.uint64(g.num_strings())).all()
        reads, pl = rsb.extract_reads(g, rows, stride=512)
        assert np.array_equal(pl, of)
        reads0, pl0 = rsb.extract_reads(g, rr, stride=512)
        assert reads0 == reads and (pl0 == 0).all()
        # the '$' rank the other way: the oracle-checked getOcc mirror
        for i in range(0, 1000, 97):
            assert g.getOcc("$", int(rr[i])) - 1 == int(od[i])
