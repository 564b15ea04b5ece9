"""The one-lane search kernel (csrc/search_solo.h) fetches no line of a window twice within an LF step: an `upper` in
the window of `lower - 1` is ranked off the line (or spill chunk) that lookup staged, or goes on from that line's header
into the window's continuation.  Held three ways: every answer against the oracle on layouts where continuation lines
are common; the fetch counters of the one-lane kernel against those of the lane-pair kernel (search_lines.hip), which
shares a line between its two lanes whenever both want it; and the 1-mismatch hit lists of a spill-heavy set, whose
walk and worklist launches run the same pass body.

The shapes are the smallest at which the library itself picks the one-lane kernel (search_lines.hip, launch_search:
>= 262,144 searches behind a table that leaves narrow intervals): one `pop` shard of 10^6 run bytes = 5,859,075
symbols behind a plain 8-mer table (4 n / 4^8 = 356 <= S), 262,147 queries.  Every launch whose kernel matters is a
counting one and asserts word 12 (WORK_SOLO).  Three layouts of the same runs: the span the library picks (490), 620
(a third of the windows end in a spill chunk, four in ten in a far line) and 900 (nearly every window has a far line,
161 far lines are a window's second)."""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

POP = 1 << 62  # the `pop` run stream (bench.py, STREAM_STYLE)
R, SEED, SEED_B, T = 1_000_000, POP | 11, POP | 12, 8
N_SYMBOLS = 5_859_075
Q = 262_147  # >= 262,144 searches on one shard; 8 n + 3: a tail group of 3
SOLO_MIN = 262_144
SPANS = (0, 620, 900)  # 0: the library's choice for these runs, AUTO_SPAN
AUTO_SPAN = 490
# csrc/layout_host.cpp, rsbwt_layout_selftest_host on these runs: span asked for -> (S, far lines, chunk windows,
# far windows, spilled symbols); far lines - far windows = far lines that are a window's second or later
LAYOUTS = {0: (490, 34, 1951, 34, 73271), 620: (620, 4006, 3200, 4006, 706659), 900: (900, 6569, 102, 6408, 2323349)}


def _runs(rsb, seed):
    runs = np.empty(R, np.uint8)
    assert rsb.lib().rsbwt_synth_runs_host(runs.ctypes.data, R, seed) == 0
    return runs


def _p(t):
    return C.c_void_p(t.data_ptr())


def test_layouts_have_chunk_windows_far_lines_and_far_chains(rsb):
    """The host layout code on the shard's runs at the three spans: the statistics the GPU tests below rely on (and
    compare their shards' far lines and spilled symbols with)."""
    L = rsb.lib()
    runs = _runs(rsb, SEED)
    assert int((runs & 31).sum()) == N_SYMBOLS

    def stats(span):
        st, bad = (C.c_uint64 * 6)(), C.c_uint64()
        assert L.rsbwt_layout_selftest_host(runs.ctypes.data, R, span or AUTO_SPAN, st, C.byref(bad)) == 0, (span, bad.value)
        return tuple(int(st[i]) for i in (0, 2, 3, 4, 5))

    with ThreadPoolExecutor(len(SPANS)) as ex:
        got = dict(zip(SPANS, ex.map(stats, SPANS)))
    assert got == LAYOUTS
    for span, (S, far_lines, chunk_windows, far_windows, spilled) in got.items():
        assert chunk_windows > 0 and far_lines > 0 and spilled > 0 and ((N_SYMBOLS >> (2 * T)) << 2) <= S
    nwin620 = -(-N_SYMBOLS // 620)
    assert LAYOUTS[620][2] > 0.3 * nwin620 and LAYOUTS[620][2] + LAYOUTS[620][3] > 0.7 * nwin620
    assert LAYOUTS[900][1] - LAYOUTS[900][3] > 100  # windows with two far lines


@pytest.fixture(scope="module")
def world(rsb, oracle):
    """the shard at its three layouts, each a handle of its own, and the set of the three; one oracle for all"""
    runs = _runs(rsb, SEED)
    shards = [rsb.GpuBWT(runs=runs, ktab_depth=T, window_span=span) for span in SPANS]
    for g, span in zip(shards, SPANS):
        S, far_lines, _, _, spilled = LAYOUTS[span]
        assert g.getBWLen() == N_SYMBOLS and g.ktab_depth() == T
        assert (g.window_span(), g.far_lines(), g.spilled_symbols()) == (S, far_lines, spilled)
        assert g.far_lines() > 0 and g.spilled_symbols() > 0
    ss = rsb.ShardSet(shards)
    yield {"shards": shards, "set": ss, "oix": oracle.from_runs(runs), "batches": {}}
    ss.close()
    for g in shards:
        g.close()


def _batch(rsb, world, k):
    """Q k-mers, half drawn from the shard and half random, interleaved, two with a foreign symbol; packed on the
    device; the oracle's intervals (the three layouts are one BWT: one answer).  Made once per k."""
    import torch
    if k not in world["batches"]:
        L = rsb.lib()
        rng = np.random.default_rng(1000 + k)
        km = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, (Q, k))].copy()
        half = (Q + 1) // 2
        d_half = torch.empty((half, k), dtype=torch.uint8, device="cuda:0")
        assert L.rsbwt_sample_present_kmers_dev(world["shards"][0].handle, half, k, k, 40 + k, _p(d_half), None) == 0
        torch.cuda.synchronize()
        km[::2] = d_half.cpu().numpy()
        km[5, 3] = ord("N")
        km[Q - 2, 0] = ord("N")
        d_km = torch.from_numpy(km).cuda()
        d_pk = torch.empty((Q, 1), dtype=torch.int64, device="cuda:0")
        d_ok = torch.empty(Q, dtype=torch.uint8, device="cuda:0")
        assert L.rsbwt_pack_kmers_dev(_p(d_km), Q, k, k, _p(d_pk), _p(d_ok), 0, None) == 0
        torch.cuda.synchronize()
        elo, eup = world["oix"].find_intervals(km, nthreads=8)
        world["batches"][k] = (km, d_pk, d_ok, elo, eup)
    return world["batches"][k]


def _search(rsb, target, nshards, d_pk, d_ok, n, k, counting):
    """separate arrays and pairs by one plain or one counting launch each; the counters of the counting launches"""
    import torch
    L = rsb.lib()
    is_set = nshards is not None
    S = nshards if is_set else 1
    h = target._s if is_set else target.handle
    find = L.rsbwt_set_find_intervals_dev if is_set else L.rsbwt_find_intervals_dev
    find_pairs = L.rsbwt_set_find_interval_pairs_dev if is_set else L.rsbwt_find_interval_pairs_dev
    set_counting = L.rsbwt_set_set_counting if is_set else L.rsbwt_set_counting
    counters = L.rsbwt_set_last_search_counters if is_set else L.rsbwt_last_search_counters
    d_lo = torch.full((S, n), -7, dtype=torch.int64, device="cuda:0")
    d_up = torch.full((S, n), -7, dtype=torch.int64, device="cuda:0")
    d_pr = torch.full((S, n, 2), -7, dtype=torch.int64, device="cuda:0")
    ws = []
    assert set_counting(h, 1 if counting else 0) == 0
    try:
        for launch in (lambda: find(h, _p(d_pk), _p(d_ok), n, k, _p(d_lo), _p(d_up), None),
                       lambda: find_pairs(h, _p(d_pk), _p(d_ok), n, k, _p(d_pr), None)):
            assert launch() == 0
            torch.cuda.synchronize()
            if counting:
                w = (C.c_uint64 * 16)()
                assert counters(h, w) == 0
                ws.append([int(x) for x in w])
    finally:
        assert set_counting(h, 0) == 0
    return d_lo.cpu().numpy().view(np.uint64), d_up.cpu().numpy().view(np.uint64), d_pr.cpu().numpy().view(np.uint64), ws


@pytest.mark.gpu
@pytest.mark.parametrize("k", [9, 12, 31])
def test_gpu_solo_line_sharing_parity(rsb, world, k):
    """Every (lower, upper) of the batch on every layout, in both result layouts, by the plain and by the counting
    instantiation: the three layouts as one set (start records made ahead, the plain one-lane kernel) and each shard
    alone (the launch that makes its own start records, FUSED).  k = 9 and 12 are one and four steps behind the table on
    intervals tens of rows wide -- upper in another window, past the line's own pieces, in the next far line; k = 31 is
    the narrow regime."""
    km, d_pk, d_ok, elo, eup = _batch(rsb, world, k)
    live = eup >= elo
    assert live[::2].all() and (k < 31 or not live[1::2].any())  # drawn from the shard: they occur; random 31-mers die
    targets = [("set", world["set"], len(SPANS))] + [(f"span {s}", g, None) for s, g in zip(SPANS, world["shards"])]
    for name, target, nshards in targets:
        for counting in (False, True):
            lo, up, pr, ws = _search(rsb, target, nshards, d_pk, d_ok, Q, k, counting)
            for w in ws:
                assert w[12] == 1, (name, "the batch did not run on the one-lane kernel")
                assert w[0] < w[1] <= 2 * w[0]  # two lookups a step (none for position -1)
            for s in range(lo.shape[0]):
                what = (k, name, s, "counting" if counting else "plain")
                assert np.array_equal(lo[s], elo) and np.array_equal(up[s], eup), what + ("separate arrays",)
                assert np.array_equal(pr[s, :, 0], elo) and np.array_equal(pr[s, :, 1], eup), what + ("pairs",)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [31, 12])
@pytest.mark.parametrize("layout", range(len(SPANS)))
def test_gpu_solo_fetches_the_lines_lane_pairs_fetch(rsb, world, layout, k):
    """The rule as a counter identity.  The batch whole runs on lone lanes; its two halves (< 262,144 searches each) run
    on lane pairs, whose upper lane reads the lower lane's row whenever both want the same line, continuation lines
    included -- so the pairs count the distinct lines each step needs.  Lines fetched (word 2) plus continuation lines
    fetched (word 11) of the whole batch must equal the halves' summed; so must the steps (word 0) and lookups (word 1).
    Before the kernel shared lines within a window the lone lanes' sum was the larger one: at span 620 and k = 31,
    3,587,860 + 554,117 against the pairs' 3,441,195 + 448,459 (now both)."""
    km, d_pk, d_ok, elo, eup = _batch(rsb, world, k)
    g = world["shards"][layout]
    _, _, pr, ws = _search(rsb, g, None, d_pk, d_ok, Q, k, True)
    assert all(w[12] == 1 for w in ws)
    assert np.array_equal(pr[0, :, 0], elo) and np.array_equal(pr[0, :, 1], eup)
    solo = ws[1]
    cut = (Q + 1) // 2
    assert cut < SOLO_MIN
    pair = [0] * 16
    for a, b in ((0, cut), (cut, Q)):
        _, _, prh, wh = _search(rsb, g, None, d_pk[a:b], d_ok[a:b], b - a, k, True)
        assert all(w[12] == 0 for w in wh), "a half ran on the one-lane kernel"
        assert np.array_equal(prh[0, :, 0], elo[a:b]) and np.array_equal(prh[0, :, 1], eup[a:b])
        pair = [x + y for x, y in zip(pair, wh[1])]
    print(f"span {SPANS[layout]} k {k}: lone lanes steps {solo[0]} lookups {solo[1]} lines {solo[2]} continuation lines {solo[11]}; "
          f"lane pairs steps {pair[0]} lookups {pair[1]} lines {pair[2]} continuation lines {pair[11]}")
    assert solo[11] > 0
    assert (solo[0], solo[1]) == (pair[0], pair[1])
    assert solo[2] + solo[11] == pair[2] + pair[11]


@pytest.mark.gpu
def test_gpu_solo_line_sharing_1mm_hit_lists_on_a_spill_heavy_set(rsb, oracle):
    """rsbwt_set_hits_1mm_dev on two `pop` shards laid out at spans 620 and 900 behind the set's 8-mer tables, 1,500
    31-mers: 2 x 1,500 x 94 = 282,000 variant searches, so the resumed launch runs on lone lanes (WL) behind the walk
    (WALK) -- with continuation lines in most windows.  Every shard's list = the oracle's exact search of every
    spelled-out variant, ordered by variant index (the composition of tests/test_gpu_sets.py)."""
    import torch
    from test_gpu_sets import _spelled
    L = rsb.lib()
    k, m = 31, 1500
    V = 3 * k + 1
    shards, oixs = [], []
    for seed, span in ((SEED, 620), (SEED_B, 900)):
        runs = _runs(rsb, seed)
        oixs.append(oracle.from_runs(runs))
        shards.append(rsb.GpuBWT(runs=runs, ktab_depth=None, window_span=span))
        assert shards[-1].window_span() == span and shards[-1].far_lines() > 0 and shards[-1].spilled_symbols() > 0
    ss = rsb.ShardSet(shards)
    try:
        assert L.rsbwt_set_attach_ktabs(ss._s, T) == 0
        S = len(shards)
        assert m * V * S >= SOLO_MIN
        rng = np.random.default_rng(62)
        km = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=(m, k))
        for s, g in enumerate(shards):  # a third from each shard, a third random
            d_part = torch.empty((m // 3, k), dtype=torch.uint8, device="cuda:0")
            assert L.rsbwt_sample_present_kmers_dev(g.handle, m // 3, k, k, 7 + s, _p(d_part), None) == 0
            torch.cuda.synchronize()
            km[s::3][: m // 3] = d_part.cpu().numpy()
        km[1::5, k // 3] = ord("G")  # one substitution away from a present k-mer, often
        km[7, k // 2] = ord("N")
        d_km = torch.from_numpy(km).cuda()
        d_pk = torch.empty((m, 1), dtype=torch.int64, device="cuda:0")
        d_ok = torch.empty(m, dtype=torch.uint8, device="cuda:0")
        assert L.rsbwt_pack_kmers_dev(_p(d_km), m, k, k, _p(d_pk), _p(d_ok), 0, None) == 0
        variants = _spelled(km).reshape(m * V, k)
        want = []
        for oix in oixs:
            elo, eup = oix.find_intervals(variants, nthreads=8)
            elo[7 * V:8 * V], eup[7 * V:8 * V] = 1, 0  # a k-mer with a foreign symbol is invalid as a whole
            idx = np.nonzero(elo <= eup)[0]
            want.append((idx, elo[idx], eup[idx]))
        assert sum(len(w[0]) for w in want) > m // 2
        d_scr = torch.empty(L.rsbwt_set_hits_1mm_scratch_bytes(ss._s, m, k), dtype=torch.uint8, device="cuda:0")
        assert L.rsbwt_set_hits_1mm_is_fused(ss._s, m, k) == 1
        cap = 8 * m
        for counting in (1, 0):  # both instantiations of the walk and of the worklist launch
            d_hits = torch.full((S, cap, 4), -1, dtype=torch.int64, device="cuda:0")
            d_tot = torch.full((S,), -1, dtype=torch.int64, device="cuda:0")
            assert L.rsbwt_set_set_counting(ss._s, counting) == 0
            assert L.rsbwt_set_hits_1mm_dev(ss._s, _p(d_pk), _p(d_ok), m, k, _p(d_hits), cap, _p(d_tot), _p(d_scr), None) == 0
            torch.cuda.synchronize()
            if counting:
                w = (C.c_uint64 * 16)()
                assert L.rsbwt_set_last_search_counters(ss._s, w) == 0 and L.rsbwt_set_set_counting(ss._s, 0) == 0
                assert int(w[12]) == 1  # WORK_SOLO: the resumed launch ran on lone lanes
                assert int(w[11]) > 0   # continuation lines were read
            for s in range(S):
                idx, elo, eup = want[s]
                assert int(d_tot[s].item()) == len(idx), (s, counting)
                n = min(cap, len(idx))
                rec = d_hits[s, :n].cpu().numpy().view(np.uint64)
                assert np.array_equal(rec[:, 2], idx[:n].astype(np.uint64)), (s, counting)
                assert np.array_equal(rec[:, 0], elo[:n]) and np.array_equal(rec[:, 1], eup[:n]), (s, counting)
                assert not rec[:, 3].any()
                assert (d_hits[s, n:] == -1).all()  # nothing past the list's end
    finally:
        ss.close()
        for g in shards:
            g.close()
