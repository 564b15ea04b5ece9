"""The host paths for queries of lengths of their own share one slicing loop (csrc/capi.hip, for_each_var_slice) and one
per-group scatter (csrc/sets.hip, group_scatter).  Here every caller of the loop crosses the 65,536-query slice boundary,
with a slice that has nothing to search on either side of it, and every caller of the scatter runs on a set whose device
groups interleave in shard order.  Expected values: the oracle's find_interval and the read lists (tests/test_read_copies.py);
the reads of the capped call are those of rsbwt_set_query_var on the distinct queries, which tests/test_gpu_sets.py pins."""
import ctypes as C

import numpy as np
import pytest

import test_kmer_fixtures as F
import test_read_copies as RC
from test_gpu_query_capped import _last_work, _raw_call
from test_gpu_sets import two_devices  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

SLICE, TAIL = 65536, 300
Q = SLICE + TAIL
LIMIT = 5       # the capped call's small limit on the rows of one query
STRIDE = 96     # (the fixture's reads have 70 symbols)


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _interval(oix, w):
    """the oracle's interval; (1, 0) for what the calls refuse: no symbols, a foreign symbol, more than 65,535 symbols"""
    if not w or set(w) - set("ACGT") or len(w) > 65535:
        return 1, 0
    return oix.find_interval(w)


def _copies_var(L, ss, qs, with_ending):
    text, off = ss._var_text(qs)
    S = len(ss.shards)
    cp = np.full((S, len(qs)), 77, np.uint64)
    en = np.full((S, len(qs)), 77, np.uint64)
    rc = L.rsbwt_set_read_copies_var(ss._s, _ptr(text), _ptr(off), len(qs), _ptr(cp), _ptr(en) if with_ending else None)
    assert rc == 0, L.rsbwt_last_error()
    return cp, en


@pytest.fixture(scope="module")
def boundary(rsb, oracle):
    """the two-shard `pop` set; 300 distinct queries -- every fifteenth of the fixture's queries of 16 symbols or more (reads,
    suffixes, prefixes, substrings, changed reads, strings with an N), "", "ACN" and one of 65,536 symbols -- and their
    per-shard answers from the oracle and from the read lists, computed once"""
    fx = F.fixture("pop")
    reads, others = RC.queries("pop")
    long_ones = [w for w in dict.fromkeys(reads + others) if len(w) >= 16]
    rng = np.random.default_rng(65536)
    distinct = long_ones[::15][:TAIL - 3] + ["", "ACN", "".join("ACGT"[x] for x in rng.integers(0, 4, SLICE))]
    assert len(distinct) == TAIL == len(set(distinct))
    oixs = [oracle.from_runs(runs, len(sh)) for sh, runs in zip(fx.shards, fx.runs())]
    iv = np.array([[_interval(oix, w) for w in distinct] for oix in oixs], np.uint64)  # [S][300][2]
    lo, up = iv[:, :, 0], iv[:, :, 1]
    ns = np.array([oix.bwlen() for oix in oixs], np.uint64)[:, None]
    width = np.where((lo <= up) & (up < ns), up - lo + np.uint64(1), np.uint64(0)).astype(np.uint64)
    cp, en = (np.array(x, np.uint64) for x in zip(*(RC.from_reads(sh, distinct) for sh in fx.shards)))
    assert int((cp > 0).sum()) > 50 and int((en > cp).sum()) > 100 and not np.array_equal(lo[0], lo[1])
    gs = [rsb.GpuBWT(runs=runs, num_strings=len(sh), ktab_depth=6) for sh, runs in zip(fx.shards, fx.runs())]
    ss = rsb.ShardSet(gs)
    ref = dict(ss=ss, distinct=distinct, lo=lo, up=up, width=width, copies=cp, ending=en)
    yield ref
    ss.close()
    for g in gs:
        g.close()


def _arrange(which):
    """slot -> index of the distinct query: (i) 65,536 empty queries, then every distinct query once -- slice 0 has nothing
    to search, at q0 = 0; (ii) the distinct queries tiled over 65,536 slots, then 300 empty ones -- the same at q0 = 65,536"""
    empty = TAIL - 3  # distinct[297] == ""
    if which == "empty-first":
        return np.concatenate([np.full(SLICE, empty), np.arange(TAIL)])
    return np.concatenate([np.arange(SLICE) % TAIL, np.full(TAIL, empty)])


ARRANGEMENTS = ["empty-first", "empty-last"]


@pytest.mark.parametrize("which", ARRANGEMENTS)
def test_gpu_intervals_and_counts_across_the_slice_boundary(rsb, boundary, which):
    ss, slot = boundary["ss"], _arrange(which)
    qs = [boundary["distinct"][j] for j in slot]
    assert len(qs) == Q and boundary["distinct"][TAIL - 3] == ""
    lo, up = ss.find_intervals_var(qs)
    assert np.array_equal(lo, boundary["lo"][:, slot]) and np.array_equal(up, boundary["up"][:, slot])
    w = np.where(boundary["up"] >= boundary["lo"], boundary["up"] - boundary["lo"] + np.uint64(1), np.uint64(0))
    assert np.array_equal(ss.count_var(qs), w.sum(axis=0, dtype=np.uint64)[slot])
    assert int(w.sum()) > 500


@pytest.mark.parametrize("which", ARRANGEMENTS)
def test_gpu_read_copies_across_the_slice_boundary(rsb, boundary, which):
    ss, slot = boundary["ss"], _arrange(which)
    qs = [boundary["distinct"][j] for j in slot]
    for with_ending in (True, False):
        cp, en = _copies_var(rsb.lib(), ss, qs, with_ending)
        assert np.array_equal(cp, boundary["copies"][:, slot]), with_ending
        assert np.array_equal(en, boundary["ending"][:, slot]) if with_ending else (en == 77).all()


@pytest.mark.parametrize("which", ARRANGEMENTS)
def test_gpu_capped_query_across_the_slice_boundary(rsb, boundary, which):
    """first[] and matches[] from the oracle's intervals, the reads from rsbwt_set_query_var on the 300 distinct queries; no
    row is uploaded from the host.  The batch's rows stay under 2e5 and some query is over the limit in both arrangements.
    "empty-last" returns more than a thousand rows at either limit; "empty-first" holds every distinct query once, so it
    returns the few hundred rows those have (a set of distinct queries with a thousand rows would, tiled 218 times in the
    other arrangement, pass 2e5)."""
    L = rsb.lib()
    ss, slot, width = boundary["ss"], _arrange(which), boundary["width"]
    qs = [boundary["distinct"][j] for j in slot]
    S = width.shape[0]
    matches = width.sum(axis=0, dtype=np.uint64)
    assert int(matches[slot].sum()) < 200000 and int((matches > LIMIT).sum()) >= 1
    # the distinct queries' reads, query by query: rows [d_first[j], d_first[j + 1])
    rc, n, d_first, *_ = _raw_call(L, ss, boundary["distinct"], 0, 0, STRIDE, fn="rsbwt_set_query_var")
    assert rc in (0, -7) and n == int(matches.sum())
    rc, n, d_first, d_sh, d_ln, d_reads, _ = _raw_call(L, ss, boundary["distinct"], 0, n, STRIDE, fn="rsbwt_set_query_var")
    assert rc == 0 and np.array_equal(np.diff(d_first), matches) and (d_ln[:n] == 70).all()
    # (per query: shard 0's rows first, as many per shard as the oracle's interval is wide)
    assert np.array_equal(d_sh[:n], np.repeat(np.tile(np.arange(S, dtype=np.uint32), TAIL), width.T.reshape(-1).astype(np.int64)))
    for max_rows in (0, LIMIT):
        kept = np.where((matches <= max_rows) | (max_rows == 0), matches, np.uint64(0))
        want_first = np.zeros(Q + 1, np.uint64)
        want_first[1:] = np.cumsum(kept[slot])
        total = int(want_first[Q])
        assert total >= (1000 if which == "empty-last" else 300), (which, max_rows, total)
        rows = np.concatenate([np.arange(int(d_first[j]), int(d_first[j]) + int(kept[j])) for j in slot])
        rc, n, first, sh, ln, reads, got_matches = _raw_call(L, ss, qs, max_rows, total + 2, STRIDE)
        assert rc == 0, L.rsbwt_last_error()
        assert n == total and np.array_equal(first, want_first), (which, max_rows)
        assert np.array_equal(got_matches, matches[slot]), (which, max_rows)
        assert np.array_equal(sh[:n], d_sh[rows]) and np.array_equal(ln[:n], d_ln[rows]), (which, max_rows)
        assert np.array_equal(reads[:n], d_reads[rows]), (which, max_rows)
        over = int((matches[slot] > max_rows).sum()) if max_rows else 0
        assert _last_work(L)[:3] == [total, 0, over], (which, max_rows)


def test_gpu_interleaved_groups_for_queries_of_their_own_lengths(rsb, oracle, two_devices):
    """four shards as device groups (0, 1, 0, 1) -- each group's rows are scattered back by shard -- and on one device: the
    same intervals, counts and whole-read matches, with and without `ending`; shard 0 against the oracle and its read list"""
    L = rsb.lib()
    fxs = [F.fixture(name) for name in ("pop", "repeat", "ragged")]
    shards = [(sh, runs) for fx in fxs for sh, runs in zip(fx.shards, fx.runs())]
    assert len(shards) == 4
    qs = [""]
    for name in ("pop", "repeat", "ragged"):
        reads, others = RC.queries(name)
        qs += reads[::11] + others[::37]
    assert 300 < len(qs) < 1000 and len({len(w) for w in qs}) > 40

    def run(devs):
        gs = [rsb.GpuBWT(runs=runs, num_strings=len(sh), ktab_depth=6, device=d) for (sh, runs), d in zip(shards, devs)]
        ss = rsb.ShardSet(gs)
        try:
            out = [L.rsbwt_set_devices(ss._s), *ss.find_intervals_var(qs), ss.count_var(qs)]
            out += _copies_var(L, ss, qs, True)
            out.append(_copies_var(L, ss, qs, False)[0])
            return out
        finally:
            ss.close()
            for g in gs:
                g.close()
    one, mixed = run([0, 0, 0, 0]), run([0, 1, 0, 1])
    assert (one[0], mixed[0]) == (1, 2)
    for a, b, what in zip(one[1:], mixed[1:], ("lower", "upper", "counts", "copies", "ending", "copies alone")):
        assert np.array_equal(a, b), what
    assert not np.array_equal(mixed[1][1], mixed[1][2]) and not np.array_equal(mixed[4][1], mixed[4][2])  # (rows that differ)
    sh0, runs0 = shards[0]
    oix = oracle.from_runs(runs0, len(sh0))
    iv = np.array([_interval(oix, w) for w in qs], np.uint64)
    assert np.array_equal(mixed[1][0], iv[:, 0]) and np.array_equal(mixed[2][0], iv[:, 1])
    want_c, want_e = (np.array(x, np.uint64) for x in RC.from_reads(sh0, qs))
    assert np.array_equal(mixed[4][0], want_c) and np.array_equal(mixed[5][0], want_e) and np.array_equal(mixed[6][0], want_c)
    assert int(want_c.sum()) > 50 and int((iv[:, 1] >= iv[:, 0]).sum()) > 100
