"""The rank primitives on the GPU (-m gpu), each on its own, against the plain references of tests/rank_reference.py.

rsbwt_debug_rank_primitives runs one primitive of csrc/rank_device.h per case (24 piece bytes, a symbol b, one argument);
every case is run twice -- b a run-time value, and b a compile-time constant through the instance compiled for it -- and
both are compared with the reference.  (runs_scan's SDWA block was wrong for a compile-time b = 0 only: its accumulator and
`b << 5` shared a register, so pieces 2 and 3 of a dword were compared with the running sum.  No kernel argument could
show that.)  The quarters: every pair of bytes in pieces 0-1 and in pieces 2-3 of dword 0, for every b; 1,050,064 seeded
quarters of eight classes (rank_reference.random_classes).  Every quarter is asked about every argument of
rank_reference.rem_values / select_values.

rsbwt_debug_staged_rank runs the staged-line readers of csrc/wave_lines.h (the LDS-DMA fetch, the swizzled stage, the
header fields, staged_occ_alts, staged_dollars) on positions of a resident shard, against naive cumulative counts of the
expanded run stream: every position of the golden popBWT in both layouts, of the seeded
read sets of tests/test_kmer_fixtures.py at their control / chunk / far spans, and of two synthetic run streams at spans
2, 37, 915 and 2944.  A position past its line's own pieces answers with a sentinel; the sentinel positions are held to be
EXACTLY the builder's spilled symbols, so the sentinel hides nothing else.

select_in24's position is unspecified where *left != 0 (the t-th b is not among the 24 pieces): it is not compared there."""
import numpy as np
import pytest

import rank_reference as R
import test_kmer_fixtures as F
import test_rank_reference as TR
from oracle_binding import read_bwt_file

pytestmark = pytest.mark.gpu

DWORD_MATCHED, MATCHED24, RUNS_SCAN1, RUNS_SCAN2, RANK24, RANK24_DOLLAR, CHAR_RANK24, CHAR_RANK24_WANT, SELECT_IN24 = range(9)
NAMES = ["dword_matched", "matched24_tab", "runs_scan<1>", "runs_scan<2>", "rank24", "rank24_dollar", "char_rank24(want=0)",
         "char_rank24(want=b)", "select_in24"]
FORMS = ((0, "run-time b"), (1, "compile-time b"))
N_PER_PART = 15000    # x 10 parts x 7 classes + 64 all-zero quarters = 1,050,064 random quarters
PARTS = 10            # a class is ten test cases of their own seeds, so that each takes seconds
PAIR_PARTS = 4        # and the 65,536 pairs four
CHUNK = 8192          # quarters per call (x 78 arguments)
ALL_ONES = np.uint64(0xFFFFFFFFFFFFFFFF)


@pytest.fixture(autouse=True)
def _hooks(monkeypatch):
    monkeypatch.setenv("RSBWT_ENABLE_TEST_HOOKS", "1")


def _run(L, op, const_b, cases):
    cases = np.ascontiguousarray(cases, dtype=np.uint32)
    out = np.empty((len(cases), 6 if op == DWORD_MATCHED else 2), np.uint32)
    rc = L.rsbwt_debug_rank_primitives(op, const_b, cases.ctypes.data, len(cases), out.ctypes.data, 0)
    assert rc == 0, L.rsbwt_last_error()
    return out


def _cases(dw, b, args):
    """(N, 6) dwords, (N,) symbols, (N, K) arguments -> (N K, 8) case records"""
    K = args.shape[1]
    c = np.empty((len(dw) * K, 8), np.uint32)
    c[:, :6] = np.repeat(dw, K, axis=0)
    c[:, 6] = np.repeat(b, K)
    c[:, 7] = args.ravel()
    return c


def _same(got, want, what, form, pieces, b, args, mask=None):
    got = got.reshape(want.shape).astype(np.uint64)
    bad = got != want
    if mask is not None:
        bad &= mask
    if bad.any():
        i, k = np.argwhere(bad)[0]
        raise AssertionError(f"{what} ({form}): pieces {pieces[i].tolist()} b {int(b[i])} argument {int(args[i, min(k, args.shape[1] - 1)])}: "
                             f"kernel {int(got[i, k])}, reference {int(want[i, k])}; {int(bad.sum())} of {bad.size} cases differ")


def _check_quarters(L, pieces, b):
    """every primitive, both forms, on these quarters at every argument"""
    b = np.asarray(b, np.int64)
    for s in range(0, len(pieces), CHUNK):
        p, bb = pieces[s:s + CHUNK], b[s:s + CHUNK]
        dw = R.dwords_of(p)
        rems = R.rem_values(p)
        acc = (np.arange(len(p), dtype=np.uint64) * np.uint64(2654435761) & np.uint64(0xFFFFFFFF))[:, None]
        ref = {
            DWORD_MATCHED: R.dword_matched_ref(p, bb, acc[:, 0]),
            MATCHED24: R.held_ref(p, bb)[:, None],
            RUNS_SCAN1: R.rank_ref(p[:, :4], bb, rems),
            RUNS_SCAN2: R.rank_ref(p[:, :8], bb, rems),
            RANK24: R.rank_ref(p, bb, rems),
        }
        ref[RANK24_DOLLAR] = ref[RANK24]  # (compared where b = 0)
        c0, occ0 = R.char_rank_ref(p, rems)
        # want = b != 0: c is b by the contract and occ its rank (tests/test_rank_reference.py holds char_rank_ref(want) to that)
        given = np.broadcast_to((bb != 0)[:, None], rems.shape)
        cw, occw = np.where(given, bb[:, None].astype(np.uint64), c0), np.where(given, ref[RANK24], occ0)
        is_dollar = np.broadcast_to((bb == 0)[:, None], rems.shape)
        one, many = _cases(dw, bb, acc), _cases(dw, bb, rems)
        for const_b, form in FORMS:
            _same(_run(L, DWORD_MATCHED, const_b, one), ref[DWORD_MATCHED], NAMES[DWORD_MATCHED], form, p, bb, acc)
            _same(_run(L, MATCHED24, const_b, one)[:, 0], ref[MATCHED24], NAMES[MATCHED24], form, p, bb, acc)
            for op in (RUNS_SCAN1, RUNS_SCAN2, RANK24):
                _same(_run(L, op, const_b, many)[:, 0], ref[op], NAMES[op], form, p, bb, rems)
            # rank24 with b = 0, rank24_dollar and the reference agree
            _same(_run(L, RANK24_DOLLAR, const_b, many)[:, 0], ref[RANK24], NAMES[RANK24_DOLLAR], form, p, bb, rems, is_dollar)
            for op, (c, occ) in ((CHAR_RANK24, (c0, occ0)), (CHAR_RANK24_WANT, (cw, occw))):
                got = _run(L, op, const_b, many)
                _same(got[:, 0], c, NAMES[op] + ".c", form, p, bb, rems)
                _same(got[:, 1], occ, NAMES[op] + ".occ", form, p, bb, rems)
        # select: the position only where the t-th b is among the pieces; and the round trip there
        ts = R.select_values(p, bb)
        pos, left = R.select_ref(p, bb, ts)
        found = (left == 0) & (ts != 0)
        sel = _cases(dw, bb, ts)
        for const_b, form in FORMS:
            got = _run(L, SELECT_IN24, const_b, sel)
            _same(got[:, 1], left, "select_in24.left", form, p, bb, ts)
            _same(got[:, 0], pos, "select_in24.position", form, p, bb, ts, (left == 0))
            gp = got[:, 0].reshape(ts.shape).astype(np.uint64)
            at = np.where(found, gp, np.uint64(0))
            _same(np.where(found, R.symbol_at_ref(p, at), bb[:, None].astype(np.uint64)), np.broadcast_to(bb[:, None].astype(np.uint64), ts.shape),
                  "symbol at select_in24's position", form, p, bb, ts)
            _same(np.where(found, R.rank_ref(p, bb, at + np.uint64(1)), ts), ts, "rank at select_in24's position", form, p, bb, ts)


CLASSES = ["uniform", "realistic", "all31", "zero", "padded", "zero_length", "long_runs", "codes_5_7"]


@pytest.mark.parametrize("name,part", [(c, k) for c in CLASSES for k in range(1 if c == "zero" else PARTS)])
def test_primitives_on_random_quarters(rsb, name, part):
    rng = np.random.default_rng(9100 + 100 * part + CLASSES.index(name))
    pieces = R.random_classes(rng, N_PER_PART)[name]
    assert len(pieces) == (64 if name == "zero" else N_PER_PART)
    _check_quarters(rsb.lib(), pieces, rng.integers(0, 5, len(pieces)))


@pytest.mark.parametrize("part", range(PAIR_PARTS))
@pytest.mark.parametrize("where", [0, 2], ids=["pieces01", "pieces23"])
@pytest.mark.parametrize("b", range(5))
def test_primitives_on_every_pair_of_bytes(rsb, b, where, part):
    """pieces 0-1 (2-3) of dword 0 take all 65,536 pairs; with the pair in pieces 2-3, pieces 0-1 are non-empty runs of b:
    a matching piece in byte 2 or 3 then follows a non-zero sum -- where a compile-time b = 0 went wrong"""
    rng = np.random.default_rng(9200 + 2 * b + where)
    n = 65536 // PAIR_PARTS
    pieces = R.exhaustive_pairs(rng, b, where)[part * n:(part + 1) * n]  # (the same 65,536 quarters in every part)
    _check_quarters(rsb.lib(), pieces, np.full(n, b))


def test_hooks_are_refused_unless_asked_for_and_take_nothing(rsb, monkeypatch):
    L = rsb.lib()
    case = np.zeros((1, 8), np.uint32)
    out = np.zeros((1, 6), np.uint32)
    one = np.zeros(13, np.uint64)
    assert L.rsbwt_debug_rank_primitives(RANK24, 0, None, 0, None, 0) == 0
    assert L.rsbwt_debug_rank_primitives(RANK24, 0, None, 1, out.ctypes.data, 0) == -1
    assert L.rsbwt_debug_rank_primitives(RANK24, 0, case.ctypes.data, 1, None, 0) == -1
    assert L.rsbwt_debug_rank_primitives(SELECT_IN24 + 1, 0, case.ctypes.data, 1, out.ctypes.data, 0) == -1
    assert L.rsbwt_debug_rank_primitives(RANK24, 0, case.ctypes.data, 1, out.ctypes.data, 1 << 20) == -5  # no such device
    assert L.rsbwt_debug_staged_rank(None, one.ctypes.data, 1, one.ctypes.data) == -1
    runs = np.array([(1 << 5) | 3, (0 << 5) | 1, (2 << 5) | 2], np.uint8)
    with rsb.GpuBWT(runs=runs, ktab_depth=None) as g:
        assert L.rsbwt_debug_staged_rank(g.handle, None, 0, None) == 0
        assert L.rsbwt_debug_staged_rank(g.handle, None, 1, one.ctypes.data) == -1
        assert L.rsbwt_debug_staged_rank(g.handle, one.ctypes.data, 1, None) == -1
        pos = np.array([6], np.uint64)
        assert L.rsbwt_debug_staged_rank(g.handle, pos.ctypes.data, 1, one.ctypes.data) == -7  # past the index
        pos[0] = 5
        assert L.rsbwt_debug_staged_rank(g.handle, pos.ctypes.data, 1, one.ctypes.data) == 0
        assert one.tolist() == [2, 0, 0] + [3, 0, 0] + [3, 2, 0] + [3, 2, 0] + [1]  # AAA$CC
        monkeypatch.delenv("RSBWT_ENABLE_TEST_HOOKS")
        assert L.rsbwt_debug_staged_rank(g.handle, pos.ctypes.data, 1, one.ctypes.data) == -1
        assert L.rsbwt_debug_staged_rank(g.handle, None, 0, None) == -1
    assert L.rsbwt_debug_rank_primitives(RANK24, 0, case.ctypes.data, 1, out.ctypes.data, 0) == -1
    assert L.rsbwt_debug_rank_primitives(RANK24, 0, None, 0, None, 0) == -1
    assert b"test hook" in L.rsbwt_last_error()


# ---- the staged-line readers ------------------------------------------------------------------------------------------

def _cut(runs, cum, a, e):
    """the run bytes of symbols [a, e) of the stream"""
    j0 = int(np.searchsorted(cum, a, side="right"))
    j1 = int(np.searchsorted(cum, e, side="left"))
    sub = runs[j0:j1 + 1].copy()
    sub[0] = (sub[0] & 0xE0) | (min(int(cum[j0]), e) - a)
    if j1 > j0:
        sub[-1] = (sub[-1] & 0xE0) | (e - int(cum[j1 - 1]))
    return sub


def spilled_mask(rsb, runs, S, room):
    """bool per position: it lies past its window line's own pieces.  From the builder's own statistics alone: a group of
    16 windows is laid out from its own symbols (line_format.h, build_group), a window from the symbols up to its end, and
    what a line does not hold are its window's LAST symbols -- so `spilled symbols` of a group cut at the end of each of
    its windows in turn gives every window's spilled tail."""
    lens = (runs & 31).astype(np.int64)
    cum = np.cumsum(lens)
    n = int(cum[-1])
    mask = np.zeros(n, bool)
    for a in range(0, n, F.GROUP * S):
        e = min(a + F.GROUP * S, n)
        if F.selftest(rsb, _cut(runs, cum, a, e), S, room)[5] == 0:
            continue
        prev = 0
        for end in range(a + S, e + S, S):
            end = min(end, e)
            sp = F.selftest(rsb, _cut(runs, cum, a, end), S, room)[5]
            mask[end - (sp - prev):end] = True
            prev = sp
    return mask


def _sweep(rsb, g, runs, pos):
    """every position of pos: the 12 base counts and the '$' count against naive cumulative counts of the expanded stream;
    returns the sentinel mask"""
    L = rsb.lib()
    bwt = np.repeat(runs >> 5, (runs & 31).astype(np.int64))
    assert bwt.size == g.getBWLen() < 1 << 32
    naive = [np.cumsum(bwt == c, dtype=np.uint32) for c in range(5)]
    sent = np.zeros(pos.size, bool)
    step = 1 << 20
    out = np.empty((step, 13), np.uint64)
    for s in range(0, pos.size, step):
        part = np.ascontiguousarray(pos[s:s + step])
        o = out[:part.size]
        assert L.rsbwt_debug_staged_rank(g.handle, part.ctypes.data, part.size, o.ctypes.data) == 0, L.rsbwt_last_error()
        snt = o[:, 0] == ALL_ONES
        assert not o[snt, 1:].any()  # the sentinel and nothing else
        sent[s:s + part.size] = snt
        for c in range(5):
            want = naive[c][part.astype(np.int64)].astype(np.uint64)
            cols = [12] if c == 0 else [3 * orig + (c - 1 if c - 1 < orig else c - 2) for orig in range(4) if orig != c - 1]
            assert len(cols) == (1 if c == 0 else 3)
            for col in cols:
                bad = ~snt & (o[:, col] != want)
                if bad.any():
                    i = int(np.argmax(bad))
                    raise AssertionError(f"Occ({'$ACGT'[c]}, {int(part[i])}) = {int(o[i, col])} in column {col}, naive count {int(want[i])}: "
                                         f"{int(bad.sum())} of {part.size} positions differ (S = {g.window_span()})")
    return sent


def _full_sweep(rsb, runs, span, room, spill_chosen, num_strings=0):
    with rsb.GpuBWT(runs=runs, num_strings=num_strings, ktab_depth=None, window_span=span, for_reads=room) as g:
        S, n = g.window_span(), g.getBWLen()
        assert S == span and rsb.lib().rsbwt_opened_for_reads(g.handle) == int(room)
        st = F.selftest(rsb, runs, S, room)
        assert (g.far_lines(), g.spilled_symbols()) == (st[2], st[5])
        sent = _sweep(rsb, g, runs, np.arange(n, dtype=np.uint64))
        # the sentinel hides the spilled symbols and nothing else: their number, and the very positions
        assert int(sent.sum()) == g.spilled_symbols()
        assert np.array_equal(sent, spilled_mask(rsb, runs, S, room))
        if spill_chosen:
            assert sent.any()
        else:
            assert sent.sum() < 0.05 * n


@pytest.mark.parametrize("room", [False, True], ids=["plain", "reads"])
def test_staged_readers_on_the_golden_popbwt(rsb, fixture_bwt, room):
    """EVERY position (the stride of 3 that tests/test_gpu_sets.py takes above 3e6 symbols is not needed: a full sweep is
    what lets the sentinels be counted against rsbwt_spilled_symbols).  The sentinel positions are held to their NUMBER --
    the builder's spilled symbols, which tests/test_rank_reference.py has from the host-side layout at this span -- and to
    their shape (a window's tail), not to spilled_mask position by position as the small inputs are: the mask takes a
    host-side layout per window of every group that spills, about 14,000 windows of 9e6 symbols here.  With
    RSBWT_OPEN_READS the lines hold at most 88 / 84 pieces and the hint words sit in dwords 30-31 / 29-30, inside quarter
    3's six dwords: no position may count them."""
    path, meta = fixture_bwt
    nstr, nsym, runs = read_bwt_file(path)
    with rsb.GpuBWT(path, ktab_depth=None, for_reads=room) as g:
        S, n = g.window_span(), g.getBWLen()
        assert n == nsym == meta["num_symbols"]
        # the layout the CPU guard laid out on the host and held below 5 % spill
        want = TR.GOLDEN_LAYOUT[room]
        assert [S, g.num_lines(), g.far_lines(), g.spilled_symbols()] == [want[0], want[1], want[2], want[5]]
        if room:  # every line keeps its last 8 piece bytes for the hint, and the hint pass has filled them
            assert rsb.lib().rsbwt_opened_for_reads(g.handle) == 1 and rsb.lib().rsbwt_psi_hint_lines(g.handle) > 0
        sent = _sweep(rsb, g, runs, np.arange(n, dtype=np.uint64))
        assert int(sent.sum()) == g.spilled_symbols() and 0 < sent.sum() < 0.05 * n
        # a line's own pieces are its window's first symbols: within a window no held position follows a spilled one
        ends = np.nonzero(sent[:-1] & ~sent[1:])[0] + 1
        assert (ends % S == 0).all()


_FIXTURE_CASES = [(name, kind, room) for name in ("pop", "repeat", "ragged") for kind, room in
                  (("control", True), ("chunk", True), ("far", True), ("far", False))]


@pytest.mark.parametrize("name,kind,room", _FIXTURE_CASES, ids=[f"{a}-{b}-{'reads' if c else 'plain'}" for a, b, c in _FIXTURE_CASES])
def test_staged_readers_on_the_seeded_read_sets(rsb, name, kind, room):
    fx = F.fixture(name)
    for sh, runs in zip(fx.shards, fx.runs()):
        _full_sweep(rsb, runs, F.SPANS[name][kind], room, spill_chosen=kind != "control", num_strings=len(sh))


@pytest.mark.parametrize("room", [False, True], ids=["plain", "reads"])
@pytest.mark.parametrize("span", TR.SYNTH_SPANS)
@pytest.mark.parametrize("name", ["mix", "dense"])
def test_staged_readers_on_synthetic_streams(rsb, name, span, room):
    _full_sweep(rsb, TR.synth_stream(rsb, name), span, room, spill_chosen=span in TR.SPILL_SPANS)
