"""CPU suite: the numpy references of the rank primitives (tests/rank_reference.py) against the naive definition -- the 24
pieces expanded to an array of symbols, counted with == and cumsum -- on 10^4 seeded quarters of every case class the GPU
module (tests/test_gpu_rank_primitives.py) runs, at every argument it asks about; and the inputs of that module's staged-line
sweeps held to what it relies on (how much of them lies past a line's own pieces), from the builder's own statistics."""
import numpy as np
import pytest

import layout_reference as LR
import rank_reference as R
import test_kmer_fixtures as F

N_CASES = 10000


def _cases():
    rng = np.random.default_rng(4101)
    per = N_CASES // 10
    parts = list(R.random_classes(rng, per).values())
    for b in (0, 3):
        for where in (0, 2):
            parts.append(R.exhaustive_pairs(rng, b, where)[rng.integers(0, 65536, per // 2)])
    p = np.concatenate(parts)
    extra = N_CASES - len(p)
    if extra > 0:
        p = np.concatenate([p, R.random_classes(rng, extra)["realistic"]])
    return p[:N_CASES], rng.integers(0, 5, N_CASES)


def test_references_are_the_naive_definition():
    pieces, b = _cases()
    assert len(pieces) == N_CASES
    rems, ts = R.rem_values(pieces), R.select_values(pieces, b)
    got_rank = R.rank_ref(pieces, b, rems)
    got_scan1 = R.rank_ref(pieces[:, :4], b, rems)
    got_scan2 = R.rank_ref(pieces[:, :8], b, rems)
    got_held = R.held_ref(pieces, b)
    got_dw = R.dword_matched_ref(pieces, b, np.full(N_CASES, 7))
    got_c, got_occ = R.char_rank_ref(pieces, rems)
    want_sym = np.where(np.arange(N_CASES) % 2 == 0, b, 0)
    got_cw, got_occw = R.char_rank_ref(pieces, rems, want_sym)
    got_pos, got_left = R.select_ref(pieces, b, ts)
    some_left = some_found = some_short = 0
    for i in range(N_CASES):
        sym, ln = pieces[i] >> 5, (pieces[i] & 31).astype(np.int64)
        arr = np.repeat(sym, ln)  # the quarter's symbols, one per position
        cum = {s: np.concatenate([[0], np.cumsum(arr == s)]) for s in set(sym.tolist()) | {int(b[i]), 0}}
        is_b = cum[int(b[i])]
        for P, got in ((4, got_scan1), (8, got_scan2)):
            part = np.concatenate([[0], np.cumsum(np.repeat(sym[:P], ln[:P]) == b[i])])
            assert got[i].tolist() == [int(part[min(int(r), len(part) - 1)]) for r in rems[i]]
        upto = np.minimum(rems[i].astype(np.int64), arr.size)
        assert got_rank[i].tolist() == is_b[upto].tolist()
        assert int(got_held[i]) == int(is_b[-1])
        assert got_dw[i].tolist() == [7 + int(ln[4 * d:4 * d + 4][sym[4 * d:4 * d + 4] == b[i]].sum()) for d in range(6)]
        for k, r in enumerate(rems[i].astype(np.int64).tolist()):
            here = int(arr[r - 1]) if 1 <= r <= arr.size else 0
            assert int(got_c[i, k]) == here
            assert int(got_occ[i, k]) == int(cum[here][min(r, arr.size)])
            cw = int(want_sym[i]) or here
            assert int(got_cw[i, k]) == cw and int(got_occw[i, k]) == int(cum[cw][min(r, arr.size)])
            some_short += r > arr.size
        where = np.nonzero(arr == b[i])[0]
        for k, t in enumerate(ts[i].astype(np.int64).tolist()):
            if t == 0:
                assert (int(got_pos[i, k]), int(got_left[i, k])) == (0, 0)
            elif t <= where.size:
                assert (int(got_pos[i, k]), int(got_left[i, k])) == (int(where[t - 1]), 0)
                some_found += 1
            else:
                assert int(got_left[i, k]) == t - where.size  # (the position is unspecified here: not compared)
                some_left += 1
        assert R.symbol_at_ref(pieces[i:i + 1], np.arange(arr.size + 2)[None, :])[0].tolist() == arr.tolist() + [255, 255]
    assert some_left > N_CASES and some_found > N_CASES and some_short > N_CASES


def test_case_classes_hold_what_they_are_for():
    rng = np.random.default_rng(5)
    cl = R.random_classes(rng, 2000)
    ln = {k: (v & 31).astype(np.int64) for k, v in cl.items()}
    sy = {k: v >> 5 for k, v in cl.items()}
    assert (ln["all31"] == 31).all() and (ln["all31"].sum(axis=1) == 744).all()
    assert not cl["zero"].any()
    real = (ln["padded"] > 0).sum(axis=1)
    assert set(real.tolist()) == set(range(25))
    assert all((ln["padded"][i, real[i]:] == 0).all() for i in range(200))
    z = (ln["zero_length"] == 0) & (sy["zero_length"] != 0)
    assert (z[:, 1:-1] & (ln["zero_length"][:, :-2] > 0) & (ln["zero_length"][:, 2:] > 0)).any(axis=1).mean() > 0.9
    same = sy["long_runs"][:, 3:8]  # pieces 3 and 4 straddle the border of dwords 0 and 1
    assert (same == same[:, :1]).all(axis=1).mean() > 0.05
    assert (sy["codes_5_7"] >= 5).any(axis=1).mean() > 0.8 and not (sy["realistic"] >= 5).any()
    assert 0.005 < (sy["realistic"] == 0).mean() < 0.02 and np.median(ln["realistic"]) <= 4
    for b, where in ((0, 0), (0, 2), (4, 2)):
        p = R.exhaustive_pairs(rng, b, where)
        assert len(np.unique(p[:, where].astype(np.int64) | (p[:, where + 1].astype(np.int64) << 8))) == 65536
        if where == 2:
            assert ((p[:, :2] >> 5) == b).all() and ((p[:, :2] & 31) > 0).all()
    r = R.rem_values(cl["realistic"])
    assert r.shape == (2000, 78) and (r[:, 0] == 0).all() and (r[:, -1] == 65535).all() and (r[:, -2] == 4095).all()
    assert (r[:, -4] == ln["realistic"].sum(axis=1)).all()
    assert R.select_values(cl["realistic"], np.ones(2000, np.int64)).shape == (2000, 77)


# ---- the staged sweeps' synthetic inputs: how much of each lies past its lines' own pieces ----------------------------

SYNTH_SPANS = (2, 37, 915, 2944)
SPILL_SPANS = (915, 2944)  # chosen FOR their spill; at the others at most 5 % of the positions may lie past their line


def synth_stream(rsb, name):
    """two seeded run streams: `mix` -- the synthesiser's population mix (run lengths around 10, 1 % '$'); `dense` -- runs of
    1..3 symbols, a tenth of them '$', so that wide windows hold hundreds of pieces"""
    if name == "mix":
        runs = np.empty(30000, np.uint8)
        assert rsb.lib().rsbwt_synth_runs_host(runs.ctypes.data, runs.size, 7301) == 0
        return runs
    rng = np.random.default_rng(7302)
    sym = np.where(rng.random(60000) < 0.1, 0, rng.integers(1, 5, 60000))
    return ((sym << 5) | rng.integers(1, 4, 60000)).astype(np.uint8)


@pytest.mark.parametrize("name", ["mix", "dense"])
def test_synthetic_streams_spill_only_where_chosen(rsb, name):
    runs = synth_stream(rsb, name)
    n = int((runs & 31).astype(np.int64).sum())
    for span in SYNTH_SPANS:
        for room in (False, True):
            st = F.selftest(rsb, runs, span, room)
            if span in SPILL_SPANS:
                assert st[5] > 0, (name, span, room, st)
            else:
                assert st[5] < 0.05 * n, (name, span, room, st)


def test_fixture_spans_spill_only_where_chosen(rsb):
    for name, spans in F.SPANS.items():
        fx = F.fixture(name)
        for p, runs in enumerate(fx.runs()):
            assert F.LAYOUT_STATS[(name, p, spans["control"], True)][5] == 0
            for kind in ("chunk", "far"):
                st = F.LAYOUT_STATS[(name, p, spans[kind], True)]
                assert st[5] > 0, (name, p, kind, st)  # chosen for their spill


# ---- the golden popBWT: the span the builder chooses for it, and how much of it then lies past its lines ----------------

# room -> [S, lines, far lines, chunk windows, far windows, spilled symbols] at the builder's own span (measured once,
# asserted exactly below, and asserted against the GPU builder in the GPU module)
GOLDEN_LAYOUT = {
    False: [670, 14434, 1, 2225, 1, 70826],
    True: [638, 15304, 157, 3992, 157, 157669],
}


def golden_layout(rsb, runs, n, room):
    """the builder's choice of span (csrc/build_lines.hip): 88 pieces per window at the mean run length -- 88 * 88 / 96 with
    room for a psi hint -- shrunk by 5 % (1.25 %) while more than 2.5 % of the positions spill or more than 1.5 % of the
    windows need far lines; the statistics are rsbwt_layout_selftest_host's at each span tried"""
    # (the rule itself is tests/layout_reference.py's, shared with the GPU builder's byte tests; this BWT has far fewer
    # than the 4,096 groups at which the builder first tries its spans on a sample)
    st, _ = LR.choose_span(n, runs.size, room, lambda S: (F.selftest(rsb, runs, S, room), None))
    return st


@pytest.mark.parametrize("room", [False, True], ids=["plain", "reads"])
def test_golden_popbwt_spills_little(rsb, fixture_bwt, room):
    from oracle_binding import read_bwt_file
    path, meta = fixture_bwt
    nstr, nsym, runs = read_bwt_file(path)
    st = golden_layout(rsb, np.ascontiguousarray(runs), nsym, room)
    assert st == GOLDEN_LAYOUT[room]
    assert 0 < st[5] < 0.05 * nsym  # the sentinel of the staged sweep hides less than 5 % of the positions, and is exercised
