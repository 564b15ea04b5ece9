"""CPU guards of the locate tests (tests/test_gpu_locate.py): the truth table of tests/locate_reference.py -- made from the
read lists and the suffix sort alone -- agrees with the oracle's LF walks and '$' ranks, and on every continuation layout
of the GPU matrix a window that holds an identity row ('$' symbol: where a walk ends and the '$' count is taken) is shown,
by counting, to be a window of the layout's kind."""
import numpy as np
import pytest

import locate_reference as R
import test_kmer_fixtures as F
from kmer_reference import Walks


@pytest.mark.parametrize("name,every", [("repeat", 1), ("ragged", 1), ("pop", 7)])
def test_truth_table_agrees_with_the_oracle(oracle, name, every):
    """Walks.identity / Walks.steps are read_row / offset, oracle.occ('$', read_row) - 1 is ordinal, and the ordinals of a
    shard are a permutation of range(num_strings)"""
    fx = F.fixture(name)
    for sh, runs, t in zip(fx.shards, fx.runs(), R.truth(fx)):
        oix = oracle.from_runs(runs, len(sh))
        assert oix.bwlen() == t.n == sum(len(r) + 1 for r in sh)
        wk = Walks(oix)
        occ = {}
        for r in range(0, t.n, every):
            rr = wk.identity(r)
            assert rr == int(t.read_row[r]) and wk.steps(r) == int(t.offset[r]), (name, r)
            if rr not in occ:
                occ[rr] = oix.occ("$", rr) - 1
            assert occ[rr] == int(t.ordinal[r]), (name, r)
        ids = t.identity_rows()
        assert len(ids) == len(sh)
        assert sorted(int(t.ordinal[r]) for r in ids) == list(range(len(sh)))
        assert all(oix.char(int(r)) == "$" for r in ids[::17])
        # the terminator block: the first num_strings rows, offset = the read's length
        assert all(int(t.offset[r]) == len(sh[int(t.read[r])]) for r in range(len(sh)))


_GUARDED = sorted({(fx, kind, span, room) for fx, kind, span, room, _ in F.LAYOUTS if span and kind != "control"})


@pytest.mark.parametrize("name,kind,span,room", _GUARDED, ids=[f"{a}-{b}-S{c}-{'reads' if d else 'plain'}" for a, b, c, d in _GUARDED])
def test_identity_rows_lie_in_continuation_windows(rsb, name, kind, span, room):
    """the counting argument of tests/test_kmer_fixtures.py for the rows where walks END: a group of W windows, K of them
    of the kind and V of them holding an identity row, with V + K > W, holds an identity row in a window of the kind --
    so the terminal '$' count is taken on a window with a continuation.  A (fixture, span) without such a group is
    listed in locate_reference.DROPPED and left out of the GPU matrix; nothing else may be listed there."""
    fx = F.fixture(name)
    proven = 0
    for p, (runs, t) in enumerate(zip(fx.runs(), R.truth(fx))):
        st = F.LAYOUT_STATS[(name, p, span, room)]
        groups = F.group_kinds(rsb, runs, span, room, st)
        seen = {}
        for w in {int(r) // span for r in t.identity_rows()}:
            seen[w // F.GROUP] = seen.get(w // F.GROUP, 0) + 1
        proven += sum(1 for g, (W, chunkw, farw) in enumerate(groups) if seen.get(g, 0) + (chunkw if kind.startswith("chunk") else farw) > W)
    assert (proven > 0) == ((name, kind, span, room) not in R.DROPPED), (name, kind, span, room, proven)


def test_gpu_matrix_is_the_layouts_less_the_dropped():
    assert set(R.DROPPED) <= set(_GUARDED)
    kept = R.gpu_layouts()
    assert len(kept) == len(F.LAYOUTS) - sum(1 for fx, kind, span, room, _ in F.LAYOUTS if (fx, kind, span, room) in R.DROPPED)
    # plain and reads layouts, with and without a k-mer table, every fixture
    assert {(fx, room, ktab is None) for fx, _, _, room, ktab in kept} >= {(fx, room, nk) for fx in F.SPANS for room, nk in
                                                                          ((True, False), (True, True), (False, False))}


def test_string_matches_and_expectations():
    t = R.Truth(["ACA", "CA", "ACA"])
    # suffixes: $0 $1 $2 | A$0 A$1 A$2 ACA$0 ACA$2 | CA$0 CA$1 CA$2
    assert t.n == 11 and list(t.offset[:3]) == [3, 2, 3]
    assert [int(x) for x in t.identity_rows()] == [6, 7, 9]          # ACA$ (0), ACA$ (2), CA$ (1)
    assert [int(t.ordinal[r]) for r in (6, 7, 9)] == [0, 1, 2]
    rr, od, of = t.expect([0, 11, 2 ** 64 - 1, 8], max_steps=2)
    assert list(rr) == [R.NONE64, R.NONE64, R.NONE64, 6] and list(of) == [R.NONE32, R.NONE32, R.NONE32, 1] and int(od[3]) == 0
    assert R.string_matches([["ACA", "CA", "ACA"]], "CA") == {(0, 0, 1), (0, 1, 0), (0, 2, 1)}
    assert R.string_matches([["AAA"]], "AA") == {(0, 0, 0), (0, 0, 1)} and R.string_matches([["AAA"]], "") == set()
