"""CPU guards for the stream tests (tests/test_gpu_match_streams.py, tests/test_gpu_overlap_streams.py): what
tests/stream_reference.py's streams, read sets and query batches reach, shown with the reference alone -- before anything
runs on a GPU.  On the read sets the restatement over the oracle is held to the computation without a BWT; a run stream
that is no BWT has no string-level truth, and there the restatement is the definition."""
import random

import numpy as np
import pytest

import match_reference as M
import overlap_reference as O
import stream_reference as R
import test_kmer_fixtures as F

T = 6  # the table depth the GPU cases use
U64 = 2 ** 64 - 1


def _src(name, oracle, rsb):
    return R.source(name, oracle, rsb)


def test_the_streams_have_the_shapes_they_are_named_for(oracle, rsb):
    for name in R.STREAMS:
        runs = R.make_runs(name, rsb)
        assert (runs == R.make_runs(name, rsb)).all()  # seeded
        sym, ln = runs >> 5, runs & 31
        assert sym.max() <= 4 and ln.min() >= 1, name  # (the builder refuses a symbol above 4 and a run of no symbols)
        n = int(ln.astype(np.int64).sum())
        assert n <= 100000, (name, n)
        if name in R.SHAPED:
            assert runs.size == R.SIZES.get(name, R.RUN_BYTES)
        print(name, "run bytes", runs.size, "symbols", n, "'$' runs", int((sym == 0).sum()))
    sym = lambda name: R.make_runs(name, rsb) >> 5  # noqa: E731
    ln = lambda name: R.make_runs(name, rsb) & 31  # noqa: E731
    assert (ln("all31") == 31).all() and ln("short").max() == 2 and set(ln("uniform")) == set(range(1, 32))
    # runs of 31 with continuation bytes: a symbol's run goes on in the next byte
    assert (np.diff(sym("all31").astype(int)) == 0).sum() > 300
    d = sym("dollars") == 0
    assert 0.27 < d.mean() < 0.33 and d[:2250].mean() > 0.7 and d[2250:].mean() < 0.05
    assert (d[1:] & d[:-1]).sum() > 1000  # '$' runs side by side: stripes of '$' longer than any run byte
    st = sym("stripes")
    assert (st == 1 + (np.arange(st.size) // 5000) % 4).mean() > 0.99 and {1, 2} <= set(st)
    assert R.make_runs("single", rsb).size == 1
    nd = sym("nodollar")
    assert (nd != 0).all() and set(nd) == {1, 2, 3, 4} and (nd[:R.LEAD] == 4).all()
    de = sym("dollar-ends")
    assert de[0] == 0 and de[-1] == 0 and set(de) == {0, 1, 2, 3, 4}
    for name in R.SYNTH_STYLES:
        assert len(set(sym(name))) >= 4, name


@pytest.mark.parametrize("name", R.STREAMS + R.FIXTURES)
def test_the_batches_have_the_sizes_and_the_edges(oracle, rsb, name):
    src = _src(name, oracle, rsb)
    small, wide = R.queries(src, "small"), R.queries(src, "wide")
    assert R.queries(src, "wide") is wide
    assert 30 <= len(small) <= 60, len(small)
    assert len(wide) >= 600 and sum(len(w) for w in wide) >= 20000, (len(wide), sum(len(w) for w in wide))
    print(name, "small", len(small), sum(len(w) for w in small), "wide", len(wide), sum(len(w) for w in wide),
          "workgroups of 256 lanes", -(-len(wide) // 256))
    assert len(wide) > 3 * 256 - 64  # three workgroups of overlap lanes per shard, the third nearly full
    for qs in (small, wide):
        assert max(len(w) for w in qs) <= (R.MAX_QUERY if src.reads is not None else 70)
        assert qs[:3] == [""] * 3 and qs[-4:] == [""] * 4
        mid = [i for i in range(4, len(qs) - 5) if qs[i:i + 3] == [""] * 3]
        assert mid, "no run of three empty queries inside the batch"
        assert {"", "A", "N"} <= set(qs) and any("N" in w[1:-1] and set(w) - {"N"} for w in qs)
    if src.reads is None:
        # the spelled queries stay alive: their whole backward search is proper
        sp = R.spelled(src, "wide")
        assert len(sp) >= R.BATCHES["wide"] // 2 and all(w in wide and M.width(src.orc.find(w), src.n) > 0 for w in sp)
        print(name, "spelled lengths", min(len(w) for w in sp), "..", max(len(w) for w in sp))
    else:
        reads = set(src.reads)
        assert sum(w in reads for w in wide) >= 200 and sum(any(w[i:] in reads for i in range(1, 21)) for w in wide if w) >= 200


@pytest.mark.parametrize("name", R.STREAMS + R.FIXTURES)
def test_match_lengths_reach_every_class(oracle, rsb, name):
    """the wide batch: matches deeper than the table, positions of length 0, matches that reach the query's start, matches
    the cap of 16 stops"""
    src = _src(name, oracle, rsb)
    qs = R.queries(src, "wide")
    ln, lo, up, (recs, first), _ = R.match_expected([src], "wide", qs, 0, 1)
    ends = np.concatenate([np.arange(1, len(w) + 1) for w in qs if w])
    N = ln.shape[1]
    assert N == ends.size
    cls = {"positions": N, f"l>{T}": int((ln[0] > T).sum()), "l==0": int((ln[0] == 0).sum()), "whole": int((ln[0] == ends).sum()),
           "lower==0": int(((ln[0] > 0) & (lo[0] == 0)).sum()), "upper==n-1": int(((ln[0] > 0) & (up[0] == src.n - 1)).sum()),
           "smems": len(recs)}
    ln16 = R.match_expected([src], "wide", qs, 16, 1)[0]
    cls["capped"] = int(((ln16[0] == 16) & (ends > 16)).sum())
    assert ln16.max() <= 16
    for mr in (3, 20):
        cls[f"shorter at min_rows={mr}"] = int((R.match_expected([src], "wide", qs, 0, mr)[0] < ln).sum())
    print(name, cls)
    assert cls["whole"] > 0 and cls["capped"] > 0 and 0 < len(recs) < N, cls
    if name in R.SHAPED:
        assert 4 * cls[f"l>{T}"] >= N and 20 * cls["l==0"] >= N, cls
    if name not in R.DEGENERATE + ("all31",):  # (runs of 31 on multiples of 31: every interval is a whole number of them)
        assert cls["shorter at min_rows=20"] > 0, cls
    if name in ("single", "nodollar"):
        assert cls["lower==0"] > 0, cls  # (only where no '$' row lies before the rows that begin with A)


def test_the_stream_without_terminators_gives_improper_intervals(oracle, rsb):
    """initInterval and LF steps of a string that is not there leave the reference's (0, 2^64 - 1): no row by the C-ABI's
    rule, whatever upper - lower + 1 says"""
    src = _src("nodollar", oracle, rsb)
    wrapped = set()
    for batch in ("small", "wide"):
        for w in R.queries(src, batch):
            for e in range(1, len(w) + 1):
                l = M.longest(src.orc, src.n, w, e, 0, 1)[0]
                if l < e and w[e - l - 1] in "ACGT":
                    iv = src.orc.find(w[e - l - 1:e])
                    if iv[1] == U64:
                        wrapped.add(iv)
    print(sorted(wrapped)[:5], len(wrapped))
    assert (0, U64) in wrapped
    assert all(M.width(iv, src.n) == 0 for iv in wrapped)
    single = _src("single", oracle, rsb)
    assert single.orc.find("A") == (0, U64) and single.orc.find("CC") == (0, 16) and M.width((0, U64), 17) == 0


@pytest.mark.parametrize("name", ["dollars", "repeat", "ragged"])
def test_overlaps_are_there_at_every_parameter_pair(oracle, rsb, name):
    src = _src(name, oracle, rsb)
    qs = R.queries(src, "wide")
    found = {}
    for mo, xo in O.PARAMS:
        cnt = R.overlap_expected([src], "wide", qs, mo, xo)[0]
        found[(mo, xo)] = (int((cnt > 0).sum()), int((cnt > 1).sum()))
    print(name, "entries (count > 0, count > 1)", [found[pr] for pr in O.PARAMS])
    assert all(a >= 50 for a, _ in found.values()), sorted(found.values())


@pytest.mark.parametrize("name", R.SHAPED)
def test_overlaps_on_every_stream_with_terminators(oracle, rsb, name):
    """(figures; what is asserted: some suffix opens a "read" on every stream that has '$')"""
    src = _src(name, oracle, rsb)
    for batch in ("small", "wide"):
        qs = R.queries(src, batch)
        cnt = R.overlap_expected([src], batch, qs, 1, 0)[0]
        print(name, batch, "entries", int((cnt > 0).sum()), "of", cnt.size, "largest count", int(cnt.max()))
        assert (cnt > 0).any()


def test_repeat_has_entries_of_duplicate_reads(oracle, rsb):
    """a suffix that is a whole read which the shard holds twice: count >= 2 with every one of the reads the same string"""
    src = _src("repeat", oracle, rsb)
    qs = R.queries(src, "wide")
    exp = R.overlap_expected([src], "wide", qs, 1, 0)[3]
    dup = 0
    for q, per in enumerate(exp[0]):
        for t, (o, cnt, _, _) in enumerate(per):
            if cnt >= 2 and {src.plain.read(x) for x in range(o, o + cnt)} == {qs[q][t:]}:
                dup += 1
    print("entries of duplicate reads", dup)
    assert dup > 0


@pytest.mark.parametrize("name", R.FIXTURES)
def test_a_read_is_reachable_at_two_overlap_lengths_and_the_cap_cuts_some(oracle, rsb, name):
    """what reads_of's "once, at its longest" rule cuts; and MAX_READS cuts some (query, shard) pairs and leaves others"""
    src = _src(name, oracle, rsb)
    qs = R.queries(src, "small")
    cap = R.MAX_READS[name]
    for mo, xo in R.READ_PARAMS:
        exp = R.overlap_expected([src], "small", qs, mo, xo)[3]
        twice = 0
        for q in range(len(qs)):
            seen = {}
            for t, (o, cnt, _, _) in enumerate(exp[0][q]):
                for x in range(o, o + cnt):
                    seen[x] = seen.get(x, 0) + 1
            twice += any(v > 1 for v in seen.values())
        first, out, matches = O.reads_of(exp, qs, [src.plain])
        first2, out2, matches2 = O.reads_of(exp, qs, [src.plain], cap)
        print(name, (mo, xo), "pairs with a read met twice", twice, "reads", len(out), "under the cap", len(out2))
        assert matches2 == matches and len(out2) < len(out) and all(len(r) <= R.READ_STRIDE[name] for _, _, r in out)
        if mo == 1:
            assert twice > 0 and len(out) < sum(e[1] for per in exp[0] for e in per)
        else:
            assert 0 < len(out2) and any(m > cap for m in matches) and any(0 < m <= cap for m in matches)


@pytest.mark.parametrize("name", R.FIXTURES)
def test_restatement_agrees_with_the_computation_without_a_bwt(oracle, rsb, name):
    """a seeded sample of the wide batch's items: len, lower and upper of every parameter pair against ScanCounts, count and
    ordinal against PlainSide"""
    src = _src(name, oracle, rsb)
    qs = R.queries(src, "wide")
    plain = R.ScanCounts(src.reads)
    assert plain.n == src.n
    rng = random.Random(name)
    items = [(q, e) for q, w in enumerate(qs) for e in range(1, len(w) + 1)]
    sample = rng.sample(items, 300)
    for max_len, min_rows in M.PARAMS:
        exp = R.match_expected([src], "wide", qs, max_len, min_rows)[4]
        for q, e in sample:
            assert exp[0][q][e - 1] == plain.longest(qs[q], e, max_len, min_rows), (q, e, max_len, min_rows)
    sample = rng.sample(items, 400)
    for mo, xo in O.PARAMS:
        exp = R.overlap_expected([src], "wide", qs, mo, xo)[3]
        for q, e in sample:
            w, t = qs[q], e - 1
            x = w[t:]
            want = src.plain.entry(x) if O.wanted(len(x), x, mo, xo) else O.PlainSide.ZERO
            assert exp[0][q][t][:2] == (want if want[1] else O.PlainSide.ZERO), (q, t, mo, xo)
    assert len(M.PARAMS) * 300 + len(O.PARAMS) * 400 <= 4000


def test_the_layouts_spill_and_have_far_lines(rsb):
    """the builder's own statistics on the host: the streams with the most run bytes per window spill at span 128 and have
    far lines from span 300 on, so a GPU case at those spans cannot be a run over plain lines only"""
    for name in R.SPILLING:
        runs = R.make_runs(name, rsb)
        st = {span: F.selftest(rsb, runs, span, True) for span in (40, 128, 300, 600, 2944)}
        print(name, st)
        assert st[128][5] > 0, (name, st[128])
        assert all(st[s][2] > 0 for s in (300, 600, 2944)), (name, st)
    for name in R.FAR_AT_DEEP:
        st = F.selftest(rsb, R.make_runs(name, rsb), 2944, True)
        print(name, st)
        assert st[2] > st[4] > 0, (name, st)
