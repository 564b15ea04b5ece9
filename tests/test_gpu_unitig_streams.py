"""Unitigs on the GPU beyond the gt fixture (-m gpu): rsbwt_set_unitigs (csrc/walk.hip's unitig_kernel, csrc/set_graph.hip) held
bit-exactly to tests/unitig_reference.py's statement over the oracle on tests/stream_reference.py's inputs: run streams in
the shapes that broke other kernels, the degenerate ones -- on the '$'-less stream the first step of a search can leave
the wrapped interval (0, 2^64 - 1), which counts 0 -- and the `repeat` and `ragged` read sets, on the builder's own span,
with spill chunks and at the widest span, behind a k-mer table and without one.  A run stream that is no BWT of reads has
no string-level truth: there the statement IS the definition, and no class of stop is asserted."""
import pytest

import stream_reference as R
import unitig_reference as U
import walk_reference as W

pytestmark = pytest.mark.gpu

SPANS = {"auto": 0, "chunk": 128, "deep": 2944}
GROUPED = ("short", "dollars", "nodollar")  # the streams whose tabled cases take the grouped table format
CTX, MAX_STEPS = 8, 16


def _open(rsb, src, span=0, ktab=6, grouped=False):
    return rsb.GpuBWT(runs=src.runs, num_strings=src.num_strings, ktab_depth=ktab, window_span=span, ktab_grouped=grouped)


def _seeds(src):
    """the small batch, cut to its queries of at least CTX symbols"""
    return [w for w in R.queries(src, "small") if len(w) >= CTX]


def _check(ss, rsb, srcs, sds, where):
    side = W.OracleSide([s.orc for s in srcs])
    key = ("streams",) + tuple(s.name for s in srcs) + (tuple(sds),)
    for both in (False, True):
        for m in (1, 2):
            us = U.unitigs(side, key, sds, CTX, m, MAX_STEPS, both)
            got = ss.unitigs(sds, CTX, m, MAX_STEPS, both, supports=True)
            want = [tuple((s.ext, s.stop, s.last, s.support) for s in pair) for pair in us]
            bad = [q for q in range(len(sds)) if got[q] != want[q]]
            assert not bad, (where, m, both, len(bad), bad[:5], got[bad[0]], want[bad[0]])
            wk = rsb.ShardSet.unitigs_last_work()
            onward = sum(len(s.onward) for pair in us for s in pair)
            back = sum(len(s.back) for pair in us for s in pair)
            assert wk["seeds"] == len(sds) and wk["appended"] == sum(len(s.ext) for pair in us for s in pair), (where, wk)
            assert wk["onward"] == onward and wk["back"] == back, (where, wk, onward, back)
            assert wk["searches"] == (onward + back) * len(srcs) * 4 * (2 if both else 1), (where, wk)
            assert wk["passes"] <= 2 * wk["lf_steps"] + wk["searches"], (where, wk)


@pytest.mark.parametrize("ktab", [6, None])
@pytest.mark.parametrize("kind", list(SPANS))
@pytest.mark.parametrize("name", R.STREAMS + R.FIXTURES)
def test_gpu_unitigs_on_every_stream_and_layout(rsb, oracle, name, kind, ktab):
    src = R.source(name, oracle, rsb)
    sds = _seeds(src)
    assert len(sds) >= 9 or name == "single"
    grouped = ktab is not None and name in GROUPED
    g = _open(rsb, src, SPANS[kind], ktab, grouped)
    ss = rsb.ShardSet([g])
    try:
        if SPANS[kind]:
            assert g.window_span() == SPANS[kind]
        if ktab is not None:
            assert g.ktab_info()[0] == (1 if grouped else 0)
        _check(ss, rsb, [src], sds, (name, kind, ktab))
    finally:
        ss.close()
        g.close()


# (first shard: span, table), (second shard: span, table); the seeds are the first shard's
PAIRS = [("uniform", 128, 6, "repeat", 0, None), ("ragged", 0, 6, "nodollar", 2944, None), ("stripes", 2944, None, "nodollar", 128, 6),
         ("repeat", 128, None, "dollar-ends", 0, 6)]


@pytest.mark.parametrize("a,span_a,ktab_a,b,span_b,ktab_b", PAIRS, ids=[f"{p[0]}+{p[3]}" for p in PAIRS])
def test_gpu_unitigs_on_sets_of_two_unlike_shards(rsb, oracle, a, span_a, ktab_a, b, span_b, ktab_b):
    """a run stream beside a read set's shard, different spans, one behind a table and one not: the supports are sums over
    both"""
    srcs = [R.source(a, oracle, rsb), R.source(b, oracle, rsb)]
    gs = [_open(rsb, srcs[0], span_a, ktab_a), _open(rsb, srcs[1], span_b, ktab_b)]
    ss = rsb.ShardSet(gs)
    try:
        _check(ss, rsb, srcs, _seeds(srcs[0]), (a, b))
    finally:
        ss.close()
        for g in gs:
            g.close()
