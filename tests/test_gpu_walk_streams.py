"""Extension counts and walks on the GPU beyond the gt fixture (-m gpu): rsbwt_set_extensions / rsbwt_extensions /
rsbwt_set_walk (csrc/walk.hip, csrc/set_graph.hip, csrc/capi.hip) held bit-exactly to tests/walk_reference.py's restatement over
the oracle on tests/stream_reference.py's inputs: run streams in the shapes that broke other kernels, the degenerate ones
-- on the '$'-less stream the first step of a search can leave the wrapped interval (0, 2^64 - 1), which counts 0 -- and
the `repeat` and `ragged` read sets, on the builder's own span, with spill chunks and at the widest span, behind a k-mer
table and without one.  A run stream that is no BWT of reads has no string-level truth: there the restatement IS the
definition, and no class of stop is asserted."""
import numpy as np
import pytest

import stream_reference as R
import walk_reference as W

pytestmark = pytest.mark.gpu

SPANS = {"auto": 0, "chunk": 128, "deep": 2944}
GROUPED = ("short", "dollars", "nodollar")  # the streams whose tabled cases take the grouped table format
CTX, MAX_STEPS = 8, 16
DIRECTIONS = [(left, both) for left in (False, True) for both in (False, True)]


def _open(rsb, src, span=0, ktab=6, grouped=False):
    return rsb.GpuBWT(runs=src.runs, num_strings=src.num_strings, ktab_depth=ktab, window_span=span, ktab_grouped=grouped)


def _seeds(src):
    """the small batch, cut to its queries of at least CTX symbols"""
    return [w for w in R.queries(src, "small") if len(w) >= CTX]


def _check(ss, rsb, srcs, sds, where, handles=()):
    side = W.OracleSide([s.orc for s in srcs])
    key = ("streams",) + tuple(s.name for s in srcs) + (tuple(sds),)
    for left, both in DIRECTIONS:
        finals = []
        for m in (1, 2):
            ws = W.walks(side, key, sds, CTX, m, MAX_STEPS, left, both)
            got = ss.walk(sds, CTX, m, MAX_STEPS, left, both, supports=True)
            want = [(w.ext, w.stop, w.last, w.support) for w in ws]
            bad = [q for q in range(len(sds)) if got[q] != want[q]]
            assert not bad, (where, m, left, both, len(bad), bad[:5], got[bad[0]], want[bad[0]])
            wk = rsb.ShardSet.walk_last_work()
            evaluations = sum(len(w.contexts) for w in ws)
            assert wk["seeds"] == len(sds) and wk["appended"] == sum(len(w.ext) for w in ws), (where, wk)
            assert wk["searches"] == evaluations * len(srcs) * 4 * (2 if both else 1), (where, wk, evaluations)
            assert wk["passes"] <= 2 * wk["lf_steps"] + wk["searches"], (where, wk)
            finals += [w.final for w in ws]
        strings = sds + finals
        want = np.array([W.extensions(side, s, CTX, left, both) for s in strings], np.uint64).transpose(1, 0, 2)
        got = ss.extensions(strings, CTX, left, both)
        bad = np.argwhere(got != want)
        assert bad.size == 0, (where, left, both, len(bad), bad[:5], got[tuple(bad[0])], want[tuple(bad[0])])
        for p, g in enumerate(handles):
            assert (g.extensions(strings, CTX, left, both) == want[p]).all(), (where, left, both, p)


@pytest.mark.parametrize("ktab", [6, None])
@pytest.mark.parametrize("kind", list(SPANS))
@pytest.mark.parametrize("name", R.STREAMS + R.FIXTURES)
def test_gpu_walk_on_every_stream_and_layout(rsb, oracle, name, kind, ktab):
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
        _check(ss, rsb, [src], sds, (name, kind, ktab), handles=[g])
    finally:
        ss.close()
        g.close()


# (first shard: span, table), (second shard: span, table); the seeds are the first shard's
PAIRS = [("uniform", 128, 6, "repeat", 0, None), ("ragged", 0, 6, "nodollar", 2944, None), ("stripes", 2944, None, "nodollar", 128, 6),
         ("repeat", 128, None, "dollar-ends", 0, 6)]


@pytest.mark.parametrize("a,span_a,ktab_a,b,span_b,ktab_b", PAIRS, ids=[f"{p[0]}+{p[3]}" for p in PAIRS])
def test_gpu_walk_on_sets_of_two_unlike_shards(rsb, oracle, a, span_a, ktab_a, b, span_b, ktab_b):
    """a run stream beside a read set's shard, different spans, one behind a table and one not: the supports are sums over
    both, each row of the counts is that shard's"""
    srcs = [R.source(a, oracle, rsb), R.source(b, oracle, rsb)]
    gs = [_open(rsb, srcs[0], span_a, ktab_a), _open(rsb, srcs[1], span_b, ktab_b)]
    ss = rsb.ShardSet(gs)
    try:
        _check(ss, rsb, srcs, _seeds(srcs[0]), (a, b), handles=gs)
    finally:
        ss.close()
        for g in gs:
            g.close()
