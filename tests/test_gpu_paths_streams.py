"""Paths on the GPU beyond the gt fixture (-m gpu): rsbwt_set_paths (csrc/paths.hip's paths_kernel, csrc/set_graph.hip) held
bit-exactly to tests/paths_reference.py's statement over the oracle on tests/stream_reference.py's inputs: run streams in
the shapes that broke other kernels, the degenerate ones -- on the '$'-less stream a step of a search can leave the
wrapped interval (0, 2^64 - 1), which counts 0 -- and the `repeat` and `ragged` read sets, on the builder's own span,
with spill chunks and at the widest span, behind a k-mer table and without one.  It is the one call whose loop goes on
where a walk would have stopped.  A run stream has no haplotype to take targets from: they come from the reference's own
paths (tests/graph_context_reference.py), and tests/test_graph_context_reference.py shows on the CPU that every seed
state and every stop, TARGET included, occur.  A run stream that is no BWT of reads has no string-level truth: there the
statement IS the definition, and no class of stop is asserted."""
import pytest

import graph_context_reference as X
import paths_reference as P
import stream_reference as R

pytestmark = pytest.mark.gpu

SPANS = {"auto": 0, "chunk": 128, "deep": 2944}
GROUPED = ("short", "dollars", "nodollar")  # the streams whose tabled cases take the grouped table format
CTX = X.CTX


def _open(rsb, src, span=0, ktab=6, grouped=False):
    return rsb.GpuBWT(runs=src.runs, num_strings=src.num_strings, ktab_depth=ktab, window_span=span, ktab_grouped=grouped)


def _check(ss, rsb, srcs, sds, where):
    for both, m, left in X.STREAM_SETTINGS:
        tgs = X.stream_targets(srcs, sds, left)
        for limits, t in ((X.STREAM_WIDE, None), (X.STREAM_TIGHT, None), (X.STREAM_WIDE, tgs)):
            ref = X.stream_searches(srcs, sds, t, m, limits, left, both)
            got = ss.paths(sds, CTX, m, limits[0], limits[1], limits[2], left, both, t)
            want = [(s.state, list(s.paths)) for s in ref]
            bad = [q for q in range(len(sds)) if got[q] != want[q]]
            assert not bad, (where, both, m, left, limits, t is not None, len(bad), bad[:5], got[bad[0]], want[bad[0]])
            wk = rsb.ShardSet.paths_last_work()
            evals = sum(len(s.evaluated) for s in ref)
            appended = sum(len(s.evaluated) - sum(p[1] == P.DEAD_END for p in s.paths) + len(s.backtracks) for s in ref)
            assert wk["seeds"] == len(sds) and wk["appended"] == appended, (where, wk, appended)
            assert wk["evals"] == evals and wk["paths"] == sum(len(s.paths) for s in ref), (where, wk, evals)
            assert wk["searches"] == evals * len(srcs) * 4 * (2 if both else 1), (where, wk, evals)
            assert wk["passes"] <= 2 * wk["lf_steps"] + wk["searches"], (where, wk)


@pytest.mark.parametrize("ktab", [6, None])
@pytest.mark.parametrize("kind", list(SPANS))
@pytest.mark.parametrize("name", R.STREAMS + R.FIXTURES)
def test_gpu_paths_on_every_stream_and_layout(rsb, oracle, name, kind, ktab):
    src = R.source(name, oracle, rsb)
    sds = X.stream_seeds(src)
    assert len(sds) >= 9
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
def test_gpu_paths_on_sets_of_two_unlike_shards(rsb, oracle, a, span_a, ktab_a, b, span_b, ktab_b):
    """a run stream beside a read set's shard, different spans, one behind a table and one not: the supports are sums over
    both, and so are the forks a path goes through"""
    srcs = [R.source(a, oracle, rsb), R.source(b, oracle, rsb)]
    gs = [_open(rsb, srcs[0], span_a, ktab_a), _open(rsb, srcs[1], span_b, ktab_b)]
    ss = rsb.ShardSet(gs)
    try:
        _check(ss, rsb, srcs, X.stream_seeds(srcs[0]), (a, b))
    finally:
        ss.close()
        for g in gs:
            g.close()
