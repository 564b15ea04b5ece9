"""CPU suite: tests/walk_reference.py's two statements of the extension counts and of rsbwt_set_walk agree -- over the
oracle's BWT and with no BWT at all -- on both read sets, the inputs reach every class of stop, walks long enough to
matter and walks a wrong cross-shard sum would change, and the new entry points are declared, exported, bound and refuse
what the header says they refuse."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import gt_reference as G
import walk_reference as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = {"rsbwt_set_extensions": 7, "rsbwt_extensions": 7, "rsbwt_set_walk": 13, "rsbwt_set_walk_dev": 15, "rsbwt_set_walk_last_work": 1}


@pytest.fixture(scope="module")
def sides(oracle):
    """{set name: (OracleSide, PlainSide)} over the two shards as they are"""
    out = {}
    for name, reads in W.read_sets().items():
        orc = [G.OracleShard(oracle.from_runs(r, len(sh))) for sh, r in zip(reads, W.runs(name, 2))]
        out[name] = (W.OracleSide(orc), W.PlainSide(reads))
    return out


def _walks(sides, name, which, ctx, m, left, both, shards=None):
    side = sides[name][which]
    return W.walks(side, (name, which), W.seeds(ctx), ctx, m, W.MAX_STEPS, left, both, shards)


def _both_directions(sides, name, ctx, m, both, shards=None):
    """the 106 walks of the 53 windows, right then left"""
    return [w for left in (False, True) for w in _walks(sides, name, 0, ctx, m, left, both, shards)[:W.N_PLAIN]]


@pytest.mark.parametrize("both", [False, True])
@pytest.mark.parametrize("left", [False, True])
@pytest.mark.parametrize("ctx", W.CTXS)
@pytest.mark.parametrize("name", ["plain", "stranded"])
def test_the_two_statements_agree(sides, name, ctx, left, both):
    for m in W.MIN_COUNTS:
        a = _walks(sides, name, 0, ctx, m, left, both)
        b = _walks(sides, name, 1, ctx, m, left, both)
        assert a == b, (name, ctx, m, left, both, [i for i, (x, y) in enumerate(zip(a, b)) if x != y][:5])
    # the one-step primitive per shard, on every seed and on every walk's last state
    o, p = sides[name]
    for s in W.seeds(ctx) + [w.final for w in _walks(sides, name, 0, ctx, 1, left, both)]:
        assert W.extensions(o, s, ctx, left, both) == W.extensions(p, s, ctx, left, both), (name, ctx, left, both, s)


def test_the_special_seeds(sides):
    for ctx in W.CTXS:
        for left in (False, True):
            ws = _walks(sides, "plain", 0, ctx, 1, left, False)[W.N_PLAIN:]
            stops = [w.stop for w in ws]
            assert [s == W.INVALID for s in stops] == [True, True, False, True, False], (ctx, left, stops)
            for w in ws:
                if w.stop == W.INVALID:
                    assert w == W.Walk("", W.INVALID, (), (0, 0, 0, 0), w.final, ())
            assert len(ws[4].final) == ctx + len(ws[4].ext)  # the seed of exactly ctx symbols walks


def test_the_inputs_reach_every_class(sides):
    """the figures of a plain count over these reads: at (plain, 12, 1, right, one strand) the 53 windows end 41 BRANCH, 2
    DEAD_END, 10 LIMIT; on `stranded` 34 / 8 / 11 with one strand and 41 / 2 / 10 with both"""
    def ends(name, both):
        ws = _walks(sides, name, 0, 12, 1, False, both)[:W.N_PLAIN]
        return tuple(sum(w.stop == s for w in ws) for s in (W.BRANCH, W.DEAD_END, W.LIMIT))
    assert ends("plain", False) == (41, 2, 10)
    assert ends("stranded", False) == (34, 8, 11)
    assert ends("stranded", True) == (41, 2, 10)
    for name in ("plain", "stranded"):
        for m in (1, 2):
            for left in (False, True):
                ws = _walks(sides, name, 0, 12, m, left, False)[:W.N_PLAIN]
                for s in (W.BRANCH, W.DEAD_END, W.LIMIT):
                    assert sum(w.stop == s for w in ws) >= 2, (name, m, left, s)
            for ctx in W.CTXS:
                all106 = _both_directions(sides, name, ctx, m, False)
                assert len(all106) == 106
                assert sum(len(w.ext) >= 16 for w in all106) >= 30, (name, ctx, m)
                # counting shard 0 alone changes many walks: a wrong cross-shard sum cannot pass
                alone = _both_directions(sides, name, ctx, m, False, shards=[0])
                assert sum(x[:4] != y[:4] for x, y in zip(all106, alone)) >= 20, (name, ctx, m)
    # LIMIT is reached inside the tandem repeat: at min_count 1 the haplotypes' substitutions branch every walk there at
    # once; at 2, on one strand of `stranded`, the repeat unit goes round until max_steps
    ws = _walks(sides, *W.IN_REPEAT[:1], 0, *W.IN_REPEAT[1:])[:W.N_PLAIN]
    inside = W.seeds_inside_the_repeat()
    assert len(inside) >= 10 and sum(ws[i].stop == W.LIMIT and len(ws[i].ext) == W.MAX_STEPS for i in inside) >= 2


def test_the_strands_matter_on_the_stranded_set(sides):
    for ctx in W.CTXS:
        one = _both_directions(sides, "stranded", ctx, 1, False)
        two = _both_directions(sides, "stranded", ctx, 1, True)
        assert sum(x[:4] != y[:4] for x, y in zip(one, two)) > 0, ctx
        # a reverse-complemented read supports the same sequence once both strands count
        assert [w[:2] for w in two] == [w[:2] for w in _both_directions(sides, "plain", ctx, 1, True)]


def test_the_walks_do_not_depend_on_the_dealing():
    """the support is a sum over the shards: the same reads dealt to 1, 2, 3, 5 and 9 shards walk alike"""
    for name in ("plain", "stranded"):
        want = None
        for S in W.DEALS:
            reads = W.dealt(name, S)
            assert len(reads) == S and sorted(r for sh in reads for r in sh) == sorted(r for sh in W.read_sets()[name] for r in sh)
            side = W.PlainSide(reads)
            got = [W.walks(side, (name, "dealt", S), W.seeds(12), 12, 2, W.MAX_STEPS, left, name == "stranded") for left in (False, True)]
            want = want or got
            assert got == want, (name, S)
        assert W.dealt(name, 2) == W.read_sets()[name]


def test_expected_work_counts_what_the_definition_says(sides):
    side = sides["plain"][0]
    ws = _walks(sides, "plain", 0, 12, 1, False, False)
    searches, steps = W.expected_work(side, ws, False, False)
    evaluations = sum(len(w.contexts) for w in ws)
    assert searches == evaluations * 2 * 4 and evaluations == sum(len(w.ext) + (w.stop in (W.BRANCH, W.DEAD_END)) for w in ws)
    assert searches * 1 <= steps <= searches * 12  # a candidate of 13 symbols: 12 steps at the most; all four bases occur
    x = ws[0].contexts[0] + ws[0].ext[0]
    assert W.search_steps(side, 0, x) == 12 or side.W(0, x) == 0


def test_entry_points_are_declared_exported_and_bound_and_refuse_bad_arguments(rsb):
    from readserver_amd import _native
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rsbwt.h")).read(), flags=re.S)
    L = C.CDLL(rsb.lib_path())
    for n, nargs in ENTRY.items():
        assert re.search(r"\b%s\s*\(" % n, txt), f"{n} is not declared in include/rsbwt.h"
        assert n in _native.SIGNATURES and hasattr(L, n) and hasattr(rsb.lib(), n)
        assert len(_native.SIGNATURES[n][1]) == nargs, n
    for name, value in (("RSBWT_WALK_LEFT", "1u"), ("RSBWT_WALK_BOTH_STRANDS", "2u"), ("RSBWT_WALK_DEAD_END", "1"), ("RSBWT_WALK_BRANCH", "2"),
                        ("RSBWT_WALK_LIMIT", "3"), ("RSBWT_WALK_INVALID", "4")):
        assert re.search(r"#define %s %s\b" % (name, value), txt), name
    assert (rsb.bwt.WALK_DEAD_END, rsb.bwt.WALK_BRANCH, rsb.bwt.WALK_LIMIT, rsb.bwt.WALK_INVALID) == (W.DEAD_END, W.BRANCH, W.LIMIT, W.INVALID)
    assert callable(rsb.GpuBWT.extensions) and callable(rsb.ShardSet.extensions) and callable(rsb.ShardSet.walk)
    assert callable(rsb.ShardSet.walk_last_work)
    L = rsb.lib()
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    text = np.frombuffer(b"ACGTACGT", np.uint8).copy()
    off = np.array([0, 4, 8], np.uint64)
    cnt = np.full(8, 77, np.uint64)
    ext, steps, stop = np.full(8, 77, np.uint8), np.full(2, 77, np.uint32), np.full(2, 77, np.uint8)
    none = L.rsbwt_device_count() == 0
    # a box without a GPU can have no set: RSBWT_ENODEV, no CPU fallback; where there is one a null set is RSBWT_EINVAL
    want = -5 if none else -1
    assert L.rsbwt_set_extensions(None, p(text), p(off), 2, 4, 0, p(cnt)) == want
    assert (b"no CPU fallback" if none else b"null") in L.rsbwt_last_error()
    assert L.rsbwt_extensions(None, p(text), p(off), 2, 4, 0, p(cnt)) == want
    assert L.rsbwt_set_walk(None, p(text), p(off), 2, 4, 1, 4, 0, p(ext), p(steps), p(stop), None, None) == want
    assert L.rsbwt_set_walk(None, None, None, 0, 4, 1, 4, 0, None, None, None, None, None) == want
    assert L.rsbwt_set_walk_dev(None, None, None, 0, 0, 4, 1, 4, 0, None, None, None, None, None, None) == -1
    assert (cnt == 77).all() and (ext == 77).all() and (steps == 77).all() and (stop == 77).all()
    w = (C.c_uint64 * 6)(*([9] * 6))
    L.rsbwt_set_walk_last_work(None)  # (nothing to write to: no crash)
    L.rsbwt_set_walk_last_work(w)
    assert list(w) == [0] * 6  # the failed calls above did no work
    if none:
        runs = np.array([(0 << 5) | 1, (1 << 5) | 3], np.uint8)
        with pytest.raises(rsb.RsbwtError) as e:
            with rsb.GpuBWT(runs=runs, num_strings=1) as g:
                g.extensions(["ACGT"], 2)
        assert e.value.code == -5 and "no CPU fallback" in str(e.value)
