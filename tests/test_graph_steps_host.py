"""CPU suite: the step loops a set over several device groups runs on the host (readserver_amd/csrc/graph_steps.h) as a
program of their own under the address and undefined-behaviour sanitizers (tests/native/graph_steps_host.cpp), held to
walk_reference, unitig_reference and paths_reference over PlainSide on the same reads.  The program's evaluator counts the
candidates in the reads, one hash map per shard; its output arrays have exactly their stated sizes."""
import os
import shutil
import subprocess
from collections import Counter

import pytest

import graph_context_reference as X
import paths_reference as P
import unitig_reference as U
import walk_reference as W
from kmer_reference import _rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHARDS = 3
WIDE_STOP = 8  # RSBWT_WALK_WIDE
SETTINGS = [(ctx, m, left, both) for ctx in W.CTXS for m in (1, 2) for left in (False, True) for both in (False, True)]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """run(op, name, seeds, *numbers, targets=None) -> the program's lines without the last two, and its work counters"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    tmp = tmp_path_factory.mktemp("graph_steps")
    exe = str(tmp / "graph_steps_host")
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(ROOT, "tests", "native", "graph_steps_host.cpp"), "-o", exe], capture_output=True, text=True)
    if b.returncode != 0 and "sanitize" in b.stderr:
        pytest.skip("no sanitizer runtime here")
    assert b.returncode == 0, b.stderr
    files = {}

    def listed(key, strings):
        if key not in files:
            files[key] = str(tmp / ("%d.txt" % len(files)))
            with open(files[key], "w") as f:
                f.write("%d\n" % len(strings) + "".join(s + "\n" for s in strings))
        return files[key]

    def reads(name):
        if name not in files:
            files[name] = str(tmp / (name + ".reads"))
            with open(files[name], "w") as f:
                f.write("%d\n" % SHARDS + "".join("%d\n" % len(sh) + "".join(r + "\n" for r in sh) for sh in W.dealt(name, SHARDS)))
        return files[name]

    def run(op, name, seeds, *numbers, targets=None):
        args = [exe, op, reads(name), listed(tuple(seeds), seeds)]
        if op == "paths":
            args.append("-" if targets is None else listed(("targets",) + tuple(targets), targets))
        r = subprocess.run(args + [str(int(n)) for n in numbers], capture_output=True, text=True, timeout=120)
        lines = r.stdout.splitlines()
        assert r.returncode == 0 and lines[-1:] == ["graph_steps ok"], (args, numbers, r.stdout[-1000:], r.stderr[-3000:])
        return lines[:-2], [int(w) for w in lines[-2].split()[1:]]
    return run


@pytest.fixture(scope="module")
def sides():
    return {name: W.PlainSide(W.dealt(name, SHARDS)) for name in ("plain", "stranded")}


def _line(ext, stop, support, last):
    """a walk or a unitig side as the program prints it; support / last None: passed as null"""
    nums = lambda v: "-" if v is None or not len(v) else ",".join(str(x) for x in v)  # noqa: E731
    return "%s %d %d %s %s" % (ext or "-", len(ext), stop, nums(support), nums(last))


def _wide_at(side, w, left, both, cap):
    """the rule of the program's row cap: the first evaluation of a walk with a candidate, of either strand on its own, that
    occurs more often than cap ends it there with WIDE, and `last` stays zero"""
    for k, c in enumerate(w.contexts):
        if any(sum(side.W(p, y) for p in range(side.S)) > cap for x in W.candidates(c, left) for y in ((x, _rc(x)) if both else (x,))):
            return w.ext[:k], WIDE_STOP, w.support[:k], (0, 0, 0, 0)
    return w.ext, w.stop, w.support, w.last


@pytest.mark.parametrize("name", ["plain", "stranded"])
def test_walk_loop(host, sides, name):
    stops = Counter()
    for ctx, m, left, both in SETTINGS:
        ws = W.walks(sides[name], (name, "dealt", SHARDS), W.seeds(ctx), ctx, m, W.MAX_STEPS, left, both)
        got, work = host("walk", name, W.seeds(ctx), ctx, m, W.MAX_STEPS, left, both, 1, 0)
        assert got == [_line(w.ext, w.stop, w.support, w.last) for w in ws], (ctx, m, left, both)
        assert work[0] == sum(len(w.ext) for w in ws)
        stops.update(w.stop for w in ws)
        # the short seed, the one with an N in its context, the empty one; the one with an N elsewhere and the one of ctx symbols walk
        assert [w.stop == W.INVALID for w in ws[W.N_PLAIN:]] == [True, True, False, True, False]
    assert all(stops[s] >= 10 for s in (W.DEAD_END, W.BRANCH, W.INVALID)), stops


def test_walk_loop_at_the_limit_without_the_optional_outputs_and_at_a_row_cap(host, sides):
    name, ctx, m, left, both = W.IN_REPEAT
    side, sds = sides[name], W.seeds(ctx)
    ws = W.walks(side, (name, "dealt", SHARDS), sds, ctx, m, W.MAX_STEPS, left, both)
    assert sum(ws[i].stop == W.LIMIT for i in W.seeds_inside_the_repeat()) >= 2
    assert host("walk", name, sds, ctx, m, W.MAX_STEPS, left, both, 1, 0)[0] == [_line(w.ext, w.stop, w.support, w.last) for w in ws]
    # support and last null: ext, steps and stop as with them
    assert host("walk", name, sds, ctx, m, W.MAX_STEPS, left, both, 0, 0)[0] == [_line(w.ext, w.stop, None, None) for w in ws]
    # a row cap: WIDE at the first step, WIDE after symbols were appended, and walks the cap leaves alone
    ctx, m, left, both, cap = 12, 1, False, True, 8
    ws = W.walks(side, (name, "dealt", SHARDS), W.seeds(ctx), ctx, m, W.MAX_STEPS, left, both)
    want = [_wide_at(side, w, left, both, cap) for w in ws]
    got, work = host("walk", name, W.seeds(ctx), ctx, m, W.MAX_STEPS, left, both, 1, cap)
    assert got == [_line(*w) for w in want]
    assert work[0] == sum(len(w[0]) for w in want)
    wide = [w for w in want if w[1] == WIDE_STOP]
    assert sum(not w[0] for w in wide) >= 2 and sum(bool(w[0]) for w in wide) >= 2 and sum(w[1] in (W.DEAD_END, W.BRANCH) for w in want) >= 2, Counter(w[1] for w in want)


@pytest.mark.parametrize("name", ["plain", "stranded"])
def test_unitig_loop(host, sides, name):
    stops = Counter()
    cases = [(ctx, m, W.MAX_STEPS, both, 1) for ctx in W.CTXS for m in (1, 2) for both in (False, True)]
    cases += [(20, 2, 6, False, 1), (12, 1, W.MAX_STEPS, True, 0)]  # a max_steps that is reached; support and last null
    for ctx, m, max_steps, both, optional in cases:
        us = U.unitigs(sides[name], (name, "dealt", SHARDS), U.seeds(ctx), ctx, m, max_steps, both)
        got, work = host("unitigs", name, U.seeds(ctx), ctx, m, max_steps, both, optional)
        assert got == [_line(s.ext, s.stop, s.support if optional else None, s.last if optional else None) for pair in us for s in pair], (ctx, m, max_steps, both)
        assert work == [sum(len(getattr(s, what)) for pair in us for s in pair) for what in ("ext", "onward", "back")]
        stops.update((s.stop, max_steps) for pair in us for s in pair)
    assert all(stops[(s, W.MAX_STEPS)] >= 4 for s in (U.DEAD_END, U.BRANCH, U.JOIN, U.INVALID)) and stops[(U.LIMIT, 6)] >= 4, stops


def _paths_lines(ss, optional=True):
    out = []
    for s in ss:
        out.append("%d %d" % (s.state, len(s.paths)))
        out += ["%s %d %d %s" % (e or "-", len(e), why, least if optional else "-") for e, why, least in s.paths]
    return out


@pytest.mark.parametrize("name", ["plain", "stranded"])
def test_paths_loop(host, sides, name):
    states, stops = Counter(), Counter()
    for ctx, m, left, both in SETTINGS:
        for limits, targets in ((P.WIDE, True), (P.WIDE, False), (P.TIGHT, True)):
            tgs = P.targets(ctx, left) if targets else None
            ss = P.searches(sides[name], (name, "dealt", SHARDS, targets), W.seeds(ctx), tgs, ctx, m, limits, left, both)
            got, work = host("paths", name, W.seeds(ctx), ctx, m, *limits, left, both, 1, targets=tgs)
            assert got == _paths_lines(ss), (ctx, m, left, both, limits, targets)
            # (every evaluation but those that found nothing live appended a symbol, and so did every backtrack)
            appended = sum(len(s.evaluated) - sum(p[1] == P.DEAD_END for p in s.paths) + len(s.backtracks) for s in ss)
            assert work == [appended, sum(len(s.evaluated) for s in ss), sum(len(s.paths) for s in ss)]
            states.update(s.state for s in ss)
            stops.update(p[1] for s in ss for p in s.paths)
    # max_paths, max_evals and max_steps each end searches, and so do targets and dead ends
    assert all(states[s] >= 4 for s in (P.COMPLETE, P.MORE, P.OUT_OF_BUDGET, P.INVALID)), states
    assert all(stops[s] >= 4 for s in (P.DEAD_END, P.LIMIT, P.TARGET, P.BUDGET)), stops


def test_paths_loop_at_dense_forks_and_without_min_support(host, sides):
    """ctx 2 on the gt reads: every node forks four ways, the frame store is full and all 256 slots of a seed are taken"""
    sds = W.seeds(2)
    for limits in (X.DENSE_FULL, (4, 256, 84)):
        ss = P.searches(sides["plain"], ("plain", "dealt", SHARDS, "dense"), sds, None, 2, 1, limits, False, False)
        want_state, want_paths = X.DENSE_LIMITS[limits]
        assert all((s.state, len(s.paths)) == (want_state, want_paths) for s in ss if s.state != P.INVALID)
        assert host("paths", "plain", sds, 2, 1, *limits, False, False, 1)[0] == _paths_lines(ss)
    ss = P.searches(sides["stranded"], ("stranded", "dealt", SHARDS, False), W.seeds(12), None, 12, 1, P.TIGHT, True, False)
    assert host("paths", "stranded", W.seeds(12), 12, 1, *P.TIGHT, True, False, 0)[0] == _paths_lines(ss, optional=False)
