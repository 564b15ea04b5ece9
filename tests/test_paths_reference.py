"""CPU suite: tests/paths_reference.py's statement of rsbwt_set_paths agrees with itself over the oracle's BWT and with no
BWT at all, on both read sets; shown by counting, the inputs reach every seed state and every stop, backtracks past the
last fork and bubbles that close at the target; a search relates to today's walk as the header says; the decision header
(readserver_amd/csrc/paths_rule.h) as a program of its own under the address and undefined-behaviour sanitizers, held to a
restatement in Python; and the new entry points are declared, exported, bound and refuse a missing set."""
import ctypes as C
import os
import re
import shutil
import subprocess
from collections import Counter

import numpy as np
import pytest

import gt_reference as G
import paths_reference as P
import walk_reference as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = {"rsbwt_set_paths": 18, "rsbwt_set_paths_dev": 21, "rsbwt_set_paths_last_work": 1}
SETTINGS = [(ctx, m, left, both) for ctx in W.CTXS for m in (1, 2) for left in (False, True) for both in (False, True)]


@pytest.fixture(scope="module")
def sides(oracle):
    """{set name: (OracleSide, PlainSide)} over the two shards as they are"""
    out = {}
    for name, reads in W.read_sets().items():
        orc = [G.OracleShard(oracle.from_runs(r, len(sh))) for sh, r in zip(reads, W.runs(name, 2))]
        out[name] = (W.OracleSide(orc), W.PlainSide(reads))
    return out


def _searches(sides, name, which, ctx, m, left, both, limits=P.WIDE, targets=True):
    return P.searches(sides[name][which], (name, which, targets), W.seeds(ctx), P.targets(ctx, left) if targets else None, ctx, m, limits, left, both)


@pytest.mark.parametrize("both", [False, True])
@pytest.mark.parametrize("ctx", W.CTXS)
@pytest.mark.parametrize("name", ["plain", "stranded"])
def test_the_two_statements_agree(sides, name, ctx, both):
    for m in (1, 2):
        for left in (False, True):
            for limits, targets in ((P.WIDE, True), (P.WIDE, False), (P.TIGHT, True)):
                a = _searches(sides, name, 0, ctx, m, left, both, limits, targets)
                b = _searches(sides, name, 1, ctx, m, left, both, limits, targets)
                assert a == b, (name, ctx, m, left, both, limits, targets, [i for i, (x, y) in enumerate(zip(a, b)) if x != y][:5])
            assert P.expected_work(sides[name][0], a, left, both) == P.expected_work(sides[name][1], b, left, both)


def test_the_special_seeds_and_targets(sides):
    for ctx in W.CTXS:
        for left in (False, True):
            tg = P.targets(ctx, left)
            assert len(tg) == len(W.seeds(ctx)) == 58 and all(len(t) <= ctx for t in tg)
            assert "N" in tg[3] and tg[5] == "" and tg[W.N_PLAIN:] == [""] * 5 and sum(bool(t) for t in tg) >= 45
            ss = _searches(sides, "plain", 1, ctx, 1, left, False)[W.N_PLAIN:]
            # shorter than ctx; an N in either context; an N outside both; empty; exactly ctx symbols
            assert [s.state == P.INVALID for s in ss] == [True, True, False, True, False]
            assert all(s == P.Search(P.INVALID, (), (), ()) for s in ss if s.state == P.INVALID)
        # a target that holds an N never matches: the seed's paths are those without a target
        with_t, without = (_searches(sides, "plain", 1, ctx, 1, False, False, targets=t) for t in (True, False))
        assert with_t[3] == without[3] and with_t[5] == without[5]
        assert sum(a != b for a, b in zip(with_t, without)) >= 10


def test_paths_do_not_depend_on_the_dealing():
    for name, both in (("plain", False), ("stranded", True)):
        want = None
        for S in W.DEALS:
            side = W.PlainSide(W.dealt(name, S))
            got = [s[:2] for s in P.searches(side, (name, "dealt", S), W.seeds(12), P.targets(12, False), 12, 2, P.WIDE, False, both)]
            want = want or got
            assert got == want, (name, S)


def test_the_inputs_reach_every_class(sides):
    """shown by counting over the tested settings: every seed state and every stop on two seeds or more of some setting,
    a backtrack to a depth that is not the seed's last fork, and seeds with two or more TARGET paths (closed bubbles)"""
    best_state, best_stop, tight = Counter(), Counter(), Counter()
    past_fork = bubbles = most_evals = 0
    for name in ("plain", "stranded"):
        for ctx, m, left, both in SETTINGS:
            for limits, targets in ((P.WIDE, True), (P.WIDE, False), (P.TIGHT, True)):
                ss = _searches(sides, name, 1, ctx, m, left, both, limits, targets)
                states = Counter(s.state for s in ss)
                stops = Counter()
                for s in ss:
                    stops.update({p[1] for p in s.paths})  # (seeds that have the stop)
                    assert len(s.paths) <= limits[1] and len(s.evaluated) <= limits[2]
                    assert all(len(p[0]) <= limits[0] for p in s.paths)
                    assert len({p[0] for p in s.paths}) == len(s.paths)  # no path twice
                    assert (s.state == P.MORE) <= (len(s.paths) == limits[1])
                    assert (s.state == P.OUT_OF_BUDGET) == (bool(s.paths) and s.paths[-1][1] == P.BUDGET)
                    assert all(p[1] != P.BUDGET for p in s.paths[:-1])
                for k, v in states.items():
                    best_state[k] = max(best_state[k], v)
                for k, v in stops.items():
                    best_stop[k] = max(best_stop[k], v)
                if limits == P.WIDE:
                    past_fork = max(past_fork, sum(any(d != f for d, f in s.backtracks) for s in ss))
                    if targets:
                        bubbles = max(bubbles, sum(sum(p[1] == P.TARGET for p in s.paths) >= 2 for s in ss))
                    else:
                        most_evals = max(most_evals, max(len(s.evaluated) for s in ss))
                if limits == P.TIGHT:  # the tight set is there for MORE and BUDGET: some setting has two seeds or more of each
                    tight[P.MORE] = max(tight[P.MORE], states[P.MORE])
                    tight[P.OUT_OF_BUDGET] = max(tight[P.OUT_OF_BUDGET], states[P.OUT_OF_BUDGET])
    print(dict(best_state), dict(best_stop), dict(tight), past_fork, bubbles, most_evals)
    assert tight[P.MORE] >= 2 and tight[P.OUT_OF_BUDGET] >= 2, tight
    assert all(best_state[s] >= 2 for s in (P.COMPLETE, P.MORE, P.OUT_OF_BUDGET, P.INVALID)), best_state
    assert all(best_stop[s] >= 2 for s in (P.DEAD_END, P.LIMIT, P.TARGET, P.BUDGET)), best_stop
    assert past_fork >= 2 and bubbles >= 5, (past_fork, bubbles)
    assert most_evals < P.WIDE[2]  # without a target no seed runs out of the wide budget: its BUDGET cases are the tight set's


@pytest.mark.parametrize("name", ["plain", "stranded"])
def test_paths_and_the_walk(sides, name):
    """a seed whose walk stops DEAD_END or LIMIT has exactly that one path; where the walk stops BRANCH every path strictly
    extends the walk's ext (no targets; the wide limits)"""
    branches = 0
    for ctx, m, left, both in SETTINGS:
        ws = W.walks(sides[name][1], (name, 1, "paths seeds"), W.seeds(ctx), ctx, m, P.WIDE[0], left, both)
        ss = _searches(sides, name, 1, ctx, m, left, both, targets=False)
        for w, s in zip(ws, ss):
            assert (w.stop == W.INVALID) == (s.state == P.INVALID)
            if w.stop in (W.DEAD_END, W.LIMIT):
                assert s.state == P.COMPLETE and s.paths == ((w.ext, w.stop, min(w.support) if w.support else 0),), (ctx, m, left, both, w, s)
            elif w.stop == W.BRANCH:
                branches += 1
                assert len(s.paths) >= 2 or s.state != P.COMPLETE
                assert all(len(p[0]) > len(w.ext) and p[0].startswith(w.ext) for p in s.paths), (ctx, m, left, both, w, s)
    assert branches >= 100, branches


def _search(seed, m, max_steps, max_paths, max_evals, target):
    """tests/native/paths_rule_host.cpp's search in Python, by the header's pseudocode: (state, npaths, evals, [lines])"""
    table = [0, 0, 0, 0, 0, 0, 0, 1, 1, 2, 3, 5, 9, 0xFFFFFFFF, 0x100000000, 0x200000005]

    def support(path, c):
        h = 1469598103934665603
        for ch in ("%d:%s%s" % (seed, path, "ACGT"[c])).encode():
            h = ((h ^ ch) * 1099511628211) & (2 ** 64 - 1)
        return table[(h >> 20) & 15]

    path, pend, evals, out, sups = "", {}, 0, [], []
    while True:
        if target and len(path) >= 1 and path.endswith(target):
            stop = P.TARGET
        elif len(path) == max_steps:
            stop = P.LIMIT
        elif evals == max_evals:
            stop = P.BUDGET
        else:
            evals += 1
            tot = [support(path, c) for c in range(4)]
            live = [c for c in range(4) if tot[c] >= m]
            if live:
                if live[1:]:
                    pend[len(path)] = (live[1:], tot, list(sups))
                path += "ACGT"[live[0]]
                sups.append(min(tot[live[0]], P.SAT))
                continue
            stop = P.DEAD_END
        out.append("%s %d %d" % (path or "-", stop, min(sups) if sups else 0))
        state = P.OUT_OF_BUDGET if stop == P.BUDGET else P.COMPLETE if not pend else P.MORE if len(out) == max_paths else 0
        if state:
            return state, len(out), evals, out
        d = max(pend)
        untried, tot, before = pend[d]
        c = untried.pop(0)
        if not untried:
            del pend[d]
        path, sups = path[:d] + "ACGT"[c], before + [min(tot[c], P.SAT)]


def test_rule_header_under_address_and_ub_sanitizers(tmp_path):
    """tests/native/paths_rule_host.cpp: the header's decisions drive whole searches over a hashed graph whose supports
    include zeros, small counts and counts at and past 32 bits, with the frame store at exactly the size the header names"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "paths_rule_host")
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(ROOT, "tests", "native", "paths_rule_host.cpp"), "-o", exe], capture_output=True, text=True)
    if b.returncode != 0 and "sanitize" in b.stderr:
        pytest.skip("no sanitizer runtime here")
    assert b.returncode == 0, b.stderr
    states, stops, saturated = Counter(), Counter(), 0
    for m, max_steps, max_paths, max_evals, target in ((1, 12, 8, 64, "GA"), (2, 6, 3, 20, "-"), (1, 1, 1, 1, "T"), (3, 40, 256, 30, "C"),
                                                      (1, 5, 256, 1 << 20, "-"), (1, 65535, 2, 50, "-")):
        r = subprocess.run([exe, str(m), str(max_steps), str(max_paths), str(max_evals), "200", target], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stdout.rstrip().endswith("paths_rule ok"), r.stdout[-2000:] + r.stderr[-3000:]
        lines = r.stdout.splitlines()[:-1]
        at = 0
        for seed in range(200):
            state, npaths, evals, out = _search(seed, m, max_steps, max_paths, max_evals, "" if target == "-" else target)
            assert lines[at] == "%d %d %d" % (state, npaths, evals), (seed, lines[at], state, npaths, evals)
            assert lines[at + 1:at + 1 + npaths] == out, (m, max_steps, max_paths, max_evals, target, seed)
            at += 1 + npaths
            states[state] += 1
            stops.update(int(ln.split()[1]) for ln in out)
            saturated += sum(ln.endswith(" %d" % P.SAT) for ln in out)
        assert at == len(lines)
    print(states, stops, saturated)
    assert set(states) == {P.COMPLETE, P.MORE, P.OUT_OF_BUDGET} and min(states.values()) >= 20, states
    assert set(stops) == {P.DEAD_END, P.LIMIT, P.TARGET, P.BUDGET} and min(stops.values()) >= 20, stops
    assert saturated >= 5


def test_entry_points_are_declared_exported_and_bound_and_refuse_bad_arguments(rsb):
    from readserver_amd import _native
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rsbwt.h")).read(), flags=re.S)
    L = C.CDLL(rsb.lib_path())
    for n, nargs in ENTRY.items():
        m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % n, txt, flags=re.S)
        assert m and len(m.group(1).split(",")) == nargs, f"{n} is not declared in include/rsbwt.h with {nargs} arguments"
        assert n in _native.SIGNATURES and hasattr(L, n) and hasattr(rsb.lib(), n)
        assert len(_native.SIGNATURES[n][1]) == nargs, n
    for name, value in (("RSBWT_WALK_TARGET", 6), ("RSBWT_WALK_BUDGET", 7), ("RSBWT_PATHS_COMPLETE", 1), ("RSBWT_PATHS_MORE", 2),
                        ("RSBWT_PATHS_BUDGET", 3), ("RSBWT_PATHS_INVALID", 4)):
        assert re.search(r"#define %s %d\b" % (name, value), txt), name
    assert (rsb.bwt.WALK_TARGET, rsb.bwt.WALK_BUDGET) == (P.TARGET, P.BUDGET) == (6, 7)
    assert (rsb.bwt.PATHS_COMPLETE, rsb.bwt.PATHS_MORE, rsb.bwt.PATHS_BUDGET, rsb.bwt.PATHS_INVALID) == (P.COMPLETE, P.MORE, P.OUT_OF_BUDGET, P.INVALID)
    assert callable(rsb.ShardSet.paths) and callable(rsb.ShardSet.paths_last_work)
    L = rsb.lib()
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    text = np.frombuffer(b"ACGTACGT", np.uint8).copy()
    off = np.array([0, 4, 8], np.uint64)
    ext, steps, stop = np.full(2 * 2 * 4, 77, np.uint8), np.full(4, 77, np.uint32), np.full(4, 77, np.uint8)
    npaths, state = np.full(2, 77, np.uint32), np.full(2, 77, np.uint8)
    none = L.rsbwt_device_count() == 0
    # a box without a GPU can have no set: RSBWT_ENODEV, no CPU fallback; where there is one a null set is RSBWT_EINVAL
    want = -5 if none else -1
    assert L.rsbwt_set_paths(None, p(text), p(off), 2, None, None, 4, 1, 4, 2, 16, 0, p(ext), p(steps), p(stop), None, p(npaths), p(state)) == want
    assert (b"no CPU fallback" if none else b"null") in L.rsbwt_last_error()
    assert L.rsbwt_set_paths(None, None, None, 0, None, None, 4, 1, 4, 2, 16, 0, None, None, None, None, None, None) == want
    assert L.rsbwt_set_paths_dev(None, None, None, 0, 0, None, None, 0, 4, 1, 4, 2, 16, 0, None, None, None, None, None, None, None) == -1
    for a in (ext, steps, stop, npaths, state):
        assert (a == 77).all()
    w = (C.c_uint64 * 8)(*([9] * 8))
    L.rsbwt_set_paths_last_work(None)  # (nothing to write to: no crash)
    L.rsbwt_set_paths_last_work(w)
    assert list(w) == [0] * 8  # the failed calls above did no work
    assert rsb.ShardSet.paths_last_work() == dict(seeds=0, appended=0, searches=0, lf_steps=0, passes=0, table_starts=0, evals=0, paths=0)
