"""CPU suite: tests/unitig_reference.py's statement of rsbwt_set_unitigs agrees with itself over the oracle's BWT and with
no BWT at all, on both read sets and every dealing; the inputs reach every class of stop -- JOIN among them, at 0 steps
too -- and sides that differ from today's walk; the known return candidate counts what its onward twin counted; the
decision header (readserver_amd/csrc/unitig_rule.h) as a program of its own under the address and undefined-behaviour
sanitizers, held to a restatement in Python; and the new entry points are declared, exported, bound and refuse what the
header says they refuse."""
import ctypes as C
import os
import re
import shutil
import subprocess
from collections import Counter

import numpy as np
import pytest

import gt_reference as G
import unitig_reference as U
import walk_reference as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = {"rsbwt_set_unitigs": 13, "rsbwt_set_unitigs_dev": 15, "rsbwt_set_unitig_last_work": 1}


@pytest.fixture(scope="module")
def sides(oracle):
    """{set name: (OracleSide, PlainSide)} over the two shards as they are"""
    out = {}
    for name, reads in W.read_sets().items():
        orc = [G.OracleShard(oracle.from_runs(r, len(sh))) for sh, r in zip(reads, W.runs(name, 2))]
        out[name] = (W.OracleSide(orc), W.PlainSide(reads))
    return out


def _unitigs(sides, name, which, ctx, m, both):
    return U.unitigs(sides[name][which], (name, which), U.seeds(ctx), ctx, m, W.MAX_STEPS, both)


@pytest.mark.parametrize("both", [False, True])
@pytest.mark.parametrize("ctx", W.CTXS)
@pytest.mark.parametrize("name", ["plain", "stranded"])
def test_the_two_statements_agree(sides, name, ctx, both):
    for m in W.MIN_COUNTS:
        a = _unitigs(sides, name, 0, ctx, m, both)
        b = _unitigs(sides, name, 1, ctx, m, both)
        assert a == b, (name, ctx, m, both, [i for i, (x, y) in enumerate(zip(a, b)) if x != y][:5])
        assert U.expected_work(sides[name][0], a, both) == U.expected_work(sides[name][1], b, both)


def test_the_special_seeds(sides):
    for ctx in W.CTXS:
        us = _unitigs(sides, "plain", 0, ctx, 1, False)[W.N_PLAIN:]
        assert len(us) == 6
        invalid = [(r.stop == U.INVALID, l.stop == U.INVALID) for r, l in us]
        # shorter than ctx; an N in either context; an N outside both; empty; exactly ctx symbols; an N in the left context only
        assert invalid == [(True, True), (True, True), (False, False), (True, True), (False, False), (False, True)], (ctx, invalid)
        for pair in us:
            for s in pair:
                if s.stop == U.INVALID:
                    assert s == U.Side("", U.INVALID, (), U.ZERO8, s.final, (), ())
        right, left = us[5]
        assert right.onward and left.onward == ()  # the side beside an invalid one walks
        assert U.sequence("CCC", "AG", "TG") == "GTCCCAG"


def test_unitigs_do_not_depend_on_the_dealing():
    for name, both in (("plain", False), ("stranded", True)):
        want = None
        for S in W.DEALS:
            side = W.PlainSide(W.dealt(name, S))
            got = [(r[:4], l[:4]) for r, l in U.unitigs(side, (name, "dealt", S), U.seeds(12), 12, 2, W.MAX_STEPS, both)]
            want = want or got
            assert got == want, (name, S)


@pytest.mark.parametrize("both", [False, True])
@pytest.mark.parametrize("name", ["plain", "stranded"])
def test_joins_and_the_walk(sides, name, both):
    """the known return candidate is the onward candidate of the live symbol; a side that is the walk's stops as the walk
    does; a JOIN side is a proper prefix of the walk, or the walk stopped at the same length"""
    joins = 0
    for ctx in W.CTXS:
        for m in W.MIN_COUNTS:
            us = _unitigs(sides, name, 0, ctx, m, both)
            for d, left in enumerate((False, True)):
                ws = W.walks(sides[name][0], (name, 0, "unitig seeds"), U.seeds(ctx), ctx, m, W.MAX_STEPS, left, both)
                for pair, w in zip(us, ws):
                    s = pair[d]
                    if s.stop == U.JOIN:
                        joins += 1
                        live = [b for b in range(4) if s.last[b] >= m]
                        assert len(live) == 1 and sum(x >= m for x in s.last[4:]) >= 2
                        assert s.last[4 + U.known(s, ctx, left)] == s.last[live[0]], (name, ctx, m, left, s)
                        assert (len(s.ext) < len(w.ext) and w.ext.startswith(s.ext)) or len(w.ext) == len(s.ext), (name, ctx, m, left, s, w)
                        assert w.ext.startswith(s.ext)
                    else:
                        assert s.last[4:] == (0, 0, 0, 0)
                        if s.ext == w.ext:
                            assert s.stop == w.stop and s.last[:4] == w.last and s.support == w.support, (name, ctx, m, left, s, w)
                    assert len(s.onward) == len(s.ext) + (s.stop in (U.DEAD_END, U.BRANCH, U.JOIN))
                    assert len(s.back) == len(s.ext) + (s.stop == U.JOIN)
    assert joins >= 20, joins


def test_the_inputs_reach_every_class(sides):
    """the yardstick is a prototype's count over PlainSide at (plain, 12, 1, one strand, max_steps 64) on the 53 windows:
    right 2 DEAD_END, 37 BRANCH, 7 LIMIT, 7 JOIN, 7 sides unlike the walk; left 4, 33, 6, 10, 10.  At ctx 20: 16 JOIN to the
    right and 15 to the left"""
    us = _unitigs(sides, "plain", 1, 12, 1, False)[:W.N_PLAIN]
    table = {}
    for d, left in enumerate((False, True)):
        ws = W.walks(sides["plain"][1], ("plain", 1, "unitig seeds"), U.seeds(12), 12, 1, W.MAX_STEPS, left, False)[:W.N_PLAIN]
        stops = Counter(pair[d].stop for pair in us)
        differ = sum(pair[d].ext != w.ext for pair, w in zip(us, ws))
        table[left] = (stops[U.DEAD_END], stops[U.BRANCH], stops[U.LIMIT], stops[U.JOIN], differ)
        print("left" if left else "right", table[left])
        for s in (U.DEAD_END, U.BRANCH, U.LIMIT, U.JOIN):
            assert stops[s] >= 2, (left, s, stops)
        assert stops[U.JOIN] >= 5 and differ >= 5, (left, stops, differ)
        assert sum(len(pair[d].ext) >= 16 for pair in us) >= 20, left
    assert table == {False: (2, 37, 7, 7, 7), True: (4, 33, 6, 10, 10)}, table
    at20 = _unitigs(sides, "plain", 1, 20, 1, False)[:W.N_PLAIN]
    assert [sum(pair[d].stop == U.JOIN for pair in at20) for d in (0, 1)] == [16, 15]
    # a JOIN at 0 steps: the seed's own end node is entered by another path
    zero = {(m, d): sum(pair[d].stop == U.JOIN and pair[d].ext == "" for pair in _unitigs(sides, "plain", 1, 12, m, False)[:W.N_PLAIN])
            for m in (1, 2) for d in (0, 1)}
    print(zero)
    assert zero[(1, 0)] >= 1 and zero[(2, 1)] >= 1, zero


def _rule(sums, m, steps, max_steps):
    """unitig_rule.h in Python: (stop, pick)"""
    if steps >= max_steps:
        return U.LIMIT, -1
    live = [b for b in range(4) if sums[b] >= m]
    if len(live) != 1:
        return (U.BRANCH if live else U.DEAD_END), -1
    if sum(x >= m for x in sums[4:]) >= 2:
        return U.JOIN, -1
    return 0, live[0]


def test_rule_header_under_address_and_ub_sanitizers(tmp_path):
    """tests/native/unitig_rule_host.cpp: every (sum >= m) pattern of the eight sums at steps 0, max_steps - 1 and max_steps,
    with small sums and with sums past 32 bits; the two halves the kernel calls say what the whole rule says"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "unitig_rule_host")
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(ROOT, "tests", "native", "unitig_rule_host.cpp"), "-o", exe], capture_output=True, text=True)
    if b.returncode != 0 and "sanitize" in b.stderr:
        pytest.skip("no sanitizer runtime here")
    assert b.returncode == 0, b.stderr
    for m, max_steps in ((1, 1), (3, 64), (2, 65535)):
        r = subprocess.run([exe, str(m), str(max_steps)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stdout.rstrip().endswith("unitig_rule ok"), r.stdout[-2000:] + r.stderr[-3000:]
        lines = r.stdout.splitlines()[:-1]
        assert len(lines) == 2 * 3 * 256
        seen, patterns = Counter(), set()
        for ln in lines:
            f = [int(x) for x in ln.split()]
            steps, sums, (stop, pick, halves, sat) = f[0], f[1:9], f[9:]
            assert (stop, pick) == _rule(sums, m, steps, max_steps), ln
            assert halves == 1 and sat == (min(sums[pick], 2 ** 32 - 1) if stop == 0 else 0), ln
            seen[stop] += 1
            patterns.add((steps, tuple(x >= m for x in sums)))
        assert len(patterns) == len({0, max_steps - 1, max_steps}) * 256
        assert set(seen) == {0, U.DEAD_END, U.BRANCH, U.LIMIT, U.JOIN}, seen


def test_entry_points_are_declared_exported_and_bound_and_refuse_bad_arguments(rsb):
    from readserver_amd import _native
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rsbwt.h")).read(), flags=re.S)
    L = C.CDLL(rsb.lib_path())
    for n, nargs in ENTRY.items():
        m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % n, txt, flags=re.S)
        assert m and len(m.group(1).split(",")) == nargs, f"{n} is not declared in include/rsbwt.h with {nargs} arguments"
        assert n in _native.SIGNATURES and hasattr(L, n) and hasattr(rsb.lib(), n)
        assert len(_native.SIGNATURES[n][1]) == nargs, n
    assert re.search(r"#define RSBWT_WALK_JOIN 5\b", txt)
    assert rsb.bwt.WALK_JOIN == U.JOIN == 5
    assert callable(rsb.ShardSet.unitigs) and callable(rsb.ShardSet.unitigs_last_work)
    assert rsb.unitig_sequence("CCC", "AG", "TG") == U.sequence("CCC", "AG", "TG") == "GTCCCAG"
    L = rsb.lib()
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    text = np.frombuffer(b"ACGTACGT", np.uint8).copy()
    off = np.array([0, 4, 8], np.uint64)
    ext, steps, stop = np.full(16, 77, np.uint8), np.full(4, 77, np.uint32), np.full(4, 77, np.uint8)
    none = L.rsbwt_device_count() == 0
    # a box without a GPU can have no set: RSBWT_ENODEV, no CPU fallback; where there is one a null set is RSBWT_EINVAL
    want = -5 if none else -1
    assert L.rsbwt_set_unitigs(None, p(text), p(off), 2, 4, 1, 4, 0, p(ext), p(steps), p(stop), None, None) == want
    assert (b"no CPU fallback" if none else b"null") in L.rsbwt_last_error()
    assert L.rsbwt_set_unitigs(None, None, None, 0, 4, 1, 4, 0, None, None, None, None, None) == want
    assert L.rsbwt_set_unitigs_dev(None, None, None, 0, 0, 4, 1, 4, 0, None, None, None, None, None, None) == -1
    assert (ext == 77).all() and (steps == 77).all() and (stop == 77).all()
    w = (C.c_uint64 * 8)(*([9] * 8))
    L.rsbwt_set_unitig_last_work(None)  # (nothing to write to: no crash)
    L.rsbwt_set_unitig_last_work(w)
    assert list(w) == [0] * 8  # the failed calls above did no work
    assert rsb.ShardSet.unitigs_last_work() == dict(seeds=0, appended=0, searches=0, lf_steps=0, passes=0, table_starts=0, onward=0, back=0)
