"""CPU guards for the sample-walk tests: tests/sample_walk_reference.py's two restatements of rsbwt_set_extension_samples /
rsbwt_set_walk_samples -- over sample_reference.counts_plain (no BWT) and over counts_oracle -- agree on the haplotype
fixture and on the gt fixture's reads under sample_reference.sample_pairs' values; the haplotype fixture tells the story it
is there for; the host rule header (readserver_amd/csrc/sample_walk_rule.h) runs under the address and undefined-behaviour
sanitizers as a program of its own; the entry points are declared, exported and bound and refuse what they must without a
GPU."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import sample_reference as SR
import sample_walk_reference as SW
import walk_reference as WR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = {"rsbwt_set_extension_samples": 16, "rsbwt_set_walk_samples": 20, "rsbwt_set_walk_samples_dev": 23, "rsbwt_set_walk_samples_last_work": 1,
         "rsbwt_set_walk_samples_last_times": 1}
MASKS = {"a1": [SW.A1], "b1": [SW.B1], "a1+b1": [SW.A1, SW.B1], "none": []}


def _flank_seed(fx):
    return fx.a[10:40]


@pytest.mark.parametrize("S", [1, 3])
def test_the_two_restatements_agree_on_the_haplotypes(oracle, S):
    fx = SW.haplotype_fixture()
    shards = SW.dealt(fx.reads, S)
    osh = SR.OracleShards(oracle, shards, SW.runs(fx.reads, S), fx.pairs)
    seeds = [_flank_seed(fx), fx.b[60:85], fx.a[150:190], fx.a[5:24], fx.a[:19] + "N" + fx.a[20:45]]
    for name, mask in MASKS.items():
        for copies in (False, True):
            p = SW.plain_side(shards, fx.pairs, fx.codes, fx.size_of_sample, fx.has_other, mask, copies)
            o = SW.oracle_side(osh, fx.codes, fx.size_of_sample, fx.has_other, mask, copies)
            for left in (False, True):
                for both in (False, True):
                    for max_rows in (4096, 12):
                        a = [SW.walk(p, s, 20, 1, 200, left, both, max_rows) for s in seeds]
                        b = [SW.walk(o, s, 20, 1, 200, left, both, max_rows) for s in seeds]
                        assert a == b, (name, copies, left, both, max_rows)
                        assert [SW.evaluate(p, s, 20, left, both, max_rows) for s in seeds] == [SW.evaluate(o, s, 20, left, both, max_rows) for s in seeds]


def test_the_haplotype_fixture_shows_the_feature():
    """the plain walk branches at the SNP; one haplotype's samples walk through the SNP and the deletion along their own
    haplotype; both together branch; nobody dead-ends at 0 steps; a dealing to shards changes nothing"""
    fx = SW.haplotype_fixture()
    seed = _flank_seed(fx)
    assert len(fx.a) == 200 and len(fx.b) == 198 and fx.a[:fx.snp] == fx.b[:fx.snp] and fx.a[fx.snp] != fx.b[fx.snp]
    assert all(40 <= len(r) <= 60 for r in fx.reads) and len(set(fx.reads)) < len(fx.reads)  # (reads both haplotypes spell)
    want = None
    for S in (1, 2, 3, 4, 8):
        shards = SW.dealt(fx.reads, S)
        plain = WR.walk(WR.PlainSide(shards), seed, 20, 1, 200, False, False)
        assert plain.stop == WR.BRANCH and len(plain.ext) == fx.snp - 40 and seed + plain.ext == fx.a[10:fx.snp]
        got = {}
        for name, mask in MASKS.items():
            side = SW.plain_side(shards, fx.pairs, fx.codes, fx.size_of_sample, fx.has_other, mask)
            got[name] = SW.walk(side, seed, 20, 1, 200, False, False, 4096)
        a, b = got["a1"], got["b1"]
        assert a.stop == WR.DEAD_END and (seed + a.ext).startswith(fx.a[10:fx.indel + 30]) and fx.a.startswith(fx.a[:10] + seed + a.ext)
        assert b.stop == WR.DEAD_END and (seed + b.ext).startswith(fx.b[10:fx.indel + 30]) and fx.b.startswith(fx.b[:10] + seed + b.ext)
        assert got["a1+b1"].stop == WR.BRANCH and got["a1+b1"].ext == plain.ext
        assert got["none"] == WR.Walk("", WR.DEAD_END, (), (0, 0, 0, 0), seed, (seed[-20:],))
        # (the supports do depend on the dealing: a string present in two shards counts in each)
        got = {k: (w.ext, w.stop) for k, w in got.items()}
        want = want or got
        assert got == want, S


def test_the_gt_reads_reach_what_the_kernel_can_get_wrong(oracle):
    """on the gt fixture's stranded reads under sample_pairs' values (record counts 0 .. 2,000, stray tails, a code listed
    twice, negative c, unknown codes, reads left out): the restatements agree, copies differ from strings, a limit at a
    candidate's matches walks on and one below stops WIDE, and the seeds inside the tandem repeat stop WIDE at a small limit"""
    c = SW.gt_case(oracle)
    for copies in (False, True):
        for left, both in ((False, True), (True, False)):
            a = SW.gt_walks(c, "plain", copies, left, both, 4096)
            b = SW.gt_walks(c, "oracle", copies, left, both, 4096)
            assert a == b, (copies, left, both)
    one = SW.gt_walks(c, "plain", False, False, True, 4096)
    cp = SW.gt_walks(c, "plain", True, False, True, 4096)
    assert [w.support for w in one] != [w.support for w in cp]
    assert {w.stop for w in one} >= {WR.DEAD_END, WR.BRANCH, WR.LIMIT, WR.INVALID}
    # what the carriers of these walks bring: every class of record count, the read that lists a code twice, reads left out
    asked = [x for x, v in c._memo["plain"].items() if v[2] > 0]
    named, R = dict(c.pairs), SR.rec_size(c.ss, c.other)
    holders = {r for sh in c.shards for r in sh if any(x in r for x in asked)}
    assert {len(named[r]) // R for r in holders if r in named} >= {0, 15, 16, 17, 300, 2000}
    assert c.info["doubled"] in holders and len(holders & c.info["left_out"]) >= 2
    assert any(len(named[r]) % R for r in holders if r in named)  # (a stray tail)
    # the WIDE boundary of the first seed's first evaluation
    side = c.side("plain", False)
    _, _, matches = SW.evaluate(side, c.seeds[0], c.ctx, False, False, 4096)
    per = [side.matches(x) for x in WR.candidates(WR.context(c.seeds[0], c.ctx, False), False)]
    assert max(per) >= 2 and tuple(per) == matches
    assert SW.evaluate(side, c.seeds[0], c.ctx, False, False, max(per))[1] is False
    assert SW.evaluate(side, c.seeds[0], c.ctx, False, False, max(per) - 1)[1] is True
    inside = [i for i in WR.seeds_inside_the_repeat() if i < len(c.all_seeds)]
    assert inside
    ws = [SW.walk(side, c.all_seeds[i], c.ctx, 1, 8, False, False, 3) for i in inside[:3]]
    assert all(w.stop == SW.WIDE for w in ws), [w.stop for w in ws]


def test_rule_header_under_address_and_ub_sanitizers(tmp_path):
    """tests/native/sample_walk_rule_host.cpp: the mask's bitmap on exactly-sized arrays, the slice sizing against the
    budget, the set's slots and keys, WIDE at every position, the clamp and the decision over every (sum >= m) pattern"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "sample_walk_rule_host")
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(ROOT, "tests", "native", "sample_walk_rule_host.cpp"), "-o", exe], capture_output=True, text=True)
    if b.returncode != 0 and "sanitize" in b.stderr:
        pytest.skip("no sanitizer runtime here")
    assert b.returncode == 0, b.stderr
    for Cn, max_rows, m in ((1, 1, 1), (31, 73, 2), (32, 4096, 1), (33, 4097, 3), (2000, 1 << 20, 1)):
        r = subprocess.run([exe, str(Cn), str(max_rows), str(m)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stdout.rstrip().endswith("sample_walk_rule ok"), r.stdout[-2000:] + r.stderr[-3000:]
        lines = [ln.split() for ln in r.stdout.splitlines()[:-1]]
        assert [ln for ln in lines if ln[0] == "mask"][0][1:3] == [str(Cn), str((Cn + 31) // 32)]
        assert [ln for ln in lines if ln[0] == "rows_ok"][0][1:] == ["0", "1", "1", "0"]
        _, mr, per, cap = [ln for ln in lines if ln[0] == "slice"][0]
        # the restatement of the slicing: 52 bytes a row, 8 x max_rows rows a seed, 256 MiB, 1 .. 2,048 seeds
        assert int(per) == min(2048, max(1, (256 << 20) // (8 * max_rows * 52))) and int(cap) == int(per) * 8 * max_rows
        steps = [[int(x) for x in ln[1:]] for ln in lines if ln[0] == "step"]
        assert len(steps) == 32
        for pat, wide, s0, s1, s2, s3, why, pick in steps:
            live = [b_ for b_, s in enumerate((s0, s1, s2, s3)) if s >= m]
            assert live == [b_ for b_ in range(4) if (pat >> b_) & 1]
            want = (8, 99) if wide else (0, live[0]) if len(live) == 1 else (1 if not live else 2, 99)
            assert (why, pick) == want, (pat, wide)
        assert [ln[2] for ln in lines if ln[0] == "wide"] == ["1"] * 8 + ["0"]
        for _, f, rv, got in (ln for ln in lines if ln[0] == "support"):
            assert int(got) == max(int(f) + int(rv), 0)


def test_entry_points_are_declared_exported_and_bound_and_refuse_bad_arguments(rsb):
    from readserver_amd import _native
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rsbwt.h")).read(), flags=re.S)
    L = C.CDLL(rsb.lib_path())
    for n, nargs in ENTRY.items():
        assert re.search(r"\b%s\s*\(" % n, txt), f"{n} is not declared in include/rsbwt.h"
        assert n in _native.SIGNATURES and hasattr(L, n) and hasattr(rsb.lib(), n)
        assert len(_native.SIGNATURES[n][1]) == nargs, n
    for name, value in (("RSBWT_WALK_SAMPLE_COPIES", "4u"), ("RSBWT_WALK_WIDE", "8")):
        assert re.search(r"#define %s %s\b" % (name, value), txt), name
    assert rsb.bwt.WALK_WIDE == SW.WIDE
    assert callable(rsb.ShardSet.extension_samples) and callable(rsb.ShardSet.walk_samples) and callable(rsb.ShardSet.walk_samples_last_work)
    L = rsb.lib()
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    text = np.frombuffer(b"ACGTACGT", np.uint8).copy()
    off = np.array([0, 4, 8], np.uint64)
    codes, mask = np.frombuffer(b"a1b1", np.uint8).copy(), np.array([1, 0], np.uint8)
    msup, wide = np.full(8, 77, np.uint64), np.full(2, 77, np.uint8)
    ext, steps, stop = np.full(8, 77, np.uint8), np.full(2, 77, np.uint32), np.full(2, 77, np.uint8)
    none = L.rsbwt_device_count() == 0
    want = -5 if none else -1  # (no set can be had without a GPU: RSBWT_ENODEV; with one a null set is RSBWT_EINVAL)
    assert L.rsbwt_set_extension_samples(None, p(text), p(off), 2, 4, 0, p(codes), 2, 2, 1, p(mask), 16, 0, p(msup), p(wide), None) == want
    assert (b"no CPU fallback" if none else b"null") in L.rsbwt_last_error()
    assert L.rsbwt_set_walk_samples(None, p(text), p(off), 2, 4, 1, 4, 0, p(codes), 2, 2, 1, p(mask), 16, 0, p(ext), p(steps), p(stop), None, None) == want
    assert L.rsbwt_set_walk_samples(None, None, None, 0, 4, 1, 4, 0, None, 0, 0, 0, None, 0, 0, None, None, None, None, None) == want
    assert L.rsbwt_set_walk_samples_dev(None, None, None, 0, 0, 4, 1, 4, 0, None, 0, 0, 0, None, 0, 0, None, None, None, None, None, None, None) == -1
    assert (msup == 77).all() and (wide == 77).all() and (ext == 77).all() and (steps == 77).all() and (stop == 77).all()
    w = (C.c_uint64 * 10)(*([9] * 10))
    L.rsbwt_set_walk_samples_last_work(None)  # (nothing to write to: no crash)
    L.rsbwt_set_walk_samples_last_work(w)
    assert list(w) == [0] * 10  # the failed calls above did no work
    t = (C.c_double * 7)(*([9.0] * 7))
    L.rsbwt_set_walk_samples_last_times(None)
    L.rsbwt_set_walk_samples_last_times(t)
    assert list(t) == [0.0] * 7 and tuple(rsb.ShardSet.walk_samples_last_times()) == ("init", "search", "plan", "rows", "locate", "tally", "decide")
