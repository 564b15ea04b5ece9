"""CPU suite: the launch plan (readserver_amd/csrc/launch_plan.h) -- the knobs, the resident-workgroup cap, the grid, the
draw size and the pair-or-lone-lane choice of every persistent launch.  tests/native/launch_plan_test.cpp prints what the
header plans for a table of inputs; the rules are restated here in plain Python, as the launchers spelled them out
before they shared the header, and every line is held to them -- once per environment, since a knob is read once per
process."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WG_WAVES = 4          # waves per workgroup of every kernel planned here
MIN_WGS = 4           # workgroups per CU: the search kernels, the branch kernel, the walkers, kmer_reads
WALK1MM_WGS = 3       # ... of the 1-mismatch walk
ROW_CHUNK = 256
KNOBS = ["RSBWT_WAVE_WGS_PER_CU", "RSBWT_WALK1MM_WGS_PER_CU", "RSBWT_EXTRACT_WGS_PER_CU", "RSBWT_SEARCH_SPARE_WGS",
         "RSBWT_SEARCH_KERNEL", "RSBWT_SET_1MM_SIDE_LOG2", "RSBWT_SET_1MM_TABLE_PREPASS", "RSBWT_KMER_WIDE_ROWS",
         "RSBWT_NO_STAGED_RESULTS"]


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("launch_plan") / "launch_plan_test")
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        f"-I{os.path.join(ROOT, 'readserver_amd', 'csrc')}", os.path.join(ROOT, "tests", "native", "launch_plan_test.cpp"),
                        "-o", exe], capture_output=True, text=True)
    if b.returncode != 0 and "sanitize" in b.stderr:
        pytest.skip("no sanitizer runtime here")
    assert b.returncode == 0, b.stderr
    return exe


def _run(exe, knobs):
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    env.update(knobs)
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=60)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    rows = []
    for line in r.stdout.splitlines():
        given, planned = line.split(" => ") if " => " in line else ("", line)
        kind, name, *kv = (given or planned).split()
        fields = lambda words: {w.split("=")[0]: int(w.split("=")[1]) for w in words}
        rows.append((kind, name, fields(kv) if given else {}, fields(planned.split()) if given else fields(kv)))
    return rows


# ---- the rules, as the launchers had them ------------------------------------------------------------------------------
def _atoi(text):
    m = re.match(r"\s*[+-]?\d+", text)
    return int(m.group()) if m else 0


def _knob(env, name, ok, fallback):
    """an integer knob: its value where `ok` accepts it, the fallback for anything else and when unset"""
    v = _atoi(env[name]) if name in env else None
    return v if v is not None and ok(v) else fallback


def _cap(cus, wgs_per_cu, spare=0):
    cap_all = cus * wgs_per_cu
    return cap_all - spare if cap_all > 2 * spare else cap_all


def _grid(items, per_wg, cap, nshards=None):
    g = min((items + per_wg - 1) // per_wg, cap)
    if nshards and g >= nshards:
        g -= g % nshards
    return g


def _draw(most, least, waves, draws, items):
    chunk = most
    while chunk > least and chunk * waves * draws > items:
        chunk >>= 1
    return chunk


def _expected(kind, a, env):
    wave_wgs = _knob(env, "RSBWT_WAVE_WGS_PER_CU", lambda v: v > 0, MIN_WGS)
    walk_wgs = _knob(env, "RSBWT_WALK1MM_WGS_PER_CU", lambda v: 0 < v <= WALK1MM_WGS, WALK1MM_WGS)
    extract_wgs = _knob(env, "RSBWT_EXTRACT_WGS_PER_CU", lambda v: 0 < v <= 20, MIN_WGS)
    spare = _knob(env, "RSBWT_SEARCH_SPARE_WGS", lambda v: v > 0, 0)
    choice = {"pair": 0, "solo": 1}.get(env.get("RSBWT_SEARCH_KERNEL"), 2)
    if kind == "knobs":
        return dict(wave_wgs=wave_wgs, walk1mm_wgs=walk_wgs, extract_wgs=extract_wgs, spare=spare, choice=choice,
                    side_log2=_knob(env, "RSBWT_SET_1MM_SIDE_LOG2", lambda v: 10 <= v <= 40, 26),
                    table_prepass=int(_atoi(env["RSBWT_SET_1MM_TABLE_PREPASS"]) != 0) if "RSBWT_SET_1MM_TABLE_PREPASS" in env else 1,
                    wide_rows=_knob(env, "RSBWT_KMER_WIDE_ROWS", lambda v: v > 0, 1 << 22),
                    no_staged=int("RSBWT_NO_STAGED_RESULTS" in env))
    cus = a["cus"]
    if kind == "search":
        n = a["Q"] * a["S"]
        cap = _cap(cus, wave_wgs, spare)
        solo = not a["table"] and (choice == 1 or (choice == 2 and n >= cap * WG_WAVES * 64 and bool(a["resumed"] or a["narrow"])))
        g = _grid(n, (64 if solo else 32) * WG_WAVES, cap)
        return dict(cap=cap, solo=int(solo), grid=g, draw=_draw(1024, 64 if solo else 32, g * WG_WAVES, 4, n))
    if kind == "walk":
        n = a["m"] * a["S"]
        cap = _cap(cus, walk_wgs, spare)
        g = _grid(n, 64 * WG_WAVES, cap)
        return dict(cap=cap, grid=g, draw=_draw(1024, 64, g * WG_WAVES, 4, n))
    if kind == "worklist":  # the grid by all it may hold, the draw by the implicit items alone
        implicit = a["m"] * 3 * (a["k"] - a["tn"])
        cap = _cap(cus, wave_wgs, spare)
        g = _grid((implicit + a["wl_cap"]) * a["S"], 64 * WG_WAVES, cap)
        return dict(cap=cap, grid=g, draw=_draw(1024, 64, g * WG_WAVES, 4, implicit * a["S"]))
    if kind == "extract":
        cap = _cap(cus, extract_wgs)
        g = _grid(a["total"], 64 * WG_WAVES, cap, a["S"])
        return dict(cap=cap, grid=g, draw=_draw(ROW_CHUNK, 1, g * WG_WAVES, 2, a["total"]))
    if kind == "locate":
        cap = _cap(cus, MIN_WGS)
        g = max(1, _grid(a["n"], 64 * WG_WAVES, cap, a["S"]))
        return dict(cap=cap, grid=g, draw=_draw(256, 64, max(1, g * WG_WAVES // a["S"]), 2, a["n"]))
    assert kind in ("branch", "kmer_reads"), kind
    return dict(grid=_grid(a["items"], 64 * WG_WAVES, _cap(cus, MIN_WGS)))


ENVIRONMENTS = [
    {},
    {"RSBWT_SEARCH_SPARE_WGS": "32"},
    {"RSBWT_SEARCH_SPARE_WGS": "600"},                                           # more than half the chip: not trimmed
    {"RSBWT_SEARCH_SPARE_WGS": "512"},                                           # exactly half: not trimmed either
    {"RSBWT_SEARCH_SPARE_WGS": "-5", "RSBWT_WAVE_WGS_PER_CU": "0", "RSBWT_WALK1MM_WGS_PER_CU": "4", "RSBWT_EXTRACT_WGS_PER_CU": "21",
     "RSBWT_SET_1MM_SIDE_LOG2": "9", "RSBWT_KMER_WIDE_ROWS": "0", "RSBWT_SEARCH_KERNEL": "both"},   # all out of range
    {"RSBWT_WAVE_WGS_PER_CU": "x", "RSBWT_WALK1MM_WGS_PER_CU": "", "RSBWT_EXTRACT_WGS_PER_CU": "-1", "RSBWT_SET_1MM_SIDE_LOG2": "41",
     "RSBWT_SET_1MM_TABLE_PREPASS": "no", "RSBWT_KMER_WIDE_ROWS": "-3", "RSBWT_NO_STAGED_RESULTS": ""},
    {"RSBWT_WAVE_WGS_PER_CU": "1", "RSBWT_WALK1MM_WGS_PER_CU": "1", "RSBWT_EXTRACT_WGS_PER_CU": "1", "RSBWT_SET_1MM_SIDE_LOG2": "10",
     "RSBWT_SET_1MM_TABLE_PREPASS": "0", "RSBWT_KMER_WIDE_ROWS": "1", "RSBWT_NO_STAGED_RESULTS": "1"},
    {"RSBWT_WAVE_WGS_PER_CU": "5", "RSBWT_WALK1MM_WGS_PER_CU": "3", "RSBWT_EXTRACT_WGS_PER_CU": "20", "RSBWT_SET_1MM_SIDE_LOG2": "40",
     "RSBWT_SET_1MM_TABLE_PREPASS": "1", "RSBWT_KMER_WIDE_ROWS": "1000000000000", "RSBWT_SEARCH_SPARE_WGS": "32"},
    {"RSBWT_WALK1MM_WGS_PER_CU": "2", "RSBWT_EXTRACT_WGS_PER_CU": "3", "RSBWT_SET_1MM_TABLE_PREPASS": "7"},
    {"RSBWT_SEARCH_KERNEL": "pair"},
    {"RSBWT_SEARCH_KERNEL": "solo", "RSBWT_SEARCH_SPARE_WGS": "32"},
]


@pytest.mark.parametrize("env", ENVIRONMENTS, ids=lambda e: ",".join(f"{k[6:]}={v}" for k, v in e.items()) or "unset")
def test_every_row_of_the_plan_follows_the_launchers_rules(plan_exe, env):
    rows = _run(plan_exe, env)
    kinds = {kind for kind, *_ in rows}
    assert kinds == {"knobs", "search", "walk", "worklist", "extract", "locate", "branch", "kmer_reads"} and len(rows) > 150
    for kind, name, given, planned in rows:
        assert planned == _expected(kind, given, env), (kind, name, given)


def _row(rows, kind, name, **given):
    hits = [p for k, n, g, p in rows if k == kind and n == name and all(g[x] == v for x, v in given.items())]
    assert len(hits) == 1, (kind, name, given)
    return hits[0]


def test_the_rows_worked_by_hand_at_256_cus(plan_exe):
    """256 CUs, 4 waves per workgroup, 4 workgroups per CU (the walk: 3) -- figures worked from the launchers by hand."""
    rows = _run(plan_exe, {})
    assert _row(rows, "search", "headline", cus=256) == dict(cap=1024, solo=1, grid=1024, draw=1024)
    assert _row(rows, "search", "window", cus=256) == dict(cap=1024, solo=0, grid=256, draw=32)       # 32,768 < 262,144; the pairs' floor
    assert _row(rows, "search", "threshold", cus=256) == dict(cap=1024, solo=1, grid=1024, draw=64)   # exactly 262,144; the lone lanes' floor
    assert _row(rows, "search", "below", cus=256)["solo"] == 0
    assert _row(rows, "search", "wide", cus=256)["solo"] == 0                                          # not narrow
    assert _row(rows, "search", "resumed", cus=256)["solo"] == 1
    assert _row(rows, "search", "one", cus=256) == dict(cap=1024, solo=0, grid=1, draw=32)
    assert _row(rows, "search", "table", cus=256)["solo"] == 0                                         # a table's own searches stay on pairs
    assert _row(rows, "walk", "slice", cus=256) == dict(cap=768, grid=768, draw=256)
    assert _row(rows, "worklist", "slice", cus=256) == dict(cap=1024, grid=1024, draw=1024)
    # extraction and locate: a launch that fills the chip, a service window's few hundred rows, one row
    assert _row(rows, "extract", "full", cus=256, S=1) == dict(cap=1024, grid=1024, draw=64)           # 128 x 4,096 waves x 2 > 1e6
    assert _row(rows, "extract", "full", cus=256, S=8) == dict(cap=1024, grid=1024, draw=256)
    assert _row(rows, "extract", "full", cus=256, S=3) == dict(cap=1024, grid=1023, draw=256)          # 1,024 - 1,024 % 3
    assert _row(rows, "extract", "window", cus=256, S=1) == dict(cap=1024, grid=1, draw=16)            # 242 rows: 16 x 4 waves x 2 <= 242
    assert _row(rows, "extract", "window", cus=256, total=300, S=8) == dict(cap=1024, grid=2, draw=16) # 2 < 8 workgroups: as they come
    assert _row(rows, "extract", "window", cus=256, total=1936) == dict(cap=1024, grid=8, draw=16)     # 8 = one per shard; 32 x 32 x 2 > 1,936
    assert _row(rows, "extract", "mid", cus=256, S=3) == dict(cap=1024, grid=195, draw=32)             # 196 - 196 % 3
    assert _row(rows, "extract", "one", cus=256, S=8) == dict(cap=1024, grid=1, draw=1)                # the floor
    assert _row(rows, "locate", "full", cus=256, S=1) == dict(cap=1024, grid=1024, draw=64)            # 4,096 waves on the one list
    assert _row(rows, "locate", "full", cus=256, S=8) == dict(cap=1024, grid=1024, draw=256)           # 512 waves per shard
    assert _row(rows, "locate", "window", cus=256, S=1) == dict(cap=1024, grid=1, draw=64)             # the floor
    assert _row(rows, "locate", "one", cus=0, S=8) == dict(cap=0, grid=1, draw=64)                     # never no workgroup at all
    assert _row(rows, "branch", "wg_and_one", cus=256) == dict(grid=2)


def test_the_spare_workgroups_come_off_the_search_launches_alone(plan_exe):
    rows = _run(plan_exe, {"RSBWT_SEARCH_SPARE_WGS": "32"})
    assert _row(rows, "search", "headline", cus=256) == dict(cap=992, solo=1, grid=992, draw=1024)
    assert _row(rows, "walk", "slice", cus=256)["cap"] == 736 and _row(rows, "worklist", "slice", cus=256)["cap"] == 992
    assert _row(rows, "extract", "full", cus=256, S=8)["cap"] == _row(rows, "locate", "full", cus=256, S=8)["cap"] == 1024
    assert _row(rows, "branch", "full", cus=256) == _row(rows, "kmer_reads", "full", cus=256) == dict(grid=1024)
    assert _row(rows, "search", "one", cus=1)["cap"] == 4                                              # 4 <= 2 x 32: not trimmed
    rows = _run(plan_exe, {"RSBWT_SEARCH_SPARE_WGS": "600"})
    assert _row(rows, "search", "headline", cus=256)["cap"] == 1024                                    # 2 x 600 > 1,024: not trimmed
