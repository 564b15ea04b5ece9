"""The alignment restatement (tests/ksw_reference.py) against outputs recorded from the reference's own ksw.c
(tests/golden/ksw_v1.npz, made by tests/golden/make_ksw_golden.py), the verdict batch the GPU tests reuse, and the lane's
walk of the kernel (csrc/ksw_pass.h) compiled for the host with the sanitizers on -- no GPU anywhere."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import ksw_reference as kr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QLENS = (1, 7, 8, 9, 16, 17, 63, 64, 65, 100, 255, 256, 257)


@pytest.fixture(scope="module")
def golden(golden_dir):
    return kr.load_golden(golden_dir)


def test_the_fixture_has_every_class(golden):
    pairs, sets, classes, mask = golden
    assert sets[0][0] == kr.SERVICE and sets[1][0] == kr.OTHER
    want = ["qe_tie"] + [f"qlen_{n}" for n in QLENS] + ["tlen_1", "score_0", "n_in_target", "n_in_query", "insertion", "deletion", "block_7",
                                                        "read_longer"]
    assert classes == want
    for b, c in enumerate(classes):
        assert int(((mask >> b) & 1).sum()) >= 20, c
    for n in QLENS:
        assert sum(len(q) == n for q, _ in pairs) >= 20
    assert sum(len(t) == 1 for _, t in pairs) >= 20 and sum(len(q) > len(t) for q, t in pairs) >= 20
    assert int((sets[0][1][:, 0] == 0).sum()) >= 20
    assert all((res[:, 3:] >= 0).all() for _, res in sets), "tb / qb are never left at -1"


def test_restatement_equals_every_record(golden):
    pairs, sets, _, _ = golden
    for params, res in sets:
        for i, (q, t) in enumerate(pairs):
            assert kr.ksw_align(kr.code(q), kr.code(t), params) == tuple(int(x) for x in res[i]), (i, params)


def test_cell_by_cell_definition_equals_the_records(golden):
    """pass_scalar is the definition as the documents state it; the column-at-a-time pass_np is what the other tests run"""
    pairs, sets, classes, mask = golden
    tie = np.flatnonzero(mask & 1)[:8]
    short = [i for i, (q, t) in enumerate(pairs) if len(q) * len(t) <= 3000][::5][:40]
    for params, res in sets:
        for i in list(tie) + short:
            q, t = pairs[i]
            assert kr.ksw_align(kr.code(q), kr.code(t), params, scalar=True) == tuple(int(x) for x in res[i]), (i, params)


def test_the_tie_records_pin_the_striped_order(golden):
    pairs, sets, _, mask = golden
    for params, res in sets:
        for i in np.flatnonzero(mask & 1):
            q, t = pairs[i]
            assert kr.ksw_align(kr.code(q), kr.code(t), params, tie="row") != tuple(int(x) for x in res[i])


def test_verdict_batch_reaches_every_exit():
    reads, item, requests, codes, C = kr.verdicts()
    assert len(reads) == len(item) == len(codes) and set(codes) <= set(range(1, 14))
    missed = {c: C[c] for c in range(1, 14) if C[c] < 10}
    assert not missed, f"exits reached fewer than 10 times: {missed} ({ {c: kr.GT_LABELS[c] for c in missed} })"
    assert sum(C.values()) == len(reads)


def test_divergences_of_align_gt_read():
    w = "ACGTTGCAAGGCTTACCGATACGATTAGGC"
    assert kr.align_gt_read(w[5:25], w, 0, "A", False) == 3 and kr.align_gt_read(w[5:25], w, len(w) + 1, "A", True) == 3
    # alt is coded like every other symbol: a lower-case alt is the same request
    for alt in "acgtn":
        for isalt in (False, True):
            assert kr.align_gt_read(w[5:25], w, 12, alt, isalt) == kr.align_gt_read(w[5:25], w, 12, alt.upper(), isalt)


def _host_walk(golden, tmp_path, name, flags):
    """tests/native/ksw_pass_host.cpp built with `flags` and run over every golden record (a column of exactly the kernel's
    size, at two strides) and the verdict batch: (its answer lines, the expected ones, how many of them are golden records)"""
    pairs, sets, _, _ = golden
    exe, inp = str(tmp_path / name), str(tmp_path / (name + ".txt"))
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", *flags, f"-I{os.path.join(ROOT, 'readserver_amd', 'csrc')}",
                        os.path.join(ROOT, "tests", "native", "ksw_pass_host.cpp"), "-o", exe], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    reads, item, requests, codes, _ = kr.verdicts()
    want = []
    with open(inp, "w") as f:
        for params, res in sets:
            for i, (q, t) in enumerate(pairs):
                f.write("K %d %d %d %d %d %d %s %s\n" % (*params, (64, 3)[i % 2], q.decode("latin-1"), t.decode("latin-1")))
                want.append(" ".join(str(int(x)) for x in res[i]))
        for s, r, c in zip(reads, item, codes):
            w, pos, alt, isalt = requests[r]
            f.write("G %d %s %s %d %s %d\n" % ((64, 5)[r % 2], s, w, pos, alt, isalt))
            want.append(str(c))
    r = subprocess.run([exe, inp], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    got = r.stdout.split("\n")[:-1]
    assert len(got) == len(want)
    return got, want, 2 * len(pairs)


def test_lane_walk_on_the_host(golden, tmp_path):
    """csrc/ksw_pass.h -- the code every lane of ksw_align.hip runs -- built with g++ and the address / undefined-behaviour
    sanitizers: every golden record and every verdict of the batch"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    got, want, _ = _host_walk(golden, tmp_path, "ksw_pass_host", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    bad = [i for i in range(len(want)) if got[i] != want[i]]
    assert not bad, f"{len(bad)} of {len(want)} records differ, first {bad[0]}: got {got[bad[0]]}, want {want[bad[0]]}"


def test_lane_walk_mutations_on_the_host(golden, tmp_path):
    """the two one-line variants of DESIGN 8k.  Ties broken by the smallest row: every record of the qe_tie class differs, for
    both parameter sets.  The reversed pass over te + 1 columns instead of tlen: NOTHING differs -- the reversed pass always
    stops at a column <= te, where it reaches the forward score, so the columns after te are never walked; the variant is
    the same function, which is why no test here or on the GPU can tell it apart"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    pairs, _, _, mask = golden
    got, want, nk = _host_walk(golden, tmp_path, "tie_row", ["-DRSB_MUTATE_KSW_TIE_ROW"])
    bad = {i for i in range(nk) if got[i] != want[i]}
    for i in np.flatnonzero(mask & 1):
        assert int(i) in bad and int(i) + len(pairs) in bad, i
    got, want, _ = _host_walk(golden, tmp_path, "rev_columns", ["-DRSB_MUTATE_KSW_REV_COLUMNS"])
    assert got == want
