"""The SiteMatch window fix-up and Reply code of csrc/service_slice.cpp without a GPU: tests/native/site_window_host.cpp
links it against a stub engine that returns canned reads, is built with -fsanitize=address,undefined and run as a program
of its own.  The fix-up is walked over every (|q|, p, strand) for |q| <= 2L + 3 at L = 5, negative and oversized p
included, against the plain restatement below (GtTask::run, service.cpp:1028-1046, in signed arithmetic); the Replies of
every return type, per partition and joined, against bytes the protobuf runtime makes."""
import os
import shutil
import subprocess

import pytest

import meta_proto
import proto_schema

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = 5
PARTS = 3
SEQ = "ACGTTGCAAGCTCAGGTACCATG"
_RC = str.maketrans("ACGT", "TGCA")


def rc(s):
    return s[::-1].translate(_RC)


def fixup(q, p, a, strand):
    query, pos, alt = (rc(q), len(q) - p + 1, rc(a)) if strand else (q, p, a)
    if pos < 0:
        return None
    if pos <= L:
        w = query[:max(L + pos - 1, 0)]
    else:
        if pos - L > len(query):
            return None
        w, pos = query[pos - L:pos + L - 1], L
    return None if pos > len(w) else (w, pos, alt)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    out = str(tmp_path_factory.mktemp("site_window") / "site_window_host")
    csrc = os.path.join(ROOT, "readserver_amd", "csrc")
    srcs = [os.path.join(ROOT, "tests", "native", "site_window_host.cpp"), os.path.join(csrc, "service_slice.cpp"), os.path.join(csrc, "service_loop.cpp")]
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", f"-I{os.path.join(ROOT, 'include')}",
                        f"-I{csrc}", *srcs, "-ldl", "-lpthread", "-o", out], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    return out


def _run(exe, *args):
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-300:], r.stderr[-2000:])
    return r.stdout.splitlines()


def test_site_window_fixup_over_every_length_position_and_strand(exe):
    lines = _run(exe, "fixup", str(L))
    want, kinds = [], set()
    for n in range(2 * L + 4):
        for p in range(-3, n + L + 3):
            for strand in (0, 1):
                f = fixup(SEQ[:n], p, "AG", strand)
                want.append(f"{n} {p} {strand} header" if f is None else f"{n} {p} {strand} ok {f[0]} {f[1]} {f[2]}")
                pos = n - p + 1 if strand else p
                kinds.add((f is None, pos < 0, 0 <= pos <= L, pos > L and pos - L > n))
    assert lines == want, next((a, b) for a, b in zip(lines + [None], want + [None]) if a != b)
    # the walk reaches: pos < 0, a start past the end, pos > |w| on either branch, and kept windows on either branch
    # (kinds: header-only?, pos < 0, the first branch, a start past the end)
    assert {(True, True, False, False), (True, False, False, True), (True, False, True, False), (True, False, False, False), (False, False, True, False),
            (False, False, False, False)} <= kinds, kinds
    assert max(len(x.split()[4]) for x in want if " ok " in x and len(x.split()) == 7) == 2 * L - 1


def _requests():
    q = SEQ[:2 * L + 3]
    rq = []
    for rt in (1, 2, 3, 4):
        rq += [(4, rt, q, 3, 0, L + 2, "G", 0), (4, rt, q, 3, 0, 2, "GT", 1), (4, rt, q, 4, 1, len(q) + 1, "C", 0), (4, rt, q, 4, 1, 3, "", 0),
               (4, rt, q[:3], 3, 0, 4, "T", 2)]
    return rq + [(2, 2, q, 0, 0, 0, "", 0), (4, 1, q, 9, 9, 1, "A", 0)]


@pytest.mark.parametrize("per_partition", [1, 0], ids=["per-partition", "joined"])
def test_site_window_replies_of_every_return_type(exe, per_partition):
    Request, ReplyR = proto_schema.build()
    Reply, _, _ = meta_proto.build()
    rq = _requests()
    strands = {(i, s): fixup(r[2], r[5], r[6], s) for i, r in enumerate(rq) if r[0] == 4 for s in (0, 1)}
    groups = {}
    for (i, s), f in sorted(strands.items()):
        if f is not None and f[2]:
            groups.setdefault((rq[i][3], rq[i][4]), []).append((i, s))
    cells = {}
    for members in groups.values():
        for j, (i, s) in enumerate(members):
            w, _, alt = strands[(i, s)]
            cells[(i, s)] = [[w + alt[0] + chr(65 + p) * (r + 1) for r in range((j + p) % 3)] for p in range(PARTS)]
    want = []
    for i, (t, rt, q, k, sk, p, a, isalt) in enumerate(rq):
        if t != 4:
            continue
        for row in (range(PARTS) if per_partition else [None]):
            for s in (0, 1):
                m = ReplyR()
                m.rt, m.t, m.q = 4, rt, q
                if strands[(i, s)] is None:
                    want.append(m.SerializeToString().hex())
                    continue
                c = cells.get((i, s), [[]] * PARTS)
                reads = c[row] if per_partition else [x for part in c for x in part]
                side = "revcomp_matches" if s else "forward_matches"
                if rt == 1:
                    getattr(m.c, side).c = len(reads)
                elif rt == 2:
                    m.r.SetInParent()
                    for x in reads:
                        getattr(m.r, side).add().r = x
                else:
                    want.append(meta_proto.all_reply(Reply, 4, rt, q, s == 1, reads, [b"ab!#cd$%" if len(x) % 2 else b"" for x in reads], {}, 2, True).hex())
                    continue
                want.append(m.SerializeToString().hex())
    lines = _run(exe, "replies", str(L), str(per_partition))
    assert lines[-1] == "calls 2 1", lines[-1]  # one call per distinct (k, s); the group whose requests all ask for Count counts
    assert lines[:-1] == want, next((n, a, b) for n, (a, b) in enumerate(zip(lines[:-1] + [None], want + [None])) if a != b)
    assert sorted(groups) == [(3, 0), (4, 1), (9, 9)] and len({len(x) for x in want}) > 6  # (reads and records are there: the Replies differ in length)
