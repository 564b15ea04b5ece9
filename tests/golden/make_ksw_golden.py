#!/usr/bin/env python3
"""Generates tests/golden/ksw_v1.npz from the REAL reference: the five fields score, te, qe, tb, qb that the reference's
own src/service/ksw.c returns for ksw_align(qlen, q, tlen, t, 5, mat, gapo, gape, KSW_XSTART, 0) -- the call of
align_gt_read (src/service/service.cpp:134) -- on seeded pairs, for the service's scores (1, 4, 1, 6, 1) and for
(2, 3, 1, 5, 2).

Runs only where the reference's sources are (RSBWT_REFERENCE, default /root/reference).  ksw.c is compiled into a
temporary directory that is removed again; only inputs and expected outputs are stored.  The generator fails unless
every class of CLASSES has at least 20 pairs, and unless tests/ksw_reference.py agrees with every record."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ksw_reference as kr  # noqa: E402

REF = os.environ.get("RSBWT_REFERENCE", "/root/reference")
QLENS = (1, 7, 8, 9, 16, 17, 63, 64, 65, 100, 255, 256, 257)
CLASSES = ["qe_tie"] + [f"qlen_{n}" for n in QLENS] + ["tlen_1", "score_0", "n_in_target", "n_in_query", "insertion", "deletion",
                                                         "block_7", "read_longer"]
KSW_XSTART = 0x80000


class KswR(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("score", "te", "qe", "score2", "te2", "tb", "qb")]


def compile_ksw(tmp):
    so = os.path.join(tmp, "libksw_ref.so")
    subprocess.check_call(["gcc", "-O2", "-shared", "-fPIC", "-msse2", f"-I{os.path.join(REF, 'include', 'service')}",
                           os.path.join(REF, "src", "service", "ksw.c"), "-o", so])
    L = C.CDLL(so)
    L.ksw_align.restype = KswR
    L.ksw_align.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    return L


def ref_align(L, q, t, params):
    a, b, n, gapo, gape = params
    mat = np.full((5, 5), -n, np.int8)
    for i in range(4):
        for j in range(4):
            mat[i, j] = a if i == j else -b
    qc, tc = kr.code(q).astype(np.uint8), kr.code(t).astype(np.uint8)
    r = L.ksw_align(len(qc), qc.ctypes.data, len(tc), tc.ctypes.data, 5, mat.ctypes.data, gapo, gape, KSW_XSTART, None)
    return (r.score, r.te, r.qe, r.tb, r.qb)


def main():
    rng = np.random.default_rng(20261020)
    rnd = lambda n, ab="ACGT": "".join(ab[c] for c in rng.integers(0, len(ab), n))  # noqa: E731

    def mutate(s, subs):
        s = list(s)
        for _ in range(subs):
            p = int(rng.integers(len(s)))
            s[p] = "ACGT"[(("ACGT".find(s[p]) if s[p] in "ACGT" else 0) + int(rng.integers(1, 4))) % 4]
        return "".join(s)

    pairs = []  # (q, t, {classes})

    def derived(qlen, tlen=None):
        """a read cut from a target (or the target from the read when the read is the longer one), a few substitutions"""
        tlen = tlen if tlen is not None else int(rng.integers(max(1, min(qlen, 199) // 2), 200))
        if qlen <= tlen:
            t = rnd(tlen)
            a = int(rng.integers(0, tlen - qlen + 1))
            return mutate(t[a:a + qlen], int(rng.integers(0, 4))), t
        q = rnd(qlen)
        a = int(rng.integers(0, qlen - tlen + 1))
        return q, mutate(q[a:a + tlen], int(rng.integers(0, 4)))
    for n in QLENS:
        for i in range(22):
            q, t = derived(n) if i % 4 else (rnd(n), rnd(int(rng.integers(1, 200))))
            pairs.append((q, t, {f"qlen_{n}"}))
    for _ in range(24):
        pairs.append((rnd(int(rng.integers(1, 120))), rnd(1), {"tlen_1"}))
    for _ in range(12):
        pairs.append(("A" * int(rng.integers(1, 90)), rnd(int(rng.integers(1, 199)), "CGT"), {"score_0"}))
        pairs.append((rnd(int(rng.integers(1, 90))), "N" * int(rng.integers(1, 199)), {"score_0", "n_in_target"}))
    for _ in range(24):
        q, t = derived(int(rng.integers(30, 120)), 199)
        t = list(t)
        for p in rng.integers(0, 199, int(rng.integers(1, 6))):
            t[p] = "Nnx-"[int(rng.integers(4))]
        pairs.append((q, "".join(t), {"n_in_target"}))
        q, t = derived(int(rng.integers(30, 120)), 199)
        q = list(q)
        for p in rng.integers(0, len(q), int(rng.integers(1, 5))):
            q[p] = "NnR*"[int(rng.integers(4))]
        pairs.append(("".join(q), t, {"n_in_query"}))
    for _ in range(26):
        t = rnd(199)
        a, n = int(rng.integers(0, 90)), int(rng.integers(60, 101))
        r, p, g = t[a:a + n], int(rng.integers(10, 50)), int(rng.integers(1, 13))
        pairs.append((mutate(r[:p] + rnd(g) + r[p:], int(rng.integers(0, 3))), t, {"insertion"}))
        pairs.append((mutate(r[:p] + r[p + g:], int(rng.integers(0, 3))), t, {"deletion"}))
        b = int(rng.integers(7, 15))
        pairs.append((r[:p] + mutate(r[p:p + b], b) + r[p + b:], t, {"block_7"}))
        pairs.append((rnd(int(rng.integers(3, 30)), "ac") + r.lower() + rnd(int(rng.integers(3, 30)), "AC"), t[a:a + n], {"read_longer"}))
    for _ in range(30):  # a 2-letter alphabet, and unrelated pairs
        pairs.append((rnd(int(rng.integers(2, 150)), "AC"), rnd(int(rng.integers(2, 200)), "AC"), set()))
        pairs.append((rnd(int(rng.integers(2, 150))), rnd(int(rng.integers(2, 200))), set()))
    # a qe tie the striped order and the smallest-row order decide differently: the target's piece occurs twice in the read
    want, tries = 28, 0
    while want and tries < 20000:
        tries += 1
        x = rnd(int(rng.integers(4, 24)))
        q = rnd(int(rng.integers(0, 12))) + x + rnd(int(rng.integers(1, 40))) + x + rnd(int(rng.integers(0, 12)))
        t = rnd(int(rng.integers(0, 30))) + x + rnd(int(rng.integers(0, 30)))
        differ = [kr.ksw_align(kr.code(q), kr.code(t), p) != kr.ksw_align(kr.code(q), kr.code(t), p, tie="row") for p in (kr.SERVICE, kr.OTHER)]
        if all(differ):
            pairs.append((q, t, {"qe_tie"}))
            want -= 1
    assert want == 0, "could not make the qe ties"

    with tempfile.TemporaryDirectory() as tmp:
        L = compile_ksw(tmp)
        res = {p: np.array([ref_align(L, q, t, p) for q, t, _ in pairs], np.int32) for p in (kr.SERVICE, kr.OTHER)}
        del L
    mask = np.zeros(len(pairs), np.uint32)
    for i, (q, t, cls) in enumerate(pairs):
        if len(q) > len(t):
            cls = cls | {"read_longer"}
        if res[kr.SERVICE][i][0] == 0:
            cls = cls | {"score_0"}
        for c in cls:
            mask[i] |= 1 << CLASSES.index(c)
    for b, c in enumerate(CLASSES):
        n = int(((mask >> b) & 1).sum())
        assert n >= 20, f"class {c}: {n} pairs"
    for i in np.flatnonzero(mask & 1):  # the recorded qe IS the striped order's, not the smallest row's
        q, t = kr.code(pairs[i][0]), kr.code(pairs[i][1])
        for p in (kr.SERVICE, kr.OTHER):
            assert tuple(res[p][i]) != kr.ksw_align(q, t, p, tie="row")
    bad = 0
    for i, (q, t, _) in enumerate(pairs):
        for p in (kr.SERVICE, kr.OTHER):
            bad += tuple(res[p][i]) != kr.ksw_align(kr.code(q), kr.code(t), p)
    assert bad == 0, f"tests/ksw_reference.py differs from ksw.c on {bad} records"
    assert (res[kr.SERVICE][:, 3:] >= 0).all() and (res[kr.OTHER][:, 3:] >= 0).all(), "tb / qb left at -1"
    qtext = "".join(q for q, _, _ in pairs).encode("latin-1")
    ttext = "".join(t for _, t, _ in pairs).encode("latin-1")
    out = os.path.join(HERE, "ksw_v1.npz")
    np.savez_compressed(out, qtext=np.frombuffer(qtext, np.uint8), ttext=np.frombuffer(ttext, np.uint8),
                        qoff=np.cumsum([0] + [len(q) for q, _, _ in pairs]).astype(np.uint64),
                        toff=np.cumsum([0] + [len(t) for _, t, _ in pairs]).astype(np.uint64),
                        service=res[kr.SERVICE], other=res[kr.OTHER], params_service=np.array(kr.SERVICE, np.int32),
                        params_other=np.array(kr.OTHER, np.int32), classes=np.array(CLASSES), mask=mask)
    print(f"{out}: {len(pairs)} pairs, {os.path.getsize(out)} bytes")
    assert os.path.getsize(out) < 400_000


if __name__ == "__main__":
    main()
