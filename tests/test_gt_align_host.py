"""The boundary of the SiteMatch alignment calls without a GPU: the header, the ctypes binding, and the null, length and
parameter rules (RSBWT_EINVAL / RSBWT_ERANGE), all of which are decided before a device is touched."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = {"rsbwt_ksw_align": 8, "rsbwt_ksw_align_dev": 9, "rsbwt_gt_align": 12, "rsbwt_gt_align_dev": 13, "rsbwt_set_gt_aligned_reads": 17,
         "rsbwt_set_gt_aligned_count": 11, "rsbwt_gt_align_last_work": 1}
EINVAL, ERANGE = -1, -7
CODES = ["ALT_NOT_BETTER", "REF_WORSE", "OFF_SITE", "UNALIGNED", "FLOOR_PLAIN", "FLOOR_INS", "FLOOR_DEL", "SITE_MISMATCH", "KEEP_PLAIN", "RIGHT_QB",
         "KEEP_RIGHT", "LEFT_QE", "KEEP_LEFT"]


def p(a):
    return a.ctypes.data_as(C.c_void_p)


def texts(seqs):
    off = np.zeros(len(seqs) + 1, np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs], dtype=np.uint64)
    return np.frombuffer(("".join(seqs) + "\0").encode(), np.uint8).copy(), off


def test_header_declares_and_native_binds_the_entry_points(rsb):
    from readserver_amd import _native
    raw = open(os.path.join(ROOT, "include", "rsbwt.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    L = C.CDLL(rsb.lib_path())
    for n, nargs in ENTRY.items():
        assert re.search(r"\b%s\s*\(" % n, txt), f"{n} is not declared in include/rsbwt.h"
        assert n in _native.SIGNATURES and hasattr(L, n) and hasattr(rsb.lib(), n)
        assert len(_native.SIGNATURES[n][1]) == nargs, n
    for v, name in enumerate(CODES, 1):  # thirteen codes, one per exit of align_gt_read, in source order
        assert re.search(r"#define RSBWT_GT_%s %d\b" % (name, v), txt), name
    assert re.search(r"#define RSBWT_KSW_LDS_ROWS %d\b" % rsb.bwt.KSW_LDS_ROWS, txt) and re.search(r"#define RSBWT_KSW_MAX_LEN 4096\b", txt)
    assert re.search(r"int32_t match, mismatch, ambiguous, gapo, gape;", txt) and re.search(r"int32_t score, te, qe, tb, qb, reserved;", txt)
    for word in ("(a)", "(b)", "(c)", "alt[0]", "RSBWT_GT_OFF_SITE for every read"):  # the divergences are stated where the calls are
        assert word in raw
    assert callable(rsb.ksw_align) and callable(rsb.gt_align) and callable(rsb.ShardSet.gt_aligned_reads) and callable(rsb.ShardSet.gt_aligned_count)
    assert rsb.bwt.GT_KEEP == (9, 11, 13)
    # the candidate calls keep their signatures
    assert len(_native.SIGNATURES["rsbwt_set_gt_reads"][1]) == 15 and len(_native.SIGNATURES["rsbwt_set_gt_count"][1]) == 9


def test_ksw_align_argument_rules(rsb):
    L = rsb.lib()
    qt, qo = texts(["ACGT", "ACGTACGT"])
    tt, to = texts(["ACGTT", "TTACGTACGTAA"])
    out = np.full((2, 6), 77, np.int32)
    assert L.rsbwt_ksw_align(0, None, None, None, None, None, 0, None) == 0          # n = 0 touches nothing
    assert L.rsbwt_ksw_align_dev(None, None, None, None, None, 0, None, 0, None) == 0
    assert L.rsbwt_ksw_align(0, None, None, p(qo), p(tt), p(to), 2, p(out)) == EINVAL and b"null" in L.rsbwt_last_error()
    assert L.rsbwt_ksw_align(0, None, p(qt), p(qo), p(tt), p(to), 2, None) == EINVAL
    assert L.rsbwt_ksw_align_dev(None, None, p(qo), p(tt), p(to), 2, p(out), 0, None) == EINVAL
    for bad in ((0, 4, 1, 6, 1), (1, 128, 1, 6, 1), (1, 4, -1, 6, 1), (1, 4, 1, 0, 1), (1, 4, 1, 6, 128)):
        prm = np.array(bad, np.int32)
        assert L.rsbwt_ksw_align(0, p(prm), p(qt), p(qo), p(tt), p(to), 2, p(out)) == EINVAL, bad
        assert b"1 to 127" in L.rsbwt_last_error()
        assert L.rsbwt_ksw_align(0, p(prm), None, None, None, None, 0, None) == EINVAL    # (even with nothing to align)
        assert L.rsbwt_ksw_align_dev(p(prm), p(qt), p(qo), p(tt), p(to), 2, p(out), 0, None) == EINVAL
    # lengths: 1..4096 on either side
    empty_q = np.array([0, 0, 8], np.uint64)
    assert L.rsbwt_ksw_align(0, None, p(qt), p(empty_q), p(tt), p(to), 2, p(out)) == EINVAL and b"query 0" in L.rsbwt_last_error()
    backwards = np.array([0, 9, 5], np.uint64)
    assert L.rsbwt_ksw_align(0, None, p(qt), p(qo), p(tt), p(backwards), 2, p(out)) == EINVAL and b"target 1" in L.rsbwt_last_error()
    big = np.frombuffer(b"A" * 4097 + b"\0", np.uint8).copy()
    long_off = np.array([0, 4097], np.uint64)
    one_off = np.array([0, 4], np.uint64)
    assert L.rsbwt_ksw_align(0, None, p(big), p(long_off), p(tt), p(one_off), 1, p(out)) == EINVAL
    assert L.rsbwt_ksw_align(0, None, p(qt), p(one_off), p(big), p(long_off), 1, p(out)) == EINVAL
    # where the reference's 16-bit lanes saturate: match x min(qlen, tlen) >= 2^15
    prm = np.array((127, 4, 1, 6, 1), np.int32)
    off259 = np.array([0, 259], np.uint64)
    assert L.rsbwt_ksw_align(0, p(prm), p(big), p(off259), p(big), p(off259), 1, p(out)) == ERANGE and b"2^15" in L.rsbwt_last_error()
    assert (out == 77).all()


def test_gt_align_argument_rules(rsb):
    L = rsb.lib()
    rt, ro = texts(["ACGTACGTAC", "ACGTACGTACGT"])
    wt, wo = texts(["TTACGTACGTACGTAA"])
    item, pos = np.array([0, 0], np.uint64), np.array([5], np.uint64)
    alt, isalt = np.frombuffer(b"G", np.uint8).copy(), np.array([1], np.uint8)
    v = np.full(2, 77, np.uint8)
    w = (C.c_uint64 * 14)(*([9] * 14))
    L.rsbwt_gt_align_last_work(None)  # (nothing to write to: no crash)
    assert L.rsbwt_gt_align(0, None, None, None, 0, None, None, None, None, None, 0, None) == 0
    assert L.rsbwt_gt_align_dev(None, None, None, 0, None, None, None, None, None, 0, None, 0, None) == 0
    L.rsbwt_gt_align_last_work(w)
    assert list(w) == [0] * 14
    args = [p(rt), p(ro), p(item), 2, p(wt), p(wo), p(pos), p(alt), p(isalt), 1, p(v)]
    for k in (0, 1, 2, 4, 5, 6, 7, 8, 10):
        a = list(args)
        a[k] = None
        assert L.rsbwt_gt_align(0, *a) == EINVAL and b"null" in L.rsbwt_last_error(), k
        assert L.rsbwt_gt_align_dev(*a, 0, None) == EINVAL, k
    bad_item = np.array([0, 1], np.uint64)
    a = list(args)
    a[2] = p(bad_item)
    assert L.rsbwt_gt_align(0, *a) == EINVAL and b"request 1 of 1" in L.rsbwt_last_error()
    a = list(args)
    a[1] = p(np.array([0, 10, 10], np.uint64))  # an empty read
    assert L.rsbwt_gt_align(0, *a) == EINVAL and b"read 1" in L.rsbwt_last_error()
    big = np.frombuffer(b"A" * 4097 + b"\0", np.uint8).copy()
    a = list(args)
    a[4], a[5] = p(big), p(np.array([0, 4097], np.uint64))  # divergence (c): a window outside 1..4096
    assert L.rsbwt_gt_align(0, *a) == EINVAL and b"request 0" in L.rsbwt_last_error()
    a = list(args)
    a[0], a[1], a[3] = p(big), p(np.array([0, 4097], np.uint64)), 1
    assert L.rsbwt_gt_align(0, *a) == EINVAL
    L.rsbwt_gt_align_last_work(w)
    assert list(w) == [0] * 14 and (v == 77).all()  # the failed calls did no work


def test_set_calls_refuse_null(rsb):
    L = rsb.lib()
    t, off = texts(["ACGTACGT"])
    pos, alt, isalt = np.array([3], np.uint64), np.frombuffer(b"G", np.uint8).copy(), np.array([0], np.uint8)
    first, n = np.zeros(2, np.uint64), C.c_size_t(77)
    assert L.rsbwt_set_gt_aligned_reads(None, p(t), p(off), 1, p(pos), p(alt), p(isalt), 4, 0, 0, p(first), None, 256, None, None, 0, C.byref(n)) == EINVAL
    assert b"null" in L.rsbwt_last_error() and n.value == 0
    assert L.rsbwt_set_gt_aligned_reads(None, p(t), p(off), 1, p(pos), p(alt), p(isalt), 4, 0, 0, p(first), None, 256, None, None, 0, None) == EINVAL
    assert L.rsbwt_set_gt_aligned_reads(None, p(t), p(off), 1, p(pos), p(alt), p(isalt), 4, 0, 0, p(first), None, 0, None, None, 0, C.byref(n)) == EINVAL
    assert L.rsbwt_set_gt_aligned_count(None, p(t), p(off), 1, p(pos), p(alt), p(isalt), 4, 0, 0, None) == EINVAL
    assert L.rsbwt_set_gt_aligned_count(None, p(t), p(off), 1, p(pos), None, p(isalt), 4, 0, 0, p(first)) == EINVAL
