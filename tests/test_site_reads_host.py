"""rsbwt_set_site_reads / rsbwt_set_site_read_counts / rsbwt_set_site_reads_last_work without a GPU: the symbols are bound
with the composed calls' argument lists, the Python side has the methods, and what the calls refuse before they touch a
device -- a null set, a null nreads, a zero stride, null counts -- is RSBWT_EINVAL with the counters left zero.  The answers
are tests/test_gpu_site_reads.py's business."""
import ctypes as C

import numpy as np

EINVAL = -1


def test_site_reads_symbols_take_the_composed_calls_arguments(rsb):
    L = rsb.lib()
    for new, old in (("rsbwt_set_site_reads", "rsbwt_set_gt_aligned_reads"), ("rsbwt_set_site_read_counts", "rsbwt_set_gt_aligned_count")):
        f, g = getattr(L, new), getattr(L, old)
        assert f.restype is g.restype and list(f.argtypes) == list(g.argtypes), new
    assert L.rsbwt_set_site_reads_last_work.restype is None
    for name in ("site_reads", "site_read_counts", "site_reads_last_work"):
        assert callable(getattr(rsb.ShardSet, name))


def test_site_reads_refuse_before_any_device(rsb):
    L = rsb.lib()
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    t = np.frombuffer(b"ACGTACGTAC", np.uint8).copy()
    off, pos = np.array([0, 10], np.uint64), np.array([5], np.uint64)
    alt, isalt = np.frombuffer(b"A", np.uint8).copy(), np.zeros(1, np.uint8)
    first, n = np.full(2, 7, np.uint64), C.c_size_t(99)
    args = (p(t), p(off), 1, p(pos), p(alt), p(isalt), 4, 0, 0)
    assert L.rsbwt_set_site_reads(None, *args, p(first), None, 256, None, None, 0, C.byref(n)) == EINVAL and n.value == 0
    assert b"null set" in L.rsbwt_last_error()
    assert L.rsbwt_set_site_reads(None, *args, p(first), None, 256, None, None, 0, None) == EINVAL
    assert L.rsbwt_set_site_reads(None, *args, p(first), None, 0, None, None, 0, C.byref(n)) == EINVAL and b"stride" in L.rsbwt_last_error()
    assert L.rsbwt_set_site_reads(None, *args, None, None, 256, None, None, 0, C.byref(n)) == EINVAL
    assert L.rsbwt_set_site_read_counts(None, *args, None) == EINVAL
    assert L.rsbwt_set_site_read_counts(None, *args, p(first)) == EINVAL and b"null set" in L.rsbwt_last_error()
    w = np.full(9, 5, np.uint64)
    L.rsbwt_set_site_reads_last_work(None)
    L.rsbwt_set_site_reads_last_work(w.ctypes.data_as(C.POINTER(C.c_uint64)))
    assert not w.any()
    assert rsb.ShardSet.site_reads_last_work() == dict.fromkeys(
        ("legs", "narrow_steps", "candidates", "kept", "extracted", "classes", "aligned", "items_kept", "reported"), 0)
