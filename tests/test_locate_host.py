"""The boundary of the locate calls (csrc/locate.hip, csrc/sets.hip) without a GPU: the header, the ctypes binding, the
null-argument rules, and that a box without a GPU says RSBWT_ENODEV instead of answering from the CPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = {"rsbwt_locate": 7, "rsbwt_locate_dev": 8, "rsbwt_set_locate": 8, "rsbwt_set_locate_dev": 9, "rsbwt_set_locate_var_capped": 15,
         "rsbwt_locate_last_work": 1}
OK, EINVAL, ENODEV = 0, -1, -5


def test_header_declares_and_native_binds_the_entry_points(rsb):
    from readserver_amd import _native
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rsbwt.h")).read(), flags=re.S)
    L = C.CDLL(rsb.lib_path())
    for n, nargs in ENTRY.items():
        assert re.search(r"\b%s\s*\(" % n, txt), f"{n} is not declared in include/rsbwt.h"
        assert n in _native.SIGNATURES and hasattr(L, n) and hasattr(rsb.lib(), n)
        assert len(_native.SIGNATURES[n][1]) == nargs, n
    assert callable(rsb.GpuBWT.locate) and callable(rsb.ShardSet.locate) and callable(rsb.ShardSet.locate_queries)
    # the calls beside them keep their signatures
    assert len(_native.SIGNATURES["rsbwt_set_query_var_capped"][1]) == 13 and len(_native.SIGNATURES["rsbwt_extract"][1]) == 7


def test_null_arguments_and_empty_batches(rsb):
    L = rsb.lib()
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    rows = np.arange(4, dtype=np.uint64)
    sh = np.zeros(4, np.uint32)
    o64, o32 = np.zeros(4, np.uint64), np.zeros(4, np.uint32)
    assert L.rsbwt_strerror(EINVAL)
    # a null handle / set, with and without rows
    assert L.rsbwt_locate(None, p(rows), 4, 0, p(o64), None, None) == EINVAL and b"null" in L.rsbwt_last_error()
    assert L.rsbwt_locate(None, None, 0, 0, p(o64), None, None) == EINVAL
    assert L.rsbwt_locate_dev(None, p(rows), 4, 0, p(o64), None, None, None) == EINVAL
    assert L.rsbwt_set_locate(None, p(sh), p(rows), 4, 0, None, p(o64), None) == EINVAL
    assert L.rsbwt_set_locate_dev(None, p(sh), p(rows), 4, 0, None, None, p(o32), None) == EINVAL
    text = np.frombuffer(b"ACGTACGT", np.uint8).copy()
    off = np.array([0, 4, 8], np.uint64)
    first = np.zeros(3, np.uint64)
    n = C.c_size_t(77)
    assert L.rsbwt_set_locate_var_capped(None, p(text), p(off), 2, 5, 0, p(first), None, None, None, None, None, 0, C.byref(n), None) == EINVAL
    assert b"null" in L.rsbwt_last_error()
    L.rsbwt_locate_last_work(None)  # (nothing to write to: no crash)
    w = (C.c_uint64 * 2)(9, 9)
    L.rsbwt_locate_last_work(w)
    assert list(w) == [0, 0]  # the failed calls above walked nothing


def test_no_gpu_is_enodev_and_argument_rules_on_a_handle(rsb):
    """on a box without a GPU no handle can be had: RSBWT_ENODEV, no CPU fallback.  Where there is one: all outputs null
    and null rows are RSBWT_EINVAL, n == 0 is RSBWT_OK"""
    L = rsb.lib()
    runs = np.array([(0 << 5) | 1, (1 << 5) | 3], np.uint8)
    if L.rsbwt_device_count() == 0:
        with pytest.raises(rsb.RsbwtError) as e:
            with rsb.GpuBWT(runs=runs, num_strings=1) as g:
                g.locate([0, 1])
        assert e.value.code == ENODEV and "no CPU fallback" in str(e.value)
        return
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    rows = np.arange(4, dtype=np.uint64)
    sh = np.zeros(4, np.uint32)
    o64 = np.zeros(4, np.uint64)
    with rsb.GpuBWT(runs=runs, num_strings=1) as g:
        h = g.handle
        assert L.rsbwt_locate(h, p(rows), 4, 0, None, None, None) == EINVAL and b"output" in L.rsbwt_last_error()
        assert L.rsbwt_locate(h, None, 4, 0, p(o64), None, None) == EINVAL
        assert L.rsbwt_locate(h, None, 0, 0, p(o64), None, None) == OK
        assert L.rsbwt_locate_dev(h, None, 0, 0, p(o64), None, None, None) == OK
        assert L.rsbwt_locate_dev(h, None, 0, 0, None, None, None, None) == EINVAL
        ss = rsb.ShardSet([g])
        try:
            assert L.rsbwt_set_locate(ss._s, None, None, 0, 0, p(o64), None, None) == OK
            assert L.rsbwt_set_locate(ss._s, p(sh), p(rows), 4, 0, None, None, None) == EINVAL
            assert L.rsbwt_set_locate(ss._s, None, p(rows), 4, 0, p(o64), None, None) == EINVAL
            bad = np.array([0, 0, 1, 0], np.uint32)  # shard 1 of a set of one
            assert L.rsbwt_set_locate(ss._s, p(bad), p(rows), 4, 0, p(o64), None, None) == EINVAL and b"shard" in L.rsbwt_last_error()
            assert L.rsbwt_set_locate_dev(ss._s, None, None, 0, 0, p(o64), None, None, None) == OK
        finally:
            ss.close()
