"""The boundary of the capped set query and of the service's max_match_reads, without a GPU: the header, the ctypes
binding, the null-argument rules, the service.cfg key, and (tests/native/query_capped_host.cpp, a CPU build of the service
code over a stub engine) the hook the service reaches the capped entry point through."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = ["rsbwt_set_query_var_capped", "rsbwt_set_interval_rows_dev", "rsbwt_set_query_last_work"]
SERVICE = ["rsbwt_service_set_max_match_reads", "rsbwt_service_capped_requests"]
EINVAL = -1


def test_header_declares_and_native_binds_the_entry_points(rsb):
    from readserver_amd import _native
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rsbwt.h")).read(), flags=re.S)
    L = C.CDLL(rsb.lib_path())
    for n in ENTRY + SERVICE:
        assert re.search(r"\b%s\s*\(" % n, txt), f"{n} is not declared in include/rsbwt.h"
        assert n in _native.SIGNATURES and hasattr(L, n) and hasattr(rsb.lib(), n)
    assert len(_native.SIGNATURES["rsbwt_set_query_var_capped"][1]) == 13
    assert len(_native.SIGNATURES["rsbwt_set_interval_rows_dev"][1]) == 10
    assert callable(rsb.ShardSet.query_var_capped)
    # rsbwt_set_query_var itself keeps its signature
    assert len(_native.SIGNATURES["rsbwt_set_query_var"][1]) == 11


def test_null_arguments(rsb):
    L = rsb.lib()
    text = np.frombuffer(b"ACGTACGT", np.uint8).copy()
    off = np.array([0, 4, 8], np.uint64)
    first = np.zeros(3, np.uint64)
    n = C.c_size_t(77)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert L.rsbwt_set_query_var_capped(None, p(text), p(off), 2, 5, p(first), None, None, 256, None, 0, C.byref(n), None) == EINVAL
    assert b"null" in L.rsbwt_last_error()
    assert L.rsbwt_set_query_var_capped(None, p(text), p(off), 2, 5, p(first), None, None, 256, None, 0, None, None) == EINVAL
    assert L.rsbwt_set_query_var_capped(None, p(text), p(off), 2, 5, p(first), None, None, 0, None, 0, C.byref(n), None) == EINVAL
    assert L.rsbwt_set_interval_rows_dev(None, None, 2, 5, None, None, None, None, 0, None) == EINVAL
    L.rsbwt_set_query_last_work(None)  # (nothing to write to: no crash)
    w = (C.c_uint64 * 4)(9, 9, 9, 9)
    L.rsbwt_set_query_last_work(w)
    assert list(w) == [0, 0, 0, 0]  # the failed calls above did no work
    assert L.rsbwt_service_set_max_match_reads(None, 0) == EINVAL and L.rsbwt_service_capped_requests(None) == 0


def test_service_cfg_with_and_without_the_key(rsb, golden_dir, tmp_path):
    L = rsb.lib()
    text = open(os.path.join(golden_dir, "service_template.cfg")).read()
    for value in (None, "100000", "0"):
        p = tmp_path / "service.cfg"
        p.write_text(text + (f'\nmax_match_reads = "{value}";\n' if value is not None else ""))
        h = C.c_void_p()
        assert L.rsbwt_service_config_load(str(p).encode(), C.byref(h)) == 0
        got = L.rsbwt_service_config_get(h, b"max_match_reads")
        assert got == (value.encode() if value is not None else None)
        assert L.rsbwt_service_config_get(h, b"pull") is not None
        L.rsbwt_service_config_free(h)


def test_service_limit_through_the_hook_on_a_stub_engine(tmp_path):
    """tests/native/query_capped_host.cpp: with the hook null a limit is RSBWT_ENODEV (0 is taken); with a stub engine
    behind it a window's one-symbol queries get empty Replies and their neighbours their reads"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "query_capped_host")
    csrc = os.path.join(ROOT, "readserver_amd", "csrc")
    srcs = [os.path.join(ROOT, "tests", "native", "query_capped_host.cpp"), os.path.join(csrc, "service_slice.cpp"),
            os.path.join(csrc, "service_loop.cpp")]
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", f"-I{os.path.join(ROOT, 'include')}", f"-I{csrc}", *srcs, "-ldl", "-lpthread", "-o", exe],
                       capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout + r.stderr
