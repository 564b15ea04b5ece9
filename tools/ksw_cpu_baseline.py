#!/usr/bin/env python3
"""What a caller had before csrc/ksw_align.hip: the reference's own src/service/ksw.c on CPU threads, on the pairs of
tools/ksw_probe.py (inputs(reads, seed): the same reads against the same windows).  ksw.c is compiled (-O2, as the
reference's build does) with a ten-line loop of this tool's own into a temporary directory that is removed again; THREADS
threads each align a contiguous share of the pairs (ctypes releases the interpreter lock for the call).  Timed as the median
of RUNS after a warm-up, wall clock around all threads; the symbols are coded by seq_nt4_table beforehand, outside the
clock.  Needs the reference's sources (RSBWT_REFERENCE, default /root/reference) and no GPU; writes the section
"cpu_ksw_c" into the probe's JSON (made if it is not there) without touching the rest.
usage: tools/ksw_cpu_baseline.py [reads=100000] [threads=16] [out=profiles/ksw_probe.json]"""
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ksw_probe as P  # noqa: E402

REF = os.environ.get("RSBWT_REFERENCE", "/root/reference")
RUNS = 5
LOOP = r"""
#include <stdint.h>
#include "ksw.h"
/* pairs [lo, hi): out[5 i ..] = score, te, qe, tb, qb of ksw_align as align_gt_read calls it (service.cpp:134) */
void ksw_loop(const uint8_t *q, const uint64_t *qoff, const uint8_t *t, const uint64_t *toff, uint64_t lo, uint64_t hi, const int8_t *mat, int32_t *out) {
    for (uint64_t i = lo; i < hi; ++i) {
        kswr_t r = ksw_align((int)(qoff[i + 1] - qoff[i]), (uint8_t *)q + qoff[i], (int)(toff[i + 1] - toff[i]), (uint8_t *)t + toff[i], 5, mat, 6, 1,
                             KSW_XSTART, 0);
        out[5 * i] = r.score; out[5 * i + 1] = r.te; out[5 * i + 2] = r.qe; out[5 * i + 3] = r.tb; out[5 * i + 4] = r.qb;
    }
}
"""


def main():
    n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 100000
    threads = int(sys.argv[2]) if len(sys.argv) > 2 else 16
    out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "ksw_probe.json")
    rtext, roff, item, wtext, off, _, _, _ = P.inputs(n)
    ttext, toff = P.pair_windows(item, wtext, off)
    nt4 = np.full(256, 4, np.uint8)
    for i, c in enumerate(b"ACGT"):
        nt4[c] = nt4[c + 32] = i
    q, t = nt4[rtext], nt4[ttext]  # (ksw_align reverses its inputs in place and puts them back: each thread has its own pairs)
    mat = np.full((5, 5), -1, np.int8)
    for i in range(4):
        for j in range(4):
            mat[i, j] = 1 if i == j else -4
    out = np.zeros((n, 5), np.int32)
    pv = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    with tempfile.TemporaryDirectory() as tmp:
        with open(os.path.join(tmp, "ksw_loop.c"), "w") as f:
            f.write(LOOP)
        so = os.path.join(tmp, "libksw_loop.so")
        subprocess.check_call(["gcc", "-O2", "-shared", "-fPIC", "-msse2", f"-I{os.path.join(REF, 'include', 'service')}",
                               os.path.join(REF, "src", "service", "ksw.c"), os.path.join(tmp, "ksw_loop.c"), "-o", so])
        L = C.CDLL(so)
        L.ksw_loop.restype = None
        L.ksw_loop.argtypes = [C.c_void_p] * 4 + [C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p]
        cuts = [n * k // threads for k in range(threads + 1)]

        def run():
            th = [threading.Thread(target=L.ksw_loop, args=(pv(q), pv(roff), pv(t), pv(toff), cuts[k], cuts[k + 1], pv(mat), pv(out)))
                  for k in range(threads)]
            t0 = time.perf_counter()
            for x in th:
                x.start()
            for x in th:
                x.join()
            return time.perf_counter() - t0
        run()
        times = [run() for _ in range(RUNS)]
        del L
    res = {}
    if os.path.exists(out_path):
        res = json.load(open(out_path))
    med = statistics.median(times)
    res["cpu_ksw_c"] = {"reads": n, "threads": threads, "cpus_of_the_machine": os.cpu_count(), "compiler_flags": "-O2 -msse2", "runs": RUNS,
                        "ms": [round(x * 1e3, 3) for x in times], "pairs_per_s": round(n / med, 1),
                        "checksum_score_sum": int(out[:, 0].sum()),
                        "timing": "wall clock around all threads; the machine is the one the library is built on, not the GPU host"}
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res["cpu_ksw_c"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
