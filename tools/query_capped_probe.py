#!/usr/bin/env python3
"""What making a batch's rows on the GPU costs against the host loop, and what the service pays for the max_match_reads
key when it is absent.
  1. On the set tools/service_reads_probe.py opens (P suffix partitions of a synthetic read collection): rsbwt_set_query_var
     against rsbwt_set_query_var_capped(max_rows = 0), alternating, five runs each, over one window-sized batch (4,096
     mixed-length queries) and one large batch; medians, spreads and the capped call's work counters
     (rsbwt_set_query_last_work); then the window batch with "A" in it and a limit, to show what the limit bounds.
  2. With --parent DIR (a built checkout of the parent commit): tools/service_reads_probe.py 100000 4 of that checkout
     and of this one (key absent), alternating, three runs each.
usage: tools/query_capped_probe.py [--parent DIR] [--large 65536] [--out profiles/query_capped_probe.json]"""
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def arg(name, dflt):
    if name in sys.argv:
        i = sys.argv.index(name)
        v = sys.argv[i + 1]
        del sys.argv[i:i + 2]
        return v
    return dflt


PARENT = arg("--parent", None)
LARGE = int(float(arg("--large", "65536")))
OUT = arg("--out", None)
P, GENOME, COV, READ_LEN, MINL, MAXL = 4, 300000, 8.0, 100, 73, 100
result = {"set": f"{P} suffix partitions, genome {GENOME}, coverage {COV}, read length {READ_LEN} (tools/service_reads_probe.py's)"}

import readserver_amd as rsb  # noqa: E402

L = rsb.lib()


def timed(ss, qs, which, max_rows, room, stride=256):
    text, off = ss._var_text(qs)
    Q = len(qs)
    first = np.zeros(Q + 1, np.uint64)
    sh = np.zeros(room, np.uint32)
    ln = np.zeros(room, np.uint32)
    reads = np.zeros((room, stride), np.uint8)
    matches = np.zeros(Q, np.uint64)
    n = C.c_size_t()
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    t0 = time.perf_counter()
    if which == "query_var":
        rc = L.rsbwt_set_query_var(ss._s, p(text), p(off), Q, p(first), p(sh), p(reads), stride, p(ln), room, C.byref(n))
    else:
        rc = L.rsbwt_set_query_var_capped(ss._s, p(text), p(off), Q, max_rows, p(first), p(sh), p(reads), stride, p(ln), room, C.byref(n), p(matches))
    dt = (time.perf_counter() - t0) * 1e3
    assert rc == 0, L.rsbwt_last_error()
    w = (C.c_uint64 * 4)()
    L.rsbwt_set_query_last_work(w)
    return dt, n.value, [int(x) for x in w]


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "runs_ms": [round(x, 3) for x in ms]}


with tempfile.TemporaryDirectory() as td:
    kw = dict(seed=77, genome_len=GENOME, haplotypes=8, snp_rate=0.002, read_len=READ_LEN, coverage=COV)
    shards, reads = [], []
    for s in range(P):
        p_, rd = os.path.join(td, f"s{s}.bwt"), os.path.join(td, f"s{s}.reads")
        rsb.synth_popbwt(p_, rd, shard=s, num_shards=P, **kw)
        shards.append(rsb.GpuBWT(p_, for_reads=True))
        reads += open(rd).read().split()
    ss = rsb.ShardSet(shards)
    rng = np.random.default_rng(5)

    def batch(n):
        qs = []
        for _ in range(n):
            r = reads[int(rng.integers(len(reads)))]
            k = int(rng.integers(25, MAXL))
            st = int(rng.integers(0, len(r) - k + 1))
            qs.append(r[st:st + k])
        return qs
    for name, Q in (("window", 4096), ("large", LARGE)):
        qs = batch(Q)
        _, total, _ = timed(ss, qs, "capped", 0, 64 * Q)  # (warm: buffers, first launches)
        room = total + 16
        runs = {"query_var": [], "capped": []}
        work = None
        for _ in range(5):
            for which in ("query_var", "capped"):
                dt, n, w = timed(ss, qs, which, 0, room)
                assert n == total
                runs[which].append(dt)
                if which == "capped":
                    work = w
        result[name] = {"queries": Q, "reads": total, "rsbwt_set_query_var": summary(runs["query_var"]),
                        "rsbwt_set_query_var_capped(max_rows=0)": summary(runs["capped"]),
                        "work {rows expanded on the device, rows uploaded from the host, queries over the limit, bytes to the host before the extraction}": work}
    # what the limit bounds: the window batch with one "A" in it
    qs = batch(4095) + ["A"]
    dt, n, w = timed(ss, qs, "capped", 100000, 100000)
    text, off = ss._var_text(qs)
    m = np.zeros(len(qs), np.uint64)
    first = np.zeros(len(qs) + 1, np.uint64)
    nn = C.c_size_t()
    L.rsbwt_set_query_var_capped(ss._s, text.ctypes.data_as(C.c_void_p), off.ctypes.data_as(C.c_void_p), len(qs), 100000, first.ctypes.data_as(C.c_void_p), None, None, 256,
                                 None, 0, C.byref(nn), m.ctypes.data_as(C.c_void_p))
    result["window_with_A"] = {"queries": len(qs), "max_rows": 100000, "rows_of_A": int(m[-1]), "reads_returned": n, "ms": round(dt, 3), "work": w,
                               "bytes_the_uncapped_call_would_stage": int(m.sum()) * 256}
    ss.close()
    for g in shards:
        g.close()

if PARENT:
    rates = {"parent": [], "this": []}
    for _ in range(3):
        for who in ("parent", "this"):
            probe = os.path.join(os.path.abspath(PARENT) if who == "parent" else ROOT, "tools", "service_reads_probe.py")
            env = {k: v for k, v in os.environ.items() if k != "RSBWT_LIB"}
            r = subprocess.run([sys.executable, probe, "100000", "4"], env=env, capture_output=True, text=True, timeout=900)
            assert r.returncode == 0, r.stdout + r.stderr
            rates[who].append(json.loads(r.stdout.strip().splitlines()[-1])["requests_per_s"])
    result["service_reads_probe 100000 4, key absent"] = {
        who: {"median_requests_per_s": statistics.median(v), "min": min(v), "max": max(v), "runs": v} for who, v in rates.items()}

line = json.dumps(result)
print(line)
if OUT:
    with open(OUT, "w") as f:
        f.write(json.dumps(result, indent=1) + "\n")
