#!/usr/bin/env python3
"""SiteMatch candidates on a population BWT (csrc/gt_narrow.hip, rsbwt_set_gt_legs / rsbwt_set_gt_reads): the popBWT of
tools/popbwt_gpu.py (make_reads + bwt_runs: haplotypes of a seeded genome, reads of both strands, suffix-sorted on the GPU)
as one shard opened for reads, QUERIES windows of 79 symbols of the genome with the site in the middle, k = 12, skip = 3
and a max_interval_size M low enough that tiles are lengthened; the legs call and the reads call RUNS times each, every
step under a time limit of its own (a step that outlasts it ends the process with status 124).
usage: tools/gt_probe.py [queries=2000] [genome=1e6] [haplotypes=32] [coverage=1] [M=8] [out=profiles/gt_probe.json]
       -> the JSON written to `out` and printed: legs/s, candidate rows/s and the work counters."""
import json
import os
import statistics
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import readserver_amd as rsb  # noqa: E402

QUERIES = int(float(sys.argv[1])) if len(sys.argv) > 1 else 2000
GENOME = int(float(sys.argv[2])) if len(sys.argv) > 2 else 1_000_000
HAPS = int(sys.argv[3]) if len(sys.argv) > 3 else 32
COV = float(sys.argv[4]) if len(sys.argv) > 4 else 1.0
M = int(sys.argv[5]) if len(sys.argv) > 5 else 8
OUT = sys.argv[6] if len(sys.argv) > 6 else os.path.join(ROOT, "profiles", "gt_probe.json")
READ_LEN, QLEN, K, SKIP, RUNS, STEP_LIMIT_S = 100, 79, 12, 3, 5, 120.0


def timed(what, fn):
    guard = threading.Timer(STEP_LIMIT_S, lambda: (sys.stderr.write(f"gt_probe: {what} exceeded {STEP_LIMIT_S} s\n"), os._exit(124)))
    guard.daemon = True
    guard.start()
    try:
        t0 = time.perf_counter()
        out = fn()
        dt = time.perf_counter() - t0
    finally:
        guard.cancel()
    return dt, out


def main():
    import popbwt_gpu as P
    reads, genome = P.make_reads(GENOME, HAPS, COV, READ_LEN, 1e-3, 0.0, 5)
    runs, n, _ = P.bwt_runs(reads)
    g = rsb.GpuBWT(runs=runs.cpu().numpy(), num_strings=int(reads.shape[0]), for_reads=True)
    ss = rsb.ShardSet([g])
    try:
        rng = np.random.default_rng(23)
        gen = np.frombuffer(b"$ACGT", np.uint8)[genome.cpu().numpy()]
        at = rng.integers(0, GENOME - QLEN, QUERIES)
        qs = [gen[a:a + QLEN].tobytes().decode() for a in at]
        pos = np.full(QUERIES, QLEN // 2 + 1, np.uint64)
        timed("legs (warm-up)", lambda: ss.gt_legs(qs, pos, K, SKIP, M))
        t_legs, t_reads = [], []
        for _ in range(RUNS):
            dt, legs = timed("legs", lambda: ss.gt_legs(qs, pos, K, SKIP, M))
            t_legs.append(dt)
            w_legs = rsb.ShardSet.gt_last_work()
            dt, got = timed("reads", lambda: ss.gt_reads(qs, pos, K, SKIP, M, read_stride=128))
            t_reads.append(dt)
            w_reads = rsb.ShardSet.gt_last_work()
        m_legs, m_reads = statistics.median(t_legs), statistics.median(t_reads)
        res = {"symbols": int(n), "reads_indexed": int(reads.shape[0]), "ktab_depth": g.ktab_depth(), "queries": QUERIES, "query_length": QLEN,
               "k": K, "skip": SKIP, "M": M, "runs": RUNS, "legs_ms": [round(t * 1e3, 3) for t in t_legs],
               "reads_ms": [round(t * 1e3, 3) for t in t_reads], "legs_median_ms": round(m_legs * 1e3, 3),
               "reads_median_ms": round(m_reads * 1e3, 3), "legs_per_s": round(w_legs["legs"] / m_legs, 1),
               "candidate_rows_per_s": round(w_reads["candidates"] / m_reads, 1), "work_legs_call": w_legs, "work_reads_call": w_reads,
               "reads_returned": sum(len(x) for per in got for x in per), "legs_returned": sum(len(x) for x in legs),
               "timing": "host wall clock around the Python call: upload, kernels, copies back and the host's merge included"}
    finally:
        ss.close()
        g.close()
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
