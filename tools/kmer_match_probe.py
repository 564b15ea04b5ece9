#!/usr/bin/env python3
"""KmerMatch / Reads on a resident shard set: Requests/s, the work counters (candidate rows, rows walked to '$', LF
steps, distinct read identities, reads extracted) and the host / device split of a window (device_ms: wall time inside
the calls that wait for the GPU -- search, exact-match, identity walks, extraction; host_ms: the rest of the call).  Each "request" is one
query, both strands (two jobs), as the service loop sends them through rsbwt_set_kmer_reads' path.

  python tools/kmer_match_probe.py --queries 256 --k 31 --skip 0 --qlen 100
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import readserver_amd as rsb  # noqa: E402


def rc(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=256)
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--skip", type=int, default=0)
    ap.add_argument("--qlen", type=int, default=100)
    ap.add_argument("--shards", type=int, default=4)
    ap.add_argument("--genome", type=int, default=200000)
    ap.add_argument("--haplotypes", type=int, default=16)
    ap.add_argument("--coverage", type=float, default=8.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--exactmatch", choices=("extract", "search"), default="extract",
                    help="how the shards answer query_exactmatch: by extraction, or by search from the terminator rows")
    a = ap.parse_args()
    rng = np.random.default_rng(7)
    with tempfile.TemporaryDirectory() as d:
        kw = dict(seed=11, genome_len=a.genome, haplotypes=a.haplotypes, snp_rate=0.002, read_len=150, coverage=a.coverage)
        shards = []
        for s in range(a.shards):
            p = os.path.join(d, f"s{s}.bwt")
            rsb.synth_popbwt(p, None, shard=s, num_shards=a.shards, **kw)
            shards.append(rsb.GpuBWT(p, ktab_depth=10, for_reads=True))
        rd = os.path.join(d, "all.reads")
        rsb.synth_popbwt(os.path.join(d, "all.bwt"), rd, **kw)
        reads = open(rd).read().split()
        ss = rsb.ShardSet(shards)
        ss.exactmatch_by_search(a.exactmatch == "search")
        qs = []
        for _ in range(a.queries):
            r = reads[rng.integers(len(reads))]
            s = int(rng.integers(0, len(r) - a.qlen + 1))
            qs.append(r[s:s + a.qlen])
        both = qs + [rc(q) for q in qs]
        ss.kmer_reads(both, a.k, a.skip, read_stride=256)  # warm-up
        times, split = [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            got = ss.kmer_reads(both, a.k, a.skip, read_stride=256)
            times.append(time.perf_counter() - t0)
            split.append(rsb.ShardSet.kmer_last_times())
        work = rsb.ShardSet.kmer_last_work()
        best = min(times)
        sp = split[times.index(best)]
        line = dict(exactmatch=a.exactmatch, queries=a.queries, k=a.k, skip=a.skip, qlen=a.qlen, shards=a.shards,
                    requests_per_s=round(a.queries / best, 1), window_ms=round(best * 1e3, 2),
                    call_ms=round(sp["total_ms"], 2), device_ms=round(sp["device_ms"], 2), host_ms=round(sp["host_ms"], 2),
                    reads_returned=sum(len(x) for row in got for x in row), **work,
                    rows_per_identity=round(work["candidates"] / max(work["identities"], 1), 2))
        print(json.dumps(line))
        ss.close()
        for g in shards:
            g.close()


if __name__ == "__main__":
    main()
