#!/usr/bin/env python3
"""rsbwt_query_exactmatch by extraction against the same call by backward search from the terminator rows
(rsbwt_exactmatch_by_search, csrc/read_lookup.hip), on a VALID population BWT built on the GPU as tools/popbwt_gpu.py
builds it: ONE shard holding every read of H haplotypes at coverage c each (depth H * c).

Tiles, 10^5 per length by default:
  --tile = read length : half of them whole reads of the collection, half reads with one base changed;
  --tile < read length : windows cut from reads (in a collection of one read length none of them IS a read: the
                         extraction's worst case -- every read that contains the window is extracted and compared).
Both modes answer the same strings; the answers are compared (and readserver_amd.selfcheck.exactmatch_modes run on its
own sample) before anything is timed.  Timing: one warm-up call per mode, then --reps calls; median and minimum of the
wall time of the whole call (upload, launches, copy back) in ms.  --only search|extract: that mode's calls alone (what a
profiler run wants); --counting: the '$' count's counters of one search-mode call (rsbwt_set_counting).

usage: tools/exactmatch_probe.py [--genome 2e5 --haplotypes 64 --coverage 2 --read-len 100 --tiles 1e5 --tile 100 --tile 73]
  -> one JSON line
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import popbwt_gpu  # noqa: E402
import readserver_amd as rsb  # noqa: E402
from readserver_amd import selfcheck  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", type=float, default=2e5)
    ap.add_argument("--haplotypes", type=int, default=64)
    ap.add_argument("--coverage", type=float, default=2.0, help="per haplotype")
    ap.add_argument("--read-len", type=int, default=100)
    ap.add_argument("--snp", type=float, default=1e-3)
    ap.add_argument("--tiles", type=float, default=1e5)
    ap.add_argument("--tile", type=int, action="append", help="tile length (repeatable; default: 100 and 73)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", choices=("search", "extract"))
    ap.add_argument("--counting", action="store_true")
    ap.add_argument("--for-reads", action="store_true", help="open the shard with RSBWT_OPEN_READS")
    ap.add_argument("--seed", type=int, default=7)
    a = ap.parse_args()
    L = rsb.lib()
    RL, Q = a.read_len, int(a.tiles)
    reads, _ = popbwt_gpu.make_reads(int(a.genome), a.haplotypes, a.coverage, RL, a.snp, 0.0, a.seed)
    runs, n, _ = popbwt_gpu.bwt_runs(reads)
    torch.cuda.synchronize()
    g = rsb.GpuBWT(device_runs=(runs.data_ptr(), int(runs.numel())), num_strings=int(reads.shape[0]), ktab_depth=10, for_reads=a.for_reads)
    assert g.getBWLen() == n
    lut = np.frombuffer(b"$ACGT", np.uint8)
    rng = np.random.default_rng(a.seed)
    pick = torch.from_numpy(rng.integers(0, reads.shape[0], Q)).to(reads.device)
    base = lut[reads[pick].cpu().numpy()]  # [Q, RL] ASCII
    out = dict(symbols=int(n), reads=int(reads.shape[0]), read_len=RL, depth=a.haplotypes * a.coverage, window_span=g.window_span(),
               for_reads=bool(a.for_reads), tiles=Q, reps=a.reps, timing="wall ms of the whole call; one warm-up call, then reps; median / min")
    chk = selfcheck.exactmatch_modes(g, n=20000, seed=a.seed, stride=((RL + 16) // 16) * 16)
    assert chk["differing"] == 0, chk
    out["selfcheck"] = chk
    for tl in a.tile or [100, 73]:
        tl = min(tl, RL)
        if tl == RL:
            ws = base.copy()
            j = rng.integers(0, RL, Q // 2)
            rows = np.arange(Q // 2) * 2 + 1
            ws[rows, j] = lut[1 + (np.searchsorted(lut[1:], ws[rows, j]) + rng.integers(1, 4, Q // 2)) % 4]
        else:
            st = rng.integers(0, RL - tl + 1, Q)
            ws = np.stack([base[i, s:s + tl] for i, s in enumerate(st)])
        ws = np.ascontiguousarray(ws)
        res, found = {}, {}
        for mode in ("extract", "search"):
            if a.only and a.only != mode:
                continue
            g.exactmatch_by_search = mode == "search"
            found[mode] = rsb.query_exactmatch_batch(g, ws)  # warm-up
            ts = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                rsb.query_exactmatch_batch(g, ws)
                ts.append((time.perf_counter() - t0) * 1e3)
            res[mode + "_ms"] = dict(median=round(statistics.median(ts), 3), min=round(min(ts), 3))
        if len(found) == 2:
            assert np.array_equal(found["extract"], found["search"]), tl
            res["speedup_median"] = round(res["extract_ms"]["median"] / res["search_ms"]["median"], 2)
        res["found"] = int(next(iter(found.values())).sum())
        if a.counting and (not a.only or a.only == "search"):
            g.exactmatch_by_search = True
            assert L.rsbwt_set_counting(g.handle, 1) == 0
            rsb.query_exactmatch_batch(g, ws[:1 << 16])
            words = (C.c_uint64 * 16)()
            assert L.rsbwt_last_search_counters(g.handle, words) == 0
            assert L.rsbwt_set_counting(g.handle, 0) == 0
            res["counters_of_the_first_65536"] = dict(lf_steps=int(words[0]), occ_lookups=int(words[1]), lines=int(words[2]), continuation_lines=int(words[11]),
                                                      one_lane_per_search=int(words[12]), results_ranked=int(words[13]),
                                                      positions_on_a_continuation=int(words[14]), second_lines=int(words[15]))
        out[f"tile_{tl}"] = res
    g.exactmatch_by_search = False
    print(json.dumps(out))
    g.close()


if __name__ == "__main__":
    main()
