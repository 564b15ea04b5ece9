#!/usr/bin/env python3
"""Locate against extraction on the same rows (csrc/locate.hip against csrc/extract_lines.hip): the resident set of
tools/service_reads_probe.py (P suffix partitions of a synthetic read collection, opened for reads, one process), one
(shard, row) batch of ROWS rows per shard made on the device by rsbwt_set_interval_rows_dev, then rsbwt_set_locate_dev and
rsbwt_set_extract_dev on those rows in turn, RUNS times each, every step under a time limit of its own (a step that
outlasts it ends the process with status 124).  Locate's memory requests are a subset of extraction's -- the LF walk
without the psi walk, the character stores and the prefix move -- so its median should not exceed extraction's.
usage: tools/locate_probe.py [rows_per_shard=2e6] [partitions=4] [genome=300000] [coverage=8] [out=profiles/locate_probe.json]
       -> the JSON written to `out` and printed."""
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import readserver_amd as rsb  # noqa: E402

ROWS = int(float(sys.argv[1])) if len(sys.argv) > 1 else 2_000_000
P = int(sys.argv[2]) if len(sys.argv) > 2 else 4
GENOME = int(float(sys.argv[3])) if len(sys.argv) > 3 else 300000
COV = float(sys.argv[4]) if len(sys.argv) > 4 else 8.0
OUT = sys.argv[5] if len(sys.argv) > 5 else os.path.join(ROOT, "profiles", "locate_probe.json")
READ_LEN, STRIDE, WIDTH, RUNS, STEP_LIMIT_S = 100, 128, 100, 5, 60.0
L = rsb.lib()


def timed(what, fn):
    """fn() followed by a device synchronise, under the step's time limit: seconds"""
    import torch
    guard = threading.Timer(STEP_LIMIT_S, lambda: (sys.stderr.write(f"locate_probe: {what} exceeded {STEP_LIMIT_S} s\n"), os._exit(124)))
    guard.daemon = True
    guard.start()
    try:
        t0 = time.perf_counter()
        rc = fn()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    finally:
        guard.cancel()
    assert rc == 0, (what, L.rsbwt_last_error())
    return dt


def main():
    import torch
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    with tempfile.TemporaryDirectory() as td:
        kw = dict(seed=77, genome_len=GENOME, haplotypes=8, snp_rate=0.002, read_len=READ_LEN, coverage=COV)
        shards = []
        for s in range(P):
            path = os.path.join(td, f"s{s}.bwt")
            rsb.synth_popbwt(path, None, shard=s, num_shards=P, **kw)
            shards.append(rsb.GpuBWT(path, for_reads=True))
        ss = rsb.ShardSet(shards)
        try:
            ns = [g.getBWLen() for g in shards]
            # Q intervals of WIDTH rows in every shard, at random places: ROWS rows per shard, in rsbwt_set_query's order
            Q = max(1, ROWS // WIDTH)
            rng = np.random.default_rng(11)
            lo = np.stack([rng.integers(0, n - WIDTH, Q) for n in ns]).astype(np.uint64)
            pairs = np.stack([lo, lo + np.uint64(WIDTH - 1)], axis=-1)
            total, n_per = P * Q * WIDTH, Q * WIDTH
            d_pairs = torch.from_numpy(pairs.view(np.int64)).cuda()
            d_first = torch.zeros(Q + 1, dtype=torch.int64, device="cuda")
            d_matches = torch.zeros(Q, dtype=torch.int64, device="cuda")
            d_shard = torch.zeros(total, dtype=torch.int32, device="cuda")
            d_rows = torch.zeros(total, dtype=torch.int64, device="cuda")
            timed("interval rows", lambda: L.rsbwt_set_interval_rows_dev(ss._s, p(d_pairs), Q, 0, p(d_first), p(d_matches), p(d_shard), p(d_rows),
                                                                         total, None))
            assert int(d_first[Q]) == total
            # extraction takes the same rows as [shard][n]
            d_xrows = torch.stack([d_rows[d_shard == s] for s in range(P)]).contiguous()
            assert tuple(d_xrows.shape) == (P, n_per)
            d_rr = torch.zeros(total, dtype=torch.int64, device="cuda")
            d_od = torch.zeros(total, dtype=torch.int64, device="cuda")
            d_of = torch.zeros(total, dtype=torch.int32, device="cuda")
            d_out = torch.zeros((P, n_per, STRIDE), dtype=torch.uint8, device="cuda")
            d_len = torch.zeros((P, n_per), dtype=torch.int32, device="cuda")
            d_pl = torch.zeros((P, n_per), dtype=torch.int32, device="cuda")
            locate = lambda: L.rsbwt_set_locate_dev(ss._s, p(d_shard), p(d_rows), total, 0, p(d_rr), p(d_od), p(d_of), None)  # noqa: E731
            extract = lambda: L.rsbwt_set_extract_dev(ss._s, p(d_xrows), n_per, p(d_out), STRIDE, p(d_len), p(d_pl), None)  # noqa: E731
            timed("locate (warm-up)", locate)
            timed("extract (warm-up: builds nothing, the shards were opened for reads)", extract)
            t_loc, t_ext = [], []
            for _ in range(RUNS):
                t_loc.append(timed("locate", locate))
                t_ext.append(timed("extract", extract))
            # the two agree: extraction's prefix length is locate's offset
            of = torch.stack([d_of[d_shard == s] for s in range(P)])
            agree = bool(torch.equal(of, d_pl)) and bool((d_len.view(-1) != -1).all())
            # the work counters, from the host form on the same batch (not timed)
            sh_h, rows_h = d_shard.cpu().numpy().view(np.uint32), d_rows.cpu().numpy().view(np.uint64)
            of_h = np.empty(total, np.uint32)
            assert L.rsbwt_set_locate(ss._s, sh_h.ctypes.data_as(C.c_void_p), rows_h.ctypes.data_as(C.c_void_p), total, 0, None, None,
                                      of_h.ctypes.data_as(C.c_void_p)) == 0, L.rsbwt_last_error()
            work = rsb.ShardSet.locate_last_work()
            m_loc, m_ext = statistics.median(t_loc), statistics.median(t_ext)
            res = {"partitions": P, "symbols_per_shard": [int(n) for n in ns], "rows": total, "rows_per_shard": n_per, "read_length": READ_LEN,
                   "extract_stride": STRIDE, "runs": RUNS, "locate_ms": [round(t * 1e3, 3) for t in t_loc],
                   "extract_ms": [round(t * 1e3, 3) for t in t_ext], "locate_median_ms": round(m_loc * 1e3, 3),
                   "extract_median_ms": round(m_ext * 1e3, 3), "locate_over_extract": round(m_loc / m_ext, 4),
                   "locate_rows_per_s": round(total / m_loc, 1), "extract_rows_per_s": round(total / m_ext, 1),
                   "work2": [work["located"], work["lf_steps"]], "locate_lf_steps_per_s": round(work["lf_steps"] / m_loc, 1),
                   "offsets_equal_prefix_lengths": agree,
                   "timing": "host wall clock around the call and a device synchronise; the two calls alternate"}
        finally:
            ss.close()
            for g in shards:
                g.close()
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 0 if agree else 1


if __name__ == "__main__":
    sys.exit(main())
