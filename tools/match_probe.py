#!/usr/bin/env python3
"""Matching statistics on a population BWT (csrc/match_stats.hip, rsbwt_set_match_lengths / _dev / rsbwt_set_smems): the
popBWT of tools/popbwt_gpu.py (make_reads + bwt_runs: haplotypes of a seeded genome, reads of both strands, suffix-sorted
on the GPU) as one shard, WINDOWS windows of 100 symbols of its haplotypes (indexed reads: each is such a window), every
second one with one substitution in it.  The host-buffer call gives the work counters and a wall-clock time; the
device-resident call is timed with events around the launch alone, RUNS times each, every step under a time limit of its
own (a step that outlasts it ends the process with status 124).
usage: tools/match_probe.py [windows=20000] [genome=1e6] [haplotypes=32] [coverage=1] [out=profiles/match_probe.json]
       -> the JSON written to `out` and printed: positions/s, LF steps/s, lane-passes per step, the share of table starts
          and the counters."""
import ctypes as C
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

WINDOWS = int(float(sys.argv[1])) if len(sys.argv) > 1 else 20000
GENOME = int(float(sys.argv[2])) if len(sys.argv) > 2 else 1_000_000
HAPS = int(sys.argv[3]) if len(sys.argv) > 3 else 32
COV = float(sys.argv[4]) if len(sys.argv) > 4 else 1.0
OUT = sys.argv[5] if len(sys.argv) > 5 else os.path.join(ROOT, "profiles", "match_probe.json")
READ_LEN, RUNS, STEP_LIMIT_S = 100, 5, 120.0
CEILING = (45e9, 47e9)  # random line requests per second of the memory system (profiles/r01_gather_microbench.txt)


def timed(what, fn):
    guard = threading.Timer(STEP_LIMIT_S, lambda: (sys.stderr.write(f"match_probe: {what} exceeded {STEP_LIMIT_S} s\n"), os._exit(124)))
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
    import torch
    import popbwt_gpu as P
    reads, _ = P.make_reads(GENOME, HAPS, COV, READ_LEN, 1e-3, 0.0, 5)
    runs, n, _ = P.bwt_runs(reads)
    g = rsb.GpuBWT(runs=runs.cpu().numpy(), num_strings=int(reads.shape[0]))
    ss = rsb.ShardSet([g])
    L = rsb.lib()
    try:
        rng = np.random.default_rng(29)
        pick = rng.integers(0, int(reads.shape[0]), WINDOWS)
        win = np.frombuffer(b"$ACGT", np.uint8)[reads[torch.from_numpy(pick).to(reads.device)].cpu().numpy()].copy()
        for i in range(1, WINDOWS, 2):  # one substitution in every second window
            j = int(rng.integers(0, READ_LEN))
            win[i, j] = [c for c in b"ACGT" if c != win[i, j]][int(rng.integers(0, 3))]
        qs = [w.tobytes() for w in win]
        N = WINDOWS * READ_LEN
        timed("host call (warm-up)", lambda: ss.match_lengths(qs))
        t_host, t_smem = [], []
        for _ in range(RUNS):
            dt, ln = timed("host call", lambda: ss.match_lengths(qs, intervals=True))
            t_host.append(dt)
            wk = rsb.ShardSet.match_last_work()
            dt, (recs, first) = timed("smems", lambda: ss.smems(qs, raw=True))
            t_smem.append(dt)
            wk_smem = rsb.ShardSet.match_last_work()
        # the launch alone: device-resident form, events on the stream it is enqueued on
        text, off = ss._var_text(qs)
        d_text, d_off = torch.from_numpy(text).cuda(), torch.from_numpy(off.view(np.int64)).cuda()
        d_len = torch.zeros(N, dtype=torch.int32, device="cuda")
        d_pairs = torch.zeros(2 * N, dtype=torch.int64, device="cuda")
        p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

        def launch():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rc = L.rsbwt_set_match_lengths_dev(ss._s, p(d_text), p(d_off), WINDOWS, N, 0, 1, p(d_len), p(d_pairs), None)
            e1.record()
            torch.cuda.synchronize()
            if rc:
                raise RuntimeError(L.rsbwt_last_error().decode())
            return e0.elapsed_time(e1) * 1e-3
        timed("device call (warm-up)", launch)
        t_dev = [timed("device call", launch)[1] for _ in range(RUNS)]
        same = bool((d_len.cpu().numpy().view(np.uint32) == ln[0][0]).all())
        m_host, m_dev, m_smem = statistics.median(t_host), statistics.median(t_dev), statistics.median(t_smem)
        steps_s = wk["lf_steps"] / m_dev
        lens = ln[0][0]
        res = {"symbols": int(n), "reads_indexed": int(reads.shape[0]), "ktab_depth": g.ktab_depth(), "window_span": g.window_span(),
               "windows": WINDOWS, "window_length": READ_LEN, "positions": N, "runs": RUNS,
               "host_ms": [round(t * 1e3, 3) for t in t_host], "smems_ms": [round(t * 1e3, 3) for t in t_smem],
               "device_ms": [round(t * 1e3, 4) for t in t_dev], "host_median_ms": round(m_host * 1e3, 3),
               "smems_median_ms": round(m_smem * 1e3, 3), "device_median_ms": round(m_dev * 1e3, 4),
               "positions_per_s_host_call": round(N / m_host, 1), "positions_per_s_launch": round(N / m_dev, 1),
               "lf_steps_per_s_launch": round(steps_s, 1), "lane_passes_per_s_launch": round(wk["passes"] / m_dev, 1),
               "lane_passes_per_step": round(wk["passes"] / max(wk["lf_steps"], 1), 4),
               "table_start_share": round(wk["table_starts"] / max(wk["items"], 1), 4),
               "fraction_of_request_ceiling": [round(wk["passes"] / m_dev / c, 4) for c in CEILING],
               "mean_length": round(float(lens.mean()), 2), "work_lengths_call": wk, "work_smems_call": wk_smem,
               "smems_returned": int(len(recs)), "device_form_agrees_with_host_form": same,
               "timing": "host_*: wall clock around the Python call (upload, kernels, copies back, the host's split of the pairs); "
                         "device_*: events around the device-resident call's launch alone (lengths and pairs written)"}
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
