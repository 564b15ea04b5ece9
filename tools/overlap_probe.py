#!/usr/bin/env python3
"""Overlaps on a population BWT (csrc/overlaps.hip, rsbwt_set_overlaps / _dev): the popBWT of tools/popbwt_gpu.py
(make_reads + bwt_runs: haplotypes of a seeded genome, reads of both strands, suffix-sorted on the GPU) as one shard,
WINDOWS windows of 100 symbols of its haplotypes (indexed reads: each is such a window), every second one with one
substitution in it, at min_overlap 31 and 1.  Per min_overlap, as medians of RUNS: the host-buffer call (wall clock, work
counters), the device-resident call (events around the launch alone), and the way to the same counts without the call --
every suffix of min_overlap symbols or more as a query of its own through rsbwt_set_find_intervals_var, then
rsbwt_debug_dollar_count on the intervals (wall clock; the suffixes' text is made before the clock starts) -- whose counts
must agree with the call's everywhere.  Every step runs under a time limit of its own (a step that outlasts it ends the
process with status 124).
usage: tools/overlap_probe.py [windows=20000] [genome=1e6] [haplotypes=32] [coverage=1] [out=profiles/overlap_probe.json]"""
import ctypes as C
import json
import os
import statistics
import sys
import threading
import time

import numpy as np

os.environ.setdefault("RSBWT_ENABLE_TEST_HOOKS", "1")  # (rsbwt_debug_dollar_count, the baseline's second half, is a test hook)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import readserver_amd as rsb  # noqa: E402

WINDOWS = int(float(sys.argv[1])) if len(sys.argv) > 1 else 20000
GENOME = int(float(sys.argv[2])) if len(sys.argv) > 2 else 1_000_000
HAPS = int(sys.argv[3]) if len(sys.argv) > 3 else 32
COV = float(sys.argv[4]) if len(sys.argv) > 4 else 1.0
OUT = sys.argv[5] if len(sys.argv) > 5 else os.path.join(ROOT, "profiles", "overlap_probe.json")
READ_LEN, RUNS, STEP_LIMIT_S = 100, 5, 120.0
MIN_OVERLAPS = (31, 1)


def timed(what, fn):
    guard = threading.Timer(STEP_LIMIT_S, lambda: (sys.stderr.write(f"overlap_probe: {what} exceeded {STEP_LIMIT_S} s\n"), os._exit(124)))
    guard.daemon = True
    guard.start()
    try:
        t0 = time.perf_counter()
        out = fn()
        dt = time.perf_counter() - t0
    finally:
        guard.cancel()
    return dt, out


def suffix_batch(win, m):
    """every suffix of m symbols or more of every window as a query of its own: (text, off, suffixes per window)"""
    per = READ_LEN - m + 1
    idx = np.concatenate([np.arange(s, READ_LEN) for s in range(per)])
    text = np.append(win[:, idx].ravel(), np.uint8(0))
    lens = np.tile(np.arange(READ_LEN, m - 1, -1, dtype=np.uint64), win.shape[0])
    off = np.zeros(lens.size + 1, np.uint64)
    off[1:] = np.cumsum(lens, dtype=np.uint64)
    return text, off, per


def main():
    import torch
    import popbwt_gpu as P
    reads, _ = P.make_reads(GENOME, HAPS, COV, READ_LEN, 1e-3, 0.0, 5)
    runs, n, _ = P.bwt_runs(reads)
    g = rsb.GpuBWT(runs=runs.cpu().numpy(), num_strings=int(reads.shape[0]))
    ss = rsb.ShardSet([g])
    L = rsb.lib()
    pv = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    res = {"symbols": int(n), "reads_indexed": int(reads.shape[0]), "ktab_depth": g.ktab_depth(), "window_span": g.window_span(),
           "windows": WINDOWS, "window_length": READ_LEN, "shards": 1, "runs": RUNS, "by_min_overlap": {}}
    try:
        rng = np.random.default_rng(29)
        pick = rng.integers(0, int(reads.shape[0]), WINDOWS)
        win = np.frombuffer(b"$ACGT", np.uint8)[reads[torch.from_numpy(pick).to(reads.device)].cpu().numpy()].copy()
        for i in range(1, WINDOWS, 2):  # one substitution in every second window
            j = int(rng.integers(0, READ_LEN))
            win[i, j] = [c for c in b"ACGT" if c != win[i, j]][int(rng.integers(0, 3))]
        qs = [w.tobytes() for w in win]
        N = WINDOWS * READ_LEN
        text, off = ss._var_text(qs)
        d_text, d_off = torch.from_numpy(text).cuda(), torch.from_numpy(off.view(np.int64)).cuda()
        d_pairs = torch.zeros(2 * N, dtype=torch.int64, device="cuda")
        p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
        for m in MIN_OVERLAPS:
            timed("host call (warm-up)", lambda: ss.overlaps(qs, m))
            t_host = []
            for _ in range(RUNS):
                dt, (cnt, od) = timed("host call", lambda: ss.overlaps(qs, m, ordinals=True))
                t_host.append(dt)
                wk = rsb.ShardSet.overlap_last_work()

            def launch():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                rc = L.rsbwt_set_overlaps_dev(ss._s, p(d_text), p(d_off), WINDOWS, N, m, 0, p(d_pairs), None)
                e1.record()
                torch.cuda.synchronize()
                if rc:
                    raise RuntimeError(L.rsbwt_last_error().decode())
                return e0.elapsed_time(e1) * 1e-3
            timed("device call (warm-up)", launch)
            t_dev = [timed("device call", launch)[1] for _ in range(RUNS)]
            dp = d_pairs.cpu().numpy().view(np.uint64).reshape(N, 2)
            same_dev = bool((dp[:, 1] == cnt[0]).all() and (dp[:, 0] == od[0]).all())
            # ---- the way without the call: one query per suffix, then the '$' count of the intervals
            stext, soff, per = suffix_batch(win, m)
            nq = WINDOWS * per
            lo, up = np.zeros(nq, np.uint64), np.zeros(nq, np.uint64)
            pairs, copies = np.zeros((nq, 2), np.uint64), np.zeros(nq, np.uint64)

            def baseline():
                rc = L.rsbwt_set_find_intervals_var(ss._s, pv(stext), pv(soff), nq, pv(lo), pv(up))
                if rc == 0:
                    pairs[:, 0], pairs[:, 1] = lo, up
                    rc = L.rsbwt_debug_dollar_count(g.handle, pv(pairs), nq, pv(copies), None)
                if rc:
                    raise RuntimeError(L.rsbwt_last_error().decode())
            timed("baseline (warm-up)", baseline)
            t_base = [timed("baseline", baseline)[0] for _ in range(RUNS)]
            want = np.zeros((WINDOWS, READ_LEN), np.uint64)
            want[:, :per] = copies.reshape(WINDOWS, per)
            agree = bool((want.ravel() == cnt[0]).all())
            m_host, m_dev, m_base = statistics.median(t_host), statistics.median(t_dev), statistics.median(t_base)
            res["by_min_overlap"][str(m)] = {
                "host_ms": [round(t * 1e3, 3) for t in t_host], "device_ms": [round(t * 1e3, 4) for t in t_dev],
                "baseline_ms": [round(t * 1e3, 3) for t in t_base], "host_median_ms": round(m_host * 1e3, 3),
                "device_median_ms": round(m_dev * 1e3, 4), "baseline_median_ms": round(m_base * 1e3, 3),
                "baseline_over_host_call": round(m_base / m_host, 2), "baseline_queries": int(nq), "baseline_text_bytes": int(soff[-1]),
                "items_per_s_host_call": round(wk["items"] / m_host, 1), "items_per_s_launch": round(wk["items"] / m_dev, 1),
                "lf_steps_per_s_host_call": round(wk["lf_steps"] / m_host, 1), "lf_steps_per_s_launch": round(wk["lf_steps"] / m_dev, 1),
                "lane_passes_per_step": round(wk["passes"] / max(wk["lf_steps"], 1), 4),
                "dollar_only_share_of_passes": round(wk["dollar_only_passes"] / max(wk["passes"], 1), 5),
                "mean_steps_per_item": round(wk["lf_steps"] / max(wk["items"], 1), 2),
                "entries_per_item": round(wk["entries"] / max(wk["items"], 1), 2), "work": wk,
                "device_form_agrees_with_host_form": same_dev, "baseline_agrees_everywhere": agree}
            if not (agree and same_dev):
                raise RuntimeError(f"min_overlap {m}: the call and the baseline disagree")
        res["timing"] = ("host_* and baseline_*: wall clock around the C calls from Python (upload, kernels, copies back); device_*: events "
                         "around the device-resident call's launch alone ({ordinal, count} zeroed and written)")
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
