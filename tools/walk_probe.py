#!/usr/bin/env python3
"""Walks on a population BWT (csrc/walk.hip, rsbwt_set_walk / _dev): the popBWT of tools/overlap_probe.py (make_reads +
bwt_runs of tools/popbwt_gpu.py: haplotypes of a seeded genome, reads of both strands) as ONE shard and dealt to EIGHT,
SEEDS seeds of 31 symbols cut from its reads (each read is a window of a haplotype, on either strand), ctx 30, max_steps
200, min_count 1, both strands counted.  Per set, as medians of RUNS: the host-buffer call (wall clock, work counters),
the device-resident call (events round the launch alone), and the way to the same answers without the call -- a host loop
of rsbwt_set_count_var over the candidates of the seeds still walking, one call (two with both strands) per step, the rule
applied in numpy (wall clock) -- whose ext, steps and stop must agree with the call's everywhere.  Every step runs under a
time limit of its own (a step that outlasts it ends the process with status 124).
usage: tools/walk_probe.py [seeds=10000] [genome=1e6] [haplotypes=32] [coverage=1] [out=profiles/walk_probe.json]"""
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

SEEDS = int(float(sys.argv[1])) if len(sys.argv) > 1 else 10000
GENOME = int(float(sys.argv[2])) if len(sys.argv) > 2 else 1_000_000
HAPS = int(sys.argv[3]) if len(sys.argv) > 3 else 32
COV = float(sys.argv[4]) if len(sys.argv) > 4 else 1.0
OUT = sys.argv[5] if len(sys.argv) > 5 else os.path.join(ROOT, "profiles", "walk_probe.json")
READ_LEN, RUNS, STEP_LIMIT_S = 100, 5, 120.0
SEED_LEN, CTX, MAX_STEPS, MIN_COUNT, FLAGS = 31, 30, 200, 1, 2  # (flags: both strands, to the right)
COMP = np.zeros(256, np.uint8)
COMP[list(b"ACGT")] = list(b"TGCA")
BASES = np.frombuffer(b"ACGT", np.uint8)


def timed(what, fn):
    guard = threading.Timer(STEP_LIMIT_S, lambda: (sys.stderr.write(f"walk_probe: {what} exceeded {STEP_LIMIT_S} s\n"), os._exit(124)))
    guard.daemon = True
    guard.start()
    try:
        t0 = time.perf_counter()
        out = fn()
        dt = time.perf_counter() - t0
    finally:
        guard.cancel()
    return dt, out


def count_var_loop(L, ss, seeds):
    """the parent's way: per step, the candidates of the seeds still walking spelled out, rsbwt_set_count_var of them (and of
    their reverse complements), the sums over the shards come back, the rule is applied on the host"""
    pv = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    Q = seeds.shape[0]
    ext, steps, stop = np.zeros((Q, MAX_STEPS), np.uint8), np.zeros(Q, np.uint32), np.zeros(Q, np.uint8)
    ctx = seeds[:, SEED_LEN - CTX:].copy()
    live = np.arange(Q)
    calls = 0
    for it in range(MAX_STEPS):
        if live.size == 0:
            break
        n = live.size
        cand = np.empty((n, 4, CTX + 1), np.uint8)
        cand[:, :, :CTX] = ctx[live][:, None, :]
        cand[:, :, CTX] = BASES[None, :]
        off = np.arange(0, (4 * n + 1) * (CTX + 1), CTX + 1, dtype=np.uint64)
        sup = np.zeros(4 * n, np.uint64)
        for text in (cand, COMP[cand[:, :, ::-1]]):
            cnt = np.zeros(4 * n, np.uint64)
            flat = np.append(text.ravel(), np.uint8(0))
            rc = L.rsbwt_set_count_var(ss._s, pv(flat), pv(off), 4 * n, pv(cnt))
            if rc:
                raise RuntimeError(L.rsbwt_last_error().decode())
            sup += cnt
            calls += 1
        ok = sup.reshape(n, 4) >= MIN_COUNT
        nlive = ok.sum(axis=1)
        go = nlive == 1
        pick = ok.argmax(axis=1)
        stop[live[~go]] = np.where(nlive[~go] == 0, 1, 2)
        on = live[go]
        ext[on, it] = BASES[pick[go]]
        steps[on] = it + 1
        ctx[on, :-1] = ctx[on, 1:]
        ctx[on, -1] = BASES[pick[go]]
        live = on
    stop[live] = 3
    return ext, steps, stop, calls


def main():
    import torch
    import popbwt_gpu as P
    reads, _ = P.make_reads(GENOME, HAPS, COV, READ_LEN, 1e-3, 0.0, 5)
    nreads = int(reads.shape[0])
    rng = np.random.default_rng(31)
    pick = torch.from_numpy(rng.integers(0, nreads, SEEDS)).to(reads.device)
    at = int(rng.integers(0, READ_LEN - SEED_LEN - 1))
    seeds = np.frombuffer(b"$ACGT", np.uint8)[reads[pick][:, at:at + SEED_LEN].cpu().numpy()].copy()
    qs = [s.tobytes() for s in seeds]
    L = rsb.lib()
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    res = {"reads_indexed": nreads, "seeds": SEEDS, "seed_length": SEED_LEN, "ctx": CTX, "max_steps": MAX_STEPS, "min_count": MIN_COUNT,
           "both_strands": True, "runs": RUNS, "by_shards": {}}
    for S in (1, 8):
        gs = []
        for part in range(S):
            sub = reads[part::S].contiguous()
            runs, n, _ = P.bwt_runs(sub)
            gs.append(rsb.GpuBWT(runs=runs.cpu().numpy(), num_strings=int(sub.shape[0])))
        ss = rsb.ShardSet(gs)
        try:
            timed("host call (warm-up)", lambda: ss.walk(qs[:64], CTX, MIN_COUNT, MAX_STEPS, both_strands=True))
            text, off = ss._var_text(qs)
            pv = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
            ext, steps, stop = np.zeros((SEEDS, MAX_STEPS), np.uint8), np.zeros(SEEDS, np.uint32), np.zeros(SEEDS, np.uint8)

            def host():
                rc = L.rsbwt_set_walk(ss._s, pv(text), pv(off), SEEDS, CTX, MIN_COUNT, MAX_STEPS, FLAGS, pv(ext), pv(steps), pv(stop), None, None)
                if rc:
                    raise RuntimeError(L.rsbwt_last_error().decode())
            timed("host call (warm-up)", host)
            t_host = [timed("host call", host)[0] for _ in range(RUNS)]
            wk = rsb.ShardSet.walk_last_work()
            d_text, d_off = torch.from_numpy(text).cuda(), torch.from_numpy(off.view(np.int64)).cuda()
            d_ext = torch.zeros(SEEDS * MAX_STEPS, dtype=torch.uint8, device="cuda")
            d_steps, d_stop = torch.zeros(SEEDS, dtype=torch.int32, device="cuda"), torch.zeros(SEEDS, dtype=torch.uint8, device="cuda")

            def launch():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                rc = L.rsbwt_set_walk_dev(ss._s, p(d_text), p(d_off), SEEDS, int(off[-1]), CTX, MIN_COUNT, MAX_STEPS, FLAGS, p(d_ext), p(d_steps),
                                          p(d_stop), None, None, None)
                e1.record()
                torch.cuda.synchronize()
                if rc:
                    raise RuntimeError(L.rsbwt_last_error().decode())
                return e0.elapsed_time(e1) * 1e-3
            timed("device call (warm-up)", launch)
            t_dev = [timed("device call", launch)[1] for _ in range(RUNS)]
            same_dev = bool((d_ext.cpu().numpy().reshape(SEEDS, MAX_STEPS) == ext).all() and (d_steps.cpu().numpy().view(np.uint32) == steps).all()
                            and (d_stop.cpu().numpy() == stop).all())
            timed("count_var loop (warm-up)", lambda: count_var_loop(L, ss, seeds[:64]))
            t_base, base = [], None
            for _ in range(RUNS):
                dt, base = timed("count_var loop", lambda: count_var_loop(L, ss, seeds))
                t_base.append(dt)
            agree = bool((base[0] == ext).all() and (base[1] == steps).all() and (base[2] == stop).all())
            m_host, m_dev, m_base = statistics.median(t_host), statistics.median(t_dev), statistics.median(t_base)
            res["by_shards"][str(S)] = {
                "symbols": int(sum(g.getBWLen() for g in gs)), "ktab_depth": gs[0].ktab_depth(), "window_span": gs[0].window_span(),
                "host_ms": [round(t * 1e3, 3) for t in t_host], "device_ms": [round(t * 1e3, 4) for t in t_dev],
                "count_var_loop_ms": [round(t * 1e3, 3) for t in t_base], "host_median_ms": round(m_host * 1e3, 3),
                "device_median_ms": round(m_dev * 1e3, 4), "count_var_loop_median_ms": round(m_base * 1e3, 3),
                "count_var_loop_over_host_call": round(m_base / m_host, 2), "count_var_calls": int(base[3]),
                "stops": {k: int((stop == v).sum()) for k, v in (("dead_end", 1), ("branch", 2), ("limit", 3), ("invalid", 4))},
                "mean_steps_per_seed": round(float(steps.mean()), 2),
                "lf_steps_per_s_host_call": round(wk["lf_steps"] / m_host, 1), "lf_steps_per_s_launch": round(wk["lf_steps"] / m_dev, 1),
                "lane_passes_per_step": round(wk["passes"] / max(wk["lf_steps"], 1), 4),
                "lf_steps_per_search": round(wk["lf_steps"] / max(wk["searches"], 1), 2),
                "us_per_walk_step_launch": round(m_dev * 1e6 / MAX_STEPS, 2), "work": wk,
                "device_form_agrees_with_host_form": same_dev, "count_var_loop_agrees_everywhere": agree}
            if not (agree and same_dev):
                raise RuntimeError(f"{S} shards: the call and the count_var loop disagree")
        finally:
            ss.close()
            for g in gs:
                g.close()
    res["timing"] = ("host_* and count_var_loop_*: wall clock round the C calls from Python (upload, kernels, copies back; the loop's numpy "
                     "included); device_*: events round the device-resident call's launch alone (ext zeroed, every output written)")
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
