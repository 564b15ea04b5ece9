#!/usr/bin/env python3
"""Unitigs on a population BWT (csrc/walk.hip's unitig_kernel, rsbwt_set_unitigs / _dev): the popBWT of tools/walk_probe.py
(make_reads + bwt_runs of tools/popbwt_gpu.py: haplotypes of a seeded genome, reads of both strands) as ONE shard and dealt
to EIGHT, SEEDS seeds of 31 symbols cut from its reads, ctx 30, max_steps 200 per side, min_count 1, both strands counted.
Per set, as medians of RUNS: the host-buffer call (wall clock, the eight work counters, the stops per side), the
device-resident call (events round the launch alone), the way to the same answers without the call -- a host loop of
rsbwt_set_extensions, per step and direction one call for the onward contexts and one for the nodes entered, the rule
applied in numpy (wall clock) -- whose ext, steps and stop must agree with the call's for every item, and, for scale,
rsbwt_set_walk to the right plus to the left on the same seeds.  Every step runs under a time limit of its own (a step
that outlasts it ends the process with status 124).
usage: tools/unitig_probe.py [seeds=10000] [genome=1e6] [haplotypes=32] [coverage=1] [out=profiles/unitig_probe.json]"""
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
OUT = sys.argv[5] if len(sys.argv) > 5 else os.path.join(ROOT, "profiles", "unitig_probe.json")
READ_LEN, RUNS, STEP_LIMIT_S = 100, 5, 120.0
SEED_LEN, CTX, MAX_STEPS, MIN_COUNT, BOTH = 31, 30, 200, 1, 2  # (flags: both strands)
BASES = np.frombuffer(b"ACGT", np.uint8)
STOPS = (("dead_end", 1), ("branch", 2), ("limit", 3), ("invalid", 4), ("join", 5))


def timed(what, fn):
    guard = threading.Timer(STEP_LIMIT_S, lambda: (sys.stderr.write(f"unitig_probe: {what} exceeded {STEP_LIMIT_S} s\n"), os._exit(124)))
    guard.daemon = True
    guard.start()
    try:
        t0 = time.perf_counter()
        out = fn()
        dt = time.perf_counter() - t0
    finally:
        guard.cancel()
    return dt, out


def supports(L, ss, ctxs, left):
    """the four supports of every row of `ctxs` (n, CTX) in one direction: rsbwt_set_extensions summed over the shards"""
    pv = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    n = ctxs.shape[0]
    off = np.arange(0, (n + 1) * CTX, CTX, dtype=np.uint64)
    cnt = np.zeros((len(ss.shards), n, 4), np.uint64)
    rc = L.rsbwt_set_extensions(ss._s, pv(np.append(ctxs.ravel(), np.uint8(0))), pv(off), n, CTX, BOTH | (1 if left else 0), pv(cnt))
    if rc:
        raise RuntimeError(L.rsbwt_last_error().decode())
    return cnt.sum(axis=0)


def extensions_loop(L, ss, seeds):
    """the parent's way: per step and direction the onward contexts of the sides still walking go to rsbwt_set_extensions,
    the rule is applied on the host, the nodes entered go to rsbwt_set_extensions in the opposite direction, the host
    decides"""
    Q = seeds.shape[0]
    ext, steps, stop = np.zeros((Q, 2, MAX_STEPS), np.uint8), np.zeros((Q, 2), np.uint32), np.zeros((Q, 2), np.uint8)
    calls = 0
    for d, left in enumerate((False, True)):
        ctx = (seeds[:, :CTX] if left else seeds[:, SEED_LEN - CTX:]).copy()
        live = np.arange(Q)
        for it in range(MAX_STEPS):
            if live.size == 0:
                break
            ok = supports(L, ss, ctx[live], left) >= MIN_COUNT
            calls += 1
            nlive = ok.sum(axis=1)
            go = nlive == 1
            pick = BASES[ok.argmax(axis=1)]
            stop[live[~go], d] = np.where(nlive[~go] == 0, 1, 2)
            on = live[go]
            if on.size == 0:
                live = on
                break
            node = np.empty((on.size, CTX), np.uint8)
            if left:
                node[:, 1:], node[:, 0] = ctx[on, :-1], pick[go]
            else:
                node[:, :-1], node[:, -1] = ctx[on, 1:], pick[go]
            join = (supports(L, ss, node, not left) >= MIN_COUNT).sum(axis=1) >= 2
            calls += 1
            stop[on[join], d] = 5
            on, node, sym = on[~join], node[~join], pick[go][~join]
            ext[on, d, it] = sym
            steps[on, d] = it + 1
            ctx[on] = node
            live = on
        stop[live, d] = 3
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
    pv = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    res = {"reads_indexed": nreads, "seeds": SEEDS, "seed_length": SEED_LEN, "ctx": CTX, "max_steps_per_side": MAX_STEPS, "min_count": MIN_COUNT,
           "both_strands": True, "runs": RUNS, "by_shards": {}}
    for S in (1, 8):
        gs = []
        for part in range(S):
            sub = reads[part::S].contiguous()
            runs, n, _ = P.bwt_runs(sub)
            gs.append(rsb.GpuBWT(runs=runs.cpu().numpy(), num_strings=int(sub.shape[0])))
        ss = rsb.ShardSet(gs)
        try:
            timed("host call (warm-up)", lambda: ss.unitigs(qs[:64], CTX, MIN_COUNT, MAX_STEPS, both_strands=True))
            text, off = ss._var_text(qs)
            ext, steps, stop = np.zeros((SEEDS, 2, MAX_STEPS), np.uint8), np.zeros((SEEDS, 2), np.uint32), np.zeros((SEEDS, 2), np.uint8)

            def host():
                rc = L.rsbwt_set_unitigs(ss._s, pv(text), pv(off), SEEDS, CTX, MIN_COUNT, MAX_STEPS, BOTH, pv(ext), pv(steps), pv(stop), None, None)
                if rc:
                    raise RuntimeError(L.rsbwt_last_error().decode())
            timed("host call (warm-up)", host)
            t_host = [timed("host call", host)[0] for _ in range(RUNS)]
            wk = rsb.ShardSet.unitigs_last_work()
            d_text, d_off = torch.from_numpy(text).cuda(), torch.from_numpy(off.view(np.int64)).cuda()
            d_ext = torch.zeros(2 * SEEDS * MAX_STEPS, dtype=torch.uint8, device="cuda")
            d_steps, d_stop = torch.zeros(2 * SEEDS, dtype=torch.int32, device="cuda"), torch.zeros(2 * SEEDS, dtype=torch.uint8, device="cuda")

            def launch():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                rc = L.rsbwt_set_unitigs_dev(ss._s, p(d_text), p(d_off), SEEDS, int(off[-1]), CTX, MIN_COUNT, MAX_STEPS, BOTH, p(d_ext), p(d_steps),
                                             p(d_stop), None, None, None)
                e1.record()
                torch.cuda.synchronize()
                if rc:
                    raise RuntimeError(L.rsbwt_last_error().decode())
                return e0.elapsed_time(e1) * 1e-3
            timed("device call (warm-up)", launch)
            t_dev = [timed("device call", launch)[1] for _ in range(RUNS)]
            same_dev = bool((d_ext.cpu().numpy().reshape(ext.shape) == ext).all() and (d_steps.cpu().numpy().view(np.uint32).reshape(steps.shape) == steps).all()
                            and (d_stop.cpu().numpy().reshape(stop.shape) == stop).all())
            timed("extensions loop (warm-up)", lambda: extensions_loop(L, ss, seeds[:64]))
            t_base, base = [], None
            for _ in range(RUNS):
                dt, base = timed("extensions loop", lambda: extensions_loop(L, ss, seeds))
                t_base.append(dt)
            agree = bool((base[0] == ext).all() and (base[1] == steps).all() and (base[2] == stop).all())
            # for scale: today's walks of the same seeds, to the right and to the left
            w_ext, w_steps, w_stop = np.zeros((SEEDS, MAX_STEPS), np.uint8), np.zeros(SEEDS, np.uint32), np.zeros(SEEDS, np.uint8)
            walk_steps = []

            def walks():
                walk_steps.clear()
                for flags in (BOTH, BOTH | 1):
                    rc = L.rsbwt_set_walk(ss._s, pv(text), pv(off), SEEDS, CTX, MIN_COUNT, MAX_STEPS, flags, pv(w_ext), pv(w_steps), pv(w_stop), None, None)
                    if rc:
                        raise RuntimeError(L.rsbwt_last_error().decode())
                    walk_steps.append(w_steps.copy())
            timed("two walks (warm-up)", walks)
            t_walks = [timed("two walks", walks)[0] for _ in range(RUNS)]
            through = [int((walk_steps[d] > steps[:, d]).sum()) for d in (0, 1)]
            m_host, m_dev, m_base, m_walks = (statistics.median(t) for t in (t_host, t_dev, t_base, t_walks))
            res["by_shards"][str(S)] = {
                "symbols": int(sum(g.getBWLen() for g in gs)), "ktab_depth": gs[0].ktab_depth(), "window_span": gs[0].window_span(),
                "host_ms": [round(t * 1e3, 3) for t in t_host], "device_ms": [round(t * 1e3, 4) for t in t_dev],
                "extensions_loop_ms": [round(t * 1e3, 3) for t in t_base], "two_walks_ms": [round(t * 1e3, 3) for t in t_walks],
                "host_median_ms": round(m_host * 1e3, 3), "device_median_ms": round(m_dev * 1e3, 4),
                "extensions_loop_median_ms": round(m_base * 1e3, 3), "two_walks_median_ms": round(m_walks * 1e3, 3),
                "extensions_loop_over_host_call": round(m_base / m_host, 2), "host_call_over_two_walks": round(m_host / m_walks, 2),
                "extensions_calls": int(base[3]),
                "stops": {side: {k: int((stop[:, d] == v).sum()) for k, v in STOPS} for d, side in enumerate(("right", "left"))},
                "walks_that_run_on_past_the_unitig": {"right": through[0], "left": through[1]},
                "mean_steps_per_side": round(float(steps.mean()), 2),
                "lf_steps_per_s_host_call": round(wk["lf_steps"] / m_host, 1), "lf_steps_per_s_launch": round(wk["lf_steps"] / m_dev, 1),
                "lane_passes_per_step": round(wk["passes"] / max(wk["lf_steps"], 1), 4),
                "lf_steps_per_search": round(wk["lf_steps"] / max(wk["searches"], 1), 2), "work": wk,
                "device_form_agrees_with_host_form": same_dev, "extensions_loop_agrees_for_every_item": agree}
            if not (agree and same_dev):
                raise RuntimeError(f"{S} shards: the call and the extensions loop disagree")
        finally:
            ss.close()
            for g in gs:
                g.close()
    res["timing"] = ("host_*, extensions_loop_* and two_walks_*: wall clock round the C calls from Python (upload, kernels, copies back; the "
                     "loop's numpy included); device_*: events round the device-resident call's launch alone (ext zeroed, every output written)")
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
