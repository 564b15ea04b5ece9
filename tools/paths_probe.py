#!/usr/bin/env python3
"""Paths on a population BWT (csrc/paths.hip's paths_kernel, rsbwt_set_paths / _dev): the popBWT of tools/walk_probe.py
(make_reads + bwt_runs of tools/popbwt_gpu.py: haplotypes of a seeded genome, reads of both strands) as ONE shard and dealt
to EIGHT, SEEDS seeds of 31 symbols cut from its reads, walking right at ctx 30, the target the 30 symbols of the seed's own
read that end 60 symbols past the seed, max_steps 200, max_paths 8, max_evals 800, min_count 1, both strands counted.
Per set, ALTERNATING, RUNS runs each, medians: the host-buffer call (wall clock, the eight work counters, states and stops)
and the way to the same answers without the call -- a depth-first host loop over rsbwt_set_extensions, one call per round
for the current nodes of the seeds still searching, the decisions taken in numpy over every seed at once (wall clock) --
whose ext, steps, stop, min_support, npaths and state must agree with the call's for every seed; and, for the launch alone,
the device-resident call between events.  Every step runs under a time limit of its own (a step that outlasts it ends the
process with status 124).  Nothing here asserts a time.
usage: tools/paths_probe.py [seeds=10000] [genome=1e6] [haplotypes=32] [coverage=1] [out=profiles/paths_probe.json]"""
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

SEEDS = int(float(sys.argv[1])) if len(sys.argv) > 1 else 10000
GENOME = int(float(sys.argv[2])) if len(sys.argv) > 2 else 1_000_000
HAPS = int(sys.argv[3]) if len(sys.argv) > 3 else 32
COV = float(sys.argv[4]) if len(sys.argv) > 4 else 1.0
OUT = sys.argv[5] if len(sys.argv) > 5 else os.path.join(ROOT, "profiles", "paths_probe.json")
READ_LEN, RUNS, STEP_LIMIT_S = 100, 5, 120.0
SEED_LEN, CTX, TARGET_LEN, TARGET_ENDS = 31, 30, 30, 60
MAX_STEPS, MAX_PATHS, MAX_EVALS, MIN_COUNT, BOTH = 200, 8, 800, 1, 2  # (flags: both strands, walking right)
BASES = np.frombuffer(b"ACGT", np.uint8)
SAT = 2 ** 32 - 1
DEAD_END, LIMIT, TARGET, BUDGET = 1, 3, 6, 7
STOPS = (("dead_end", DEAD_END), ("limit", LIMIT), ("target", TARGET), ("budget", BUDGET))
STATES = (("complete", 1), ("more", 2), ("budget", 3), ("invalid", 4))


def timed(what, fn):
    guard = threading.Timer(STEP_LIMIT_S, lambda: (sys.stderr.write(f"paths_probe: {what} exceeded {STEP_LIMIT_S} s\n"), os._exit(124)))
    guard.daemon = True
    guard.start()
    try:
        t0 = time.perf_counter()
        out = fn()
        dt = time.perf_counter() - t0
    finally:
        guard.cancel()
    return dt, out


def extensions_dfs(supports, seed_ctx, target, has_target, m=MIN_COUNT, max_steps=MAX_STEPS, max_paths=MAX_PATHS, max_evals=MAX_EVALS):
    """The parent's way, walking right: per round supports(contexts (n, ctx) uint8) -> (n, 4) sums over the shards for the
    seeds still searching; include/rsbwt.h's decisions in numpy over all of them at once.  seed_ctx (Q, ctx) all ACGT,
    target (Q, T), has_target (Q,) bool.  Returns ext, steps, stop, min_support, npaths, state, rounds."""
    Q, ctx = seed_ctx.shape
    T = target.shape[1]
    cap = min(max_steps, max_evals)
    col = np.arange(max_steps)
    path = np.zeros((Q, max_steps), np.uint8)
    steps, evals, npaths, nfr = (np.zeros(Q, np.int64) for _ in range(4))
    least = np.full(Q, SAT, np.uint64)
    f_depth, f_mask = np.zeros((Q, cap), np.int64), np.zeros((Q, cap), np.int64)
    f_least, f_sup = np.zeros((Q, cap), np.uint64), np.zeros((Q, cap, 4), np.uint64)
    ext = np.zeros((Q, max_paths, max_steps), np.uint8)
    o_steps, o_stop = np.zeros((Q, max_paths), np.uint32), np.zeros((Q, max_paths), np.uint8)
    o_least, state = np.zeros((Q, max_paths), np.uint32), np.zeros(Q, np.uint8)

    def contexts(qs):  # the ctx symbols at the right end of seed + path
        full = np.concatenate([seed_ctx[qs], path[qs]], axis=1)
        return np.take_along_axis(full, steps[qs, None] + np.arange(ctx)[None, :], axis=1)

    def end_test(qs):  # (every path here has a symbol)
        at = has_target[qs] & (contexts(qs)[:, ctx - T:] == target[qs]).all(axis=1) if T else np.zeros(qs.size, bool)
        return np.where(at, TARGET, np.where(steps[qs] >= max_steps, LIMIT, np.where(evals[qs] >= max_evals, BUDGET, 0)))

    rounds = 0
    live = np.arange(Q)
    while live.size:
        sup = supports(contexts(live)).astype(np.uint64)
        rounds += 1
        evals[live] += 1
        ok = sup >= np.uint64(m)
        some = ok.any(axis=1)
        stop = np.where(some, 0, DEAD_END)
        adv, pick = live[some], ok[some].argmax(axis=1)
        rest = ok[some].copy()
        rest[np.arange(adv.size), pick] = False
        fork = rest.any(axis=1)
        fq = adv[fork]
        f_depth[fq, nfr[fq]] = steps[fq]
        f_mask[fq, nfr[fq]] = (rest[fork] << np.arange(4)).sum(axis=1)
        f_least[fq, nfr[fq]] = least[fq]
        f_sup[fq, nfr[fq]] = np.minimum(sup[some][fork], np.uint64(SAT))
        nfr[fq] += 1
        path[adv, steps[adv]] = BASES[pick]
        least[adv] = np.minimum(least[adv], np.minimum(sup[some][np.arange(adv.size), pick], np.uint64(SAT)))
        steps[adv] += 1
        stop[some] = end_test(adv)
        out, why = live[stop != 0], stop[stop != 0]
        while out.size:  # a path goes out; the seeds that are not done backtrack and are tested again
            j = npaths[out]
            ext[out, j] = path[out]
            o_steps[out, j], o_stop[out, j] = steps[out], why
            o_least[out, j] = np.where(steps[out] == 0, 0, least[out])
            npaths[out] += 1
            st = np.where(why == BUDGET, 3, np.where(nfr[out] == 0, 1, np.where(npaths[out] >= max_paths, 2, 0)))
            state[out] = st
            bt = out[st == 0]
            if bt.size == 0:
                break
            k = nfr[bt] - 1
            mask = f_mask[bt, k]
            c = ((mask[:, None] >> np.arange(4)) & 1).argmax(axis=1)
            left_over = mask & ~(1 << c)
            d = f_depth[bt, k]
            least[bt] = np.minimum(f_least[bt, k], f_sup[bt, k, c])
            f_mask[bt, k] = left_over
            nfr[bt] -= left_over == 0
            path[bt] = path[bt] * (col[None, :] < d[:, None])
            path[bt, d] = BASES[c]
            steps[bt] = d + 1
            why = end_test(bt)
            out, why = bt[why != 0], why[why != 0]
        live = live[state[live] == 0]
    return ext, o_steps, o_stop, o_least, npaths.astype(np.uint32), state, rounds


def main():
    import torch
    import readserver_amd as rsb
    import popbwt_gpu as P
    reads, _ = P.make_reads(GENOME, HAPS, COV, READ_LEN, 1e-3, 0.0, 5)
    nreads = int(reads.shape[0])
    rng = np.random.default_rng(31)
    pick = torch.from_numpy(rng.integers(0, nreads, SEEDS)).to(reads.device)
    at = int(rng.integers(0, READ_LEN - SEED_LEN - TARGET_ENDS + 1))
    rows = np.frombuffer(b"$ACGT", np.uint8)[reads[pick].cpu().numpy()]
    seeds = rows[:, at:at + SEED_LEN].copy()
    tend = at + SEED_LEN + TARGET_ENDS
    targets = rows[:, tend - TARGET_LEN:tend].copy()
    qs, ts = [s.tobytes() for s in seeds], [t.tobytes() for t in targets]
    L = rsb.lib()
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    pv = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    res = {"reads_indexed": nreads, "seeds": SEEDS, "seed_length": SEED_LEN, "ctx": CTX, "target_length": TARGET_LEN,
           "target_ends_past_the_seed": TARGET_ENDS, "max_steps": MAX_STEPS, "max_paths": MAX_PATHS, "max_evals": MAX_EVALS, "min_count": MIN_COUNT,
           "both_strands": True, "left": False, "runs": RUNS, "by_shards": {}}
    for S in (1, 8):
        gs = []
        for part in range(S):
            sub = reads[part::S].contiguous()
            runs, n, _ = P.bwt_runs(sub)
            gs.append(rsb.GpuBWT(runs=runs.cpu().numpy(), num_strings=int(sub.shape[0])))
        ss = rsb.ShardSet(gs)
        try:
            text, off = ss._var_text(qs)
            ttext, toff = ss._var_text(ts)
            shape = (SEEDS, MAX_PATHS)
            ext = np.zeros(shape + (MAX_STEPS,), np.uint8)
            steps, stop, least = np.zeros(shape, np.uint32), np.zeros(shape, np.uint8), np.zeros(shape, np.uint32)
            npaths, state = np.zeros(SEEDS, np.uint32), np.zeros(SEEDS, np.uint8)

            def host():
                rc = L.rsbwt_set_paths(ss._s, pv(text), pv(off), SEEDS, pv(ttext), pv(toff), CTX, MIN_COUNT, MAX_STEPS, MAX_PATHS, MAX_EVALS, BOTH,
                                       pv(ext), pv(steps), pv(stop), pv(least), pv(npaths), pv(state))
                if rc:
                    raise RuntimeError(L.rsbwt_last_error().decode())

            def supports(ctxs):
                n = ctxs.shape[0]
                o = np.arange(0, (n + 1) * CTX, CTX, dtype=np.uint64)
                cnt = np.zeros((S, n, 4), np.uint64)
                rc = L.rsbwt_set_extensions(ss._s, pv(np.append(ctxs.ravel(), np.uint8(0))), pv(o), n, CTX, BOTH, pv(cnt))
                if rc:
                    raise RuntimeError(L.rsbwt_last_error().decode())
                return cnt.sum(axis=0)

            def loop(n=SEEDS):
                return extensions_dfs(supports, seeds[:n, SEED_LEN - CTX:].copy(), targets[:n], np.ones(n, bool))
            timed("host call (warm-up)", host)
            timed("extensions loop (warm-up)", lambda: loop(64))
            t_host, t_base, base = [], [], None
            for _ in range(RUNS):  # alternating
                t_host.append(timed("host call", host)[0])
                dt, base = timed("extensions loop", loop)
                t_base.append(dt)
            wk = rsb.ShardSet.paths_last_work()
            agree = bool((base[0] == ext).all() and (base[1] == steps).all() and (base[2] == stop).all() and (base[3] == least).all()
                         and (base[4] == npaths).all() and (base[5] == state).all())
            d_text, d_off = torch.from_numpy(text).cuda(), torch.from_numpy(off.view(np.int64)).cuda()
            d_tt, d_toff = torch.from_numpy(ttext).cuda(), torch.from_numpy(toff.view(np.int64)).cuda()
            slots = SEEDS * MAX_PATHS
            d_ext = torch.zeros(slots * MAX_STEPS, dtype=torch.uint8, device="cuda")
            d_steps, d_stop = torch.zeros(slots, dtype=torch.int32, device="cuda"), torch.zeros(slots, dtype=torch.uint8, device="cuda")
            d_least, d_np = torch.zeros(slots, dtype=torch.int32, device="cuda"), torch.zeros(SEEDS, dtype=torch.int32, device="cuda")
            d_state = torch.zeros(SEEDS, dtype=torch.uint8, device="cuda")

            def launch():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                rc = L.rsbwt_set_paths_dev(ss._s, p(d_text), p(d_off), SEEDS, int(off[-1]), p(d_tt), p(d_toff), int(toff[-1]), CTX, MIN_COUNT,
                                           MAX_STEPS, MAX_PATHS, MAX_EVALS, BOTH, p(d_ext), p(d_steps), p(d_stop), p(d_least), p(d_np), p(d_state), None)
                e1.record()
                torch.cuda.synchronize()
                if rc:
                    raise RuntimeError(L.rsbwt_last_error().decode())
                return e0.elapsed_time(e1) * 1e-3
            timed("device call (warm-up)", launch)
            t_dev = [timed("device call", launch)[1] for _ in range(RUNS)]
            same_dev = bool((d_ext.cpu().numpy().reshape(ext.shape) == ext).all() and (d_steps.cpu().numpy().view(np.uint32).reshape(shape) == steps).all()
                            and (d_stop.cpu().numpy().reshape(shape) == stop).all() and (d_np.cpu().numpy().view(np.uint32) == npaths).all()
                            and (d_state.cpu().numpy() == state).all())
            m_host, m_dev, m_base = (statistics.median(t) for t in (t_host, t_dev, t_base))
            used = np.arange(MAX_PATHS)[None, :] < npaths[:, None]
            res["by_shards"][str(S)] = {
                "symbols": int(sum(g.getBWLen() for g in gs)), "ktab_depth": gs[0].ktab_depth(), "window_span": gs[0].window_span(),
                "host_ms": [round(t * 1e3, 3) for t in t_host], "extensions_loop_ms": [round(t * 1e3, 3) for t in t_base],
                "device_ms": [round(t * 1e3, 4) for t in t_dev],
                "host_median_ms": round(m_host * 1e3, 3), "extensions_loop_median_ms": round(m_base * 1e3, 3),
                "device_median_ms": round(m_dev * 1e3, 4), "extensions_loop_over_host_call": round(m_base / m_host, 2),
                "extensions_calls": int(base[6]),
                "states": {k: int((state == v).sum()) for k, v in STATES},
                "paths_by_stop": {k: int(((stop == v) & used).sum()) for k, v in STOPS},
                "seeds_with_two_or_more_target_paths": int((((stop == TARGET) & used).sum(axis=1) >= 2).sum()),
                "mean_paths_per_seed": round(float(npaths.mean()), 3), "mean_evals_per_seed": round(wk["evals"] / SEEDS, 2),
                "lf_steps_per_s_host_call": round(wk["lf_steps"] / m_host, 1), "lf_steps_per_s_launch": round(wk["lf_steps"] / m_dev, 1),
                "lane_passes_per_step": round(wk["passes"] / max(wk["lf_steps"], 1), 4),
                "lf_steps_per_search": round(wk["lf_steps"] / max(wk["searches"], 1), 2), "work": wk,
                "device_form_agrees_with_host_form": same_dev, "extensions_loop_agrees_for_every_seed": agree}
            if not (agree and same_dev):
                raise RuntimeError(f"{S} shards: the call and the extensions loop disagree")
        finally:
            ss.close()
            for g in gs:
                g.close()
    res["timing"] = ("host_* and extensions_loop_*: wall clock round the C calls from Python (upload, kernels, copies back; the loop's numpy "
                     "included), the two alternating; device_*: events round the device-resident call's launch alone (outputs zeroed, every "
                     "output written)")
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
