#!/usr/bin/env python3
"""Sample walks on a population BWT (csrc/sample_walk.hip, rsbwt_set_walk_samples / _dev): the popBWT of tools/walk_probe.py
(make_reads + bwt_runs of tools/popbwt_gpu.py) as ONE shard and dealt to EIGHT, a sample table like
tools/site_counts_probe.py's (SAMPLES samples, nine reads in ten with 1-3 records of 4 bytes), SEEDS seeds of 31 symbols cut
from the reads, ctx 30, max_steps 200, min_count 1, both strands, max_rows 256.  Two masks: one sample, and 100 samples.
Per set and mask, as medians of RUNS: the host-buffer call (wall clock, work counters), the device-resident call (events
round everything it enqueues), and the way to the same answers without the call -- a host loop of rsbwt_set_sample_counts over
the candidates of the seeds still walking, the masked columns added and the rule applied in numpy (wall clock) -- whose ext,
steps and stop must agree with the call's everywhere.  Every step runs under a time limit of its own (a step that outlasts
it ends the process with status 124).
usage: tools/sample_walk_probe.py [seeds=500] [samples=2000] [genome=1e6] [haplotypes=32] [coverage=1] [out=profiles/sample_walk_probe.json]"""
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

SEEDS = int(float(sys.argv[1])) if len(sys.argv) > 1 else 500
SAMPLES = int(float(sys.argv[2])) if len(sys.argv) > 2 else 2000
GENOME = int(float(sys.argv[3])) if len(sys.argv) > 3 else 1_000_000
HAPS = int(sys.argv[4]) if len(sys.argv) > 4 else 32
COV = float(sys.argv[5]) if len(sys.argv) > 5 else 1.0
OUT = sys.argv[6] if len(sys.argv) > 6 else os.path.join(ROOT, "profiles", "sample_walk_probe.json")
READ_LEN, RUNS, STEP_LIMIT_S, RECORD = 100, 3, 150.0, 4
SEED_LEN, CTX, MAX_STEPS, MIN_COUNT, FLAGS, MAX_ROWS = 31, 30, 200, 1, 2, 256
COMP = np.zeros(256, np.uint8)
COMP[list(b"ACGT")] = list(b"TGCA")
BASES = np.frombuffer(b"ACGT", np.uint8)


def timed(what, fn):
    guard = threading.Timer(STEP_LIMIT_S, lambda: (sys.stderr.write(f"sample_walk_probe: {what} exceeded {STEP_LIMIT_S} s\n"), os._exit(124)))
    guard.daemon = True
    guard.start()
    try:
        t0 = time.perf_counter()
        out = fn()
        dt = time.perf_counter() - t0
    finally:
        guard.cancel()
    return dt, out


def sample_counts_loop(L, ss, seeds, flat, mask):
    """what the call replaces: per step, the candidates of the seeds still walking and their reverse complements spelled out,
    ONE rsbwt_set_sample_counts over all of them, the masked columns of strings[] added, the WIDE rule and the walk's rule
    applied on the host"""
    pv = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    Q = seeds.shape[0]
    cols = np.flatnonzero(mask[:SAMPLES])
    ext, steps, stop = np.zeros((Q, MAX_STEPS), np.uint8), np.zeros(Q, np.uint32), np.zeros(Q, np.uint8)
    ctx = seeds[:, SEED_LEN - CTX:].copy()
    live = np.arange(Q)
    calls = 0
    for it in range(MAX_STEPS):
        if live.size == 0:
            break
        n = live.size
        cand = np.empty((n, 4, 2, CTX + 1), np.uint8)
        cand[:, :, 0, :CTX] = ctx[live][:, None, :]
        cand[:, :, 0, CTX] = BASES[None, :]
        cand[:, :, 1, :] = COMP[cand[:, :, 0, ::-1]]
        off = np.arange(0, (8 * n + 1) * (CTX + 1), CTX + 1, dtype=np.uint64)
        strings = np.zeros((8 * n, SAMPLES + 1), np.uint32)
        matches = np.zeros(8 * n, np.uint64)
        text = np.append(cand.ravel(), np.uint8(0))
        rc = L.rsbwt_set_sample_counts(ss._s, pv(text), pv(off), 8 * n, pv(flat), SAMPLES, 2, 1, MAX_ROWS, 0, pv(strings), None, pv(matches), None)
        if rc:
            raise RuntimeError(L.rsbwt_last_error().decode())
        calls += 1
        wide = (matches.reshape(n, 8) > MAX_ROWS).any(axis=1)
        sup = strings[:, cols].sum(axis=1, dtype=np.uint64).reshape(n, 4, 2).sum(axis=2)
        ok = sup >= MIN_COUNT
        nlive = ok.sum(axis=1)
        go = (nlive == 1) & ~wide
        pick = ok.argmax(axis=1)
        stop[live[~go]] = np.where(wide[~go], 8, np.where(nlive[~go] == 0, 1, 2))
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
    R = int(reads.shape[0])
    rng = np.random.default_rng(31)
    pick = torch.from_numpy(rng.integers(0, R, SEEDS)).to(reads.device)
    at = int(rng.integers(0, READ_LEN - SEED_LEN - 1))
    sym = np.frombuffer(b"$ACGT", np.uint8)
    seeds = sym[reads[pick][:, at:at + SEED_LEN].cpu().numpy()].copy()
    qs = [s.tobytes() for s in seeds]
    L = rsb.lib()
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    pv = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    chk = lambda rc: rc == 0 or (_ for _ in ()).throw(RuntimeError(L.rsbwt_last_error().decode()))  # noqa: E731
    # the sample table: nine reads in ten get a value of 1-3 records (site_counts_probe.py's)
    host_reads = sym[reads.cpu().numpy()]
    named = np.flatnonzero(rng.random(R) < 0.9)
    ntext = np.append(host_reads[named].ravel(), np.uint8(0))
    noff = np.arange(named.size + 1, dtype=np.uint64) * np.uint64(READ_LEN)
    codes = (np.arange(SAMPLES, dtype=np.uint32) * 7 + 3).astype(">u2")
    flat = np.append(codes.view(np.uint8), np.uint8(0))
    keys = np.zeros(SAMPLES, np.uint64)
    chk(L.rsbwt_sample_keys(pv(flat), SAMPLES, 2, pv(keys)))
    nrec = rng.integers(1, 4, named.size).astype(np.int64)
    voff = np.zeros(named.size + 1, np.uint64)
    voff[1:] = np.cumsum(nrec * RECORD, dtype=np.uint64)
    total_rec = int(nrec.sum())
    rec = np.zeros((total_rec, RECORD), np.uint8)
    rec[:, :2] = codes[rng.integers(0, SAMPLES, total_rec)].view(np.uint8).reshape(-1, 2)
    rec[:, 2] = 33 + rng.integers(0, 6, total_rec)
    rec[:, 3] = 33 + rng.integers(0, 40, total_rec)
    values = np.append(rec.ravel(), np.uint8(0))
    masks = {}
    one = np.zeros(SAMPLES + 1, np.uint8)
    one[int(rng.integers(0, SAMPLES))] = 1
    masks["one_sample"] = one
    hundred = np.zeros(SAMPLES + 1, np.uint8)
    hundred[rng.choice(SAMPLES, min(100, SAMPLES), replace=False)] = 1
    masks["hundred_samples"] = hundred
    res = {"reads_indexed": R, "samples": SAMPLES, "records": total_rec, "seeds": SEEDS, "seed_length": SEED_LEN, "ctx": CTX, "max_steps": MAX_STEPS,
           "min_count": MIN_COUNT, "both_strands": True, "max_rows": MAX_ROWS, "runs": RUNS, "launches_per_step": 7, "by_shards": {}}
    for S in (1, 8):
        gs = []
        for part in range(S):
            sub = reads[part::S].contiguous()
            runs, n, _ = P.bwt_runs(sub)
            gs.append(rsb.GpuBWT(runs=runs.cpu().numpy(), num_strings=int(sub.shape[0])))
        ss = rsb.ShardSet(gs)
        try:
            st = np.zeros(4, np.uint64)
            chk(L.rsbwt_set_meta_build(ss._s, pv(ntext), pv(noff), pv(values), pv(voff), named.size, pv(st)))
            text, off = ss._var_text(qs)
            d_text, d_off = torch.from_numpy(text).cuda(), torch.from_numpy(off.view(np.int64)).cuda()
            d_keys = torch.from_numpy(keys.view(np.int64)).cuda()
            per_mask = {}
            for name, mask in masks.items():
                ext, steps, stop = np.zeros((SEEDS, MAX_STEPS), np.uint8), np.zeros(SEEDS, np.uint32), np.zeros(SEEDS, np.uint8)

                def host():
                    chk(L.rsbwt_set_walk_samples(ss._s, pv(text), pv(off), SEEDS, CTX, MIN_COUNT, MAX_STEPS, FLAGS, pv(flat), SAMPLES, 2, 1, pv(mask),
                                                 MAX_ROWS, 0, pv(ext), pv(steps), pv(stop), None, None))
                timed("host call (warm-up)", host)
                t_host = [timed("host call", host)[0] for _ in range(RUNS)]
                wk = rsb.ShardSet.walk_samples_last_work()
                # one more call with an event round every launch: where the call's device time goes, by kind of launch
                os.environ["RSBWT_SAMPLE_WALK_TIMES"] = "1"
                try:
                    t_marked = timed("host call (events)", host)[0]
                    by_launch = {k: round(v, 3) for k, v in rsb.ShardSet.walk_samples_last_times().items()}
                finally:
                    del os.environ["RSBWT_SAMPLE_WALK_TIMES"]
                d_mask =torch.from_numpy(mask[:SAMPLES].copy()).cuda()
                d_ext = torch.zeros(SEEDS * MAX_STEPS, dtype=torch.uint8, device="cuda")
                d_steps, d_stop = torch.zeros(SEEDS, dtype=torch.int32, device="cuda"), torch.zeros(SEEDS, dtype=torch.uint8, device="cuda")
                d_status = torch.zeros(8, dtype=torch.int64, device="cuda")

                def launch():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    rc = L.rsbwt_set_walk_samples_dev(ss._s, p(d_text), p(d_off), SEEDS, int(off[-1]), CTX, MIN_COUNT, MAX_STEPS, FLAGS, p(d_keys), SAMPLES,
                                                      2, 1, p(d_mask), MAX_ROWS, 0, p(d_ext), p(d_steps), p(d_stop), None, None, p(d_status), None)
                    e1.record()
                    torch.cuda.synchronize()
                    chk(rc)
                    return e0.elapsed_time(e1) * 1e-3
                timed("device call (warm-up)", launch)
                t_dev = [timed("device call", launch)[1] for _ in range(RUNS)]
                same_dev = bool((d_ext.cpu().numpy().reshape(SEEDS, MAX_STEPS) == ext).all() and (d_steps.cpu().numpy().view(np.uint32) == steps).all()
                                and (d_stop.cpu().numpy() == stop).all())
                timed("sample_counts loop (warm-up)", lambda: sample_counts_loop(L, ss, seeds[:16], flat, mask))
                t_base, base = [], None
                for _ in range(RUNS):
                    dt, base = timed("sample_counts loop", lambda: sample_counts_loop(L, ss, seeds, flat, mask))
                    t_base.append(dt)
                agree = bool((base[0] == ext).all() and (base[1] == steps).all() and (base[2] == stop).all())
                m_host, m_dev, m_base = statistics.median(t_host), statistics.median(t_dev), statistics.median(t_base)
                walked = int(steps.max()) + 1 if SEEDS else 0
                per_mask[name] = {
                    "masked_samples": int(mask.sum()), "host_ms": [round(t * 1e3, 3) for t in t_host], "device_ms": [round(t * 1e3, 3) for t in t_dev],
                    "sample_counts_loop_ms": [round(t * 1e3, 3) for t in t_base], "host_median_ms": round(m_host * 1e3, 3),
                    "device_median_ms": round(m_dev * 1e3, 3), "sample_counts_loop_median_ms": round(m_base * 1e3, 3),
                    "sample_counts_loop_over_host_call": round(m_base / m_host, 2), "sample_counts_calls": int(base[3]),
                    "stops": {k: int((stop == v).sum()) for k, v in (("dead_end", 1), ("branch", 2), ("limit", 3), ("invalid", 4), ("wide", 8))},
                    "mean_steps_per_seed": round(float(steps.mean()), 2), "steps_with_a_seed_walking": min(walked, MAX_STEPS),
                    "device_ms_by_launch": by_launch, "host_ms_with_events": round(t_marked * 1e3, 3), "launches_enqueued": MAX_STEPS * 7 + 2, "us_per_enqueued_step_device_call": round(m_dev * 1e6 / MAX_STEPS, 2),
                    "rows_located_per_appended_symbol": round(wk["rows"] / max(wk["appended"], 1), 2),
                    "locate_lf_steps_per_row": round(wk["lf_steps"] / max(wk["rows"], 1), 2),
                    "search_lf_steps_per_search": round(wk["search_steps"] / max(wk["searches"], 1), 2), "work": wk,
                    "device_form_agrees_with_host_form": same_dev, "sample_counts_loop_agrees_everywhere": agree}
                if not (agree and same_dev):
                    raise RuntimeError(f"{S} shards, {name}: the call and the sample_counts loop disagree")
            res["by_shards"][str(S)] = {"symbols": int(sum(g.getBWLen() for g in gs)), "ktab_depth": gs[0].ktab_depth(),
                                        "window_span": gs[0].window_span(), "masks": per_mask}
        finally:
            ss.close()
            for g in gs:
                g.close()
    res["timing"] = ("host_* and sample_counts_loop_*: wall clock round the C calls from Python (upload, launches, copies back; the loop's numpy "
                     "included); device_*: events round everything the device-resident call enqueues (max_steps x 7 launches, most of which leave at "
                     "once when no seed still walks); device_ms_by_launch: one more host call under RSBWT_SAMPLE_WALK_TIMES=1, an event round every "
                     "launch, summed by kind -- the events cost time of their own (host_ms_with_events against host_median_ms)")
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
