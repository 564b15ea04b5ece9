#!/usr/bin/env python3
"""The per-read sample table on a population BWT (csrc/read_meta.hip, rsbwt_set_meta_*): the popBWT of tools/popbwt_gpu.py
(make_reads + bwt_runs: haplotypes of a seeded genome, reads of both strands, suffix-sorted on the GPU) as one shard, every
indexed read given a value, at two value-length mixes:
    few     every read in 1-3 samples (records of 4 bytes: 4, 8 or 12 bytes)
    skewed  the same, but 1 % of the reads in 2,000 samples (8,000 bytes)
Per mix, as medians of RUNS: the build (wall clock), the gather of ITEMS random ordinals through the host-buffer call (wall
clock) and through the device-resident call (events around LAUNCHES calls in a row, per call), the string-keyed call over ITEMS indexed
reads (wall clock: one whole-read search + the gather) -- and beside it, for scale, rsbwt_set_extract of the same reads in
the same run (the rows of their ordinals).  The values that come back are held to the pairs given: by ordinal on every item,
by string on every query.  Every step runs under a time limit of its own (a step that outlasts it ends the process with
status 124).
usage: tools/meta_probe.py [items=2000000] [genome=1e6] [haplotypes=32] [coverage=1] [out=profiles/meta_probe.json]"""
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

ITEMS = int(float(sys.argv[1])) if len(sys.argv) > 1 else 2000000
GENOME = int(float(sys.argv[2])) if len(sys.argv) > 2 else 1_000_000
HAPS = int(sys.argv[3]) if len(sys.argv) > 3 else 32
COV = float(sys.argv[4]) if len(sys.argv) > 4 else 1.0
OUT = sys.argv[5] if len(sys.argv) > 5 else os.path.join(ROOT, "profiles", "meta_probe.json")
READ_LEN, RUNS, STEP_LIMIT_S, RECORD = 100, 5, 120.0, 4
LAUNCHES = 20  # device-resident calls between one pair of events: a single one is tens of microseconds


def timed(what, fn):
    guard = threading.Timer(STEP_LIMIT_S, lambda: (sys.stderr.write(f"meta_probe: {what} exceeded {STEP_LIMIT_S} s\n"), os._exit(124)))
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
    R = int(reads.shape[0])
    g = rsb.GpuBWT(runs=runs.cpu().numpy(), num_strings=R, for_reads=True)
    ss = rsb.ShardSet([g])
    L = rsb.lib()
    pv = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    chk = lambda rc: rc == 0 or (_ for _ in ()).throw(RuntimeError(L.rsbwt_last_error().decode()))  # noqa: E731
    res = {"symbols": int(n), "reads_indexed": R, "ktab_depth": g.ktab_depth(), "window_span": g.window_span(), "items": ITEMS,
           "read_length": READ_LEN, "record_bytes": RECORD, "shards": 1, "runs": RUNS, "launches_per_device_timing": LAUNCHES, "by_mix": {}}
    try:
        rng = np.random.default_rng(31)
        text = np.append(np.frombuffer(b"$ACGT", np.uint8)[reads.cpu().numpy()].ravel(), np.uint8(0))
        off = np.arange(R + 1, dtype=np.uint64) * np.uint64(READ_LEN)
        # the reads' ordinals (one search of all of them), and for every ordinal the pair that wins it: the last of its copies
        od, cp = np.zeros(R, np.uint64), np.zeros(R, np.uint64)
        chk(L.rsbwt_set_read_ordinals_var(ss._s, pv(text), pv(off), R, pv(od), pv(cp)))
        assert (cp > 0).all()
        winner = np.zeros(R, np.int64)
        for c in range(int(cp.max())):  # (ascending pair index: the highest stays)
            m = cp > c
            winner[(od[m] + np.uint64(c)).astype(np.int64)] = np.flatnonzero(m)
        for mix in ("few", "skewed"):
            lens = rng.integers(1, 4, R).astype(np.uint64) * np.uint64(RECORD)
            if mix == "skewed":
                lens[rng.random(R) < 0.01] = 2000 * RECORD
            voff = np.zeros(R + 1, np.uint64)
            voff[1:] = np.cumsum(lens, dtype=np.uint64)
            values = rng.integers(0, 256, int(voff[-1]) + 1, dtype=np.uint8)
            st = np.zeros(4, np.uint64)
            t_build = []
            for _ in range(3):
                dt, rc = timed("build", lambda: L.rsbwt_set_meta_build(ss._s, pv(text), pv(off), pv(values), pv(voff), R, pv(st)))
                chk(rc)
                t_build.append(dt)
            assert int(st[0]) == R and int(st[2]) == R, st
            # ---- the ordinal gather
            sh = np.zeros(ITEMS, np.uint32)
            ods = rng.integers(0, R, ITEMS).astype(np.uint64)
            first = np.zeros(ITEMS + 1, np.uint64)
            nb = C.c_size_t()
            rc = L.rsbwt_set_meta_by_ordinal(ss._s, pv(sh), pv(ods), ITEMS, pv(first), None, 0, C.byref(nb))
            assert rc in (0, -7)
            total = nb.value
            out = np.zeros(total + 1, np.uint8)
            host = lambda: L.rsbwt_set_meta_by_ordinal(ss._s, pv(sh), pv(ods), ITEMS, pv(first), pv(out), total, C.byref(nb))  # noqa: E731
            chk(timed("ordinal gather (warm-up)", host)[1])
            t_host = [timed("ordinal gather", host)[0] for _ in range(RUNS)]
            w = winner[ods.astype(np.int64)]
            want_first = np.zeros(ITEMS + 1, np.uint64)
            want_first[1:] = np.cumsum(lens[w], dtype=np.uint64)
            same = bool((first == want_first).all())
            for i in rng.integers(0, ITEMS, 2000):
                same = same and bool((out[int(first[i]):int(first[i + 1])] == values[int(voff[w[i]]):int(voff[w[i] + 1])]).all())
            d_sh, d_od = torch.from_numpy(sh.view(np.int32)).cuda(), torch.from_numpy(ods.view(np.int64)).cuda()
            d_first = torch.zeros(ITEMS + 1, dtype=torch.int64, device="cuda")
            d_bytes = torch.zeros(total + 16, dtype=torch.uint8, device="cuda")

            def launch():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                rc = 0
                for _ in range(LAUNCHES):
                    rc = rc or L.rsbwt_set_meta_by_ordinal_dev(ss._s, p(d_sh), p(d_od), ITEMS, p(d_first), p(d_bytes), total, None)
                e1.record()
                torch.cuda.synchronize()
                chk(rc)
                return e0.elapsed_time(e1) * 1e-3 / LAUNCHES
            timed("device gather (warm-up)", launch)
            t_dev = [timed("device gather", launch)[1] for _ in range(RUNS)]
            same_dev = bool((d_bytes[:total].cpu().numpy() == out[:total]).all() and (d_first.cpu().numpy().view(np.uint64) == first).all())
            # ---- the string-keyed call over ITEMS indexed reads, and their extraction beside it
            pick = rng.integers(0, R, ITEMS)
            qtext = np.append(text[:-1].reshape(R, READ_LEN)[pick].ravel(), np.uint8(0))
            qoff = np.arange(ITEMS + 1, dtype=np.uint64) * np.uint64(READ_LEN)
            sfirst = np.zeros(ITEMS + 1, np.uint64)
            rc = L.rsbwt_set_read_meta_var(ss._s, pv(qtext), pv(qoff), ITEMS, pv(sfirst), None, 0, C.byref(nb), None)
            assert rc in (0, -7)
            stotal = nb.value
            sout = np.zeros(stotal + 1, np.uint8)
            keyed = lambda: L.rsbwt_set_read_meta_var(ss._s, pv(qtext), pv(qoff), ITEMS, pv(sfirst), pv(sout), stotal, C.byref(nb), None)  # noqa: E731
            chk(timed("string-keyed call (warm-up)", keyed)[1])
            t_key = [timed("string-keyed call", keyed)[0] for _ in range(RUNS)]
            wq = winner[od[pick].astype(np.int64)]  # (the value at the read's first ordinal: all copies hold the same)
            want_first[1:] = np.cumsum(lens[wq], dtype=np.uint64)
            same_key = bool((sfirst == want_first).all())
            for i in rng.integers(0, ITEMS, 2000):
                same_key = same_key and bool((sout[int(sfirst[i]):int(sfirst[i + 1])] == values[int(voff[wq[i]]):int(voff[wq[i] + 1])]).all())
            rows = g.occ_at_batch("$", od[pick] + np.uint64(1))
            xs, xl, xp = np.zeros((ITEMS, 128), np.uint8), np.zeros(ITEMS, np.uint32), np.zeros(ITEMS, np.uint32)
            ext = lambda: L.rsbwt_set_extract(ss._s, pv(sh), pv(rows), ITEMS, pv(xs), 128, pv(xl), pv(xp))  # noqa: E731
            chk(timed("extract (warm-up)", ext)[1])
            t_ext = [timed("extract", ext)[0] for _ in range(RUNS)]
            same_ext = bool((xl == READ_LEN).all() and (xs[:, :READ_LEN] == qtext[:-1].reshape(ITEMS, READ_LEN)).all())
            mh, md, mk, mx = (statistics.median(t) for t in (t_host, t_dev, t_key, t_ext))
            res["by_mix"][mix] = {
                "value_bytes_in_table": int(st[3]), "table_bytes": int(ss.meta_bytes()), "long_values": int((lens > 64).sum()),
                "build_s": [round(t, 4) for t in t_build], "build_median_s": round(statistics.median(t_build), 4),
                "pairs_per_s_build": round(R / statistics.median(t_build), 1),
                "ordinal_host_ms": [round(t * 1e3, 3) for t in t_host], "ordinal_device_ms": [round(t * 1e3, 4) for t in t_dev],
                "keyed_host_ms": [round(t * 1e3, 3) for t in t_key], "extract_host_ms": [round(t * 1e3, 3) for t in t_ext],
                "ordinal_bytes": int(total), "keyed_bytes": int(stotal),
                "ordinal_values_per_s_host_call": round(ITEMS / mh, 1), "ordinal_bytes_per_s_host_call": round(total / mh, 1),
                "ordinal_values_per_s_launches": round(ITEMS / md, 1), "ordinal_bytes_per_s_launches": round(total / md, 1),
                "keyed_values_per_s_host_call": round(ITEMS / mk, 1), "keyed_bytes_per_s_host_call": round(stotal / mk, 1),
                "extract_reads_per_s_host_call": round(ITEMS / mx, 1), "extract_over_keyed": round(mx / mk, 2),
                "ordinal_values_agree": same, "device_form_agrees_with_host_form": same_dev, "keyed_values_agree": same_key,
                "extracted_reads_are_the_queries": same_ext}
            if not (same and same_dev and same_key and same_ext):
                raise RuntimeError(f"mix {mix}: the values that came back are not the pairs'")
        res["timing"] = ("build_*, *_host_*: wall clock around the C calls from Python (uploads, kernels, copies back); ordinal_device_*: "
                         f"events around {LAUNCHES} device-resident calls in a row, per call (sizes, scan, copy; nothing crosses PCIe)")
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
