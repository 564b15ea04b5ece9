#!/usr/bin/env python3
"""Sample counts on a population BWT (csrc/sample_counts.hip, rsbwt_set_sample_counts): tools/meta_probe.py's shard (the
popBWT of tools/popbwt_gpu.py as one shard, every indexed read given a value) with values that are records of a dictionary
of SAMPLES samples (size_of_sample 2 + the c and l bytes: 4 bytes a record), at meta_probe's two mixes:
    few     every read in 1-3 samples
    skewed  the same, but 1 % of the reads in all 2,000 samples
Per call QUERIES 31-mers drawn from the reads.  Timed side by side in one run, as medians of RUNS:
    new      rsbwt_set_sample_counts, host form (wall clock around the C call, the matrices' copy back included), and
             rsbwt_set_sample_counts_dev (events around LAUNCHES calls in a row, per call)
    composed the only route to the same matrices without the call, spelt here: rsbwt_set_locate_var_capped (ordinals of
             every row), a numpy dedupe of (query, ordinal) on the head ordinals (the probe keeps the head bits it learnt from
             rsbwt_set_read_ordinals_var when it built the table), rsbwt_set_meta_by_ordinal of the carriers, and a numpy
             tally of the records.  It dedupes BEFORE it gathers, which is the cheaper order.
The two routes' matrices are asserted equal before any time is reported.  Every step runs under a time limit of its own (a
step that outlasts it ends the process with status 124).
usage: tools/sample_counts_probe.py [queries=10000] [samples=2000] [genome=1e6] [haplotypes=32] [coverage=1] [out=profiles/sample_counts_probe.json]"""
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

QUERIES = int(float(sys.argv[1])) if len(sys.argv) > 1 else 10000
SAMPLES = int(float(sys.argv[2])) if len(sys.argv) > 2 else 2000
GENOME = int(float(sys.argv[3])) if len(sys.argv) > 3 else 1_000_000
HAPS = int(sys.argv[4]) if len(sys.argv) > 4 else 32
COV = float(sys.argv[5]) if len(sys.argv) > 5 else 1.0
OUT = sys.argv[6] if len(sys.argv) > 6 else os.path.join(ROOT, "profiles", "sample_counts_probe.json")
READ_LEN, K, RUNS, STEP_LIMIT_S, RECORD, LAUNCHES = 100, 31, 5, 120.0, 4, 20


def timed(what, fn):
    guard = threading.Timer(STEP_LIMIT_S, lambda: (sys.stderr.write(f"sample_counts_probe: {what} exceeded {STEP_LIMIT_S} s\n"), os._exit(124)))
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
    width = SAMPLES + 1
    res = {"symbols": int(n), "reads_indexed": R, "ktab_depth": g.ktab_depth(), "window_span": g.window_span(), "queries": QUERIES, "k": K,
           "samples": SAMPLES, "record_bytes": RECORD, "shards": 1, "runs": RUNS, "launches_per_device_timing": LAUNCHES,
           "matrix_bytes_per_call": 12 * QUERIES * width, "by_mix": {}}
    try:
        rng = np.random.default_rng(47)
        text = np.append(np.frombuffer(b"$ACGT", np.uint8)[reads.cpu().numpy()].ravel(), np.uint8(0))
        off = np.arange(R + 1, dtype=np.uint64) * np.uint64(READ_LEN)
        od, cp = np.zeros(R, np.uint64), np.zeros(R, np.uint64)
        chk(L.rsbwt_set_read_ordinals_var(ss._s, pv(text), pv(off), R, pv(od), pv(cp)))
        assert (cp > 0).all()
        is_head = np.zeros(R, bool)
        is_head[od.astype(np.int64)] = True
        # the dictionary: sample i has the code of the big-endian number 7 i + 3 -- ascending, and not every code there is
        codes = (np.arange(SAMPLES, dtype=np.uint32) * 7 + 3).astype(">u2")
        flat = codes.view(np.uint8).copy()
        keys = np.zeros(SAMPLES, np.uint64)
        chk(L.rsbwt_sample_keys(pv(flat), SAMPLES, 2, pv(keys)))
        # the queries: K-mers cut from reads
        pick, at = rng.integers(0, R, QUERIES), rng.integers(0, READ_LEN - K + 1, QUERIES)
        rows2d = text[:-1].reshape(R, READ_LEN)
        qtext = np.append(np.stack([rows2d[i, a:a + K] for i, a in zip(pick, at)]).ravel(), np.uint8(0))
        qoff = np.arange(QUERIES + 1, dtype=np.uint64) * np.uint64(K)
        for mix in ("few", "skewed"):
            nrec = rng.integers(1, 4, R).astype(np.int64)
            if mix == "skewed":
                nrec[rng.random(R) < 0.01] = SAMPLES
            voff = np.zeros(R + 1, np.uint64)
            voff[1:] = np.cumsum(nrec * RECORD, dtype=np.uint64)
            total_rec = int(nrec.sum())
            rec = np.zeros((total_rec, RECORD), np.uint8)
            which = rng.integers(0, SAMPLES, total_rec)
            full = np.flatnonzero(nrec == SAMPLES)
            starts = (voff[:-1] // np.uint64(RECORD)).astype(np.int64)
            for i in full:  # a read of a common sequence lists every sample once
                which[starts[i]:starts[i] + SAMPLES] = np.arange(SAMPLES)
            rec[:, :2] = codes[which].view(np.uint8).reshape(-1, 2)
            rec[:, 2] = 33 + rng.integers(0, 6, total_rec)
            rec[:, 3] = 33 + rng.integers(0, 40, total_rec)
            values = np.append(rec.ravel(), np.uint8(0))
            st = np.zeros(4, np.uint64)
            dt_build, rc = timed("build", lambda: L.rsbwt_set_meta_build(ss._s, pv(text), pv(off), pv(values), pv(voff), R, pv(st)))
            chk(rc)
            # ---- new: the host form
            strings, copies = np.zeros((QUERIES, width), np.uint32), np.zeros((QUERIES, width), np.int64)
            matches, carriers = np.zeros(QUERIES, np.uint64), np.zeros(QUERIES, np.uint64)
            new = lambda: L.rsbwt_set_sample_counts(ss._s, pv(qtext), pv(qoff), QUERIES, pv(flat), SAMPLES, 2, 1, 0, 0, pv(strings), pv(copies),  # noqa: E731
                                                    pv(matches), pv(carriers))
            chk(timed("sample counts (warm-up)", new)[1])
            wk = rsb.ShardSet.sample_last_work()
            # ---- composed: locate, dedupe, gather, tally
            total = wk["rows"]
            first = np.zeros(QUERIES + 1, np.uint64)
            r_od = np.zeros(total + 1, np.uint64)
            nr = C.c_size_t()

            def composed():
                chk(L.rsbwt_set_locate_var_capped(ss._s, pv(qtext), pv(qoff), QUERIES, 0, 0, pv(first), None, None, None, pv(r_od), None, total,
                                                  C.byref(nr), None))
                q_of = np.repeat(np.arange(QUERIES, dtype=np.uint64), np.diff(first).astype(np.int64))
                o = r_od[:total]
                keep = is_head[o.astype(np.int64)]
                uq = np.unique((q_of[keep] << np.uint64(40)) | o[keep])
                cq, co = (uq >> np.uint64(40)).astype(np.int64), uq & np.uint64((1 << 40) - 1)
                sh = np.zeros(co.size, np.uint32)
                vfirst = np.zeros(co.size + 1, np.uint64)
                nb = C.c_size_t()
                rc = L.rsbwt_set_meta_by_ordinal(ss._s, pv(sh), pv(co), co.size, pv(vfirst), None, 0, C.byref(nb))
                assert rc in (0, -7)
                out = np.zeros(nb.value + 1, np.uint8)
                chk(L.rsbwt_set_meta_by_ordinal(ss._s, pv(sh), pv(co), co.size, pv(vfirst), pv(out), nb.value, C.byref(nb)))
                recs = out[:nb.value].reshape(-1, RECORD)
                per = (np.diff(vfirst) // np.uint64(RECORD)).astype(np.int64)
                rq = np.repeat(cq, per)
                k = (recs[:, 0].astype(np.uint64) << np.uint64(8)) | recs[:, 1].astype(np.uint64)
                col = np.searchsorted(keys, k)
                col = np.where((col < SAMPLES) & (keys[np.minimum(col, SAMPLES - 1)] == k), col, SAMPLES)
                cell = rq * width + col
                s2 = np.bincount(cell, minlength=QUERIES * width).astype(np.uint32).reshape(QUERIES, width)
                c2 = np.bincount(cell, weights=recs[:, 2].astype(np.int8).astype(np.float64) - 33, minlength=QUERIES * width)
                return s2, c2.astype(np.int64).reshape(QUERIES, width), np.bincount(cq, minlength=QUERIES).astype(np.uint64), np.diff(first)

            dt, (s2, c2, car2, m2) = timed("composed route (warm-up)", composed)
            equal = bool((s2 == strings).all() and (c2 == copies).all() and (car2 == carriers).all() and (m2 == matches).all())
            if not equal:
                raise RuntimeError(f"mix {mix}: the composed route's matrices are not the call's")
            t_new = [timed("sample counts", new)[0] for _ in range(RUNS)]
            t_old = [timed("composed route", composed)[0] for _ in range(RUNS)]
            # ---- new: the device form
            d_text, d_off = torch.from_numpy(qtext).cuda(), torch.from_numpy(qoff.view(np.int64)).cuda()
            d_keys = torch.from_numpy(keys.view(np.int64)).cuda()
            d_str = torch.zeros(QUERIES * width, dtype=torch.int32, device="cuda")
            d_cp = torch.zeros(QUERIES * width, dtype=torch.int64, device="cuda")
            d_mt, d_ca = torch.zeros(QUERIES, dtype=torch.int64, device="cuda"), torch.zeros(QUERIES, dtype=torch.int64, device="cuda")
            d_st = torch.zeros(8, dtype=torch.int64, device="cuda")

            def launch():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                rc = 0
                for _ in range(LAUNCHES):
                    rc = rc or L.rsbwt_set_sample_counts_dev(ss._s, p(d_text), p(d_off), QUERIES, K, p(d_keys), SAMPLES, 2, 1, 0, 0, total, p(d_str),
                                                             p(d_cp), p(d_mt), p(d_ca), p(d_st), None)
                e1.record()
                torch.cuda.synchronize()
                chk(rc)
                return e0.elapsed_time(e1) * 1e-3 / LAUNCHES
            timed("device form (warm-up)", launch)
            t_dev = [timed("device form", launch)[1] for _ in range(RUNS)]
            same_dev = bool((d_str.cpu().numpy().view(np.uint32).reshape(QUERIES, width) == strings).all()
                            and (d_cp.cpu().numpy().reshape(QUERIES, width) == copies).all()
                            and (d_ca.cpu().numpy().view(np.uint64) == carriers).all() and int(d_st[6]) == 0 and int(d_st[0]) == total)
            if not same_dev:
                raise RuntimeError(f"mix {mix}: the device form's matrices are not the host form's")
            mn, mo, md = statistics.median(t_new), statistics.median(t_old), statistics.median(t_dev)
            res["by_mix"][mix] = {
                "value_bytes_in_table": int(st[3]), "head_bytes": int(ss.meta_head_bytes()), "build_s": round(dt_build, 4), "work": wk,
                "host_form_ms": [round(t * 1e3, 3) for t in t_new], "composed_ms": [round(t * 1e3, 3) for t in t_old],
                "device_form_ms": [round(t * 1e3, 4) for t in t_dev], "host_form_median_ms": round(mn * 1e3, 3),
                "composed_median_ms": round(mo * 1e3, 3), "device_form_median_ms": round(md * 1e3, 4),
                "composed_over_host_form": round(mo / mn, 2), "composed_over_device_form": round(mo / md, 2),
                "queries_per_s_host_form": round(QUERIES / mn, 1), "queries_per_s_device_form": round(QUERIES / md, 1),
                "matrices_equal": equal, "device_form_agrees_with_host_form": same_dev}
        res["timing"] = ("host_form_*, composed_*: wall clock from Python around the C calls (and, composed, the numpy steps between them); "
                         f"device_form_*: events around {LAUNCHES} device-resident calls in a row, per call (nothing crosses PCIe)")
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
