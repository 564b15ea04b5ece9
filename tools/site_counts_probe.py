#!/usr/bin/env python3
"""Site sample counts on a population BWT (csrc/site_counts.hip, rsbwt_set_site_sample_counts): tools/meta_probe.py's shard
(the popBWT of tools/popbwt_gpu.py as one shard) with nine reads in ten given a value of 1-3 records of a dictionary of
SAMPLES samples (size_of_sample 2 + the c and l bytes: 4 bytes a record).  Per call SITES of the shard's planted SNPs, two
requests each -- the reference window (alt = the other base) and the alt window (alt = the reference base), windows of 199
symbols with the site at 100, isalt 0.  Timed side by side in one run, as medians of RUNS after a warm-up:
    new      rsbwt_set_site_sample_counts (wall clock around the C call, the matrices' copy back included), and its stages
             from events (RSBWT_SITE_TIMES=1, in a run of their own: the events wait)
    composed the route to the same matrices from the calls that existed before: rsbwt_set_gt_aligned_reads (its sizing call
             not timed), rsbwt_set_read_meta_var of every kept read, and a numpy tally of the records
The two routes' matrices and carriers are asserted equal before any time is taken.  Every step runs under a time limit of its
own (a step that outlasts it ends the process with status 124).
usage: tools/site_counts_probe.py [sites=500] [samples=2000] [genome=1e6] [haplotypes=32] [coverage=1] [out=profiles/site_counts_probe.json]"""
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

SITES = int(float(sys.argv[1])) if len(sys.argv) > 1 else 500
SAMPLES = int(float(sys.argv[2])) if len(sys.argv) > 2 else 2000
GENOME = int(float(sys.argv[3])) if len(sys.argv) > 3 else 1_000_000
HAPS = int(sys.argv[4]) if len(sys.argv) > 4 else 32
COV = float(sys.argv[5]) if len(sys.argv) > 5 else 1.0
OUT = sys.argv[6] if len(sys.argv) > 6 else os.path.join(ROOT, "profiles", "site_counts_probe.json")
READ_LEN, WINDOW, K, SKIP, RUNS, STEP_LIMIT_S, RECORD, SNP, SEED = 100, 199, 31, 4, 5, 120.0, 4, 1e-3, 5


def timed(what, fn):
    guard = threading.Timer(STEP_LIMIT_S, lambda: (sys.stderr.write(f"site_counts_probe: {what} exceeded {STEP_LIMIT_S} s\n"), os._exit(124)))
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
    reads, genome0 = P.make_reads(GENOME, HAPS, COV, READ_LEN, SNP, 0.0, SEED)
    # the genome and the planted SNPs: make_reads' first three draws, drawn again
    gen = torch.Generator(device=P.dev)
    gen.manual_seed(SEED)
    genome = torch.randint(1, 5, (GENOME,), generator=gen, device=P.dev, dtype=torch.uint8)
    nsites = int(GENOME * SNP)
    sites = torch.randint(0, GENOME, (nsites,), generator=gen, device=P.dev)
    alt = ((genome[sites].long() - 1 + torch.randint(1, 4, (nsites,), generator=gen, device=P.dev)) % 4 + 1).to(torch.uint8)
    assert torch.equal(genome, genome0), "the redraw is not make_reads' genome"
    genome, sites, alt = genome.cpu().numpy(), sites.cpu().numpy(), alt.cpu().numpy()
    runs, n, _ = P.bwt_runs(reads)
    R = int(reads.shape[0])
    g = rsb.GpuBWT(runs=runs.cpu().numpy(), num_strings=R, for_reads=True)
    ss = rsb.ShardSet([g])
    L = rsb.lib()
    pv = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    chk = lambda rc: rc == 0 or (_ for _ in ()).throw(RuntimeError(L.rsbwt_last_error().decode()))  # noqa: E731
    width = SAMPLES + 1
    half = WINDOW // 2
    res = {"symbols": int(n), "reads_indexed": R, "ktab_depth": g.ktab_depth(), "window_span": g.window_span(), "samples": SAMPLES,
           "record_bytes": RECORD, "shards": 1, "runs": RUNS, "window": WINDOW, "k": K, "skip": SKIP, "max_interval_size": 10000}
    try:
        rng = np.random.default_rng(47)
        sym = np.frombuffer(b"$ACGT", np.uint8)
        text = np.append(sym[reads.cpu().numpy()].ravel(), np.uint8(0))
        off = np.arange(R + 1, dtype=np.uint64) * np.uint64(READ_LEN)
        # nine reads in ten get a value of 1-3 records
        named = np.flatnonzero(rng.random(R) < 0.9)
        ntext = np.append(text[:-1].reshape(R, READ_LEN)[named].ravel(), np.uint8(0))
        noff = np.arange(named.size + 1, dtype=np.uint64) * np.uint64(READ_LEN)
        codes = (np.arange(SAMPLES, dtype=np.uint32) * 7 + 3).astype(">u2")
        flat = codes.view(np.uint8).copy()
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
        st = np.zeros(4, np.uint64)
        dt_build, rc = timed("build", lambda: L.rsbwt_set_meta_build(ss._s, pv(ntext), pv(noff), pv(values), pv(voff), named.size, pv(st)))
        chk(rc)
        # the requests
        ok = np.flatnonzero((sites >= half) & (sites < GENOME - half))
        ok = ok[np.unique(sites[ok], return_index=True)[1]][:SITES]
        ws, pos, alts = [], [], []
        for j in ok:
            i = int(sites[j])
            w = sym[genome[i - half:i + half + 1]].copy()
            ws.append(w.copy())
            alts.append(sym[alt[j]])
            w[half] = sym[alt[j]]
            ws.append(w)
            alts.append(sym[genome[i]])
            pos += [half + 1, half + 1]
        Q = len(ws)
        qtext = np.append(np.concatenate(ws), np.uint8(0))
        qoff = np.arange(Q + 1, dtype=np.uint64) * np.uint64(WINDOW)
        qpos, qalt, qisalt = np.array(pos, np.uint64), np.array(alts, np.uint8), np.zeros(Q, np.uint8)
        res["requests"] = Q
        res["matrix_bytes_per_call"] = 12 * Q * width
        # ---- new
        strings, copies = np.zeros((Q, width), np.uint32), np.zeros((Q, width), np.int64)
        aligned, carriers = np.zeros(Q, np.uint64), np.zeros(Q, np.uint64)
        new = lambda: L.rsbwt_set_site_sample_counts(ss._s, pv(qtext), pv(qoff), Q, pv(qpos), pv(qalt), pv(qisalt), K, SKIP, 0, pv(flat), SAMPLES, 2, 1,  # noqa: E731
                                                     pv(strings), pv(copies), pv(aligned), pv(carriers))
        chk(timed("site sample counts (warm-up)", new)[1])
        wk = rsb.ShardSet.site_last_work()
        assert carriers.sum() > 0 and wk["extracted"] < wk["aligned"], wk
        # ---- composed: the aligned reads come down, go up again as queries for their values, and are tallied here
        first = np.zeros(Q + 1, np.uint64)
        nr = C.c_size_t()
        rc = L.rsbwt_set_gt_aligned_reads(ss._s, pv(qtext), pv(qoff), Q, pv(qpos), pv(qalt), pv(qisalt), K, SKIP, 0, pv(first), None, 128, None, None, 0,
                                          C.byref(nr))
        assert rc in (0, -7), L.rsbwt_last_error()
        cap = nr.value
        rbuf, rlen = np.zeros((max(cap, 1), 128), np.uint8), np.zeros(max(cap, 1), np.uint32)
        moved = {}

        def composed():
            chk(L.rsbwt_set_gt_aligned_reads(ss._s, pv(qtext), pv(qoff), Q, pv(qpos), pv(qalt), pv(qisalt), K, SKIP, 0, pv(first), pv(rbuf), 128, pv(rlen),
                                             None, cap, C.byref(nr)))
            m = nr.value
            assert (rlen[:m] == READ_LEN).all()
            rtext = np.append(rbuf[:m, :READ_LEN].ravel(), np.uint8(0))
            roff = np.arange(m + 1, dtype=np.uint64) * np.uint64(READ_LEN)
            vfirst, cp = np.zeros(m + 1, np.uint64), np.zeros(m, np.uint64)
            nb = C.c_size_t()
            rc = L.rsbwt_set_read_meta_var(ss._s, pv(rtext), pv(roff), m, pv(vfirst), None, 0, C.byref(nb), pv(cp))
            assert rc in (0, -7)
            out = np.zeros(nb.value + 1, np.uint8)
            chk(L.rsbwt_set_read_meta_var(ss._s, pv(rtext), pv(roff), m, pv(vfirst), pv(out), nb.value, C.byref(nb), pv(cp)))
            moved.update(reads_down=m * 128 + m * 4, reads_up=2 * (m * READ_LEN + (m + 1) * 8), values_down=int(nb.value) + 2 * (m + 1) * 8 + 2 * m * 8)
            rq = np.repeat(np.arange(Q), np.diff(first).astype(np.int64))
            per = (np.diff(vfirst) // np.uint64(RECORD)).astype(np.int64)
            recs = out[:nb.value].reshape(-1, RECORD)
            k = (recs[:, 0].astype(np.uint64) << np.uint64(8)) | recs[:, 1].astype(np.uint64)
            col = np.searchsorted(keys, k)
            col = np.where((col < SAMPLES) & (keys[np.minimum(col, SAMPLES - 1)] == k), col, SAMPLES)
            cell = np.repeat(rq, per) * width + col
            s2 = np.bincount(cell, minlength=Q * width).astype(np.uint32).reshape(Q, width)
            c2 = np.bincount(cell, weights=recs[:, 2].astype(np.int8).astype(np.float64) - 33, minlength=Q * width)
            return s2, c2.astype(np.int64).reshape(Q, width), np.bincount(rq[per > 0], minlength=Q).astype(np.uint64)

        _, (s2, c2, car2) = timed("composed route (warm-up)", composed)
        equal = bool((s2 == strings).all() and (c2 == copies).all() and (car2 == carriers).all())
        if not equal:
            raise RuntimeError("the composed route's matrices are not the call's")
        t_new = [timed("site sample counts", new)[0] for _ in range(RUNS)]
        t_old = [timed("composed route", composed)[0] for _ in range(RUNS)]
        os.environ["RSBWT_SITE_TIMES"] = "1"
        stages = []
        for _ in range(RUNS):
            chk(timed("site sample counts (stage events)", new)[1])
            stages.append(rsb.ShardSet.site_last_times())
        del os.environ["RSBWT_SITE_TIMES"]
        mn, mo = statistics.median(t_new), statistics.median(t_old)
        sizes = 5 * 8
        res.update({
            "value_bytes_in_table": int(st[3]), "build_s": round(dt_build, 4), "work": wk, "carriers": int(carriers.sum()),
            "new_ms": [round(t * 1e3, 3) for t in t_new], "composed_ms": [round(t * 1e3, 3) for t in t_old],
            "new_median_ms": round(mn * 1e3, 3), "composed_median_ms": round(mo * 1e3, 3), "composed_over_new": round(mo / mn, 2),
            "stage_median_ms": {k: round(statistics.median(s[k] for s in stages), 4) for k in stages[0]},
            "pcie_bytes_new": {"up": int(qtext.size + (Q + 1) * 8 + Q * 8 + 2 * Q + Q * 4 * 3 + SAMPLES * 8),
                               "down": int(12 * Q * width + 2 * Q * 8 + 8 * 32 * 8 + 24 + sizes)},
            "pcie_bytes_composed_beyond_the_request": dict(moved),
            "matrices_equal": equal})
        res["timing"] = ("new_*, composed_*: wall clock from Python around the C calls (and, composed, the numpy steps between them); stage_median_ms: "
                         "events around each stage's launches inside the call, in runs of their own")
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
