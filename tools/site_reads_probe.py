#!/usr/bin/env python3
"""Site reads on a population BWT (csrc/site_reads.hip, rsbwt_set_site_reads): tools/site_counts_probe.py's workload -- the
popBWT of tools/popbwt_gpu.py as one shard; per call SITES of its planted SNPs, two requests each (the reference window with
alt = the other base, and the alt window with alt = the reference base), windows of 199 symbols with the site at 100, isalt 0.
Timed side by side in one run, as medians of RUNS after a warm-up, wall clock around the C call with room for the exact
number of reads (the sizing calls are not timed):
    new       rsbwt_set_site_reads
    composed  rsbwt_set_gt_aligned_reads, the call it restates (its code is what it was before the new call existed)
first[], the reads' bytes, lengths and rows of the two are asserted equal before any time is taken.  Every step runs under a
time limit of its own (a step that outlasts it ends the process with status 124).
usage: tools/site_reads_probe.py [sites=500] [genome=1e6] [haplotypes=32] [coverage=1] [out=profiles/site_reads_probe.json]"""
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
GENOME = int(float(sys.argv[2])) if len(sys.argv) > 2 else 1_000_000
HAPS = int(sys.argv[3]) if len(sys.argv) > 3 else 32
COV = float(sys.argv[4]) if len(sys.argv) > 4 else 1.0
OUT = sys.argv[5] if len(sys.argv) > 5 else os.path.join(ROOT, "profiles", "site_reads_probe.json")
READ_LEN, WINDOW, K, SKIP, RUNS, STEP_LIMIT_S, SNP, SEED, STRIDE = 100, 199, 31, 4, 5, 120.0, 1e-3, 5, 128


def timed(what, fn):
    guard = threading.Timer(STEP_LIMIT_S, lambda: (sys.stderr.write(f"site_reads_probe: {what} exceeded {STEP_LIMIT_S} s\n"), os._exit(124)))
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
    half = WINDOW // 2
    res = {"symbols": int(n), "reads_indexed": R, "ktab_depth": g.ktab_depth(), "window_span": g.window_span(), "shards": 1, "runs": RUNS,
           "window": WINDOW, "k": K, "skip": SKIP, "max_interval_size": 10000, "read_stride": STRIDE}
    try:
        sym = np.frombuffer(b"$ACGT", np.uint8)
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
        args = (ss._s, pv(qtext), pv(qoff), Q, pv(qpos), pv(qalt), pv(qisalt), K, SKIP, 0)
        nr = C.c_size_t()
        first0 = np.zeros(Q + 1, np.uint64)
        rc = L.rsbwt_set_site_reads(*args, pv(first0), None, STRIDE, None, None, 0, C.byref(nr))
        assert rc in (0, -7), L.rsbwt_last_error()
        cap = nr.value
        assert cap > 0, "no read is kept: nothing to time"

        def route(fn):
            first = np.zeros(Q + 1, np.uint64)
            buf, ln, rr = np.zeros((cap, STRIDE), np.uint8), np.zeros(cap, np.uint32), np.zeros(cap, np.uint64)
            m = C.c_size_t()

            def call():
                chk(fn(*args, pv(first), pv(buf), STRIDE, pv(ln), pv(rr), cap, C.byref(m)))
                return m.value
            return call, (first, buf, ln, rr)

        new, out_new = route(L.rsbwt_set_site_reads)
        old, out_old = route(L.rsbwt_set_gt_aligned_reads)
        assert timed("site reads (warm-up)", new)[1] == cap
        wk = rsb.ShardSet.site_reads_last_work()
        assert timed("composed call (warm-up)", old)[1] == cap
        gw = rsb.ShardSet.gt_last_work()
        equal = bool(all((a == b).all() for a, b in zip(out_new[:1] + out_new[2:], out_old[:1] + out_old[2:])))
        equal = equal and all(out_new[1][i, :out_new[2][i]].tobytes() == out_old[1][i, :out_old[2][i]].tobytes() for i in range(cap))
        if not equal:
            raise RuntimeError("the composed call's reads are not the new call's")
        t_new = [timed("site reads", new)[0] for _ in range(RUNS)]
        t_old = [timed("composed call", old)[0] for _ in range(RUNS)]
        mn, mo = statistics.median(t_new), statistics.median(t_old)
        tiles = Q * len(range(0, WINDOW - K + 1, SKIP + 1))
        batch_up = int((qtext.size - 1) * 5 + Q * 20 + tiles * 8)  # text, nprev, q_off / q_pos / q_len, the slots' query and tile
        res.update({
            "reads_reported": cap, "work": wk, "new_ms": [round(t * 1e3, 3) for t in t_new], "composed_ms": [round(t * 1e3, 3) for t in t_old],
            "new_median_ms": round(mn * 1e3, 3), "composed_median_ms": round(mo * 1e3, 3), "composed_over_new": round(mo / mn, 2),
            # new: the batch and the requests' off / alt / isalt go up; first[], the reported reads' slots, lengths and rows, the
            # counters (8 counters 256 bytes apart and three words) and seven sizes come down
            "pcie_bytes_new": {"up": batch_up + (Q + 1) * 8 + 2 * Q, "down": int((Q + 1) * 8 + cap * (STRIDE + 12) + 8 * 32 * 8 + 24 + 7 * 8)},
            # composed: the batch goes up; the legs' records and the kept rows' records come down; the distinct reads' rows go up
            # and their slots (at max(stride, 256)) and lengths come down; the reads that pass the length rule go up again with the
            # requests that have one, and a verdict a read comes down
            "pcie_bytes_composed": {"up": int(batch_up + gw["extracted"] * 12 + wk["aligned"] * (READ_LEN + 16) + (qtext.size - 1) + Q * 18),
                                    "down": int(tiles * 2 * 32 + gw["kept"] * 24 + gw["extracted"] * (256 + 4) + wk["aligned"])},
            "reads_equal": equal})
        res["timing"] = "new_*, composed_*: wall clock from Python around the one C call, the copies into the caller's arrays included"
        res["pcie_note"] = ("bytes computed from the calls' arguments and counters (the composed call's from the record sizes in csrc/kernels.h), not "
                            "measured on the bus")
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
