#!/usr/bin/env python3
"""SiteMatch alignment rates (csrc/ksw_align.hip): READS reads of 100 symbols, each against the 199-symbol window of its
request -- the shape of GtTask::run's second half (src/service/service.cpp:1077-1108).  The reads are cut around the
request's site from the window and carry substitutions and, one in ten, an indel of 1-3.  Timed as medians of RUNS after a
warm-up:
    ksw_host   rsbwt_ksw_align      wall clock around the C call: ordering, upload, the launches, the copy back, the wait
    ksw_dev    rsbwt_ksw_align_dev  device events around LAUNCHES calls in a row, per call (nothing crosses PCIe)
    gt_host    rsbwt_gt_align       wall clock around the C call (two to five passes a read)
    gt_dev     rsbwt_gt_align_dev   device events, as above
Before any time is reported the device forms' outputs are asserted equal to the host forms', and SPOT pairs and verdicts to
tests/ksw_reference.py.  inputs(reads, seed) is what tools/ksw_cpu_baseline.py aligns with the reference's own ksw.c on CPU
threads, so the two are measured on the same pairs.  Every step runs under a time limit of its own (a step that outlasts it
ends the process with status 124).
usage: tools/ksw_probe.py [reads=100000] [out=profiles/ksw_probe.json]"""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

READ_LEN, WINDOW, REQUESTS, RUNS, LAUNCHES, SPOT, STEP_LIMIT_S, SEED = 100, 199, 500, 5, 5, 48, 120.0, 811


def inputs(reads, seed=SEED):
    """(read text u8, roff, item, window text u8, off, pos, alt u8, isalt u8): seeded, the same on every machine"""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    win = rng.integers(0, 4, (REQUESTS, WINDOW))
    pos = rng.integers(60, 140, REQUESTS).astype(np.uint64)  # 1-based
    alt = (win[np.arange(REQUESTS), pos.astype(np.int64) - 1] + rng.integers(1, 4, REQUESTS)) % 4
    isalt = rng.integers(0, 2, REQUESTS).astype(np.uint8)
    item = rng.integers(0, REQUESTS, reads).astype(np.uint64)
    out, lens = [], np.zeros(reads, np.int64)
    for i in range(reads):
        r = int(item[i])
        a = int(pos[r]) - 1 - int(rng.integers(5, READ_LEN - 5))
        a = max(0, min(WINDOW - READ_LEN, a))
        s = win[r, a:a + READ_LEN].copy()
        if rng.random() < 0.5:
            s[int(pos[r]) - 1 - a] = alt[r]
        for p in rng.integers(0, READ_LEN, int(rng.integers(0, 4))):
            s[p] = (s[p] + 1) % 4
        if i % 10 == 0:
            p, n = int(rng.integers(10, READ_LEN - 10)), int(rng.integers(1, 4))
            s = np.concatenate((s[:p], rng.integers(0, 4, n), s[p:-n])) if i % 20 == 0 else np.concatenate((s[:p], s[p + n:], rng.integers(0, 4, n)))
        out.append(acgt[s])
        lens[i] = len(s)
    roff = np.zeros(reads + 1, np.uint64)
    roff[1:] = np.cumsum(lens)
    off = np.arange(REQUESTS + 1, dtype=np.uint64) * np.uint64(WINDOW)
    return (np.append(np.concatenate(out), np.uint8(0)), roff, item, np.append(acgt[win].ravel(), np.uint8(0)), off, pos, acgt[alt].copy(), isalt)


def pair_windows(item, wtext, off):
    """the target side of the ksw pairs: every read's own copy of its request's window"""
    w2 = wtext[:-1].reshape(REQUESTS, WINDOW)[item.astype(np.int64)]
    return np.append(w2.ravel(), np.uint8(0)), np.arange(len(item) + 1, dtype=np.uint64) * np.uint64(WINDOW)


def timed(what, fn):
    guard = threading.Timer(STEP_LIMIT_S, lambda: (sys.stderr.write(f"ksw_probe: {what} exceeded {STEP_LIMIT_S} s\n"), os._exit(124)))
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
    import readserver_amd as rsb
    import ksw_reference as kr
    n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 100000
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "ksw_probe.json")
    L = rsb.lib()
    if L.rsbwt_device_count() <= 0:
        raise SystemExit("ksw_probe: no GPU -- nothing is measured without one")
    rtext, roff, item, wtext, off, pos, alt, isalt = inputs(n)
    ttext, toff = pair_windows(item, wtext, off)
    pv = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    chk = lambda rc: rc == 0 or (_ for _ in ()).throw(RuntimeError(L.rsbwt_last_error().decode()))  # noqa: E731
    res_h, ver_h = np.zeros((n, 6), np.int32), np.zeros(n, np.uint8)
    ksw_host = lambda: chk(L.rsbwt_ksw_align(0, None, pv(rtext), pv(roff), pv(ttext), pv(toff), n, pv(res_h)))  # noqa: E731
    gt_host = lambda: chk(L.rsbwt_gt_align(0, pv(rtext), pv(roff), pv(item), n, pv(wtext), pv(off), pv(pos), pv(alt), pv(isalt), REQUESTS, pv(ver_h)))  # noqa: E731
    timed("ksw host form (warm-up)", ksw_host)
    timed("gt host form (warm-up)", gt_host)
    work = rsb.gt_align_last_work()
    # spot check against the restatement
    rb, wb = rtext.tobytes(), wtext.tobytes()
    for i in np.random.default_rng(1).integers(0, n, SPOT):
        s, r = rb[int(roff[i]):int(roff[i + 1])], int(item[i])
        w = wb[int(off[r]):int(off[r + 1])]
        assert tuple(res_h[i, :5]) == kr.ksw_align(kr.code(s), kr.code(w)), i
        assert int(ver_h[i]) == kr.align_gt_read(s.decode(), w.decode(), int(pos[r]), chr(alt[r]), bool(isalt[r])), i
    t_ksw = [timed("ksw host form", ksw_host)[0] for _ in range(RUNS)]
    t_gt = [timed("gt host form", gt_host)[0] for _ in range(RUNS)]
    # device forms
    d = {k: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8)).cuda()
         for k, a in dict(rtext=rtext, roff=roff, item=item, wtext=wtext, off=off, pos=pos, alt=alt, isalt=isalt, ttext=ttext, toff=toff).items()}
    d_res = torch.zeros(n * 24, dtype=torch.uint8, device="cuda")
    d_ver = torch.zeros(n, dtype=torch.uint8, device="cuda")

    def events(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rc = 0
        for _ in range(LAUNCHES):
            rc = rc or call()
        e1.record()
        torch.cuda.synchronize()
        chk(rc)
        return e0.elapsed_time(e1) * 1e-3 / LAUNCHES
    ksw_dev = lambda: L.rsbwt_ksw_align_dev(None, p(d["rtext"]), p(d["roff"]), p(d["ttext"]), p(d["toff"]), n, p(d_res), 0, None)  # noqa: E731
    gt_dev = lambda: L.rsbwt_gt_align_dev(p(d["rtext"]), p(d["roff"]), p(d["item"]), n, p(d["wtext"]), p(d["off"]), p(d["pos"]), p(d["alt"]),  # noqa: E731
                                          p(d["isalt"]), REQUESTS, p(d_ver), 0, None)
    timed("ksw device form (warm-up)", lambda: events(ksw_dev))
    timed("gt device form (warm-up)", lambda: events(gt_dev))
    assert (d_res.cpu().numpy().view(np.int32).reshape(n, 6) == res_h).all(), "the device form's answers are not the host form's"
    assert (d_ver.cpu().numpy() == ver_h).all(), "the device form's verdicts are not the host form's"
    t_ksw_dev = [timed("ksw device form", lambda: events(ksw_dev))[1] for _ in range(RUNS)]
    t_gt_dev = [timed("gt device form", lambda: events(gt_dev))[1] for _ in range(RUNS)]
    cells = int(((roff[1:] - roff[:-1]) * np.uint64(WINDOW)).sum())
    med = statistics.median
    res = {"reads": n, "read_len": READ_LEN, "window": WINDOW, "requests": REQUESTS, "seed": SEED, "runs": RUNS,
           "launches_per_device_timing": LAUNCHES, "cells_per_forward_pass": cells, "spot_checked": SPOT,
           "verdicts": work["by_verdict"], "kept": sum(work["by_verdict"][v] for v in (9, 11, 13)),
           "ksw_host_ms": [round(t * 1e3, 3) for t in t_ksw], "ksw_dev_ms": [round(t * 1e3, 3) for t in t_ksw_dev],
           "gt_host_ms": [round(t * 1e3, 3) for t in t_gt], "gt_dev_ms": [round(t * 1e3, 3) for t in t_gt_dev],
           "ksw_host_pairs_per_s": round(n / med(t_ksw), 1), "ksw_dev_pairs_per_s": round(n / med(t_ksw_dev), 1),
           "gt_host_reads_per_s": round(n / med(t_gt), 1), "gt_dev_reads_per_s": round(n / med(t_gt_dev), 1),
           "ksw_dev_forward_cells_per_s": round(cells / med(t_ksw_dev), 1),
           "device_forms_agree_with_host_forms": True, "checksum_score_sum": int(res_h[:, 0].astype(np.int64).sum()),
           "timing": ("*_host_*: wall clock from Python around the C call, which ends in a stream synchronise; *_dev_*: events around "
                      f"{LAUNCHES} device-resident calls in a row, per call.  A ksw pair is a forward and a reversed pass; "
                      "cells_per_forward_pass counts the forward pass alone")}
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
