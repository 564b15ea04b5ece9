"""The one-lane search kernel's STAGED RESULTS (csrc/search_solo.h) on batches of every shape that takes a path of its
own there, and the share of results that left unstaged -- the GPU half of tests/test_gpu_staged_results.py, runnable by hand:

    python tools/staged_results_probe.py [--out FILE.npz] [--big Q]

Every plain search of this process runs on the one-lane kernel (RSBWT_SEARCH_KERNEL=solo; a batch of a few thousand
queries would otherwise run on lane pairs) and counting launches add the results stored by their own lane to word 15
of the counters (RSBWT_COUNT_UNSTAGED): both are read by the library once per process, at its first search, hence a
process of its own -- main() sets them; importing this file for its shapes and helpers sets nothing.
Prints one JSON line: per batch the results, the unstaged ones (buffer taken, or the result does not fit a slot) and
their share.  --out: the queries and every answer, for the caller to hold against the oracle.  --big Q: only the
two-shard set at Q queries per batch (default run: the test's shapes)."""
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import readserver_amd as rsb  # noqa: E402

POP = 1 << 62  # the `pop` run stream (bench.py, STREAM_STYLE)
K = 31
SET_SHARDS = ((1_000_000, POP | 11), (1_000_000, POP | 12))  # (run bytes, seed)
SET_KTAB = 9          # narrow at this size (capi_internal.h, view_is_narrow): shard 0 alone runs FUSED
MIXED_Q = (4099, 61)  # 8 n + 3: a tail group of 3; less than one wave
EXHAUST_Q, EXHAUST_SEEDS = 600_003, (1, 2)  # 2 Q / 4096 waves / 8 = 36 groups per wave > RES_BUFS = 28
ESCAPE_SHARD = (20_000_000, POP | 77)
ESCAPE_Q = (403, 61)  # 61: one draw of one wave, so every group finds its buffer free and only the escape stores directly
WRAPPED_Q, WRAPPED_K = 403, 24


def pop_runs(R, seed):
    runs = np.empty(R, np.uint8)
    assert rsb.lib().rsbwt_synth_runs_host(runs.ctypes.data, R, seed) == 0
    return runs


def wrapped_runs():
    """tests/test_gpu_parity.py, test_gpu_interval_at_the_top_of_a_bwt_without_terminators: no '$', long runs"""
    rng = np.random.default_rng(12)
    return (rng.integers(1, 5, 60000).astype(np.uint8) << 5) | 31


def random_kmers(rng, Q, k):
    return np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, (Q, k))].copy()


def wrapped_kmers():
    """ordinary random 24-mers; every fourth with the poly-A stretch that keeps lower at 0 (the wrap happens on the way);
    every eighth all A: its search ENDS on the wrapped interval (0, 2^64 - 1)"""
    km = random_kmers(np.random.default_rng(13), WRAPPED_Q, WRAPPED_K)
    km[1::4, 12:23] = ord("A")
    km[3::8, :] = ord("A")
    return km


def _p(t):
    return C.c_void_p(t.data_ptr())


def mixed_kmers(g0, Q, seed):
    """half drawn from shard 0 (all 30 steps there), half random (they die early), interleaved; two invalid ones"""
    import torch
    km = random_kmers(np.random.default_rng(seed), Q, K)
    half = (Q + 1) // 2
    d_half = torch.empty((half, K), dtype=torch.uint8, device="cuda:0")
    assert rsb.lib().rsbwt_sample_present_kmers_dev(g0.handle, half, K, K, seed, _p(d_half), None) == 0
    torch.cuda.synchronize()
    km[::2] = d_half.cpu().numpy()
    km[5, 3] = ord("N")
    km[Q - 2, 0] = ord("N")
    return km


def search(target, km, nshards):
    """both result layouts, each by a plain and by a counting launch (two instantiations of the kernel);
    target: a GpuBWT or a ShardSet"""
    import torch
    L = rsb.lib()
    is_set = nshards is not None
    S = nshards if is_set else 1
    h = target._s if is_set else target.handle
    find = L.rsbwt_set_find_intervals_dev if is_set else L.rsbwt_find_intervals_dev
    find_pairs = L.rsbwt_set_find_interval_pairs_dev if is_set else L.rsbwt_find_interval_pairs_dev
    counting = L.rsbwt_set_set_counting if is_set else L.rsbwt_set_counting
    counters = L.rsbwt_set_last_search_counters if is_set else L.rsbwt_last_search_counters
    Q, k = km.shape
    d_km = torch.from_numpy(km).cuda()
    d_pk = torch.empty((Q, (k + 31) // 32), dtype=torch.int64, device="cuda:0")
    d_ok = torch.empty(Q, dtype=torch.uint8, device="cuda:0")
    assert L.rsbwt_pack_kmers_dev(_p(d_km), Q, k, k, _p(d_pk), _p(d_ok), 0, None) == 0
    out = {"km": km}
    w = (C.c_uint64 * 16)()
    for tag, on in (("", 0), ("_counting", 1)):
        d_lo = torch.full((S, Q), -7, dtype=torch.int64, device="cuda:0")
        d_up = torch.full((S, Q), -7, dtype=torch.int64, device="cuda:0")
        d_pr = torch.full((S, Q, 2), -7, dtype=torch.int64, device="cuda:0")
        assert counting(h, on) == 0
        assert find(h, _p(d_pk), _p(d_ok), Q, k, _p(d_lo), _p(d_up), None) == 0
        torch.cuda.synchronize()
        if on:
            assert counters(h, w) == 0
            assert int(w[12]) == 1, "the batch did not run on the one-lane kernel"
            out["unstaged_arrays"] = np.uint64(w[15])
        assert find_pairs(h, _p(d_pk), _p(d_ok), Q, k, _p(d_pr), None) == 0
        torch.cuda.synchronize()
        if on:
            assert counters(h, w) == 0
            out["unstaged_pairs"] = np.uint64(w[15])
        assert counting(h, 0) == 0
        out["lo" + tag] = d_lo.cpu().numpy().view(np.uint64)
        out["up" + tag] = d_up.cpu().numpy().view(np.uint64)
        out["pairs" + tag] = d_pr.cpu().numpy().view(np.uint64)
    return out


def main(argv):
    os.environ["RSBWT_SEARCH_KERNEL"] = "solo"   # (before the process's first search: the library latches them there)
    os.environ["RSBWT_COUNT_UNSTAGED"] = "1"
    out_path = argv[argv.index("--out") + 1] if "--out" in argv else None
    big = int(float(argv[argv.index("--big") + 1])) if "--big" in argv else 0
    cases = {}
    shards = [rsb.GpuBWT(runs=pop_runs(R, seed), ktab_depth=SET_KTAB) for R, seed in SET_SHARDS]
    ss = rsb.ShardSet(shards)
    if big:
        cases[f"set_Q{big}"] = search(ss, mixed_kmers(shards[0], big, 1), len(shards))
    else:
        for Q in MIXED_Q:
            km = mixed_kmers(shards[0], Q, 100 + Q)
            cases[f"mixed_set_Q{Q}"] = search(ss, km, len(shards))
            cases[f"mixed_one_Q{Q}"] = search(shards[0], km, None)
        for seed in EXHAUST_SEEDS:
            cases[f"exhaust_seed{seed}"] = search(ss, mixed_kmers(shards[0], EXHAUST_Q, seed), len(shards))
    n0, T0, span0 = int(shards[0].getBWLen()), shards[0].ktab_depth(), shards[0].window_span()
    ss.close()
    for g in shards:
        g.close()
    if not big:
        with rsb.GpuBWT(runs=pop_runs(*ESCAPE_SHARD), ktab_depth=None) as g:
            for k in (1, 2):
                for Q in ESCAPE_Q:
                    cases[f"escape_k{k}_Q{Q}"] = search(g, random_kmers(np.random.default_rng(20 + k), Q, k), None)
        with rsb.GpuBWT(runs=wrapped_runs(), ktab_depth=None) as g:
            cases["wrapped"] = search(g, wrapped_kmers(), None)
    report = {"shard0": {"symbols": n0, "ktab_depth": T0, "window_span": span0}, "cases": {}}
    for name, c in cases.items():
        n = int(c["lo"].size)
        report["cases"][name] = {"results": n, "unstaged_separate_arrays": int(c["unstaged_arrays"]), "unstaged_pairs": int(c["unstaged_pairs"]),
                                 "unstaged_share_pairs": round(int(c["unstaged_pairs"]) / n, 4)}
    if out_path:
        flat = {f"{name}.{key}": v for name, c in cases.items() for key, v in c.items()}
        flat["shard0"] = np.array([n0, T0, span0], np.uint64)
        np.savez(out_path, **flat)
    print(json.dumps(report), flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
