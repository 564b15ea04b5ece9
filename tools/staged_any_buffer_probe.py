"""The one-lane search kernel's STAGED RESULTS (csrc/search_solo.h) where a group of 8 results takes ANY free LDS buffer:
the shapes on which the choice of buffer and its hand-over from lane to lane can go wrong -- the GPU half of
tests/test_gpu_staged_any_buffer.py, runnable by hand:

    python tools/staged_any_buffer_probe.py [--out FILE.npz] [--count-only]

Three `pop` shards of unequal size behind 9-mer tables (waves change shard at different times, with groups open), at
31 and at 40 symbols (k > 32: a query of two packed words), the first shard alone (the launch that makes its own start
records), the two-shard set of tools/staged_results_probe.py at 600,003 queries (the unstaged results counted: what
`g mod 28` left out and any free buffer does not), and the 1- and 2-mers of its 1.2e8-symbol shard (results too wide for
a slot among results that fit).  Helpers, knobs and the report are that probe's; --count-only runs the counted set
alone (an A/B of two builds: RSBWT_LIB picks the library)."""
import importlib.util
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import readserver_amd as rsb  # noqa: E402


def _base():
    spec = importlib.util.spec_from_file_location("staged_results_probe", os.path.join(HERE, "staged_results_probe.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


base = _base()
POP = base.POP
SET3_SHARDS = (base.SET_SHARDS[0], (600_000, POP | 21), (300_000, POP | 22))  # (run bytes, seed); shard 0 is the other probe's
SET_KTAB = base.SET_KTAB
SET3_Q = (4099, 61)  # 8 n + 3: a tail group of 3; less than one wave
LONG_K, LONG_Q = 40, 4099
COUNT_Q, COUNT_SEED = base.EXHAUST_Q, base.EXHAUST_SEEDS[0]
ESCAPE_SHARD, ESCAPE_Q = base.ESCAPE_SHARD, 403


def mixed_kmers(g0, Q, k, seed):
    """staged_results_probe.mixed_kmers at any k: half drawn from shard g0, half random, interleaved; two invalid ones"""
    import torch
    km = base.random_kmers(np.random.default_rng(seed), Q, k)
    half = (Q + 1) // 2
    d_half = torch.empty((half, k), dtype=torch.uint8, device="cuda:0")
    assert rsb.lib().rsbwt_sample_present_kmers_dev(g0.handle, half, k, k, seed, base._p(d_half), None) == 0
    torch.cuda.synchronize()
    km[::2] = d_half.cpu().numpy()
    km[5, 3] = ord("N")
    km[Q - 2, 0] = ord("N")
    return km


def main(argv):
    os.environ["RSBWT_SEARCH_KERNEL"] = "solo"   # (before the process's first search: the library latches them there)
    os.environ["RSBWT_COUNT_UNSTAGED"] = "1"
    out_path = argv[argv.index("--out") + 1] if "--out" in argv else None
    count_only = "--count-only" in argv
    cases = {}
    g0 = rsb.GpuBWT(runs=base.pop_runs(*SET3_SHARDS[0]), ktab_depth=SET_KTAB)
    n0, T0, span0 = int(g0.getBWLen()), g0.ktab_depth(), g0.window_span()
    if not count_only:
        rest = [rsb.GpuBWT(runs=base.pop_runs(R, seed), ktab_depth=SET_KTAB) for R, seed in SET3_SHARDS[1:]]
        ss = rsb.ShardSet([g0] + rest)
        for Q in SET3_Q:
            km = mixed_kmers(g0, Q, base.K, 300 + Q)
            cases[f"set3_Q{Q}"] = base.search(ss, km, 3)
            if Q == LONG_Q:
                cases[f"one_Q{Q}"] = base.search(g0, km, None)
        cases[f"set3_k{LONG_K}_Q{LONG_Q}"] = base.search(ss, mixed_kmers(g0, LONG_Q, LONG_K, 340), 3)
        ss.close()
        for g in rest:
            g.close()
    g1 = rsb.GpuBWT(runs=base.pop_runs(*base.SET_SHARDS[1]), ktab_depth=SET_KTAB)
    ss = rsb.ShardSet([g0, g1])
    cases[f"count_Q{COUNT_Q}"] = base.search(ss, base.mixed_kmers(g0, COUNT_Q, COUNT_SEED), 2)
    ss.close()
    g1.close()
    g0.close()
    if not count_only:
        with rsb.GpuBWT(runs=base.pop_runs(*ESCAPE_SHARD), ktab_depth=None) as g:
            for k in (1, 2):
                cases[f"escape_k{k}_Q{ESCAPE_Q}"] = base.search(g, base.random_kmers(np.random.default_rng(20 + k), ESCAPE_Q, k), None)
    report = {"library": os.path.abspath(rsb.lib_path()), "shard0": {"symbols": n0, "ktab_depth": T0, "window_span": span0}, "cases": {}}
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
