"""The one-lane search kernel's staged results (csrc/search_solo.h) with a group of 8 results in ANY free LDS buffer: the
i-th group that begins among a pass's draws takes the i-th free buffer, every lane keeps its query's buffer number, and a
group whose queries are drawn over two passes hands its buffer on through a wave-uniform pair.  Every answer is held
against the oracle's findInterval on the same run bytes, in both result layouts, from the plain and from the counting
instantiation of the kernel.

The batches run in ONE child process (tools/staged_any_buffer_probe.py), as tests/test_gpu_staged_results.py's do: the
library reads RSBWT_SEARCH_KERNEL and RSBWT_COUNT_UNSTAGED once per process."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ESCAPED = 2**24 - 1  # search_solo.h, RES_ESCAPED: the narrowest width that does not fit a slot

# The results that left unstaged on the two-shard set at 600,003 queries (1,200,006 results) when a group's buffer was
# g mod 28: the parent commit's library on the same box and in the same visit as this one's, profiles/staged_any_buffer_ab.json
# ("unstaged_counter", "parent").  Which wave draws which chunk varies from run to run, and the model of one wave
# (tools/staged_buffer_model.py) predicts a drop of far more than tenfold: the cap is a quarter.
PARENT_UNSTAGED = {"unstaged_pairs": 390_176, "unstaged_separate_arrays": 394_936}


def _probe_module():
    """the probe's shapes and helpers (importing it sets no environment variable: only its main() does, in the child)"""
    spec = importlib.util.spec_from_file_location("staged_any_buffer_probe", os.path.join(ROOT, "tools", "staged_any_buffer_probe.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def probe(rsb):
    return _probe_module()


@pytest.fixture(scope="module")
def ran(rsb, probe, tmp_path_factory):
    """the child's queries and answers (npz) and its report line"""
    out = str(tmp_path_factory.mktemp("staged_any") / "staged_any.npz")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "staged_any_buffer_probe.py"), "--out", out],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    report = json.loads(r.stdout.strip().splitlines()[-1])
    print(json.dumps(report["cases"]))
    return np.load(out), report


@pytest.fixture(scope="module")
def oracles(oracle, probe):
    """the oracle of every shard the probe builds, by (run bytes, seed): made once"""
    shards = set(probe.SET3_SHARDS) | set(probe.base.SET_SHARDS)
    return {s: oracle.from_runs(probe.base.pop_runs(*s)) for s in sorted(shards)}


def _hold(npz, name, oixs):
    """every layout and both instantiations of case `name` against the oracles of its shards; returns the oracle's"""
    km = npz[name + ".km"]
    want = [oix.find_intervals(km, nthreads=8) for oix in oixs]
    elo, eup = np.stack([w[0] for w in want]), np.stack([w[1] for w in want])
    for tag in ("", "_counting"):
        lo, up, pr = npz[f"{name}.lo{tag}"], npz[f"{name}.up{tag}"], npz[f"{name}.pairs{tag}"]
        assert lo.shape == elo.shape and pr.shape == elo.shape + (2,)
        assert np.array_equal(lo, elo) and np.array_equal(up, eup), (name, tag, "separate arrays")
        assert np.array_equal(pr[..., 0], elo) and np.array_equal(pr[..., 1], eup), (name, tag, "pairs")
    return km, elo, eup


def _mixed(km, elo, eup, Q, k):
    """what makes the batch a mixed one: two invalid queries, the ones drawn from shard 0 live there, random ones die"""
    assert km.shape == (Q, k) and Q % 8 != 0
    bad = (km == ord("N")).any(1)
    assert bad.sum() == 2 and (elo[:, bad] == 1).all() and (eup[:, bad] == 0).all()
    live = eup[0] >= elo[0]
    assert live[::2][~bad[::2]].all() and not live[1::2].all()


@pytest.mark.parametrize("Q", [4099, 61])
def test_gpu_any_buffer_three_unequal_shards(ran, probe, oracles, Q):
    """Three `pop` shards of 10^6, 6*10^5 and 3*10^5 run bytes behind 9-mer tables; 31-mers half drawn from shard 0 and
    half random, interleaved, two of them with an N.  The waves finish a shard at times of their own and go on to the
    next with other waves' groups still open; the buffers are reset per wave and shard.  Q = 4099 = 8 n + 3: a tail group
    of 3; Q = 61: less than one wave, a tail group of 5."""
    assert Q in probe.SET3_Q
    sizes = [R for R, _ in probe.SET3_SHARDS]
    assert sizes == [1_000_000, 600_000, 300_000]
    npz, _ = ran
    km, elo, eup = _hold(npz, f"set3_Q{Q}", [oracles[s] for s in probe.SET3_SHARDS])
    _mixed(km, elo, eup, Q, 31)
    assert ((eup + np.uint64(1) == elo) & (elo != 1)).any()  # an empty interval after a step keeps its own values


def test_gpu_any_buffer_three_unequal_shards_at_k_40(ran, probe, oracles):
    """The same set at k = 40: a query of two packed words (the kernel's LONGK instantiations)."""
    npz, _ = ran
    km, elo, eup = _hold(npz, f"set3_k{probe.LONG_K}_Q{probe.LONG_Q}", [oracles[s] for s in probe.SET3_SHARDS])
    assert probe.LONG_K == 40 and probe.LONG_Q == 4099
    _mixed(km, elo, eup, 4099, 40)


def test_gpu_any_buffer_single_shard_that_makes_its_own_start_records(ran, probe, oracles):
    """Shard 0 alone: behind a table this deep the launch makes its own start records (FUSED) -- a reserve is taken up
    two passes after its draw, and its buffer number waits with it."""
    npz, _ = ran
    n, T, span = (int(x) for x in npz["shard0"])
    assert T == probe.SET_KTAB and ((n >> (2 * T)) << 2) <= span  # capi_internal.h, view_is_narrow: what makes the launch FUSED
    km, elo, eup = _hold(npz, "one_Q4099", [oracles[probe.SET3_SHARDS[0]]])
    _mixed(km, elo, eup, 4099, 31)


def test_gpu_any_buffer_leaves_at_most_a_quarter_of_the_parents_unstaged_results(ran, probe, oracles):
    """tests/test_gpu_staged_results.py's exhaustion shape -- the two-shard set at 600,003 queries, 36 groups of 8 per
    wave -- under RSBWT_COUNT_UNSTAGED with a counting launch.  With g mod 28 about a third of the 1,200,006 results left
    unstaged (PARENT_UNSTAGED); with any free buffer a group goes unstaged only when all 28 are taken."""
    npz, report = ran
    assert probe.COUNT_Q == 600_003 and probe.base.SET_SHARDS == ((1_000_000, probe.POP | 11), (1_000_000, probe.POP | 12))
    name = f"count_Q{probe.COUNT_Q}"
    km, elo, eup = _hold(npz, name, [oracles[s] for s in probe.base.SET_SHARDS])
    assert km.shape == (600_003, 31)
    c = report["cases"][name]
    assert c["results"] == 1_200_006
    for layout, parent in PARENT_UNSTAGED.items():
        print(f"{layout}: {c[layout]} unstaged of {c['results']} results (parent: {parent}, cap {parent // 4})")
    for layout, parent in PARENT_UNSTAGED.items():
        assert 0 <= c[layout] <= c["results"], c
        assert 4 * c[layout] <= parent, (layout, c[layout], parent)


def test_gpu_any_buffer_escape_for_intervals_too_wide_for_a_slot(ran, probe, oracle):
    """One `pop` shard of 2*10^7 run bytes, 403 queries of the four bases: the 1-mers' intervals are wider than a slot
    holds (>= 2^24 - 1 rows), so every one leaves by its lane's own store from inside a claimed buffer and the flush
    skips its slot -- the unstaged count is Q exactly, as before; the 2-mers' all fit."""
    npz, report = ran
    oix = oracle.from_runs(probe.base.pop_runs(*probe.ESCAPE_SHARD))
    Q = probe.ESCAPE_Q
    assert Q == 403
    for k, too_wide in ((1, True), (2, False)):
        km, elo, eup = _hold(npz, f"escape_k{k}_Q{Q}", [oix])
        assert km.shape == (Q, k) and len(np.unique(km, axis=0)) == 4**k
        width = eup[0] - elo[0] + np.uint64(1)
        assert (width >= ESCAPED).all() if too_wide else (width < ESCAPED).all(), (k, int(width.min()), int(width.max()))
        c = report["cases"][f"escape_k{k}_Q{Q}"]
        print(k, c)
        for layout in ("unstaged_pairs", "unstaged_separate_arrays"):
            if too_wide:
                assert c[layout] == Q, c  # k = 1: every result by its lane's own store, none twice
            else:
                assert c[layout] < Q, c
