"""The one-lane search kernel's staged results (csrc/search_solo.h): 8-byte {lower:40, width:24} slots in LDS, flushed by
the line; a result that does not fit a slot leaves by its own lane's store.  Every answer is held against the oracle's
findInterval on the same run bytes.

The batches run in ONE child process (tools/staged_results_probe.py): which kernel a plain search takes and whether the
unstaged results are counted are read by the library once per process (RSBWT_SEARCH_KERNEL, RSBWT_COUNT_UNSTAGED), and
batches of these sizes run on lane pairs otherwise.  Every batch goes through both result layouts, and through the
plain and the counting instantiation of the kernel."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WRAPPED = 2**64 - 1
ESCAPED = 2**24 - 1  # search_solo.h, RES_ESCAPED: the narrowest width that does not fit a slot


def _probe_module():
    """the probe's shapes and helpers (importing it sets no environment variable: only its main() does, in the child)"""
    spec = importlib.util.spec_from_file_location("staged_results_probe", os.path.join(ROOT, "tools", "staged_results_probe.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def probe(rsb):
    return _probe_module()


@pytest.fixture(scope="module")
def ran(rsb, probe, tmp_path_factory):
    """the child's queries and answers (npz) and its report line"""
    out = str(tmp_path_factory.mktemp("staged") / "staged.npz")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "staged_results_probe.py"), "--out", out],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    report = json.loads(r.stdout.strip().splitlines()[-1])
    print(json.dumps(report["cases"]))
    return np.load(out), report


@pytest.fixture(scope="module")
def set_oracles(oracle, probe):
    return [oracle.from_runs(probe.pop_runs(R, seed)) for R, seed in probe.SET_SHARDS]


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


@pytest.mark.parametrize("Q", [4099, 61])
def test_gpu_staged_results_mixed_batch_on_a_two_shard_set(ran, probe, set_oracles, Q):
    """Two `pop` shards of 10^6 run bytes, 31-mers half drawn from shard 0 and half random, interleaved: long and short
    searches side by side in every wave, groups of 8 stay open.  Q = 8 n + 3 (a tail group of 3) and Q = 61 (less than
    a wave).  Every (lower, upper) of every shard, the empty intervals' exact values and the (1, 0) of the queries with an
    invalid symbol included, in both layouts."""
    assert Q in probe.MIXED_Q and Q % 8 != 0
    npz, _ = ran
    km, elo, eup = _hold(npz, f"mixed_set_Q{Q}", set_oracles)
    assert km.shape == (Q, 31)
    bad = (km == ord("N")).any(1)
    assert bad.sum() == 2 and (elo[:, bad] == 1).all() and (eup[:, bad] == 0).all()
    live = eup[0] >= elo[0]
    assert live[::2][~bad[::2]].all() and not live[1::2].all()  # drawn from shard 0: they occur there; random ones die
    assert ((eup + np.uint64(1) == elo) & (elo != 1)).any()  # an empty interval after a step keeps its own values


@pytest.mark.parametrize("Q", [4099, 61])
def test_gpu_staged_results_single_shard_that_makes_its_own_start_records(ran, probe, set_oracles, Q):
    """The same batches on shard 0 alone: behind a table this deep the single-shard launch makes its own start records
    (FUSED) and stages its results with the same code."""
    npz, report = ran
    n, T, span = (int(x) for x in npz["shard0"])
    assert T == probe.SET_KTAB and ((n >> (2 * T)) << 2) <= span  # capi_internal.h, view_is_narrow: what makes the launch FUSED
    _hold(npz, f"mixed_one_Q{Q}", set_oracles[:1])


def test_gpu_staged_results_escape_for_intervals_too_wide_for_a_slot(ran, probe, oracle):
    """One `pop` shard of 2*10^7 run bytes = 117,196,177 symbols: the four 1-mers' intervals are 28,712,613 to 28,749,806
    rows wide (>= 2^24 - 1 = 16,777,215: no slot holds them, every one leaves by its lane's own store), the 2-mers'
    7,026,249 to 7,060,116 (every one fits).  403 queries per batch, the four bases only, so every group of 8 mixes
    them; and 61, which one wave draws at once: every group then finds its buffer free (a wave that draws several chunks
    can find the buffer of a group taken by a group of another chunk), and the direct stores counted are the escape's alone."""
    npz, report = ran
    oix = oracle.from_runs(probe.pop_runs(*probe.ESCAPE_SHARD))
    for k, too_wide in ((1, True), (2, False)):
        for Q in probe.ESCAPE_Q:
            km, elo, eup = _hold(npz, f"escape_k{k}_Q{Q}", [oix])
            assert km.shape == (Q, k) and len(np.unique(km, axis=0)) == 4**k
            width = eup[0] - elo[0] + np.uint64(1)
            assert (width >= ESCAPED).all() if too_wide else (width < ESCAPED).all(), (k, int(width.min()), int(width.max()))
            c = report["cases"][f"escape_k{k}_Q{Q}"]
            for layout in ("unstaged_pairs", "unstaged_separate_arrays"):
                if too_wide:
                    assert c[layout] == Q, c  # k = 1: every result by its lane's own store
                elif Q <= 64:
                    assert c[layout] == 0, c  # k = 2: none
                else:
                    assert c[layout] < Q, c


def test_gpu_staged_results_wrapped_interval(ran, probe, oracle):
    """A BWT without terminators whose first rows hold no A (test_gpu_interval_at_the_top_of_a_bwt_without_terminators'
    construction): a step from lower = 0 that finds none gives upper = 2^64 - 1, and the reference carries on.  Every
    eighth query ends ON that interval, (0, 2^64 - 1) -- width 0 in its slot -- every fourth passes through it, the rest
    are ordinary 24-mers: the case sits inside ordinary groups."""
    npz, _ = ran
    km, elo, eup = _hold(npz, "wrapped", [oracle.from_runs(probe.wrapped_runs())])
    wrapped = (elo[0] == 0) & (eup[0] == WRAPPED)
    assert wrapped[3::8].all() and 0 < wrapped.sum() < km.shape[0] // 4
    groups = wrapped[:400].reshape(-1, 8)
    assert (groups.any(1) & ~groups.all(1)).all()  # every group of 8 holds the case beside other results


def test_gpu_staged_results_when_a_wave_opens_more_groups_than_it_has_buffers(ran, probe, set_oracles):
    """The two-shard set at 600,003 queries per batch: 2 Q searches over the launch's 4,096 waves are 36 groups of 8 per
    wave, more than the 28 buffers.  The answers are the oracle's whatever left unstaged; the counter of unstaged results
    (word 15 of a counting launch under RSBWT_COUNT_UNSTAGED) must be non-zero for some seed: a group that finds its
    buffer taken.  The shape is the first test's, only larger: nothing here is built to force the case."""
    npz, report = ran
    unstaged = []
    for seed in probe.EXHAUST_SEEDS:
        name = f"exhaust_seed{seed}"
        km, elo, eup = _hold(npz, name, set_oracles)
        assert km.shape == (probe.EXHAUST_Q, 31)
        c = report["cases"][name]
        assert c["results"] == 2 * probe.EXHAUST_Q
        assert 0 <= c["unstaged_pairs"] <= c["results"] and 0 <= c["unstaged_separate_arrays"] <= c["results"]
        unstaged += [c["unstaged_pairs"], c["unstaged_separate_arrays"]]
    print("unstaged results per launch:", unstaged)
    assert any(u > 0 for u in unstaged), unstaged
