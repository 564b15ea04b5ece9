"""Site sample counts on the GPU beyond the gt fixture (-m gpu): rsbwt_set_site_sample_counts on the read sets, dealings
and requests of tests/site_sets_reference.py -- reads of 12 to 600 symbols dealt so that only some shards have reads over 256
symbols, one shard has no candidate row and one no pair; tandem repeats with exact duplicates; one read of exactly 4,096
symbols.  Every case goes through tests/test_gpu_site_counts.py's _check: the four outputs bit-exact, work10 against the
restatement, and legs, narrow_steps, candidates and kept against rsbwt_set_gt_last_work of gt_count on the same set.
tests/test_site_sets_reference.py shows on the CPU what these inputs reach."""
import pytest

import site_sets_reference as SS
from test_gpu_site_counts import KEYS, OUT, _build, _check, _close, _got, _open

pytestmark = pytest.mark.gpu

RAGGED = [(d, p) for d in SS.DEALINGS["ragged-alleles"] for p in SS.PARAMS["ragged-alleles"]]
REPEAT = [(d, p) for d in SS.DEALINGS["repeat"] for p in SS.PARAMS["repeat"]]


def _ids(cases):
    return [f"{d}-M{p[0]}-k{p[1]}-skip{p[2]}" for d, p in cases]


def _two_groups(rsb, monkeypatch):
    if rsb.lib().rsbwt_device_count() < 2:
        monkeypatch.setenv("RSBWT_ENABLE_TEST_HOOKS", "1")
        monkeypatch.setenv("RSBWT_TEST_DEVICE_ALIASES", "2")


def _run(rsb, r, params, where, **how):
    gs = _open(rsb, r, **how)
    ss = rsb.ShardSet(gs)
    try:
        _build(ss, r.pairs)
        return [_check(ss, rsb, r, M, k, skip, (where, M, k, skip)) for M, k, skip in params]
    finally:
        _close(ss, gs)


@pytest.mark.parametrize("dealing,params", RAGGED, ids=_ids(RAGGED))
def test_gpu_site_sets_ragged_alleles(rsb, oracle, dealing, params):
    """one shard, the dealing over four (wide reads in shards 1 and 3 only, no candidate in shard 2, no pair in shard 0)
    and round-robin over eight, behind 6-mer tables"""
    r = SS.get(oracle, "ragged-alleles", dealing)
    got, = _run(rsb, r, [params], dealing)
    wk = got["work"]
    assert wk["candidates"] > wk["kept"] > wk["head_rows"] > wk["aligned"] > wk["carriers"] > 0 and wk["extracted"] < wk["aligned"]
    assert all(got["carriers"][a] > 0 and got["carriers"][b] > 0 for a, b in r.alleles[-1:])  # the wide windows keep long reads


@pytest.mark.parametrize("how", [dict(span=128), dict(span=2944), dict(ktab=None), dict(grouped=True)], ids=["S128", "S2944", "notable", "grouped"])
def test_gpu_site_sets_wide_dealing_on_line_layouts(rsb, oracle, how):
    """the dealing over four at window spans 128 and 2,944, with no table and with a grouped one"""
    r = SS.get(oracle, "ragged-alleles", "wide4")
    _run(rsb, r, SS.PARAMS["ragged-alleles"][:1], tuple(how.items()), **how)


@pytest.mark.parametrize("dealing,devices", [("wide4", (0, 1, 1, 0)), ("rr8", (0, 1) * 4)], ids=["wide4", "rr8"])
def test_gpu_site_sets_two_device_groups(rsb, oracle, monkeypatch, dealing, devices):
    """two device groups (two logical devices on GPU 0 where the box has one).  The dealing over four as (0, 1, 1, 0): each
    group has one shard with wide reads and one without, and extracts wide reads of its own; the answers and counters are
    the one-group ones (the restatement's, and gt_count's on the same set)"""
    _two_groups(rsb, monkeypatch)
    r = SS.get(oracle, "ragged-alleles", dealing)
    gs = _open(rsb, r, devices=devices)
    ss = rsb.ShardSet(gs)
    try:
        assert rsb.lib().rsbwt_set_devices(ss._s) == 2
        _build(ss, r.pairs)
        for M, k, skip in SS.PARAMS["ragged-alleles"][:2]:
            _check(ss, rsb, r, M, k, skip, ("two groups", dealing, M, k, skip))
    finally:
        _close(ss, gs)


@pytest.mark.parametrize("ss,other", [(1, False), (8, True)])
def test_gpu_site_sets_record_shapes(rsb, oracle, ss, other):
    r = SS.get(oracle, "ragged-alleles", "wide4", ss, other)
    _run(rsb, r, SS.PARAMS["ragged-alleles"][:1], (ss, other))


@pytest.mark.parametrize("dealing,params", REPEAT, ids=_ids(REPEAT))
def test_gpu_site_sets_repeat(rsb, oracle, dealing, params):
    """tandem repeats: one (request, read) entry reached through dozens of rows, head and non-head copies side by side"""
    r = SS.get(oracle, "repeat", dealing)
    got, = _run(rsb, r, [params], dealing)
    assert got["carriers"].sum() > 0 and got["work"]["kept"] > got["work"]["head_rows"]


def test_gpu_site_sets_repeat_tight_set_and_repeatability(rsb, oracle, monkeypatch):
    """the set loaded to the brim (RSBWT_SAMPLE_TIGHT_SET=1: long probe chains under many rows per entry) gives the same
    answers, and two calls agree byte for byte"""
    r = SS.get(oracle, "repeat", "halves")
    gs = _open(rsb, r)
    ss = rsb.ShardSet(gs)
    try:
        _build(ss, r.pairs)
        M, k, skip = SS.PARAMS["repeat"][0]
        for tight in ("1", "0"):
            monkeypatch.setenv("RSBWT_SAMPLE_TIGHT_SET", tight)
            _check(ss, rsb, r, M, k, skip, ("tight", tight))
            a, b = _got(ss, rsb, r, M, k, skip), _got(ss, rsb, r, M, k, skip)
            assert all(a[x].tobytes() == b[x].tobytes() for x in OUT) and a["work"] == b["work"]
    finally:
        _close(ss, gs)


def _with_and_without(rsb, oracle, reqs, params):
    a, b = SS.get(oracle, "exact4096", "with"), SS.get(oracle, "exact4096", "without")
    out = []
    for r in (a, b):
        gs = _open(rsb, r)
        ss = rsb.ShardSet(gs)
        try:
            _build(ss, r.pairs)
            out.append(_check(ss, rsb, r, *params, ("4096", r.name), reqs=reqs))
        finally:
            _close(ss, gs)
    assert tuple(out[0]["work"]) == KEYS
    return out


@pytest.mark.parametrize("params", SS.PARAMS["exact4096"], ids=lambda p: f"M{p[0]}-k{p[1]}-skip{p[2]}")
def test_gpu_site_sets_accept_a_read_of_4096_symbols(rsb, oracle, params):
    """a read of exactly 4,096 symbols is extracted at the wide stride, ordered with a key of 4,096 and aligned: the call
    succeeds, the read is a candidate of both windows of 79 it contains (hanging out of them, it is no carrier there),
    `extracted` counts it, and the other reads' answers are those of the set opened without it"""
    got, less = _with_and_without(rsb, oracle, SS.exact4096().reqs[:2], params)
    assert (got["aligned"] == less["aligned"] + 1).all() and (got["carriers"] == less["carriers"]).all()
    assert got["work"]["extracted"] == less["work"]["extracted"] + 1
    assert all((got[x] == less[x]).all() for x in ("strings", "copies"))


def test_gpu_site_sets_a_read_of_4096_symbols_is_a_carrier(rsb, oracle):
    """... and of the request whose window is its own 4,096 symbols it is a carrier, tallied with its value's records
    (one alignment of 4,096 rows by 4,096 columns: the slowest case of the file)"""
    ex = SS.exact4096()
    got, less = _with_and_without(rsb, oracle, ex.reqs[2:], SS.PARAMS["exact4096"][0])
    assert list(got["aligned"] - less["aligned"]) == [1] and list(got["carriers"] - less["carriers"]) == [1]
    assert got["work"]["extracted"] == less["work"]["extracted"] + 1
    value = dict(SS.get(oracle, "exact4096", "with").pairs)[ex.big]
    assert int(got["strings"][0].sum() - less["strings"][0].sum()) == len(value) // 4
