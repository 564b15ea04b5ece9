"""GPU suite (-m gpu): the index builder (readserver_amd/csrc/build_lines.hip) and the two kernels that finish an index
for read extraction (select_sample_kernel, psi_hint_kernel: csrc/kernels.hip) held to the host layout BYTE FOR BYTE.

tests/test_layout_host.py certifies the host layout at every position; rsbwt_layout_lines_host hands those lines and the
select sample table out (tests/layout_reference.py).  Equal bytes carry that certificate over to what the GPU built -- all
of it, not the lines some random k-mers happen to touch -- and a difference names the first wrong line.  What only the
device does is what the cases are chosen for: the tile / chunk totals and their scans, seek_reader's two binary searches,
the three-kernel scan of the far lines, the sampled choice of the span, and the two kernels above.  Each case is the
smallest shape at which its seam exists.

Every case runs in two forms: the plain layout (lines compared as opened, then again with the hints
rsbwt_prepare_extraction writes) and RSBWT_OPEN_READS (hints written at open); the sample table is compared in both.
No search runs here: the searches of the other GPU modules stay what they are."""
import ctypes as C
import time

import numpy as np
import pytest

import layout_reference as LR

pytestmark = pytest.mark.gpu

FORMS = pytest.mark.parametrize("for_reads", [False, True], ids=["plain", "reads"])


# ---- the run streams (plain numpy: the CPU suite's shapes, tests/test_layout_host.py) -------------------------------

def rand_runs(R, seed):
    """symbols 0..4, lengths 1..31"""
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 5, R).astype(np.uint8) << 5) | rng.integers(1, 32, R).astype(np.uint8)


def dense_runs(R, seed):
    """every run of length 1"""
    return (np.random.default_rng(seed).integers(1, 5, R).astype(np.uint8) << 5) | np.uint8(1)


def mixed_runs(R, seed, stretch=5000):
    """stretches of 5,000 run bytes, of 1-symbol and of 31-symbol runs in turn"""
    ln = np.where((np.arange(R) // stretch) % 2 == 0, 1, 31).astype(np.uint8)
    return (np.random.default_rng(seed).integers(0, 5, R).astype(np.uint8) << 5) | ln


ZERO_R = 250_000


def zero_length_runs():
    """"rand" with a quarter of the bytes of length 0 (their symbol kept), 300 such bytes at the very start and at the
    very end, and one stretch of them from run 65,436 to run 131,272: chunk 1 (runs 65,536 .. 131,071) holds no symbol at
    all, nor do the tiles on either side of it -- equal prefixes over whole tiles and a whole chunk"""
    rng = np.random.default_rng(250)
    runs = rand_runs(ZERO_R, 251)
    runs[rng.random(ZERO_R) < 0.25] &= 0xE0
    runs[:300] &= 0xE0
    runs[-300:] &= 0xE0
    runs[65_436:131_273] &= 0xE0
    runs[[65_435, 131_273]] |= 1  # (the stretch ends where it is said to)
    return runs


# ---- the comparison ------------------------------------------------------------------------------------------------

def _peek(L, g, region, nbytes):
    buf = np.empty(nbytes, np.uint8)
    rc = L.rsbwt_debug_peek(g.handle, region, 0, buf.ctypes.data, nbytes)
    assert rc == 0, (rc, L.rsbwt_last_error())
    return buf


def _same_lines(dev, host, what):
    """np.array_equal -- and, where they differ, the first line that does: its number, its group, its kind"""
    want = host["dwords"]
    assert dev.shape == want.shape, (what, dev.shape, want.shape)
    if np.array_equal(dev, want):
        return
    wrong = np.nonzero((dev != want).any(axis=1))[0]
    far_before = np.concatenate([[0], np.cumsum(host["group"][:, 0])]).astype(np.int64)
    kind, group = LR.line_kind(int(wrong[0]), host["groups"], far_before[:-1])
    cols = np.nonzero(dev[wrong[0]] != want[wrong[0]])[0]
    raise AssertionError(f"{what}: {len(wrong)} of {len(want)} lines differ from the host's; the first is line {wrong[0]}, a {kind} "
                         f"line of group {group} (of {host['groups']}), dwords {cols.tolist()}: device "
                         f"{[hex(x) for x in dev[wrong[0], cols]]}, host {[hex(x) for x in want[wrong[0], cols]]}")


def _same_table(L, g, host, what):
    sel = _peek(L, g, 2, host["sel_words"] * 8).view(np.uint64)
    if not np.array_equal(sel, host["sel"]):
        wrong = np.nonzero(sel != host["sel"])[0]
        stride = host["sel_words"] // 5
        raise AssertionError(f"{what}: {len(wrong)} of {sel.size} sample words differ; the first is sample {wrong[0] % stride} of "
                             f"symbol {wrong[0] // stride}: device {int(sel[wrong[0]]):#x}, host {int(host['sel'][wrong[0]]):#x}")
    # the table has exactly the size the host says: one byte more is outside it
    one = np.empty(1, np.uint8)
    assert L.rsbwt_debug_peek(g.handle, 2, host["sel_words"] * 8, one.ctypes.data, 1) == -7


def check_bytes(rsb, runs, span, for_reads, device_runs=None, times=None):
    """Opens `runs` (or the same bytes at device_runs = (pointer, R)) and holds everything the builder left to the host's;
    returns (the host layout with hints, the device's lines with hints)."""
    L = rsb.lib()
    R = runs.size
    lens, sym = (runs & 31).astype(np.int64), runs >> 5
    n = int(lens.sum())
    per_symbol = np.bincount(sym, weights=lens, minlength=5).astype(np.int64)
    what = f"R={R} span={span} {'reads' if for_reads else 'plain'}"
    src = dict(device_runs=device_runs) if device_runs is not None else dict(runs=runs)
    t0 = time.perf_counter()
    with rsb.GpuBWT(ktab_depth=None, window_span=span, for_reads=for_reads, **src) as g:
        t_open = time.perf_counter() - t0
        S = g.window_span()
        assert span == 0 or S == span
        # the totals: plain sums over the run bytes
        assert g.getBWLen() == n
        assert [g.getPC(b) for b in "$ACGT"] == np.concatenate([[0], np.cumsum(per_symbol)[:4]]).tolist()
        t0 = time.perf_counter()
        hinted = LR.host_layout(L, runs, S, for_reads, hints=True)
        t_host = time.perf_counter() - t0
        assert (g.num_lines(), g.far_lines(), g.spilled_symbols()) == (hinted["lines"], hinted["far_lines"], hinted["spilled_symbols"])
        assert hinted["lines"] == hinted["groups"] * 17 + int(hinted["group"][:, 0].sum())
        dev = _peek(L, g, 0, hinted["lines"] * 128).view(np.uint32).reshape(-1, 32)
        if not for_reads:
            # as opened: no hint anywhere, no sample table yet; then the owner's open-time step writes both
            _same_lines(dev, LR.host_layout(L, runs, S, False), what + ", as opened")
            one = np.empty(8, np.uint8)
            assert L.rsbwt_debug_peek(g.handle, 2, 0, one.ctypes.data, 8) == -7 and L.rsbwt_psi_hint_lines(g.handle) == 0
            assert L.rsbwt_prepare_extraction(g.handle) == 0, L.rsbwt_last_error()
            dev = _peek(L, g, 0, hinted["lines"] * 128).view(np.uint32).reshape(-1, 32)
        _same_lines(dev, hinted, what + ", with hints")
        assert L.rsbwt_psi_hint_lines(g.handle) == hinted["hint_lines"]
        _same_table(L, g, hinted, what)
    if times is not None:
        times.update(open_s=t_open, host_s=t_host)
    print(f"{what}: n={n} S={S} groups={hinted['groups']} lines={hinted['lines']} far={hinted['far_lines']} chunk_windows="
          f"{hinted['chunk_windows']} spilled={hinted['spilled_symbols']} hint_lines={hinted['hint_lines']} sel_words={hinted['sel_words']} "
          f"open {t_open * 1e3:.0f} ms, host layout {t_host * 1e3:.0f} ms")
    return hinted, dev


@pytest.fixture
def hooks(monkeypatch):
    monkeypatch.setenv("RSBWT_ENABLE_TEST_HOOKS", "1")  # rsbwt_debug_peek is refused without it


# ---- tile and chunk borders: R around 256 (a tile) and 65,536 (a chunk of 256 tiles) --------------------------------

@FORMS
@pytest.mark.parametrize("span", [0, 40])
@pytest.mark.parametrize("R", [1, 255, 256, 257, 65_535, 65_536, 65_537, 131_073])
def test_gpu_lines_at_tile_and_chunk_borders(rsb, hooks, R, span, for_reads):
    """the last tile / chunk full, one byte short, one byte over (a chunk of ONE run byte: R = 65,537, 131,073)"""
    check_bytes(rsb, rand_runs(R, R), span, for_reads)


# ---- a group's first symbol is the first of a tile / of a chunk; more than 1,024 groups without far lines -----------

@FORMS
@pytest.mark.parametrize("R,span,groups", [(300_000, 2, 9_375), (131_072, 16, 512)])
def test_gpu_lines_where_groups_start_on_tile_and_chunk_borders(rsb, hooks, R, span, groups, for_reads):
    """every run of length 1: symbol p is run byte p.  Span 2: a group is 32 run bytes, every 8th group starts a tile,
    every 2,048th a chunk (seek_reader's searches end ON the border: symbols-before == P), and the 9,375 groups are ten
    blocks of the far-line scan whose sums are all zero.  Span 16: a group is one tile, group 256 begins at run 65,536,
    the first of chunk 1."""
    hinted, _ = check_bytes(rsb, dense_runs(R, R + span), span, for_reads)
    assert hinted["groups"] == groups and hinted["far_lines"] == 0


# ---- the far-line scan across its 1,024-group blocks ----------------------------------------------------------------

FAR_R, FAR_SPAN = 1_000_000, 768


def far_case_groups(L, room):
    return LR.host_layout(L, mixed_runs(FAR_R, 768), FAR_SPAN, room, lines=False)


@FORMS
def test_gpu_far_lines_across_scan_blocks(rsb, hooks, for_reads):
    """scan_sums / scan_top / scan_final: group 1,024 and later take their far lines after ALL of block 0's (sums[1]).  The
    dense stretches of "mixed" need chains of far lines at span 768, the 31-symbol stretches none: groups on both sides
    of the border need some, and groups on both sides need none -- a block offset that is wrong cannot cancel."""
    L = rsb.lib()
    far = far_case_groups(L, for_reads)["group"][:, 0]
    assert len(far) > 1024 + 64
    assert (far[:1024] > 0).sum() >= 32 and (far[1024:] > 0).sum() >= 8, "far lines on both sides of the block border"
    assert (far[:1024] == 0).sum() >= 32 and (far[1024:] == 0).sum() >= 8, "and groups without any on both sides"
    assert far[:1024].sum() > 0 and far[1024:].max() > 1  # (sums[1] != 0; chains, not single far lines)
    check_bytes(rsb, mixed_runs(FAR_R, 768), FAR_SPAN, for_reads)


# ---- zero-length run bytes ----------------------------------------------------------------------------------------

@FORMS
@pytest.mark.parametrize("span", [0, 300])
def test_gpu_lines_over_zero_length_run_bytes(rsb, hooks, span, for_reads):
    """run_reader::take skips them; whole tiles and a whole chunk of them give seek_reader equal prefixes to choose among"""
    runs = zero_length_runs()
    assert ((runs[65_536:131_072] & 31) == 0).all() and (runs & 31)[131_273] != 0 and (runs & 31)[65_435] != 0 and (runs >> 5).max() == 4
    assert 0.2 < ((runs & 31) == 0).mean() < 0.5
    check_bytes(rsb, runs, span, for_reads)


def test_gpu_zero_length_byte_with_a_symbol_above_four_is_refused(rsb, hooks):
    """RSBWT_EFORMAT from the device open (tile_totals_kernel looks at the code whatever the length) and from the host hook"""
    from readserver_amd import RsbwtError
    L = rsb.lib()
    runs = rand_runs(70_000, 6)
    runs[66_000] = 6 << 5
    assert LR.host_layout(L, runs, 0, False, rc_only=True) == -3
    with pytest.raises(RsbwtError) as e:
        rsb.GpuBWT(runs=runs, ktab_depth=None)
    assert e.value.code == -3
    runs[66_000] = 4 << 5  # (the same stream with a code the alphabet has: opens, and its bytes are the host's)
    check_bytes(rsb, runs, 0, False)


# ---- run bytes that do not start on a 16-byte border ----------------------------------------------------------------

@FORMS
def test_gpu_lines_from_unaligned_run_bytes(rsb, hooks, for_reads):
    """tile_totals_kernel reads 16 bytes at a time only from a 16-byte aligned pointer; rsbwt_open_device_runs asks for no
    alignment (include/rsbwt.h), so any other pointer takes its byte path: the same lines as the host's, and as the
    aligned open's"""
    import torch
    L = rsb.lib()
    R = 100_001
    runs = np.empty(R, np.uint8)
    assert L.rsbwt_synth_runs_host(runs.ctypes.data, R, 555) == 0
    _, aligned = check_bytes(rsb, runs, 0, for_reads)
    for off in (1, 3, 8, 15, 16):
        d = torch.zeros(R + 32, dtype=torch.uint8, device="cuda:0")
        assert d.data_ptr() % 16 == 0
        d[off:off + R].copy_(torch.from_numpy(runs))
        torch.cuda.synchronize()
        _, got = check_bytes(rsb, runs, 0, for_reads, device_runs=(d.data_ptr() + off, R))
        assert np.array_equal(got, aligned), off


# ---- more than 1,024 chunks: scan_chunks_kernel with two chunks per thread; the sampled span loop --------------------

BIG_R = 67_108_864 + 70_000


@FORMS
def test_gpu_lines_over_more_than_1024_chunks(rsb, hooks, for_reads):
    """1,026 chunks of 65,536 run bytes (the last one of 70,000 - 65,536 bytes): every thread of scan_chunks_kernel scans
    two, and 47,000 groups send the choice of the span through its sample loop.  The GPU builds this in tens of
    milliseconds; the host lays 67 MB of run bytes out and 104 MB (114 MB for reads) of lines are compared.  Measured:
    one host layout 1.5 s (1.9 s for reads, hints included; the plain form needs two), a comparison 0.03 s."""
    import torch
    L = rsb.lib()
    d = torch.empty(BIG_R, dtype=torch.uint8, device="cuda:0")
    assert L.rsbwt_synth_runs_dev(C.c_void_p(d.data_ptr()), BIG_R, 555, 0, None) == 0
    torch.cuda.synchronize()
    runs = d.cpu().numpy()
    assert (BIG_R + 65_535) // 65_536 > 1024
    hinted, _ = check_bytes(rsb, runs, 0, for_reads, device_runs=(d.data_ptr(), BIG_R))
    assert hinted["groups"] >= 4096  # (the sample loop ran)


# ---- the rule the builder settles on a span by ------------------------------------------------------------------------

RULE_R = 6_500_000


def rule_case(L, runs, room):
    """(stats6 at the span chosen, trace) by the restated rule over the host hook's per-group numbers"""
    n = int((runs & 31).astype(np.int64).sum())

    def stats_at(S):
        h = LR.host_layout(L, runs, S, room, lines=False)
        return [h[k] for k in LR.STATS[:6]], h["group"]
    return LR.choose_span(n, runs.size, room, stats_at)


@FORMS
@pytest.mark.parametrize("stretch", [5000, 3000])
def test_gpu_span_is_the_restated_rules(rsb, hooks, stretch, for_reads):
    """"mixed" at 6,500,000 run bytes: 4,600 groups at the starting span, and no single span suits stretches of 1- and of
    31-symbol runs.  The span the device ends on is the one the rule, restated in Python (tests/layout_reference.py) over
    the host's per-group numbers, ends on; and the bytes at it are the host's.

    The sample loop (groups 0, 64, 128, ... through count_groups_kernel with every = 64) rejects spans -- all 16 it may
    try on the layout for reads, and all 4 on the plain layout where the stretches are 3,000 run bytes.  On the plain
    layout with stretches of 5,000 the sample is blind: 64 groups of the starting span, 1,408, are 9.01 periods of the
    stream, every sampled group lies in a stretch of 31-symbol runs, the sample PASSES the span and the full pass, which
    sees 3.1 % of the positions spill, rejects it -- the other way through the rule, asserted as such."""
    L = rsb.lib()
    runs = mixed_runs(RULE_R, 65, stretch)
    st, trace = rule_case(L, runs, for_reads)
    print("spans tried:", trace)
    sampled = [ok for kind, _, ok in trace if kind == "sample"]
    full = [ok for kind, _, ok in trace if kind == "full"]
    if stretch == 5000 and not for_reads:
        assert sampled == [True] and full[0] is False and len(full) > 1, "the sample lets a span through that the full pass rejects"
    else:
        assert sampled.count(False) >= 1, "the sample loop rejects at least one span"
    assert len(sampled) >= 1 and len(full) >= 1
    hinted, _ = check_bytes(rsb, runs, 0, for_reads)
    assert hinted["S"] == st[0] and [hinted[k] for k in LR.STATS[:6]] == st
