"""Sample walks on the GPU (-m gpu): rsbwt_set_extension_samples / rsbwt_set_walk_samples / _dev (csrc/sample_walk.hip,
csrc/set_graph.hip) held bit-exactly to tests/sample_walk_reference.py, the definition restated over
sample_reference.counts_plain -- no BWT.  tests/test_sample_walk_reference.py holds that restatement to the one over the
oracle on the CPU and shows that the inputs reach what the kernels can get wrong."""
import ctypes as C

import numpy as np
import pytest

import sample_reference as SR
import sample_walk_reference as SW
import walk_reference as WR

pytestmark = pytest.mark.gpu

SPANS = {"control": 40, "chunk": 128, "far": 300, "chain": 600, "deep": 2944}
MASKS = {"a1": [SW.A1], "b1": [SW.B1], "a1+b1": [SW.A1, SW.B1], "none": []}
WORK = ("seeds", "appended", "searches", "search_steps", "rows", "head_rows", "carriers", "records", "lf_steps", "wide")


def _open(rsb, shards, runs, span=0, ktab=6, devices=None, grouped=False):
    devices = devices or [0] * len(shards)
    return [rsb.GpuBWT(runs=r, num_strings=len(sh), ktab_depth=ktab, window_span=span, device=d, ktab_grouped=grouped)
            for d, sh, r in zip(devices, shards, runs)]


def _close(ss, gs):
    ss.close()
    for g in gs:
        g.close()


def _build(ss, pairs):
    return ss.meta_build([w for w, _ in pairs], [v for _, v in pairs])


def _as_walks(got):
    """ShardSet.walk_samples(..., supports=True) -> what the reference's Walk holds of it"""
    return [(e, s, sup, last) for e, s, last, sup in got]


def _ref_walks(ws):
    return [(w.ext, w.stop, w.support, w.last) for w in ws]


# ---- the fixture that shows the feature ------------------------------------------------------------------------------

@pytest.mark.parametrize("S", [1, 2, 3, 4, 8])
def test_gpu_walk_samples_follows_one_haplotype(rsb, S):
    """the plain walk stops BRANCH at the SNP (the control); mask {a1} walks through the SNP and the deletion along A, {b1}
    along B, {a1, b1} branches where the plain walk does, the empty mask dead-ends at 0 steps -- all as the reference says,
    supports and last included; S = 1 .. 8 are walk_kernel's wave counts, and at S = 1 the reads both haplotypes spell are
    duplicate strings of one shard (non-head copies)"""
    fx = SW.haplotype_fixture()
    shards = SW.dealt(fx.reads, S)
    gs = _open(rsb, shards, SW.runs(fx.reads, S))
    ss = rsb.ShardSet(gs)
    try:
        _build(ss, fx.pairs)
        seed = fx.a[10:40]
        (ext, stop, _), = ss.walk([seed], 20, max_steps=200)
        assert stop == rsb.bwt.WALK_BRANCH and seed + ext == fx.a[10:fx.snp]
        for name, mask in MASKS.items():
            side = SW.plain_side(shards, fx.pairs, fx.codes, 2, True, mask)
            seeds = [seed, fx.b[60:85], fx.a[5:24], fx.a[:19] + "N" + fx.a[20:45]]
            want = [SW.walk(side, s, 20, 1, 200, False, False, 4096) for s in seeds]
            got = ss.walk_samples(seeds, 20, fx.codes, 2, mask_codes=mask, max_steps=200, supports=True)
            assert _as_walks(got) == _ref_walks(want), (S, name)
        a, = ss.walk_samples([seed], 20, fx.codes, 2, mask_codes=[SW.A1], max_steps=200)
        b, = ss.walk_samples([seed], 20, fx.codes, 2, mask_codes=[SW.B1], max_steps=200)
        assert (seed + a[0]).startswith(fx.a[10:fx.indel + 30]) and (seed + b[0]).startswith(fx.b[10:fx.indel + 30])
        both, = ss.walk_samples([seed], 20, fx.codes, 2, mask_codes=[SW.A1, SW.B1], max_steps=200)
        assert both[1] == rsb.bwt.WALK_BRANCH and both[0] == ext
        none, = ss.walk_samples([seed], 20, fx.codes, 2, mask_codes=[], max_steps=200)
        assert none == ("", rsb.bwt.WALK_DEAD_END, (0, 0, 0, 0))
    finally:
        _close(ss, gs)


def test_gpu_walk_samples_is_the_host_loop_of_sample_counts(rsb):
    """the composition: ShardSet.sample_counts on the candidates of every seed, the masked columns added, the rule -- the
    loop walk_samples takes off the host -- gives walk_samples' answers on the haplotype fixture, left and both strands"""
    fx = SW.haplotype_fixture()
    shards = SW.dealt(fx.reads, 2)
    gs = _open(rsb, shards, SW.runs(fx.reads, 2))
    ss = rsb.ShardSet(gs)
    try:
        _build(ss, fx.pairs)
        for mask in ([SW.A1], [SW.B1, SW.A2]):
            for left, both, copies in ((False, False, False), (True, True, True)):
                side = SW.Side(lambda x: ss.sample_counts([x], fx.codes, 2, True), fx.codes, mask, copies)
                seeds = [fx.a[10:40], fx.b[100:130], fx.a[150:190]]
                want = [SW.walk(side, s, 20, 1, 60, left, both, 4096) for s in seeds]
                got = ss.walk_samples(seeds, 20, fx.codes, 2, mask_codes=mask, max_steps=60, left=left, both_strands=both, copies=copies, supports=True)
                assert _as_walks(got) == _ref_walks(want), (mask, left, both, copies)
    finally:
        _close(ss, gs)


def test_gpu_extension_samples_palindromes_and_repeated_offsets(rsb):
    """ctx 3 on the haplotype reads: a candidate of four symbols lies at several offsets of one read (the rows are many, the
    carriers few: de-duplication) and ACGT, GCGC, AATT are their own reverse complements (counted twice with both strands)"""
    fx = SW.haplotype_fixture()
    shards = SW.dealt(fx.reads, 3)
    gs = _open(rsb, shards, SW.runs(fx.reads, 3), ktab=None)
    ss = rsb.ShardSet(gs)
    try:
        _build(ss, fx.pairs)
        seeds = ["ACG", "GCG", "AAT", "TTT", "CAN", "AC", fx.a[:3]]
        for mask in ([SW.A1], [SW.B1], [SW.A1, SW.A2, SW.B1]):
            for left, both, copies in ((False, True, False), (True, True, True), (False, False, False)):
                side = SW.plain_side(shards, fx.pairs, fx.codes, 2, True, mask, copies)
                want = [SW.evaluate(side, s, 3, left, both, 1 << 20) for s in seeds]
                got = ss.extension_samples(seeds, 3, fx.codes, 2, mask_codes=mask, max_rows=1 << 20, left=left, both_strands=both, copies=copies)
                assert [tuple(int(x) for x in r) for r in got["msup"]] == [w[0] for w in want], (mask, left, both, copies)
                assert [bool(x) for x in got["wide"]] == [w[1] for w in want]
                assert [tuple(int(x) for x in r) for r in got["matches"]] == [w[2] for w in want]
        wk = rsb.ShardSet.walk_samples_last_work()
        # the last call's work is sample counts' over its candidates: rows, rows on a head ordinal, distinct carriers, records
        cands = [x for s in seeds if WR.context(s, 3, False) for x in WR.candidates(WR.context(s, 3, False), False)]
        sc = SR.counts_plain(shards, fx.pairs, cands, fx.codes, 2, True)["work"]
        assert tuple(wk) == WORK and wk["seeds"] == len(seeds) and wk["searches"] == len(cands) * 3
        assert (wk["rows"], wk["head_rows"], wk["carriers"], wk["records"], wk["lf_steps"]) == tuple(sc[k] for k in ("rows", "head_rows", "carriers", "records", "lf_steps"))
        assert wk["rows"] >= wk["head_rows"] > wk["carriers"] > 0  # (a read holding a candidate at two offsets is one carrier)
        pal = ss.extension_samples(["ACG"], 3, fx.codes, 2, mask_codes=[SW.A1], max_rows=1 << 20, both_strands=True)
        one = ss.extension_samples(["ACG"], 3, fx.codes, 2, mask_codes=[SW.A1], max_rows=1 << 20)
        assert int(pal["msup"][0][3]) == 2 * int(one["msup"][0][3]) > 0 and int(pal["matches"][0][3]) == 2 * int(one["matches"][0][3])
    finally:
        _close(ss, gs)


# ---- shapes at which the kernels can go wrong: the gt reads under sample_pairs' values -----------------------------

def _gt_open(rsb, c, **kw):
    gs = _open(rsb, c.shards, WR.runs("stranded", c.S), **kw)
    ss = rsb.ShardSet(gs)
    _build(ss, c.pairs)
    return ss, gs


def _gt_check(ss, c, where, copies=False, left=False, both=False, max_rows=4096, min_count=1, max_steps=None, seeds=None):
    want = SW.gt_walks(c, "plain", copies, left, both, max_rows, min_count, max_steps, seeds)
    got = ss.walk_samples(c.seeds if seeds is None else seeds, c.ctx, c.codes, c.ss, mask_codes=c.mask, has_other_meta_data=c.other,
                          min_count=min_count, max_steps=c.max_steps if max_steps is None else max_steps, max_rows=max_rows, left=left,
                          both_strands=both, copies=copies, supports=True)
    assert _as_walks(got) == _ref_walks(want), where
    return got


@pytest.mark.parametrize("S", [1, 2, 3, 4, 8])
def test_gpu_walk_samples_on_the_gt_reads(rsb, S):
    """record counts 0, 15, 16, 17, 300 and 2,000, stray tails, a code listed twice, negative c with copies, unknown codes,
    reads left out of the pairs; right and left, one and both strands; min_count 1, 2 and one above the largest support;
    max_steps 1; Q = 12 (a workgroup and a half)"""
    c = SW.gt_case(S=S)
    ss, gs = _gt_open(rsb, c)
    try:
        for copies in (False, True):
            for left, both in ((False, True), (True, False)):
                got = _gt_check(ss, c, (S, copies, left, both), copies=copies, left=left, both=both)
        top = max([x for w in got for x in w[2] + w[3]] + [1])  # (the last configuration's: copies, left, one strand)
        _gt_check(ss, c, "min_count 2", both=True, min_count=2)
        dead = _gt_check(ss, c, "min_count above every support", copies=True, left=True, min_count=top + 1)
        assert all(w[1] in (WR.DEAD_END, WR.INVALID) and w[0] == "" for w in dead)
        one = _gt_check(ss, c, "max_steps 1", both=True, max_steps=1)
        assert any(w[1] == WR.LIMIT for w in one)
    finally:
        _close(ss, gs)


@pytest.mark.parametrize("Q", [1, 7, 8, 9])
def test_gpu_walk_samples_batch_sizes_and_repeatability(rsb, Q):
    c = SW.gt_case()
    ss, gs = _gt_open(rsb, c, span=SPANS["chunk"])
    try:
        seeds = (c.seeds[:7] + c.seeds[-2:])[:Q]
        a = _gt_check(ss, c, Q, both=True, seeds=seeds)
        b = _gt_check(ss, c, Q, both=True, seeds=seeds)
        assert a == b  # the same call twice
        assert rsb.ShardSet.walk_samples_last_work()["seeds"] == Q
    finally:
        _close(ss, gs)


def test_gpu_walk_samples_stops_wide_at_the_boundary(rsb):
    """max_rows equal to the widest candidate of the first evaluation walks on as with no limit to speak of; one less stops
    WIDE at 0 steps with last = zeros; the primitive reports the rows either way; seeds inside the tandem repeat stop WIDE"""
    c = SW.gt_case()
    ss, gs = _gt_open(rsb, c)
    try:
        side = c.side("plain", False)
        seed = c.seeds[0]
        per = [side.matches(x) for x in WR.candidates(WR.context(seed, c.ctx, False), False)]
        assert max(per) >= 2
        at = _gt_check(ss, c, "at the limit", max_rows=max(per), seeds=[seed])
        below = _gt_check(ss, c, "one below", max_rows=max(per) - 1, seeds=[seed])
        assert below == [("", SW.WIDE, (0, 0, 0, 0), ())] and at[0][1] != SW.WIDE
        for limit in (max(per), max(per) - 1):
            got = ss.extension_samples([seed], c.ctx, c.codes, c.ss, mask_codes=c.mask, max_rows=limit)
            want = SW.evaluate(side, seed, c.ctx, False, False, limit)
            assert (tuple(int(x) for x in got["msup"][0]), bool(got["wide"][0]), tuple(int(x) for x in got["matches"][0])) == want
            assert tuple(int(x) for x in got["matches"][0]) == tuple(per)
        inside = [c.all_seeds[i] for i in WR.seeds_inside_the_repeat()[:3]]
        ws = _gt_check(ss, c, "inside the repeat", max_rows=3, max_steps=8, seeds=inside)
        assert all(w[1] == SW.WIDE for w in ws)
        assert rsb.ShardSet.walk_samples_last_work()["wide"] == len(inside)
    finally:
        _close(ss, gs)


@pytest.mark.parametrize("ss_,other", [(1, True), (1, False), (4, True), (4, False), (8, True), (8, False)])
def test_gpu_walk_samples_record_shapes(rsb, ss_, other):
    c = SW.gt_case(S=2, size_of_sample=ss_, has_other=other)
    ss, gs = _gt_open(rsb, c)
    try:
        _gt_check(ss, c, (ss_, other, "strings"), both=True)
        _gt_check(ss, c, (ss_, other, "copies"), copies=True, left=True)
    finally:
        _close(ss, gs)


@pytest.mark.parametrize("kind", list(SPANS))
@pytest.mark.parametrize("ktab", [6, None])
def test_gpu_walk_samples_on_every_line_layout(rsb, kind, ktab):
    c = SW.gt_case()
    ss, gs = _gt_open(rsb, c, span=SPANS[kind], ktab=ktab)
    try:
        assert all(g.window_span() == SPANS[kind] for g in gs)
        _gt_check(ss, c, (kind, ktab), both=True, copies=True)
    finally:
        _close(ss, gs)


@pytest.mark.parametrize("ktab,grouped", [(6, True), (10, False), (10, True)])
def test_gpu_walk_samples_table_formats_and_depths(rsb, ktab, grouped):
    c = SW.gt_case()
    ss, gs = _gt_open(rsb, c, span=SPANS["far"], ktab=ktab, grouped=grouped)
    try:
        assert all(g.ktab_depth() == ktab and g.ktab_info()[0] == (1 if grouped else 0) for g in gs)
        _gt_check(ss, c, (ktab, grouped), left=True, both=True)
    finally:
        _close(ss, gs)


def test_gpu_walk_samples_on_two_logical_devices(rsb, monkeypatch):
    """a set over two device groups walks with the one-step primitive, one round trip per step: the same outputs; WIDE is
    decided over both groups' rows"""
    L = rsb.lib()
    if L.rsbwt_device_count() < 2:
        monkeypatch.setenv("RSBWT_ENABLE_TEST_HOOKS", "1")
        monkeypatch.setenv("RSBWT_TEST_DEVICE_ALIASES", "2")
    c = SW.gt_case(S=3)
    ss, gs = _gt_open(rsb, c, span=SPANS["far"], devices=(0, 1, 0))
    try:
        assert L.rsbwt_set_devices(ss._s) == 2
        _gt_check(ss, c, "two devices", both=True)
        _gt_check(ss, c, "two devices, copies, left", copies=True, left=True, min_count=2)
        side = c.side("plain", False)
        seed = c.seeds[0]
        per = [side.matches(x) for x in WR.candidates(WR.context(seed, c.ctx, False), False)]
        _gt_check(ss, c, "two devices, at the limit", max_rows=max(per), seeds=[seed])
        assert _gt_check(ss, c, "two devices, below", max_rows=max(per) - 1, seeds=[seed])[0][1] == SW.WIDE
        got = ss.extension_samples(c.seeds, c.ctx, c.codes, c.ss, mask_codes=c.mask, both_strands=True)
        want = [SW.evaluate(c.side("plain", False), s, c.ctx, False, True, 4096) for s in c.seeds]
        assert [tuple(int(x) for x in r) for r in got["msup"]] == [w[0] for w in want]
        assert [tuple(int(x) for x in r) for r in got["matches"]] == [w[2] for w in want]
        # support and last null: ext, steps and stop of the call that has them
        pv = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        flat, n, mask = rsb.ShardSet._sample_mask(c.codes, c.ss, c.mask)
        text, off = rsb.ShardSet._var_text(c.seeds)
        Q, mx = len(c.seeds), c.max_steps
        full = [np.full((Q, mx), 77, np.uint8), np.full(Q, 77, np.uint32), np.full(Q, 77, np.uint8)]
        bare = [a.copy() for a in full]
        sup, last = np.zeros((Q, mx), np.uint32), np.zeros((Q, 4), np.uint64)
        args = (ss._s, pv(text), pv(off), Q, 12, 1, mx, 0, pv(flat), n, c.ss, 1 if c.other else 0, pv(mask), 4096, 0)
        assert L.rsbwt_set_walk_samples(*args, *[pv(a) for a in full], pv(sup), pv(last)) == 0, L.rsbwt_last_error()
        assert L.rsbwt_set_walk_samples(*args, *[pv(a) for a in bare], None, None) == 0, L.rsbwt_last_error()
        assert all((a == b).all() for a, b in zip(full, bare)) and full[1].any() and (sup != 0).sum() == full[1].sum()
    finally:
        _close(ss, gs)


def test_gpu_walk_samples_device_resident_form(rsb):
    """rsbwt_set_walk_samples_dev inside 0xAA guard bytes, the buffers pre-filled with 0xAA: every byte of every output is
    the host form's, the status block is the host form's work"""
    import torch
    L = rsb.lib()
    c = SW.gt_case()
    ss, gs = _gt_open(rsb, c, span=SPANS["far"])
    p = lambda t, byte=0: C.c_void_p(t.data_ptr() + byte)  # noqa: E731
    pv = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    try:
        flat, n, mask = rsb.ShardSet._sample_mask(c.codes, c.ss, c.mask)
        keys = np.zeros(n, np.uint64)
        assert L.rsbwt_sample_keys(pv(flat), n, c.ss, pv(keys)) == 0
        text, off = rsb.ShardSet._var_text(c.seeds)
        Q, N, PAD, steps = len(c.seeds), int(off[-1]), 256, c.max_steps
        d_text, d_off = torch.from_numpy(text).cuda(), torch.from_numpy(off.view(np.int64)).cuda()
        d_keys, d_mask = torch.from_numpy(keys.view(np.int64)).cuda(), torch.from_numpy(mask[:n].copy()).cuda()
        sizes = dict(ext=Q * steps, steps=Q * 4, stop=Q, support=Q * steps * 4, last=Q * 32, status=64)
        for flags in (2, 1 | 4):
            h_ext, h_steps, h_stop = np.zeros((Q, steps), np.uint8), np.zeros(Q, np.uint32), np.zeros(Q, np.uint8)
            h_sup, h_last = np.zeros((Q, steps), np.uint32), np.zeros((Q, 4), np.uint64)
            assert L.rsbwt_set_walk_samples(ss._s, pv(text), pv(off), Q, c.ctx, 1, steps, flags, pv(flat), n, c.ss, 1, pv(mask), 4096, 0, pv(h_ext),
                                            pv(h_steps), pv(h_stop), pv(h_sup), pv(h_last)) == 0, L.rsbwt_last_error()
            wk = rsb.ShardSet.walk_samples_last_work()
            d = {k: torch.full((PAD + b + PAD,), 0xAA, dtype=torch.uint8, device="cuda") for k, b in sizes.items()}
            rc = L.rsbwt_set_walk_samples_dev(ss._s, p(d_text), p(d_off), Q, N, c.ctx, 1, steps, flags, p(d_keys), n, c.ss, 1, p(d_mask), 4096, 0,
                                              p(d["ext"], PAD), p(d["steps"], PAD), p(d["stop"], PAD), p(d["support"], PAD), p(d["last"], PAD),
                                              p(d["status"], PAD), None)
            assert rc == 0, L.rsbwt_last_error()
            torch.cuda.synchronize()
            h = {k: t.cpu().numpy() for k, t in d.items()}
            for k, b in sizes.items():
                assert (h[k][:PAD] == 0xAA).all() and (h[k][PAD + b:] == 0xAA).all(), (flags, k)
            body = lambda k: h[k][PAD:PAD + sizes[k]].tobytes()  # noqa: E731
            assert body("ext") == h_ext.tobytes() and body("steps") == h_steps.tobytes() and body("stop") == h_stop.tobytes(), flags
            assert body("support") == h_sup.tobytes() and body("last") == h_last.tobytes(), flags
            status = np.frombuffer(body("status"), np.uint64).tolist()
            assert status == [wk["rows"], wk["head_rows"], wk["carriers"], wk["records"], wk["appended"], wk["lf_steps"], 0, wk["wide"]], (status, wk)
            assert wk["appended"] == int(h_steps.sum()) and wk["rows"] > 0 and wk["lf_steps"] > 0
        # Q = 0: the status zeroed and nothing else; null arguments; a set on two devices is refused by the host checks below
        d_st = torch.full((128,), 0xAA, dtype=torch.uint8, device="cuda")
        assert L.rsbwt_set_walk_samples_dev(ss._s, None, None, 0, 0, c.ctx, 1, steps, 0, p(d_keys), n, c.ss, 1, p(d_mask), 4096, 0, None, None, None, None,
                                            None, p(d_st, 64), None) == 0
        torch.cuda.synchronize()
        hs = d_st.cpu().numpy()
        assert (hs[:64] == 0xAA).all() and not hs[64:].any()
        args = (p(d_text), p(d_off), Q, N, c.ctx, 1, steps, 0)
        out = (p(d["ext"], PAD), p(d["steps"], PAD), p(d["stop"], PAD), None, None)
        assert L.rsbwt_set_walk_samples_dev(ss._s, *args, None, n, c.ss, 1, p(d_mask), 4096, 0, *out, p(d_st), None) == -1
        assert L.rsbwt_set_walk_samples_dev(ss._s, *args, p(d_keys), n, c.ss, 1, None, 4096, 0, *out, p(d_st), None) == -1
        assert L.rsbwt_set_walk_samples_dev(ss._s, *args, p(d_keys), n, c.ss, 1, p(d_mask), 4096, 0, *out, None, None) == -1
        assert L.rsbwt_set_walk_samples_dev(ss._s, *args, p(d_keys), n, c.ss, 1, p(d_mask), 0, 0, *out, p(d_st), None) == -1
        assert L.rsbwt_set_walk_samples_dev(ss._s, *args, p(d_keys), n, c.ss, 1, p(d_mask), 4096, 0, None, out[1], out[2], None, None, p(d_st), None) == -1
    finally:
        _close(ss, gs)


def test_gpu_walk_samples_refuses_what_the_definition_refuses(rsb):
    L = rsb.lib()
    c = SW.gt_case()
    gs = _open(rsb, c.shards, WR.runs("stranded", c.S))
    ss = rsb.ShardSet(gs)
    pv = lambda x: x.ctypes.data_as(C.c_void_p) if x is not None else None  # noqa: E731
    try:
        text, off = rsb.ShardSet._var_text(c.seeds[:2])
        good, mask = np.frombuffer(b"ab" b"ac" b"\xff\x00", np.uint8).copy(), np.array([1, 0, 1], np.uint8)
        MARK = 0x7A
        ext, steps, stop = np.full((2, 4), MARK, np.uint8), np.full(2, MARK, np.uint32), np.full(2, MARK, np.uint8)
        msup, wide = np.full((2, 4), MARK, np.uint64), np.full(2, MARK, np.uint8)

        def walk(codes=good, n=3, size=2, mk=mask, max_rows=16, ctx=20, max_steps=4, flags=0, e=ext, st=steps, sp=stop, t=text, o=off):
            return L.rsbwt_set_walk_samples(ss._s, pv(t), pv(o), 2, ctx, 1, max_steps, flags, pv(codes), n, size, 1, pv(mk), max_rows, 0, pv(e), pv(st),
                                            pv(sp), None, None)

        def evaluate(codes=good, n=3, size=2, mk=mask, max_rows=16, ctx=20, flags=0, ms=msup, wd=wide):
            return L.rsbwt_set_extension_samples(ss._s, pv(text), pv(off), 2, ctx, flags, pv(codes), n, size, 1, pv(mk), max_rows, 0, pv(ms), pv(wd), None)
        assert walk() == -1 and b"no sample table" in L.rsbwt_last_error()
        assert evaluate() == -1 and b"no sample table" in L.rsbwt_last_error()
        _build(ss, c.pairs)
        assert walk() == 0 and (stop != MARK).all() and (steps != MARK).all() and (ext != MARK).all()
        assert evaluate() == 0 and (msup != MARK).all() and (wide != MARK).all()
        ext[:], steps[:], stop[:], msup[:], wide[:] = MARK, MARK, MARK, MARK, MARK
        bad = [dict(codes=np.frombuffer(b"ab" b"ab" b"ac", np.uint8).copy()), dict(codes=np.frombuffer(b"ac" b"ab", np.uint8).copy(), n=2),
               dict(size=0), dict(size=9, n=1), dict(n=0), dict(codes=None), dict(mk=None), dict(max_rows=0), dict(max_rows=(1 << 20) + 1),
               dict(ctx=0), dict(ctx=256), dict(flags=8), dict(flags=16)]
        for kw in bad:
            assert walk(**kw) == -1, kw
            assert evaluate(**kw) == -1, kw
        for kw in (dict(max_steps=0), dict(max_steps=65536), dict(e=None), dict(st=None), dict(sp=None), dict(o=None)):
            assert walk(**kw) == -1, kw
        assert evaluate(ms=None) == -1 and evaluate(wd=None) == -1
        assert (ext == MARK).all() and (steps == MARK).all() and (stop == MARK).all() and (msup == MARK).all() and (wide == MARK).all()
        # Q = 0 succeeds and touches nothing
        assert L.rsbwt_set_walk_samples(ss._s, None, pv(np.zeros(1, np.uint64)), 0, 20, 1, 4, 0, pv(good), 3, 2, 1, pv(mask), 16, 0, None, None, None, None,
                                        None) == 0
        # the same flag bits the Python layer sets are all the call knows
        assert walk(flags=7) == 0 and walk(max_rows=1 << 20, max_steps=1) == 0
        with pytest.raises(ValueError):
            ss.walk_samples(c.seeds[:1], 20, [b"ab", b"ac"], 2, mask_codes=[b"zz"])
        # a row that cannot be located within max_locate_steps fails the call: it is not left out silently
        with pytest.raises(rsb.RsbwtError) as e:
            ss.walk_samples(c.seeds[:1], c.ctx, c.codes, c.ss, mask_codes=c.mask, max_locate_steps=1)
        assert e.value.code == -1 and "does not end" in str(e.value), str(e.value)
    finally:
        _close(ss, gs)


@pytest.mark.parametrize("ktab", [None, 2])
def test_gpu_walk_samples_on_a_shard_without_terminators(rsb, ktab):
    """7,037 x 'T' and no '$': a candidate without rows has no support; one with rows cannot be located and fails the call,
    as rsbwt_set_sample_counts fails it"""
    runs = np.full(227, (4 << 5) | 31, np.uint8)
    with rsb.GpuBWT(runs=runs, num_strings=0, ktab_depth=ktab) as g:
        ss = rsb.ShardSet([g])
        try:
            ss.meta_build(["TTTT", "ACGT"], [b"ab!!", b"cd!!"])
            got = ss.walk_samples(["ACA", "GGG"], 3, [b"ab", b"cd"], 2, mask_codes=[b"ab"], max_steps=4, max_rows=1 << 20)
            assert got == [("", WR.DEAD_END, (0, 0, 0, 0))] * 2
            with pytest.raises(rsb.RsbwtError) as e:
                ss.walk_samples(["TTT"], 3, [b"ab", b"cd"], 2, mask_codes=[b"ab"], max_steps=4, max_rows=1 << 20, max_locate_steps=8)
            assert e.value.code == -1 and "does not end" in str(e.value)
        finally:
            ss.close()
