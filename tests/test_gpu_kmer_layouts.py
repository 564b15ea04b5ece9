"""KmerMatch's read-identity walk (csrc/kmer_reads.hip: kr_ident_kernel, kr_jump_kernel, kr_resolve_kernel, run_pass) on every
line layout and read shape (-m gpu), held to tests/kmer_reference.py: per-row LF walks on the oracle, no chains, nothing
deduplicated before the end.

Fixtures, spans and queries come from tests/test_kmer_fixtures.py, which proves on the CPU that every layout is of the kind
its case means and that the walks enter windows of that kind; here the GPU builder's far_lines() / spilled_symbols() are
held to those stats, so a builder change that moves a case off its layout fails instead of passing on the easy path.  Only
valid BWTs are walked: every LF walk ends on a '$' row.

rsbwt_set_kmer_reads ACCEPTS a set whose shards were opened without RSBWT_OPEN_READS (only the service loop refuses one:
tests/test_gpu_kmer_match.py), so the plain layout is part of the matrix, at two spans per fixture.

What is asserted per call is exact where it counts the same operation: the strings against the oracle composition, and the
work counters -- candidates, identities, extracted -- against the reference's identities, per pass."""
import ctypes as C

import numpy as np
import pytest

import proto_schema
import test_kmer_fixtures as F
from kmer_reference import Walks, _expected, _rc, candidate_rows, expected_over

pytestmark = pytest.mark.gpu

WIDE_DEFAULT = 1 << 22  # candidate rows above which a job gets a pass of its own (kmer_reads.hip; RSBWT_KMER_WIDE_ROWS)


class Ref:
    """one fixture's oracle side: per shard the index and its walks, and per request the expectations, computed once"""

    def __init__(self, oracle, name):
        self.fx = F.fixture(name)
        self.oix = [oracle.from_runs(r, len(sh)) for sh, r in zip(self.fx.shards, self.fx.runs())]
        self.walks = [Walks(o) for o in self.oix]
        self.cache = {}
        self.lens = [{} for _ in self.oix]

    def read_len(self, p, ident):
        if ident not in self.lens[p]:
            self.lens[p][ident] = len("".join(self.oix[p].extract(ident, cap=1 << 12)))
        return self.lens[p][ident]

    def request(self, qs, k, skip, minl, maxl):
        """per query and shard: the strings, the candidate rows' identities, the full walks' LF steps; and whether the
        oracle says a chain saves steps (a row of the tile at skip + 1 whose predecessors spell the query back to the tile
        at 0, in a read that goes on before it)"""
        key = (tuple(qs), k, skip, minl, maxl)
        if key in self.cache:
            return self.cache[key]
        out = []
        chain = False
        step = skip + 1
        for w in qs:
            per = []
            for p, oix in enumerate(self.oix):
                rows = candidate_rows(oix, w, k, skip, maxl)
                wk = self.walks[p]
                per.append(dict(strings=_expected(oix, w, k, skip, minl, maxl), ncand=len(rows), ids={wk.identity(r) for r in rows},
                                steps=sum(wk.steps(r) for r in rows)))
                if 0 < k < minl and len(w) >= k + step and set(w[:k + step]) <= set("ACGT"):
                    lo, up = oix.find_interval(w[:k + step])
                    chain = chain or any(oix.char(r) != "$" for r in range(lo, up + 1))
            out.append(per)
        self.cache[key] = (out, chain)
        return self.cache[key]

    def work(self, exp, wide, stride):
        """the exact work counters of one call: jobs with more than `wide` candidate rows have a pass of their own, the
        others share one; identities are deduplicated per pass and shard"""
        S = len(self.oix)
        passes = [[j for j, per in enumerate(exp) if sum(x["ncand"] for x in per) <= wide]]
        passes += [[j] for j, per in enumerate(exp) if sum(x["ncand"] for x in per) > wide]
        ident = over = 0
        for pas in passes:
            for p in range(S):
                ids = set().union(*[exp[j][p]["ids"] for j in pas]) if pas else set()
                ident += len(ids)
                over += sum(1 for r in ids if self.read_len(p, r) > stride)
        return dict(candidates=sum(x["ncand"] for per in exp for x in per), identities=ident, extracted=ident + over,
                    steps=sum(x["steps"] for per in exp for x in per))


@pytest.fixture(scope="module")
def refs(oracle):
    built = {}

    def get(name):
        if name not in built:
            built[name] = Ref(oracle, name)
        return built[name]
    return get


def _open(rsb, ref, span, room, ktab, shards=None):
    gs = []
    for p, (sh, runs) in enumerate(zip(ref.fx.shards, ref.fx.runs())):
        if shards is None or p in shards:
            gs.append(rsb.GpuBWT(runs=runs, num_strings=len(sh), ktab_depth=ktab, window_span=span, for_reads=room))
    return gs


def _check_layout(rsb, ref, gs, kind, span, room):
    """the GPU builder's layout is the one the CPU guard saw"""
    for p, g in enumerate(gs):
        S = g.window_span()
        if span:
            assert S == span
            st = F.LAYOUT_STATS[(ref.fx.name, p, span, room)]
        else:
            st = F.selftest(rsb, ref.fx.runs()[p], S, room)  # (the builder's own choice of S: the CPU guard run at that S)
        assert (g.far_lines(), g.spilled_symbols()) == (st[2], st[5]), (ref.fx.name, p, S, st)
        if span:
            F.assert_kind(kind, st)


def _check_call(rsb, ss, ref, qs, k, skip, minl, maxl, wide, where):
    exp, chain = ref.request(qs, k, skip, minl, maxl)
    got = ss.kmer_reads(qs, k, skip, minl, maxl, read_stride=1024)
    work = rsb.ShardSet.kmer_last_work()
    cnt = ss.kmer_count(qs, k, skip, minl, maxl)
    work_c = rsb.ShardSet.kmer_last_work()
    for q, w in enumerate(qs):
        for p in range(len(ref.oix)):
            e = exp[q][p]["strings"]
            assert len(got[q][p]) == len(set(got[q][p])), (where, k, skip, q, p, w)
            assert set(got[q][p]) == e, (where, k, skip, q, p, w)
            assert int(cnt[q, p]) == len(e), (where, k, skip, q, p, w)
    for wk, stride in ((work, 1024), (work_c, 256)):
        want = ref.work(exp, wide, stride)
        at = (where, k, skip, wide, stride, wk, want)
        assert wk["candidates"] == want["candidates"], at
        assert wk["identities"] == want["identities"], at
        assert wk["extracted"] == want["extracted"], at
        assert wk["identities"] <= wk["walked"] <= wk["candidates"], at
        assert wk["lf_steps"] <= want["steps"], at
        if chain:
            assert wk["lf_steps"] < want["steps"], at
    return got


def _requests(fx):
    return [(k, s, F.MINL, F.MAXL) for k, s in fx.ks] + [(k, s, F.LONG_MINL, F.LONG_MAXL) for k, s in F.LONG_KS]


@pytest.mark.parametrize("lay", F.LAYOUTS, ids=[F.layout_id(x) for x in F.LAYOUTS])
def test_gpu_kmer_identities_on_every_layout(rsb, refs, monkeypatch, lay):
    """every request of the fixture in one call, and again with every job in a pass of its own (RSBWT_KMER_WIDE_ROWS=1: the
    same lists, order included): strings, counts and work counters against the per-row reference"""
    name, kind, span, room, ktab = lay
    ref = refs(name)
    gs = _open(rsb, ref, span, room, ktab)
    ss = rsb.ShardSet(gs)
    try:
        _check_layout(rsb, ref, gs, kind, span, room)
        nonempty = chains = 0
        for k, skip, minl, maxl in _requests(ref.fx):
            qs = ref.fx.queries(k, skip)
            monkeypatch.delenv("RSBWT_KMER_WIDE_ROWS", raising=False)
            together = _check_call(rsb, ss, ref, qs, k, skip, minl, maxl, WIDE_DEFAULT, F.layout_id(lay))
            monkeypatch.setenv("RSBWT_KMER_WIDE_ROWS", "1")
            alone = _check_call(rsb, ss, ref, qs, k, skip, minl, maxl, 1, F.layout_id(lay))
            assert alone == together, (F.layout_id(lay), k, skip)
            exp, chain = ref.request(qs, k, skip, minl, maxl)
            nonempty += sum(bool(x["strings"]) for per in exp for x in per)
            chains += chain
        assert nonempty > 50 and chains >= len(ref.fx.ks)  # (the oracle: the requests match reads, and chains exist)
    finally:
        monkeypatch.delenv("RSBWT_KMER_WIDE_ROWS", raising=False)
        ss.close()
        for g in gs:
            g.close()


def test_gpu_kmer_repeats_have_many_rows_per_identity(rsb, refs):
    """the tandem repeats with their flanks, skip + 1 equal to the period (the predecessor tile is the tile itself), coprime
    to it, and skip = 0 on the homopolymer and on "ACGT" * n (a cycle of four tiles): real hits, more candidate rows than
    identities (the oracle's count), every identity found once"""
    ref = refs("repeat")
    span = F.SPANS["repeat"]["chain"]
    gs = _open(rsb, ref, span, True, 6)
    ss = rsb.ShardSet(gs)
    try:
        _check_layout(rsb, ref, gs, "chain", span, True)
        for k, skip in ref.fx.ks:
            for w in ref.fx.extra:
                exp, chain = ref.request([w], k, skip, F.MINL, F.MAXL)
                assert exp[0][0]["ncand"] > len(exp[0][0]["ids"]) > 0 and chain, (k, skip, w[:20])
                _check_call(rsb, ss, ref, [w], k, skip, F.MINL, F.MAXL, WIDE_DEFAULT, ("repeat stretch", w[:20]))
    finally:
        ss.close()
        for g in gs:
            g.close()


def test_gpu_kmer_shards_of_different_layouts_in_one_set(rsb, refs):
    """shard 0 at the builder's span, shard 1 at the far-chain span, in ONE set: per shard the answers of the single-layout
    sets, order included"""
    ref = refs("pop")
    far = F.SPANS["pop"]["chain"]
    answers = {}
    for label, spans in (("auto", (0, 0)), ("far", (far, far)), ("mixed", (0, far))):
        gs = [_open(rsb, ref, sp, True, 6, shards=(p,))[0] for p, sp in enumerate(spans)]
        ss = rsb.ShardSet(gs)
        try:
            for p, sp in enumerate(spans):
                if sp:  # (the far-chain span: the layout the CPU guard saw)
                    st = F.LAYOUT_STATS[("pop", p, sp, True)]
                    assert (gs[p].window_span(), gs[p].far_lines(), gs[p].spilled_symbols()) == (sp, st[2], st[5])
                    F.assert_kind("chain", st)
            for k, skip in ref.fx.ks:
                answers[label, k, skip] = _check_call(rsb, ss, ref, ref.fx.queries(k, skip), k, skip, F.MINL, F.MAXL, WIDE_DEFAULT, label)
        finally:
            ss.close()
            for g in gs:
                g.close()
    for k, skip in ref.fx.ks:
        for q, per in enumerate(answers["mixed", k, skip]):
            assert per[0] == answers["auto", k, skip][q][0] and per[1] == answers["far", k, skip][q][1], (k, skip, q)


def _long_queries(ref):
    longs = ref.fx.longs
    return [longs[6][100:200], longs[-1][350:450], longs[1][:80], longs[0][150:], longs[12][40:120], _rc(longs[17][300:380])]


@pytest.mark.parametrize("kind", ["auto", "chain"])
def test_gpu_kmer_reads_longer_than_the_internal_stride(rsb, refs, kind):
    """reads of 257 .. 600 symbols: whole at read_stride = 1024; counted by kmer_count, whose stride is 256 inside, with the
    second extraction shown by `extracted`; and at read_stride = 256 through the C call exactly the over-long reads are
    marked 0xFFFFFFFF, the others intact"""
    ref = refs("ragged")
    span = F.SPANS["ragged"][kind] if kind != "auto" else 0
    gs = _open(rsb, ref, span, True, 6)
    ss = rsb.ShardSet(gs)
    L = rsb.lib()
    try:
        _check_layout(rsb, ref, gs, kind, span, True)
        qs = _long_queries(ref)
        for k, skip in ((15, 0), (20, 3), (31, 5)):
            exp, _ = ref.request(qs, k, skip, F.MINL, F.MAXL)
            want = ref.work(exp, WIDE_DEFAULT, 256)
            n_over = want["extracted"] - want["identities"]
            assert n_over == expected_over(ref.oix[0], set().union(*[per[0]["ids"] for per in exp]), 256)
            assert n_over >= 5 and any(len(x) > 512 for per in exp for x in per[0]["strings"])  # (the oracle: over-long reads are matched)
            assert any(256 < len(x) <= 1024 for per in exp for x in per[0]["strings"])
            got = _check_call(rsb, ss, ref, qs, k, skip, F.MINL, F.MAXL, WIDE_DEFAULT, ("long", kind))
            assert any(len(x) > 256 for per in got for x in per[0])
            cnt = ss.kmer_count(qs, k, skip, F.MINL, F.MAXL)
            wk = rsb.ShardSet.kmer_last_work()
            assert [int(c) for c in cnt[:, 0]] == [len(per[0]["strings"]) for per in exp]
            assert wk["extracted"] == wk["identities"] + n_over and wk["extracted"] > wk["identities"]
            # read_stride = 256 through the C call
            text, off = ss._var_text(qs)
            Q = len(qs)
            first = np.zeros(Q + 1, np.uint64)
            total = sum(len(per[0]["strings"]) for per in exp)
            reads = np.zeros((total, 256), np.uint8)
            ln = np.zeros(total, np.uint32)
            n = C.c_size_t()
            rc = L.rsbwt_set_kmer_reads(ss._s, text.ctypes.data_as(C.c_void_p), off.ctypes.data_as(C.c_void_p), Q, k, skip, F.MINL, F.MAXL,
                                        first.ctypes.data_as(C.c_void_p), reads.ctypes.data_as(C.c_void_p), 256,
                                        ln.ctypes.data_as(C.c_void_p), total, C.byref(n))
            assert rc == 0 and n.value == total, L.rsbwt_last_error()
            for q, per in enumerate(exp):
                mine = range(int(first[q]), int(first[q + 1]))
                fit = {x for x in per[0]["strings"] if len(x) <= 256}
                assert sum(1 for r in mine if ln[r] == 0xFFFFFFFF) == len(per[0]["strings"]) - len(fit), (k, skip, q)
                assert sorted(reads[r, :ln[r]].tobytes().decode() for r in mine if ln[r] != 0xFFFFFFFF) == sorted(fit), (k, skip, q)
    finally:
        ss.close()
        for g in gs:
            g.close()


def test_gpu_service_kmer_replies_hold_reads_longer_than_256(rsb, refs):
    """through the service loop: the KmerMatch Reads replies of requests that match reads longer than 256 symbols, parsed
    with the re-typed schema, hold the oracle's sets; the Count replies its counts"""
    from test_gpu_kmer_match import MAXL, MINL, _serve
    ref = refs("ragged")
    gs = _open(rsb, ref, F.SPANS["ragged"]["chain"], True, 6)
    ss = rsb.ShardSet(gs)
    Request, Reply = proto_schema.build()
    try:
        qs = _long_queries(ref)[:3]
        reqs = []
        for q in qs:
            for rt in (1, 2):
                r = Request()
                r.t, r.rt, r.q, r.k, r.s = 3, rt, q, 31, 5
                reqs.append(r)
        out = _serve(rsb, ss, [r.SerializeToString() for r in reqs], 1)
        assert out[1] == [] and len(out[0]) == 2 * len(reqs)
        longest = 0
        for i, r in enumerate(reqs):
            for strand, w in ((0, r.q), (1, _rc(r.q))):
                exp = _expected(ref.oix[0], w, 31, 5, MINL, MAXL)
                rep = Reply()
                rep.ParseFromString(out[0][2 * i + strand])
                assert (rep.rt, rep.t, rep.q) == (3, r.rt, r.q)
                if r.rt == 2:
                    got = [x.r for x in (rep.r.revcomp_matches if strand else rep.r.forward_matches)]
                    assert len(got) == len(set(got)) and set(got) == exp, (r.q, strand)
                    longest = max([longest] + [len(x) for x in got])
                else:
                    m = rep.c.revcomp_matches if strand else rep.c.forward_matches
                    assert m.c == len(exp), (r.q, strand)
        assert longest > 512
    finally:
        ss.close()
        for g in gs:
            g.close()
