"""SiteMatch through the service loop (-m gpu): rsbwt_service_set_sitematch over rsbwt_set_site_reads, driven through the
in-process transport as tests/test_gpu_service_all.py drives All.  The requests are built on the gt fixture as a client
builds them -- a stretch of a haplotype longer than the window, p on either side of max_read_length (40 here: the
fixture's reads have 40 symbols), so that both substr branches of GtTask::run's fix-up and the reverse strand's pos run --
with both isalt values, return types 1 to 4 and two (k, s) pairs in one window, mixed with ExactMatch and KmerMatch
requests.  The expected Replies are encoded by the protobuf runtime: the reads are what ShardSet.gt_aligned_reads returns
for the windows (the fix-up restated below from service.cpp:1028-1040), in its order -- ascending read_row per partition,
not the reference's unordered_set order --, the `s` records are meta_proto.records of the pairs.  Byte for byte."""
import ctypes as C
import hashlib

import pytest

import gt_reference as G
import meta_proto
import meta_reference as MR
import proto_schema
import site_reference as SITE
from kmer_reference import _bwt_runs

pytestmark = pytest.mark.gpu

L_MAX, L_MIN = 40, 30
SS, OTHER = 2, True
BUF = 1 << 20
KS = ((8, 3), (12, 0))
_RC = str.maketrans("ACGTacgt", "TGCAtgca")


def rc(s):
    return s[::-1].translate(_RC)


def fixup(q, p, a, strand, L=L_MAX):
    """GtTask::run:1028-1046 for one strand, in signed arithmetic: (w, pos, alt), or None for the Reply without sub-message"""
    query, pos, alt = q, p, a
    if strand:
        query, pos, alt = rc(q), len(q) - p + 1, rc(a)
    if pos < 0:
        return None
    if pos <= L:
        w = query[:max(L + pos - 1, 0)]
    else:
        if pos - L > len(query):
            return None
        w, pos = query[pos - L:pos - L + 2 * L - 1], L
    return None if pos > len(w) else (w, pos, alt)


class World:
    def __init__(self):
        self.Request, self.ReplyR = proto_schema.build()
        self.Reply, _, _ = meta_proto.build()
        fx = self.fx = G.fixture()
        reads = [r for pair in zip(*fx.shards) for r in pair]
        self.deals = {2: fx.shards, 4: [reads[i::4] for i in range(4)]}
        self.runs = {n: [_bwt_runs(sh) for sh in d] for n, d in self.deals.items()}
        order = sorted(set(reads), key=lambda r: hashlib.sha256(r.encode()).digest())
        kept = [r for r in order if r not in set(order[4::5])]  # every 5th read has no pair: an empty `s`
        short = [0, 4, 5, 8, 12]
        self.pairs = [(r, MR.value_of(r, 0, short)) for r in kept]
        self.value = dict(self.pairs)
        codes = sorted({v[i:i + SS] for v in self.value.values() for i in range(0, len(v) - SS - 1, SS + 2)})[::2]
        codes = [c for c in codes if b"\n" not in c]
        self.hash_text = b"".join(b"sample-%d\t" % i + c + b"\n" for i, c in enumerate(codes))
        self.hash_map = {c: "sample-%d" % i for i, c in enumerate(codes)}
        # the sites: both alleles of allele_pairs' positions, asked from stretches around them
        ref = fx.haps[1]
        self.sites = []
        for (w, _, other, _), _ in SITE.allele_pairs(fx, 12):
            i = ref.find(w) + 39
            assert ref[i - 39:i + 40] == w
            if 100 <= i <= len(ref) - 100 and len(self.sites) < 4:  # (room for a stretch of 200 around the site)
                self.sites.append((i, other))
        assert len(self.sites) == 4

    def site_requests(self):
        """(rt, q, k, s, p, a, isalt): for every site the stretch [i - 100, i + 100) with p = 101 (both strands past
        max_read_length), [i - 20, i + 100) with p = 21 (forward: the first branch) and [i - 100, i + 20) with p = 101 (the
        reverse strand: the first branch), the alt stretch too; return types 1 .. 4 and isalt by turns, the two (k, s) pairs"""
        ref = self.fx.haps[1]
        out = []
        for n, (i, other) in enumerate(self.sites):
            for m, (lo, hi) in enumerate(((100, 100), (20, 100), (100, 20))):
                q, p = ref[i - lo:i + hi], lo + 1
                k, s = KS[(n + m) % 2]
                out.append((1 + (n + m) % 4, q, k, s, p, other, 0))
                out.append((1 + (n + m + 1) % 4, q[:lo] + other + q[lo + 1:], k, s, p, ref[i], (n + m) % 2))
                out.append((2, q, k, s, p, other + "GG", 1))  # (alt[q] is the first character of a)
                # the same site asked on the other strand (the fixture's reads are all of one strand: a window finds them
                # on the strand that reads like the haplotype, here the request's reverse complement)
                out.append((1 + (n + m + 2) % 4, rc(q), k, s, len(q) - p + 1, rc(other), 0))
        return out

    def message(self, t, rt, q, k=None, s=None, p=None, a=None, isalt=None):
        r = self.Request()
        r.t, r.rt, r.q = t, rt, q
        for name, v in (("k", k), ("s", s), ("p", p), ("a", a), ("isalt", isalt)):
            if v is not None:
                setattr(r, name, v)
        return r.SerializeToString()

    def expected(self, ss, S, reqs, per_partition, with_all=True):
        """per request the Replies in sending order: partition by partition (or joined), forward then reverse complement"""
        strands = [[fixup(q, p, a, strand) for strand in (0, 1)] for _, q, _, _, p, a, _ in reqs]
        kept = {}
        for ks in {(k, s) for _, _, k, s, _, _, _ in reqs}:
            items = [(i, strand) for i, r in enumerate(reqs) for strand in (0, 1) if (r[2], r[3]) == ks and strands[i][strand] and strands[i][strand][2]]
            if not items:
                continue
            ws = [strands[i][st][0] for i, st in items]
            res = ss.gt_aligned_reads(ws, [strands[i][st][1] for i, st in items], [strands[i][st][2][:1] for i, st in items],
                                      [1 if reqs[i][6] == 1 else 0 for i, _ in items], ks[0], ks[1], 0)
            for it, cells in zip(items, res):
                kept[it] = cells
        out = []
        for i, (rt, q, k, s, p, a, isalt) in enumerate(reqs):
            mine = []
            rows = range(S) if per_partition else [None]
            for row in rows:
                for strand in (0, 1):
                    if strands[i][strand] is None:
                        m = self.ReplyR()
                        m.rt, m.t, m.q = 4, rt, q
                        mine.append(m.SerializeToString())
                        continue
                    cells = kept.get((i, strand), [[]] * S)
                    reads = cells[row] if per_partition else [r for c in cells for r in c]
                    if rt >= 3:
                        mine.append(meta_proto.all_reply(self.Reply, 4, rt, q, strand == 1, reads, [self.value.get(r, b"") for r in reads], self.hash_map, SS,
                                                         OTHER))
                        continue
                    m = self.ReplyR()
                    m.rt, m.t, m.q = 4, rt, q
                    if rt == 1:
                        (m.c.revcomp_matches if strand else m.c.forward_matches).c = len(reads)
                    else:
                        m.r.SetInParent()
                        for r in reads:
                            (m.r.revcomp_matches if strand else m.r.forward_matches).add().r = r
                    mine.append(m.SerializeToString())
            out.append(mine)
        return out


@pytest.fixture(scope="module")
def world():
    return World()


class Service:
    def __init__(self, rsb, world, tmp_path, partitions=2, per_partition=1, site=True, meta=True, unserved=False, for_reads=True):
        L = self.L = rsb.lib()
        self.S = partitions
        self.gs = [rsb.GpuBWT(runs=runs, num_strings=len(sh), ktab_depth=6, for_reads=for_reads) for sh, runs in zip(world.deals[partitions], world.runs[partitions])]
        self.ss = rsb.ShardSet(self.gs)
        self.tr, self.svc = C.c_void_p(), C.c_void_p()
        assert L.rsbwt_transport_inproc(C.byref(self.tr)) == 0
        assert L.rsbwt_service_create(self.ss._s, self.tr, 2000, 512, per_partition, C.byref(self.svc)) == 0
        L.rsbwt_service_set_reads(self.svc, 1, L_MIN, L_MAX)
        if for_reads:
            assert L.rsbwt_service_set_kmermatch(self.svc, 1) == 0
        L.rsbwt_service_set_unserved(self.svc, 1 if unserved else 0)
        if meta:
            self.ss.meta_build([r for r, _ in world.pairs], [v for _, v in world.pairs])
            hf = tmp_path / "hash.txt"
            hf.write_bytes(world.hash_text)
            assert L.rsbwt_service_set_all(self.svc, 1, str(hf).encode(), SS, 1 if OTHER else 0) == 0, L.rsbwt_last_error()
        self.site_rc = L.rsbwt_service_set_sitematch(self.svc, 1) if site else 0

    def run(self, msgs):
        """push, drain: every Reply of channel PUSH in order"""
        L = self.L
        assert L.rsbwt_service_start(self.svc) == 0
        for w in msgs:
            buf = (C.c_uint8 * len(w)).from_buffer_copy(w)
            assert L.rsbwt_transport_push_request(self.tr, buf, len(w)) == 0
        L.rsbwt_transport_close(self.tr)
        assert L.rsbwt_service_stop(self.svc) == 0, L.rsbwt_last_error()
        out, buf, n = [], (C.c_uint8 * BUF)(), C.c_size_t()
        while L.rsbwt_transport_pop_reply(self.tr, 0, buf, BUF, C.byref(n), 1000) == 0:
            out.append(bytes(buf[:n.value]))
        return out

    def close(self):
        self.L.rsbwt_service_free(self.svc)
        self.L.rsbwt_transport_free(self.tr)
        self.ss.close()
        for g in self.gs:
            g.close()


def _site_msgs(world, reqs):
    return [world.message(4, rt, q, k, s, p, a, isalt) for rt, q, k, s, p, a, isalt in reqs]


@pytest.mark.parametrize("partitions,per_partition", [(2, 1), (4, 1), (2, 0)], ids=["two", "four", "joined"])
def test_gpu_service_site_replies(rsb, world, tmp_path, partitions, per_partition):
    """per partition over two and four partitions, and joined: every return type, both isalt values, two (k, s) pairs, woven
    with ExactMatch and KmerMatch requests whose Replies are what the same service sends with sitematch off"""
    reqs = world.site_requests()
    site = _site_msgs(world, reqs)
    ref = world.fx.haps[1]
    others = [world.message(2, 1, ref[100:130]), world.message(3, 1, ref[200:260], 20, 0), world.message(2, 2, ref[300:340]), world.message(3, 2, ref[1500:1560], 30, 3)]
    msgs, kind = [], []
    for j, m in enumerate(site):
        msgs.append(m)
        kind.append(("site", j))
        if j % 5 == 0:
            msgs.append(others[(j // 5) % 4])
            kind.append(("other", (j // 5) % 4))
    rows = partitions if per_partition else 1
    sv = Service(rsb, world, tmp_path, partitions, per_partition)
    try:
        assert sv.site_rc == 0
        want = world.expected(sv.ss, partitions, reqs, per_partition)
        got = sv.run(msgs)
        assert len(got) == 2 * rows * len(msgs)
        assert sv.L.rsbwt_service_site_requests(sv.svc) == sum(1 for r in reqs if r[0] <= 2)
    finally:
        sv.close()
    off = Service(rsb, world, tmp_path, partitions, per_partition, site=False)
    try:
        plain = off.run(others)
        assert len(plain) == 2 * rows * len(others) and off.L.rsbwt_service_site_requests(off.svc) == 0
    finally:
        off.close()
    for n, (what, j) in enumerate(kind):
        mine = got[n * 2 * rows:(n + 1) * 2 * rows]
        if what == "other":
            assert mine == plain[j * 2 * rows:(j + 1) * 2 * rows], (n, j)
            continue
        assert mine == want[j], (j, reqs[j][0], reqs[j][2:5], [len(x) for x in mine], [len(x) for x in want[j]])
    # (reads are kept on both strands and under every return type: the comparison is not of empty Replies)
    for rt in (1, 2, 3, 4):
        for strand in (0, 1):
            n = 0
            for j, w in enumerate(want):
                for x in w[strand::2] if reqs[j][0] == rt else ():
                    m = (world.Reply if rt > 2 else world.ReplyR).FromString(x)
                    side = "revcomp_matches" if strand else "forward_matches"
                    n += getattr(m.c, side).c if rt == 1 else len(getattr(m.r if rt == 2 else m.a, side))
            assert n > 0, (rt, strand)


def test_gpu_service_site_header_only_and_empty_answers(rsb, world, tmp_path):
    """p > |q| and p with pos > |w|: the Reply carries rt, t and q only; p = 0, k = 0, an empty a, k > |w|, a negative s:
    zero / empty with the sub-message present; a negative p"""
    ref = world.fx.haps[1]
    (i, other), q = world.sites[0], None
    q = ref[i - 100:i + 100]
    reqs = []
    for rt in (1, 2, 3):
        reqs += [(rt, q, 8, 3, 201, other, 0),    # p > |q|: forward pos - L = 161 <= |q| but w = 39 symbols < pos = 40; reverse pos = 0
                 (rt, q, 8, 3, 300, other, 0),    # forward: substr start past the end; reverse: pos < 0
                 (rt, q[:30], 8, 3, 31, other, 0),  # pos = 31 <= L, w = q whole (30 symbols): pos > |w|
                 (rt, q, 8, 3, -5, other, 0),     # forward pos < 0
                 (rt, q, 8, 3, 0, other, 0), (rt, q, 0, 3, 101, other, 0), (rt, q, 8, 3, 101, "", 0), (rt, q, 200, 3, 101, other, 0),
                 (rt, q, 8, -1, 101, other, 0), (rt, q, 8, 3, 101, other, 0)]
    sv = Service(rsb, world, tmp_path)
    try:
        want = world.expected(sv.ss, 2, reqs, True)
        got = sv.run(_site_msgs(world, reqs))
    finally:
        sv.close()
    assert len(got) == 4 * len(reqs)
    for j, r in enumerate(reqs):
        assert got[4 * j:4 * j + 4] == want[j], (j, r[0], r[2:5])
    header = lambda j, strand: fixup(reqs[j][1], reqs[j][4], reqs[j][5], strand) is None  # noqa: E731
    assert header(0, 0) and not header(0, 1) and header(1, 0) and header(1, 1) and header(2, 0) and header(3, 0)
    for j in range(10):
        for strand in (0, 1):
            m = world.ReplyR.FromString(got[4 * j + strand])
            assert (m.rt, m.t) == (4, 1) and m.HasField("c") == (not header(j, strand))
    assert any(world.ReplyR.FromString(x).c.forward_matches.c > 0 for x in got[4 * 9:4 * 9 + 4])  # the plain request keeps reads
    assert all(world.ReplyR.FromString(x).c.forward_matches.c == 0 and world.ReplyR.FromString(x).c.revcomp_matches.c == 0 for x in got[4 * 4:4 * 9])


def test_gpu_service_site_off_is_todays_behaviour(rsb, world, tmp_path):
    """sitematch off: under unserved = "empty" the bytes the same requests get today (rsbwt_proto_encode_empty_reply), and
    nothing without it; with sitematch on and no rsbwt_service_set_all, All / Samples stay unserved"""
    reqs = world.site_requests()[:12]
    msgs = _site_msgs(world, reqs)

    def empty(L, rt, q, strand):
        b = (C.c_uint8 * 1024)()
        n = L.rsbwt_proto_encode_empty_reply(b, 1024, 4, rt, q.encode(), len(q), strand)
        return bytes(b[:n])
    sv = Service(rsb, world, tmp_path, site=False, unserved=True)
    try:
        got = sv.run(msgs)
        assert got == [empty(sv.L, r[0], r[1], strand) for r in reqs for _ in range(2) for strand in (0, 1)]
    finally:
        sv.close()
    sv = Service(rsb, world, tmp_path, site=False)
    try:
        assert sv.run(msgs) == []
    finally:
        sv.close()
    sv = Service(rsb, world, tmp_path, meta=False)
    try:
        assert sv.site_rc == 0
        want = world.expected(sv.ss, 2, reqs, True)
        got = sv.run(msgs)
        assert got == [x for r, w in zip(reqs, want) if r[0] <= 2 for x in w] and any(r[0] >= 3 for r in reqs)
    finally:
        sv.close()
    sv = Service(rsb, world, tmp_path, meta=False, unserved=True)
    try:
        got = sv.run(msgs)
        want = [w if r[0] <= 2 else [empty(sv.L, r[0], r[1], strand) for _ in range(2) for strand in (0, 1)] for r, w in zip(reqs, want)]
        assert got == [x for w in want for x in w]
    finally:
        sv.close()


def test_gpu_service_site_refusals(rsb, world, tmp_path):
    """shards not opened for reads; a max_read_length over 2,048"""
    sv = Service(rsb, world, tmp_path, meta=False, for_reads=False)
    try:
        assert sv.site_rc == -1 and b"RSBWT_OPEN_READS" in sv.L.rsbwt_last_error()
    finally:
        sv.close()
    sv = Service(rsb, world, tmp_path, meta=False, site=False)
    try:
        sv.L.rsbwt_service_set_reads(sv.svc, 1, 73, 2049)
        assert sv.L.rsbwt_service_set_sitematch(sv.svc, 1) == -1 and b"2048" in sv.L.rsbwt_last_error()
        sv.L.rsbwt_service_set_reads(sv.svc, 1, 73, 2048)
        assert sv.L.rsbwt_service_set_sitematch(sv.svc, 1) == 0 and sv.L.rsbwt_service_set_sitematch(sv.svc, 0) == 0
    finally:
        sv.close()
