"""The site-sample-counts reference the site tests share -- TEST INFRASTRUCTURE.  include/rsbwt.h's definition of
rsbwt_set_site_sample_counts restated from the restatements that exist:

  * counts_by_ordinal: per (request, shard) the candidates of gt_reference.expected(...)[q][p][1], head and value from
    sample_reference.OracleShards (sides[p].lookup, heads, tables), the verdict from ksw_reference.align_gt_read in GT_KEEP
    (memoised), the records cut and tallied as sample_reference.counts_oracle cuts them;
  * counts_by_string: with no ordinals at all -- the survivors looked up by string in a plain dict of the pairs in which later
    pairs overwrite, restricted to strings that occur in that shard's read list, the records tallied in plain Python.

Both give {strings, copies, aligned, carriers}.  rows_by_ordinal walks every row of every leg the way the device does (the
span filter as csrc/gt_narrow.hip applies it, the head bit, the row's own length test) and gives the work numbers that are
about rows -- legs, candidates, kept, head_rows, extracted -- and, per (request, shard, head ordinal), how each of its kept
rows fares: what the class test asks about."""
import numpy as np

import gt_reference as G
import ksw_reference as kr
import meta_reference as MR
import sample_reference as SR

WORK_KEYS = ("legs", "narrow_steps", "candidates", "kept", "head_rows", "extracted", "aligned", "carriers", "records", "unknown")
_KEEP = {}


def keeps(s, w, pos, alt, isalt):
    at = (s, w, pos, alt, isalt)
    if at not in _KEEP:
        _KEEP[at] = kr.align_gt_read(s, w, pos, alt, isalt) in kr.GT_KEEP
    return _KEEP[at]


def fixture_requests(fx):
    """the 28 requests of tests/test_gpu_gt_align.py's fixture, restated: the gt fixture's queries plus pos = 0 and pos =
    L + 1; the alt allele the next base for most, the reference base itself for some, an N for a few; isalt alternating"""
    g = fx.haps[1]
    qs = fx.queries() + [(g[100:179], 0), (g[1500:1579], 80)]
    out = []
    for i, (w, pos) in enumerate(qs):
        c = w[pos - 1] if 1 <= pos <= len(w) else "A"
        alt = "N" if i % 7 == 6 else c if i % 5 == 4 else "ACGT"[("ACGT".find(c) + 1) % 4]
        out.append((w, pos, alt, i % 2))
    return out


def allele_pairs(fx, n=8):
    """the first n positions (at least 60 from either end) where some haplotype differs from haps[1]: for each the request
    for the reference allele (w, alt = the other base) and the one for the other allele (w with the other base at the site,
    alt = the reference base), both isalt = 0, the site at 40 of a window of 79"""
    ref = fx.haps[1]
    out = []
    for i in range(60, len(ref) - 60):
        others = [h[i] for h in fx.haps if h[i] != ref[i]]
        if not others:
            continue
        w = ref[i - 39:i + 40]
        o = others[0]
        out.append(((w, 40, o, 0), (w[:39] + o + w[40:], 40, ref[i], 0)))
        if len(out) == n:
            break
    return out


def batch(fx):
    """(requests, pairs): the fixture's requests and the 8 allele pairs behind them; pairs = [(index of the reference
    allele's request, index of the other's)].  Behind those, for the first two pairs, the reference window asked with a THIRD
    base as alt: a read with the other allele then scores the same against both targets and leaves align_gt_read by the
    mismatch at the site (verdict 8), which no request above reaches"""
    reqs = fixture_requests(fx)
    pairs = []
    found = allele_pairs(fx)
    for a, b in found:
        pairs.append((len(reqs), len(reqs) + 1))
        reqs += [a, b]
    for (w, pos, other, _), _ in found[:2]:
        third = next(c for c in "ACGT" if c not in (w[pos - 1], other))
        reqs.append((w, pos, third, 0))
    return reqs, pairs


class Side:
    """one read set under one pair list: the gt restatement's shards and the sample restatement's, built once"""

    def __init__(self, oracle, shards, runs, pairs, name):
        self.shards, self.pairs, self.name = shards, pairs, name
        self.gt = [G.OracleShard(oracle.from_runs(r, len(sh))) for sh, r in zip(shards, runs)]
        self.osh = SR.OracleShards(oracle, shards, runs, pairs)

    def expected(self, requests, k, skip, M):
        key = ("site", self.name, tuple((w, pos) for w, pos, _, _ in requests))
        return G.expected(self.gt, key, [(w, pos) for w, pos, _, _ in requests], k, skip, M)


class _Tally:
    """the record cut of sample_reference.counts_oracle: a value's per-column counts, memoised"""

    def __init__(self, codes, size_of_sample, has_other):
        self.C, self.ss, self.other = len(codes), size_of_sample, has_other
        self.R = SR.rec_size(size_of_sample, has_other)
        keys = np.array([SR.key_of(c) for c in codes], np.uint64)
        self.by_key = np.argsort(keys)
        self.skeys = keys[self.by_key]
        self.memo = {}

    def parse(self, value):
        if value not in self.memo:
            C, R = self.C, self.R
            n = len(value) // R
            a = np.frombuffer(value[:n * R], np.uint8).reshape(n, R)
            k = np.zeros(n, np.uint64)
            for b in range(self.ss):
                k = (k << np.uint64(8)) | a[:, b].astype(np.uint64)
            at = np.searchsorted(self.skeys, k)
            hit = (at < C) & (self.skeys[np.minimum(at, C - 1)] == k)
            col = np.where(hit, self.by_key[np.minimum(at, C - 1)], C)
            c = a[:, self.ss].astype(np.int8).astype(np.int64) - 33 if self.other else np.ones(n, np.int64)
            self.memo[value] = (np.bincount(col, minlength=C + 1).astype(np.uint32), np.bincount(col, weights=c, minlength=C + 1).astype(np.int64), n,
                                int((col == C).sum()))
        return self.memo[value]


def counts_by_ordinal(side, requests, k, skip, M, codes, size_of_sample, has_other):
    exp = side.expected(requests, k, skip, M)
    osh, Q, C = side.osh, len(requests), len(codes)
    t = _Tally(codes, size_of_sample, has_other)
    strings, copies = np.zeros((Q, C + 1), np.uint32), np.zeros((Q, C + 1), np.int64)
    aligned, carriers = np.zeros(Q, np.uint64), np.zeros(Q, np.uint64)
    work = dict(aligned=0, carriers=0, records=0, unknown=0)
    for q, (w, pos, alt, isalt) in enumerate(requests):
        for p in range(len(side.shards)):
            for _, s in exp[q][p][1]:
                o, c, _ = osh.sides[p].lookup(s)
                if c == 0 or o not in osh.heads[p]:
                    continue
                aligned[q] += 1
                work["aligned"] += 1
                if not keeps(s, w, pos, alt, isalt):
                    continue
                st, cp, n, unk = t.parse(osh.tables[p][o])
                strings[q] += st
                copies[q] += cp
                carriers[q] += 1
                work["carriers"] += 1
                work["records"] += n
                work["unknown"] += unk
    return dict(strings=strings, copies=copies, aligned=aligned, carriers=carriers, work=work)


def counts_by_string(side, requests, k, skip, M, codes, size_of_sample, has_other):
    exp = side.expected(requests, k, skip, M)
    Q, C, R = len(requests), len(codes), SR.rec_size(size_of_sample, has_other)
    column = {c: i for i, c in enumerate(codes)}
    named = {}
    for read, value in side.pairs:
        if MR.searchable(read):
            named[read] = value  # a later pair overwrites
    strings, copies = [[0] * (C + 1) for _ in range(Q)], [[0] * (C + 1) for _ in range(Q)]
    aligned, carriers = [0] * Q, [0] * Q
    work = dict(aligned=0, carriers=0, records=0, unknown=0)
    for q, (w, pos, alt, isalt) in enumerate(requests):
        for p, sh in enumerate(side.shards):
            here = set(sh)
            for _, s in exp[q][p][1]:
                if s not in named or s not in here:
                    continue
                aligned[q] += 1
                work["aligned"] += 1
                if not keeps(s, w, pos, alt, isalt):
                    continue
                carriers[q] += 1
                work["carriers"] += 1
                value = named[s]
                for i in range(len(value) // R):
                    rec = value[i * R:(i + 1) * R]
                    col = column.get(rec[:size_of_sample], C)
                    b = rec[size_of_sample] if has_other else 34
                    strings[q][col] += 1
                    copies[q][col] += (b - 256 if b > 127 else b) - 33
                    work["records"] += 1
                    work["unknown"] += col == C
    return dict(strings=np.array(strings, np.uint32).reshape(Q, C + 1), copies=np.array(copies, np.int64).reshape(Q, C + 1),
                aligned=np.array(aligned, np.uint64), carriers=np.array(carriers, np.uint64), work=work)


def left_row_stays(pos, end, offset, k, read_len):
    """gt_reference's test of a row of a LEFT leg (find_gt_reads :538) in its own words: dropped iff
    (pos - end) mod 2^64 > (|postfix| - k) + 4"""
    return not (((pos - end) & G.U64) > ((read_len - offset) - k) + G.INDEL)


_ROWS = {}


def rows_by_ordinal(side, requests, k, skip, M):
    """every row of every leg as the device takes it.  Returns (work, items): work = legs, candidates, kept (rows the span
    filter of csrc/gt_narrow.hip keeps: every COVER row, a RIGHT row by its offset, a LEFT row pending its read's length),
    head_rows (of those on a head ordinal), extracted (the distinct (shard, ordinal) among them); items[(q, p, ordinal)] =
    (read string, [(pending, stays)] of its kept rows)"""
    at = (side.name, tuple(requests), k, skip, M)
    if at in _ROWS:
        return _ROWS[at]
    exp = side.expected(requests, k, skip, M)
    work = dict(legs=0, candidates=0, kept=0, head_rows=0, extracted=0)
    items = {}
    for q, (w, pos, _, _) in enumerate(requests):
        for p, gt in enumerate(side.gt):
            oix = side.osh.sides[p].oix
            for tile, _, a, b, lo, up in exp[q][p][0]:
                work["legs"] += 1
                width = (up - lo + 1) & G.U64
                work["candidates"] += width
                start, end = (skip + 1) * tile + 1, (skip + 1) * tile + k  # the TILE's span decides the side, 1-based
                for j in range(lo, lo + width):
                    prefix, postfix = gt.extract(j)
                    offset, n = len(prefix), len(prefix) + len(postfix)
                    if pos > end:
                        kept, pending, stays = ((pos - b) & G.U64) <= 65536 + 4, True, left_row_stays(pos, b, offset, k, n)
                    elif pos < start:
                        kept, pending, stays = ((a + 1 - pos) & G.U64) <= offset + G.INDEL, False, True
                    else:
                        kept, pending, stays = True, False, True
                    if not kept:
                        continue
                    work["kept"] += 1
                    o = oix.occ("$", gt.identity(j)) - 1
                    if o not in side.osh.heads[p]:
                        continue
                    work["head_rows"] += 1
                    items.setdefault((q, p, o), (prefix + postfix, []))[1].append((pending, stays))
    work["extracted"] = len({(p, o) for _, p, o in items})
    _ROWS[at] = (work, items)
    return _ROWS[at]


def want(side, requests, k, skip, M, codes, size_of_sample, has_other):
    """the call's four outputs and its work numbers (all but narrow_steps, which depends on the k-mer tables: the GPU test
    takes it from rsbwt_set_gt_last_work)"""
    out = counts_by_ordinal(side, requests, k, skip, M, codes, size_of_sample, has_other)
    out["work"] = dict(out["work"], **rows_by_ordinal(side, requests, k, skip, M)[0])
    return out


def same(a, b, work=True):
    """the first difference between two answers, or None"""
    for k in ("aligned", "carriers", "strings", "copies"):
        if a[k].shape != b[k].shape or a[k].dtype != b[k].dtype or not (a[k] == b[k]).all():
            return k, np.argwhere(a[k] != b[k])[:5].tolist() if a[k].shape == b[k].shape else (a[k].shape, b[k].shape)
    if work:
        diff = {k: (a["work"].get(k), b["work"].get(k)) for k in set(a["work"]) & set(b["work"]) if a["work"][k] != b["work"][k]}
        return ("work", diff) if diff else None
    return None
