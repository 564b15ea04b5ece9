"""The sample-counts reference the sample tests share -- TEST INFRASTRUCTURE.  include/rsbwt.h's definition of
rsbwt_set_sample_counts restated twice:

  * over the oracle's BWT (counts_oracle): the rows of findInterval(w), every row's LF walk to '$', ordinal =
    Occ('$', that row) - 1, the head ordinals from meta_reference.OracleSide.lookup of the pairs, the values from
    meta_reference.build_tables, the records cut and tallied with numpy;
  * with no BWT at all (counts_plain): for every shard the distinct read strings r with w in r that a searchable pair
    names, the value from a dict in which later pairs overwrite, the records tallied in plain Python; rows, head rows and
    LF steps from str.find over the read lists (an occurrence at offset j of a read is one row, j LF steps from its '$').

Both give {strings, copies, matches, carriers, work} with work = the six numbers of rsbwt_set_sample_last_work.

The pair generator (sample_pairs) makes values that ARE records: codes drawn from a universe of samples plus a few codes
outside it, c and l bytes 33 + small numbers with some c bytes below 33 (a negative c), record counts on LADDER (which
straddles the kernel's lane / wave split of 16 records and 1 KiB), some values ending in 1 .. R - 1 stray bytes, one value
listing a code twice; pairs are left out for every ninth read and two strings are given twice, as meta_reference.pairs_for
does."""
import hashlib

import numpy as np

import meta_reference as MR

SPLIT = 16  # records a lane parses by itself (csrc/sample_counts.hip, TALLY_LANE_RECORDS)
LADDER = [0, 1, 2, SPLIT - 1, SPLIT, SPLIT + 1, 300, 2000]
# how often each rung is drawn (of 40): the long values are rare, so that a test stays quick
_DRAW = [0, 1, 2, SPLIT - 1, SPLIT, SPLIT + 1] * 6 + [1, 2, 300, 2000]


def rec_size(size_of_sample, has_other):
    return size_of_sample + (2 if has_other else 0)


def universe(size_of_sample, n=70, seed="samples"):
    """n distinct codes of size_of_sample bytes (any byte values, above 0x7F too: codes compare as unsigned bytes), and 4
    more that stand outside every dictionary made from it: (codes, outside)"""
    n = min(n, 180) if size_of_sample == 1 else n
    seen, i = [], 0
    while len(seen) < n + 4:
        c = hashlib.sha256(f"{seed}/{size_of_sample}/{i}".encode()).digest()[:size_of_sample]
        i += 1
        if c not in seen:
            seen.append(c)
    return seen[:n], seen[n:]


def _stream(h, n):
    out, i = b"", 0
    while len(out) < n:
        out += hashlib.sha256(h + i.to_bytes(4, "little")).digest()
        i += 1
    return out[:n]


def value_of(read, codes, outside, size_of_sample, has_other, tag=0):
    """the records of a read, a deterministic function of the string: (value bytes, number of whole records)"""
    h = hashlib.sha256(f"rec/{tag}/{read}".encode()).digest()
    n = _DRAW[int.from_bytes(h[:4], "little") % len(_DRAW)]
    s = _stream(h, 4 * n + 8)
    out = bytearray()
    for i in range(n):
        a, b, c, d = s[4 * i:4 * i + 4]
        code = outside[a % len(outside)] if b % 11 == 0 else codes[(a | (b << 8)) % len(codes)]
        out += code
        if has_other:
            cb = 33 + c % 6 if c % 7 else 33 - 1 - c % 5  # (c % 7 == 0: a byte below 33, a negative c)
            out += bytes([cb, 33 + d % 40])
    R = rec_size(size_of_sample, has_other)
    if R > 1 and s[4 * n] % 4 == 0:  # a stray tail of 1 .. R - 1 bytes
        out += s[4 * n + 1:4 * n + 2] * (1 + s[4 * n + 2] % (R - 1))
    return bytes(out), n


def sample_pairs(shards, codes, outside, size_of_sample, has_other, every=9, seed="sample"):
    """meta_reference.pairs_for with record values.  Returns (pairs, info); info: left_out, twice, nothing, with_n, doubled
    (the read whose value lists its first code twice)"""
    distinct = sorted({r for sh in shards for r in sh})
    order = sorted(distinct, key=lambda r: hashlib.sha256(f"{seed}/{r}".encode()).digest())
    left_out = set(order[every - 1::every])
    kept = [r for r in order if r not in left_out]
    val = lambda r, tag=0: value_of(r, codes, outside, size_of_sample, has_other, tag)[0]  # noqa: E731
    R = rec_size(size_of_sample, has_other)
    doubled = next(r for r in kept if 2 <= len(val(r)) // R <= SPLIT - 2)
    pairs = [(r, val(r) if r != doubled else val(r)[:R] * 2 + val(r)[R:]) for r in kept]
    differs = [r for r in kept if val(r, 1) != val(r) and r != doubled]
    twice = [differs[3], differs[len(differs) // 2]]
    pairs += [(r, val(r, 1)) for r in twice]
    longest = max(distinct, key=len)
    nothing = [w for w in (longest[:len(longest) - 1], longest[1:], "ACGT" * 10 + "TTTTT") if w not in set(distinct)]
    with_n = kept[0][:5] + "N" + kept[0][6:]
    pairs += [(w, val(w)) for w in nothing] + [(with_n, val(with_n)), ("", b"empty-string")]
    return pairs, dict(left_out=left_out, twice=twice, nothing=nothing, with_n=with_n, doubled=doubled)


def key_of(code):
    return int.from_bytes(code, "big")


# ---- over the oracle ------------------------------------------------------------------------------------------------

class OracleShards:
    """what counts_oracle asks of a fixture's shards: built once per fixture and pair list, shared by the tests"""

    def __init__(self, oracle, shards, runs, pairs):
        from kmer_reference import Walks
        self.sides = [MR.OracleSide(oracle.from_runs(r, len(sh)), len(sh)) for sh, r in zip(shards, runs)]
        self.walks = [Walks(s.oix) for s in self.sides]
        self.rebuild(pairs)
        self._rows = {}

    def rebuild(self, pairs):
        self.tables, self.stats = MR.build_tables(self.sides, pairs)
        self.heads = [set() for _ in self.sides]
        for w, _ in pairs:
            for p, s in enumerate(self.sides):
                o, c, _ = s.lookup(w)
                if c > 0:
                    self.heads[p].add(o)
        self._parsed = {}

    def rows(self, p, w):
        """[(ordinal, LF steps)] of the rows of findInterval(w) in shard p"""
        if (p, w) not in self._rows:
            out = []
            if MR.searchable(w):
                oix = self.sides[p].oix
                lo, up = oix.find_interval(w)
                if lo <= up < oix.bwlen():
                    for row in range(lo, up + 1):
                        walk = self.walks[p].rows(row)
                        out.append((oix.occ("$", walk[-1]) - 1, len(walk) - 1))
            self._rows[(p, w)] = out
        return self._rows[(p, w)]


def counts_oracle(osh, queries, codes, size_of_sample, has_other, max_rows=0):
    C, R = len(codes), rec_size(size_of_sample, has_other)
    keys = np.array([key_of(c) for c in codes], np.uint64)
    by_key = np.argsort(keys)
    skeys = keys[by_key]
    Q = len(queries)
    strings, copies = np.zeros((Q, C + 1), np.uint32), np.zeros((Q, C + 1), np.int64)
    matches, carriers = np.zeros(Q, np.uint64), np.zeros(Q, np.uint64)
    work = dict(rows=0, head_rows=0, carriers=0, records=0, unknown=0, lf_steps=0)
    parsed = {}

    def parse(value):
        if value not in parsed:
            n = len(value) // R
            a = np.frombuffer(value[:n * R], np.uint8).reshape(n, R)
            k = np.zeros(n, np.uint64)
            for b in range(size_of_sample):
                k = (k << np.uint64(8)) | a[:, b].astype(np.uint64)
            at = np.searchsorted(skeys, k)
            hit = (at < C) & (skeys[np.minimum(at, C - 1)] == k)
            col = np.where(hit, by_key[np.minimum(at, C - 1)], C)
            c = a[:, size_of_sample].astype(np.int8).astype(np.int64) - 33 if has_other else np.ones(n, np.int64)
            parsed[value] = (np.bincount(col, minlength=C + 1).astype(np.uint32),
                             np.bincount(col, weights=c, minlength=C + 1).astype(np.int64), n, int((col == C).sum()))
        return parsed[value]

    for q, w in enumerate(queries):
        per = [osh.rows(p, w) for p in range(len(osh.sides))]
        matches[q] = sum(len(r) for r in per)
        if max_rows and int(matches[q]) > max_rows:
            continue
        for p, rows in enumerate(per):
            work["rows"] += len(rows)
            work["lf_steps"] += sum(st for _, st in rows)
            on_head = [o for o, _ in rows if o in osh.heads[p]]
            work["head_rows"] += len(on_head)
            for o in sorted(set(on_head)):
                s, c, n, unk = parse(osh.tables[p][o])
                strings[q] += s
                copies[q] += c
                carriers[q] += 1
                work["carriers"] += 1
                work["records"] += n
                work["unknown"] += unk
    return dict(strings=strings, copies=copies, matches=matches, carriers=carriers, work=work)


# ---- with no BWT ----------------------------------------------------------------------------------------------------

def _offsets(r, w):
    out, j = [], r.find(w)
    while j >= 0:
        out.append(j)
        j = r.find(w, j + 1)
    return out


def counts_plain(shards, pairs, queries, codes, size_of_sample, has_other, max_rows=0):
    C, R = len(codes), rec_size(size_of_sample, has_other)
    column = {c: i for i, c in enumerate(codes)}
    named = {}
    for read, value in pairs:
        if MR.searchable(read):
            named[read] = value  # a later pair overwrites
    Q = len(queries)
    strings, copies = [[0] * (C + 1) for _ in range(Q)], [[0] * (C + 1) for _ in range(Q)]
    matches, carriers = [0] * Q, [0] * Q
    work = dict(rows=0, head_rows=0, carriers=0, records=0, unknown=0, lf_steps=0)
    for q, w in enumerate(queries):
        if not MR.searchable(w):
            continue
        occ = [{r: _offsets(r, w) for r in set(sh) if w in r} for sh in shards]
        mult = [{r: sh.count(r) for r in o} for sh, o in zip(shards, occ)]
        matches[q] = sum(len(js) * m[r] for o, m in zip(occ, mult) for r, js in o.items())
        if max_rows and matches[q] > max_rows:
            continue
        for o, m in zip(occ, mult):
            for r, js in o.items():
                work["rows"] += len(js) * m[r]
                work["lf_steps"] += sum(js) * m[r]
                if r not in named:
                    continue
                work["head_rows"] += len(js)
                work["carriers"] += 1
                carriers[q] += 1
                value = named[r]
                for i in range(len(value) // R):
                    rec = value[i * R:(i + 1) * R]
                    col = column.get(rec[:size_of_sample], C)
                    b = rec[size_of_sample] if has_other else 34
                    strings[q][col] += 1
                    copies[q][col] += (b - 256 if b > 127 else b) - 33
                    work["records"] += 1
                    work["unknown"] += col == C
    return dict(strings=np.array(strings, np.uint32).reshape(Q, C + 1), copies=np.array(copies, np.int64).reshape(Q, C + 1),
                matches=np.array(matches, np.uint64), carriers=np.array(carriers, np.uint64), work=work)


def same(a, b):
    """the first difference between two answers, or None"""
    for k in ("matches", "carriers", "strings", "copies"):
        if a[k].shape != b[k].shape or a[k].dtype != b[k].dtype or not (a[k] == b[k]).all():
            return k, np.argwhere(a[k] != b[k])[:5].tolist() if a[k].shape == b[k].shape else (a[k].shape, b[k].shape)
    return ("work", a["work"], b["work"]) if a["work"] != b["work"] else None


def queries_for(shards, seed="sq"):
    """what the tests ask: substrings of reads of length 1, 4, 8 and 12, whole reads, a read plus one symbol, strings with an
    N, the empty string, an absent 12-mer, and (where the fixture has it) a query a read holds many times"""
    distinct = sorted({r for sh in shards for r in sh})
    order = sorted(distinct, key=lambda r: hashlib.sha256(f"{seed}/{r}".encode()).digest())
    out = ["A", "C"]
    for i, r in enumerate(order[:24]):
        ln = (4, 8, 12)[i % 3]
        at = (7 * i) % (len(r) - ln + 1)
        out.append(r[at:at + ln])
    out += order[24:36] + [order[36] + "A", order[37][:6] + "N" + order[37][7:], "N", "", "ACGTTGCAAGGT"[::-1] * 1 + "ACGTAC"]
    # the strings held 2 or more times in one shard, and those in more than one shard
    for sh in shards:
        many = [r for r in set(sh) if sh.count(r) >= 2]
        out += sorted(many, key=lambda r: -sh.count(r))[:2]
    both = sorted(set.intersection(*[set(sh) for sh in shards])) if len(shards) > 1 else []
    out += both[:2]
    if any("A" * 45 in r for sh in shards for r in sh):
        out += ["AAAA", "ACAC"]
    else:
        out += [order[40][3:7]]
    return out
