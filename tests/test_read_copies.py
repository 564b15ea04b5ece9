"""CPU suite for whole-read matches by backward search from the terminator rows (csrc/read_lookup.hip, rsbwt_read_copies).

The definition the GPU path implements, stated here in plain Python on the oracle's pc / occ:

    step w, right to left, from the rows [0, C['A'] - 1] (the suffixes that begin with a terminator);
    copies = Occ('$', upper) - Occ('$', lower - 1), ending = upper - lower + 1 -- zeros for anything else.

It is held to two expectations that come from the read lists alone -- collections.Counter(reads)[w] and the number of reads
that end with w -- for every distinct read of the three seeded fixtures of tests/test_kmer_fixtures.py and for the
seeded non-read sample the GPU module (tests/test_gpu_read_copies.py) asks: that module's expected values are the read
lists', not the code under test's.  The query lists and the definition are built here and imported there."""
import collections
import ctypes as C
import os
import random
import re

import numpy as np
import pytest

import test_kmer_fixtures as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["rsbwt_read_copies", "rsbwt_read_copies_dev", "rsbwt_set_read_copies_var", "rsbwt_exactmatch_by_search",
       "rsbwt_exactmatch_is_by_search", "rsbwt_set_exactmatch_by_search"]
M64 = (1 << 64) - 1


def definition(oix, w):
    """(copies, ending, lower, upper) of w on the oracle index: lower / upper None when nothing is ranked"""
    n, na = oix.bwlen(), oix.pc("A")
    if not w or set(w) - set("ACGT") or len(w) > 65535 or na == 0:
        return 0, 0, None, None
    lo, up = 0, na - 1
    for ch in reversed(w):  # updateInterval, src/bwt/query.cpp:11-15
        c = oix.pc(ch)
        lo, up = c + (oix.occ(ch, lo - 1) if lo else 0), (c + oix.occ(ch, up) - 1) & M64
        if lo > up:
            return 0, 0, None, None
    if up >= n:
        return 0, 0, None, None
    return oix.occ("$", up) - (oix.occ("$", lo - 1) if lo else 0), up - lo + 1, lo, up


def from_reads(reads, qs):
    """the same two numbers from the read list alone"""
    cnt = collections.Counter(reads)
    suf = collections.Counter(r[i:] for r in reads for i in range(len(r)))
    ok = [bool(w) and not (set(w) - set("ACGT")) for w in qs]
    return [cnt.get(w, 0) if o else 0 for w, o in zip(qs, ok)], [suf.get(w, 0) if o else 0 for w, o in zip(qs, ok)]


def queries(name):
    """(reads, non-reads) the GPU module asks of fixture `name`: every distinct read of every shard; and a seeded sample of
    strings that are mostly not reads -- proper suffixes (three of every read: each ends reads, so each ranks two positions),
    proper prefixes, interior substrings, reads with one base changed, strings with an N, the empty string and a string
    longer than any read"""
    fx = F.fixture(name)
    rng = random.Random(f"read_copies/{name}")
    reads = sorted({r for sh in fx.shards for r in sh})
    out = []
    for r in reads:
        for _ in range(3):
            out.append(r[rng.randrange(1, len(r)):])
    for r in rng.sample(reads, min(200, len(reads))):
        out.append(r[:rng.randrange(1, len(r))])
        a = rng.randrange(1, len(r) - 1)
        out.append(r[a:rng.randrange(a + 1, len(r))])
        i = rng.randrange(len(r))
        out.append(r[:i] + rng.choice([c for c in "ACGT" if c != r[i]]) + r[i + 1:])
        out.append(r[:i] + "N" + r[i + 1:])
    out += ["", "N", "".join(rng.choice("ACGT") for _ in range(max(map(len, reads)) + 50))]
    return reads, out


def all_suffixes(name):
    """every proper suffix of every read of the fixture: between them their end positions are nearly every row outside the
    terminator block -- what the GPU module adds on the layouts with continuations, so that the few symbols a spill chunk
    holds are among the ranked positions"""
    fx = F.fixture(name)
    return sorted({r[i:] for sh in fx.shards for r in sh for i in range(1, len(r))})


# a layout of this module's own: the one span of `ragged` at which spill CHUNKS hold end positions of w$ (below: at the
# matrix's own chunk span, 128, no query at all has one there)
EXTRA_LAYOUTS = [("ragged", "chunk+", 150, True, 6)]
EXTRA_STATS = {("ragged", 0, 150, True): [150, 377, 3, 7, 3, 319]}


def spilled_tails(rsb, runs, span, room):
    """{window: first spilled position}: the symbols a window's own line does not hold are its LAST ones (the pieces past
    the line's own, line_format.h build_group), and a window is laid out from the symbols up to its end alone -- so the
    builder's `spilled symbols` of the run stream cut at the end of window w, less that of the stream cut one window earlier,
    is how many of w's symbols sit in its spill chunk / far lines"""
    lens = (runs & 31).astype(np.int64)
    cum = np.cumsum(lens)
    n = int(cum[-1])
    out, prev = {}, 0
    for end in range(span, n + span, span):
        end = min(end, n)
        j = int(np.searchsorted(cum, end, side="right"))
        cut = runs[:j]
        rest = end - (int(cum[j - 1]) if j else 0)
        if rest:
            cut = np.append(cut, np.uint8((runs[j] & 0xE0) | rest))
        sp = F.selftest(rsb, np.ascontiguousarray(cut), span, room)[5]
        if sp > prev:
            out[(end - 1) // span] = end - (sp - prev)
        prev = sp
    return out


def expected_counters(oix, tails, span, qs):
    """what the '$' count's counting-mode words must say for these queries on this layout: (results ranked, positions that
    took a continuation, results that needed a second line) -- csrc/read_lookup.hip: `upper` is ranked off its window's
    line; `lower - 1` off the same line when it lies in that window, from the header when it is the last position of the
    window before, else from a second line"""
    ranked = conts = second = 0
    for w in qs:
        _, _, lo, up = definition(oix, w)
        if up is None:
            continue
        ranked += 1
        win = up // span
        first = tails.get(win)
        conts += first is not None and up >= first
        if lo:
            if (lo - 1) // span == win:
                conts += first is not None and lo - 1 >= first
            elif lo != win * span:
                second += 1
    return ranked, conts, second


def end_positions(oix, qs):
    """the positions the '$' count ranks for these queries: upper and lower - 1 of every non-empty result"""
    pos = set()
    for w in qs:
        _, _, lo, up = definition(oix, w)
        if up is not None:
            pos.add(up)
            if lo:
                pos.add(lo - 1)
    return pos


# ---- the boundary ---------------------------------------------------------------------------------------------------

def test_header_declares_and_native_binds_the_six(rsb):
    from readserver_amd import _native
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rsbwt.h")).read(), flags=re.S)
    L = C.CDLL(rsb.lib_path())
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, txt), f"{n} is not declared in include/rsbwt.h"
        assert n in _native.SIGNATURES and hasattr(L, n)
    assert callable(rsb.read_copies) and hasattr(rsb.ShardSet, "read_copies_var") and hasattr(rsb.ShardSet, "exactmatch_by_search")
    assert isinstance(rsb.GpuBWT.exactmatch_by_search, property)


def test_null_arguments_and_no_gpu(rsb):
    """null handles / sets are RSBWT_EINVAL (as rsbwt_find_intervals says it), a switch on no handle reads as off, and a
    box without GPU cannot get as far as a handle: RSBWT_ENODEV, no CPU fallback"""
    L = rsb.lib()
    out = np.zeros(4, np.uint64)
    km = np.frombuffer(b"ACGTACGT", np.uint8).copy()
    off = np.array([0, 4, 8], np.uint64)
    EINVAL = -1
    assert L.rsbwt_strerror(EINVAL) and L.rsbwt_read_copies(None, km.ctypes.data, 2, 4, 4, out.ctypes.data, None) == EINVAL
    assert b"null" in L.rsbwt_last_error()
    assert L.rsbwt_read_copies_dev(None, km.ctypes.data, km.ctypes.data, 2, 4, out.ctypes.data, None, None) == EINVAL
    assert L.rsbwt_set_read_copies_var(None, km.ctypes.data, off.ctypes.data, 2, out.ctypes.data, None) == EINVAL
    assert L.rsbwt_exactmatch_by_search(None, 1) == EINVAL
    assert L.rsbwt_set_exactmatch_by_search(None, 1) == EINVAL
    assert L.rsbwt_exactmatch_is_by_search(None) == 0
    if L.rsbwt_device_count() == 0:
        runs = np.array([(0 << 5) | 1, (1 << 5) | 3], np.uint8)
        with pytest.raises(rsb.RsbwtError) as e:
            with rsb.GpuBWT(runs=runs, num_strings=1) as g:
                rsb.read_copies(g, ["A"])
        assert e.value.code == -5 and "no CPU fallback" in str(e.value)


# ---- the definition against the read lists ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["pop", "repeat", "ragged"])
def test_definition_equals_the_read_lists(oracle, name):
    fx = F.fixture(name)
    reads, others = queries(name)
    seen_dup = seen_suffix = 0
    for sh, runs in zip(fx.shards, fx.runs()):
        oix = oracle.from_runs(runs, len(sh))
        assert oix.pc("A") == len(sh)  # the terminator rows are the first num_strings rows
        qs = reads + others
        want_c, want_e = from_reads(sh, qs)
        cnt = collections.Counter(sh)
        for w, wc, we in zip(qs, want_c, want_e):
            c, e, _, _ = definition(oix, w)
            assert (c, e) == (wc, we), (name, w[:30], len(w))
            seen_suffix += e > c
        for w in reads:  # every distinct read, the two expectations spelled out
            c, e, _, _ = definition(oix, w)
            assert c == cnt[w] and e == sum(1 for r in sh if r.endswith(w))
            seen_dup += c > 1
    assert seen_suffix > 0
    if name == "repeat":
        assert seen_dup >= 50  # exact duplicates: copies > 1
    nonreads = [w for w in others if all(w not in set(sh) for sh in fx.shards)]
    assert len(nonreads) > len(others) // 2 and "" in others and any("N" in w for w in others)


_CONT = sorted({(fx, kind, span, room) for fx, kind, span, room, _ in F.LAYOUTS + EXTRA_LAYOUTS if span and kind != "control"})
NONE_POSSIBLE = ("ragged", 128, True)  # shown below: no query has an end position in this layout's continuations


@pytest.mark.parametrize("name,kind,span,room", _CONT, ids=[f"{a}-{b}-S{c}-{'reads' if d else 'plain'}" for a, b, c, d in _CONT])
def test_ranked_positions_take_continuations(rsb, oracle, name, kind, span, room):
    """On every layout with continuations the positions the '$' count ranks (upper and lower - 1 of w$, for the GPU module's
    queries) include symbols that sit in a spill chunk / far line -- computed from the builder's own statistics of cut run
    streams (spilled_tails) and the oracle's intervals: the number the GPU module then asserts the kernel's counter against,
    exactly.  At window level the same is shown by counting, as tests/test_kmer_fixtures.py shows it for candidate rows: a
    group of W windows, K of them of the kind and V of them holding a ranked position, with V + K > W, holds one.
    One layout has none: `ragged` at span 128 -- there NO string at all has an end position on a spilled symbol (every
    string with a non-empty answer is a read or a proper suffix of one: all of them are tried), which is why this module
    adds span 150 (EXTRA_LAYOUTS), where spill chunks do hold end positions."""
    fx = F.fixture(name)
    reads, others = queries(name)
    proven = conts = 0
    for p, (sh, runs) in enumerate(zip(fx.shards, fx.runs())):
        st = F.selftest(rsb, runs, span, room)
        assert st == {**F.LAYOUT_STATS, **EXTRA_STATS}[(name, p, span, room)]
        F.assert_kind(kind, st)
        groups = F.group_kinds(rsb, runs, span, room, st)
        oix = oracle.from_runs(runs, len(sh))
        seen = collections.Counter()
        for w in {r // span for r in end_positions(oix, reads + others)}:
            seen[w // F.GROUP] += 1
        proven += sum(1 for g, (W, chunkw, farw) in enumerate(groups) if seen[g] + (chunkw if kind.startswith("chunk") else farw) > W)
        tails = spilled_tails(rsb, runs, span, room)
        assert sum(min((w + 1) * span, oix.bwlen()) - first for w, first in tails.items()) == st[5]  # the tails are the builder's spilled symbols
        if (name, span, room) == NONE_POSSIBLE:
            assert expected_counters(oix, tails, span, reads + others + all_suffixes(name))[1] == 0
        else:
            conts += expected_counters(oix, tails, span, reads + others)[1]
    assert proven > 0, (name, kind, span)
    assert (conts > 0) == ((name, span, room) != NONE_POSSIBLE), (name, kind, span, conts)
