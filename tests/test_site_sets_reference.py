"""CPU guards for tests/test_gpu_site_sets.py: what the read sets, dealings and requests of tests/site_sets_reference.py
reach, shown with the restatement alone (tests/site_reference.py) before anything runs on a GPU.  These are conditions on
the inputs: where one fails, the seeds or the sites move, not the assertion."""
from collections import Counter

import pytest

import gt_reference as G
import ksw_reference as kr
import meta_reference as MR
import site_reference as SITE
import site_sets_reference as SS

CASES = [(name, dealing) for name, ds in SS.DEALINGS.items() for dealing in ds]


@pytest.mark.parametrize("name,dealing", CASES, ids=[f"{a}-{b}" for a, b in CASES])
def test_by_head_ordinal_means_by_string(oracle, name, dealing):
    """the restatement by head ordinal and its statement by string agree on all four outputs and the work numbers they
    share, on every input, dealing and parameter set; every set has carriers"""
    r = SS.get(oracle, name, dealing)
    for M, k, skip in SS.PARAMS[name]:
        a = SITE.counts_by_ordinal(r.side, r.reqs, k, skip, M, r.codes, r.ss, r.other)
        b = SITE.counts_by_string(r.side, r.reqs, k, skip, M, r.codes, r.ss, r.other)
        assert SITE.same(a, b) is None, (M, k, skip, SITE.same(a, b))
        assert a["work"]["aligned"] > a["work"]["carriers"] > 0


def _classes(items):
    """per item of rows_by_ordinal: how its kept rows fare"""
    hit = Counter()
    for _, (s, rows) in items.items():
        fails = any(p and not st for p, st in rows)
        stays = any(st for _, st in rows)
        hit["pending only, one fails and one stays"] += all(p for p, _ in rows) and fails and stays
        hit["a pending row fails beside a row that is not pending"] += fails and any(not p for p, _ in rows)
        hit["dropped by the length rule alone"] += not stays
        hit["a read under 38 symbols"] += len(s) < 38
    return hit


def test_ragged_alleles_reach_the_length_rule_on_reads_of_many_lengths(oracle):
    """over the parameter sets, on one shard: the four classes of the needed-length rule, and items of at least eight
    different lengths over 256 symbols that pass it, some kept and some not kept by the alignment"""
    ra = SS.ragged_alleles()
    r = SS.get(oracle, "ragged-alleles", "one")
    g = ra.genome
    # the read set: the three sites the issue names, nested reads, duplicates
    at = lambda s: g.find(s)  # noqa: E731
    covering = lambda i: [s for s in set(ra.reads) if 0 <= at(s) <= i < at(s) + len(s)]  # noqa: E731
    assert sum(1 for s in ra.longs if at(s) <= ra.long_site < at(s) + len(s)) >= 2
    assert covering(ra.short_site) and all(len(s) < SS.WIDE for s in covering(ra.short_site))
    assert any(len(s) < 38 for s in covering(ra.tiny_site))
    assert len(ra.reads) - len(set(ra.reads)) >= 5 and min(len(s) for s in ra.reads) == 12
    assert sum(1 for w, _, _, _ in ra.reqs if len(w) > 100) <= 4 and max(len(w) for w, _, _, _ in ra.reqs) == 600
    hit, lens = Counter(), {}
    for M, k, skip in SS.PARAMS["ragged-alleles"]:
        work, items = SITE.rows_by_ordinal(r.side, r.reqs, k, skip, M)
        hit.update(_classes(items))
        for (q, _, _), (s, rows) in items.items():
            if len(s) > SS.WIDE and any(st for _, st in rows):
                lens.setdefault(len(s), set()).add(SITE.keeps(s, *r.reqs[q]))
    assert len(hit) == 4 and all(hit.values()), dict(hit)
    assert len(lens) >= 8 and sum(1 for v in lens.values() if True in v) >= 4 and any(False in v for v in lens.values()), lens
    assert (0, 12, 3) in SS.PARAMS["ragged-alleles"] and any(M > 0 for M, _, _ in SS.PARAMS["ragged-alleles"])


def test_ragged_alleles_reach_every_exit_of_the_alignment(oracle):
    """every exit of align_gt_read that ksw_reference.verdicts() reaches is reached by a candidate with a pair against a
    request with a window of 79, too (no exit is unreachable here: the list of exceptions is empty)"""
    ra = SS.ragged_alleles()
    r = SS.get(oracle, "ragged-alleles", "one")
    named = {w for w, _ in r.pairs if MR.searchable(w)}
    seen = set()
    for M, k, skip in SS.PARAMS["ragged-alleles"]:
        exp = r.side.expected(r.reqs, k, skip, M)
        for q in range(ra.narrow):
            assert len(r.reqs[q][0]) == 79
            seen |= {kr.align_gt_read(s, *r.reqs[q]) for _, s in exp[q][0][1] if s in named}
    unreachable = set()
    assert seen | unreachable >= set(kr.verdicts()[4]), sorted(set(kr.verdicts()[4]) - seen)


def test_the_dealing_over_four_has_the_shards_the_wide_extraction_needs(oracle):
    """shards 1 and 3 have reads over 256 symbols, shards 0 and 2 none; shard 2 has no candidate row at all; shard 0 has
    kept rows and not one on a head ordinal; the shards extract different numbers of reads"""
    r = SS.get(oracle, "ragged-alleles", "wide4")
    wide = [sum(len(s) > SS.WIDE for s in sh) for sh in r.shards]
    assert wide[1] > 0 and wide[3] > 0 and wide[0] == wide[2] == 0, wide
    named = {w for w, _ in r.pairs if MR.searchable(w)}
    assert not named & set(r.shards[0]) and len(named & set(r.shards[2])) > 20
    for M, k, skip in SS.PARAMS["ragged-alleles"]:
        exp = r.side.expected(r.reqs, k, skip, M)
        cand = [sum((up - lo + 1) & G.U64 for q in range(len(r.reqs)) for _, _, _, _, lo, up in exp[q][p][0]) for p in range(4)]
        assert cand[2] == 0 and min(cand[0], cand[1], cand[3]) > 0, cand
        assert sum(len(exp[q][0][1]) for q in range(len(r.reqs))) > 0  # shard 0: rows the filter keeps, reads it would return
        work, items = SITE.rows_by_ordinal(r.side, r.reqs, k, skip, M)
        extracted = Counter(p for p, _ in {(p, o) for _, p, o in items})
        assert set(extracted) == {1, 3} and extracted[1] != extracted[3], extracted
        # the second extraction has reads in both of them
        assert all(any(len(s) > SS.WIDE for (_, p, _), (s, _) in items.items() if p == x) for x in (1, 3))
    # round-robin over 8: every shard takes part
    r8 = SS.get(oracle, "ragged-alleles", "rr8")
    _, items = SITE.rows_by_ordinal(r8.side, r8.reqs, 12, 3, 0)
    assert {p for _, p, _ in items} == set(range(8))


def test_repeat_reaches_many_rows_on_one_entry(oracle):
    """an entry reached through 16 kept rows or more; a request with head and non-head copies of one string among its kept
    rows; a leg wider than a positive M that is dropped for it (its lengthening runs off the window)"""
    rp = SS.repeat()
    r = SS.get(oracle, "repeat", "one")
    reads = r.shards[0]
    most, copies = 0, False
    for M, k, skip in SS.PARAMS["repeat"]:
        work, items = SITE.rows_by_ordinal(r.side, r.reqs, k, skip, M)
        most = max(most, max(len(rows) for _, rows in items.values()))
        # kept rows count every copy, head rows one of them: an item whose string the shard holds twice has both
        copies |= work["kept"] > work["head_rows"] and any(reads.count(s) > 1 for s, _ in items.values())
        c = Counter()
        qs = [(w, pos) for w, pos, _, _ in r.reqs]
        G.expected(r.side.gt, ("site", r.side.name, tuple(qs)), qs, k, skip, M, c)  # (Side.expected's key: computed once)
        if M > 0:
            assert c["left.leg1"] + c["right.leg1"] + c["cover.leg1"] > 0 and c["noleg.end>L"] + c["noleg.start<1"] > 0, dict(c)
    assert most >= 16 and copies, (most, copies)
    assert any(M == 0 for M, _, _ in SS.PARAMS["repeat"]) and len(rp.alleles) == 2


def test_the_read_of_4096_symbols_is_a_candidate_and_a_carrier(oracle):
    """exactly 4,096 symbols, on a head ordinal, a candidate of the requests with the window of 79 it contains (hanging
    4,017 symbols out of it, it is not kept there: align_gt_read's exit 4) and a carrier of the request whose window is its
    own 4,096 symbols; without it the other reads' answers are the same"""
    ex = SS.exact4096()
    a, b = SS.get(oracle, "exact4096", "with"), SS.get(oracle, "exact4096", "without")
    assert len(ex.big) == 4096 and ex.reqs[0][0] in ex.big and len(ex.reqs[2][0]) == 4096
    o, c, _ = a.side.osh.sides[1].lookup(ex.big)
    assert c == 1 and o in a.side.osh.heads[1]
    assert kr.align_gt_read(ex.big, *ex.reqs[0]) == 4 and SITE.keeps(ex.big, *ex.reqs[2])
    for M, k, skip in SS.PARAMS["exact4096"]:
        wa, wb = a.want(M, k, skip), b.want(M, k, skip)
        _, items = SITE.rows_by_ordinal(a.side, a.reqs, k, skip, M)
        assert all((q, 1, o) in items for q in range(3))
        assert (wa["aligned"] == wb["aligned"] + 1).all() and list(wa["carriers"] - wb["carriers"]) == [0, 0, 1]
        assert wa["work"]["extracted"] == wb["work"]["extracted"] + 1
