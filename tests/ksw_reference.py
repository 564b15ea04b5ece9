"""The alignment reference the ksw tests share -- TEST INFRASTRUCTURE.  ksw_align of the reference's src/service/ksw.c
(the 16-bit striped path ksw_i16 with KSW_XSTART, :223-352) restated as the scalar dynamic programme it computes, and
align_gt_read (src/service/service.cpp:105-225) branch by branch over it, every exit counted under its RSBWT_GT_* code.

One pass P(q, t, endsc) over columns i = 0..tlen-1 and rows j = 0..qlen-1, all values >= 0, borders 0:

    H[i][j]   = max(0, H[i-1][j-1] + s(t[i], q[j]), E[i][j], F[i][j])
    E[i+1][j] = max(E[i][j] - gape, H[i][j] - (gapo + gape))         (subtractions floored at 0, :265-270)
    F[i][j+1] = max(F[i][j] - gape, H[i][j] - (gapo + gape))

te is the last column whose maximum rose above every earlier one (:295-296); the pass stops after the column at which that
maximum reaches endsc (:299); qe is the row of the maximum in column te, ties to the smallest (j mod slen, j div slen) with
slen = (qlen + 7) / 8 -- the order :307-308 scans the striped vectors in.  Nothing scores: score 0, te -1, qe 0.

pass_scalar is that definition cell by cell.  pass_np is the same column at a time: F[i][j+1] = max(0, max over k <= j
of H^[k] - gapoe - (j - k) gape) with H^ = H without its F term (an H that came from F cannot open a better gap:
F - gapoe < F - gape), one running maximum.  tests/test_ksw_reference.py holds both to the recorded outputs."""
from collections import Counter

import numpy as np

NO_STOP = 0x10000
SERVICE = (1, 4, 1, 6, 1)   # match, mismatch, ambiguous, gapo, gape: service.cpp:108-114 and :84
OTHER = (2, 3, 1, 5, 2)
_NT4 = np.full(256, 4, np.int64)
for _i, _c in enumerate("ACGT"):
    _NT4[ord(_c)] = _NT4[ord(_c.lower())] = _i

GT_LABELS = {1: "alt: ra.score >= r.score (:138)", 2: "ref: r.score < ra.score (:143)", 3: "site outside [tb, te] (:150)",
             4: "more than 4 read bases unaligned (:158)", 5: "score floor, no indel (:166)", 6: "score floor, insertion (:173)",
             7: "score floor, deletion (:180)", 8: "mismatch at the site (:190)", 9: "KEEP, no indel",
             10: "right sub-alignment, qb != 0 (:205)", 11: "KEEP, right sub-alignment", 12: "left sub-alignment, qe + 1 != len (:218)",
             13: "KEEP, left sub-alignment"}
GT_KEEP = (9, 11, 13)


def load_golden(golden_dir):
    """tests/golden/ksw_v1.npz: (pairs of (query, target) bytes, [(params, int32 [n][5] score te qe tb qb)] for the service's
    scores and for OTHER, the class names, a bit mask of classes per pair)"""
    import os
    z = np.load(os.path.join(golden_dir, "ksw_v1.npz"))
    qt, tt, qo, to = z["qtext"].tobytes(), z["ttext"].tobytes(), z["qoff"], z["toff"]
    pairs = [(qt[int(qo[i]):int(qo[i + 1])], tt[int(to[i]):int(to[i + 1])]) for i in range(len(qo) - 1)]
    sets = [(tuple(int(x) for x in z["params_service"]), z["service"]), (tuple(int(x) for x in z["params_other"]), z["other"])]
    return pairs, sets, [str(c) for c in z["classes"]], z["mask"]


def code(s):
    """seq_nt4_table: ACGTacgt -> 0..3, anything else 4"""
    if isinstance(s, str):
        s = s.encode("latin-1")
    return _NT4[np.frombuffer(bytes(s), np.uint8)]


def _matrix(params):
    a, b, n = params[0], params[1], params[2]
    m = np.full((5, 5), -n, np.int64)
    for i in range(4):
        for j in range(4):
            m[i, j] = a if i == j else -b
    return m


def _order(qlen):
    """rank of every row in the scan order of :307-308"""
    slen = (qlen + 7) // 8
    j = np.arange(qlen)
    return (j % slen) * 8 + j // slen


def pass_scalar(q, t, params, endsc=NO_STOP, tie="striped"):
    mat, gapoe, gape = _matrix(params), params[3] + params[4], params[4]
    qlen, slen = len(q), (len(q) + 7) // 8
    H, E = [0] * qlen, [0] * qlen
    gmax, te, qe = 0, -1, 0
    for i in range(len(t)):
        f = diag = imax = 0
        best = None
        for j in range(qlen):
            up = H[j]
            h = max(0, diag + int(mat[t[i], q[j]]), E[j], f)
            key = (j % slen, j // slen) if tie == "striped" else (j,)
            if h > imax or (h == imax and (best is None or key < best[0])):
                imax, best = h, (key, j)
            g = max(h - gapoe, 0)
            E[j] = max(E[j] - gape, g)
            f = max(f - gape, g)
            H[j] = h
            diag = up
        if imax > gmax:
            gmax, te, qe = imax, i, best[1]
            if gmax >= endsc:
                break
    return gmax, te, qe


def pass_np(q, t, params, endsc=NO_STOP, tie="striped"):
    mat, gapoe, gape = _matrix(params), params[3] + params[4], params[4]
    q, t = np.asarray(q, np.int64), np.asarray(t, np.int64)
    qlen = len(q)
    prof = mat[:, q]                      # prof[c][j] = s(c, q[j])
    ramp = np.arange(qlen, dtype=np.int64) * gape
    order = _order(qlen) if tie == "striped" else np.arange(qlen)
    H, E = np.zeros(qlen, np.int64), np.zeros(qlen, np.int64)
    gmax, te, qe = 0, -1, 0
    for i in range(len(t)):
        diag = np.concatenate(([0], H[:-1]))
        hh = np.maximum(np.maximum(diag + prof[t[i]], E), 0)
        run = np.maximum.accumulate(hh - gapoe + ramp)
        F = np.concatenate(([0], np.maximum(run[:-1] - ramp[1:] + gape, 0)))   # F[j] = max_k<j (hh[k] - gapoe - (j-1-k) gape)
        H = np.maximum(hh, F)
        E = np.maximum(E - gape, np.maximum(H - gapoe, 0))
        imax = int(H.max())
        if imax > gmax:
            at = np.flatnonzero(H == imax)
            gmax, te, qe = imax, i, int(at[np.argmin(order[at])])
            if gmax >= endsc:
                break
    return gmax, te, qe


def ksw_align(q, t, params=SERVICE, tie="striped", scalar=False):
    """(score, te, qe, tb, qb) of ksw_align(qlen, q, tlen, t, 5, mat, gapo, gape, KSW_XSTART, 0) over coded sequences"""
    P = pass_scalar if scalar else pass_np
    q, t = np.asarray(q, np.int64), np.asarray(t, np.int64)
    score, te, qe = P(q, t, params, NO_STOP, tie)
    tr = np.concatenate((t[:te + 1][::-1], t[te + 1:]))       # revseq(r.te + 1, target): tlen stays (:344-346)
    s2, te2, qe2 = P(q[:qe + 1][::-1], tr, params, score, tie)
    tb, qb = (te - te2, qe - qe2) if s2 == score else (-1, -1)
    return score, te, qe, tb, qb


def align_gt_read(read, target, pos, alt, isalt, count=None):
    """the RSBWT_GT_* code of the exit align_gt_read leaves by (9, 11, 13 keep the read).  Two divergences from the
    reference, both where it is undefined: alt[0] is coded by the nt4 table (the reference stores the raw character into
    the coded target, :126), and pos = 0 or pos > |target| is code 3 (it writes outside the array there)."""
    C = count if count is not None else Counter()

    def out(c):
        C[c] += 1
        return c
    if pos == 0 or pos > len(target):
        return out(3)
    ref, rd = code(target), code(read)
    altseq = ref.copy()
    altseq[pos - 1] = code(alt[:1])[0]
    n = len(read)
    score, te, qe, tb, qb = ksw_align(rd, ref)                      # :134
    ra = pass_np(rd, altseq, SERVICE)[0]                            # :135
    if isalt:
        if ra >= score:                                             # :138
            return out(1)
    elif score < ra:                                                # :143
        return out(2)
    pi = pos - 1                                                    # :149
    if tb > pi or te < pi:                                          # :150
        return out(3)
    tgt, qry = te + 1 - tb, qe + 1 - qb
    indels = qry - tgt
    if ((n - qry) & ((1 << 64) - 1)) > 4:                           # :158, size_t
        return out(4)
    if indels == 0:
        if score < n - 3 - 3 * 4:                                   # :164-166
            return out(5)
    elif indels > 0:
        if score < n - indels - 2 - 2 * 4 - (6 + indels - 1):       # :171-173
            return out(6)
    elif score < n - 2 - 2 * 4 - (6 + indels - 1):                  # :178-180
        return out(7)
    if tgt == qry:
        return out(8 if target[pi] != read[qb + pi - tb] else 9)    # :190, the raw characters
    if te - pi > pi - tb:                                           # :196
        sub = ref[pi:te + 1]
        return out(10 if ksw_align(sub, rd)[4] != 0 else 11)        # :203-205
    sub = ref[tb:pi + 1]
    return out(12 if ksw_align(sub, rd)[2] + 1 != len(sub) else 13)  # :216-218


# ---- the verdict batch the CPU and GPU tests share: the gt fixtures' reads against windows of their haplotypes, plus
# reads made for the exits a plain simulation hardly reaches
def verdict_batch():
    """(reads, item, requests): read i belongs to request item[i]; request = (w, pos, alt, isalt)"""
    import random
    import gt_reference
    fx = gt_reference.fixture()
    rng = random.Random(1105)
    other = lambda c: rng.choice([x for x in "ACGT" if x != c])  # noqa: E731
    g = fx.haps[0]
    requests, reads, item = [], [], []
    for at in (80, 400, fx.rep[0] - 30, fx.rep[0] + 120, 1500, 1800):
        w = g[at:at + 79]
        for pos in (12, 40, 70):
            for isalt in (0, 1):
                requests.append((w, pos, other(w[pos - 1]), isalt))
    requests.append((g[200:279], 0, "A", 0))       # divergence (b): pos = 0 and pos = L + 1
    requests.append((g[200:279], 80, "A", 1))
    requests.append((g[900:979].lower(), 40, "n", 0))  # lower case, and an alt outside ACGT

    def add(r, s):
        if 1 <= len(s) <= 4096:
            reads.append(s)
            item.append(r)
    pool = [s for sh in fx.shards for s in sh]
    for r, (w, pos, alt, isalt) in enumerate(requests):
        L = len(w)
        for s in rng.sample(pool, 6):  # unrelated reads of the fixture
            add(r, s)
        if not 1 <= pos <= L:
            continue
        for _ in range(20):
            a = max(0, min(L - 40, pos - 1 - rng.randrange(0, 40)))
            s = list(w[a:a + 40].upper())
            site = pos - 1 - a
            kind = rng.randrange(11)
            if kind >= 8:  # substitutions 7 to 9 apart, too many for the score floor and too far apart to be clipped ...
                # (every stretch between them is worth crossing: 6 matches or more against a mismatch's 4, 10 against a gap's 7)
                j = rng.randrange(-1, 2)
                for p in ((6, 15, 24, 33) if kind == 8 else (8, 31)):  # 4 with no indel, 2 beside one: one more than the floor allows
                    if p + j == site:
                        p += 1
                    s[p + j] = other(s[p + j])
                if kind > 8:  # an insertion (9) or a deletion (10) in the middle, off the site
                    p = 19 if abs(19 - site) > 1 else 22
                    if kind == 9:
                        s[p:p] = [other(s[p])]
                    else:
                        del s[p]
            elif kind == 0:  # the alt allele
                s[site] = alt.upper() if alt.upper() in "ACGT" else other(s[site])
            elif kind == 1:  # a third allele
                s[site] = rng.choice([x for x in "ACGT" if x not in (w[pos - 1].upper(), alt.upper())])
            elif kind == 2:  # soft-clipped ends
                for e in range(rng.randrange(1, 7)):
                    s[e] = other(s[e])
                for e in range(rng.randrange(0, 4)):
                    s[-1 - e] = other(s[-1 - e])
            elif kind in (3, 4):  # an insertion of 1-3 left or right of the site
                n = rng.randrange(1, 4)
                p = max(3, site - rng.randrange(4, 14)) if kind == 3 else min(len(s) - 3, site + rng.randrange(4, 14))
                s[p:p] = [rng.choice("ACGT") for _ in range(n)]
            elif kind in (5, 6):  # a deletion of 1-3 left or right of the site
                n = rng.randrange(1, 4)
                p = max(3, site - rng.randrange(4, 14)) if kind == 5 else min(len(s) - 3 - n, site + rng.randrange(4, 14))
                del s[p:p + n]
            for _ in range(rng.choice((0, 0, 1, 2, 4))):  # substitutions anywhere
                p = rng.randrange(len(s))
                s[p] = other(s[p])
            add(r, "".join(s))
    return reads, item, requests


_VERDICTS = []


def verdicts():
    """(reads, item, requests, codes, Counter) of verdict_batch, computed once"""
    if not _VERDICTS:
        reads, item, requests = verdict_batch()
        C = Counter()
        codes = [align_gt_read(s, requests[r][0], requests[r][1], requests[r][2], requests[r][3], C) for s, r in zip(reads, item)]
        _VERDICTS.append((reads, item, requests, codes, C))
    return _VERDICTS[0]
