// ksw_pass.h -- ksw_align of the reference's src/service/ksw.c (the 16-bit striped path, KSW_XSTART) as ONE LANE's
// scalar walk, and align_gt_read (src/service/service.cpp:105-225) over it.  Compiles for the device (ksw_align.hip) and
// for the host (tests/native/ksw_pass_host.cpp checks it against recorded outputs of the reference without a GPU).
//
// One pass P(q, t, endsc): the lane walks the target column by column; the column's H and E live as packed 16-bit
// pairs in he[row * stride] (LDS laid out [row][lane], or a scratch buffer in HBM: the same code over another
// pointer), the rows' codes as nibbles in qc[(row / 8) * stride]; F, the column's maximum and the tie-break key are
// carried in registers down the column.  All values are >= 0 and below 2^15 (the caller refuses match * min(qlen,
// tlen) >= 2^15, where the reference's 16-bit lanes would saturate).
//   H[i][j]   = max(0, H[i-1][j-1] + s(t[i], q[j]), E[i][j], F[i][j])
//   E[i+1][j] = max(E[i][j] - gape, H[i][j] - (gapo + gape))     F[i][j+1] likewise, both floored at 0
//   te = the LAST column whose maximum rose above every column before it; the pass stops after the column at which
//        that maximum reaches endsc (ksw.c:295-300)
//   qe = the row of the maximum in column te; ties go to the smallest (j mod slen, j div slen), slen = (qlen + 7) / 8:
//        the order ksw.c:307-308 scans the striped vectors in
// Nothing is reversed in memory: a seq_view reads its first flip + 1 symbols backwards.
#ifndef RSBWT_KSW_PASS_H
#define RSBWT_KSW_PASS_H

#include <stdint.h>

#if defined(__HIPCC__)
#define KSW_HD __host__ __device__ inline
#else
#define KSW_HD inline
#endif

namespace rsb {
namespace ksw {

constexpr int MAX_LEN = 4096;    // symbols of a query or a target
constexpr int NO_STOP = 0x10000;  // endsc of a pass that runs to the last column (ksw.c:240)

struct scores {
    int match, mismatch, ambiguous, gapoe, gape;  // gapoe = gapo + gape: what the first gap symbol costs
};

// ASCII symbols p[0 .. len), read as  i <= flip ? p[flip - i] : p[i]  (flip = 0: as they lie; revseq of ksw.c:344
// without the copy), coded by seq_nt4_table; position sub_idx (of p, -1 = none) reads as sub_code instead.
struct seq_view {
    const char *p;
    int len, flip, sub_idx, sub_code;
};

KSW_HD int nt4(unsigned char c) {
    switch (c & 0xDFu) {  // ACGTacgt -> 0..3, anything else 4
    case 'A': return 0;
    case 'C': return 1;
    case 'G': return 2;
    case 'T': return 3;
    default: return 4;
    }
}

KSW_HD int code_at(const seq_view &v, int i) {
    int idx = i <= v.flip ? v.flip - i : i;
    idx = idx < 0 ? 0 : (idx >= v.len ? v.len - 1 : idx);  // (never taken by a correct caller: no read leaves the text)
    return idx == v.sub_idx ? v.sub_code : nt4((unsigned char)v.p[idx]);
}

struct pass_result {
    int score, te, qe;
};

// The lane's column: he[j * stride] for row j, qc[(j >> 3) * stride] for the codes of rows 8 (j >> 3) .. + 7;
// room for `rows` rows.
struct column {
    uint32_t *he, *qc;
    uint32_t stride;
    int rows;
};

KSW_HD pass_result pass(const scores &s, const seq_view &q, int qlen, const seq_view &t, int tlen, int endsc, const column &col) {
    if (qlen > col.rows) qlen = col.rows;  // (never taken: the launch sized the column for the longest pass)
    const int slen = (qlen + 7) >> 3;
    for (int w = 0; w < slen; ++w) {
        uint32_t word = 0;
        for (int k = 0; k < 8 && w * 8 + k < qlen; ++k) word |= (uint32_t)code_at(q, w * 8 + k) << (4 * k);
        col.qc[(uint32_t)w * col.stride] = word;
    }
    for (int j = 0; j < qlen; ++j) col.he[(uint32_t)j * col.stride] = 0u;
    int gmax = 0, te = -1, qe = 0;  // nothing scores: ksw.c:307-308 picks row 0 of an all-zero Hmax
    for (int i = 0; i < tlen; ++i) {
        const int c = code_at(t, i);
        int f = 0, hdiag = 0, imax = 0, brow = 0, seg = 0, lane = 0;
        uint32_t bkey = ~0u, word = 0;
        for (int j = 0; j < qlen; ++j) {
            if ((j & 7) == 0) word = col.qc[(uint32_t)(j >> 3) * col.stride];
            const int cj = (int)((word >> ((j & 7) * 4)) & 7u);
            const uint32_t x = col.he[(uint32_t)j * col.stride];
            const int hup = (int)(x & 0xFFFFu);
            int e = (int)(x >> 16);
            int h = hdiag + ((c == 4 || cj == 4) ? -s.ambiguous : (c == cj ? s.match : -s.mismatch));
            h = h > e ? h : e;
            h = h > f ? h : f;
            h = h > 0 ? h : 0;
#ifdef RSB_MUTATE_KSW_TIE_ROW  // mutation check: ties to the smallest row
            const uint32_t key = (uint32_t)j;
#else
            const uint32_t key = (uint32_t)seg * 8u + (uint32_t)lane;
#endif
            if (h > imax || (h == imax && key < bkey)) {
                imax = h;
                bkey = key;
                brow = j;
            }
            int g = h - s.gapoe;
            g = g > 0 ? g : 0;
            e -= s.gape;
            e = e > g ? e : g;
            f -= s.gape;
            f = f > g ? f : g;
            col.he[(uint32_t)j * col.stride] = (uint32_t)h | ((uint32_t)e << 16);
            hdiag = hup;
            if (++seg == slen) {
                seg = 0;
                ++lane;
            }
        }
        if (imax > gmax) {
            gmax = imax;
            te = i;
            qe = brow;
            if (gmax >= endsc) break;
        }
    }
    return pass_result{gmax, te, qe};
}

struct align_result {
    int score, te, qe, tb, qb;
};

// ksw_align(..., KSW_XSTART, 0) of ksw.c:330-352; q and t with flip = 0
KSW_HD align_result align(const scores &s, const seq_view &q, const seq_view &t, const column &col, bool start = true) {
    const pass_result r = pass(s, q, q.len, t, t.len, NO_STOP, col);
    align_result o{r.score, r.te, r.qe, -1, -1};
    if (!start) return o;
    seq_view qr = q, tr = t;
    qr.flip = r.qe;
    tr.flip = r.te;  // (-1: nothing is reversed)
#ifdef RSB_MUTATE_KSW_REV_COLUMNS  // mutation check: the reversed pass over te + 1 columns only
    const pass_result rr = pass(s, qr, r.qe + 1, tr, r.te + 1, r.score, col);
#else
    const pass_result rr = pass(s, qr, r.qe + 1, tr, t.len, r.score, col);
#endif
    if (rr.score == r.score) {
        o.tb = r.te - rr.te;
        o.qb = r.qe - rr.qe;
    }
    return o;
}

// align_gt_read (service.cpp:105-225) exit by exit: the RSBWT_GT_* code of include/rsbwt.h.  The column must hold
// max(rlen, wlen) rows (the sub-alignments of :196-221 put a piece of the window on the rows).
KSW_HD int gt_verdict(const scores &s, const char *read, int rlen, const char *w, int wlen, uint64_t pos, int alt_code, bool isalt,
                      const column &col) {
    if (pos == 0 || pos > (uint64_t)wlen) return 3;  // (the reference writes outside altseq at :126)
    const int pi = (int)(pos - 1);                   // pos_index, :149
    const seq_view rq{read, rlen, 0, -1, 0}, tw{w, wlen, 0, -1, 0}, ta{w, wlen, 0, pi, alt_code};
    const align_result r = align(s, rq, tw, col);                          // :134
    const int ra = pass(s, rq, rlen, ta, wlen, NO_STOP, col).score;         // :135 (only the score is read)
    if (isalt) {
        if (ra >= r.score) return 1;  // :138
    } else {
        if (r.score < ra) return 2;   // :143
    }
    if (r.tb > pi || r.te < pi) return 3;  // :150
    const int tgtbases = r.te + 1 - r.tb, qrybases = r.qe + 1 - r.qb, indels = qrybases - tgtbases;
    if ((uint64_t)rlen - (uint64_t)(int64_t)qrybases > 4u) return 4;  // :158, size_t arithmetic
    if (indels == 0) {
        if (r.score < rlen - 3 - 3 * 4) return 5;  // :164-166
    } else if (indels > 0) {
        if (r.score < rlen - indels - 2 - 2 * 4 - (6 + indels - 1)) return 6;  // :171-173
    } else {
        if (r.score < rlen - 2 - 2 * 4 - (6 + indels - 1)) return 7;  // :178-180
    }
    if (tgtbases == qrybases) {
        const int at = r.qb + pi - r.tb;  // within [qb, qe]: tb <= pi <= te
        return w[pi] != read[at < 0 ? 0 : (at >= rlen ? rlen - 1 : at)] ? 8 : 9;  // :190, the raw characters
    }
    if ((uint64_t)(int64_t)r.te - (uint64_t)pi > (uint64_t)pi - (uint64_t)(int64_t)r.tb) {  // :196, size_t arithmetic
        const int sub = r.te - pi + 1;
        const seq_view sq{w + pi, sub, 0, -1, 0};
        return align(s, sq, rq, col).qb != 0 ? 10 : 11;  // :203-205
    }
    const int tb = r.tb < 0 ? 0 : r.tb;  // (tb is never -1: the reversed pass always reaches the score)
    const int sub = pi - tb + 1;
    const seq_view sq{w + tb, sub, 0, -1, 0};
    return align(s, sq, rq, col, false).qe + 1 != sub ? 12 : 13;  // :216-218
}

}  // namespace ksw
}  // namespace rsb
#endif
