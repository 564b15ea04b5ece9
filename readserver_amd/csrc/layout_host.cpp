// layout_host.cpp -- host-side check of the window-line layout (line_format.h).
//
// TEST HOOK, not a query path: lays a run stream out with the very code the GPU builder kernels
// run (build_group) and holds the scalar readers the secondary kernels run (view_occ, view_char,
// view_occ_at) to naive ranks at every position.  It answers no query and nothing in the engine
// calls it; all searches, mirrors and extractions run on the GPU only.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/rsbwt.h"
#include "line_format.h"

using namespace rsb;

// (bit 31 of window_span, both hooks: the RSBWT_OPEN_READS layout -- room for a psi hint in every window line)
static constexpr uint32_t SELFTEST_ROOM = 1u << 31;

// ---- the build passes: one piece of code for the two selftests and for rsbwt_layout_lines_host, so that the lines the
// hook hands out are the lines whose every position the selftests check

// what a run stream holds: symbols per code; RSBWT_EFORMAT for a code above 4 (a zero-length byte's code counts too, as
// in the GPU builder's tile totals)
static int scan_runs(const uint8_t *runs, uint64_t num_runs, uint64_t total[5]) {
    for (int c = 0; c < 5; ++c) total[c] = 0;
    for (uint64_t r = 0; r < num_runs; ++r) {
        if ((runs[r] >> 5) > 4) return RSBWT_EFORMAT;
        total[runs[r] >> 5] += runs[r] & 31u;
    }
    return RSBWT_OK;
}

struct host_layout {
    span_params sp;
    bool room;
    uint64_t n, nwin, ngroups, first_far, nlines;
    std::vector<uint64_t> far_base;  // far lines before each group (ngroups + 1)
    std::vector<group_stats> per_group;
    group_stats tot;
};

// pass 1: the span (0 = 90 pieces per window at the mean run length), then far lines and statistics per group, one
// reader over the whole stream
static void count_pass(const uint8_t *runs, uint64_t num_runs, uint64_t n, uint32_t window_span, bool room, host_layout &lay) {
    uint32_t S = window_span;
    if (!S) S = (uint32_t)(90.0 * (double)n / (double)num_runs + 0.5);
    lay.sp = make_span(S);
    lay.room = room;
    lay.n = n;
    lay.nwin = (n + lay.sp.S - 1) / lay.sp.S;
    lay.ngroups = (lay.nwin + GROUP - 1) / GROUP;
    lay.far_base.assign(lay.ngroups + 1, 0);
    lay.per_group.resize(lay.ngroups);
    lay.tot = {0, 0, 0, 0};
    const uint64_t zero[4] = {0, 0, 0, 0};
    run_reader rd;
    rd.start(runs, num_runs, 0, zero);
    for (uint64_t g = 0; g < lay.ngroups; ++g) {
        const group_stats st = build_group<false>(lay.sp, n, lay.nwin, g, rd, nullptr, 0, room);
        lay.per_group[g] = st;
        lay.far_base[g + 1] = lay.far_base[g] + st.far_lines;
        lay.tot.far_lines += st.far_lines;
        lay.tot.chunk_windows += st.chunk_windows;
        lay.tot.far_windows += st.far_windows;
        lay.tot.spilled_symbols += st.spilled_symbols;
    }
    lay.first_far = lay.ngroups * (GROUP + 1);
    lay.nlines = lay.first_far + lay.far_base[lay.ngroups];
}

// pass 2 of rsbwt_layout_selftest_host: every group from a reader re-seated at its first symbol (as the GPU threads
// are).  `lines`: nlines * LINE_DWORDS zeroed dwords.
static void write_pass_reseated(const uint8_t *runs, uint64_t num_runs, const host_layout &lay, uint32_t *lines) {
    uint64_t cnt[4] = {0, 0, 0, 0};
    uint64_t r = 0, at = 0;
    for (uint64_t g = 0; g < lay.ngroups; ++g) {
        const uint64_t gstart = g * GROUP * (uint64_t)lay.sp.S;
        // runs wholly before the group's first symbol
        while (r < num_runs && at + (runs[r] & 31u) <= gstart) {
            const uint32_t sy = runs[r] >> 5;
            if (sy >= 1 && sy <= 4) cnt[sy - 1] += runs[r] & 31u;
            at += runs[r] & 31u;
            ++r;
        }
        run_reader rd;
        rd.start(runs, num_runs, r, cnt);
        rd.skip_symbols(gstart - at);
        build_group<true>(lay.sp, lay.n, lay.nwin, g, rd, lines, lay.first_far + lay.far_base[g], lay.room);
    }
}

// pass 2 of rsbwt_layout_selftest_psi_host: one reader over the whole stream
static void write_pass_sequential(const uint8_t *runs, uint64_t num_runs, const host_layout &lay, uint32_t *lines) {
    const uint64_t zero[4] = {0, 0, 0, 0};
    run_reader rd;
    rd.start(runs, num_runs, 0, zero);
    for (uint64_t g = 0; g < lay.ngroups; ++g)
        build_group<true>(lay.sp, lay.n, lay.nwin, g, rd, lines, lay.first_far + lay.far_base[g], lay.room);
}

static shard_view host_view(const host_layout &lay, const uint32_t *lines, const uint64_t total[5]) {
    shard_view v;
    memset(&v, 0, sizeof v);
    v.lines = lines;
    v.n = lay.n;
    v.nwin = lay.nwin;
    v.nlines = lay.nlines;
    v.first_far = lay.first_far;
    v.sp = lay.sp;
    v.sel_shift = lay.room ? SEL_SHIFT_SPARSE : SEL_SHIFT_DENSE;
    v.hint_room = lay.room ? 1u : 0u;
    for (int c = 0; c < 5; ++c) v.total[c] = total[c];
    for (int c = 1; c < 5; ++c) v.C[c] = v.C[c - 1] + v.total[c - 1];
    return v;
}

static void put_stats6(const host_layout &lay, uint64_t *stats6) {
    stats6[0] = lay.sp.S;
    stats6[1] = lay.nlines;
    stats6[2] = lay.tot.far_lines;
    stats6[3] = lay.tot.chunk_windows;
    stats6[4] = lay.tot.far_windows;
    stats6[5] = lay.tot.spilled_symbols;
}

// the select sample table (5 * select_stride(v) zeroed words) as select_sample_kernel fills it; the words written
static uint64_t build_samples(const shard_view &v, uint64_t *sel) {
    const uint64_t stride = select_stride(v);
    uint64_t words = 0;
    for (uint64_t w = 0; w < v.nwin; ++w)
        for (uint32_t c = 0; c <= 4; ++c)
            window_samples(v, w, c, [&](uint64_t m, uint64_t word) {
                sel[c * stride + m] = word;
                ++words;
            });
    return words;
}

// the psi hints, written into the lines as psi_hint_kernel writes them; the lines that got one
static uint64_t write_hints(const shard_view &v, const uint64_t *sel, uint32_t *lines) {
    const uint64_t stride = select_stride(v);
    uint64_t hint_lines = 0;
    for (uint64_t w = 0; w < v.nwin; ++w) {
        uint32_t w0, kk;
        if (!window_psi_hint(v, sel, stride, w, &w0, &kk)) continue;
        uint32_t *Ln = lines + line_of_window(w) * LINE_DWORDS;
        const uint32_t hd = hint_dword(parse_line(Ln).kind);
        Ln[hd] = w0;
        Ln[hd + 1u] = kk;
        Ln[1] |= 1u << (8u + HINT_META0_BIT);
        ++hint_lines;
    }
    return hint_lines;
}

extern "C" int rsbwt_layout_selftest_host(const uint8_t *runs, uint64_t num_runs, uint32_t window_span,
                                          uint64_t *stats6, uint64_t *first_bad) {
    if (!runs && num_runs) return RSBWT_EINVAL;
    const bool room = (window_span & SELFTEST_ROOM) != 0u;
    window_span &= ~SELFTEST_ROOM;
    // naive expansion
    std::vector<uint8_t> bwt;
    for (uint64_t r = 0; r < num_runs; ++r) {
        if ((runs[r] >> 5) > 4) return RSBWT_EFORMAT;
        bwt.insert(bwt.end(), runs[r] & 31u, (uint8_t)(runs[r] >> 5));
    }
    const uint64_t n = bwt.size();
    if (first_bad) *first_bad = ~0ull;
    if (n == 0) return RSBWT_OK;
    host_layout lay;
    count_pass(runs, num_runs, n, window_span, room, lay);
    std::vector<uint32_t> lines(lay.nlines * LINE_DWORDS, 0);
    write_pass_reseated(runs, num_runs, lay, lines.data());
    uint64_t total[5] = {0, 0, 0, 0, 0};
    for (uint64_t p = 0; p < n; ++p) total[bwt[p]]++;
    const shard_view v = host_view(lay, lines.data(), total);
    const uint64_t nwin = lay.nwin;
    if (stats6) put_stats6(lay, stats6);
    // every position: Occ of all five symbols, the symbol itself, and select of that occurrence
    uint64_t occ[5] = {0, 0, 0, 0, 0};
    for (uint64_t p = 0; p < n; ++p) {
        const uint32_t c = bwt[p];
        occ[c]++;
        bool ok = view_char(v, p) == c;
        for (uint32_t b = 0; b < 5 && ok; ++b) ok = view_occ(v, b, p) == occ[b];
        uint64_t oc = 0;
        ok = ok && view_char_occ(v, p, &oc) == c && oc == occ[c];
        ok = ok && view_occ_at(v, c, occ[c], 0, nwin - 1) == p;
        if (!ok) {
            if (first_bad) *first_bad = p;
            return RSBWT_EFORMAT;
        }
    }
    return RSBWT_OK;
}


// TEST HOOK, host only: the select samples and psi hints (line_format.h: window_samples, sample_window,
// window_psi_hint, hint_window -- the code the builder kernels and the walk kernels run) built over a host-side layout
// of `runs` and held to the naive answer: for EVERY occurrence of every symbol the sample names the window that holds
// it (or, where it says "not exact", a window at or before it); for EVERY row whose window's line carries a hint that
// claims to be exact, the hint names the window psi takes the row to; and with the hints written into the lines every
// scalar reader still gives the naive answer at every position.  stats4 = {sample words, occurrences whose sample is
// only a bound, lines with a hint, rows answered by a hint}.
extern "C" int rsbwt_layout_selftest_psi_host(const uint8_t *runs, uint64_t num_runs, uint32_t window_span, uint64_t *stats4,
                                              uint64_t *first_bad) {
    if (!runs && num_runs) return RSBWT_EINVAL;
    const bool room = (window_span & SELFTEST_ROOM) != 0u;
    window_span &= ~SELFTEST_ROOM;
    std::vector<uint8_t> bwt;
    for (uint64_t r = 0; r < num_runs; ++r) {
        if ((runs[r] >> 5) > 4) return RSBWT_EFORMAT;
        bwt.insert(bwt.end(), runs[r] & 31u, (uint8_t)(runs[r] >> 5));
    }
    const uint64_t n = bwt.size();
    if (first_bad) *first_bad = ~0ull;
    if (stats4) stats4[0] = stats4[1] = stats4[2] = stats4[3] = 0;
    if (n == 0) return RSBWT_OK;
    host_layout lay;
    count_pass(runs, num_runs, n, window_span, room, lay);
    std::vector<uint32_t> lines(lay.nlines * LINE_DWORDS, 0);
    write_pass_sequential(runs, num_runs, lay, lines.data());
    uint64_t total[5] = {0, 0, 0, 0, 0};
    for (uint64_t p = 0; p < n; ++p) total[bwt[p]]++;
    const shard_view v = host_view(lay, lines.data(), total);
    const span_params sp = lay.sp;
    const uint64_t nwin = lay.nwin;
    // positions of the occurrences of every symbol (the naive select)
    std::vector<uint64_t> where[5];
    for (uint64_t p = 0; p < n; ++p) where[bwt[p]].push_back(p);
    // ---- samples
    const uint64_t stride = select_stride(v);
    std::vector<uint64_t> sel(5 * stride, 0);
    const uint64_t words = build_samples(v, sel.data());
    uint64_t inexact = 0;
    for (uint32_t c = 0; c <= 4; ++c)
        for (uint64_t bc = 1; bc <= v.total[c]; ++bc) {
            bool exact;
            const uint32_t w = sample_window(sel[c * stride + ((bc - 1) >> v.sel_shift)], bc, v.sel_shift, &exact);
            const uint64_t truth = where[c][bc - 1] / sp.S;
            if (!exact) ++inexact;
            // exact or a bound -- and, either way, the floor search between the samples ends on the window
            if ((exact ? w != truth : w > truth) || select_window(v, sel.data(), stride, c, bc) != truth) {
                if (first_bad) *first_bad = where[c][bc - 1];
                return RSBWT_EFORMAT;
            }
        }
    // ---- hints, written into the lines as the kernel writes them
    const uint64_t hint_lines = write_hints(v, sel.data(), lines.data());
    uint64_t by_hint = 0;
    const uint32_t hs = hint_shift(sp.S);
    for (uint64_t i = 0; i < n; ++i) {  // row i: psi(i) = select_f(i - C[f] + 1), f = F(i)
        uint32_t f = 0;
        while (f < 4u && v.C[f + 1] <= i) ++f;
        if (f == 0u) continue;
        const uint64_t w = i / sp.S, r0 = w * (uint64_t)sp.S;
        const uint32_t *Ln = lines.data() + line_of_window(w) * LINE_DWORDS;
        const line_meta lm = parse_line(Ln);
        if (!lm.hint || Ln[hint_dword(lm.kind)] == HINT_NONE || r0 < v.C[f]) continue;  // (the walk kernel's own conditions)
        const hint_range hr = hint_windows(Ln[hint_dword(lm.kind)], Ln[hint_dword(lm.kind) + 1u], (uint32_t)(i - r0), hs);
        const uint64_t truth = where[f][i - v.C[f]] / sp.S;
        // the row's window lies in lo..hi -- or, an open range, anywhere from lo on
        if (truth < hr.lo || (!hr.open && truth > hr.hi)) {
            if (first_bad) *first_bad = i;
            return RSBWT_EFORMAT;
        }
        if (hr.lo == hr.hi && !hr.open) ++by_hint;
    }
    if (stats4) {
        stats4[0] = words;
        stats4[1] = inexact;
        stats4[2] = hint_lines;
        stats4[3] = by_hint;
    }
    // ---- every scalar reader again, over the lines that now carry hints
    uint64_t occ[5] = {0, 0, 0, 0, 0};
    for (uint64_t p = 0; p < n; ++p) {
        const uint32_t c = bwt[p];
        occ[c]++;
        bool ok = view_char(v, p) == c;
        for (uint32_t b = 0; b < 5 && ok; ++b) ok = view_occ(v, b, p) == occ[b];
        uint64_t oc = 0;
        ok = ok && view_char_occ(v, p, &oc) == c && oc == occ[c];
        ok = ok && view_occ_at(v, c, occ[c], 0, nwin - 1) == p;
        if (!ok) {
            if (first_bad) *first_bad = p;
            return RSBWT_EFORMAT;
        }
    }
    return RSBWT_OK;
}

// TEST HOOK, host only (answers no query): the lines the two selftests above certify, handed out -- so that a GPU test
// can hold the device builder's lines, and the select sample table, to them byte for byte.  The stream is laid out by
// the selftests' own passes (RSBWT_LAYOUT_HINTS clear: rsbwt_layout_selftest_host's, every group from a re-seated
// reader; set: rsbwt_layout_selftest_psi_host's, then its sample table and its hints written into the lines).
// window_span as for the selftests (bit 31: the RSBWT_OPEN_READS layout; 0: 90 pieces per window).
//   out_lines     nlines * 128 bytes (cap_bytes of room); NULL = the count pass only: statistics, nothing built
//   out_sel       with RSBWT_LAYOUT_HINTS, 5 * select_stride words (cap_sel_words of room); may be NULL
//   group_stats   4 numbers per group {far lines, chunk windows, far windows, spilled symbols} (cap_groups of room);
//                 may be NULL
//   stats10       {S, lines, far lines, chunk windows, far windows, spilled symbols, groups, words of the sample table,
//                 sample words written, lines with a hint} (the last two 0 unless built)
// RSBWT_ERANGE when a buffer is too small (stats10 is filled all the same: call once without buffers to size them).
extern "C" int rsbwt_layout_lines_host(const uint8_t *runs, uint64_t num_runs, uint32_t window_span, uint32_t flags,
                                       uint32_t *out_lines, uint64_t cap_bytes, uint64_t *out_sel, uint64_t cap_sel_words,
                                       uint64_t *group_stats4, uint64_t cap_groups, uint64_t *stats10) {
    if ((!runs && num_runs) || !stats10 || (flags & ~RSBWT_LAYOUT_HINTS)) return RSBWT_EINVAL;
    const bool room = (window_span & SELFTEST_ROOM) != 0u, hints = (flags & RSBWT_LAYOUT_HINTS) != 0u;
    window_span &= ~SELFTEST_ROOM;
    for (int i = 0; i < 10; ++i) stats10[i] = 0;
    uint64_t total[5];
    const int rc = scan_runs(runs, num_runs, total);
    if (rc != RSBWT_OK) return rc;
    const uint64_t n = total[0] + total[1] + total[2] + total[3] + total[4];
    if (n == 0) return RSBWT_OK;
    host_layout lay;
    count_pass(runs, num_runs, n, window_span, room, lay);
    shard_view v = host_view(lay, out_lines, total);
    const uint64_t sel_words = 5 * select_stride(v);
    put_stats6(lay, stats10);
    stats10[6] = lay.ngroups;
    stats10[7] = sel_words;
    if (group_stats4) {
        if (cap_groups < lay.ngroups) return RSBWT_ERANGE;
        for (uint64_t g = 0; g < lay.ngroups; ++g) {
            group_stats4[4 * g] = lay.per_group[g].far_lines;
            group_stats4[4 * g + 1] = lay.per_group[g].chunk_windows;
            group_stats4[4 * g + 2] = lay.per_group[g].far_windows;
            group_stats4[4 * g + 3] = lay.per_group[g].spilled_symbols;
        }
    }
    if (!out_lines) return RSBWT_OK;
    if (cap_bytes / LINE_BYTES < lay.nlines || (hints && out_sel && cap_sel_words < sel_words)) return RSBWT_ERANGE;
    memset(out_lines, 0, lay.nlines * (uint64_t)LINE_BYTES);
    if (!hints) {
        write_pass_reseated(runs, num_runs, lay, out_lines);
        return RSBWT_OK;
    }
    write_pass_sequential(runs, num_runs, lay, out_lines);
    std::vector<uint64_t> sel(sel_words, 0);
    stats10[8] = build_samples(v, sel.data());
    stats10[9] = write_hints(v, sel.data(), out_lines);
    if (out_sel) memcpy(out_sel, sel.data(), sel_words * sizeof(uint64_t));
    return RSBWT_OK;
}

// TEST HOOK: the grouped k-mer table's record code (line_format.h: what ktab_group_encode_kernel writes and what
// ktab_entry reads) on the host: `groups` x 4 (lower, upper) pairs in, the 4 entries each record gives back out, in
// the plain table's form {lower:40 | width:24}, width RSBWT_KTAB_WIDE = left to the search.
extern "C" int rsbwt_ktab_group_selftest_host(const uint64_t *lower, const uint64_t *upper, size_t groups, uint64_t *entries) {
    if ((!lower || !upper || !entries) && groups) return RSBWT_EINVAL;
    for (size_t g = 0; g < groups; ++g) {
        uint32_t rec[3];
        ktab_group_encode(lower + 4 * g, upper + 4 * g, rec);
        for (uint32_t i = 0; i < 4u; ++i) entries[4 * g + i] = ktab_group_entry(rec[0], rec[1], rec[2], i);
    }
    return RSBWT_OK;
}
