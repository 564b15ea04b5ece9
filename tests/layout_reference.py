"""What the tests hold the GPU index builder (readserver_amd/csrc/build_lines.hip) to: the host's lines, and the rule by
which the builder settles on a window span.

host_layout() is rsbwt_layout_lines_host: the run stream laid out on the host by the very passes whose every position
tests/test_layout_host.py checks (rsbwt_layout_selftest_host, rsbwt_layout_selftest_psi_host), handed out as arrays.

choose_span() restates the builder's choice of span in Python, from per-group statistics the caller supplies (the host
hook's): tests/test_rank_reference.py (golden_layout) and tests/test_gpu_builder_bytes.py share it."""
import numpy as np

ROOM = 1 << 31   # bit 31 of window_span: the RSBWT_OPEN_READS layout
HINTS = 1        # RSBWT_LAYOUT_HINTS
GROUP = 16       # windows per group; a group is 17 lines: 16 window lines and its spill line
MAX_SPAN = 2944
SAMPLE_EVERY = 64

STATS = ("S", "lines", "far_lines", "chunk_windows", "far_windows", "spilled_symbols", "groups", "sel_words", "sample_words",
         "hint_lines")


def host_layout(L, runs, span, room, hints=False, lines=True, rc_only=False):
    """dict of the ten statistics (STATS), `group` (groups, 4) uint64 = {far lines, chunk windows, far windows, spilled
    symbols} per group, and -- lines=True -- `dwords` (lines, 32) uint32 and, with hints, `sel` (sel_words,) uint64: the
    sample table, the hints written into the lines.  lines=False: the count pass alone."""
    runs = np.ascontiguousarray(runs, dtype=np.uint8)
    st = np.zeros(10, np.uint64)
    arg = (int(span) | (ROOM if room else 0), HINTS if hints else 0)
    rc = L.rsbwt_layout_lines_host(runs.ctypes.data, runs.size, *arg, None, 0, None, 0, None, 0, st.ctypes.data)
    if rc_only:
        return rc
    assert rc == 0, rc
    out = dict(zip(STATS, (int(x) for x in st)))
    group = np.zeros((out["groups"], 4), np.uint64)
    if not lines:
        rc = L.rsbwt_layout_lines_host(runs.ctypes.data, runs.size, *arg, None, 0, None, 0, group.ctypes.data, len(group), st.ctypes.data)
        assert rc == 0, rc
        out["group"] = group
        return out
    buf = np.empty((out["lines"], 32), np.uint32)
    sel = np.empty(out["sel_words"] if hints else 0, np.uint64)
    rc = L.rsbwt_layout_lines_host(runs.ctypes.data, runs.size, *arg, buf.ctypes.data, buf.nbytes, sel.ctypes.data if hints else None,
                                   sel.size, group.ctypes.data, len(group), st.ctypes.data)
    assert rc == 0, rc
    out.update(zip(STATS, (int(x) for x in st)))
    out.update(group=group, dwords=buf)
    if hints:
        out["sel"] = sel
    return out


def _clamp(S):
    return max(2, min(MAX_SPAN, int(S)))


def choose_span(n, R, room, stats_at, want_span=0):
    """The builder's choice of span (csrc/build_lines.hip), restated.  It starts at 88 pieces per window at the mean run
    length (88 * 88 / 96 with room for a psi hint).  A shard of 4,096 groups or more first tries its spans on a SAMPLE,
    the groups 0, 64, 128, ...: their spilled symbols and far windows, times 64, held to the limits below plus 5 % -- at
    most 4 (16) spans, each 0.95 (0.9875) of the one before.  Then the full pass decides: a span is shrunk the same way
    while more than 2.5 % of the positions spill or more than 1.5 % of the windows need far lines, 4 (16) times at most.
    A span asked for is taken as it is.

    stats_at(S) -> (stats6 = [S, lines, far lines, chunk windows, far windows, spilled symbols], per-group (groups, 4)
    array {far lines, chunk windows, far windows, spilled symbols} or None where no sample can be asked for).
    Returns (stats6 at the span chosen, trace): trace lists ("sample" | "full", S, passed) for every span tried."""
    target = 88.0 * 88 / 96 if room else 88.0
    shrink = 0.9875 if room else 0.95
    max_attempts = 16 if room else 4
    S = _clamp(want_span if want_span else int(target * (n / R) + 0.5))
    trace = []
    if not want_span and ((n + S - 1) // S) // GROUP >= 64 * SAMPLE_EVERY:
        for attempt in range(max_attempts):
            if S <= 8:
                break
            nw = (n + S - 1) // S
            _, group = stats_at(S)
            assert group is not None and len(group) == (nw + GROUP - 1) // GROUP
            far_windows, spilled = int(group[::SAMPLE_EVERY, 2].sum()), int(group[::SAMPLE_EVERY, 3].sum())
            ok = spilled * SAMPLE_EVERY * 40 <= n + n // 20 and far_windows * SAMPLE_EVERY * 200 <= (nw + nw // 20) * 3
            trace.append(("sample", S, ok))
            if ok:
                break
            smaller = _clamp(S * shrink)
            if smaller >= S:
                break
            S = smaller
    attempt = 0
    while True:
        st, _ = stats_at(S)
        nwin = (n + S - 1) // S
        ok = st[5] * 40 <= n and st[4] * 200 <= nwin * 3
        trace.append(("full", S, ok))
        if want_span or ok or attempt >= max_attempts or S <= 8:
            break
        smaller = _clamp(S * shrink)
        if smaller >= S:
            break
        S = smaller
        attempt += 1
    return st, trace


def line_kind(line, groups, far_before):
    """(kind, group) of line number `line`: "window", "spill" or "far"; far_before = far lines before each group"""
    first_far = groups * (GROUP + 1)
    if line < first_far:
        return ("spill" if line % (GROUP + 1) == GROUP else "window"), line // (GROUP + 1)
    return "far", int(np.searchsorted(far_before, line - first_far, side="right")) - 1
