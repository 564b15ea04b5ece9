"""Host-side mirror of ReadServer's ``BWT`` / ``query.h`` interface over librsbwt.so.

Names and argument meaning follow the reference so parity tests read like its call sites:
``class BWT`` (include/bwt/bwt.h:6-15), ``RLEBWT(filename)`` (include/bwt/rlebwt.h:17),
``findInterval / extractPrefix / extractPostfix / query / query_exactmatch``
(include/bwt/query.h:18-32).  Every query runs in the HIP library; numpy is used only to hand
buffers across the C-ABI.
"""
import ctypes as C
from collections import namedtuple

import numpy as np

from . import _native
from ._native import RsbwtError, check, lib

BWTInterval = namedtuple("BWTInterval", ["lower", "upper"])  # include/bwt/query.h:8-11


def _ptr(a):
    return C.c_void_p(a.ctypes.data)


# rsbwt_set_walk's stop codes and the flag word of the walk / extension calls (include/rsbwt.h)
WALK_DEAD_END, WALK_BRANCH, WALK_LIMIT, WALK_INVALID = 1, 2, 3, 4
WALK_JOIN = 5  # rsbwt_set_unitigs alone: another path enters the node the side would enter
# rsbwt_set_paths alone: a path reached its seed's target / the seed's evaluations ran out; and the seed states
WALK_TARGET, WALK_BUDGET = 6, 7
WALK_WIDE = 8  # rsbwt_set_walk_samples alone: a candidate of the evaluation has more rows than max_rows
PATHS_COMPLETE, PATHS_MORE, PATHS_BUDGET, PATHS_INVALID = 1, 2, 3, 4


def unitig_sequence(seed, right_ext, left_ext):
    """the sequence of a unitig of ShardSet.unitigs: the left side's symbols are in the order they were appended"""
    return left_ext[::-1] + seed + right_ext


def _walk_flags(left, both_strands):
    return (1 if left else 0) | (2 if both_strands else 0)


def _kmer_matrix(kmers):
    """list of equal-length str/bytes, or a (Q, k) uint8 array -> (contiguous uint8 (Q, k), k)."""
    if isinstance(kmers, np.ndarray):
        a = np.ascontiguousarray(kmers, dtype=np.uint8)
        if a.ndim != 2:
            raise ValueError("k-mer array must be (Q, k) uint8")
        return a, a.shape[1]
    ks = [s.encode() if isinstance(s, str) else bytes(s) for s in kmers]
    if not ks:
        return np.zeros((0, 0), np.uint8), 0
    k = len(ks[0])
    if any(len(s) != k for s in ks):
        raise ValueError("all k-mers of one batch must have the same length")
    return np.frombuffer(b"".join(ks), dtype=np.uint8).reshape(len(ks), k).copy(), k


class GpuBWT:
    """One BWT shard resident in HBM: ``RLEBWT`` (include/bwt/rlebwt.h:15-61) on the GPU.

    GpuBWT(filename)                      # SGA .bwt, as RLEBWT(filename)
    GpuBWT(runs=uint8 array, num_strings=) # RLUnit bytes in host memory
    GpuBWT(device_runs=(ptr, n), ...)      # RLUnit bytes already in HBM (e.g. a torch tensor)
    """

    def __init__(self, filename=None, device=0, *, runs=None, device_runs=None, num_strings=0,
                 ktab_depth=0, window_span=0, for_reads=False, ktab_grouped=False):
        """ktab_depth: depth of the k-mer table (0 = auto, None = no table); ktab_grouped: RSBWT_OPEN_KTAB_GROUPED
        -- its 3-bytes-per-T-mer format (include/rsbwt.h).  window_span: symbols
        per window of the HBM layout (0 = from the data: ~88 run pieces per 128-byte line).
        for_reads: RSBWT_OPEN_READS -- a psi hint in every window line, built with the index
        (the layout for a shard that serves read extraction)."""
        self._h = C.c_void_p()
        L = lib()
        flags = (31 if ktab_depth is None else int(ktab_depth) & 0x1F) << 5
        flags |= (int(window_span) & 0xFFF) << 12
        flags |= 1 if for_reads else 0
        flags |= 2 if ktab_grouped else 0
        if filename is not None:
            check(L.rsbwt_open(str(filename).encode(), device, flags, C.byref(self._h)))
        elif runs is not None:
            r = np.ascontiguousarray(runs, dtype=np.uint8)
            check(L.rsbwt_open_runs(_ptr(r), r.size, num_strings, device, flags, C.byref(self._h)))
        elif device_runs is not None:
            ptr, n = device_runs
            check(L.rsbwt_open_device_runs(C.c_void_p(ptr), n, num_strings, device, flags,
                                           C.byref(self._h)))
        else:
            raise ValueError("one of filename, runs, device_runs is required")

    # -- lifetime
    def close(self):
        if self._h:
            lib().rsbwt_close(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def handle(self):
        return self._h

    # -- class BWT (include/bwt/bwt.h:6-15)
    def getBWLen(self):
        return lib().rsbwt_bwlen(self._h)

    def getPC(self, b):
        return lib().rsbwt_pc(self._h, b.encode() if isinstance(b, str) else b)

    def getF(self, index):
        return lib().rsbwt_f(self._h, index).decode()

    def getOcc(self, b, index):
        out = C.c_uint64()
        check(lib().rsbwt_occ(self._h, b.encode() if isinstance(b, str) else b,
                              index & 0xFFFFFFFFFFFFFFFF, C.byref(out)))
        return out.value

    def getChar(self, index):
        out = C.create_string_buffer(1)
        check(lib().rsbwt_char(self._h, index, out))
        return out.raw.decode()

    def getOccAt(self, b, bc):
        out = C.c_uint64()
        check(lib().rsbwt_occ_at(self._h, b.encode() if isinstance(b, str) else b, bc, C.byref(out)))
        return out.value

    # -- batched forms
    def occ_batch(self, syms, index):
        s = np.ascontiguousarray(np.frombuffer(syms.encode() if isinstance(syms, str) else bytes(syms),
                                               dtype=np.uint8))
        idx = np.ascontiguousarray(index, dtype=np.uint64)
        if s.size == 1 and idx.size > 1:
            s = np.repeat(s, idx.size)
        out = np.empty(idx.size, np.uint64)
        check(lib().rsbwt_occ_batch(self._h, _ptr(s), _ptr(idx), idx.size, _ptr(out)))
        return out

    def char_batch(self, index):
        idx = np.ascontiguousarray(index, dtype=np.uint64)
        out = np.empty(idx.size, np.uint8)
        check(lib().rsbwt_char_batch(self._h, _ptr(idx), idx.size, _ptr(out)))
        return out

    def occ_at_batch(self, syms, bc):
        s = np.ascontiguousarray(np.frombuffer(syms.encode() if isinstance(syms, str) else bytes(syms),
                                               dtype=np.uint8))
        c = np.ascontiguousarray(bc, dtype=np.uint64)
        if s.size == 1 and c.size > 1:
            s = np.repeat(s, c.size)
        out = np.empty(c.size, np.uint64)
        check(lib().rsbwt_occ_at_batch(self._h, _ptr(s), _ptr(c), c.size, _ptr(out)))
        return out

    # -- shape
    def num_runs(self):
        return lib().rsbwt_num_runs(self._h)

    def num_strings(self):
        return lib().rsbwt_num_strings(self._h)

    def num_lines(self):
        return lib().rsbwt_num_lines(self._h)

    def ktab_depth(self):
        return lib().rsbwt_ktab_depth(self._h)

    def ktab_info(self):
        """(format, bytes, untabulated): 0 = plain / 1 = grouped, the table's HBM bytes, the T-mers a grouped table
        leaves to the search (rsbwt_ktab_info)."""
        f, b, u = C.c_uint32(), C.c_uint64(), C.c_uint64()
        check(lib().rsbwt_ktab_info(self._h, C.byref(f), C.byref(b), C.byref(u)))
        return f.value, b.value, u.value

    def window_span(self):
        return lib().rsbwt_window_span(self._h)

    def far_lines(self):
        return lib().rsbwt_far_lines(self._h)

    def spilled_symbols(self):
        return lib().rsbwt_spilled_symbols(self._h)

    def hbm_bytes(self):
        return lib().rsbwt_hbm_bytes(self._h)

    def locate(self, rows, max_steps=0):
        """(read_row, ordinal, offset) of SA rows (rsbwt_locate): the row of the read's full suffix, the read's number
        among the shard's reads (Occ('$', read_row) - 1) and where the row's suffix starts in the read.  A row past the
        index, or one whose walk needs more than max_steps LF steps (0 = 2^20), gets 2^64-1 / 2^64-1 / 2^32-1."""
        r = np.ascontiguousarray(rows, dtype=np.uint64).ravel()
        rr, od, of = np.empty(r.size, np.uint64), np.empty(r.size, np.uint64), np.empty(r.size, np.uint32)
        check(lib().rsbwt_locate(self.handle, _ptr(r), r.size, max_steps, _ptr(rr), _ptr(od), _ptr(of)))
        return rr, od, of

    def match_lengths(self, queries, max_len=0, min_rows=1, intervals=False):
        """Matching statistics of this shard (rsbwt_match_lengths): len, a uint32 array over the positions of the queries
        laid back to back -- the longest string ending at each position that occurs in at least max(min_rows, 1) rows, at
        most max_len symbols long (0 = no cap); intervals=True: (len, lower, upper) with findInterval of that string,
        (1, 0) where len is 0.  ShardSet.match_last_work() tells the work."""
        text, off = ShardSet._var_text(queries)
        N = int(off[-1])
        ln = np.zeros(N, np.uint32)
        lo, up = (np.zeros(N, np.uint64), np.zeros(N, np.uint64)) if intervals else (None, None)
        check(lib().rsbwt_match_lengths(self.handle, _ptr(text), _ptr(off), len(queries), max_len, min_rows, _ptr(ln),
                                        _ptr(lo) if intervals else None, _ptr(up) if intervals else None))
        return (ln, lo, up) if intervals else ln

    def overlaps(self, queries, min_overlap, max_overlap=0, ordinals=False):
        """The reads of this shard that begin with a suffix of a query (rsbwt_overlaps): count, a uint64 array over the
        positions of the queries laid back to back -- position t names the suffix of its query that starts there, count[t]
        the reads beginning with it when it has min_overlap symbols or more (and at most max_overlap, 0 = no limit), else
        0; ordinals=True: (count, ordinal), the reads being the rsbwt_locate ordinals [ordinal, ordinal + count).
        ShardSet.overlap_last_work() tells the work."""
        text, off = ShardSet._var_text(queries)
        N = int(off[-1])
        cnt = np.zeros(N, np.uint64)
        od = np.zeros(N, np.uint64) if ordinals else None
        check(lib().rsbwt_overlaps(self.handle, _ptr(text), _ptr(off), len(queries), min_overlap, max_overlap, _ptr(cnt),
                                   _ptr(od) if ordinals else None))
        return (cnt, od) if ordinals else cnt

    def extensions(self, queries, ctx, left=False, both_strands=False):
        """Extension counts of this shard (rsbwt_extensions): a uint64 array of shape (Q, 4) -- the rows of the query's
        context of ctx symbols with A, C, G, T put behind it (left=True: in front of it), the reverse complement's rows
        added with both_strands; zeros for a query shorter than ctx or with a symbol outside ACGT in its context.
        ShardSet.walk_last_work() tells the work."""
        text, off = ShardSet._var_text(queries)
        cnt = np.zeros((len(queries), 4), np.uint64)
        check(lib().rsbwt_extensions(self.handle, _ptr(text), _ptr(off), len(queries), ctx, _walk_flags(left, both_strands), _ptr(cnt)))
        return cnt

    @property
    def exactmatch_by_search(self):
        """True: query_exactmatch on this shard answers by backward search from the terminator rows
        (rsbwt_exactmatch_by_search) instead of extracting and comparing reads."""
        return bool(lib().rsbwt_exactmatch_is_by_search(self._h))

    @exactmatch_by_search.setter
    def exactmatch_by_search(self, on):
        check(lib().rsbwt_exactmatch_by_search(self._h, 1 if on else 0))


# ---- query.h (src/bwt/query.cpp) ------------------------------------------------------------

def find_intervals(pBWT, kmers):
    """Batched findInterval (query.cpp:24-41): returns (lower, upper) uint64 arrays."""
    a, k = _kmer_matrix(kmers)
    Q = a.shape[0]
    lower = np.empty(Q, np.uint64)
    upper = np.empty(Q, np.uint64)
    check(lib().rsbwt_find_intervals(pBWT.handle, _ptr(a), Q, k, max(k, 1), _ptr(lower), _ptr(upper)))
    return lower, upper


def count_kmers(pBWT, kmers):
    """Batched count of count_reads (src/service/service.cpp:303-304)."""
    a, k = _kmer_matrix(kmers)
    Q = a.shape[0]
    out = np.empty(Q, np.uint64)
    check(lib().rsbwt_count(pBWT.handle, _ptr(a), Q, k, max(k, 1), _ptr(out)))
    return out


def read_copies(pBWT, kmers):
    """Whole-read matches by backward search from the terminator rows (rsbwt_read_copies): (copies, ending) uint64
    arrays -- how many indexed reads equal each k-mer, and how many end with it."""
    a, k = _kmer_matrix(kmers)
    Q = a.shape[0]
    copies = np.empty(Q, np.uint64)
    ending = np.empty(Q, np.uint64)
    check(lib().rsbwt_read_copies(pBWT.handle, _ptr(a), Q, k, max(k, 1), _ptr(copies), _ptr(ending)))
    return copies, ending


def find_intervals_1mm(pBWT, kmers):
    """1-mismatch search by composition: (lower, upper) of shape (Q, 3k+1); column 0 is the k-mer
    itself, column 1 + 3i + d position i with the d-th base of ACGT minus the original."""
    a, k = _kmer_matrix(kmers)
    Q = a.shape[0]
    lower = np.empty((Q, 3 * k + 1), np.uint64)
    upper = np.empty((Q, 3 * k + 1), np.uint64)
    check(lib().rsbwt_find_intervals_1mm(pBWT.handle, _ptr(a), Q, k, max(k, 1), _ptr(lower), _ptr(upper)))
    return lower, upper


HIT_1MM = np.dtype([("lower", "<u8"), ("upper", "<u8"), ("query", "<u4"), ("pos", "<i2"), ("base", "S1"),
                    ("reserved", "u1")])  # = rsbwt_hit_1mm
SMEM = np.dtype([("query", "<u8"), ("shard", "<u4"), ("start", "<u4"), ("end", "<u4"), ("reserved", "<u4"), ("lower", "<u8"),
                 ("upper", "<u8")])  # = rsbwt_smem
OVERLAP = np.dtype([("query", "<u8"), ("shard", "<u4"), ("start", "<u4"), ("length", "<u4"), ("reserved", "<u4"), ("ordinal", "<u8"),
                    ("count", "<u8"), ("lower", "<u8"), ("upper", "<u8")])  # = rsbwt_overlap
GT_LEG = np.dtype([("query", "<u8"), ("tile", "<u4"), ("leg", "<u4"), ("shard", "<u4"), ("a", "<u4"), ("b", "<u4"), ("reserved", "<u4"),
                   ("lower", "<u8"), ("upper", "<u8")])  # = rsbwt_gt_leg


def hits_1mm_batch(pBWT, kmers, cap=None):
    """1-mismatch search with SURVEY 8 f3's output: a structured array (HIT_1MM) of the variants
    that occur, sorted by (query, pos, base); pos = -1 / base = b'' for the k-mer itself."""
    a, k = _kmer_matrix(kmers)
    Q = a.shape[0]
    cap = int(cap) if cap is not None else max(1024, 4 * Q)
    while True:
        out = np.zeros(cap, HIT_1MM)
        n = C.c_size_t()
        rc = lib().rsbwt_hits_1mm(pBWT.handle, _ptr(a), Q, k, max(k, 1), _ptr(out), cap, C.byref(n))
        if rc == -7 and n.value > cap:  # RSBWT_ERANGE: the list is longer than the buffer
            cap = n.value
            continue
        check(rc)
        return out[:n.value]


def hits_1mm(kmer, lower_row, upper_row):
    """The sorted list of (pos, base, lower, upper) of the non-empty variants of one k-mer
    (pos = -1 for the exact hit), from one row of find_intervals_1mm."""
    out = []
    if upper_row[0] >= lower_row[0]:
        out.append((-1, "", int(lower_row[0]), int(upper_row[0])))
    for v in range(1, len(lower_row)):
        if upper_row[v] >= lower_row[v]:
            pos, d = (v - 1) // 3, (v - 1) % 3
            alt = [c for c in "ACGT" if c != kmer[pos]][d]
            out.append((pos, alt, int(lower_row[v]), int(upper_row[v])))
    return out


def findInterval(pBWT, w):
    """BWTInterval findInterval(const BWT*, const std::string& w) (query.cpp:24-41)."""
    lo, up = find_intervals(pBWT, [w])
    return BWTInterval(int(lo[0]), int(up[0]))


def extractPrefix(pBWT, index, limit=1 << 16):
    """query.cpp:43-63: LF-walk left from row `index` until '$'."""
    out = []
    idx = index
    while True:
        b = pBWT.getChar(idx)
        if b == "$":
            break
        if len(out) >= limit:
            raise RsbwtError(-1, "extractPrefix did not meet '$'")
        idx = pBWT.getPC(b) + pBWT.getOcc(b, idx - 1)
        out.append(b)
    return "".join(reversed(out))


def extractPostfix(pBWT, index, limit=1 << 16):
    """query.cpp:65-85: F/select walk right from row `index` until '$'."""
    out = []
    idx = index
    while True:
        f = pBWT.getF(idx)
        if f == "$":
            break
        if len(out) >= limit:
            raise RsbwtError(-1, "extractPostfix did not meet '$'")
        fc = idx - pBWT.getPC(f) + 1
        idx = pBWT.getOccAt(f, fc)
        out.append(f)
    return "".join(out)


def extract_reads(pBWT, rows, stride=512):
    """Batched extractPrefix(row) + extractPostfix(row) (query.cpp:43-85) on the GPU: returns
    (list of read strings, prefix lengths)."""
    r = np.ascontiguousarray(rows, dtype=np.uint64)
    out = np.zeros((r.size, stride), np.uint8)
    ln = np.empty(r.size, np.uint32)
    pl = np.empty(r.size, np.uint32)
    check(lib().rsbwt_extract(pBWT.handle, _ptr(r), r.size, _ptr(out), stride, _ptr(ln), _ptr(pl)))
    if (ln == 0xFFFFFFFF).any():
        raise RsbwtError(-1, "a read does not fit the stride / a row is out of range")
    return [out[i, :ln[i]].tobytes().decode() for i in range(r.size)], pl


def query_batch(pBWT, kmers, read_stride=256):
    """Batched query (query.cpp:87-100) through rsbwt_query: a list, per k-mer, of the reads that
    contain it, in SA-row order."""
    a, k = _kmer_matrix(kmers)
    Q = a.shape[0]
    first = np.zeros(Q + 1, np.uint64)
    n = C.c_size_t()
    rc = lib().rsbwt_query(pBWT.handle, _ptr(a), Q, k, max(k, 1), _ptr(first), None, read_stride, None, 0, C.byref(n))
    if rc not in (0, -7):
        check(rc)
    total = n.value
    reads = np.zeros((max(total, 1), read_stride), np.uint8)
    ln = np.zeros(max(total, 1), np.uint32)
    if total:
        check(lib().rsbwt_query(pBWT.handle, _ptr(a), Q, k, max(k, 1), _ptr(first), _ptr(reads), read_stride, _ptr(ln),
                                total, C.byref(n)))
        if (ln[:total] == 0xFFFFFFFF).any():
            raise RsbwtError(-1, "a read does not fit read_stride")
    out = []
    for q in range(Q):
        out.append([reads[r, :ln[r]].tobytes().decode() for r in range(int(first[q]), int(first[q + 1]))])
    return out


def query_exactmatch_batch(pBWT, kmers):
    """Batched query_exactmatch (query.cpp:102-120) through rsbwt_query_exactmatch: bool array."""
    a, k = _kmer_matrix(kmers)
    Q = a.shape[0]
    found = np.zeros(Q, np.uint8)
    check(lib().rsbwt_query_exactmatch(pBWT.handle, _ptr(a), Q, k, max(k, 1), _ptr(found)))
    return found.astype(bool)


def query(pBWT, w):
    """vector<string> query(const BWT*, const string& w) (query.cpp:87-100): every read containing w."""
    if len(w) == 0:
        return []
    return query_batch(pBWT, [w])[0]


def query_exactmatch(pBWT, w):
    """bool query_exactmatch(const BWT*, const string& w) (query.cpp:102-120): is w itself a read."""
    if len(w) == 0:
        return False
    return bool(query_exactmatch_batch(pBWT, [w])[0])


# ---- SiteMatch alignment (csrc/ksw_align.hip): ksw_align of src/service/ksw.c and align_gt_read over it -----------

KSW_SERVICE = (1, 4, 1, 6, 1)  # match, mismatch, ambiguous, gapo, gape: what align_gt_read aligns with
KSW_LDS_ROWS, KSW_MAX_LEN = 224, 4096
GT_KEEP = (9, 11, 13)          # RSBWT_GT_KEEP_PLAIN / _RIGHT / _LEFT: the exits of align_gt_read that keep the read


def _texts(seqs):
    bs = [s if isinstance(s, (bytes, bytearray)) else str(s).encode("latin-1") for s in seqs]
    off = np.zeros(len(bs) + 1, np.uint64)
    off[1:] = np.cumsum([len(b) for b in bs], dtype=np.uint64)
    return np.frombuffer(b"".join(bs) + b"\0", np.uint8).copy(), off


def ksw_align(pairs, params=None, device=0):
    """pairs of (query, target) -> int32 (n, 5): score, te, qe, tb, qb of ksw_align(..., KSW_XSTART, 0) with the query on
    the rows; params = (match, mismatch, ambiguous, gapo, gape), None = the service's (rsbwt_ksw_align)"""
    qtext, qoff = _texts([p[0] for p in pairs])
    ttext, toff = _texts([p[1] for p in pairs])
    n = len(pairs)
    out = np.zeros((max(n, 1), 6), np.int32)
    prm = None if params is None else np.ascontiguousarray(params, np.int32)
    if prm is not None and prm.shape != (5,):
        raise ValueError("params: (match, mismatch, ambiguous, gapo, gape)")
    check(lib().rsbwt_ksw_align(device, None if prm is None else _ptr(prm), _ptr(qtext), _ptr(qoff), _ptr(ttext), _ptr(toff), n, _ptr(out)))
    return out[:n, :5].copy()


def gt_align(reads, item, requests, device=0):
    """verdict u8[n]: the exit of align_gt_read(read i, w, pos, alt, isalt) for requests[item[i]] = (w, pos, alt, isalt),
    one of RSBWT_GT_* (GT_KEEP = the read stays) (rsbwt_gt_align)"""
    rtext, roff = _texts(reads)
    text, off = _texts([r[0] for r in requests])
    n, Q = len(reads), len(requests)
    pos, alt, isalt = ShardSet._gt_requests([r[0] for r in requests], [r[1] for r in requests], [r[2] for r in requests],
                                            [1 if r[3] else 0 for r in requests])
    it = np.ascontiguousarray(item, np.uint64)
    if len(it) != n:
        raise ValueError("item needs one entry per read")
    pad = lambda a: a if len(a) else np.zeros(1, a.dtype)  # noqa: E731
    out = np.zeros(max(n, 1), np.uint8)
    check(lib().rsbwt_gt_align(device, _ptr(rtext), _ptr(roff), _ptr(pad(it)), n, _ptr(text), _ptr(off), _ptr(pad(pos)), _ptr(pad(alt)),
                               _ptr(pad(isalt)), Q, _ptr(out)))
    return out[:n].copy()


def gt_align_last_work():
    """{reads, by_verdict: {1..13: reads}} of this thread's last host-buffer verdict call"""
    w = np.zeros(14, np.uint64)
    lib().rsbwt_gt_align_last_work(w.ctypes.data_as(C.POINTER(C.c_uint64)))
    return dict(reads=int(w[0]), by_verdict={v: int(w[v]) for v in range(1, 14)})


# ---- shard sets -----------------------------------------------------------------

class ShardSet:
    """The shards held by one process; every query is searched in all of them (the reference
    broadcasts each request to all partitions: src/service/server.cpp:124,578)."""

    def __init__(self, shards):
        self.shards = list(shards)
        arr = (C.c_void_p * len(self.shards))(*[s.handle for s in self.shards])
        self._s = C.c_void_p()
        check(lib().rsbwt_set_from_handles(arr, len(self.shards), C.byref(self._s)))

    def close(self):
        if self._s:
            lib().rsbwt_set_close(self._s)
            self._s = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def find_intervals(self, kmers):
        a, k = _kmer_matrix(kmers)
        Q, S = a.shape[0], len(self.shards)
        lower = np.empty((S, Q), np.uint64)
        upper = np.empty((S, Q), np.uint64)
        check(lib().rsbwt_set_find_intervals(self._s, _ptr(a), Q, k, max(k, 1), _ptr(lower), _ptr(upper)))
        return lower, upper

    def count(self, kmers):
        a, k = _kmer_matrix(kmers)
        out = np.empty(a.shape[0], np.uint64)
        check(lib().rsbwt_set_count(self._s, _ptr(a), a.shape[0], k, max(k, 1), _ptr(out)))
        return out

    # -- queries of lengths of their own in one call (a window of the service loop): rsbwt_set_*_var
    @staticmethod
    def _var_text(queries):
        bs = [q if isinstance(q, (bytes, bytearray)) else str(q).encode() for q in queries]
        off = np.zeros(len(bs) + 1, np.uint64)
        off[1:] = np.cumsum([len(b) for b in bs], dtype=np.uint64)
        text = np.frombuffer(b"".join(bs) + b"\0", np.uint8).copy()
        return text, off

    def find_intervals_var(self, queries):
        text, off = self._var_text(queries)
        Q, S = len(queries), len(self.shards)
        lower = np.empty((S, Q), np.uint64)
        upper = np.empty((S, Q), np.uint64)
        check(lib().rsbwt_set_find_intervals_var(self._s, _ptr(text), _ptr(off), Q, _ptr(lower), _ptr(upper)))
        return lower, upper

    def count_var(self, queries):
        text, off = self._var_text(queries)
        out = np.empty(len(queries), np.uint64)
        check(lib().rsbwt_set_count_var(self._s, _ptr(text), _ptr(off), len(queries), _ptr(out)))
        return out

    def read_copies_var(self, queries):
        """(copies, ending) of shape (shards, Q): per shard, how many of its reads equal / end with each query
        (rsbwt_set_read_copies_var)"""
        text, off = self._var_text(queries)
        Q, S = len(queries), len(self.shards)
        copies = np.empty((S, Q), np.uint64)
        ending = np.empty((S, Q), np.uint64)
        check(lib().rsbwt_set_read_copies_var(self._s, _ptr(text), _ptr(off), Q, _ptr(copies), _ptr(ending)))
        return copies, ending

    def exactmatch_by_search(self, on):
        """rsbwt_query_exactmatch of every shard of the set by search (True) or by extraction (False, the default)"""
        check(lib().rsbwt_set_exactmatch_by_search(self._s, 1 if on else 0))

    def query_var(self, queries, read_stride=256):
        """per query: [(shard, read)] of every read containing it, shard 0's first (rsbwt_set_query_var)"""
        text, off = self._var_text(queries)
        Q = len(queries)
        first = np.zeros(Q + 1, np.uint64)
        n = C.c_size_t()
        rc = lib().rsbwt_set_query_var(self._s, _ptr(text), _ptr(off), Q, _ptr(first), None, None, read_stride, None, 0, C.byref(n))
        if rc not in (0, -7):
            check(rc)
        total = n.value
        reads = np.zeros((max(total, 1), read_stride), np.uint8)
        ln = np.zeros(max(total, 1), np.uint32)
        sh = np.zeros(max(total, 1), np.uint32)
        if total:
            check(lib().rsbwt_set_query_var(self._s, _ptr(text), _ptr(off), Q, _ptr(first), _ptr(sh), _ptr(reads), read_stride, _ptr(ln), total, C.byref(n)))
            if (ln[:total] == 0xFFFFFFFF).any():
                raise RsbwtError(-1, "a read does not fit read_stride")
        return [[(int(sh[r]), reads[r, :ln[r]].tobytes().decode()) for r in range(int(first[q]), int(first[q + 1]))] for q in range(Q)]

    def query_var_capped(self, queries, max_rows, read_stride=256):
        """(reads, matches): reads[q][shard] = the reads containing query q that shard holds, in SA-row order -- none for a
        query whose rows over all shards exceed max_rows (0 = no limit); matches[q] = that number of rows, over the
        limit or not (rsbwt_set_query_var_capped)"""
        text, off = self._var_text(queries)
        Q, S = len(queries), len(self.shards)
        first = np.zeros(Q + 1, np.uint64)
        matches = np.zeros(max(Q, 1), np.uint64)
        n = C.c_size_t()
        rc = lib().rsbwt_set_query_var_capped(self._s, _ptr(text), _ptr(off), Q, max_rows, _ptr(first), None, None, read_stride, None, 0,
                                              C.byref(n), _ptr(matches))
        if rc not in (0, -7):
            check(rc)
        total = n.value
        reads = np.zeros((max(total, 1), read_stride), np.uint8)
        ln = np.zeros(max(total, 1), np.uint32)
        sh = np.zeros(max(total, 1), np.uint32)
        if total:
            check(lib().rsbwt_set_query_var_capped(self._s, _ptr(text), _ptr(off), Q, max_rows, _ptr(first), _ptr(sh), _ptr(reads), read_stride,
                                                   _ptr(ln), total, C.byref(n), _ptr(matches)))
            if (ln[:total] == 0xFFFFFFFF).any():
                raise RsbwtError(-1, "a read does not fit read_stride")
        out = [[[] for _ in range(S)] for _ in range(Q)]
        for q in range(Q):
            for r in range(int(first[q]), int(first[q + 1])):
                out[q][int(sh[r])].append(reads[r, :ln[r]].tobytes().decode())
        return out, matches[:Q].copy()

    def kmer_reads(self, queries, k, skip=0, min_read_length=73, max_read_length=100, read_stride=256):
        """KmerMatch / Reads (find_kmer_reads, src/service/service.cpp:466-502) of every query in every shard: [query][shard]
        -> the distinct reads, in the reference's unordered_set order (rsbwt_set_kmer_reads)"""
        text, off = self._var_text(queries)
        Q, S = len(queries), len(self.shards)
        first = np.zeros(Q * S + 1, np.uint64)
        n = C.c_size_t()
        rc = lib().rsbwt_set_kmer_reads(self._s, _ptr(text), _ptr(off), Q, k, skip, min_read_length, max_read_length, _ptr(first), None,
                                        read_stride, None, 0, C.byref(n))
        if rc not in (0, -7):
            check(rc)
        total = n.value
        reads = np.zeros((max(total, 1), read_stride), np.uint8)
        ln = np.zeros(max(total, 1), np.uint32)
        if total:
            check(lib().rsbwt_set_kmer_reads(self._s, _ptr(text), _ptr(off), Q, k, skip, min_read_length, max_read_length, _ptr(first),
                                             _ptr(reads), read_stride, _ptr(ln), total, C.byref(n)))
            if (ln[:total] == 0xFFFFFFFF).any():
                raise RsbwtError(-1, "a read does not fit read_stride")
        return [[[reads[r, :ln[r]].tobytes().decode() for r in range(int(first[q * S + p]), int(first[q * S + p + 1]))] for p in range(S)]
                for q in range(Q)]

    def kmer_count(self, queries, k, skip=0, min_read_length=73, max_read_length=100):
        """KmerMatch / Count: [query][shard] -> the number of distinct reads (rsbwt_set_kmer_count)"""
        text, off = self._var_text(queries)
        Q, S = len(queries), len(self.shards)
        out = np.zeros(Q * S, np.uint64)
        check(lib().rsbwt_set_kmer_count(self._s, _ptr(text), _ptr(off), Q, k, skip, min_read_length, max_read_length, _ptr(out)))
        return out.reshape(Q, S)

    @staticmethod
    def kmer_last_work():
        """{candidates, walked, lf_steps, identities, extracted} of this thread's last kmer call"""
        w = np.zeros(5, np.uint64)
        lib().rsbwt_set_kmer_last_work(w.ctypes.data_as(C.POINTER(C.c_uint64)))
        return dict(zip(("candidates", "walked", "lf_steps", "identities", "extracted"), (int(x) for x in w)))

    @staticmethod
    def kmer_last_times():
        """{total_ms, device_ms, host_ms} of this thread's last kmer call (device_ms: inside the calls that wait for the GPU)"""
        t = (C.c_double * 3)()
        lib().rsbwt_set_kmer_last_times(t)
        return dict(total_ms=t[0], device_ms=t[1], host_ms=t[2])

    # -- SiteMatch candidates (find_gt_reads, src/service/service.cpp:507-711): rsbwt_set_gt_*
    def gt_legs(self, queries, pos, k, skip=0, max_interval_size=0):
        """per query: the legs of its tiles as (tile, leg, shard, a, b, lower, upper), ordered by (tile, leg, shard): the
        final string of a leg is query[a:b), its interval in that shard [lower, upper]; leg 0 = the tile itself, 1 / 2 =
        the lengthened legs (rsbwt_set_gt_legs)"""
        text, off = self._var_text(queries)
        Q = len(queries)
        p = np.ascontiguousarray(pos, np.uint64)
        first = np.zeros(Q + 1, np.uint64)
        n = C.c_size_t()
        rc = lib().rsbwt_set_gt_legs(self._s, _ptr(text), _ptr(off), Q, _ptr(p), k, skip, max_interval_size, _ptr(first), None, 0, C.byref(n))
        if rc not in (0, -7):
            check(rc)
        total = n.value
        legs = np.zeros(max(total, 1), GT_LEG)
        if total:
            check(lib().rsbwt_set_gt_legs(self._s, _ptr(text), _ptr(off), Q, _ptr(p), k, skip, max_interval_size, _ptr(first), _ptr(legs), total,
                                          C.byref(n)))
        return [[(int(r["tile"]), int(r["leg"]), int(r["shard"]), int(r["a"]), int(r["b"]), int(r["lower"]), int(r["upper"]))
                 for r in legs[int(first[q]):int(first[q + 1])]] for q in range(Q)]

    def gt_reads(self, queries, pos, k, skip=0, max_interval_size=0, read_stride=256, with_rows=False):
        """[query][shard] -> the distinct reads over the rows the span filter keeps, ascending read_row (with_rows: (read_row,
        read) pairs) (rsbwt_set_gt_reads)"""
        text, off = self._var_text(queries)
        Q, S = len(queries), len(self.shards)
        p = np.ascontiguousarray(pos, np.uint64)
        first = np.zeros(Q * S + 1, np.uint64)
        n = C.c_size_t()
        rc = lib().rsbwt_set_gt_reads(self._s, _ptr(text), _ptr(off), Q, _ptr(p), k, skip, max_interval_size, _ptr(first), None, read_stride, None,
                                      None, 0, C.byref(n))
        if rc not in (0, -7):
            check(rc)
        total = n.value
        reads = np.zeros((max(total, 1), read_stride), np.uint8)
        ln = np.zeros(max(total, 1), np.uint32)
        rr = np.zeros(max(total, 1), np.uint64)
        if total:
            check(lib().rsbwt_set_gt_reads(self._s, _ptr(text), _ptr(off), Q, _ptr(p), k, skip, max_interval_size, _ptr(first), _ptr(reads),
                                           read_stride, _ptr(ln), _ptr(rr), total, C.byref(n)))
            if (ln[:total] == 0xFFFFFFFF).any():
                raise RsbwtError(-1, "a read does not fit read_stride")

        def one(r):
            t = reads[r, :ln[r]].tobytes().decode()
            return (int(rr[r]), t) if with_rows else t
        return [[[one(r) for r in range(int(first[q * S + s]), int(first[q * S + s + 1]))] for s in range(S)] for q in range(Q)]

    def gt_count(self, queries, pos, k, skip=0, max_interval_size=0):
        """[query][shard] -> the number of those reads (rsbwt_set_gt_count)"""
        text, off = self._var_text(queries)
        Q, S = len(queries), len(self.shards)
        p = np.ascontiguousarray(pos, np.uint64)
        out = np.zeros(Q * S, np.uint64)
        check(lib().rsbwt_set_gt_count(self._s, _ptr(text), _ptr(off), Q, _ptr(p), k, skip, max_interval_size, _ptr(out)))
        return out.reshape(Q, S)

    @staticmethod
    def gt_last_work():
        """{legs, no_answer, narrow_steps, candidates, kept, extracted} of this thread's last gt call"""
        w = np.zeros(6, np.uint64)
        lib().rsbwt_set_gt_last_work(w.ctypes.data_as(C.POINTER(C.c_uint64)))
        return dict(zip(("legs", "no_answer", "narrow_steps", "candidates", "kept", "extracted"), (int(x) for x in w)))

    # -- SiteMatch reads that align_gt_read keeps (csrc/ksw_align.hip): rsbwt_set_gt_aligned_*
    @staticmethod
    def _gt_requests(queries, pos, alt, isalt):
        Q = len(queries)
        a = np.frombuffer(b"".join((x if isinstance(x, bytes) else str(x).encode("latin-1"))[:1] or b"\0" for x in alt), np.uint8).copy()
        if len(a) != Q or len(isalt) != Q or len(pos) != Q:
            raise ValueError("pos, alt and isalt need one entry per query")
        return np.ascontiguousarray(pos, np.uint64), a, np.ascontiguousarray(isalt, np.uint8)

    def gt_aligned_reads(self, queries, pos, alt, isalt, k, skip=0, max_interval_size=0, read_stride=256, with_rows=False):
        """gt_reads cut down to the reads align_gt_read keeps against (query, pos, alt, isalt): [query][shard] -> reads,
        ascending read_row (rsbwt_set_gt_aligned_reads)"""
        text, off = self._var_text(queries)
        Q, S = len(queries), len(self.shards)
        p, a, ia = self._gt_requests(queries, pos, alt, isalt)
        first = np.zeros(Q * S + 1, np.uint64)
        n = C.c_size_t()
        rc = lib().rsbwt_set_gt_aligned_reads(self._s, _ptr(text), _ptr(off), Q, _ptr(p), _ptr(a), _ptr(ia), k, skip, max_interval_size, _ptr(first),
                                              None, read_stride, None, None, 0, C.byref(n))
        if rc not in (0, -7):
            check(rc)
        total = n.value
        reads = np.zeros((max(total, 1), read_stride), np.uint8)
        ln = np.zeros(max(total, 1), np.uint32)
        rr = np.zeros(max(total, 1), np.uint64)
        if total:
            check(lib().rsbwt_set_gt_aligned_reads(self._s, _ptr(text), _ptr(off), Q, _ptr(p), _ptr(a), _ptr(ia), k, skip, max_interval_size,
                                                   _ptr(first), _ptr(reads), read_stride, _ptr(ln), _ptr(rr), total, C.byref(n)))
            if (ln[:total] == 0xFFFFFFFF).any():
                raise RsbwtError(-1, "a read does not fit read_stride")

        def one(r):
            t = reads[r, :ln[r]].tobytes().decode()
            return (int(rr[r]), t) if with_rows else t
        return [[[one(r) for r in range(int(first[q * S + s]), int(first[q * S + s + 1]))] for s in range(S)] for q in range(Q)]

    def gt_aligned_count(self, queries, pos, alt, isalt, k, skip=0, max_interval_size=0):
        """[query][shard] -> the number of those reads (rsbwt_set_gt_aligned_count)"""
        text, off = self._var_text(queries)
        Q, S = len(queries), len(self.shards)
        p, a, ia = self._gt_requests(queries, pos, alt, isalt)
        out = np.zeros(Q * S, np.uint64)
        check(lib().rsbwt_set_gt_aligned_count(self._s, _ptr(text), _ptr(off), Q, _ptr(p), _ptr(a), _ptr(ia), k, skip, max_interval_size, _ptr(out)))
        return out.reshape(Q, S)

    # -- matching statistics (csrc/match_stats.hip): rsbwt_set_match_lengths / rsbwt_set_smems
    def match_lengths(self, queries, max_len=0, min_rows=1, intervals=False):
        """len of shape (shards, N), N the positions of the queries laid back to back: per shard the longest string ending
        at each position that occurs in at least max(min_rows, 1) rows, at most max_len symbols long (0 = no cap);
        intervals=True: (len, lower, upper) with findInterval of that string, (1, 0) where len is 0
        (rsbwt_set_match_lengths)"""
        text, off = self._var_text(queries)
        S, N = len(self.shards), int(off[-1])
        ln = np.zeros((S, N), np.uint32)
        lo, up = (np.zeros((S, N), np.uint64), np.zeros((S, N), np.uint64)) if intervals else (None, None)
        check(lib().rsbwt_set_match_lengths(self._s, _ptr(text), _ptr(off), len(queries), max_len, min_rows, _ptr(ln),
                                            _ptr(lo) if intervals else None, _ptr(up) if intervals else None))
        return (ln, lo, up) if intervals else ln

    def smems(self, queries, max_len=0, min_rows=1, raw=False):
        """[query][shard] -> the super-maximal exact matches as (start, end, lower, upper), ascending end: query[start:end)
        is a longest match that no neighbouring position's match contains, [lower, upper] its interval in that shard;
        raw=True: (SMEM array ordered by (query, shard, end), first) as rsbwt_set_smems writes them"""
        text, off = self._var_text(queries)
        Q, S = len(queries), len(self.shards)
        first = np.zeros(Q * S + 1, np.uint64)
        n = C.c_size_t()
        rc = lib().rsbwt_set_smems(self._s, _ptr(text), _ptr(off), Q, max_len, min_rows, _ptr(first), None, 0, C.byref(n))
        if rc not in (0, -7):
            check(rc)
        total = n.value
        out = np.zeros(max(total, 1), SMEM)
        if total:
            check(lib().rsbwt_set_smems(self._s, _ptr(text), _ptr(off), Q, max_len, min_rows, _ptr(first), _ptr(out), total, C.byref(n)))
        if raw:
            return out[:total], first
        return [[[(int(r["start"]), int(r["end"]), int(r["lower"]), int(r["upper"]))
                  for r in out[int(first[q * S + p]):int(first[q * S + p + 1])]] for p in range(S)] for q in range(Q)]

    @staticmethod
    def match_last_work():
        """{items, lf_steps, passes, table_starts, restarts, smems} of this thread's last matching-statistics call"""
        w = np.zeros(6, np.uint64)
        lib().rsbwt_set_match_last_work(w.ctypes.data_as(C.POINTER(C.c_uint64)))
        return dict(zip(("items", "lf_steps", "passes", "table_starts", "restarts", "smems"), (int(x) for x in w)))

    # -- overlaps (csrc/overlaps.hip): rsbwt_set_overlaps / rsbwt_set_overlap_records / rsbwt_set_overlap_reads
    def overlaps(self, queries, min_overlap, max_overlap=0, ordinals=False):
        """count of shape (shards, N), N the positions of the queries laid back to back: position t names the suffix of its
        query that starts there, count[p, t] the reads of shard p that begin with it when it has min_overlap symbols or
        more (and at most max_overlap, 0 = no limit), else 0; ordinals=True: (count, ordinal), the reads being the
        rsbwt_locate ordinals [ordinal, ordinal + count) of that shard (rsbwt_set_overlaps)"""
        text, off = self._var_text(queries)
        S, N = len(self.shards), int(off[-1])
        cnt = np.zeros((S, N), np.uint64)
        od = np.zeros((S, N), np.uint64) if ordinals else None
        check(lib().rsbwt_set_overlaps(self._s, _ptr(text), _ptr(off), len(queries), min_overlap, max_overlap, _ptr(cnt),
                                       _ptr(od) if ordinals else None))
        return (cnt, od) if ordinals else cnt

    def overlap_records(self, queries, min_overlap, max_overlap=0, raw=False):
        """[query][shard] -> the suffixes some read begins with as (start, length, ordinal, count, lower, upper), ascending
        start (the longest overlap first): query[start:start+length] opens the reads [ordinal, ordinal + count) of that
        shard, [lower, upper] is its interval; raw=True: (OVERLAP array ordered by (query, shard, start), first) as
        rsbwt_set_overlap_records writes them"""
        text, off = self._var_text(queries)
        Q, S = len(queries), len(self.shards)
        first = np.zeros(Q * S + 1, np.uint64)
        n = C.c_size_t()
        rc = lib().rsbwt_set_overlap_records(self._s, _ptr(text), _ptr(off), Q, min_overlap, max_overlap, _ptr(first), None, 0, C.byref(n))
        if rc not in (0, -7):
            check(rc)
        total = n.value
        out = np.zeros(max(total, 1), OVERLAP)
        if total:
            check(lib().rsbwt_set_overlap_records(self._s, _ptr(text), _ptr(off), Q, min_overlap, max_overlap, _ptr(first), _ptr(out), total,
                                                  C.byref(n)))
        if raw:
            return out[:total], first
        return [[[tuple(int(r[f]) for f in ("start", "length", "ordinal", "count", "lower", "upper"))
                  for r in out[int(first[q * S + p]):int(first[q * S + p + 1])]] for p in range(S)] for q in range(Q)]

    def overlap_reads(self, queries, min_overlap, max_overlap=0, max_reads=0, read_stride=256, raw=False):
        """(reads, matches): reads[q][shard] = [(overlap, ordinal, read)] of the reads of that shard that begin with a
        suffix of query q of min_overlap symbols or more, each once at its longest overlap, overlap descending then ordinal
        ascending -- none for a (query, shard) with more than max_reads of them (0 = no limit); matches of shape (Q,
        shards) = that number of distinct reads, over the limit or not; raw=True: (first, read strings, overlap, ordinal,
        matches) as rsbwt_set_overlap_reads writes them.  Every shard must be opened for reads."""
        text, off = self._var_text(queries)
        Q, S = len(queries), len(self.shards)
        first = np.zeros(Q * S + 1, np.uint64)
        matches = np.zeros(max(Q * S, 1), np.uint64)
        n = C.c_size_t()
        rc = lib().rsbwt_set_overlap_reads(self._s, _ptr(text), _ptr(off), Q, min_overlap, max_overlap, max_reads, _ptr(first), None,
                                           read_stride, None, None, None, 0, C.byref(n), _ptr(matches))
        if rc not in (0, -7):
            check(rc)
        total = n.value
        reads = np.zeros((max(total, 1), read_stride), np.uint8)
        ln = np.zeros(max(total, 1), np.uint32)
        ov = np.zeros(max(total, 1), np.uint32)
        od = np.zeros(max(total, 1), np.uint64)
        if total:
            check(lib().rsbwt_set_overlap_reads(self._s, _ptr(text), _ptr(off), Q, min_overlap, max_overlap, max_reads, _ptr(first),
                                                _ptr(reads), read_stride, _ptr(ln), _ptr(ov), _ptr(od), total, C.byref(n), _ptr(matches)))
            if (ln[:total] == 0xFFFFFFFF).any():
                raise RsbwtError(-1, "a read does not fit read_stride")
        strs = [reads[r, :ln[r]].tobytes().decode() for r in range(total)]
        m = matches[:Q * S].reshape(Q, S).copy()
        if raw:
            return first, strs, ov[:total], od[:total], m
        return [[[(int(ov[r]), int(od[r]), strs[r]) for r in range(int(first[q * S + p]), int(first[q * S + p + 1]))]
                 for p in range(S)] for q in range(Q)], m

    @staticmethod
    def overlap_last_work():
        """{items, lf_steps, passes, table_starts, dollar_only_passes, entries} of this thread's last overlap call"""
        w = np.zeros(6, np.uint64)
        lib().rsbwt_set_overlap_last_work(w.ctypes.data_as(C.POINTER(C.c_uint64)))
        return dict(zip(("items", "lf_steps", "passes", "table_starts", "dollar_only_passes", "entries"), (int(x) for x in w)))

    # -- extension counts and walks (csrc/walk.hip): rsbwt_set_extensions / rsbwt_set_walk
    def extensions(self, queries, ctx, left=False, both_strands=False):
        """counts of shape (shards, Q, 4): counts[p, q, c] = the rows in shard p of query q's context of ctx symbols with
        "ACGT"[c] put behind it (left=True: in front of it), the reverse complement's rows added with both_strands; zeros
        for a query shorter than ctx or with a symbol outside ACGT in its context (rsbwt_set_extensions)"""
        text, off = self._var_text(queries)
        cnt = np.zeros((len(self.shards), len(queries), 4), np.uint64)
        check(lib().rsbwt_set_extensions(self._s, _ptr(text), _ptr(off), len(queries), ctx, _walk_flags(left, both_strands), _ptr(cnt)))
        return cnt

    def walk(self, seeds, ctx, min_count=1, max_steps=256, left=False, both_strands=False, supports=False):
        """Walks every seed through the reads' k-mer graph (rsbwt_set_walk): while exactly one of the four extensions of
        the seed's context has a support -- its count summed over every shard -- of max(min_count, 1) or more, that symbol
        is appended (left=True: put in front).  Returns a list of (ext, stop, last) per seed: ext the appended symbols in
        the order they were appended (a left walk's sequence is ext[::-1] + seed), stop one of WALK_DEAD_END, WALK_BRANCH,
        WALK_LIMIT (max_steps symbols appended), WALK_INVALID (a seed shorter than ctx or with a symbol outside ACGT in its
        context), last the four supports of the evaluation that stopped the walk (zeros for LIMIT and INVALID);
        supports=True: (ext, stop, last, support) with the support of every appended symbol (saturated at 2^32 - 1)."""
        text, off = self._var_text(seeds)
        Q = len(seeds)
        ext = np.zeros((Q, max_steps), np.uint8)
        steps, stop = np.zeros(Q, np.uint32), np.zeros(Q, np.uint8)
        sup = np.zeros((Q, max_steps), np.uint32) if supports else None
        last = np.zeros((Q, 4), np.uint64)
        check(lib().rsbwt_set_walk(self._s, _ptr(text), _ptr(off), Q, ctx, min_count, max_steps, _walk_flags(left, both_strands), _ptr(ext),
                                   _ptr(steps), _ptr(stop), _ptr(sup) if supports else None, _ptr(last)))
        out = []
        for q in range(Q):
            n = int(steps[q])
            one = (ext[q, :n].tobytes().decode(), int(stop[q]), tuple(int(x) for x in last[q]))
            out.append(one + (tuple(int(x) for x in sup[q, :n]),) if supports else one)
        return out

    @staticmethod
    def walk_last_work():
        """{seeds, appended, searches, lf_steps, passes, table_starts} of this thread's last walk or extensions call"""
        w = np.zeros(6, np.uint64)
        lib().rsbwt_set_walk_last_work(w.ctypes.data_as(C.POINTER(C.c_uint64)))
        return dict(zip(("seeds", "appended", "searches", "lf_steps", "passes", "table_starts"), (int(x) for x in w)))

    # -- unitigs (csrc/walk.hip, unitig_kernel): rsbwt_set_unitigs
    def unitigs(self, seeds, ctx, min_count=1, max_steps=256, both_strands=False, supports=False):
        """The maximal unitig through every seed (rsbwt_set_unitigs): both sides walk from the seed as given, the right
        side from its last ctx symbols and the left side from its first, and a side stops where the graph forks onward
        (WALK_BRANCH), where another path joins the node it would enter (WALK_JOIN: the symbol is not appended), where the
        path ends (WALK_DEAD_END), after max_steps symbols on that side (WALK_LIMIT) or at once where its own context is
        missing or holds a symbol outside ACGT (WALK_INVALID).  Returns, per seed, (right, left), each (ext, stop, last):
        ext the symbols in the order they were appended, last a tuple of 8 -- the four onward supports of the evaluation
        that stopped the side, then the four return supports when the stop is WALK_JOIN (zeros otherwise; all zeros for
        LIMIT and INVALID); supports=True: (ext, stop, last, support).  unitig_sequence spells the sequence."""
        text, off = self._var_text(seeds)
        Q = len(seeds)
        ext = np.zeros((Q, 2, max_steps), np.uint8)
        steps, stop = np.zeros((Q, 2), np.uint32), np.zeros((Q, 2), np.uint8)
        sup = np.zeros((Q, 2, max_steps), np.uint32) if supports else None
        last = np.zeros((Q, 2, 8), np.uint64)
        check(lib().rsbwt_set_unitigs(self._s, _ptr(text), _ptr(off), Q, ctx, min_count, max_steps, _walk_flags(False, both_strands), _ptr(ext),
                                      _ptr(steps), _ptr(stop), _ptr(sup) if supports else None, _ptr(last)))
        out = []
        for q in range(Q):
            sides = []
            for d in range(2):
                n = int(steps[q, d])
                one = (ext[q, d, :n].tobytes().decode(), int(stop[q, d]), tuple(int(x) for x in last[q, d]))
                sides.append(one + (tuple(int(x) for x in sup[q, d, :n]),) if supports else one)
            out.append(tuple(sides))
        return out

    @staticmethod
    def unitigs_last_work():
        """{seeds, appended, searches, lf_steps, passes, table_starts, onward, back} of this thread's last unitigs call:
        onward and back count the onward and the return evaluations"""
        w = np.zeros(8, np.uint64)
        lib().rsbwt_set_unitig_last_work(w.ctypes.data_as(C.POINTER(C.c_uint64)))
        return dict(zip(("seeds", "appended", "searches", "lf_steps", "passes", "table_starts", "onward", "back"), (int(x) for x in w)))

    # -- paths (csrc/paths.hip): rsbwt_set_paths
    def paths(self, seeds, ctx, min_count=1, max_steps=256, max_paths=8, max_evals=None, left=False, both_strands=False, targets=None):
        """Every path from every seed through the reads' k-mer graph, depth first (rsbwt_set_paths): where a walk stops at
        a fork, the search takes A before C before G before T and comes back for the others.  A path ends where no symbol
        has a support of max(min_count, 1) (WALK_DEAD_END), after max_steps symbols (WALK_LIMIT), where its walking end
        spells the seed's target (WALK_TARGET; targets: one string of at most ctx symbols per seed, "" = none; not looked at
        before the first symbol) or when the seed has made max_evals evaluations (WALK_BUDGET; default 4 * max_steps).
        Returns, per seed, (state, [(ext, stop, min_support), ...]): state PATHS_COMPLETE (every path is there), PATHS_MORE
        (max_paths paths are out and forks are left), PATHS_BUDGET or PATHS_INVALID (no paths); ext the symbols in the order
        they were appended (left=True: the sequence is ext[::-1] + seed), min_support the least support of its symbols."""
        if max_evals is None:
            max_evals = 4 * max_steps
        text, off = self._var_text(seeds)
        Q = len(seeds)
        if targets is not None and len(targets) != Q:
            raise ValueError("one target per seed")
        ttext, toff = self._var_text(targets) if targets is not None else (None, None)
        ext = np.zeros((Q, max_paths, max_steps), np.uint8)
        steps, stop, sup = np.zeros((Q, max_paths), np.uint32), np.zeros((Q, max_paths), np.uint8), np.zeros((Q, max_paths), np.uint32)
        npaths, state = np.zeros(Q, np.uint32), np.zeros(Q, np.uint8)
        check(lib().rsbwt_set_paths(self._s, _ptr(text), _ptr(off), Q, _ptr(ttext) if targets is not None else None,
                                    _ptr(toff) if targets is not None else None, ctx, min_count, max_steps, max_paths, max_evals,
                                    _walk_flags(left, both_strands), _ptr(ext), _ptr(steps), _ptr(stop), _ptr(sup), _ptr(npaths), _ptr(state)))
        return [(int(state[q]), [(ext[q, j, :int(steps[q, j])].tobytes().decode(), int(stop[q, j]), int(sup[q, j])) for j in range(int(npaths[q]))])
                for q in range(Q)]

    @staticmethod
    def paths_last_work():
        """{seeds, appended, searches, lf_steps, passes, table_starts, evals, paths} of this thread's last paths call"""
        w = np.zeros(8, np.uint64)
        lib().rsbwt_set_paths_last_work(w.ctypes.data_as(C.POINTER(C.c_uint64)))
        return dict(zip(("seeds", "appended", "searches", "lf_steps", "passes", "table_starts", "evals", "paths"), (int(x) for x in w)))

    # -- the per-read sample table (csrc/read_meta.hip): rsbwt_set_meta_* / rsbwt_set_read_meta_var
    @staticmethod
    def _var_bytes(values):
        bs = [bytes(v) for v in values]
        off = np.zeros(len(bs) + 1, np.uint64)
        off[1:] = np.cumsum([len(b) for b in bs], dtype=np.uint64)
        return np.frombuffer(b"".join(bs) + b"\0", np.uint8).copy(), off

    def meta_build(self, reads, values):
        """Builds the set's sample table from (read, value bytes) pairs; a read given twice keeps the later value.
        Returns {matched, unmatched, ordinals, bytes} (rsbwt_set_meta_build).  Not beside a lookup on this set."""
        if len(reads) != len(values):
            raise ValueError("reads and values differ in length")
        text, off = self._var_text(reads)
        vals, voff = self._var_bytes(values)
        st = np.zeros(4, np.uint64)
        check(lib().rsbwt_set_meta_build(self._s, _ptr(text), _ptr(off), _ptr(vals), _ptr(voff), len(reads), _ptr(st)))
        return dict(zip(("matched", "unmatched", "ordinals", "bytes"), (int(x) for x in st)))

    def meta_load(self, path):
        """The same from the file load_data_into_rocksdb reads: a read line, a value line, repeated (rsbwt_set_meta_load)"""
        st = np.zeros(4, np.uint64)
        check(lib().rsbwt_set_meta_load(self._s, str(path).encode(), _ptr(st)))
        return dict(zip(("matched", "unmatched", "ordinals", "bytes"), (int(x) for x in st)))

    def meta_clear(self):
        check(lib().rsbwt_set_meta_clear(self._s))

    def meta_bytes(self):
        """bytes of the sample table in HBM over all shards (0: none)"""
        return int(lib().rsbwt_set_meta_bytes(self._s))

    def read_ordinals(self, queries):
        """(ordinal, copies) of shape (shards, Q): per shard the first ordinal of the reads equal to each query (0 where
        there is none) and how many there are (rsbwt_set_read_ordinals_var)"""
        text, off = self._var_text(queries)
        Q, S = len(queries), len(self.shards)
        od = np.zeros((S, Q), np.uint64)
        cp = np.zeros((S, Q), np.uint64)
        check(lib().rsbwt_set_read_ordinals_var(self._s, _ptr(text), _ptr(off), Q, _ptr(od), _ptr(cp)))
        return od, cp

    def meta_by_ordinal(self, shard_of, ordinal, raw=False):
        """the values of (shard, ordinal) items, in the order asked: a list of bytes; raw=True: (first, bytes array)
        (rsbwt_set_meta_by_ordinal)"""
        sh = np.ascontiguousarray(shard_of, dtype=np.uint32).ravel()
        od = np.ascontiguousarray(ordinal, dtype=np.uint64).ravel()
        if sh.size != od.size:
            raise ValueError("shard_of and ordinal differ in length")
        first = np.zeros(od.size + 1, np.uint64)
        n = C.c_size_t()
        rc = lib().rsbwt_set_meta_by_ordinal(self._s, _ptr(sh), _ptr(od), od.size, _ptr(first), None, 0, C.byref(n))
        if rc not in (0, -7):
            check(rc)
        out = np.zeros(max(n.value, 1), np.uint8)
        if n.value:
            check(lib().rsbwt_set_meta_by_ordinal(self._s, _ptr(sh), _ptr(od), od.size, _ptr(first), _ptr(out), n.value, C.byref(n)))
        if raw:
            return first, out[:n.value]
        return [out[int(first[i]):int(first[i + 1])].tobytes() for i in range(od.size)]

    def meta_by_ordinal_dev(self, d_shard, d_ordinal, n, d_first, d_bytes, cap, stream=None):
        """device pointers (ints) in, nothing synchronised (rsbwt_set_meta_by_ordinal_dev)"""
        check(lib().rsbwt_set_meta_by_ordinal_dev(self._s, d_shard, d_ordinal, n, d_first, d_bytes, cap, stream))

    def read_meta(self, queries, raw=False):
        """strings in, values out: ([query][shard] -> bytes, copies of shape (shards, Q)); raw=True: (first, bytes array,
        copies) with the value of query q in shard p at item q * S + p (rsbwt_set_read_meta_var)"""
        text, off = self._var_text(queries)
        Q, S = len(queries), len(self.shards)
        first = np.zeros(Q * S + 1, np.uint64)
        cp = np.zeros((S, max(Q, 1)), np.uint64)
        n = C.c_size_t()
        cap = 64 * Q * S + 256
        out = np.zeros(cap, np.uint8)
        rc = lib().rsbwt_set_read_meta_var(self._s, _ptr(text), _ptr(off), Q, _ptr(first), _ptr(out), cap, C.byref(n), _ptr(cp))
        if rc == -7:
            cap = n.value
            out = np.zeros(max(cap, 1), np.uint8)
            rc = lib().rsbwt_set_read_meta_var(self._s, _ptr(text), _ptr(off), Q, _ptr(first), _ptr(out), cap, C.byref(n), _ptr(cp))
        check(rc)
        cp = cp[:, :Q]
        if raw:
            return first, out[:n.value], cp
        return [[out[int(first[q * S + p]):int(first[q * S + p + 1])].tobytes() for p in range(S)] for q in range(Q)], cp

    @staticmethod
    def meta_last_work():
        """{items, valued, bytes, lf_steps} of this thread's last sample lookup (lf_steps: in counting mode only)"""
        w = np.zeros(4, np.uint64)
        lib().rsbwt_set_meta_last_work(w.ctypes.data_as(C.POINTER(C.c_uint64)))
        return dict(zip(("items", "valued", "bytes", "lf_steps"), (int(x) for x in w)))

    # -- sample counts (csrc/sample_counts.hip): rsbwt_set_sample_counts
    def meta_head_bytes(self):
        """bytes of the sample table's head bitmaps in HBM over all shards (0: no table); not part of meta_bytes()"""
        return int(lib().rsbwt_set_meta_head_bytes(self._s))

    def sample_counts(self, queries, codes, size_of_sample, has_other_meta_data=True, max_rows=0, max_steps=0):
        """In which samples each query occurs and how often (rsbwt_set_sample_counts).  codes: the sample dictionary, byte
        strings of size_of_sample bytes in any order.  Returns a dict of strings (Q, C + 1) uint32 -- the distinct reads
        holding the query that list the sample --, copies (Q, C + 1) int64 -- the sum of their c fields --, both with the
        columns in the caller's order and the records of unknown codes in the last column, matches (Q) -- the query's rows
        over the shards -- and carriers (Q) -- the distinct reads with a value entry that hold it."""
        cs = [bytes(c) for c in codes]
        if any(len(c) != size_of_sample for c in cs):
            raise ValueError("a code is not size_of_sample bytes long")
        order = sorted(range(len(cs)), key=lambda i: cs[i])
        flat = np.frombuffer(b"".join(cs[i] for i in order) + b"\0", np.uint8).copy()
        text, off = self._var_text(queries)
        Q, n = len(queries), len(cs)
        strings = np.zeros((max(Q, 1), n + 1), np.uint32)
        copies = np.zeros((max(Q, 1), n + 1), np.int64)
        matches, carriers = np.zeros(max(Q, 1), np.uint64), np.zeros(max(Q, 1), np.uint64)
        check(lib().rsbwt_set_sample_counts(self._s, _ptr(text), _ptr(off), Q, _ptr(flat), n, size_of_sample, 1 if has_other_meta_data else 0,
                                            max_rows, max_steps, _ptr(strings), _ptr(copies), _ptr(matches), _ptr(carriers)))
        back = np.empty(n + 1, np.int64)  # the caller's column -> the sorted column
        back[np.array(order, np.int64)] = np.arange(n)
        back[n] = n
        return dict(strings=strings[:Q][:, back], copies=copies[:Q][:, back], matches=matches[:Q].copy(), carriers=carriers[:Q].copy())

    @staticmethod
    def sample_last_work():
        """{rows, head_rows, carriers, records, unknown, lf_steps} of this thread's last sample_counts call (lf_steps: in
        counting mode only)"""
        w = np.zeros(6, np.uint64)
        lib().rsbwt_set_sample_last_work(w.ctypes.data_as(C.POINTER(C.c_uint64)))
        return dict(zip(("rows", "head_rows", "carriers", "records", "unknown", "lf_steps"), (int(x) for x in w)))

    # -- sample walks (csrc/sample_walk.hip): rsbwt_set_extension_samples / rsbwt_set_walk_samples
    @staticmethod
    def _sample_mask(codes, size_of_sample, mask_codes):
        """the dictionary in ascending order and the mask over it: (flat codes, n, mask u8[n])"""
        cs = [bytes(c) for c in codes]
        if any(len(c) != size_of_sample for c in cs):
            raise ValueError("a code is not size_of_sample bytes long")
        wanted = {bytes(c) for c in mask_codes}
        if wanted - set(cs):
            raise ValueError("a mask code is not in the dictionary")
        order = sorted(range(len(cs)), key=lambda i: cs[i])
        flat = np.frombuffer(b"".join(cs[i] for i in order) + b"\0", np.uint8).copy()
        mask = np.array([1 if cs[i] in wanted else 0 for i in order] + [0], np.uint8)
        return flat, len(cs), mask

    def extension_samples(self, queries, ctx, codes, size_of_sample, mask_codes=(), has_other_meta_data=True, max_rows=4096, max_locate_steps=0,
                          left=False, both_strands=False, copies=False):
        """One evaluation of a sample walk (rsbwt_set_extension_samples).  codes: the sample dictionary in any order, as
        sample_counts takes it; mask_codes: the codes of it whose reads count.  Returns a dict of msup (Q, 4) uint64 -- per
        symbol, the distinct reads holding the query's context + symbol that list a masked sample (copies=True: the sum of
        their c fields, at least 0), the reverse complement's added with both_strands --, wide (Q) uint8 -- 1 where a
        candidate has more than max_rows rows: its supports are 0 -- and matches (Q, 4) uint64, the candidates' rows."""
        flat, n, mask = self._sample_mask(codes, size_of_sample, mask_codes)
        text, off = self._var_text(queries)
        Q = len(queries)
        msup, matches = np.zeros((max(Q, 1), 4), np.uint64), np.zeros((max(Q, 1), 4), np.uint64)
        wide = np.zeros(max(Q, 1), np.uint8)
        check(lib().rsbwt_set_extension_samples(self._s, _ptr(text), _ptr(off), Q, ctx, _walk_flags(left, both_strands) | (4 if copies else 0),
                                                _ptr(flat), n, size_of_sample, 1 if has_other_meta_data else 0, _ptr(mask), max_rows,
                                                max_locate_steps, _ptr(msup), _ptr(wide), _ptr(matches)))
        return dict(msup=msup[:Q], wide=wide[:Q], matches=matches[:Q])

    def walk_samples(self, seeds, ctx, codes, size_of_sample, mask_codes=(), has_other_meta_data=True, min_count=1, max_steps=256, max_rows=4096,
                     max_locate_steps=0, left=False, both_strands=False, copies=False, supports=False):
        """Walks every seed through the reads of the samples mask_codes names (rsbwt_set_walk_samples): walk() with the
        support of a symbol counted over the distinct reads that hold the candidate and list a masked sample (copies=True:
        the sum of their c fields).  Returns what walk() returns; stop may also be WALK_WIDE: a candidate of the evaluation
        had more than max_rows rows (last is zeros then)."""
        flat, n, mask = self._sample_mask(codes, size_of_sample, mask_codes)
        text, off = self._var_text(seeds)
        Q = len(seeds)
        ext = np.zeros((max(Q, 1), max_steps), np.uint8)
        steps, stop = np.zeros(max(Q, 1), np.uint32), np.zeros(max(Q, 1), np.uint8)
        sup = np.zeros((max(Q, 1), max_steps), np.uint32) if supports else None
        last = np.zeros((max(Q, 1), 4), np.uint64)
        check(lib().rsbwt_set_walk_samples(self._s, _ptr(text), _ptr(off), Q, ctx, min_count, max_steps,
                                           _walk_flags(left, both_strands) | (4 if copies else 0), _ptr(flat), n, size_of_sample,
                                           1 if has_other_meta_data else 0, _ptr(mask), max_rows, max_locate_steps, _ptr(ext), _ptr(steps),
                                           _ptr(stop), _ptr(sup) if supports else None, _ptr(last)))
        out = []
        for q in range(Q):
            k = int(steps[q])
            one = (ext[q, :k].tobytes().decode(), int(stop[q]), tuple(int(x) for x in last[q]))
            out.append(one + (tuple(int(x) for x in sup[q, :k]),) if supports else one)
        return out

    @staticmethod
    def walk_samples_last_work():
        """{seeds, appended, searches, search_steps, rows, head_rows, carriers, records, lf_steps, wide} of this thread's last
        walk_samples or extension_samples call"""
        w = np.zeros(10, np.uint64)
        lib().rsbwt_set_walk_samples_last_work(w.ctypes.data_as(C.POINTER(C.c_uint64)))
        return dict(zip(("seeds", "appended", "searches", "search_steps", "rows", "head_rows", "carriers", "records", "lf_steps", "wide"),
                        (int(x) for x in w)))

    @staticmethod
    def walk_samples_last_times():
        """{init, search, plan, rows, locate, tally, decide}: the device time in ms of this thread's last walk_samples call on a
        one-device set by kind of launch, measured only while the environment holds RSBWT_SAMPLE_WALK_TIMES=1 (zeros otherwise)"""
        t = (C.c_double * 7)()
        lib().rsbwt_set_walk_samples_last_times(t)
        return dict(zip(("init", "search", "plan", "rows", "locate", "tally", "decide"), (float(x) for x in t)))

    # -- site sample counts (csrc/site_counts.hip): rsbwt_set_site_sample_counts
    def site_sample_counts(self, queries, pos, alt, isalt, k, skip=0, max_interval_size=0, *, codes, size_of_sample, has_other_meta_data=True):
        """Which samples have reads supporting each site request, and how many (rsbwt_set_site_sample_counts).  Requests as
        gt_aligned_reads takes them, the dictionary as sample_counts takes it.  Returns a dict of strings (Q, C + 1) uint32 and
        copies (Q, C + 1) int64 with the columns in the caller's order and the records of unknown codes in the last column,
        aligned (Q) -- the candidate reads with a value entry -- and carriers (Q) -- those align_gt_read keeps."""
        cs = [bytes(c) for c in codes]
        if any(len(c) != size_of_sample for c in cs):
            raise ValueError("a code is not size_of_sample bytes long")
        order = sorted(range(len(cs)), key=lambda i: cs[i])
        flat = np.frombuffer(b"".join(cs[i] for i in order) + b"\0", np.uint8).copy()
        text, off = self._var_text(queries)
        Q, n = len(queries), len(cs)
        p, a, ia = self._gt_requests(queries, pos, alt, isalt)
        strings = np.zeros((max(Q, 1), n + 1), np.uint32)
        copies = np.zeros((max(Q, 1), n + 1), np.int64)
        aligned, carriers = np.zeros(max(Q, 1), np.uint64), np.zeros(max(Q, 1), np.uint64)
        check(lib().rsbwt_set_site_sample_counts(self._s, _ptr(text), _ptr(off), Q, _ptr(p), _ptr(a), _ptr(ia), k, skip, max_interval_size, _ptr(flat), n,
                                                 size_of_sample, 1 if has_other_meta_data else 0, _ptr(strings), _ptr(copies), _ptr(aligned),
                                                 _ptr(carriers)))
        back = np.empty(n + 1, np.int64)  # the caller's column -> the sorted column
        back[np.array(order, np.int64)] = np.arange(n)
        back[n] = n
        return dict(strings=strings[:Q][:, back], copies=copies[:Q][:, back], aligned=aligned[:Q].copy(), carriers=carriers[:Q].copy())

    @staticmethod
    def site_last_work():
        """{legs, narrow_steps, candidates, kept, head_rows, extracted, aligned, carriers, records, unknown} of this thread's
        last site_sample_counts call"""
        w = np.zeros(10, np.uint64)
        lib().rsbwt_set_site_last_work(w.ctypes.data_as(C.POINTER(C.c_uint64)))
        return dict(zip(("legs", "narrow_steps", "candidates", "kept", "head_rows", "extracted", "aligned", "carriers", "records", "unknown"),
                        (int(x) for x in w)))

    @staticmethod
    def site_last_times():
        """{filter, set, reads, items, align, tally} in ms of this thread's last site_sample_counts call, from events; zeros
        unless RSBWT_SITE_TIMES=1 (rsbwt_set_site_last_times)"""
        t = np.zeros(6, np.float64)
        lib().rsbwt_set_site_last_times(t.ctypes.data_as(C.POINTER(C.c_double)))
        return dict(zip(("filter", "set", "reads", "items", "align", "tally"), (float(x) for x in t)))

    # -- site reads (csrc/site_reads.hip): gt_aligned_reads / gt_aligned_count with the batch kept on the device
    def site_reads(self, queries, pos, alt, isalt, k, skip=0, max_interval_size=0, read_stride=256, with_rows=False):
        """What gt_aligned_reads returns, from the device-resident call (rsbwt_set_site_reads): [query][shard] -> reads,
        ascending read_row, a string once"""
        text, off = self._var_text(queries)
        Q, S = len(queries), len(self.shards)
        p, a, ia = self._gt_requests(queries, pos, alt, isalt)
        first = np.zeros(Q * S + 1, np.uint64)
        n = C.c_size_t()
        rc = lib().rsbwt_set_site_reads(self._s, _ptr(text), _ptr(off), Q, _ptr(p), _ptr(a), _ptr(ia), k, skip, max_interval_size, _ptr(first), None,
                                        read_stride, None, None, 0, C.byref(n))
        if rc not in (0, -7):
            check(rc)
        total = n.value
        reads = np.zeros((max(total, 1), read_stride), np.uint8)
        ln = np.zeros(max(total, 1), np.uint32)
        rr = np.zeros(max(total, 1), np.uint64)
        if total:
            check(lib().rsbwt_set_site_reads(self._s, _ptr(text), _ptr(off), Q, _ptr(p), _ptr(a), _ptr(ia), k, skip, max_interval_size, _ptr(first),
                                             _ptr(reads), read_stride, _ptr(ln), _ptr(rr), total, C.byref(n)))
            if (ln[:total] == 0xFFFFFFFF).any():
                raise RsbwtError(-1, "a read does not fit read_stride")

        def one(r):
            t = reads[r, :ln[r]].tobytes().decode()
            return (int(rr[r]), t) if with_rows else t
        return [[[one(r) for r in range(int(first[q * S + s]), int(first[q * S + s + 1]))] for s in range(S)] for q in range(Q)]

    def site_read_counts(self, queries, pos, alt, isalt, k, skip=0, max_interval_size=0):
        """[query][shard] -> the number of those reads (rsbwt_set_site_read_counts)"""
        text, off = self._var_text(queries)
        Q, S = len(queries), len(self.shards)
        p, a, ia = self._gt_requests(queries, pos, alt, isalt)
        out = np.zeros(Q * S, np.uint64)
        check(lib().rsbwt_set_site_read_counts(self._s, _ptr(text), _ptr(off), Q, _ptr(p), _ptr(a), _ptr(ia), k, skip, max_interval_size, _ptr(out)))
        return out.reshape(Q, S)

    @staticmethod
    def site_reads_last_work():
        """{legs, narrow_steps, candidates, kept, extracted, classes, aligned, items_kept, reported} of this thread's last
        site_reads / site_read_counts call"""
        w = np.zeros(9, np.uint64)
        lib().rsbwt_set_site_reads_last_work(w.ctypes.data_as(C.POINTER(C.c_uint64)))
        return dict(zip(("legs", "narrow_steps", "candidates", "kept", "extracted", "classes", "aligned", "items_kept", "reported"), (int(x) for x in w)))

    # -- BASELINE configs[3] / configs[4] over the set: per-shard results side by side, the way the front-end
    # concatenates its partitions' replies (src/service/server.cpp:199-261)
    def hits_1mm(self, kmers):
        """Every shard's 1-mismatch hit list: (HIT_1MM array, first) with shard i's hits at first[i]:first[i+1]."""
        a, k = _kmer_matrix(kmers)
        Q, S = a.shape[0], len(self.shards)
        cap = max(1024, 4 * Q * S)
        first = np.zeros(S + 1, np.uint64)
        while True:
            out = np.zeros(cap, HIT_1MM)
            n = C.c_size_t()
            rc = lib().rsbwt_set_hits_1mm(self._s, _ptr(a), Q, k, max(k, 1), _ptr(out), cap, _ptr(first), C.byref(n))
            if rc == -7 and n.value > cap:
                cap = n.value
                continue
            check(rc)
            return out[:n.value], first

    def extract(self, shard_of, rows, stride=512):
        """Reads at (shard, row) pairs: (list of strings, prefix lengths)."""
        sh = np.ascontiguousarray(shard_of, dtype=np.uint32)
        r = np.ascontiguousarray(rows, dtype=np.uint64)
        out = np.zeros((r.size, stride), np.uint8)
        ln, pl = np.empty(r.size, np.uint32), np.empty(r.size, np.uint32)
        check(lib().rsbwt_set_extract(self._s, _ptr(sh), _ptr(r), r.size, _ptr(out), stride, _ptr(ln), _ptr(pl)))
        if (ln == 0xFFFFFFFF).any():
            raise RsbwtError(-1, "a read does not fit the stride / a row is out of range")
        return [out[i, :ln[i]].tobytes().decode() for i in range(r.size)], pl

    def locate(self, shard_of, rows, max_steps=0):
        """(read_row, ordinal, offset) of (shard, row) pairs (rsbwt_set_locate; GpuBWT.locate's answers per shard)"""
        sh = np.ascontiguousarray(shard_of, dtype=np.uint32).ravel()
        r = np.ascontiguousarray(rows, dtype=np.uint64).ravel()
        if sh.size != r.size:
            raise ValueError("shard_of and rows differ in length")
        rr, od, of = np.empty(r.size, np.uint64), np.empty(r.size, np.uint64), np.empty(r.size, np.uint32)
        check(lib().rsbwt_set_locate(self._s, _ptr(sh), _ptr(r), r.size, max_steps, _ptr(rr), _ptr(od), _ptr(of)))
        return rr, od, of

    def locate_queries(self, queries, max_rows=0, max_steps=0):
        """The matches of every query as positions (rsbwt_set_locate_var_capped): a dict of first (Q + 1), matches (Q),
        and per match shard, row, read_row, ordinal, offset -- query q's matches at first[q]:first[q+1], shard ascending,
        SA row ascending; none for a query whose rows over all shards exceed max_rows (0 = no limit)."""
        text, off = self._var_text(queries)
        Q = len(queries)
        first = np.zeros(Q + 1, np.uint64)
        matches = np.zeros(max(Q, 1), np.uint64)
        n = C.c_size_t()
        rc = lib().rsbwt_set_locate_var_capped(self._s, _ptr(text), _ptr(off), Q, max_rows, max_steps, _ptr(first), None, None, None, None,
                                               None, 0, C.byref(n), _ptr(matches))
        if rc not in (0, -7):
            check(rc)
        total = n.value
        m = max(total, 1)
        sh, of = np.zeros(m, np.uint32), np.zeros(m, np.uint32)
        rows, rr, od = np.zeros(m, np.uint64), np.zeros(m, np.uint64), np.zeros(m, np.uint64)
        if total:
            check(lib().rsbwt_set_locate_var_capped(self._s, _ptr(text), _ptr(off), Q, max_rows, max_steps, _ptr(first), _ptr(sh), _ptr(rows),
                                                    _ptr(rr), _ptr(od), _ptr(of), total, C.byref(n), _ptr(matches)))
        return dict(first=first, matches=matches[:Q].copy(), shard=sh[:total], row=rows[:total], read_row=rr[:total], ordinal=od[:total],
                    offset=of[:total])

    @staticmethod
    def locate_last_work():
        """{located, lf_steps} of this thread's last locate call: rows that ended on '$', LF steps of all walks"""
        w = np.zeros(2, np.uint64)
        lib().rsbwt_locate_last_work(w.ctypes.data_as(C.POINTER(C.c_uint64)))
        return dict(located=int(w[0]), lf_steps=int(w[1]))

    def query(self, kmers, read_stride=256):
        """query() in every shard (query.cpp:87-100): per k-mer a list of (shard, read), shard 0's reads first."""
        a, k = _kmer_matrix(kmers)
        Q = a.shape[0]
        first = np.zeros(Q + 1, np.uint64)
        n = C.c_size_t()
        rc = lib().rsbwt_set_query(self._s, _ptr(a), Q, k, max(k, 1), _ptr(first), None, None, read_stride, None, 0, C.byref(n))
        if rc not in (0, -7):
            check(rc)
        total = n.value
        reads = np.zeros((max(total, 1), read_stride), np.uint8)
        ln = np.zeros(max(total, 1), np.uint32)
        sh = np.zeros(max(total, 1), np.uint32)
        if total:
            check(lib().rsbwt_set_query(self._s, _ptr(a), Q, k, max(k, 1), _ptr(first), _ptr(sh), _ptr(reads), read_stride,
                                        _ptr(ln), total, C.byref(n)))
            if (ln[:total] == 0xFFFFFFFF).any():
                raise RsbwtError(-1, "a read does not fit read_stride")
        return [[(int(sh[r]), reads[r, :ln[r]].tobytes().decode()) for r in range(int(first[q]), int(first[q + 1]))]
                for q in range(Q)]


def encode_all_reply(request_type, return_type, q, revcomp, reads, values, hash_text=b"", size_of_sample=2, has_other_meta_data=True):
    """Reply{rt, t = return type, q, a = ReplyAll{ResultAll{r, s*}*}} as the reference's QueryTask / KmerTask send it for All
    and Samples: reads (str / bytes) with their sample-table values (bytes); hash_text = the hash file's text
    (rsbwt_proto_encode_all_reply)"""
    rs = [r if isinstance(r, (bytes, bytearray)) else str(r).encode() for r in reads]
    vs = [bytes(v) for v in values]
    if len(rs) != len(vs):
        raise ValueError("reads and values differ in length")
    qb = q if isinstance(q, (bytes, bytearray)) else str(q).encode()
    hb = hash_text if isinstance(hash_text, (bytes, bytearray)) else str(hash_text).encode()
    n = len(rs)
    rp = (C.c_char_p * max(n, 1))(*rs)
    rl = (C.c_size_t * max(n, 1))(*[len(r) for r in rs])
    keep = [C.create_string_buffer(v, max(len(v), 1)) for v in vs]
    vp = (C.c_void_p * max(n, 1))(*[C.addressof(b) for b in keep])
    vl = (C.c_size_t * max(n, 1))(*[len(v) for v in vs])
    args = (request_type, return_type, qb, len(qb), 1 if revcomp else 0, rp, rl, vp, vl, n, hb, len(hb), size_of_sample,
            1 if has_other_meta_data else 0)
    need = lib().rsbwt_proto_encode_all_reply(None, 0, *args)
    if need == 0:
        raise RsbwtError(-1, "bad arguments to rsbwt_proto_encode_all_reply")
    out = np.zeros(need, np.uint8)
    lib().rsbwt_proto_encode_all_reply(_ptr(out), need, *args)
    return out.tobytes()


def parse_meta_file(path):
    """(reads, values): the pairs rsbwt_set_meta_load builds from a file, as lists of bytes (host only: rsbwt_meta_parse_file)"""
    sz = (C.c_size_t * 3)()
    rc = lib().rsbwt_meta_parse_file(str(path).encode(), None, 0, None, None, 0, None, 0, sz)
    if rc not in (0, -7):
        check(rc)
    n, tb, vb = sz[0], sz[1], sz[2]
    text, vals = np.zeros(max(tb, 1), np.uint8), np.zeros(max(vb, 1), np.uint8)
    off, voff = np.zeros(n + 1, np.uint64), np.zeros(n + 1, np.uint64)
    check(lib().rsbwt_meta_parse_file(str(path).encode(), _ptr(text), tb, _ptr(off), _ptr(vals), vb, _ptr(voff), n, sz))
    return ([text[int(off[i]):int(off[i + 1])].tobytes() for i in range(n)],
            [vals[int(voff[i]):int(voff[i + 1])].tobytes() for i in range(n)])


def write_bpi2(bwt_path, bpi2_path=None):
    """src/util/index_rlebwt.cpp:19-22: writes the reference's FM-index file for a .bwt (default
    "<bwt>.bpi2"), byte-identical to RLEBWT::serialiseFMIndex.  Host only."""
    out = str(bpi2_path) if bpi2_path else str(bwt_path) + ".bpi2"
    check(lib().rsbwt_bpi2_write(str(bwt_path).encode(), out.encode()))
    return out


def check_bpi2(pBWT, bpi2_path, max_samples=1 << 20):
    """Validates a prebuilt .bpi2 against the resident index on the GPU: (buckets checked,
    mismatches, first difference or '')."""
    n, bad = C.c_uint64(), C.c_uint64()
    check(lib().rsbwt_bpi2_check(pBWT.handle, str(bpi2_path).encode(), max_samples, C.byref(n), C.byref(bad)))
    return n.value, bad.value, (lib().rsbwt_last_error().decode() if bad.value else "")


def synth_popbwt(bwt_path, reads_path=None, *, seed, genome_len, haplotypes, snp_rate, read_len,
                 coverage, shard=-1, num_shards=1):
    """Deterministic synthetic population BWT written as an SGA .bwt (host only; csrc/synth.cpp)."""
    check(lib().rsbwt_synth_popbwt(str(bwt_path).encode(),
                                   str(reads_path).encode() if reads_path else None,
                                   seed, genome_len, haplotypes, snp_rate, read_len, coverage,
                                   shard, num_shards))
