"""Plain numpy references of the rank primitives (readserver_amd/csrc/rank_device.h), restated from the contracts in their
header comments and nothing else: the 24 pieces of a quarter are walked one by one in uint64 arithmetic -- no tables, no
prefix sums by multiplication, no dword totals.

A piece byte is `sym << 5 | len`.  A piece of length 0 counts for nothing, whatever its symbol.  A symbol code 5..7 is a
symbol like any other here: it is no b of 0..4, so it matches none.  `rem = 0` gives 0; `rem` beyond what the pieces hold
gives all they hold.

Shapes: `pieces` (N, P) uint8 with P = 4, 8 or 24; `b` (N,); the arguments `rem` / `t` (N, K): every quarter is asked K
questions at once.  Results are (N, K) uint64.

tests/test_rank_reference.py holds these functions to the naive definition (the pieces expanded to a symbol array, counted
with == and cumsum); tests/test_gpu_rank_primitives.py holds the kernels' primitives to them.  The case classes both
modules use are built here too."""
import numpy as np

U64 = np.uint64


def pieces_of(dwords):
    """(N, D) uint32 dwords -> (N, 4 D) piece bytes, little endian: piece 0 is the low byte of dword 0"""
    return np.ascontiguousarray(dwords, dtype="<u4").view(np.uint8).reshape(len(dwords), -1)


def dwords_of(pieces):
    return np.ascontiguousarray(pieces, dtype=np.uint8).view("<u4").reshape(len(pieces), -1)


def _split(pieces):
    p = np.asarray(pieces, dtype=np.uint8)
    return (p >> 5).astype(U64), (p & 31).astype(U64)


def rank_ref(pieces, b, rem):
    """how many of the first `rem` symbols of the pieces are b (rank24, rank24_dollar, runs_scan<P / 4>)"""
    sym, ln = _split(pieces)
    b = np.asarray(b, dtype=U64)
    left = np.array(rem, dtype=U64, copy=True)
    acc = np.zeros(left.shape, U64)
    take = np.empty(left.shape, U64)
    for i in range(sym.shape[1]):
        np.minimum(left, ln[:, i, None], out=take)
        left -= take
        take *= (sym[:, i] == b).astype(U64)[:, None]
        acc += take
    return acc


def held_ref(pieces, b):
    """what the pieces hold of b (matched24_tab); (N,)"""
    sym, ln = _split(pieces)
    b = np.asarray(b, dtype=U64)
    acc = np.zeros(len(sym), U64)
    for i in range(sym.shape[1]):
        acc += np.where(sym[:, i] == b, ln[:, i], U64(0))
    return acc


def dword_matched_ref(pieces, b, acc):
    """(N, 6): acc + what each dword's four pieces hold of b, as the 32-bit sum it is"""
    out = np.empty((len(pieces), pieces.shape[1] // 4), U64)
    for d in range(out.shape[1]):
        out[:, d] = (held_ref(pieces[:, 4 * d:4 * d + 4], b) + np.asarray(acc, dtype=U64)) & U64(0xFFFFFFFF)
    return out


def char_rank_ref(pieces, rem, want=None):
    """char_rank24: c = symbol of the piece holding the rem-th symbol (rem >= 1; 0 when the pieces hold fewer or rem == 0),
    occ = how many of the first rem symbols are c.  want (N,) non-zero: c = want whatever the piece says."""
    sym, ln = _split(pieces)
    rem = np.asarray(rem, dtype=U64)
    c = np.zeros(rem.shape, U64)
    lo = np.zeros(len(sym), U64)
    for i in range(sym.shape[1]):
        hi = lo + ln[:, i]
        hit = (rem > lo[:, None]) & (rem <= hi[:, None])  # (a piece of no length holds no position)
        c = np.where(hit, sym[:, i, None], c)
        lo = hi
    if want is not None:
        w = np.asarray(want, dtype=U64)[:, None]
        c = np.where(w != 0, w, c)
    left = rem.copy()
    occ = np.zeros(rem.shape, U64)
    for i in range(sym.shape[1]):
        take = np.minimum(left, ln[:, i, None])
        left -= take
        occ += np.where(sym[:, i, None] == c, take, U64(0))
    return c, occ


def select_ref(pieces, b, t):
    """select_in24: (position, left).  position = symbols before the t-th b, counted from the first piece (t >= 1);
    left = t - held when the pieces hold fewer than t of b, else 0.  t = 0 gives (0, 0).  Where left != 0 the position is
    UNSPECIFIED (the caller goes on in the next pieces): the value returned here, 0, must not be compared."""
    sym, ln = _split(pieces)
    b = np.asarray(b, dtype=U64)
    t = np.asarray(t, dtype=U64)
    pos = np.zeros(t.shape, U64)
    seen = np.zeros(len(sym), U64)   # b's in the pieces walked so far
    before = np.zeros(len(sym), U64)  # symbols in them
    for i in range(sym.shape[1]):
        nb = np.where(sym[:, i] == b, ln[:, i], U64(0))
        hit = (t > seen[:, None]) & (t <= (seen + nb)[:, None])
        pos = np.where(hit, before[:, None] + (t - seen[:, None]) - U64(1), pos)
        seen = seen + nb
        before = before + ln[:, i]
    left = np.where(t > seen[:, None], t - seen[:, None], U64(0))
    return pos, left


def symbol_at_ref(pieces, pos):
    """symbol of the piece holding 0-based position pos (N, K); 255 past the pieces"""
    sym, ln = _split(pieces)
    pos = np.asarray(pos, dtype=U64)
    out = np.full(pos.shape, 255, U64)
    lo = np.zeros(len(sym), U64)
    for i in range(sym.shape[1]):
        hi = lo + ln[:, i]
        out = np.where((pos >= lo[:, None]) & (pos < hi[:, None]), sym[:, i, None], out)
        lo = hi
    return out


# ---- the arguments every quarter is asked about -----------------------------------------------------------------------

def rem_values(pieces):
    """(N, 78): 0, 1, each of the 24 cumulative piece boundaries - 1 / + 0 / + 1, the total, the total + 1, 4095, 65535"""
    ln = (np.asarray(pieces, np.uint8) & 31).astype(np.int64)
    cum = np.cumsum(ln, axis=1)
    tot = cum[:, -1:]
    n = len(ln)
    cols = [np.zeros((n, 1), np.int64), np.ones((n, 1), np.int64), np.maximum(cum - 1, 0), cum, cum + 1, tot, tot + 1,
            np.full((n, 1), 4095, np.int64), np.full((n, 1), 65535, np.int64)]
    return np.concatenate(cols, axis=1).astype(U64)


def select_values(pieces, b):
    """(N, 77): 0, 1, every cumulative count of b - 1 / + 0 / + 1, the total, the total + 1, 4095"""
    p = np.asarray(pieces, np.uint8)
    nb = np.where((p >> 5) == np.asarray(b)[:, None], p & 31, 0).astype(np.int64)
    cum = np.cumsum(nb, axis=1)
    tot = cum[:, -1:]
    n = len(p)
    cols = [np.zeros((n, 1), np.int64), np.ones((n, 1), np.int64), np.maximum(cum - 1, 0), cum, cum + 1, tot, tot + 1,
            np.full((n, 1), 4095, np.int64)]
    return np.concatenate(cols, axis=1).astype(U64)


# ---- case classes -----------------------------------------------------------------------------------------------------

def _realistic(rng, n):
    """symbols mostly 1..4, 1 % '$', lengths skewed short (geometric, capped at 31)"""
    sym = np.where(rng.random((n, 24)) < 0.01, 0, rng.integers(1, 5, (n, 24)))
    ln = np.minimum(rng.geometric(0.25, (n, 24)), 31)
    return ((sym << 5) | ln).astype(np.uint8)


def random_classes(rng, n):
    """name -> (n, 24) piece bytes, n quarters of every class but the all-zero one (which is one quarter, a few times)"""
    out = {}
    out["uniform"] = rng.integers(0, 256, (n, 24)).astype(np.uint8)
    out["realistic"] = _realistic(rng, n)
    # every length 31: the pieces hold 744 symbols, every byte-multiply prefix sum (ps, qs) is at its maximum of 124
    out["all31"] = ((np.where(rng.random((n, 24)) < 0.1, 0, rng.integers(1, 5, (n, 24))) << 5) | 31).astype(np.uint8)
    out["zero"] = np.zeros((64, 24), np.uint8)
    p = _realistic(rng, n)  # k real pieces, then padding zeros, k = 0..24
    p[np.arange(24)[None, :] >= (np.arange(n) % 25)[:, None]] = 0
    out["padded"] = p
    p = _realistic(rng, n)  # pieces of no length that still name a symbol, between real ones
    p[rng.random((n, 24)) < 0.25] &= 0xE0
    out["zero_length"] = p
    p = _realistic(rng, n)  # one symbol over several pieces, across a dword border
    start = rng.integers(0, 20, n)
    span = rng.integers(5, 13, n)
    col = np.arange(24)[None, :]
    inside = (col >= start[:, None]) & (col < (start + span)[:, None])
    s = rng.integers(0, 5, n).astype(np.uint8)
    out["long_runs"] = np.where(inside, (s[:, None] << 5) | (p & 31), p).astype(np.uint8)
    p = _realistic(rng, n)  # symbol codes no BWT has
    bad = rng.random((n, 24)) < 0.1
    out["codes_5_7"] = np.where(bad, (rng.integers(5, 8, (n, 24)) << 5) | (p & 31), p).astype(np.uint8)
    return out


def exhaustive_pairs(rng, b, where):
    """(65536, 24): pieces `where`, `where` + 1 (0 or 2) of dword 0 take every pair of bytes, the rest is random; where = 2:
    pieces 0 and 1 are non-empty runs of b, so that a matching piece in byte 2 or 3 follows a non-zero sum"""
    p = rng.integers(0, 256, (65536, 24)).astype(np.uint8)
    v = np.arange(65536)
    p[:, where] = v & 0xFF
    p[:, where + 1] = v >> 8
    if where == 2:
        p[:, 0:2] = (b << 5) | rng.integers(1, 32, (65536, 2))
    return p
