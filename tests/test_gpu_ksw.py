"""ksw_align on the GPU (-m gpu): rsbwt_ksw_align / rsbwt_ksw_align_dev (csrc/ksw_align.hip) held field by field to the
outputs recorded from the reference's own ksw.c (tests/golden/ksw_v1.npz) and, where no record exists (the lengths each
side of every length class and of the LDS / HBM column switch, the 4,096-symbol pairs), to tests/ksw_reference.py, which
tests/test_ksw_reference.py holds to the same records on the CPU."""
import ctypes as C
import threading

import numpy as np
import pytest

import ksw_reference as kr

pytestmark = pytest.mark.gpu

SWITCHES = (32, 33, 64, 65, 104, 105, 160, 161, 224, 225)  # the last row of every length class and the first of the next


@pytest.fixture(scope="module")
def golden(golden_dir):
    return kr.load_golden(golden_dir)


def _want(pairs, params):
    return np.array([kr.ksw_align(kr.code(q), kr.code(t), params) for q, t in pairs], np.int32)


@pytest.fixture(scope="module")
def switch_pairs():
    """reads of every length beside a class boundary against targets cut around them, with an indel and substitutions;
    and the restatement's answers for both parameter sets, computed once"""
    rng = np.random.default_rng(225)
    rnd = lambda n: "".join("ACGT"[c] for c in rng.integers(0, 4, n))  # noqa: E731
    pairs = []
    for n in SWITCHES:
        for _ in range(3):
            core = rnd(n)
            q = list(core)
            for p in rng.integers(0, n, 3):
                q[p] = "ACGTN"[int(rng.integers(5))]
            a = int(rng.integers(8, n - 8))
            t = rnd(int(rng.integers(0, 9))) + core[:a] + rnd(int(rng.integers(0, 3))) + core[a + int(rng.integers(0, 3)):] + rnd(int(rng.integers(0, 9)))
            pairs.append(("".join(q).encode(), t[:int(rng.integers(40, 90))].encode() if n > 160 else t.encode()))
    return pairs, {p: _want(pairs, p) for p in (kr.SERVICE, kr.OTHER)}


def test_every_golden_record_through_the_host_call(rsb, golden):
    pairs, sets, _, _ = golden
    for params, res in sets:
        got = rsb.ksw_align(pairs, params)
        bad = np.flatnonzero((got != res).any(axis=1))
        assert len(bad) == 0, (params, len(bad), int(bad[0]), got[bad[0]], res[bad[0]])
    assert (rsb.ksw_align(pairs) == sets[0][1]).all()  # params = NULL is the service's


def test_every_golden_record_through_the_device_call(rsb, golden):
    """every array in HBM, the items in the caller's order, the output inside guard bytes, every byte of it written"""
    import torch
    L = rsb.lib()
    pairs, sets, _, _ = golden
    n, PAD = len(pairs), 256
    qtext, qoff = rsb.bwt._texts([q for q, _ in pairs])
    ttext, toff = rsb.bwt._texts([t for _, t in pairs])
    d = [torch.from_numpy(a.view(np.uint8)).cuda() for a in (qtext, qoff, ttext, toff)]
    p = lambda t, byte=0: C.c_void_p(t.data_ptr() + byte)  # noqa: E731
    for params, res in sets:
        prm = np.array(params, np.int32)
        out = torch.full((PAD + n * 24 + PAD,), 0xAB, dtype=torch.uint8, device="cuda")
        assert L.rsbwt_ksw_align_dev(prm.ctypes.data_as(C.c_void_p), p(d[0]), p(d[1]), p(d[2]), p(d[3]), n, p(out, PAD), 0, None) == 0, L.rsbwt_last_error()
        torch.cuda.synchronize()
        hb = out.cpu().numpy()
        assert (hb[:PAD] == 0xAB).all() and (hb[PAD + n * 24:] == 0xAB).all()
        got = hb[PAD:PAD + n * 24].view(np.int32).reshape(n, 6)
        assert (got[:, 5] == 0).all() and (got[:, :5] == res).all(), params


def test_device_call_marks_pairs_it_cannot_refuse(rsb):
    """a zero-length query, a target over 4,096 symbols and a pair whose scores would pass 2^15 get all five fields -1; their
    neighbours their answers"""
    import torch
    L = rsb.lib()
    qs = [b"ACGTACGTAC", b"", b"ACGT", b"A" * 300, b"TTGACCA"]
    ts = [b"TTACGTACGTACTT", b"ACGT", b"C" * 4097, b"A" * 300, b"GGTTGACCAGG"]
    qtext, qoff = rsb.bwt._texts(qs)
    ttext, toff = rsb.bwt._texts(ts)
    d = [torch.from_numpy(a.view(np.uint8)).cuda() for a in (qtext, qoff, ttext, toff)]
    out = torch.full((5 * 24,), 0xAB, dtype=torch.uint8, device="cuda")
    prm = np.array((120, 4, 1, 6, 1), np.int32)  # 120 x 300 >= 2^15
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    assert L.rsbwt_ksw_align_dev(prm.ctypes.data_as(C.c_void_p), p(d[0]), p(d[1]), p(d[2]), p(d[3]), 5, p(out), 0, None) == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.int32).reshape(5, 6)
    assert (got[[1, 2, 3], :5] == -1).all() and (got[:, 5] == 0).all()
    for i in (0, 4):
        assert tuple(got[i, :5]) == kr.ksw_align(kr.code(qs[i]), kr.code(ts[i]), tuple(prm))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_batches_in_given_and_shuffled_order(rsb, golden, n):
    """mixed lengths, so the host's ordering by length is a real permutation; the answers come back in the caller's order"""
    pairs, sets, _, _ = golden
    rng = np.random.default_rng(n)
    pick = rng.choice(len(pairs), n, replace=False)
    assert n == 1 or len({len(pairs[i][0]) for i in pick}) > 1
    for order in (np.sort(pick), pick):
        for params, res in sets:
            assert (rsb.ksw_align([pairs[i] for i in order], params) == res[order]).all(), (n, params)


def test_lengths_each_side_of_every_column_switch(rsb, switch_pairs):
    """rows 224 and 225 are the last in LDS and the first in the HBM scratch column; the others end a length class.  Alone
    (one pair, one block, its own class) and all in one batch (blocks of several classes, partly filled)"""
    pairs, want = switch_pairs
    assert {len(q) for q, _ in pairs} == set(SWITCHES) and rsb.bwt.KSW_LDS_ROWS == 224
    for params in (kr.SERVICE, kr.OTHER):
        assert (rsb.ksw_align(pairs, params) == want[params]).all(), params
        for i in range(0, len(pairs), 3):
            assert (rsb.ksw_align(pairs[i:i + 1], params) == want[params][i:i + 1]).all(), (params, len(pairs[i][0]))


def test_the_longest_pairs(rsb):
    """4,096 x 64 (the column in HBM) and 64 x 4,096, beside a short pair that shares their batch"""
    rng = np.random.default_rng(4096)
    rnd = lambda n: "".join("ACGT"[c] for c in rng.integers(0, 4, n))  # noqa: E731
    long_ = rnd(4096)
    piece = long_[2000:2030] + "G" + long_[2030:2063]
    pairs = [(long_, piece), (piece, long_), ("ACGTTGCA", "TTACGTTGCATT")]
    for params in (kr.SERVICE, kr.OTHER):
        want = _want([(q.encode(), t.encode()) for q, t in pairs], params)
        assert want[0][0] > 40 and want[1][0] > 40
        assert (rsb.ksw_align(pairs, params) == want).all(), params


def test_two_concurrent_host_threads(rsb, golden):
    pairs, sets, _, _ = golden
    got, errs = {}, []

    def run(which):
        try:
            params, _ = sets[which]
            for rep in range(3):
                got[(which, rep)] = rsb.ksw_align(pairs[which::2], params)
        except Exception as e:  # noqa: BLE001
            errs.append(e)
    th = [threading.Thread(target=run, args=(w,)) for w in (0, 1)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs
    for (which, rep), g in got.items():
        assert (g == sets[which][1][which::2]).all(), (which, rep)
