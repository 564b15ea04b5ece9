#!/usr/bin/env python3
"""Generates tests/golden/service_kmer_v1.json: serialised KmerMatch `Request`s (return type Count or Reads) and, for
each, the bytes of the two `Reply` messages (forward strand, then reverse complement) a reference `service` process
holding the popbwt_v1 fixture as its one partition sends back: KmerTask::run (src/service/service.cpp:871-960) around
find_kmer_reads (:466-502), with min_read_length = 50 and max_read_length = 70 as service_reads_v1.json has them; and
the empty Replies of one Request of every (type, return type) pair this service does not serve (`unserved = "empty"`).

The BWT work is the REAL reference's (oracle/_ref/libref_bwt.so, through make_service_reads_golden.py's `Ref` and its
restatement of find_reads).  find_kmer_reads' control flow is restated below with the lines it follows.  The two orders
that come from std::unordered_set<std::string> -- get_tiles(w, k, skip)'s (:232-246: ref_tiles_order has no skip) and
that of the set the reads are folded into -- come from a small C++ helper of this generator's own, compiled into a
temporary directory with the C++ library the reference is built with.  The Reply bytes are the Python protobuf
runtime's on the re-typed schema (tests/proto_schema.py).  Only inputs and expected outputs are stored; replies longer
than 4 KB as their length and SHA-256.
"""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_service_reads_golden as msr  # noqa: E402  (Ref, find_reads with min / max 50 / 70, rc; ROOT on sys.path)
import proto_schema  # noqa: E402
import readserver_amd as rsb  # noqa: E402

HELPER = r'''
#include <string.h>
#include <string>
#include <unordered_set>
#include <vector>
extern "C" {
// get_tiles(w, kmer, skip) (service.cpp:232-246), its iteration order, '\n'-separated
size_t tiles(const char *w, size_t len, size_t kmer, size_t skip, char *out, size_t cap) {
    std::unordered_set<std::string> vs;
    const std::string s(w, len);
    if (len >= kmer)
        for (size_t i = 0; i <= len - kmer;) { vs.insert(s.substr(i, kmer)); i += skip + 1; }
    std::string o;
    for (const std::string &t : vs) { o += t; o += '\n'; }
    if (out && o.size() <= cap) memcpy(out, o.data(), o.size());
    return o.size();
}
void *set_new() { return new std::unordered_set<std::string>(); }
void set_free(void *h) { delete (std::unordered_set<std::string> *)h; }
// seqs.insert(v.begin(), v.end()) for v = the '\n'-separated strings (find_kmer_reads :491,497)
void set_insert(void *h, const char *joined, size_t len) {
    std::vector<std::string> v;
    size_t a = 0;
    for (size_t i = 0; i < len; ++i)
        if (joined[i] == '\n') { v.emplace_back(joined + a, i - a); a = i + 1; }
    ((std::unordered_set<std::string> *)h)->insert(v.begin(), v.end());
}
size_t set_dump(void *h, char *out, size_t cap) {
    std::string o;
    for (const std::string &t : *(std::unordered_set<std::string> *)h) { o += t; o += '\n'; }
    if (out && o.size() <= cap) memcpy(out, o.data(), o.size());
    return o.size();
}
}
'''


class Orders:
    def __init__(self, d):
        src, so = os.path.join(d, "uset.cpp"), os.path.join(d, "libuset.so")
        open(src, "w").write(HELPER)
        subprocess.check_call(["g++", "-O1", "-std=c++11", "-shared", "-fPIC", "-o", so, src])
        L = C.CDLL(so)
        L.tiles.restype = C.c_size_t
        L.tiles.argtypes = [C.c_char_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_char_p, C.c_size_t]
        L.set_new.restype = C.c_void_p
        L.set_free.argtypes = [C.c_void_p]
        L.set_insert.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
        L.set_dump.restype = C.c_size_t
        L.set_dump.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
        self.L = L

    def tiles(self, w, k, skip):
        n = self.L.tiles(w.encode(), len(w), k, skip, None, 0)
        buf = C.create_string_buffer(max(n, 1))
        self.L.tiles(w.encode(), len(w), k, skip, buf, n)
        return buf.raw[:n].decode().split("\n")[:-1] if n else []

    def fold(self, vectors):
        h = self.L.set_new()
        for v in vectors:
            b = "".join(x + "\n" for x in v).encode()
            self.L.set_insert(h, b, len(b))
        n = self.L.set_dump(h, None, 0)
        buf = C.create_string_buffer(max(n, 1))
        self.L.set_dump(h, buf, n)
        self.L.set_free(h)
        return buf.raw[:n].decode().split("\n")[:-1] if n else []


def find_kmer_reads(ref, orders, w, k, skip):
    """service.cpp:466-502 for k > 0, skip >= 0 (the other cases are answered empty)"""
    tiles = orders.tiles(w, k, skip)                      # :472
    vsize, sync, vectors = len(tiles), [], []
    for count, t in enumerate(tiles, 1):                  # :476
        if any(c not in "ACGT" for c in t):               # :477-479
            continue
        if count < vsize:                                 # :481-489: a MatchTask per tile
            vectors.append(msr.find_reads(ref, t))
            continue
        sync = msr.find_reads(ref, t)                     # :491-492: the last tile, synchronously, inserted FIRST
    return orders.fold([sync] + vectors)                  # :492, :496-498


def main():
    meta = json.load(open(os.path.join(HERE, "popbwt_v1.json")))
    subprocess.check_call(["make", "-C", os.path.join(msr.ROOT, "oracle"), "ref"])
    tmp = tempfile.mkdtemp()
    bwt_path, reads_path = os.path.join(tmp, "popbwt_v1.bwt"), os.path.join(tmp, "popbwt_v1.reads")
    rsb.build()
    rsb.synth_popbwt(bwt_path, reads_path, **meta["synth"])
    assert hashlib.sha256(open(bwt_path, "rb").read()).hexdigest() == meta["bwt_sha256"]
    reads = open(reads_path).read().split()
    ref, orders = msr.Ref(bwt_path), Orders(tmp)
    Request, Reply = proto_schema.build()
    rng = np.random.default_rng(31)
    rnd = lambda n: "".join("ACGT"[x] for x in rng.integers(0, 4, n))
    cut = lambda n: (lambda r: r[(s := int(rng.integers(0, len(r) - n + 1))):s + n])(reads[rng.integers(len(reads))])
    cases = []  # (q, k, skip)
    for k in (15, 31, 50, 60, 70):
        for skip in (0, 1, 5, 40):
            cases.append((cut(70) + cut(30), k, skip))                   # a region and its neighbour's
            cases.append((cut(70), k, skip))
    for k, skip in ((15, 0), (31, 1), (50, 5), (15, 40)):
        r = cut(70)
        cases.append((r[:35] + "N" + r[36:], k, skip))                   # a symbol outside ACGT
        cases.append((rnd(90), k, skip))                                  # absent
        cases.append((r[:k - 1], k, skip))                                # shorter than k
        cases.append((r[:20] * 4, k, skip))                               # repeated k-mers
        cases.append(("A" * 60, k, skip))
    cases.append((cut(12), 8, 0))                                          # wide intervals (the chunked order)
    cases.append((cut(20), 6, 3))
    items, big = [], 0
    for q, k, skip in cases:
        for rt in (1, 2):
            rq = Request()
            rq.t, rq.rt, rq.q, rq.k, rq.s = 3, rt, q, k, skip
            item = {"request": rq.SerializeToString().hex(), "t": 3, "rt": rt, "q": q, "k": k, "s": skip, "replies": [],
                    "reads": [], "channel": 0}
            for strand, w in ((0, q), (1, msr.rc(q))):                   # KmerTask::run, :883-885
                seqs = find_kmer_reads(ref, orders, w, k, skip)
                rep = Reply()
                rep.rt, rep.t, rep.q = 3, rt, q                            # :877-880
                if rt == 1:                                                # :889-897
                    (rep.c.revcomp_matches if strand else rep.c.forward_matches).c = len(seqs)
                else:                                                      # :898-910
                    rep.r.SetInParent()
                    for sq in seqs:
                        (rep.r.revcomp_matches if strand else rep.r.forward_matches).add().r = sq
                b = rep.SerializeToString()
                item["reads"].append(len(seqs))
                if len(b) > 4096:
                    item["replies"].append({"len": len(b), "sha256": hashlib.sha256(b).hexdigest()})
                    big += 1
                else:
                    item["replies"].append(b.hex())
            items.append(item)
    # unserved pairs: what the reference sends for an empty result (KmerTask :917-, QueryTask :1283-, GtTask :1136-);
    # `a` (ReplyAll, field 6) is not in the re-typed schema: an empty one is the two bytes 0x32 0x00 after q
    empty = []
    for t, rt in ((2, 3), (2, 4), (3, 3), (3, 4), (4, 1), (4, 2), (4, 3), (4, 4)):
        q = cut(60)
        rq = Request()
        rq.t, rq.rt, rq.q, rq.k, rq.s, rq.p = t, rt, q, 31, 0, 30
        reps = []
        for strand in (0, 1):
            rep = Reply()
            rep.rt, rep.t, rep.q = t, rt, q
            if rt == 1:
                (rep.c.revcomp_matches if strand else rep.c.forward_matches).c = 0
            elif rt == 2:
                rep.r.SetInParent()
            b = rep.SerializeToString() + (b"\x32\x00" if rt > 2 else b"")
            reps.append(b.hex())
        empty.append({"request": rq.SerializeToString().hex(), "t": t, "rt": rt, "q": q, "replies": reps, "channel": 0})
    json.dump(dict(what="KmerMatch Requests (Count, Reads) and the two Reply bytes (forward, reverse complement) a reference service "
                        "holding popbwt_v1 as its one partition sends for each (KmerTask::run + find_kmer_reads, service.cpp:466-502,"
                        "871-960) with min_read_length 50, max_read_length 70; reads from the compiled reference, unordered_set orders "
                        "from the C++ library; and the empty Replies of every unserved (t, rt) pair",
                   generator="tests/golden/make_service_kmer_golden.py", fixture="popbwt_v1.json",
                   min_read_length=msr.MIN_READ_LENGTH, max_read_length=msr.MAX_READ_LENGTH, items=items, unserved=empty),
              open(os.path.join(HERE, "service_kmer_v1.json"), "w"), indent=0)
    print(f"wrote service_kmer_v1.json: {len(items)} requests, {sum(sum(x['reads']) for x in items)} reads in their replies, "
          f"{big} replies stored as hashes, {sum(1 for x in items if sum(x['reads']) == 0)} without a read, {len(empty)} unserved")


if __name__ == "__main__":
    main()
