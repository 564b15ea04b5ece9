// kmer_reads.h -- KmerMatch's find_kmer_reads (src/service/service.cpp:466-502) over a shard set: what kmer_reads.hip
// (device identity walks + the host replay of the reference's unordered_set) offers the C-ABI and the service loop.
#ifndef RSBWT_KMER_READS_H
#define RSBWT_KMER_READS_H

#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/rsbwt.h"

namespace rsb {

// Work of one call (rsbwt_set_kmer_last_work): candidate rows (every row of every tile's interval, summed over the
// shards), rows whose walk went on to '$', LF steps of those walks, distinct (shard, read identity) pairs, reads
// extracted.
// extracted counts the rows handed to the extraction calls (a read longer than the stride is extracted twice).
// ms_device: wall time inside the calls that wait for the device (search, exact-match, identity walks, extraction);
// the rest of ms_total is host work (tiles, segments, sorts, the set).
struct kmer_work {
    uint64_t candidates = 0, walked = 0, lf_steps = 0, identities = 0, extracted = 0;
    double ms_total = 0, ms_device = 0;
};

// A shard's segments: the non-empty tile intervals of a call, candidate rows first[i] .. first[i+1] = rows lo[i] ..;
// pred[i] = the segment of the tile at p - skip - 1 (0xFFFFFFFF: none), whose check symbols are text[chk[i] - j] for
// j < chklen[i] (w[p-1] down to w[p-skip-1]).
struct kr_segments {
    std::vector<uint64_t> first, lo, chk;
    std::vector<uint32_t> pred, chklen;
};
int kmer_ident_shard(rsbwt_t *h, const kr_segments &sg, const std::string &text, std::vector<uint64_t> *ident, kmer_work *work);

// One (query, strand) of find_kmer_reads: w is already the strand's string.  k <= 0, skip < 0 or |w| < k: no tiles.
struct kmer_job {
    std::string w;
    int64_t k = 0, skip = 0;
};
// out[j][p]: the distinct reads job j finds in shard p, in the order of the reference's unordered_set.  failed[j] = 1:
// job j could not be answered (its lists are empty) -- a job whose candidate rows run into the millions goes through
// the device on its own, so that its failure touches no other job.  read_stride: the extraction buffer per read.
// min / max_read_length: find_reads' three branches (service.cpp:714-797) -- a tile shorter than min_read_length
// stands for the reads of its interval's rows, a longer one for its sub-tiles that are reads (and, below
// max_read_length, the reads that contain it).
int kmer_reads_batch(rsbwt_set_t *set, const std::vector<kmer_job> &jobs, size_t min_read_length, size_t max_read_length, uint32_t read_stride,
                     std::vector<std::vector<std::vector<std::string>>> *out, std::vector<char> *failed, kmer_work *work);

// What the service code (service_slice.cpp, service_loop.cpp: host-only translation units that the CPU harnesses under
// tests/native build without the engine) reaches the k-mer path through: filled in by kmer_reads.hip when the engine
// is linked; empty otherwise (the KmerMatch path then answers RSBWT_ENODEV).
struct kmer_engine {
    int (*batch)(rsbwt_set_t *, const std::vector<kmer_job> &, size_t, size_t, uint32_t, std::vector<std::vector<std::vector<std::string>>> *,
                 std::vector<char> *, kmer_work *);
    int (*opened_for_reads)(const rsbwt_t *);
};
extern kmer_engine kmer_engine_hooks;

}  // namespace rsb
#endif
