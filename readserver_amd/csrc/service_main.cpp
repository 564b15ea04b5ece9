// service_main.cpp -- `rsbwt_service <service.cfg>`: the GPU twin of ReadServer's `service` process for
// the BWT-only paths (src/service/service.cpp:1366-1583).  Reads the same configuration file, loads the
// BWT(s) into HBM, connects the same three sockets and answers CountReads, ExactMatch-Count and ExactMatch-Reads
// requests in micro-batches (`GET /get?output=count|reads`), and KmerMatch Count / Reads when `kmermatch = "on"`;
// with `meta = "<pairs file>"` also ExactMatch requests whose return type is All or Samples (`output=all`, what
// scripts/client.pl asks for by default) and, with kmermatch on, KmerMatch ones: every read with its samples, from a
// table in HBM built from the file the reference loads into RocksDB.  SiteMatch requests (`/gt`) are answered when
// `sitematch = "on"`: Count and Reads, and All / Samples with `meta`; the reads of a Reply come in ascending read_row per
// partition, not in the reference's unordered_set order.  Requests of other types (SiteMatch with sitematch off; All / Samples
// without `meta`) are left unanswered unless `unserved = "empty"` (they belong to the RocksDB-backed paths of the
// reference's service, which can run beside this process on `push`).
//
// One process may hold many partitions: besides the reference's `prefix` (one BWT), the engine reads
//   shards  = [ "<prefix of shard 0>", ... ];     one .bwt per suffix partition (64)
//   devices = [ "0", "0", ..., "7" ];             HIP device of each shard (default: shard s -> GPU s * ndev / nshards)
//   batch_window_us = "200";  batch_max = "4096";  replies = "per_partition" | "summed";
//   query_threads = "8";                          windows answered at once (the reference's query pool: service.cpp:88)
//   suffixes = [ "<suffix of shard 0>", ... ];    the partitions' `suffix` values (default: `suffix` for a single shard)
//   reads = "on" | "off";                         off: ExactMatch-Reads requests are not answered here
//   kmermatch = "on" | "off";                     on: KmerMatch Count / Reads requests are answered here (default off)
//   sitematch = "on" | "off";                     on: SiteMatch requests are answered here (rsbwt_set_site_reads; needs
//                                                 max_read_length <= 2048; default off)
//   exactmatch = "extract" | "search";            how "is this tile itself a read?" is answered (Reads, KmerMatch): by extracting
//                                                 the reads of its interval, or by backward search from the terminator
//                                                 rows (rsbwt_exactmatch_by_search); the replies are the same (default extract)
//   max_match_reads = "100000";                   an ExactMatch-Reads query (each strand by itself) that brings more reads than
//                                                 this over all shards is answered with none (default: absent or "0", no limit)
//   meta = "<pairs file>";                        the file load_data_into_rocksdb reads (line 1 a read, line 2 its value, repeated;
//                                                 the reads.ids files of all partitions concatenated): loaded into the
//                                                 per-read sample table in HBM, and All / Samples requests are answered with
//                                                 `hashfile`, `size_of_sample` and `has_other_meta_data` as the reference reads
//                                                 them (service.cpp:1410-1415,1425,1477-1488); needs reads = "on" (default: absent)
//   unserved = "empty";                           requests of any other kind get 2 x shards Replies with no matches
//                                                 (default: no reply, as before)
// and then sends 2 x shards replies per request (front-end `workers` = 2 x shards) or 2 (`summed`).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/rsbwt.h"

static const char *get(const rsbwt_service_config_t *c, const char *k, const char *dflt) {
    const char *v = rsbwt_service_config_get(c, k);
    return v ? v : dflt;
}

int main(int argc, char **argv) {
    if (argc < 2) {
        fprintf(stderr, "Require more arguments to run the programme.\nusage: %s <service.cfg>\n", argv[0]);
        return EXIT_FAILURE;
    }
    rsbwt_service_config_t *cfg = nullptr;
    if (rsbwt_service_config_load(argv[1], &cfg) != RSBWT_OK) {
        fprintf(stderr, "%s\n", rsbwt_last_error());
        return EXIT_FAILURE;
    }
    // the opt-in keys, checked before anything is connected or loaded
    const char *kmermatch = get(cfg, "kmermatch", "off"), *unserved = get(cfg, "unserved", "");
    if (strcmp(kmermatch, "on") != 0 && strcmp(kmermatch, "off") != 0) {
        fprintf(stderr, "service.cfg: kmermatch = \"%s\": \"on\" or \"off\"\n", kmermatch);
        return EXIT_FAILURE;
    }
    const char *sitematch = get(cfg, "sitematch", "off");
    if (strcmp(sitematch, "on") != 0 && strcmp(sitematch, "off") != 0) {
        fprintf(stderr, "service.cfg: sitematch = \"%s\": \"on\" or \"off\"\n", sitematch);
        return EXIT_FAILURE;
    }
    const bool serve_site = strcmp(sitematch, "on") == 0;
    if (*unserved && strcmp(unserved, "empty") != 0) {
        fprintf(stderr, "service.cfg: unserved = \"%s\": the one value known is \"empty\"\n", unserved);
        return EXIT_FAILURE;
    }
    const char *exactmatch = get(cfg, "exactmatch", "extract");
    if (strcmp(exactmatch, "extract") != 0 && strcmp(exactmatch, "search") != 0) {
        fprintf(stderr, "service.cfg: exactmatch = \"%s\": \"extract\" or \"search\"\n", exactmatch);
        return EXIT_FAILURE;
    }
    const char *max_match = get(cfg, "max_match_reads", "0");
    if (!*max_match || strspn(max_match, "0123456789") != strlen(max_match) || strlen(max_match) > 19) {
        fprintf(stderr, "service.cfg: max_match_reads = \"%s\": a non-negative decimal number\n", max_match);
        return EXIT_FAILURE;
    }
    const bool serve_kmer = strcmp(kmermatch, "on") == 0;
    const char *meta = get(cfg, "meta", "");
    const char *sos = get(cfg, "size_of_sample", "2");  // (defaults: service.cpp:59-60)
    if (*meta && (!*sos || strspn(sos, "0123456789") != strlen(sos) || strlen(sos) > 6)) {
        fprintf(stderr, "service.cfg: size_of_sample = \"%s\": a non-negative decimal number\n", sos);
        return EXIT_FAILURE;
    }
    printf("starting server for %s\n", get(cfg, "suffix", ""));
    // the sockets first: a box without libzmq should say so before minutes are spent loading shards into HBM
    // (connecting is asynchronous in ZeroMQ: nothing is received until the loop polls)
    rsbwt_transport_t *tr = nullptr;
    if (rsbwt_transport_zmq(get(cfg, "pull", ""), get(cfg, "push", ""), get(cfg, "push_count", ""), &tr) != RSBWT_OK) {
        fprintf(stderr, "%s\n", rsbwt_last_error());
        return EXIT_FAILURE;
    }
    std::vector<std::string> paths;
    const size_t ns = rsbwt_service_config_array_len(cfg, "shards");
    for (size_t i = 0; i < ns; ++i) paths.push_back(std::string(rsbwt_service_config_array_item(cfg, "shards", i)) + ".bwt");
    if (paths.empty()) paths.push_back(std::string(get(cfg, "prefix", "")) + ".bwt");
    const int ndev = rsbwt_device_count();
    if (ndev <= 0) {
        fprintf(stderr, "no HIP device is visible: the popBWT engine has no CPU fallback\n");
        return EXIT_FAILURE;
    }
    std::vector<int> devs(paths.size());
    const size_t nd = rsbwt_service_config_array_len(cfg, "devices");
    for (size_t i = 0; i < paths.size(); ++i)
        devs[i] = i < nd ? atoi(rsbwt_service_config_array_item(cfg, "devices", i)) : (int)(i * (size_t)ndev / paths.size());
    std::vector<const char *> cpaths;
    for (const std::string &p : paths) cpaths.push_back(p.c_str());
    rsbwt_set_t *set = nullptr;
    // (shards that serve reads are laid out with a psi hint in every window line and their select samples, built at open:
    // include/rsbwt.h, RSBWT_OPEN_READS)
    const bool serve_reads = strcmp(get(cfg, "reads", "on"), "off") != 0;
    if (rsbwt_set_open(cpaths.data(), cpaths.size(), devs.data(),
                       RSBWT_OPEN_KTAB_GROUPED | (serve_reads || serve_kmer || serve_site || *meta ? RSBWT_OPEN_READS : 0u), &set) != RSBWT_OK) {
        fprintf(stderr, "%s\n", rsbwt_last_error());
        return EXIT_FAILURE;
    }
    if (strcmp(exactmatch, "search") == 0 && rsbwt_set_exactmatch_by_search(set, 1) != RSBWT_OK) {
        fprintf(stderr, "%s\n", rsbwt_last_error());
        return EXIT_FAILURE;
    }
    printf("loaded %zu bwt shard(s) on %zu GPU(s).\n", rsbwt_set_size(set), rsbwt_set_devices(set));
    if (*meta) {
        uint64_t st[4] = {0, 0, 0, 0};
        if (rsbwt_set_meta_load(set, meta, st) != RSBWT_OK) {
            fprintf(stderr, "%s\n", rsbwt_last_error());
            return EXIT_FAILURE;
        }
        printf("loaded the sample table: %llu pairs matched, %llu matched no shard, %llu reads with samples, %llu bytes in HBM.\n",
               (unsigned long long)st[0], (unsigned long long)st[1], (unsigned long long)st[2], (unsigned long long)rsbwt_set_meta_bytes(set));
    }
    rsbwt_service_t *svc = nullptr;
    const bool summed = strcmp(get(cfg, "replies", "per_partition"), "summed") == 0;
    if (rsbwt_service_create(set, tr, atoll(get(cfg, "batch_window_us", "200")), (size_t)atoll(get(cfg, "batch_max", "4096")),
                             summed ? 0 : 1, &svc) != RSBWT_OK) {
        fprintf(stderr, "%s\n", rsbwt_last_error());
        return EXIT_FAILURE;
    }
    rsbwt_service_set_workers(svc, atoi(get(cfg, "query_threads", "8")));
    // min_read_length / max_read_length: service.cpp:1417-1420 (defaults 73 / 100, :56-57)
    rsbwt_service_set_reads(svc, serve_reads ? 1 : 0, (uint32_t)atoi(get(cfg, "min_read_length", "0")), (uint32_t)atoi(get(cfg, "max_read_length", "0")));
    if (rsbwt_service_set_kmermatch(svc, serve_kmer ? 1 : 0) != RSBWT_OK) {
        fprintf(stderr, "%s\n", rsbwt_last_error());
        return EXIT_FAILURE;
    }
    if (rsbwt_service_set_sitematch(svc, serve_site ? 1 : 0) != RSBWT_OK) {
        fprintf(stderr, "%s\n", rsbwt_last_error());
        return EXIT_FAILURE;
    }
    if (rsbwt_service_set_max_match_reads(svc, strtoull(max_match, nullptr, 10)) != RSBWT_OK) {
        fprintf(stderr, "%s\n", rsbwt_last_error());
        return EXIT_FAILURE;
    }
    // has_other_meta_data: "1" turns it on, anything else off (service.cpp:1413-1415); absent: on (:60)
    if (*meta && rsbwt_service_set_all(svc, 1, get(cfg, "hashfile", ""), (uint32_t)atoi(sos),
                                       rsbwt_service_config_get(cfg, "has_other_meta_data") ? strcmp(get(cfg, "has_other_meta_data", ""), "1") == 0 : 1) != RSBWT_OK) {
        fprintf(stderr, "%s\n", rsbwt_last_error());
        return EXIT_FAILURE;
    }
    rsbwt_service_set_unserved(svc, *unserved ? 1 : 0);
    {
        std::vector<std::string> suf;
        const size_t nsuf = rsbwt_service_config_array_len(cfg, "suffixes");
        for (size_t i = 0; i < paths.size(); ++i)
            suf.push_back(i < nsuf ? rsbwt_service_config_array_item(cfg, "suffixes", i) : (paths.size() == 1 ? get(cfg, "suffix", "") : ""));
        std::vector<const char *> csuf;
        for (const std::string &x : suf) csuf.push_back(x.c_str());
        if (rsbwt_service_set_suffixes(svc, csuf.data(), csuf.size()) != RSBWT_OK) {
            fprintf(stderr, "%s\n", rsbwt_last_error());
            return EXIT_FAILURE;
        }
    }
    printf("ready to serve from %s\n", get(cfg, "suffix", ""));
    fflush(stdout);
    const int rc = rsbwt_service_run(svc);  // forever (service.cpp:1521)
    rsbwt_service_free(svc);
    rsbwt_transport_free(tr);
    rsbwt_set_close(set);
    rsbwt_service_config_free(cfg);
    return rc == RSBWT_OK ? 0 : EXIT_FAILURE;
}
