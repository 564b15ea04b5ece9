// sample_codes_host.cpp -- readserver_amd/csrc/sample_codes.h (the dictionary check and the key spelling of
// rsbwt_set_sample_counts) as a program of its own, for tests/test_sample_reference.py to build with
// -fsanitize=address,undefined and run.  Input on the command line: size_of_sample, then the codes in hex, back to back in
// one argument (may be empty).  Output: "status <n> bad <i>" and, when the dictionary is good, one "key <hex>" line per
// code, then "column <i>" for every code looked up again, for every code with its last byte changed, and for the keys 0
// and 2^64 - 1.  Heap copies sized exactly let the sanitizer see a read past either end.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../readserver_amd/csrc/sample_codes.h"

static int hexval(char c) {
    if (c >= '0' && c <= '9') return c - '0';
    if (c >= 'a' && c <= 'f') return c - 'a' + 10;
    if (c >= 'A' && c <= 'F') return c - 'A' + 10;
    return -1;
}

int main(int argc, char **argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: %s size_of_sample hexcodes\n", argv[0]);
        return 2;
    }
    const uint32_t ss = (uint32_t)strtoul(argv[1], nullptr, 10);
    const size_t hl = strlen(argv[2]);
    if (hl % 2) return 2;
    const size_t nbytes = hl / 2;
    uint8_t *codes = nbytes ? (uint8_t *)malloc(nbytes) : nullptr;  // exactly the bytes given
    for (size_t i = 0; i < nbytes; ++i) {
        const int a = hexval(argv[2][2 * i]), b = hexval(argv[2][2 * i + 1]);
        if (a < 0 || b < 0) return 2;
        codes[i] = (uint8_t)(a * 16 + b);
    }
    const size_t C = ss ? nbytes / ss : 0;
    std::vector<uint64_t> keys;
    size_t bad = 0;
    const int st = rsb::sample_codes_check(codes, C, ss, &keys, &bad);
    printf("status %d bad %zu\n", st, bad);
    if (st == rsb::SAMPLE_CODES_OK) {
        uint64_t *exact = (uint64_t *)malloc(C * sizeof(uint64_t));
        memcpy(exact, keys.data(), C * sizeof(uint64_t));
        for (size_t i = 0; i < C; ++i) printf("key %016llx\n", (unsigned long long)exact[i]);
        for (size_t i = 0; i < C; ++i) printf("column %zu\n", rsb::sample_column(exact, C, rsb::sample_key(codes + i * ss, ss)));
        for (size_t i = 0; i < C; ++i) {
            uint8_t tmp[rsb::SAMPLE_CODE_MAX];
            memcpy(tmp, codes + i * ss, ss);
            tmp[ss - 1] ^= 1u;
            printf("column %zu\n", rsb::sample_column(exact, C, rsb::sample_key(tmp, ss)));
        }
        printf("column %zu\n", rsb::sample_column(exact, C, 0ull));
        printf("column %zu\n", rsb::sample_column(exact, C, ~0ull));
        free(exact);
    }
    free(codes);
    puts("sample_codes ok");
    return 0;
}
