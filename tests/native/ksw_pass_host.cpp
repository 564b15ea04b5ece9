// ksw_pass_host.cpp -- TEST INFRASTRUCTURE: csrc/ksw_pass.h (the lane's walk of ksw_align.hip) compiled for the host.
// Reads records from the file named on the command line and prints one answer line each:
//   K match mismatch ambiguous gapo gape stride query target   ->  score te qe tb qb
//   G stride read window pos alt isalt                         ->  verdict
// The column is allocated exactly as large as the kernel's would be for the record (rows x stride words + the code
// words) with `stride` lanes, the lane under test in the middle, so an index outside the lane's own words is a heap
// overflow the sanitizers see, and every other lane's words must still hold their fill pattern afterwards.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "ksw_pass.h"

using namespace rsb::ksw;

struct lane_store {
    std::vector<uint32_t> w;
    uint32_t stride, lane;
    int rows;
    lane_store(int r, uint32_t s) : w((size_t)(r + (r + 7) / 8) * s, 0xDEADBEEFu), stride(s), lane(s / 2), rows(r) {}
    column col() { return column{w.data() + lane, w.data() + (size_t)rows * stride + lane, stride, rows}; }
    bool others_untouched() const {
        for (size_t i = 0; i < w.size(); ++i)
            if (i % stride != lane && w[i] != 0xDEADBEEFu) return false;
        return true;
    }
};

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    std::ifstream in(argv[1]);
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ss(line);
        std::string kind;
        ss >> kind;
        if (kind == "K") {
            int m, x, a, go, ge;
            uint32_t stride;
            std::string q, t;
            ss >> m >> x >> a >> go >> ge >> stride >> q >> t;
            lane_store st((int)q.size(), stride);
            const scores s{m, x, a, go + ge, ge};
            const seq_view qv{q.data(), (int)q.size(), 0, -1, 0}, tv{t.data(), (int)t.size(), 0, -1, 0};
            const align_result r = align(s, qv, tv, st.col());
            if (!st.others_untouched()) return 3;
            printf("%d %d %d %d %d\n", r.score, r.te, r.qe, r.tb, r.qb);
        } else if (kind == "G") {
            uint32_t stride;
            std::string rd, w, alt;
            unsigned long long pos;
            int isalt;
            ss >> stride >> rd >> w >> pos >> alt >> isalt;
            lane_store st((int)std::max(rd.size(), w.size()), stride);
            const scores s{1, 4, 1, 7, 1};
            const int v = gt_verdict(s, rd.data(), (int)rd.size(), w.data(), (int)w.size(), pos, nt4((unsigned char)alt[0]), isalt != 0, st.col());
            if (!st.others_untouched()) return 3;
            printf("%d\n", v);
        }
    }
    return 0;
}
