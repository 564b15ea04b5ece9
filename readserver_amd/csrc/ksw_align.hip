// ksw_align.hip -- ksw_align of the reference's src/service/ksw.c and align_gt_read (src/service/service.cpp:105-225) on
// the GPU: one lane per (read, target) item, ksw_pass.h's scalar walk.  A block is one wave of 64 items.  The lane's
// column (H and E as packed 16-bit pairs, a word per row, and the rows' codes as nibbles) is laid out [row][lane]: a
// wave's lanes hit 64 consecutive words, distinct banks in LDS and one coalesced run in HBM.  A block of the 104-row
// class costs 64 x (104 + 13) x 4 B = 29.3 KiB of LDS, five to a CU; a block whose longest pass has more than
// KSW_LDS_ROWS rows keeps its columns in a scratch buffer in HBM instead -- the same code over a different pointer.
// One launch per length class, each taking exactly the blocks of its class (kernels.h).
#include <hip/hip_runtime.h>

#include "../../include/rsbwt.h"
#include "kernels.h"
#include "ksw_pass.h"

namespace rsb {
namespace {

constexpr uint32_t LANES = 64;
constexpr uint32_t CLASS_ROWS[] = {32, 64, 104, 160, KSW_LDS_ROWS};
static_assert(KSW_LDS_ROWS == RSBWT_KSW_LDS_ROWS && ksw::MAX_LEN == RSBWT_KSW_MAX_LEN, "the header's numbers");

__host__ __device__ inline uint32_t words_per_lane(uint32_t rows) { return rows + ((rows + 7u) >> 3); }
static_assert((KSW_LDS_ROWS + (KSW_LDS_ROWS + 7) / 8) * LANES * 4 <= 65536, "the widest class fits a workgroup's LDS");

// the block's longest pass (0: no valid item), the same value in every lane: the block is one wave, and every lane of it
// is here together (the loops over blocks have no divergent exit)
__device__ inline uint32_t block_rows(uint32_t mine) {
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t other = (uint32_t)__shfl_xor((int)mine, d, 64);
        mine = mine > other ? mine : other;
    }
    return mine;
}

// The lane's column for a block whose longest pass has `need` rows, or rows = 0 when the block belongs to another
// launch: this one takes lo <= need <= hi.  LDS: hi rows per lane in the launch's dynamic LDS.  HBM: hi rows per lane in
// the slot of this resident block (gridDim.x <= KSW_HBM_BLOCKS slots of 64 x words_per_lane(hi) words).
template <bool HBM>
__device__ inline ksw::column lane_column(uint32_t need, uint32_t lo, uint32_t hi, uint32_t *lds, uint32_t *scratch) {
    if (need < lo || need > hi) return ksw::column{nullptr, nullptr, LANES, 0};
    if (HBM) {
        uint32_t *base = scratch + (size_t)blockIdx.x * LANES * words_per_lane(hi) + threadIdx.x;
        return ksw::column{base, base + (size_t)hi * LANES, LANES, (int)hi};
    }
    return ksw::column{lds + threadIdx.x, lds + hi * LANES + threadIdx.x, LANES, (int)hi};
}

template <bool HBM>
__global__ __launch_bounds__(64) void ksw_align_kernel(ksw_batch bt, uint32_t lo, uint32_t hi, uint32_t *scratch, rsbwt_ksw_result *out) {
    extern __shared__ uint32_t lds[];
    const ksw::scores s{bt.match, bt.mismatch, bt.ambiguous, bt.gapo + bt.gape, bt.gape};
    const size_t nblocks = (bt.n + LANES - 1) / LANES;
    for (size_t blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
        const size_t g = blk * LANES + threadIdx.x;
        const bool active = g < bt.n;
        const size_t i = active ? (bt.perm ? (size_t)bt.perm[g] : g) : 0;
        uint64_t q0 = 0, t0 = 0, ql = 0, tl = 0;
        bool valid = false;
        if (active) {
            q0 = bt.qoff[i];
            t0 = bt.toff[i];
            ql = bt.qoff[i + 1] - q0;
            tl = bt.toff[i + 1] - t0;
            valid = ql >= 1 && ql <= (uint64_t)ksw::MAX_LEN && tl >= 1 && tl <= (uint64_t)ksw::MAX_LEN &&
                    (uint64_t)bt.match * (ql < tl ? ql : tl) < 32768ull;
        }
        const uint32_t need = block_rows(valid ? (uint32_t)ql : 0u);
        const ksw::column col = lane_column<HBM>(need, lo, hi, lds, scratch);
        if (col.rows != 0 && active) {
            if (valid) {
                const ksw::seq_view q{bt.qtext + q0, (int)ql, 0, -1, 0}, t{bt.ttext + t0, (int)tl, 0, -1, 0};
                const ksw::align_result r = ksw::align(s, q, t, col);
                out[i] = rsbwt_ksw_result{r.score, r.te, r.qe, r.tb, r.qb, 0};
            } else {
                out[i] = rsbwt_ksw_result{-1, -1, -1, -1, -1, 0};
            }
        }
    }
}

template <bool HBM>
__global__ __launch_bounds__(64) void gt_align_kernel(gt_align_batch bt, uint32_t lo, uint32_t hi, uint32_t *scratch, uint8_t *verdict,
                                                      unsigned long long *work14) {
    extern __shared__ uint32_t lds[];
    const ksw::scores s{1, 4, 1, 6 + 1, 1};  // service.cpp:108-114, gapo 6 and gape 1
    const size_t nblocks = (bt.n + LANES - 1) / LANES;
    for (size_t blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
        const size_t g = blk * LANES + threadIdx.x;
        const bool active = g < bt.n;
        const size_t i = active ? (bt.perm ? (size_t)bt.perm[g] : g) : 0;
        uint64_t rl = 0, w0 = 0, wl = 0, rq = 0;
        const char *rp = nullptr;
        bool valid = false;
        if (active) {
            if (bt.rid) {  // (the launch's constant: every lane takes the same side)
                const uint32_t r = bt.rid[i];
                rp = reinterpret_cast<const char *>((uintptr_t)bt.raddr[r]);
                rl = bt.rlen[r];
            } else {
                const uint64_t r0 = bt.roff[i];
                rp = bt.reads + r0;
                rl = bt.roff[i + 1] - r0;
            }
            rq = bt.item[i];
            if (rq < bt.Q) {
                w0 = bt.off[rq];
                wl = bt.off[rq + 1] - w0;
                valid = rl >= 1 && rl <= (uint64_t)ksw::MAX_LEN && wl >= 1 && wl <= (uint64_t)ksw::MAX_LEN;
            }
        }
        // (the sub-alignments of :196-221 put a piece of w on the rows: the column holds the longer of the two)
        const uint32_t need = block_rows(valid ? (uint32_t)(rl > wl ? rl : wl) : 0u);
        const ksw::column col = lane_column<HBM>(need, lo, hi, lds, scratch);
        if (col.rows != 0 && active) {
            if (valid) {
                const int v = ksw::gt_verdict(s, rp, (int)rl, bt.text + w0, (int)wl, bt.pos[rq], ksw::nt4((unsigned char)bt.alt[rq]),
                                              bt.isalt[rq] != 0, col);
                verdict[i] = (uint8_t)v;
                if (work14) {
                    atomicAdd(&work14[0], 1ull);
                    atomicAdd(&work14[v], 1ull);
                }
            } else {
                verdict[i] = (uint8_t)RSBWT_GT_INVALID;
            }
        }
    }
}

// one launch per class that [min_rows, max_rows] reaches; the first one launched also takes the blocks with no valid item
template <class F>
hipError_t for_each_class(size_t n, uint32_t min_rows, uint32_t max_rows, void *d_scratch, F &&launch) {
    if (min_rows > max_rows || max_rows > (uint32_t)ksw::MAX_LEN) return hipErrorInvalidValue;
    if (max_rows > KSW_LDS_ROWS && !d_scratch) return hipErrorInvalidValue;
    const size_t nblocks = (n + LANES - 1) / LANES;
    uint32_t lo = 0;  // what the next launch starts at
    for (uint32_t hi : CLASS_ROWS) {
        if (min_rows > hi) continue;  // (nothing that short: lo stays, the next class takes it all)
        const unsigned grid = (unsigned)(nblocks < 4096 ? nblocks : 4096);
        launch(false, grid, (size_t)LANES * 4u * words_per_lane(hi), lo, hi);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        lo = hi + 1;
        if (max_rows <= hi) return hipSuccess;
    }
    const unsigned grid = (unsigned)(nblocks < KSW_HBM_BLOCKS ? nblocks : KSW_HBM_BLOCKS);
    launch(true, grid, (size_t)0, lo, max_rows);
    return hipGetLastError();
}

}  // namespace

size_t ksw_scratch_bytes(uint32_t max_rows) {
    return max_rows > KSW_LDS_ROWS ? (size_t)KSW_HBM_BLOCKS * LANES * 4u * words_per_lane(max_rows) : 0;
}

hipError_t launch_ksw_align(const ksw_batch &bt, uint32_t min_rows, uint32_t max_rows, void *d_scratch, void *d_out, hipStream_t stream) {
    if (bt.n == 0) return hipSuccess;
    return for_each_class(bt.n, min_rows, max_rows, d_scratch, [&](bool hbm, unsigned grid, size_t lds, uint32_t lo, uint32_t hi) {
        if (hbm)
            hipLaunchKernelGGL(ksw_align_kernel<true>, dim3(grid), dim3(LANES), 0, stream, bt, lo, hi, (uint32_t *)d_scratch, (rsbwt_ksw_result *)d_out);
        else
            hipLaunchKernelGGL(ksw_align_kernel<false>, dim3(grid), dim3(LANES), lds, stream, bt, lo, hi, (uint32_t *)nullptr, (rsbwt_ksw_result *)d_out);
    });
}

hipError_t launch_gt_align(const gt_align_batch &bt, uint32_t min_rows, uint32_t max_rows, void *d_scratch, void *d_verdict,
                           unsigned long long *d_work14, hipStream_t stream) {
    if (bt.n == 0) return hipSuccess;
    return for_each_class(bt.n, min_rows, max_rows, d_scratch, [&](bool hbm, unsigned grid, size_t lds, uint32_t lo, uint32_t hi) {
        if (hbm)
            hipLaunchKernelGGL(gt_align_kernel<true>, dim3(grid), dim3(LANES), 0, stream, bt, lo, hi, (uint32_t *)d_scratch, (uint8_t *)d_verdict, d_work14);
        else
            hipLaunchKernelGGL(gt_align_kernel<false>, dim3(grid), dim3(LANES), lds, stream, bt, lo, hi, (uint32_t *)nullptr, (uint8_t *)d_verdict,
                               d_work14);
    });
}

}  // namespace rsb
