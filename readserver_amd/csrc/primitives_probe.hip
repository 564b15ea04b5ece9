// primitives_probe.hip -- test hooks (RSBWT_ENABLE_TEST_HOOKS) that run the rank primitives on their own, so that a test can
// hold each of them to a plain reference of its header comment instead of reaching it through the intervals a search
// happens to visit.  Answers no query; no other entry point reaches these kernels.
//
//   * rsbwt_debug_rank_primitives: one thread per CASE = the 24 piece bytes of a quarter (six dwords), a symbol b, one
//     argument; the primitive is named by an op code (include/rsbwt.h).  Every op that takes a symbol exists twice: with b
//     read from memory, and with b a compile-time constant 0..4 (a template instance per symbol) -- what hipcc makes of an
//     inline-asm block or a folded table depends on which it is.
//   * rsbwt_debug_staged_rank: one lane per position of a resident shard; the lane fetches the position's window line
//     into LDS as the search kernels and the '$' count do (glds_fetch, the swizzled stage, the header readers) and ranks
//     all five symbols off it (staged_occ_alts for every `orig`, staged_dollars).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "../../include/rsbwt.h"
#include "capi_internal.h"
#include "kernels.h"
#include "line_format.h"
#include "rank_device.h"
#include "wave_lines.h"

namespace rsb {

constexpr uint32_t PRIM_CASE_DWORDS = 8;    // r[0..5], b, arg
constexpr uint32_t STAGED_OUT_WORDS = 13;  // 4 x 3 Occ of the bases other than `orig`, Occ('$')

// out[] of one case (include/rsbwt.h, RSBWT_PRIM_*); forced inline, so a literal b stays one
__device__ __forceinline__ void prim_eval(uint32_t op, const uint32_t r[6], uint32_t b, uint32_t arg, uint32_t out[6]) {
    switch (op) {
    case RSBWT_PRIM_DWORD_MATCHED: {
        const uint32_t bb = b * 0x01010101u;
#pragma unroll
        for (int i = 0; i < 6; ++i) out[i] = dword_matched(r[i], bb, arg);
        break;
    }
    case RSBWT_PRIM_MATCHED24:
        out[0] = matched24_tab(r, make_sym_tab(b));
        break;
    case RSBWT_PRIM_RUNS_SCAN1:
        out[0] = runs_scan<1>(r, b, arg);
        break;
    case RSBWT_PRIM_RUNS_SCAN2:
        out[0] = runs_scan<2>(r, b, arg);
        break;
    case RSBWT_PRIM_RANK24:
        out[0] = rank24(r, make_sym_tab(b), b, arg);
        break;
    case RSBWT_PRIM_RANK24_DOLLAR:
        out[0] = rank24_dollar(r, make_sym_tab(0u), arg);
        break;
    case RSBWT_PRIM_CHAR_RANK24: {
        const char_rank c = char_rank24(r, arg, 0u);
        out[0] = c.c;
        out[1] = c.occ;
        break;
    }
    case RSBWT_PRIM_CHAR_RANK24_WANT: {
        const char_rank c = char_rank24(r, arg, b);
        out[0] = c.c;
        out[1] = c.occ;
        break;
    }
    case RSBWT_PRIM_SELECT_IN24: {
        uint32_t left = 0;
        out[0] = select_in24(r, b, arg, &left);
        out[1] = left;
        break;
    }
    default:
        break;
    }
}
template <uint32_t B>
__device__ __forceinline__ void prim_eval_const(uint32_t op, const uint32_t r[6], uint32_t arg, uint32_t out[6]) {
    prim_eval(op, r, B, arg, out);
}

// CONST_B: the case's symbol picks the instance compiled for it (a symbol above 4 has none: all-ones)
template <bool CONST_B>
__global__ void __launch_bounds__(256)
rank_primitives_kernel(const uint32_t *__restrict__ cases, size_t n, uint32_t op, uint32_t width, uint32_t *__restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint4 c0 = reinterpret_cast<const uint4 *>(cases)[2 * i], c1 = reinterpret_cast<const uint4 *>(cases)[2 * i + 1];
    const uint32_t r[6] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y};
    const uint32_t b = c1.z, arg = c1.w;
    uint32_t o[6] = {0, 0, 0, 0, 0, 0};
    if (CONST_B) {
        switch (b) {
        case 0: prim_eval_const<0>(op, r, arg, o); break;
        case 1: prim_eval_const<1>(op, r, arg, o); break;
        case 2: prim_eval_const<2>(op, r, arg, o); break;
        case 3: prim_eval_const<3>(op, r, arg, o); break;
        case 4: prim_eval_const<4>(op, r, arg, o); break;
        default:
#pragma unroll
            for (int k = 0; k < 6; ++k) o[k] = ~0u;
            break;
        }
    } else {
        prim_eval(op, r, b, arg, o);
    }
#pragma unroll
    for (uint32_t k = 0; k < 6u; ++k)
        if (k < width) out[i * width + k] = o[k];
}

// One lane per position; the fetch, the stage and the header readers are read_dollar_count_kernel's (read_lookup.hip).
// out[13 i ..]: Occ up to and including position i of the three bases other than `orig`, orig = A, C, G, T in turn (so
// every base comes out three times, from both sides of staged_occ_alts' `d < orig ? d : d + 1`), then Occ('$').  A position
// past its line's own pieces (spill chunk / far line): out[13 i] = all ones and nothing else is written -- out[13 i + 1 .. 12]
// stay the zeros rsbwt_debug_staged_rank fills the buffer with before the launch (include/rsbwt.h promises them).
__global__ void __launch_bounds__(64 * WG_WAVES)
staged_rank_kernel(const shard_view *__restrict__ sv, const uint64_t *__restrict__ pos, size_t n, uint64_t *__restrict__ out) {
    __shared__ uint4 s_stage[WG_WAVES][64 * SLOT_U4];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint4 *stage = s_stage[wave];
    const uint32_t stage_lds = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)(lds_void_ptr)stage);
    const char *lines_bytes = reinterpret_cast<const char *>(sv->lines);
    const uint32_t S = sv->sp.S;
    const double inv = sv->sp.inv;
    const uint32_t nlines = (uint32_t)sv->nlines;

    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t p = i < n ? pos[i] : ~0ull;
    const bool ok = i < n && p < sv->n;
    uint32_t w = 0, o = 0, want = ~0u;
    if (ok) {
        uint32_t pin;
        w = fast_window(p, S, inv, pin);
        o = pin + 1u;
        want = w + (w >> GROUP_SHIFT);
        if (want >= nlines) want = 0;  // never for p < n; keeps a bad position from faulting
    }
    glds_fetch(lines_bytes, want, lane, stage_lds);  // (every lane takes part)
    glds_wait();
    if (!ok) return;
    const staged_line L = {own_stage_row(stage, lane), lane & 7u};
    const line_head h = read_head(L);
    uint64_t *dst = out + (size_t)STAGED_OUT_WORDS * i;
    if (o > h.span) {
        dst[0] = ~0ull;
        return;
    }
#pragma unroll
    for (uint32_t orig = 0; orig < 4u; ++orig) {
        uint64_t alt[3];
        staged_occ_alts(L, h, o, orig, alt);
        dst[3u * orig] = alt[0];
        dst[3u * orig + 1u] = alt[1];
        dst[3u * orig + 2u] = alt[2];
    }
    const uint64_t before = (uint64_t)w * S - (read_count(L, 1u) + read_count(L, 2u) + read_count(L, 3u) + read_count(L, 4u));
    dst[12] = before + staged_dollars(L, h, o);
}

}  // namespace rsb

using namespace rsb;

static bool hooks_enabled() { return getenv("RSBWT_ENABLE_TEST_HOOKS") != nullptr; }

extern "C" int rsbwt_debug_rank_primitives(uint32_t op, int const_b, const uint32_t *cases, size_t n, uint32_t *out, int device) {
    if ((!cases || !out) && n) return fail(RSBWT_EINVAL, "null argument");
    if (!hooks_enabled()) return fail(RSBWT_EINVAL, "rsbwt_debug_rank_primitives is a test hook: set RSBWT_ENABLE_TEST_HOOKS=1");
    if (op > RSBWT_PRIM_SELECT_IN24) return fail(RSBWT_EINVAL, "no primitive %u", op);
    if (n == 0) return RSBWT_OK;
    if (n > (1u << 28)) return fail(RSBWT_ERANGE, "%zu cases in one call (at most 2^28)", n);
    int rc = use_device(device);
    if (rc != RSBWT_OK) return rc;
    const uint32_t width = op == RSBWT_PRIM_DWORD_MATCHED ? 6u : 2u;
    const size_t in_bytes = n * PRIM_CASE_DWORDS * sizeof(uint32_t), out_bytes = n * width * sizeof(uint32_t);
    uint8_t *d = nullptr;
    hipError_t e = hipMalloc(&d, in_bytes + out_bytes);
    if (e != hipSuccess) return fail_hip(e, "hipMalloc");
    uint32_t *d_cases = reinterpret_cast<uint32_t *>(d), *d_out = reinterpret_cast<uint32_t *>(d + in_bytes);
    e = hipMemcpy(d_cases, cases, in_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        const dim3 grid((unsigned)((n + 255) / 256));
        if (const_b)
            hipLaunchKernelGGL(rank_primitives_kernel<true>, grid, dim3(256), 0, nullptr, d_cases, n, op, width, d_out);
        else
            hipLaunchKernelGGL(rank_primitives_kernel<false>, grid, dim3(256), 0, nullptr, d_cases, n, op, width, d_out);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(out, d_out, out_bytes, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    return e == hipSuccess ? RSBWT_OK : fail_hip(e, "rsbwt_debug_rank_primitives");
}

extern "C" int rsbwt_debug_staged_rank(rsbwt_t *h, const uint64_t *positions, size_t n, uint64_t *out) {
    if (!h || ((!positions || !out) && n)) return fail(RSBWT_EINVAL, "null argument");
    if (!hooks_enabled()) return fail(RSBWT_EINVAL, "rsbwt_debug_staged_rank is a test hook: set RSBWT_ENABLE_TEST_HOOKS=1");
    if (n == 0) return RSBWT_OK;
    if (n > (1u << 28)) return fail(RSBWT_ERANGE, "%zu positions in one call (at most 2^28)", n);
    for (size_t i = 0; i < n; ++i)
        if (positions[i] >= h->view.n) return fail(RSBWT_ERANGE, "position %llu past the index", (unsigned long long)positions[i]);
    int rc = use_device(h->device);
    if (rc != RSBWT_OK) return rc;
    const size_t in_bytes = n * sizeof(uint64_t), out_bytes = n * STAGED_OUT_WORDS * sizeof(uint64_t);
    uint8_t *d = nullptr;
    hipError_t e = hipMalloc(&d, in_bytes + out_bytes);
    if (e != hipSuccess) return fail_hip(e, "hipMalloc");
    uint64_t *d_pos = reinterpret_cast<uint64_t *>(d), *d_out = reinterpret_cast<uint64_t *>(d + in_bytes);
    e = hipMemcpy(d_pos, positions, in_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(d_out, 0, out_bytes);
    if (e == hipSuccess) {
        const dim3 grid((unsigned)((n + 64 * WG_WAVES - 1) / (64 * WG_WAVES)));
        hipLaunchKernelGGL(staged_rank_kernel, grid, dim3(64 * WG_WAVES), 0, nullptr, h->d_view, d_pos, n, d_out);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(out, d_out, out_bytes, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    return e == hipSuccess ? RSBWT_OK : fail_hip(e, "rsbwt_debug_staged_rank");
}
