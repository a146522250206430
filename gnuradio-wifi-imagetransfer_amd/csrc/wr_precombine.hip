// wr_precombine.hip -- pre-detection combining (NUMERICS.md rule 33): the samples of up to 8 antennas that received the same
// transmission become ONE row set, y[n] = sum_a conj(v_a) x_a[n], in front of the demodulator.  The weights v are blind: the
// principal eigenvector of the slot's A x A sample covariance R, from the column of the strongest antenna and `iters` power
// iterations.  For a flat channel (one complex gain per antenna, the reference's AP model) this is maximal-ratio combining
// on the samples, so detection, LTS search, SIGNAL and the channel estimate all see the array gain and the demod runs once.
//
// Work split: one workgroup of four waves owns one slot.  Wave w takes the tiles t = w, w + 4, ... of 64 samples, lane <->
// sample, so every load is one coalesced 512-byte row per antenna.
//   pass 1   the upper triangle of R in registers (A (A + 1) / 2 complex fma chains per lane, 36 for A = 8); the 64 lanes of a
//            wave fold by the xor butterfly of wr_irs_elem.h, the four waves meet in LDS and add as (w0 + w1) + (w2 + w3)
//   algebra  wave 0 reads the full R from LDS (the column of the reference antenna is a runtime index: LDS, not registers, so
//            nothing goes to scratch), forms v and the stats once, and leaves them in LDS and, lane 0, in global memory
//   pass 2   every wave reads its own tiles again (from L2 / the Infinity Cache: at most 8 x 36 KB per slot) and stores y
// No atomics; weights and stats are plain vector stores.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wifirx.h"
#include "wr_precombine.h"

namespace wr {

namespace {

#define PRE_WAVES 4

__device__ __forceinline__ float pre_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
// correctly rounded, as the rule asks: the builtin root and the plain division (hipcc's default for float32; the __fsqrt_rn /
// __fdiv_rn spellings are the native approximations unless the rounded OCML operations are switched on)
__device__ __forceinline__ float pre_sqrt(float a) { return __builtin_sqrtf(a); }
__device__ __forceinline__ float pre_div(float a, float b) { return a / b; }

// index of the pair a <= b in the row-major upper triangle of an NA x NA matrix
__device__ __forceinline__ constexpr int pre_tri(int na, int a, int b) { return a * na - a * (a - 1) / 2 + (b - a); }

// rule 33's fold of the 64 lanes: lane xor 32, 16, 8, 4, 2, 1 (irs_butterfly's order, one component); every lane ends with the sum
__device__ __forceinline__ float pre_butterfly(float v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = v + __shfl_xor(v, m);
    return v;
}

// v = u / sqrt(sum |u_a|^2): an ascending fma chain (re then im per antenna), correctly rounded root and divisions.
// false: the norm is not finite or not > 0 (v is then not to be used)
template <int NA>
__device__ __forceinline__ bool pre_normalise(const float2 (&u)[NA], float2 (&v)[NA])
{
    float s = 0.0f;
#pragma unroll
    for (int a = 0; a < NA; a++) { s = pre_fma(u[a].x, u[a].x, s); s = pre_fma(u[a].y, u[a].y, s); }
    const float n = pre_sqrt(s);
#pragma unroll
    for (int a = 0; a < NA; a++) v[a] = make_float2(pre_div(u[a].x, n), pre_div(u[a].y, n));
    return __builtin_isfinite(n) && n > 0.0f;
}

// u = R v: per row an ascending chain over b from +0, each step rule 2's x (c + js) continued into the accumulator
template <int NA>
__device__ __forceinline__ void pre_matvec(const float2* R, const float2 (&v)[NA], float2 (&u)[NA])
{
#pragma unroll
    for (int a = 0; a < NA; a++) {
        float re = 0.0f, im = 0.0f;
#pragma unroll
        for (int b = 0; b < NA; b++) {
            const float2 x = R[a * NA + b];
            re = pre_fma(-x.y, v[b].y, pre_fma(x.x, v[b].x, re));
            im = pre_fma(x.y, v[b].x, pre_fma(x.x, v[b].y, im));
        }
        u[a] = make_float2(re, im);
    }
}

}  // namespace

template <int NA>
__global__ __launch_bounds__(256)
void precombine_kernel(const PreArgs a)
{
    constexpr int NP = NA * (NA + 1) / 2;
    __shared__ float  s_part[PRE_WAVES][2 * NP];     // the waves' folded sums: re of pair p at [p], im at [NP + p]
    __shared__ float2 s_R[NA * NA];
    __shared__ float2 s_v[NA];
    __shared__ uint32_t s_copy;                      // 1: a degenerate slot, y = x_0

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t slot = blockIdx.x;
    const uint32_t tiles = a.slot_len >> 6;
    const size_t base = (size_t)slot * a.slot_len + lane;
    const float2* x[NA];
#pragma unroll
    for (int k = 0; k < NA; k++) x[k] = a.x[k] + base;
    float2* out = a.out + base;

    if constexpr (NA == 1) {                         // y = x_0 bit for bit, v = (1, 0), no sums
        for (uint32_t t = wave; t < tiles; t += PRE_WAVES) out[(size_t)t * 64] = x[0][(size_t)t * 64];
        if (threadIdx.x == 0) {
            if (a.weights) a.weights[slot] = make_float2(1.0f, 0.0f);
            if (a.stats) { a.stats[2 * (size_t)slot] = make_uint2(0u, 0u); a.stats[2 * (size_t)slot + 1] = make_uint2(0u, 0u); }
        }
        return;
    } else {
        // ---- pass 1: the chain (wave, lane) of every pair, ascending in t ----
        float cr[NP], ci[NP];
#pragma unroll
        for (int p = 0; p < NP; p++) { cr[p] = 0.0f; ci[p] = 0.0f; }
#pragma unroll 2
        for (uint32_t t = wave; t < tiles; t += PRE_WAVES) {
            float2 s[NA];
#pragma unroll
            for (int k = 0; k < NA; k++) s[k] = x[k][(size_t)t * 64];
#pragma unroll
            for (int i = 0; i < NA; i++) {
#pragma unroll
                for (int j = i; j < NA; j++) {
                    const int p = pre_tri(NA, i, j);
                    if (i == j) {
                        cr[p] = pre_fma(s[i].y, s[i].y, pre_fma(s[i].x, s[i].x, cr[p]));
                    } else {                         // x_i conj(x_j), rule 2's first form with (c, s) = (Re, -Im) of x_j
                        cr[p] = pre_fma(s[i].y, s[j].y, pre_fma(s[i].x, s[j].x, cr[p]));
                        ci[p] = pre_fma(s[i].y, s[j].x, pre_fma(s[i].x, -s[j].y, ci[p]));
                    }
                }
            }
        }
#pragma unroll
        for (int i = 0; i < NA; i++) {
#pragma unroll
            for (int j = i; j < NA; j++) {
                const int p = pre_tri(NA, i, j);
                const float fr = pre_butterfly(cr[p]);
                const float fi = i == j ? 0.0f : pre_butterfly(ci[p]);
                if (lane == 0) { s_part[wave][p] = fr; s_part[wave][NP + p] = fi; }
            }
        }
        __syncthreads();
        if (threadIdx.x < NA * NA) {                 // the four waves: (w0 + w1) + (w2 + w3); R_ba = conj(R_ab)
            const int i = threadIdx.x / NA, j = threadIdx.x % NA;
            const int lo = i < j ? i : j, hi = i < j ? j : i;
            const int p = pre_tri(NA, lo, hi);
            const float re = (s_part[0][p] + s_part[1][p]) + (s_part[2][p] + s_part[3][p]);
            const float im = (s_part[0][NP + p] + s_part[1][NP + p]) + (s_part[2][NP + p] + s_part[3][NP + p]);
            s_R[threadIdx.x] = make_float2(re, i == j ? 0.0f : (i < j ? im : -im));
        }
        __syncthreads();

        // ---- the slot's algebra, once (wave 0; every value is the same in all its lanes) ----
        if (wave == 0) {
            float trace = s_R[0].x, top = s_R[0].x;
            uint32_t r = 0;
#pragma unroll
            for (int k = 1; k < NA; k++) {
                const float d = s_R[k * NA + k].x;
                trace = trace + d;
                if (d > top) { top = d; r = (uint32_t)k; }       // ties keep the lower index; a NaN neither replaces nor is replaced
            }
            bool ok = __builtin_isfinite(trace) && trace > 0.0f;
            float2 v[NA], u[NA];
            float lambda = 0.0f;
            if (ok) {
#pragma unroll
                for (int k = 0; k < NA; k++) u[k] = s_R[k * NA + r];
                ok = pre_normalise<NA>(u, v);
                for (uint32_t it = 0; ok && it < a.iters; it++) {
                    pre_matvec<NA>(s_R, v, u);
                    ok = pre_normalise<NA>(u, v);
                }
            }
            if (ok) {                                // rotate: v_r real and non-negative
                float2 vr = v[0];
#pragma unroll
                for (int k = 1; k < NA; k++) vr = (uint32_t)k == r ? v[k] : vr;
                const float m = pre_sqrt(pre_fma(vr.y, vr.y, vr.x * vr.x));
                ok = __builtin_isfinite(m) && m > 0.0f;
                const float c = pre_div(vr.x, m), s = pre_div(-vr.y, m);
#pragma unroll
                for (int k = 0; k < NA; k++) {
                    const float2 w = v[k];
                    v[k] = (uint32_t)k == r ? make_float2(m, 0.0f)
                                            : make_float2(pre_fma(-w.y, s, w.x * c), pre_fma(w.y, c, w.x * s));
                }
            }
            if (ok) {                                // lambda = Re(v^H R v)
                pre_matvec<NA>(s_R, v, u);
#pragma unroll
                for (int k = 0; k < NA; k++) { lambda = pre_fma(v[k].x, u[k].x, lambda); lambda = pre_fma(v[k].y, u[k].y, lambda); }
            } else {
#pragma unroll
                for (int k = 0; k < NA; k++) v[k] = make_float2(k == 0 ? 1.0f : 0.0f, 0.0f);
                r = 0;
            }
            if (lane == 0) {
                s_copy = ok ? 0u : 1u;
#pragma unroll
                for (int k = 0; k < NA; k++) s_v[k] = v[k];
                if (a.weights) {
#pragma unroll
                    for (int k = 0; k < NA; k++) a.weights[(size_t)slot * NA + k] = v[k];
                }
                if (a.stats) {                       // two 8-byte stores: the row is only 8-byte aligned
                    a.stats[2 * (size_t)slot] = make_uint2(__float_as_uint(lambda), __float_as_uint(trace));
                    a.stats[2 * (size_t)slot + 1] = make_uint2(r, ok ? 0u : (uint32_t)WIFIRX_PRE_DEGENERATE);
                }
            }
        }
        __syncthreads();

        // ---- pass 2: y = conj(v_0) x_0 by rule 2's second form, then one fma pair per further antenna ----
        if (s_copy) {
            for (uint32_t t = wave; t < tiles; t += PRE_WAVES) out[(size_t)t * 64] = x[0][(size_t)t * 64];
            return;
        }
        float2 v[NA];
#pragma unroll
        for (int k = 0; k < NA; k++) v[k] = s_v[k];
#pragma unroll 2
        for (uint32_t t = wave; t < tiles; t += PRE_WAVES) {
            float2 s[NA];
#pragma unroll
            for (int k = 0; k < NA; k++) s[k] = x[k][(size_t)t * 64];
            float re = pre_fma(v[0].y, s[0].y, v[0].x * s[0].x);
            float im = pre_fma(-v[0].y, s[0].x, v[0].x * s[0].y);
#pragma unroll
            for (int k = 1; k < NA; k++) {
                re = pre_fma(v[k].y, s[k].y, pre_fma(v[k].x, s[k].x, re));
                im = pre_fma(-v[k].y, s[k].x, pre_fma(v[k].x, s[k].y, im));
            }
            out[(size_t)t * 64] = make_float2(re, im);
        }
    }
}

}  // namespace wr

extern "C" hipError_t wr_launch_precombine(hipStream_t st, const wr::PreArgs* args)
{
    if (args->n_slots == 0) return hipSuccess;
    if (args->n_ant < 1 || args->n_ant > WR_PRE_MAX_ANT || args->iters > WR_PRE_MAX_ITERS) return hipErrorInvalidValue;
    if (args->slot_len < 64 || (args->slot_len & 63)) return hipErrorInvalidValue;
    const dim3 grid(args->n_slots), block(64 * PRE_WAVES);
    switch (args->n_ant) {
    case 1: hipLaunchKernelGGL(wr::precombine_kernel<1>, grid, block, 0, st, *args); break;
    case 2: hipLaunchKernelGGL(wr::precombine_kernel<2>, grid, block, 0, st, *args); break;
    case 3: hipLaunchKernelGGL(wr::precombine_kernel<3>, grid, block, 0, st, *args); break;
    case 4: hipLaunchKernelGGL(wr::precombine_kernel<4>, grid, block, 0, st, *args); break;
    case 5: hipLaunchKernelGGL(wr::precombine_kernel<5>, grid, block, 0, st, *args); break;
    case 6: hipLaunchKernelGGL(wr::precombine_kernel<6>, grid, block, 0, st, *args); break;
    case 7: hipLaunchKernelGGL(wr::precombine_kernel<7>, grid, block, 0, st, *args); break;
    default: hipLaunchKernelGGL(wr::precombine_kernel<8>, grid, block, 0, st, *args); break;
    }
    return hipGetLastError();
}
