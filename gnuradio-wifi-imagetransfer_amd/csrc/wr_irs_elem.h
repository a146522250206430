// wr_irs_elem.h -- the elements and the direct path of the reflecting surface behind an AP of M = 1..8 antennas (NUMERICS.md rules
// 25 and 27), one text for every kernel that draws them: wr_irs.hip (wifirx_irs_taps, wifirx_irs_taps_multi), wr_irs_sweep.hip
// (wifirx_irs_sweep, wifirx_irs_sweep_multi; rules 26 and 28) and wr_irs_estimate.hip (wifirx_irs_estimate, rule 29).  The same
// seed gives all of them the same element bits, and antenna 0 has the one-antenna surface's counters.  Also here: the phase table,
// the argmax and the butterfly that wr_irs_optimize.hip shares with them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wr_rng.h"        // philox4x32_10, ch_noise
#include "wr_channel.h"    // ch_mul, ch_add
#include "wr_irs.h"

namespace wr {

#define IRS_MAX_ELEMS 4096
#define IRS_MAX_TAPS  16
#define IRSM_MAX_ANT  8
#define IRS_DIRECT    0xFFFFFFFFu      // counter word 0 of the direct path's draw (an element has n < 4096)

// C_k = exp(j 2 pi k / 8); code c of a B-bit surface is C_{c << (3 - B)}
static __device__ const float2 irs_phase[8] = {
    {1.0f, 0.0f}, {0.70710678118654752f, 0.70710678118654752f}, {0.0f, 1.0f}, {-0.70710678118654752f, 0.70710678118654752f},
    {-1.0f, 0.0f}, {-0.70710678118654752f, -0.70710678118654752f}, {0.0f, -1.0f}, {0.70710678118654752f, -0.70710678118654752f}};

// the line-of-sight coefficient los[at], read only where it is applied (k_factor = 0: nothing is read)
__device__ __forceinline__ float2 irs_los(const IrsArgs& a, const float2* los, uint64_t at)
{
    return a.a_los == 0.0f ? make_float2(0.0f, 0.0f) : los[at];
}

// the Rician mix of one coefficient: a_los * los + a_nlos * w per part; k_factor = 0: w itself
__device__ __forceinline__ float2 irs_mix(const IrsArgs& a, float2 los, float2 w)
{
    if (a.a_los == 0.0f) return w;
    return make_float2(a.a_los * los.x + a.a_nlos * w.x, a.a_los * los.y + a.a_nlos * w.y);
}

// row of `scatter` that the pair (r, l) reads: (M + 1) N + M values
__device__ __forceinline__ const float2* irs_row(const IrsArgs& a, uint32_t r, uint32_t l)
{
    return a.scatter + (((uint64_t)r * a.n_taps + l) % a.n_scatter) * ((uint64_t)(a.n_ant + 1) * a.n_elems + a.n_ant);
}

// counter word 2 of antenna m's draws: l for antenna 0, l + 16 ((m + 1) >> 1) for the others (l < 16: never antenna 0's)
__device__ __forceinline__ uint32_t irs_ctr(uint32_t l, uint32_t m) { return l + 16u * ((m + 1) >> 1); }

// antenna m's Gaussian of its draw: words (x, y) for antenna 0 and the odd antennas, (z, w) for the even ones
__device__ __forceinline__ float2 irs_pick(uint4 d, uint32_t m)
{
    const bool xy = m == 0 || (m & 1);
    return ch_noise(xy ? d.x : d.z, xy ? d.y : d.w, 0.70710678118654752f);
}

struct IrsElem { float2 a, b; };

// element n of antenna m, tap l, set r: the two legs (a_{m,n}, b_n) after the mix.  The rows of the sweep and of the estimator
// use it; irs_kernel shares b_n and the draws among the antennas instead
__device__ __forceinline__ IrsElem irs_elem(const IrsArgs& a, uint32_t m, uint32_t r, uint32_t l, uint32_t n, uint2 key)
{
    const uint32_t N = a.n_elems;
    float2 wa, wb;
    if (a.scatter) {
        const float2* row = irs_row(a, r, l);
        wa = row[(uint64_t)m * N + n];
        wb = row[(uint64_t)a.n_ant * N + n];
    } else {
        const uint4 d = philox4x32_10(make_uint4(n, r, l, 2u), key);
        wb = ch_noise(d.z, d.w, 0.70710678118654752f);
        uint32_t u0 = d.x, u1 = d.y;
        if (m != 0) {
            const uint4 dm = philox4x32_10(make_uint4(n, r, irs_ctr(l, m), 2u), key);
            u0 = (m & 1) ? dm.x : dm.z;
            u1 = (m & 1) ? dm.y : dm.w;
        }
        wa = ch_noise(u0, u1, 0.70710678118654752f);
    }
    return {irs_mix(a, irs_los(a, a.los_a, (uint64_t)m * N + n), wa), irs_mix(a, irs_los(a, a.los_b, n), wb)};
}

// the direct path of antenna m, tap l, set r (the same value in every lane)
__device__ __forceinline__ float2 irs_direct(const IrsArgs& a, uint32_t m, uint32_t r, uint32_t l, uint2 key)
{
    if (a.direct_gain == 0.0f) return make_float2(0.0f, 0.0f);
    float2 w;
    if (a.scatter) {
        w = irs_row(a, r, l)[(uint64_t)(a.n_ant + 1) * a.n_elems + m];
    } else {
        w = irs_pick(philox4x32_10(make_uint4(IRS_DIRECT, r, irs_ctr(l, m), 2u), key), m);
    }
    const float2 v = irs_mix(a, irs_los(a, a.los_d, m), w);
    return make_float2(a.direct_gain * v.x, a.direct_gain * v.y);
}

// rule 25's argmax: the code c of n_codes that maximises Re(g C_{c << up}), `phase` the table of the C_k.  Ascending c and a strict
// `>`: the lowest c wins a tie, and a NaN never replaces the running maximum
__device__ __forceinline__ uint32_t irs_argmax(float2 g, const float2* phase, uint32_t n_codes, uint32_t up)
{
    uint32_t best = 0;
    float top = ch_mul(g, phase[0]).x;
    for (uint32_t c = 1; c < n_codes; c++) {
        const float m = ch_mul(g, phase[c << up]).x;
        if (m > top) { top = m; best = c; }            // the lowest c wins a tie
    }
    return best;
}

// rule 25's fold of the 64 lanes' partial sums: lane xor 32, 16, 8, 4, 2, 1, each part apart (no LDS, no barrier).  Symmetric:
// every lane ends with the same bits
__device__ __forceinline__ float2 irs_butterfly(float2 acc)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const float ox = __shfl_xor(acc.x, m), oy = __shfl_xor(acc.y, m);
        acc = make_float2(acc.x + ox, acc.y + oy);
    }
    return acc;
}

}  // namespace wr
