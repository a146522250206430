// wr_irs_multi_elem.h -- the elements and the direct path of the surface behind an AP of M antennas (NUMERICS.md rule 27), one
// text for the kernels that draw them: wr_irs_multi.hip (wifirx_irs_taps_multi, wifirx_irs_sweep_multi) and wr_irs_estimate.hip
// (wifirx_irs_estimate, rule 29).  The same seed gives all of them the same element bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wr_irs_elem.h"   // irs_mix, IrsElem, IRS_MAX_*, IRS_DIRECT
#include "wr_irs_multi.h"

namespace wr {

#define IRSM_MAX_ANT  8

// C_k = exp(j 2 pi k / 8); code c of a B-bit surface is C_{c << (3 - B)} (wr_irs.hip's table)
static __device__ const float2 irs_multi_phase[8] = {
    {1.0f, 0.0f}, {0.70710678118654752f, 0.70710678118654752f}, {0.0f, 1.0f}, {-0.70710678118654752f, 0.70710678118654752f},
    {-1.0f, 0.0f}, {-0.70710678118654752f, -0.70710678118654752f}, {0.0f, -1.0f}, {0.70710678118654752f, -0.70710678118654752f}};

// row of `scatter` that the pair (r, l) reads: (M + 1) N + M values
__device__ __forceinline__ const float2* irsm_row(const IrsMultiArgs& a, uint32_t r, uint32_t l)
{
    return a.s.scatter + (((uint64_t)r * a.s.n_taps + l) % a.s.n_scatter) * ((uint64_t)(a.n_ant + 1) * a.s.n_elems + a.n_ant);
}

// counter word 2 of antenna m's draws: l for antenna 0, l + 16 ((m + 1) >> 1) for the others (l < 16: never rule 25's)
__device__ __forceinline__ uint32_t irsm_ctr(uint32_t l, uint32_t m) { return l + 16u * ((m + 1) >> 1); }

// antenna m's Gaussian of its draw: words (x, y) for antenna 0 and the odd antennas, (z, w) for the even ones
__device__ __forceinline__ float2 irsm_pick(uint4 d, uint32_t m)
{
    const bool xy = m == 0 || (m & 1);
    return ch_noise(xy ? d.x : d.z, xy ? d.y : d.w, 0.70710678118654752f);
}

// irs_mix with the line-of-sight coefficient read only where it is applied (k_factor = 0: w itself, nothing read)
__device__ __forceinline__ float2 irsm_mix(const IrsArgs& s, const float2* los, uint64_t at, float2 w)
{
    if (s.a_los == 0.0f) return w;
    return irs_mix(s, los[at], w);
}

// the direct path of antenna m, tap l, set r (the same value in every lane)
__device__ __forceinline__ float2 irsm_direct(const IrsMultiArgs& a, uint32_t m, uint32_t r, uint32_t l, uint2 key)
{
    if (a.s.direct_gain == 0.0f) return make_float2(0.0f, 0.0f);
    float2 w;
    if (a.s.scatter) {
        w = irsm_row(a, r, l)[(uint64_t)(a.n_ant + 1) * a.s.n_elems + m];
    } else {
        w = irsm_pick(philox4x32_10(make_uint4(IRS_DIRECT, r, irsm_ctr(l, m), 2u), key), m);
    }
    const float2 v = irsm_mix(a.s, a.los_d, m, w);
    return make_float2(a.s.direct_gain * v.x, a.s.direct_gain * v.y);
}

// element n of antenna m, tap l, set r: (a_{m,n}, b_n).  The sweep's rows use it; irs_multi_kernel shares b_n and the draws
// among the antennas instead
__device__ __forceinline__ IrsElem irsm_elem(const IrsMultiArgs& a, uint32_t m, uint32_t r, uint32_t l, uint32_t n, uint2 key)
{
    const uint32_t N = a.s.n_elems;
    float2 wa, wb;
    if (a.s.scatter) {
        const float2* row = irsm_row(a, r, l);
        wa = row[(uint64_t)m * N + n];
        wb = row[(uint64_t)a.n_ant * N + n];
    } else {
        const uint4 d = philox4x32_10(make_uint4(n, r, l, 2u), key);
        wb = ch_noise(d.z, d.w, 0.70710678118654752f);
        uint32_t u0 = d.x, u1 = d.y;
        if (m != 0) {
            const uint4 dm = philox4x32_10(make_uint4(n, r, irsm_ctr(l, m), 2u), key);
            u0 = (m & 1) ? dm.x : dm.z;
            u1 = (m & 1) ? dm.y : dm.w;
        }
        wa = ch_noise(u0, u1, 0.70710678118654752f);
    }
    return {irsm_mix(a.s, a.s.los_a, (uint64_t)m * N + n, wa), irsm_mix(a.s, a.s.los_b, n, wb)};
}

}  // namespace wr
