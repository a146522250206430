// wr_irs_elem.h -- the elements and the direct path of the reflecting surface (NUMERICS.md rule 25), one text for the two kernels
// that draw them: wr_irs.hip (wifirx_irs_taps) and wr_irs_sweep.hip (wifirx_irs_sweep, rule 26).  The same seed gives both the
// same element bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wr_rng.h"        // philox4x32_10, ch_noise
#include "wr_channel.h"    // ch_mul, ch_add
#include "wr_irs.h"

namespace wr {

#define IRS_MAX_ELEMS 4096
#define IRS_MAX_TAPS  16
#define IRS_DIRECT    0xFFFFFFFFu      // counter word 0 of the direct path's draw (an element has n < 4096)

// the Rician mix of one coefficient: a_los * los + a_nlos * w per part; k_factor = 0: w itself
__device__ __forceinline__ float2 irs_mix(const IrsArgs& a, float2 los, float2 w)
{
    if (a.a_los == 0.0f) return w;
    return make_float2(a.a_los * los.x + a.a_nlos * w.x, a.a_los * los.y + a.a_nlos * w.y);
}

// row of `scatter` that the pair (r, l) reads
__device__ __forceinline__ const float2* irs_row(const IrsArgs& a, uint32_t r, uint32_t l)
{
    return a.scatter + (((uint64_t)r * a.n_taps + l) % a.n_scatter) * (2ull * a.n_elems + 1);
}

struct IrsElem { float2 a, b; };

// element n of tap l of set r: the two legs after the mix
__device__ __forceinline__ IrsElem irs_elem(const IrsArgs& a, uint32_t r, uint32_t l, uint32_t n, uint2 key)
{
    float2 wa, wb;
    if (a.scatter) {
        const float2* row = irs_row(a, r, l);
        wa = row[n];
        wb = row[a.n_elems + n];
    } else {
        const uint4 d = philox4x32_10(make_uint4(n, r, l, 2u), key);
        wa = ch_noise(d.x, d.y, 0.70710678118654752f);
        wb = ch_noise(d.z, d.w, 0.70710678118654752f);
    }
    const bool los = a.a_los != 0.0f;
    const float2 zero = make_float2(0.0f, 0.0f);
    return {irs_mix(a, los ? a.los_a[n] : zero, wa), irs_mix(a, los ? a.los_b[n] : zero, wb)};
}

// the direct path of tap l of set r (the same value in every lane)
__device__ __forceinline__ float2 irs_direct(const IrsArgs& a, uint32_t r, uint32_t l, uint2 key)
{
    if (a.direct_gain == 0.0f) return make_float2(0.0f, 0.0f);
    float2 w;
    if (a.scatter) {
        w = irs_row(a, r, l)[2 * a.n_elems];
    } else {
        const uint4 d = philox4x32_10(make_uint4(IRS_DIRECT, r, l, 2u), key);
        w = ch_noise(d.x, d.y, 0.70710678118654752f);
    }
    const float2 v = irs_mix(a, a.los_d, w);
    return make_float2(a.direct_gain * v.x, a.direct_gain * v.y);
}

// rule 25's argmax: the code c of n_codes that maximises Re(g C_{c << up}), `phase` the table of the C_k.  Ascending c and a strict
// `>`: the lowest c wins a tie, and a NaN never replaces the running maximum.  One text for wr_irs.hip and wr_irs_optimize.hip
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
