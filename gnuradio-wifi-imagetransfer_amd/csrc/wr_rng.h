// wr_rng.h -- the counter-based generator of the device channels (wr_synth.hip, wr_channel.hip): Philox4x32-10 and the
// uniform on (0, 1) and the Box-Muller transform that draws from it (also wr_irs.hip).  Outputs depend only on (counter, key).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace wr {

__device__ __forceinline__ uint4 philox4x32_10(uint4 c, uint2 k)
{
    const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
    for (int r = 0; r < 10; r++) {
        uint32_t hi0 = __umulhi(M0, c.x), lo0 = M0 * c.x;
        uint32_t hi1 = __umulhi(M1, c.z), lo1 = M1 * c.z;
        c = make_uint4(hi1 ^ c.y ^ k.x, lo1, hi0 ^ c.w ^ k.y, lo0);
        k.x += W0;
        k.y += W1;
    }
    return c;
}

__device__ __forceinline__ float u01(uint32_t x) { return ((float)x + 0.5f) * 2.3283064365386963e-10f; }

// one Box-Muller sample of wr_synth.hip: radius from ua, angle from ub, each component h * r * (cos | sin)
__device__ __forceinline__ float2 ch_noise(uint32_t ua, uint32_t ub, float h)
{
    const float r = sqrtf(-2.0f * logf(u01(ua)));
    float s, c;
    sincosf(6.283185307179586f * u01(ub), &s, &c);
    return make_float2(h * r * c, h * r * s);
}

}  // namespace wr
