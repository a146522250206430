// wr_irs.hip -- the cascade channel of an intelligent reflecting surface on the device (the model of the reference's
// utils/SV_channel.py and utils/channel.py, H = H_B2R diag(psi) H_R2U + H_B2U, for one AP antenna and one user), in the
// float32 arithmetic of NUMERICS.md rule 25: per tap set r and tap l the Rician mix of N element pairs and of the direct
// path, the surface's phases (given, or aligned per draw to B bits), the sum over the surface and the tap's scale.
//
// Work split: one workgroup of four waves owns one tap set; its waves walk the set's taps (wave w: l = w, w + 4, ...).
// Lane i of the wave that owns tap l forms the elements n = i, i + 64, ... in ascending n and sums their products; the 64
// partial sums are folded by a __shfl_xor butterfly (no LDS, no barrier), so every lane holds the sum, and lane 0 stores the
// tap.  The generator is compute-bound (a Philox draw and two Box-Mullers per element against 8 bytes out per N elements).
//   aligned mode   the codes are decided on tap 0 and serve every tap of the set: the workgroup's 256 lanes form tap 0's
//                  elements once, lane t the elements t, t + 256, ..., and leave the codes in LDS (N bytes) behind the kernel's
//                  one barrier.  The other choice, every wave forming tap 0 again beside its own tap, doubles the Philox work
//                  of every tap; this one adds 1 / L of it (the wave that owns tap 0 forms those elements a second time).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wr_irs_elem.h"   // irs_elem, irs_direct, irs_mix: shared with wr_irs_sweep.hip; irs_argmax, irs_butterfly: with wr_irs_optimize.hip

namespace wr {

#define IRS_WAVES     4

// C_k = exp(j 2 pi k / 8); code c of a B-bit surface is C_{c << (3 - B)}
__device__ const float2 irs_phase[8] = {
    {1.0f, 0.0f}, {0.70710678118654752f, 0.70710678118654752f}, {0.0f, 1.0f}, {-0.70710678118654752f, 0.70710678118654752f},
    {-1.0f, 0.0f}, {-0.70710678118654752f, -0.70710678118654752f}, {0.0f, -1.0f}, {0.70710678118654752f, -0.70710678118654752f}};

// ALIGN: the phases are the B-bit codes decided on tap 0 (rule 25, genie bound), not a.psi
template <bool ALIGN>
__global__ __launch_bounds__(64 * IRS_WAVES)
void irs_kernel(const IrsArgs a)
{
    __shared__ uint8_t codes[ALIGN ? IRS_MAX_ELEMS : 1];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t r = blockIdx.x, N = a.n_elems, L = a.n_taps;
    const uint2 key = make_uint2((uint32_t)a.seed, (uint32_t)(a.seed >> 32));
    const uint32_t up = 3 - a.align_bits;               // ALIGN: code c is irs_phase[c << up]

    if constexpr (ALIGN) {
        const float2 hd = irs_direct(a, r, 0, key);
        const bool axis = hd.x == 0.0f && hd.y == 0.0f;     // no direct path to align to: the positive real axis
        const float2 hc = make_float2(hd.x, -hd.y);
        const uint32_t n_codes = 1u << a.align_bits;
        for (uint32_t n = tid; n < N; n += 64 * IRS_WAVES) {
            const IrsElem e = irs_elem(a, r, 0, n, key);
            float2 g = ch_mul(e.a, e.b);
            if (!axis) g = ch_mul(hc, g);
            const uint32_t best = irs_argmax(g, irs_phase, n_codes, up);
            codes[n] = (uint8_t)best;
            if (a.codes_out) a.codes_out[(uint64_t)r * N + n] = (uint8_t)best;
        }
        __syncthreads();
    }

    const float2* psi = ALIGN ? nullptr : a.psi + (uint64_t)(r % a.n_psi_sets) * N;
    for (uint32_t l = wave; l < L; l += IRS_WAVES) {
        float2 acc = make_float2(0.0f, 0.0f);               // a lane without an element holds +0
        float2* eo = a.elems_out ? a.elems_out + ((uint64_t)r * L + l) * 2ull * N : nullptr;
        for (uint32_t n = lane; n < N; n += 64) {
            const IrsElem e = irs_elem(a, r, l, n, key);
            if (eo) {
                eo[n] = e.a;
                eo[N + n] = e.b;
            }
            float2 ph;
            if constexpr (ALIGN) ph = irs_phase[(uint32_t)codes[n] << up];
            else ph = psi[n];
            const float2 p = ch_mul(ch_mul(e.a, ph), e.b);
            acc = n == lane ? p : ch_add(acc, p);           // ascending n, from the lane's first product
        }
        acc = irs_butterfly(acc);                           // symmetric: every lane ends with the same bits
        const float2 h = ch_add(irs_direct(a, r, l, key), acc);
        const float s = a.scale[l];
        if (lane == 0) a.taps_out[(uint64_t)r * L + l] = make_float2(h.x * s, h.y * s);
    }
}

}  // namespace wr

extern "C" hipError_t wr_launch_irs(hipStream_t st, const wr::IrsArgs* args)
{
    if (args->n_sets == 0) return hipSuccess;
    if (args->n_elems < 1 || args->n_elems > IRS_MAX_ELEMS || args->n_taps < 1 || args->n_taps > IRS_MAX_TAPS ||
        args->align_bits > 3 || args->n_sets > 0x7fffffffu)
        return hipErrorInvalidValue;                        // (the entry point refuses these first)
    const dim3 grid(args->n_sets), block(64 * IRS_WAVES);
    if (args->align_bits) hipLaunchKernelGGL((wr::irs_kernel<true>), grid, block, 0, st, *args);
    else hipLaunchKernelGGL((wr::irs_kernel<false>), grid, block, 0, st, *args);
    return hipGetLastError();
}

extern "C" uint32_t wr_irs_max_elems(void) { return IRS_MAX_ELEMS; }
extern "C" uint32_t wr_irs_max_taps(void) { return IRS_MAX_TAPS; }
