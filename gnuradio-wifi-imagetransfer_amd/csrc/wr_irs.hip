// wr_irs.hip -- the cascade channel of an intelligent reflecting surface on the device (the model of the reference's
// utils/SV_channel.py and utils/channel.py, H = H_B2R diag(psi) H_R2U + H_B2U, for an AP of M = 1..8 antennas and one user: the
// reference's Saleh_Valenzuela_Channel with antennaNum = M, H_B2R [M, N], H_B2U [M], one surface-to-user leg H_R2U shared by
// every antenna), in the float32 arithmetic of NUMERICS.md rules 25 (M = 1) and 27: per tap set r and tap l the Rician mix of N
// element pairs and of the direct path, the surface's phases (given, or aligned per draw to B bits), the sum over the surface
// and the tap's scale.  Antenna 0 is rule 25 bit for bit: the same counters, the same operations in the same order
// (wr_irs_elem.h's irs_mix, wr_rng.h's ch_noise, wr_channel.h's ch_mul / ch_add).
//
// Work split: one workgroup of four waves owns one tap set; its waves walk the set's taps (wave w: l = w, w + 4, ...).
// Lane i of the wave that owns tap l forms b_n ONCE for its elements n = i, i + 64, ... in ascending n, then a_{m,n} for the M
// antennas (one Philox draw serves the antennas 2 j - 1 and 2 j, so an element costs 1 + ceil((M - 1) / 2) draws, not M), and
// keeps M partial sums of the products in registers: the antenna loop is unrolled to MA (1, or 8 with a wave-uniform guard), so
// every accumulator has a name at compile time and nothing goes to scratch.  The 64 partial sums of an antenna are folded by a
// __shfl_xor butterfly (no LDS, no barrier), so every lane holds the sum, and lane 0 stores the tap.  The generator is
// compute-bound (a Philox draw and two Box-Mullers per element against 8 bytes out per N elements).
//   aligned mode   the codes are decided on antenna 0, tap 0 and serve every tap and antenna of the set: the workgroup's 256
//                  lanes form tap 0's elements once, lane t the elements t, t + 256, ..., and leave the codes in LDS (N bytes)
//                  behind the kernel's one barrier.  The other choice, every wave forming tap 0 again beside its own tap, doubles
//                  the Philox work of every tap; this one adds 1 / L of it (the wave that owns tap 0 forms those elements a second time).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <utility>

#include "wr_irs_elem.h"

namespace wr {

#define IRS_WAVES     4

// f(m) for the antennas m = 0 .. MA - 1 with m a compile-time constant: straight-line code from the front end on.  For a tap's
// tail: as a loop that the optimiser unrolls, the direct path's Box-Muller loses the branch around sincosf's large-argument path
// and runs it for every tap, which cost the MA = 1 instance a fifth of its time at 64 elements
template <class F, int... I>
__device__ __forceinline__ void irs_each_antenna(std::integer_sequence<int, I...>, F&& f)
{
    (f(std::integral_constant<int, I>{}), ...);
}

// ALIGN: the phases are the B-bit codes decided on antenna 0, tap 0 (rules 25 and 27, the genie of the reference antenna), not
// a.psi.  MA: the bound of the unrolled antenna loop, 1 (one antenna, one accumulator, no guard) or IRSM_MAX_ANT
template <bool ALIGN, int MA>
__global__ __launch_bounds__(64 * IRS_WAVES)
void irs_kernel(const IrsArgs a)
{
    __shared__ uint8_t codes[ALIGN ? IRS_MAX_ELEMS : 1];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t r = blockIdx.x, N = a.n_elems, L = a.n_taps, M = MA == 1 ? 1u : a.n_ant;
    const uint2 key = make_uint2((uint32_t)a.seed, (uint32_t)(a.seed >> 32));
    const uint32_t up = 3 - a.align_bits;               // ALIGN: code c is irs_phase[c << up]
    const float2 zero = make_float2(0.0f, 0.0f);

    if constexpr (ALIGN) {
        const float2 hd = irs_direct(a, 0, r, 0, key);
        const bool axis = hd.x == 0.0f && hd.y == 0.0f;     // no direct path to align to: the positive real axis
        const float2 hc = make_float2(hd.x, -hd.y);
        const uint32_t n_codes = 1u << a.align_bits;
        for (uint32_t n = tid; n < N; n += 64 * IRS_WAVES) {
            const IrsElem e = irs_elem(a, 0, r, 0, n, key);
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
        float2 acc[MA];
#pragma unroll
        for (int m = 0; m < MA; m++) acc[m] = zero;             // a lane without an element holds +0
        float2* eo = a.elems_out ? a.elems_out + ((uint64_t)r * L + l) * (uint64_t)(M + 1) * N : nullptr;
        const float2* row = a.scatter ? irs_row(a, r, l) : nullptr;
        for (uint32_t n = lane; n < N; n += 64) {
            const IrsElem e0 = irs_elem(a, 0, r, l, n, key);    // a_{0,n} and b_n: one draw serves both
            const float2 b = e0.b;
            if (eo) eo[(uint64_t)M * N + n] = b;
            float2 ph;
            if constexpr (ALIGN) ph = irs_phase[(uint32_t)codes[n] << up];
            else ph = psi[n];
            uint4 d = make_uint4(0, 0, 0, 0);
#pragma unroll
            for (int m = 0; m < MA; m++) {                      // (as a loop: the fold below costs the MA = 8 instance a wave here)
                if (MA == 1 || (uint32_t)m < M) {               // the same in every lane
                    float2 am = e0.a;
                    if (m > 0) {
                        float2 wa;
                        if (row) {
                            wa = row[(uint64_t)m * N + n];
                        } else {
                            if (m & 1) d = philox4x32_10(make_uint4(n, r, irs_ctr(l, m), 2u), key);    // serves m and m + 1
                            wa = irs_pick(d, m);
                        }
                        am = irs_mix(a, irs_los(a, a.los_a, (uint64_t)m * N + n), wa);   // (read here: 7 early loads cost a wave)
                    }
                    if (eo) eo[(uint64_t)m * N + n] = am;
                    const float2 p = ch_mul(ch_mul(am, ph), b);
                    acc[m] = n == lane ? p : ch_add(acc[m], p); // ascending n, from the lane's first product
                }
            }
        }
        const float s = a.scale[l];
        irs_each_antenna(std::make_integer_sequence<int, MA>{}, [&](auto mc) {
            constexpr int m = decltype(mc)::value;
            if (MA == 1 || (uint32_t)m < M) {                   // the same in every lane
                const float2 v = irs_butterfly(acc[m]);         // symmetric: every lane ends with the same bits
                const float2 h = ch_add(irs_direct(a, m, r, l, key), v);
                if (lane == 0) a.taps_out[((uint64_t)m * a.n_sets + r) * L + l] = make_float2(h.x * s, h.y * s);
            }
        });
    }
}

}  // namespace wr

extern "C" hipError_t wr_launch_irs(hipStream_t st, const wr::IrsArgs* args)
{
    if (args->n_sets == 0) return hipSuccess;
    if (!irs_scene_ok(*args) || args->align_bits > 3 || !args->taps_out || (args->align_bits == 0 && (!args->psi || args->n_psi_sets < 1)))
        return hipErrorInvalidValue;                        // (the entry point refuses these first)
    const dim3 grid(args->n_sets), block(64 * IRS_WAVES);
#define IRS_LAUNCH(ALIGN) \
    do { \
        if (args->n_ant == 1) hipLaunchKernelGGL((wr::irs_kernel<ALIGN, 1>), grid, block, 0, st, *args); \
        else hipLaunchKernelGGL((wr::irs_kernel<ALIGN, IRSM_MAX_ANT>), grid, block, 0, st, *args); \
    } while (0)
    if (args->align_bits) IRS_LAUNCH(true);
    else IRS_LAUNCH(false);
#undef IRS_LAUNCH
    return hipGetLastError();
}

extern "C" uint32_t wr_irs_max_elems(void) { return IRS_MAX_ELEMS; }
extern "C" uint32_t wr_irs_max_taps(void) { return IRS_MAX_TAPS; }
extern "C" uint32_t wr_irs_max_ant(void) { return IRSM_MAX_ANT; }
