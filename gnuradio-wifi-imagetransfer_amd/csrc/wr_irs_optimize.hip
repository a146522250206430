// wr_irs_optimize.hip -- the joint phase decision of the reflecting surface over antennas and taps (NUMERICS.md rule 30): cyclic
// coordinate ascent on P = sum_rho |d_rho + sum_g e_{rho,g} C_{c_g}|^2 over the B-bit codes c_g, on the coefficient matrix that
// wifirx_irs_estimate leaves in est_out.  For one group the best code is rule 25's argmax on z_g = sum_rho conj(r_rho) e_{rho,g},
// r the running sum without the group's own term, so the decision is built from wr_irs_elem.h's irs_argmax and irs_butterfly.
// The WEIGHTED instances (rule 31, wifirx_irs_optimize_weighted) ascend P_w = sum_rho w_rho |..|^2 for real weights of either sign:
// the same body with w_rho on the row's term of z and of the power; the two weights of a lane live in two registers for the call.
//
// Work split: one wave owns one set, a workgroup holds four sets.  The rows go across the lanes: lane i holds the running sums of
// the rows i and i + 64 in registers for the whole call, so a step costs no memory traffic but the group's column, and the sum over
// the rows is one add per lane and the butterfly (no LDS, no barrier).  A wave runs a dependent chain of (max_sweeps + 1) G steps;
// the kernel is bound by that chain's latency, not by bandwidth, and the other waves of the SIMD fill its gaps.
//
// Memory access: est_out's [R][J] layout puts the rows of one column 8 J bytes apart, so a column read is 64 lines per load.  Every
// lane therefore reads OPT_CHUNK = 8 consecutive columns of its own two rows at a time (64 bytes, half a line, in 8-byte loads: a
// row starts at an odd multiple of 8 bytes when J is odd, so nothing wider is aligned) and then runs the chunk's 8 steps out of
// registers.  The loads stand at the head of the chunk, so their latency shows once per 8 steps; asking for the next chunk under
// the steps of the one in work (two chunks of registers, 110 VGPRs) was measured at 3 to 5 % and not kept.
//
// The codes of the set live in LDS (1 KiB per wave).  Every lane writes every code (the lanes hold the same bits behind the
// butterfly) and later reads only what it has itself written, so the waves of a workgroup need no barrier and may leave the sweep
// loop at different times.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wr_irs_elem.h"           // irs_phase, irs_argmax, irs_butterfly; wr_channel.h's ch_mul, ch_add
#include "wr_irs_optimize.h"

namespace wr {

#define OPT_WAVES      4
#define OPT_CHUNK      8
#define OPT_MAX_ROWS   128
#define OPT_MAX_COLS   1024
#define OPT_MAX_SWEEPS 16

// C_k for a k that is the same in every lane: a chain of selects over the table's constants, no load behind the argmax
__device__ __forceinline__ float2 opt_phase(uint32_t k)
{
    float2 v = irs_phase[0];
#pragma unroll
    for (uint32_t i = 1; i < 8; i++)
        if (k == i) v = irs_phase[i];
    return v;
}

// the power of the state: q_rho = s.re s.re + s.im s.im, lane i forms q_i + q_{i+64} (absent rows +0), then the butterfly
__device__ __forceinline__ float opt_power(float2 s0, float2 s1, bool have0, bool have1)
{
    const float q0 = have0 ? s0.x * s0.x + s0.y * s0.y : 0.0f;
    const float q1 = have1 ? s1.x * s1.x + s1.y * s1.y : 0.0f;
    return irs_butterfly(make_float2(q0 + q1, 0.0f)).x;
}

// rule 31: a row's term w v of a sum over the rows, one multiply per part behind the value; +0 is selected, not multiplied, where
// w == 0 (either sign), which an absent row's weight is
__device__ __forceinline__ float opt_weigh(float w, float v) { return w != 0.0f ? w * v : 0.0f; }

// rule 31's power: w_rho q_rho in place of q_rho
__device__ __forceinline__ float opt_power_w(float2 s0, float2 s1, float w0, float w1)
{
    const float q0 = opt_weigh(w0, s0.x * s0.x + s0.y * s0.y), q1 = opt_weigh(w1, s1.x * s1.x + s1.y * s1.y);
    return irs_butterfly(make_float2(q0 + q1, 0.0f)).x;
}

template <int BITS, bool WEIGHTED>
__global__ __launch_bounds__(64 * OPT_WAVES)
void irs_optimize_kernel(const IrsOptimizeArgs a)
{
    __shared__ uint8_t codes_s[OPT_WAVES][OPT_MAX_COLS];
    constexpr uint32_t up = 3 - BITS, n_codes = 1u << BITS;     // code c is C_{c << up}
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t set = (uint64_t)blockIdx.x * OPT_WAVES + wave;
    if (set >= a.n_sets) return;                                // the whole wave; there is no barrier below
    const uint32_t R = a.n_rows, J = a.n_cols, G = J - 1;
    const bool have0 = lane < R, have1 = lane + 64 < R;
    const float2* q = a.coef + set * R * J;
    const float2* row0 = q + (uint64_t)(have0 ? lane : 0) * J;
    const float2* row1 = q + (uint64_t)(have1 ? lane + 64 : 0) * J;
    const float2 zero = make_float2(0.0f, 0.0f);
    uint8_t* cs = codes_s[wave];
    const bool blocked = a.blocked != 0;
    // rule 31: the weights of the lane's two rows, loaded once; set r reads block r % n_weight_sets, and n_weight_sets is 1 or
    // n_sets (the launcher refuses anything else), so that is block 0 or block r
    float w0 = 0.0f, w1 = 0.0f;
    if constexpr (WEIGHTED) {
        const float* w = a.weight + (a.n_weight_sets == 1 ? 0 : set) * R;
        if (have0) w0 = w[lane];
        if (have1) w1 = w[lane + 64];
    }

    // ---- 1, 2: the start codes and the state s = d + sum_g e_g C_{c_g}, g ascending ----
    float2 s0 = (have0 && !blocked) ? row0[0] : zero, s1 = (have1 && !blocked) ? row1[0] : zero;
    const float2 hd = blocked ? zero : q[0];                    // START_REF: row 0's direct term
    const bool axis = blocked || (hd.x == 0.0f && hd.y == 0.0f);
    for (uint32_t g0 = 0; g0 < G; g0 += OPT_CHUNK) {
        float2 e0[OPT_CHUNK], e1[OPT_CHUNK];
#pragma unroll
        for (int k = 0; k < OPT_CHUNK; k++) {
            const bool in = g0 + k < G;
            e0[k] = (in && have0) ? row0[g0 + k + 1] : zero;
            e1[k] = (in && have1) ? row1[g0 + k + 1] : zero;
        }
#pragma unroll
        for (int k = 0; k < OPT_CHUNK; k++) {
            const uint32_t g = g0 + k;
            if (g >= G) break;                                  // the same in every lane
            uint32_t c = 0;
            if (a.start == OPT_START_GIVEN) {
                c = a.codes_in[set * G + g] & (n_codes - 1);
            } else if (a.start == OPT_START_REF) {              // rule 29's decision: row 0 alone
                float2 v = q[g + 1];
                if (!axis) v = ch_mul(make_float2(hd.x, -hd.y), v);
                c = irs_argmax(v, irs_phase, n_codes, up);
            }
            c = __builtin_amdgcn_readfirstlane(c);
            const float2 ph = opt_phase(c << up);
            s0 = ch_add(s0, ch_mul(e0[k], ph));
            s1 = ch_add(s1, ch_mul(e1[k], ph));
            cs[g] = (uint8_t)c;
        }
    }
    float pw = WEIGHTED ? opt_power_w(s0, s1, w0, w1) : opt_power(s0, s1, have0, have1);
    float* pout = a.power_out ? a.power_out + set * (a.max_sweeps + 1) : nullptr;
    if (pout && lane == 0) pout[0] = pw;

    // ---- 3, 4, 5: the sweeps ----
    uint32_t done = 0, it = 1;
    for (; it <= a.max_sweeps; it++) {
        bool changed = false;
        for (uint32_t g0 = 0; g0 < G; g0 += OPT_CHUNK) {
            float2 e0[OPT_CHUNK], e1[OPT_CHUNK];
#pragma unroll
            for (int k = 0; k < OPT_CHUNK; k++) {
                const bool in = g0 + k < G;
                e0[k] = (in && have0) ? row0[g0 + k + 1] : zero;
                e1[k] = (in && have1) ? row1[g0 + k + 1] : zero;
            }
#pragma unroll
            for (int k = 0; k < OPT_CHUNK; k++) {
                const uint32_t g = g0 + k;
                if (g >= G) break;                              // the same in every lane
                const uint32_t c = __builtin_amdgcn_readfirstlane((uint32_t)cs[g]);
                const float2 ph = opt_phase(c << up);
                const float2 p0 = ch_mul(e0[k], ph), p1 = ch_mul(e1[k], ph);
                const float2 r0 = make_float2(s0.x - p0.x, s0.y - p0.y), r1 = make_float2(s1.x - p1.x, s1.y - p1.y);
                const float2 t0 = have0 ? ch_mul(make_float2(r0.x, -r0.y), e0[k]) : zero;      // absent rows are +0
                const float2 t1 = have1 ? ch_mul(make_float2(r1.x, -r1.y), e1[k]) : zero;
                const float2 z = irs_butterfly(                 // rule 31: tw = (w t.re, w t.im), +0 where w == 0
                    WEIGHTED ? make_float2(opt_weigh(w0, t0.x) + opt_weigh(w1, t1.x), opt_weigh(w0, t0.y) + opt_weigh(w1, t1.y))
                             : make_float2(t0.x + t1.x, t0.y + t1.y));
                const uint32_t cn = __builtin_amdgcn_readfirstlane(irs_argmax(z, irs_phase, n_codes, up));
                if (cn != c) {                                  // otherwise s stays as it was: not (s - p) + p
                    const float2 pn = opt_phase(cn << up);
                    const float2 n0 = ch_mul(e0[k], pn), n1 = ch_mul(e1[k], pn);
                    s0 = make_float2(r0.x + n0.x, r0.y + n0.y);
                    s1 = make_float2(r1.x + n1.x, r1.y + n1.y);
                    cs[g] = (uint8_t)cn;
                    changed = true;
                }
            }
        }
        pw = WEIGHTED ? opt_power_w(s0, s1, w0, w1) : opt_power(s0, s1, have0, have1);
        if (pout && lane == 0) pout[it] = pw;
        if (!changed) break;                                    // every later sweep would repeat this one bit for bit
        done++;
    }
    if (pout && lane == 0)
        for (uint32_t i = it + 1; i <= a.max_sweeps; i++) pout[i] = pw;
    if (a.sweeps_out && lane == 0) a.sweeps_out[set] = (uint8_t)done;

    // ---- the outputs: every lane reads codes it has itself written ----
    if (a.codes_out)
        for (uint32_t g = lane; g < G; g += 64) a.codes_out[set * G + g] = cs[g];
    if (a.psi_out)
        for (uint32_t n = lane; n < a.n_elems; n += 64) {
            const uint32_t g = a.group ? (uint32_t)a.group[n] : n;
            a.psi_out[set * a.n_elems + n] = irs_phase[(uint32_t)cs[g] << up];
        }
}

}  // namespace wr

extern "C" hipError_t wr_launch_irs_optimize(hipStream_t st, const wr::IrsOptimizeArgs* args)
{
    if (args->n_sets == 0) return hipSuccess;
    const uint32_t G = args->n_cols - 1;
    if (!args->coef || args->n_rows < 1 || args->n_rows > OPT_MAX_ROWS || args->n_cols < 2 || args->n_cols > OPT_MAX_COLS ||
        args->bits < 1 || args->bits > 3 || args->max_sweeps > OPT_MAX_SWEEPS || args->start > OPT_START_ZERO ||
        (args->start == OPT_START_GIVEN && !args->codes_in) || args->n_sets > 0x7fffffffu ||
        (args->psi_out && (args->n_elems < 1 || (!args->group && args->n_elems != G))))
        return hipErrorInvalidValue;                            // (the entry point refuses these first)
    if (args->weight && args->n_weight_sets != 1 && args->n_weight_sets != args->n_sets) return hipErrorInvalidValue;
    const dim3 grid((args->n_sets + OPT_WAVES - 1) / OPT_WAVES), block(64 * OPT_WAVES);
    if (args->weight) {                                         // rule 31
        if (args->bits == 1) hipLaunchKernelGGL((wr::irs_optimize_kernel<1, true>), grid, block, 0, st, *args);
        else if (args->bits == 2) hipLaunchKernelGGL((wr::irs_optimize_kernel<2, true>), grid, block, 0, st, *args);
        else hipLaunchKernelGGL((wr::irs_optimize_kernel<3, true>), grid, block, 0, st, *args);
    } else if (args->bits == 1) hipLaunchKernelGGL((wr::irs_optimize_kernel<1, false>), grid, block, 0, st, *args);
    else if (args->bits == 2) hipLaunchKernelGGL((wr::irs_optimize_kernel<2, false>), grid, block, 0, st, *args);
    else hipLaunchKernelGGL((wr::irs_optimize_kernel<3, false>), grid, block, 0, st, *args);
    return hipGetLastError();
}

extern "C" uint32_t wr_irs_max_rows(void) { return OPT_MAX_ROWS; }
extern "C" uint32_t wr_irs_max_sweeps(void) { return OPT_MAX_SWEEPS; }
