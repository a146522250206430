// wr_irs_estimate.hip -- channel estimation of the reflecting surface from pilot reflections (the reference's Channel.CH_est over
// Channel.DFT_matrix pilots, utils/channel.py), in the float32 arithmetic of NUMERICS.md rule 29.  Two float32 GEMMs on the matrix
// cores and one decision pass:
//
// irs_observe_kernel is wr_irs_sweep.hip's GEMM without its metric: the rows rho = m L + l of the sets against the T pilot
// configurations, contracted over the 2 N floats of a row's element products.  The row tables and the chunk's products are
// wr_irs_tile.h's, the elements, the direct path and s_l wr_irs_elem.h's, so a seed gives the bits wifirx_irs_taps_multi draws.  Entry t reads pilot[t][group[n]]: the group map
// expands the pilots while they are read, no [T][N] array exists.  The epilogue adds the noise and writes obs [n_sets][R][T].
//
// irs_despread_kernel contracts over the 2 T floats of an observation row (the obs array as floats IS the A operand) against the
// J = G + 1 de-spreading columns: column 0 is the constant 1 (the direct path), column g + 1 the conjugate of pilot[.][g].  Lane
// `col` reads pilot[t][j0 + col - 1]: contiguous in j, one 128-byte line per 16 lanes, where the sweep's codebook reads are N
// apart.  The epilogue scales by kappa, writes the estimate and, with align_bits, decides the codes of every set whose row 0 lies
// in the tile (rule 25's argmax fed with the estimate; a blocked direct path aligns to the real axis, as there), expands them through the group map and writes the phases for
// wr_irs.hip's irs_kernel, which forms the taps of the TRUE elements under them.
//
// No sum runs across rows, so both kernels cut the n_sets R rows into tiles of 16 consecutive rows regardless of the set borders:
// R < 16 puts several sets into a tile, R > 16 several tiles behind a set, and no row of a tile idles except in the last one.
// A workgroup of four waves owns a tile and all its columns: wave w the 16-column groups w, w + 4, ... (NG of them, 1..16).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wr_irs_tile.h"
#include "wr_irs_estimate.h"

namespace wr {

#define EST_WAVES      4
#define EST_CHUNK      IRS_TILE_CHUNK      // complex terms per chunk: 128 floats of the chain, 32 steps of 4
#define EST_RS         IRS_TILE_RS         // LDS row stride in floats (64 different banks per A read)
#define EST_MAX_PILOTS 1024
#define EST_MAX_GROUPS 1023
#define EST_NOISE_WORD 3u                  // counter word 3 of the observation noise (0 noise, 1 fader, 2 scatter are taken)

__device__ __forceinline__ uint32_t est_group(const IrsEstimateArgs& a, uint32_t n) { return a.group ? (uint32_t)a.group[n] : n; }

template <int NG>
__global__ __launch_bounds__(64 * EST_WAVES)
void irs_observe_kernel(const IrsEstimateArgs a)
{
    __shared__ float       tile[16 * EST_RS];
    __shared__ IrsTileRows rows;

    const IrsArgs& sc = a.s;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t col = lane & 15, kk = lane >> 4;             // MFMA: A[row = col][k = kk], B[k = kk][col], D[row 4 kk + j][col]
    const uint32_t N = sc.n_elems, L = sc.n_taps, T = a.n_pilots, G = a.n_groups;
    const uint32_t R = sc.n_ant * L;                            // rows of a set: rho = m L + l
    const uint64_t n_rows = (uint64_t)sc.n_sets * R, q0 = (uint64_t)blockIdx.x * 16;
    const uint2 key = make_uint2((uint32_t)sc.seed, (uint32_t)(sc.seed >> 32));

    if (tid < 16) {
        const uint64_t q = q0 + tid;
        const uint32_t r = (uint32_t)(q / R);
        irs_tile_row(rows, tid, sc, q < n_rows, r, (uint32_t)(q - (uint64_t)r * R), key);
    }
    __syncthreads();

    // this lane's pilot slot in group i of the wave is t_i = t_first + 64 i, its row of `pilot` 64 G values further each time
    const uint32_t t_first = wave * 16 + col;
    f4 acc_re[NG], acc_im[NG];
#pragma unroll
    for (int i = 0; i < NG; i++) acc_re[i] = acc_im[i] = f4{0.0f, 0.0f, 0.0f, 0.0f};
    const uint32_t half = kk >> 1;                              // which of the step's two elements this lane's k index reads
    const bool odd = kk & 1;                                    // ... and which part of it: A is e.re (even) or e.im (odd)

    for (uint32_t n0 = 0; n0 < N; n0 += EST_CHUNK) {
        irs_tile_form(tile, rows, sc, n0, lane, wave, key);
        __syncthreads();
        const uint32_t left = N - n0;
        const uint32_t steps = left >= EST_CHUNK ? EST_CHUNK / 2 : (left + 1) / 2;        // 2 N filled up to a multiple of 4, no further
        const float* arow = &tile[col * EST_RS + kk];
        for (uint32_t s = 0; s < steps; s++) {
            const float av = arow[4 * s];
            const uint32_t n = n0 + 2 * s + half;
            const bool in = n < N;
            const uint32_t g = in ? est_group(a, n) : 0;
#pragma unroll
            for (int i = 0; i < NG; i++) {
                if ((uint32_t)(i * EST_WAVES + wave) * 16 < T) {                          // the same in every lane of the wave
                    const uint32_t t = t_first + 16 * EST_WAVES * i;
                    float2 c = make_float2(0.0f, 0.0f);         // no such element or slot: a zero term / a column nobody reads
                    if (in && t < T) c = a.pilot[(uint64_t)t * G + g];
                    const float b_re = odd ? -c.y : c.x;        // real sum:      c[2n] = p.re, c[2n+1] = -p.im  (rule 26's)
                    const float b_im = odd ? c.x : c.y;         // imaginary sum: c[2n] = p.im, c[2n+1] =  p.re
                    acc_re[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b_re, acc_re[i], 0, 0, 0);
                    acc_im[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b_im, acc_im[i], 0, 0, 0);
                }
            }
        }
        __syncthreads();
    }

    // ---- x = s_l (h_d + y) ----
#pragma unroll
    for (int i = 0; i < NG; i++) {
        const uint32_t t = t_first + 16 * EST_WAVES * i;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const uint32_t row = 4 * kk + j;
            if (rows.set[row] == IRS_NO_SET || t >= T) continue;
            const float2 h = ch_add(rows.hd[row], make_float2(acc_re[i][j], acc_im[i][j]));
            const float s = rows.scale[row];
            a.obs[(q0 + row) * T + t] = make_float2(h.x * s, h.y * s);
        }
    }
    if (a.sigma == 0.0f) return;                                // the same in every thread: obs = x, nothing is drawn or read

    // ---- obs = x + sigma w: every thread over the values it has just written (a rolled loop: the accumulators are done with,
    // and the Box-Muller's code stands once) ----
    for (uint32_t v = 0; v < 4u * NG; v++) {
        const uint32_t t = t_first + 16 * EST_WAVES * (v >> 2), row = 4 * kk + (v & 3);
        if (rows.set[row] == IRS_NO_SET || t >= T) continue;
        const uint64_t q = q0 + row;
        float2 w;
        if (a.noise) {
            w = a.noise[(q % a.n_noise) * T + t];
        } else {
            const uint4 d = philox4x32_10(make_uint4(t, rows.set[row], rows.ant[row] * L + rows.tap[row], EST_NOISE_WORD), key);
            w = ch_noise(d.x, d.y, 0.70710678118654752f);
        }
        a.obs[q * T + t] = ch_add(a.obs[q * T + t], make_float2(a.sigma * w.x, a.sigma * w.y));
    }
}

template <int NG>
__global__ __launch_bounds__(64 * EST_WAVES)
void irs_despread_kernel(const IrsEstimateArgs a)
{
    __shared__ float    tile[16 * EST_RS];
    __shared__ float2   g0_s[16];                               // ghat_{0,0} of the rows that open a set
    __shared__ uint32_t row_set[16];
    __shared__ bool     row_used[16], row_first[16];
    __shared__ uint8_t  codes_s[16][EST_MAX_GROUPS + 1];

    const IrsArgs& sc = a.s;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t col = lane & 15, kk = lane >> 4;
    const uint32_t N = sc.n_elems, T = a.n_pilots, G = a.n_groups, J = G + 1;
    const uint32_t R = sc.n_ant * sc.n_taps;
    const uint64_t rows = (uint64_t)sc.n_sets * R, q0 = (uint64_t)blockIdx.x * 16;

    if (tid < 16) {
        const uint64_t q = q0 + tid;
        const bool used = q < rows;
        const uint32_t r = used ? (uint32_t)(q / R) : 0;
        row_used[tid] = used;
        row_set[tid] = r;
        row_first[tid] = used && q == (uint64_t)r * R;
    }
    __syncthreads();

    bool have[NG];
    uint32_t jc[NG];                                            // this lane's column in each of the wave's groups
    f4 acc_re[NG], acc_im[NG];
#pragma unroll
    for (int i = 0; i < NG; i++) {
        jc[i] = (uint32_t)(i * EST_WAVES + wave) * 16 + col;
        have[i] = jc[i] < J;
        acc_re[i] = acc_im[i] = f4{0.0f, 0.0f, 0.0f, 0.0f};
    }
    const uint32_t half = kk >> 1;
    const bool odd = kk & 1;

    for (uint32_t t0 = 0; t0 < T; t0 += EST_CHUNK) {
        {
            const uint32_t t = t0 + lane;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const uint32_t row = wave + 4 * j;
                float2 v = make_float2(0.0f, 0.0f);
                if (row_used[row] && t < T) v = a.obs[(q0 + row) * T + t];
                *reinterpret_cast<float2*>(&tile[row * EST_RS + 2 * lane]) = v;
            }
        }
        __syncthreads();
        const uint32_t left = T - t0;
        const uint32_t steps = left >= EST_CHUNK ? EST_CHUNK / 2 : (left + 1) / 2;        // 2 T filled up to a multiple of 4, no further
        const float* arow = &tile[col * EST_RS + kk];
        for (uint32_t s = 0; s < steps; s++) {
            const float av = arow[4 * s];
            const uint32_t t = t0 + 2 * s + half;
            const bool in = t < T;
            const float2* prow = a.pilot + (uint64_t)(in ? t : 0) * G;
#pragma unroll
            for (int i = 0; i < NG; i++) {
                if ((uint32_t)(i * EST_WAVES + wave) * 16 < J) {                          // the same in every lane of the wave
                    float2 p = make_float2(0.0f, 0.0f);
                    if (in && have[i]) p = jc[i] == 0 ? make_float2(1.0f, 0.0f) : prow[jc[i] - 1];
                    const float b_re = odd ? p.y : p.x;         // real sum:      c[2t] =  p.re, c[2t+1] = p.im   (obs conj(p))
                    const float b_im = odd ? p.x : -p.y;        // imaginary sum: c[2t] = -p.im, c[2t+1] = p.re
                    acc_re[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b_re, acc_re[i], 0, 0, 0);
                    acc_im[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b_im, acc_im[i], 0, 0, 0);
                }
            }
        }
        __syncthreads();
    }

    // ---- ghat = kappa * sum, one multiply per part ----
#pragma unroll
    for (int i = 0; i < NG; i++) {
#pragma unroll
        for (int j = 0; j < 4; j++) {
            acc_re[i][j] = a.kappa * acc_re[i][j];
            acc_im[i][j] = a.kappa * acc_im[i][j];
            const uint32_t row = 4 * kk + j;
            if (a.est_out && row_used[row] && have[i]) a.est_out[(q0 + row) * J + jc[i]] = make_float2(acc_re[i][j], acc_im[i][j]);
        }
    }
    if (sc.align_bits == 0) return;                             // the same in every thread

    // ---- the codes: rule 25's argmax on row 0 of a set, the estimate in place of the elements ----
    if (wave == 0 && col == 0) {                                // group 0 of wave 0 holds column 0
#pragma unroll
        for (int j = 0; j < 4; j++) g0_s[4 * kk + j] = make_float2(acc_re[0][j], acc_im[0][j]);
    }
    __syncthreads();
    const uint32_t up = 3 - sc.align_bits, n_codes = 1u << sc.align_bits;
#pragma unroll
    for (int i = 0; i < NG; i++) {
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const uint32_t row = 4 * kk + j;
            if (!row_first[row] || !have[i] || jc[i] == 0) continue;
            const float2 hd = g0_s[row];
            // no direct path to align to -- blocked (rule 27's direct_gain = 0: h_d is exactly +0, and its estimate, which is
            // nothing but noise and rounding, is not consulted), or an estimate of zero: the positive real axis
            const bool axis = sc.direct_gain == 0.0f || (hd.x == 0.0f && hd.y == 0.0f);
            float2 g = make_float2(acc_re[i][j], acc_im[i][j]);
            if (!axis) g = ch_mul(make_float2(hd.x, -hd.y), g);
            codes_s[row][jc[i] - 1] = (uint8_t)irs_argmax(g, irs_phase, n_codes, up);
        }
    }
    __syncthreads();
    for (uint32_t row = 0; row < 16; row++) {
        if (!row_first[row]) continue;                          // the same in every thread
        const uint32_t r = row_set[row];
        if (sc.codes_out)
            for (uint32_t g = tid; g < G; g += 64 * EST_WAVES) sc.codes_out[(uint64_t)r * G + g] = codes_s[row][g];
        if (a.psi_out)
            for (uint32_t n = tid; n < N; n += 64 * EST_WAVES)
                a.psi_out[(uint64_t)r * N + n] = irs_phase[(uint32_t)codes_s[row][est_group(a, n)] << up];
    }
}

}  // namespace wr

static bool est_args_ok(const wr::IrsEstimateArgs* a)
{
    const wr::IrsArgs& s = a->s;
    return irs_scene_ok(s) && s.align_bits <= 3 && a->pilot && a->obs &&
           a->n_pilots >= 1 && a->n_pilots <= EST_MAX_PILOTS && a->n_groups >= 1 && a->n_groups <= EST_MAX_GROUPS &&
           a->n_groups <= s.n_elems && (a->group || a->n_groups == s.n_elems) && (!a->noise || a->n_noise >= 1) &&
           ((uint64_t)s.n_sets * s.n_ant * s.n_taps + 15) / 16 <= 0x7fffffffu;
}

#define EST_LAUNCH(KERNEL, COLS) \
    do { \
        const uint32_t groups = ((COLS) + 15) / 16, per_wave = (groups + EST_WAVES - 1) / EST_WAVES; \
        if (per_wave <= 1) hipLaunchKernelGGL((wr::KERNEL<1>), grid, block, 0, st, *args); \
        else if (per_wave <= 2) hipLaunchKernelGGL((wr::KERNEL<2>), grid, block, 0, st, *args); \
        else if (per_wave <= 4) hipLaunchKernelGGL((wr::KERNEL<4>), grid, block, 0, st, *args); \
        else if (per_wave <= 8) hipLaunchKernelGGL((wr::KERNEL<8>), grid, block, 0, st, *args); \
        else hipLaunchKernelGGL((wr::KERNEL<16>), grid, block, 0, st, *args); \
    } while (0)

extern "C" hipError_t wr_launch_irs_observe(hipStream_t st, const wr::IrsEstimateArgs* args)
{
    if (args->s.n_sets == 0) return hipSuccess;
    if (!est_args_ok(args)) return hipErrorInvalidValue;        // (the entry point refuses these first)
    const uint64_t rows = (uint64_t)args->s.n_sets * args->s.n_ant * args->s.n_taps;
    const dim3 grid((uint32_t)((rows + 15) / 16)), block(64 * EST_WAVES);
    EST_LAUNCH(irs_observe_kernel, args->n_pilots);
    return hipGetLastError();
}

extern "C" hipError_t wr_launch_irs_despread(hipStream_t st, const wr::IrsEstimateArgs* args)
{
    if (args->s.n_sets == 0) return hipSuccess;
    if (!est_args_ok(args)) return hipErrorInvalidValue;        // (the entry point refuses these first)
    const uint64_t rows = (uint64_t)args->s.n_sets * args->s.n_ant * args->s.n_taps;
    const dim3 grid((uint32_t)((rows + 15) / 16)), block(64 * EST_WAVES);
    EST_LAUNCH(irs_despread_kernel, args->n_groups + 1);
    return hipGetLastError();
}
#undef EST_LAUNCH

extern "C" uint32_t wr_irs_max_pilots(void) { return EST_MAX_PILOTS; }
extern "C" uint32_t wr_irs_max_groups(void) { return EST_MAX_GROUPS; }
