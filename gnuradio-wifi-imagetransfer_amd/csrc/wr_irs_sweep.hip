// wr_irs_sweep.hip -- beam training of a reflecting surface on the device (the purpose of the reference's "IRS Traverse" block
// in gnu_radio/IRS_tranceiver.grc: step the surface through a codebook, keep the entry with the best link), in the float32
// arithmetic of NUMERICS.md rule 26: per tap set r the elements of rule 25 drawn ONCE, their products e_n run against all K
// codebook entries as one fma chain of 2 N terms per (tap, entry), the power of every entry summed over the taps, the winner,
// and the winner's taps.
//
// The sweep is a GEMM: rows (set, tap), inner dimension the 2 N floats (e_n.re, e_n.im), columns the 2 K coefficient columns
// (entry k's real sum and imaginary sum).  It runs on v_mfma_f32_16x16x4_f32, which is bit for bit a k-ascending fmaf chain
// (tools/mfma_f32_probe.hip, profiles/r02_mfma_f32_probe.txt), so consecutive instructions on one accumulator are the rule's
// chain.
//
// Work split: a workgroup of four waves owns G = max(1, 16 / L) whole sets, the G L <= 16 rows of one MFMA tile (spare rows
// are +0 and written nowhere).  It walks N in chunks of 64 elements:
//   * all 256 lanes form the chunk's e_n for the 16 rows (4 elements each) into an LDS tile [16][128 + 4] floats; the row
//     stride of 132 puts lane (row, kk)'s word at bank 4 row + kk, so the A-operand reads of a wave hit 64 different banks;
//   * every wave then runs the chunk's 32 chain steps for ITS column groups.  A group is 16 entries: one A read feeds two
//     instructions, the group's real columns and its imaginary columns, whose B operands (re, -im) / (im, re) are formed from
//     ONE float2 read of the codebook (lane (col, kk) reads psi[k0 + col][n0 + 2 s + (kk >> 1)], kk & 1 picks the part), so no
//     second copy of the codebook exists.  Wave w owns the groups w, w + 4, ...: NG of them, a template parameter (1, 2, 4, 8,
//     16 for K <= 64, 128, 256, 512, 1024), so the 2 NG accumulators of 4 registers are named at compile time and stay in
//     registers across the chunks.  The draws of a (set, tap) are made once whatever K is: K is not split into passes.
// After the last chunk a lane holds, for its entry, the sums of 4 rows.  Per group: h = h_d + y, t = h s_l, q = |t|^2 go through
// a per-wave LDS square so that the lane (set, entry) can add the set's L rows in ascending l; it writes the power and keeps
// its best entry so far (its entries ascend).  The 64 candidates of a set (4 waves x 16 columns) are folded by one thread with
// the rule's order (greater power, then lower k), which is the sequential scan's result.  The lanes that hold the winner's
// sums form its taps again and store them.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wr_irs_elem.h"
#include "wr_irs_sweep.h"

namespace wr {

#define SW_WAVES     4
#define SW_CHUNK     64                 // elements per chunk: 128 floats of the chain, 32 steps of 4
#define SW_RS        (2 * SW_CHUNK + 4) // LDS row stride in floats
#define SW_MAX_CODES 1024
#define SW_NO_SET    0xFFFFFFFFu

typedef float f4 __attribute__((ext_vector_type(4)));

template <int NG>
__global__ __launch_bounds__(64 * SW_WAVES)
void irs_sweep_kernel(const IrsSweepArgs a)
{
    __shared__ float    tile[16 * SW_RS];
    __shared__ float    q_s[SW_WAVES][16][17];
    __shared__ float    cand_top[SW_WAVES][16][16];
    __shared__ uint32_t cand_best[SW_WAVES][16][16];
    __shared__ float2   row_hd[16];
    __shared__ float    row_scale[16];
    __shared__ uint32_t row_set[16], row_tap[16], set_best[16];

    const IrsArgs& sc = a.s;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t col = lane & 15, kk = lane >> 4;             // MFMA: A[row = col][k = kk], B[k = kk][col], D[row 4 kk + j][col]
    const uint32_t N = sc.n_elems, L = sc.n_taps, K = a.n_codes;
    const uint32_t G = L >= 16 ? 1 : 16 / L;
    const uint64_t set0 = (uint64_t)blockIdx.x * G;
    const uint2 key = make_uint2((uint32_t)sc.seed, (uint32_t)(sc.seed >> 32));

    if (tid < 16) {
        const uint32_t g = tid / L, l = tid - g * L;
        const bool used = g < G && set0 + g < sc.n_sets;
        const uint32_t r = used ? (uint32_t)(set0 + g) : SW_NO_SET;
        row_set[tid] = r;
        row_tap[tid] = l;
        row_hd[tid] = used ? irs_direct(sc, r, l, key) : make_float2(0.0f, 0.0f);
        row_scale[tid] = used ? sc.scale[l] : 0.0f;
    }
    __syncthreads();

    // this lane's entry in each of the wave's groups, and its codebook row (the last row where the entry does not exist: the
    // address stays inside the codebook and the value is not used)
    const float2* cb[NG];
    bool have[NG];
#pragma unroll
    for (int i = 0; i < NG; i++) {
        const uint32_t k = (uint32_t)(i * SW_WAVES + wave) * 16 + col;
        have[i] = k < K;
        cb[i] = a.codebook + (uint64_t)(have[i] ? k : K - 1) * N;
    }
    f4 acc_re[NG], acc_im[NG];
#pragma unroll
    for (int i = 0; i < NG; i++) acc_re[i] = acc_im[i] = f4{0.0f, 0.0f, 0.0f, 0.0f};

    const uint32_t half = kk >> 1;                              // which of the step's two elements this lane's k index reads
    const bool odd = kk & 1;                                    // ... and which part of it: A is e.re (even) or e.im (odd)
    for (uint32_t n0 = 0; n0 < N; n0 += SW_CHUNK) {
        {   // the chunk's products: lane t forms element n0 + (t & 63) of the rows (t >> 6) + 4 j
            const uint32_t n = n0 + lane;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const uint32_t row = wave + 4 * j, r = row_set[row];
                float2 e = make_float2(0.0f, 0.0f);             // no such row or element: the chain's zero terms
                if (r != SW_NO_SET && n < N) {
                    const IrsElem el = irs_elem(sc, r, row_tap[row], n, key);
                    e = ch_mul(el.a, el.b);
                }
                *reinterpret_cast<float2*>(&tile[row * SW_RS + 2 * lane]) = e;
            }
        }
        __syncthreads();
        const uint32_t left = N - n0;
        const uint32_t steps = left >= SW_CHUNK ? SW_CHUNK / 2 : (left + 1) / 2;      // 2 N filled up to a multiple of 4, no further
        const float* arow = &tile[col * SW_RS + kk];
        for (uint32_t s = 0; s < steps; s++) {
            const float av = arow[4 * s];
            const uint32_t n = n0 + 2 * s + half;
            const bool in = n < N;
#pragma unroll
            for (int i = 0; i < NG; i++) {
                if ((uint32_t)(i * SW_WAVES + wave) * 16 < K) {                       // the same in every lane of the wave
                    float2 c = make_float2(0.0f, 0.0f);
                    if (in && have[i]) c = cb[i][n];
                    const float b_re = odd ? -c.y : c.x;        // real sum:      c[2n] = psi.re, c[2n+1] = -psi.im
                    const float b_im = odd ? c.x : c.y;         // imaginary sum: c[2n] = psi.im, c[2n+1] =  psi.re
                    acc_re[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b_re, acc_re[i], 0, 0, 0);
                    acc_im[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b_im, acc_im[i], 0, 0, 0);
                }
            }
        }
        __syncthreads();
    }

    // ---- the metric: per group, the powers of 16 entries for the tile's sets ----
    float top[4];
    uint32_t best[4];
#pragma unroll
    for (int t = 0; t < 4; t++) { top[t] = -1.0f; best[t] = 0; }
#pragma unroll
    for (int i = 0; i < NG; i++) {
        const uint32_t k = (uint32_t)(i * SW_WAVES + wave) * 16 + col;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const uint32_t row = 4 * kk + j;
            const float2 h = ch_add(row_hd[row], make_float2(acc_re[i][j], acc_im[i][j]));
            const float s = row_scale[row];
            const float tx = h.x * s, ty = h.y * s;
            q_s[wave][row][col] = tx * tx + ty * ty;
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const uint32_t g = kk + 4 * t;                      // lane (g, col): the set's L rows in ascending l
            if (g < G && row_set[g * L] != SW_NO_SET && k < K) {
                float p = q_s[wave][g * L][col];
                for (uint32_t l = 1; l < L; l++) p = p + q_s[wave][g * L + l][col];
                if (a.power_out) a.power_out[(uint64_t)row_set[g * L] * K + k] = p;
                if (p > top[t]) { top[t] = p; best[t] = k; }    // a NaN never wins; this lane's k ascend, so its lowest k keeps a tie
            }
        }
        __syncthreads();
    }

    // ---- the winner: 64 candidates per set, greater power first, then the lower k ----
#pragma unroll
    for (int t = 0; t < 4; t++) {
        cand_top[wave][kk + 4 * t][col] = top[t];
        cand_best[wave][kk + 4 * t][col] = best[t];
    }
    __syncthreads();
    if (tid < 16) {
        float tp = -1.0f;
        uint32_t bs = 0;
        for (uint32_t w = 0; w < SW_WAVES; w++)
            for (uint32_t c = 0; c < 16; c++) {
                const float p = cand_top[w][tid][c];
                const uint32_t b = cand_best[w][tid][c];
                if (p > tp || (p == tp && b < bs)) { tp = p; bs = b; }
            }
        set_best[tid] = bs;
        const uint32_t r = tid < G ? row_set[tid * L] : SW_NO_SET;
        if (a.best_out && r != SW_NO_SET) a.best_out[r] = (uint16_t)bs;
    }
    __syncthreads();

    // ---- the winner's taps, from the lanes that hold its sums ----
    if (sc.taps_out) {
#pragma unroll
        for (int i = 0; i < NG; i++) {
            const uint32_t k = (uint32_t)(i * SW_WAVES + wave) * 16 + col;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const uint32_t row = 4 * kk + j, r = row_set[row];
                if (r == SW_NO_SET || k >= K || set_best[row / L] != k) continue;
                const float2 h = ch_add(row_hd[row], make_float2(acc_re[i][j], acc_im[i][j]));
                const float s = row_scale[row];
                sc.taps_out[(uint64_t)r * L + row_tap[row]] = make_float2(h.x * s, h.y * s);
            }
        }
    }
}

}  // namespace wr

extern "C" hipError_t wr_launch_irs_sweep(hipStream_t st, const wr::IrsSweepArgs* args)
{
    const wr::IrsArgs& s = args->s;
    if (s.n_sets == 0) return hipSuccess;
    if (s.n_elems < 1 || s.n_elems > IRS_MAX_ELEMS || s.n_taps < 1 || s.n_taps > IRS_MAX_TAPS || args->n_codes < 1 ||
        args->n_codes > SW_MAX_CODES || s.n_sets > 0x7fffffffu || !args->codebook)
        return hipErrorInvalidValue;                        // (the entry point refuses these first)
    const uint32_t G = s.n_taps >= 16 ? 1 : 16 / s.n_taps;
    const dim3 grid((s.n_sets + G - 1) / G), block(64 * SW_WAVES);
    const uint32_t groups = (args->n_codes + 15) / 16, per_wave = (groups + SW_WAVES - 1) / SW_WAVES;
    if (per_wave <= 1) hipLaunchKernelGGL((wr::irs_sweep_kernel<1>), grid, block, 0, st, *args);
    else if (per_wave <= 2) hipLaunchKernelGGL((wr::irs_sweep_kernel<2>), grid, block, 0, st, *args);
    else if (per_wave <= 4) hipLaunchKernelGGL((wr::irs_sweep_kernel<4>), grid, block, 0, st, *args);
    else if (per_wave <= 8) hipLaunchKernelGGL((wr::irs_sweep_kernel<8>), grid, block, 0, st, *args);
    else hipLaunchKernelGGL((wr::irs_sweep_kernel<16>), grid, block, 0, st, *args);
    return hipGetLastError();
}

extern "C" uint32_t wr_irs_max_codes(void) { return SW_MAX_CODES; }
