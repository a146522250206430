// wr_irs_sweep.hip -- beam training of a reflecting surface on the device (the purpose of the reference's "IRS Traverse" block
// in gnu_radio/IRS_tranceiver.grc: step the surface through a codebook, keep the entry with the best link), in the float32
// arithmetic of NUMERICS.md rules 26 (one AP antenna) and 28 (M = 1..8 antennas, the entries ranked by the power an MRC receiver
// collects): per tap set r the elements of rule 25 / 27 drawn ONCE, their products e_n run against all K codebook entries as one
// fma chain of 2 N terms per (row, entry), the power of every entry summed over the set's rows rho = m L + l, the winner, and
// the winner's taps.
//
// The sweep is a GEMM: rows (set, rho), inner dimension the 2 N floats (e_n.re, e_n.im), columns the 2 K coefficient columns
// (entry k's real sum and imaginary sum).  It runs on v_mfma_f32_16x16x4_f32, which is bit for bit a k-ascending fmaf chain
// (tools/mfma_f32_probe.hip, profiles/r02_mfma_f32_probe.txt), so consecutive instructions on one accumulator are the rule's
// chain.
//
// Work split, R = M L <= 16 rows per set: a workgroup of four waves owns G = 16 / R whole sets, the G R <= 16 rows of one MFMA
// tile (spare rows are +0 and written nowhere).  It walks N in chunks of 64 elements:
//   * all 256 lanes form the chunk's e_n for the 16 rows (4 elements each) into an LDS tile (wr_irs_tile.h);
//   * every wave then runs the chunk's 32 chain steps for ITS column groups.  A group is 16 entries: one A read feeds two
//     instructions, the group's real columns and its imaginary columns, whose B operands (re, -im) / (im, re) are formed from
//     ONE float2 read of the codebook (lane (col, kk) reads psi[k0 + col][n0 + 2 s + (kk >> 1)], kk & 1 picks the part), so no
//     second copy of the codebook exists.  Wave w owns the groups w, w + 4, ...: NG of them, a template parameter (1, 2, 4, 8,
//     16 for K <= 64, 128, 256, 512, 1024), so the 2 NG accumulators of 4 registers are named at compile time and stay in
//     registers across the chunks.  The draws of a (set, row) are made once whatever K is: K is not split into passes.
// After the last chunk a lane holds, for its entry, the sums of 4 rows.  Per group: h = h_d + y, t = h s_l, q = |t|^2 go through
// a per-wave LDS square so that the lane (set, entry) can add the set's R rows in ascending rho; it writes the power and keeps
// its best entry so far (its entries ascend).  The 64 candidates of a set (4 waves x 16 columns) are folded by one thread with
// the rule's order (greater power, then lower k), which is the sequential scan's result.  The lanes that hold the winner's
// sums form its taps again and store them.
//
// R > 16 (up to 128, the MT instances): a workgroup owns one set and walks its ceil(R / 16) row tiles in ascending rho, re-running
// the chunk loop per tile with the same accumulators (the AGPR count does not grow); the lane that owns an entry in the metric
// step carries the entry's running power from tile to tile (a word of LDS of its own), so the sum is the rule's ascending one.
// After the last tile the earlier tiles' sums are gone: the workgroup forms the tiles' products once more (all 256 lanes, as in
// the sweep) and one thread per row runs the winner's chain over them as VALU fmaf, which by rule 26 has the MFMA chain's bits.
// The sweep forms a row's elements on their own (b_n is drawn again for every antenna's row): the Philox saving of wr_irs.hip's
// irs_kernel is not taken here, the chain dominates.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wr_irs_tile.h"
#include "wr_irs_sweep.h"

namespace wr {

#define SW_WAVES     4
#define SW_CHUNK     IRS_TILE_CHUNK
#define SW_RS        IRS_TILE_RS
#define SW_MAX_CODES 1024

// MT: a set has more than 16 rows and is walked in row tiles
template <int NG, bool MT>
__global__ __launch_bounds__(64 * SW_WAVES)
void irs_sweep_kernel(const IrsSweepArgs a)
{
    __shared__ float       tile[16 * SW_RS];
    __shared__ float       q_s[SW_WAVES][16][17];
    __shared__ float       cand_top[SW_WAVES][16][16];
    __shared__ uint32_t    cand_best[SW_WAVES][16][16];
    __shared__ IrsTileRows rows;
    __shared__ uint32_t    set_best[16];
    // MT: every entry's power over the tiles so far, read and written by the one lane (kk = 0) that owns the entry in the
    // metric step; in LDS so that the NG values are not live across the chunk loop beside the accumulators
    __shared__ float       pw_s[MT ? SW_WAVES * NG * 16 : 1];

    const IrsArgs& sc = a.s;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t col = lane & 15, kk = lane >> 4;             // MFMA: A[row = col][k = kk], B[k = kk][col], D[row 4 kk + j][col]
    const uint32_t N = sc.n_elems, L = sc.n_taps, K = a.n_codes, M = sc.n_ant;
    const uint32_t R = M * L;                                   // rows of a set: rho = m L + l
    const uint32_t G = R >= 16 ? 1 : 16 / R;                    // whole sets per tile
    const uint32_t T = MT ? (R + 15) / 16 : 1;                  // row tiles per set (MT: R > 16, and then G = 1)
    const uint64_t set0 = (uint64_t)blockIdx.x * G;
    const uint2 key = make_uint2((uint32_t)sc.seed, (uint32_t)(sc.seed >> 32));

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
    float top[4];
    uint32_t best[4];
#pragma unroll
    for (int t = 0; t < 4; t++) { top[t] = -1.0f; best[t] = 0; }

    const uint32_t half = kk >> 1;                              // which of the step's two elements this lane's k index reads
    const bool odd = kk & 1;                                    // ... and which part of it: A is e.re (even) or e.im (odd)
    // the row tables of row tile rt (the caller's barrier before it has let every reader of the previous tables through)
    const auto set_tile = [&](uint32_t rt) {
        if (tid < 16) {
            uint32_t g = 0, rho = 16 * rt + tid;
            if (!MT) { g = tid / R; rho = tid - g * R; }
            irs_tile_row(rows, tid, sc, g < G && set0 + g < sc.n_sets && rho < R, (uint32_t)(set0 + g), rho, key);
        }
        __syncthreads();
    };

    for (uint32_t rt = 0; rt < T; rt++) {
        const uint32_t rows_here = MT ? min(16u, R - 16 * rt) : R;          // rows of one set in this tile
        set_tile(rt);
#pragma unroll
        for (int i = 0; i < NG; i++) acc_re[i] = acc_im[i] = f4{0.0f, 0.0f, 0.0f, 0.0f};

        for (uint32_t n0 = 0; n0 < N; n0 += SW_CHUNK) {
            irs_tile_form(tile, rows, sc, n0, lane, wave, key);
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
                        const float b_re = odd ? -c.y : c.x;    // real sum:      c[2n] = psi.re, c[2n+1] = -psi.im
                        const float b_im = odd ? c.x : c.y;     // imaginary sum: c[2n] = psi.im, c[2n+1] =  psi.re
                        acc_re[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b_re, acc_re[i], 0, 0, 0);
                        acc_im[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b_im, acc_im[i], 0, 0, 0);
                    }
                }
            }
            __syncthreads();
        }

        // ---- the metric: per group, the powers of 16 entries for the tile's rows, added to what the earlier tiles gave ----
        const bool last = rt + 1 == T;
#pragma unroll
        for (int i = 0; i < NG; i++) {
            const uint32_t k = (uint32_t)(i * SW_WAVES + wave) * 16 + col;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const uint32_t row = 4 * kk + j;
                const float2 h = ch_add(rows.hd[row], make_float2(acc_re[i][j], acc_im[i][j]));
                const float s = rows.scale[row];
                const float tx = h.x * s, ty = h.y * s;
                q_s[wave][row][col] = tx * tx + ty * ty;
            }
            __syncthreads();
#pragma unroll
            for (int t = 0; t < 4; t++) {
                const uint32_t g = kk + 4 * t;                  // lane (g, col): the set's rows in ascending rho
                if (g < G && rows.set[g * rows_here] != IRS_NO_SET && k < K) {
                    float p = q_s[wave][g * rows_here][col];
                    if constexpr (MT) {
                        if (rt > 0) p = pw_s[(wave * NG + i) * 16 + col] + p;       // (G = 1: only g = 0, kk = 0 comes here)
                    }
                    for (uint32_t j = 1; j < rows_here; j++) p = p + q_s[wave][g * rows_here + j][col];
                    if constexpr (MT) pw_s[(wave * NG + i) * 16 + col] = p;
                    if (last) {
                        if (a.power_out) a.power_out[(uint64_t)rows.set[g * rows_here] * K + k] = p;
                        if (p > top[t]) { top[t] = p; best[t] = k; }    // a NaN never wins; this lane's k ascend: its lowest k keeps a tie
                    }
                }
            }
            __syncthreads();
        }
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
        const bool exists = tid < G && set0 + tid < sc.n_sets;
        if (a.best_out && exists) a.best_out[set0 + tid] = (uint16_t)bs;
    }
    __syncthreads();

    if (!sc.taps_out) return;
    if constexpr (!MT) {
        // ---- the winner's taps, from the lanes that hold its sums ----
#pragma unroll
        for (int i = 0; i < NG; i++) {
            const uint32_t k = (uint32_t)(i * SW_WAVES + wave) * 16 + col;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const uint32_t row = 4 * kk + j, r = rows.set[row];
                if (r == IRS_NO_SET || k >= K || set_best[row / R] != k) continue;
                const float2 h = ch_add(rows.hd[row], make_float2(acc_re[i][j], acc_im[i][j]));
                const float s = rows.scale[row];
                sc.taps_out[((uint64_t)rows.ant[row] * sc.n_sets + r) * L + rows.tap[row]] = make_float2(h.x * s, h.y * s);
            }
        }
    } else {
        // ---- the winner's taps again: the tiles' products are formed once more as above, and thread i < 16 runs row i's chain
        // for the one winning entry on the VALU, reading the LDS tile ----
        const uint32_t r = (uint32_t)set0;                      // G = 1, and the grid has one workgroup per set
        const float2* c = a.codebook + (uint64_t)set_best[0] * N;
        for (uint32_t rt = 0; rt < T; rt++) {
            const uint32_t rows_here = min(16u, R - 16 * rt);
            set_tile(rt);
            float re = 0.0f, im = 0.0f;
            for (uint32_t n0 = 0; n0 < N; n0 += SW_CHUNK) {
                irs_tile_form(tile, rows, sc, n0, lane, wave, key);
                __syncthreads();
                if (tid < rows_here) {
                    const uint32_t cnt = min((uint32_t)SW_CHUNK, N - n0);
                    for (uint32_t s = 0; s < cnt; s++) {
                        const float2 e = *reinterpret_cast<const float2*>(&tile[tid * SW_RS + 2 * s]), p = c[n0 + s];
                        re = fmaf(e.x, p.x, re);
                        re = fmaf(e.y, -p.y, re);
                        im = fmaf(e.x, p.y, im);
                        im = fmaf(e.y, p.x, im);
                    }
                }
                __syncthreads();
            }
            if (tid < rows_here) {
                if (N & 1) {                                    // the fill of 2 N to a multiple of 4: two zero terms, with the
                    re = fmaf(0.0f, 0.0f, re);                  // operands the MFMA steps have (b_re = -c.y of c = 0)
                    re = fmaf(0.0f, -0.0f, re);
                    im = fmaf(0.0f, 0.0f, im);
                    im = fmaf(0.0f, 0.0f, im);
                }
                const float2 h = ch_add(rows.hd[tid], make_float2(re, im));
                const float sl = rows.scale[tid];
                sc.taps_out[((uint64_t)rows.ant[tid] * sc.n_sets + r) * L + rows.tap[tid]] = make_float2(h.x * sl, h.y * sl);
            }
        }
    }
}

}  // namespace wr

extern "C" hipError_t wr_launch_irs_sweep(hipStream_t st, const wr::IrsSweepArgs* args)
{
    const wr::IrsArgs& s = args->s;
    if (s.n_sets == 0) return hipSuccess;
    if (!irs_scene_ok(s) || args->n_codes < 1 || args->n_codes > SW_MAX_CODES || !args->codebook)
        return hipErrorInvalidValue;                        // (the entry point refuses these first)
    const uint32_t R = s.n_ant * s.n_taps, G = R >= 16 ? 1 : 16 / R;
    const dim3 grid((s.n_sets + G - 1) / G), block(64 * SW_WAVES);
    const uint32_t groups = (args->n_codes + 15) / 16, per_wave = (groups + SW_WAVES - 1) / SW_WAVES;
#define SW_LAUNCH(NG) \
    do { \
        if (R > 16) hipLaunchKernelGGL((wr::irs_sweep_kernel<NG, true>), grid, block, 0, st, *args); \
        else hipLaunchKernelGGL((wr::irs_sweep_kernel<NG, false>), grid, block, 0, st, *args); \
    } while (0)
    if (per_wave <= 1) SW_LAUNCH(1);
    else if (per_wave <= 2) SW_LAUNCH(2);
    else if (per_wave <= 4) SW_LAUNCH(4);
    else if (per_wave <= 8) SW_LAUNCH(8);
    else SW_LAUNCH(16);
#undef SW_LAUNCH
    return hipGetLastError();
}

extern "C" uint32_t wr_irs_max_codes(void) { return SW_MAX_CODES; }
