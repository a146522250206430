// wr_irs_multi.hip -- the reflecting surface seen by an AP of M = 1..8 antennas (the reference's Saleh_Valenzuela_Channel with
// antennaNum = M: H_B2R [M, N], H_B2U [M], one surface-to-user leg H_R2U shared by every antenna), in the float32 arithmetic of
// NUMERICS.md rules 27 (the cascade, irs_multi_kernel) and 28 (beam training on the MRC metric, irs_sweep_multi_kernel).
// Antenna 0 is rule 25 / 26 bit for bit: the same counters, the same operations in the same order (wr_irs_elem.h's irs_mix,
// wr_rng.h's ch_noise, wr_channel.h's ch_mul / ch_add).
//
// irs_multi_kernel has wr_irs.hip's geometry: one workgroup of four waves per tap set, wave w the taps l = w, w + 4, ...  Lane i
// forms b_n ONCE for its elements n = i, i + 64, ..., then a_{m,n} for the M antennas (one Philox draw serves the antennas 2 j - 1
// and 2 j, so an element costs 1 + ceil((M - 1) / 2) draws, not M), and keeps M partial sums in registers: the antenna loop is
// unrolled to 8 with a wave-uniform guard, so every accumulator has a name at compile time and nothing goes to scratch.  M
// butterflies fold them.  The aligned mode decides the codes on antenna 0, tap 0, exactly as wr_irs.hip does.
//
// irs_sweep_multi_kernel is wr_irs_sweep.hip's GEMM with the rows rho = m L + l of a set.  R = M L <= 16: a tile holds
// G = 16 / R whole sets, as there.  R > 16 (up to 128): a workgroup owns one set and walks its ceil(R / 16) row tiles in
// ascending rho, re-running the chunk loop per tile with the same accumulators (the AGPR count is wr_irs_sweep.hip's); the lane
// that owns an entry in the metric step carries the entry's running power from tile to tile (a word of LDS of its own), so the sum is the
// rule's ascending one.  After the last tile the earlier tiles' sums are gone: the workgroup forms the tiles' products once more
// (all 256 lanes, as in the sweep) and one thread per row runs the winner's chain over them as VALU fmaf, which by rule 26 has
// the MFMA chain's bits.  The sweep forms a row's elements on their own (b_n is drawn again for every antenna's row): the
// Philox saving of irs_multi_kernel is not taken here, the chain dominates.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wr_irs_multi_elem.h"   // irsm_elem, irsm_direct, irs_multi_phase; wr_irs_elem.h's irs_mix, IrsElem, IRS_MAX_*

namespace wr {

#define IRSM_WAVES    4

// ALIGN: the phases are the B-bit codes decided on antenna 0, tap 0 (rule 27, the genie of the reference antenna), not a.s.psi
template <bool ALIGN>
__global__ __launch_bounds__(64 * IRSM_WAVES)
void irs_multi_kernel(const IrsMultiArgs a)
{
    __shared__ uint8_t codes[ALIGN ? IRS_MAX_ELEMS : 1];
    const IrsArgs& sc = a.s;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t r = blockIdx.x, N = sc.n_elems, L = sc.n_taps, M = a.n_ant;
    const uint2 key = make_uint2((uint32_t)sc.seed, (uint32_t)(sc.seed >> 32));
    const uint32_t up = 3 - sc.align_bits;              // ALIGN: code c is irs_multi_phase[c << up]
    const float2 zero = make_float2(0.0f, 0.0f);

    if constexpr (ALIGN) {
        const float2 hd = irsm_direct(a, 0, r, 0, key);
        const bool axis = hd.x == 0.0f && hd.y == 0.0f;     // no direct path to align to: the positive real axis
        const float2 hc = make_float2(hd.x, -hd.y);
        const uint32_t n_codes = 1u << sc.align_bits;
        for (uint32_t n = tid; n < N; n += 64 * IRSM_WAVES) {
            const IrsElem e = irsm_elem(a, 0, r, 0, n, key);
            float2 g = ch_mul(e.a, e.b);
            if (!axis) g = ch_mul(hc, g);
            uint32_t best = 0;
            float top = ch_mul(g, irs_multi_phase[0]).x;
            for (uint32_t c = 1; c < n_codes; c++) {
                const float v = ch_mul(g, irs_multi_phase[c << up]).x;
                if (v > top) { top = v; best = c; }        // the lowest c wins a tie
            }
            codes[n] = (uint8_t)best;
            if (sc.codes_out) sc.codes_out[(uint64_t)r * N + n] = (uint8_t)best;
        }
        __syncthreads();
    }

    const float2* psi = ALIGN ? nullptr : sc.psi + (uint64_t)(r % sc.n_psi_sets) * N;
    for (uint32_t l = wave; l < L; l += IRSM_WAVES) {
        float2 acc[IRSM_MAX_ANT];
#pragma unroll
        for (int m = 0; m < IRSM_MAX_ANT; m++) acc[m] = zero;   // a lane without an element holds +0
        float2* eo = sc.elems_out ? sc.elems_out + ((uint64_t)r * L + l) * (uint64_t)(M + 1) * N : nullptr;
        const float2* row = sc.scatter ? irsm_row(a, r, l) : nullptr;
        for (uint32_t n = lane; n < N; n += 64) {
            uint4 d = make_uint4(0, 0, 0, 0);
            float2 wb;
            if (row) {
                wb = row[(uint64_t)M * N + n];
            } else {
                d = philox4x32_10(make_uint4(n, r, l, 2u), key);
                wb = ch_noise(d.z, d.w, 0.70710678118654752f);
            }
            const float2 b = irsm_mix(sc, sc.los_b, n, wb);
            if (eo) eo[(uint64_t)M * N + n] = b;
            float2 ph;
            if constexpr (ALIGN) ph = irs_multi_phase[(uint32_t)codes[n] << up];
            else ph = psi[n];
#pragma unroll
            for (int m = 0; m < IRSM_MAX_ANT; m++) {
                if ((uint32_t)m < M) {                          // the same in every lane
                    float2 wa;
                    if (row) {
                        wa = row[(uint64_t)m * N + n];
                    } else {
                        if (m & 1) d = philox4x32_10(make_uint4(n, r, irsm_ctr(l, m), 2u), key);   // serves m and m + 1
                        wa = irsm_pick(d, m);
                    }
                    const float2 am = irsm_mix(sc, sc.los_a, (uint64_t)m * N + n, wa);
                    if (eo) eo[(uint64_t)m * N + n] = am;
                    const float2 p = ch_mul(ch_mul(am, ph), b);
                    acc[m] = n == lane ? p : ch_add(acc[m], p); // ascending n, from the lane's first product
                }
            }
        }
        const float s = sc.scale[l];
#pragma unroll
        for (int m = 0; m < IRSM_MAX_ANT; m++) {
            if ((uint32_t)m < M) {
                float2 v = acc[m];
#pragma unroll
                for (int x = 32; x >= 1; x >>= 1) {             // symmetric: every lane ends with the same bits
                    const float ox = __shfl_xor(v.x, x), oy = __shfl_xor(v.y, x);
                    v = make_float2(v.x + ox, v.y + oy);
                }
                const float2 h = ch_add(irsm_direct(a, m, r, l, key), v);
                if (lane == 0) sc.taps_out[((uint64_t)m * sc.n_sets + r) * L + l] = make_float2(h.x * s, h.y * s);
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------

#define SWM_WAVES     4
#define SWM_CHUNK     64                  // elements per chunk: 128 floats of the chain, 32 steps of 4
#define SWM_RS        (2 * SWM_CHUNK + 4) // LDS row stride in floats (wr_irs_sweep.hip: 64 different banks per A read)
#define SWM_MAX_CODES 1024
#define SWM_NO_SET    0xFFFFFFFFu

typedef float f4 __attribute__((ext_vector_type(4)));

// MT: a set has more than 16 rows and is walked in row tiles; without it the kernel is wr_irs_sweep.hip's with rows (m, l)
template <int NG, bool MT>
__global__ __launch_bounds__(64 * SWM_WAVES)
void irs_sweep_multi_kernel(const IrsSweepMultiArgs a)
{
    __shared__ float    tile[16 * SWM_RS];
    __shared__ float    q_s[SWM_WAVES][16][17];
    __shared__ float    cand_top[SWM_WAVES][16][16];
    __shared__ uint32_t cand_best[SWM_WAVES][16][16];
    __shared__ float2   row_hd[16];
    __shared__ float    row_scale[16];
    __shared__ uint32_t row_set[16], row_tap[16], row_ant[16], set_best[16];
    // MT: every entry's power over the tiles so far, read and written by the one lane (kk = 0) that owns the entry in the
    // metric step; in LDS so that the NG values are not live across the chunk loop beside the accumulators
    __shared__ float    pw_s[MT ? SWM_WAVES * NG * 16 : 1];

    const IrsMultiArgs& mu = a.m;
    const IrsArgs& sc = mu.s;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t col = lane & 15, kk = lane >> 4;             // MFMA: A[row = col][k = kk], B[k = kk][col], D[row 4 kk + j][col]
    const uint32_t N = sc.n_elems, L = sc.n_taps, K = a.n_codes, M = mu.n_ant;
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
        const uint32_t k = (uint32_t)(i * SWM_WAVES + wave) * 16 + col;
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
            const bool used = g < G && set0 + g < sc.n_sets && rho < R;
            const uint32_t m = used ? rho / L : 0, l = used ? rho - m * L : 0;
            const uint32_t r = used ? (uint32_t)(set0 + g) : SWM_NO_SET;
            row_set[tid] = r;
            row_tap[tid] = l;
            row_ant[tid] = m;
            row_hd[tid] = used ? irsm_direct(mu, m, r, l, key) : make_float2(0.0f, 0.0f);
            row_scale[tid] = used ? sc.scale[l] : 0.0f;
        }
        __syncthreads();
    };
    // the products of the chunk at n0 into the LDS tile: lane t forms element n0 + (t & 63) of the rows (t >> 6) + 4 j
    const auto form = [&](uint32_t n0) {
        const uint32_t n = n0 + lane;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const uint32_t row = wave + 4 * j, r = row_set[row];
            float2 e = make_float2(0.0f, 0.0f);                 // no such row or element: the chain's zero terms
            if (r != SWM_NO_SET && n < N) {
                const IrsElem el = irsm_elem(mu, row_ant[row], r, row_tap[row], n, key);
                e = ch_mul(el.a, el.b);
            }
            *reinterpret_cast<float2*>(&tile[row * SWM_RS + 2 * lane]) = e;
        }
        __syncthreads();
    };

    for (uint32_t rt = 0; rt < T; rt++) {
        const uint32_t rows_here = MT ? min(16u, R - 16 * rt) : R;          // rows of one set in this tile
        set_tile(rt);
#pragma unroll
        for (int i = 0; i < NG; i++) acc_re[i] = acc_im[i] = f4{0.0f, 0.0f, 0.0f, 0.0f};

        for (uint32_t n0 = 0; n0 < N; n0 += SWM_CHUNK) {
            form(n0);
            const uint32_t left = N - n0;
            const uint32_t steps = left >= SWM_CHUNK ? SWM_CHUNK / 2 : (left + 1) / 2;    // 2 N filled up to a multiple of 4, no further
            const float* arow = &tile[col * SWM_RS + kk];
            for (uint32_t s = 0; s < steps; s++) {
                const float av = arow[4 * s];
                const uint32_t n = n0 + 2 * s + half;
                const bool in = n < N;
#pragma unroll
                for (int i = 0; i < NG; i++) {
                    if ((uint32_t)(i * SWM_WAVES + wave) * 16 < K) {                      // the same in every lane of the wave
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
            const uint32_t k = (uint32_t)(i * SWM_WAVES + wave) * 16 + col;
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
                const uint32_t g = kk + 4 * t;                  // lane (g, col): the set's rows in ascending rho
                if (g < G && row_set[g * rows_here] != SWM_NO_SET && k < K) {
                    float p = q_s[wave][g * rows_here][col];
                    if constexpr (MT) {
                        if (rt > 0) p = pw_s[(wave * NG + i) * 16 + col] + p;       // (G = 1: only g = 0, kk = 0 comes here)
                    }
                    for (uint32_t j = 1; j < rows_here; j++) p = p + q_s[wave][g * rows_here + j][col];
                    if constexpr (MT) pw_s[(wave * NG + i) * 16 + col] = p;
                    if (last) {
                        if (a.power_out) a.power_out[(uint64_t)row_set[g * rows_here] * K + k] = p;
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
        for (uint32_t w = 0; w < SWM_WAVES; w++)
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
            const uint32_t k = (uint32_t)(i * SWM_WAVES + wave) * 16 + col;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const uint32_t row = 4 * kk + j, r = row_set[row];
                if (r == SWM_NO_SET || k >= K || set_best[row / R] != k) continue;
                const float2 h = ch_add(row_hd[row], make_float2(acc_re[i][j], acc_im[i][j]));
                const float s = row_scale[row];
                sc.taps_out[((uint64_t)row_ant[row] * sc.n_sets + r) * L + row_tap[row]] = make_float2(h.x * s, h.y * s);
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
            for (uint32_t n0 = 0; n0 < N; n0 += SWM_CHUNK) {
                form(n0);
                if (tid < rows_here) {
                    const uint32_t cnt = min((uint32_t)SWM_CHUNK, N - n0);
                    for (uint32_t s = 0; s < cnt; s++) {
                        const float2 e = *reinterpret_cast<const float2*>(&tile[tid * SWM_RS + 2 * s]), p = c[n0 + s];
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
                const float2 h = ch_add(row_hd[tid], make_float2(re, im));
                const float sl = row_scale[tid];
                sc.taps_out[((uint64_t)row_ant[tid] * sc.n_sets + r) * L + row_tap[tid]] = make_float2(h.x * sl, h.y * sl);
            }
        }
    }
}

}  // namespace wr

static bool irsm_scene_ok(const wr::IrsMultiArgs* a)
{
    const wr::IrsArgs& s = a->s;
    return s.n_elems >= 1 && s.n_elems <= IRS_MAX_ELEMS && s.n_taps >= 1 && s.n_taps <= IRS_MAX_TAPS && a->n_ant >= 1 &&
           a->n_ant <= IRSM_MAX_ANT && s.n_sets <= 0x7fffffffu && a->los_d && s.n_scatter >= 1;
}

extern "C" hipError_t wr_launch_irs_multi(hipStream_t st, const wr::IrsMultiArgs* args)
{
    if (args->s.n_sets == 0) return hipSuccess;
    if (!irsm_scene_ok(args) || args->s.align_bits > 3 || !args->s.taps_out || (args->s.align_bits == 0 && (!args->s.psi || args->s.n_psi_sets < 1)))
        return hipErrorInvalidValue;                        // (the entry point refuses these first)
    const dim3 grid(args->s.n_sets), block(64 * IRSM_WAVES);
    if (args->s.align_bits) hipLaunchKernelGGL((wr::irs_multi_kernel<true>), grid, block, 0, st, *args);
    else hipLaunchKernelGGL((wr::irs_multi_kernel<false>), grid, block, 0, st, *args);
    return hipGetLastError();
}

extern "C" hipError_t wr_launch_irs_sweep_multi(hipStream_t st, const wr::IrsSweepMultiArgs* args)
{
    const wr::IrsArgs& s = args->m.s;
    if (s.n_sets == 0) return hipSuccess;
    if (!irsm_scene_ok(&args->m) || args->n_codes < 1 || args->n_codes > SWM_MAX_CODES || !args->codebook)
        return hipErrorInvalidValue;                        // (the entry point refuses these first)
    const uint32_t R = args->m.n_ant * s.n_taps, G = R >= 16 ? 1 : 16 / R;
    const dim3 grid((s.n_sets + G - 1) / G), block(64 * SWM_WAVES);
    const uint32_t groups = (args->n_codes + 15) / 16, per_wave = (groups + SWM_WAVES - 1) / SWM_WAVES;
#define SWM_LAUNCH(NG) \
    do { \
        if (R > 16) hipLaunchKernelGGL((wr::irs_sweep_multi_kernel<NG, true>), grid, block, 0, st, *args); \
        else hipLaunchKernelGGL((wr::irs_sweep_multi_kernel<NG, false>), grid, block, 0, st, *args); \
    } while (0)
    if (per_wave <= 1) SWM_LAUNCH(1);
    else if (per_wave <= 2) SWM_LAUNCH(2);
    else if (per_wave <= 4) SWM_LAUNCH(4);
    else if (per_wave <= 8) SWM_LAUNCH(8);
    else SWM_LAUNCH(16);
#undef SWM_LAUNCH
    return hipGetLastError();
}

extern "C" uint32_t wr_irs_max_ant(void) { return IRSM_MAX_ANT; }
