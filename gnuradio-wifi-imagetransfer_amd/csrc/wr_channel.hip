// wr_channel.hip -- GNU Radio's channels.channel_model on the device (the block between TX and RX of the reference's
// loop-back, gnu_radio/IRS_tranceiver.py:282-288): per row, the multipath FIR, then the frequency-offset mixer, then the
// noise adder, in the float32 arithmetic of NUMERICS.md rule 17.
//
// Work split (the shape of wr_tx.hip): the output of every row is cut into tiles of CH_TILE consecutive samples on
// pair-aligned indices; one workgroup owns one tile.  channel_kernel, in this order:
//   place    ch_place: the tile's row and its place in it, for fixed rows and for row_off rows;
//   stage    with more than one tap, the tile's input and the n_taps - 1 samples before it (zeros before the row start: every
//            row is its own burst) into the LDS array xs.  With a sample-rate offset (wifirx_channel_sro, NUMERICS.md rule 18)
//            the raw input window (the tile, the FIR halo, the resampler's 31 neighbours, the drift spread over the tile) and
//            the table go into LDS, and xs takes the resampled samples u of the tile and its FIR halo;
//   fade     with Doppler fading (wifirx_channel_fading, rule 19) the row's oscillators (8 per tap and the line-of-sight one: a
//            Philox draw, one sp_sincos and one double product each), set up in front of the staging, and behind it the gains
//            of every tap on the 32-sample grid of the stream time that covers the tile, in LDS;
//   FIR      every lane forms CH_TILE / 512 pairs of consecutive samples in one loop over xs, whose coefficient (ch_coef) is
//            the tap or, with fading, the tap times the gain interpolated between two grid points; one tap reads its pair
//            from global memory instead;
//   mix, noise, store   the phase is fixed point (a uint64 in 2^-64 turns: exact for any row length), the noise is
//            wr_synth.hip's Philox4x32-10 + Box-Muller on the counter (pair index of the sample, row), one 16-byte store a pair.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wr_device.h"     // sp_sincos (rule 1), sp_sincos_phase (rule 17)
#include "wr_rng.h"        // philox4x32_10, u01, ch_noise
#include "wr_channel.h"    // ch_mul, ch_add
#include "wr_resample_table.h"

namespace wr {

#define CH_TILE     2048     // samples per workgroup: four pairs per lane of a 256-lane group
#define CH_MAX_TAPS 64
#define CH_FADE_TAPS 16      // the most taps with fading: the grid gains of 64 would leave one workgroup per CU
#define CH_FADE_SINES 8      // sinusoids per tap
#define CH_FADE_STEP 32      // samples between two grid points of the gains: a power of two
#define CH_FADE_GRID (CH_TILE / CH_FADE_STEP + 2)      // grid points a tile touches: it may start anywhere between two
#define CH_FADE_LOS  (CH_FADE_TAPS * CH_FADE_SINES)    // counter index (and slot) of tap 0's line-of-sight oscillator
// raw input window of a resampling tile: the CH_TILE + CH_MAX_TAPS - 1 outputs u it forms read input positions that spread
// over at most that many samples plus ceil((CH_TILE + CH_MAX_TAPS - 2) / 256) = 9 of drift (|sro| <= 2^-8), plus the
// resampler's WR_RS_TAPS - 1 neighbours
#define CH_RAW      (CH_TILE + CH_MAX_TAPS - 1 + 9 + WR_RS_TAPS - 1)

__device__ const float rs_table[(WR_RS_PHASES + 1) * WR_RS_TAPS] = WR_RS_TABLE_INIT;

// sample n of the row after the FIR: gain * (s * exp(j phi(n)))
__device__ __forceinline__ float2 ch_rotate(float2 s, uint64_t P, float gain)
{
    float sn, cs;
    sp_sincos_phase((uint32_t)(P >> 32), sn, cs);
    const float2 y = ch_mul(s, make_float2(cs, sn));
    return make_float2(gain * y.x, gain * y.y);
}

// rad/sample -> phase increment in 2^-64 turns: llround(cfo / (2 pi) * 2^64) as a uint64, the turns reduced to [-1/2, 1/2]
// first (exact), so that any finite cfo has one (+-1/2 turn = 2^63).  IEEE double, once per workgroup.
__device__ __forceinline__ uint64_t ch_phase_inc(float cfo)
{
    double f = (double)cfo / 6.283185307179586;
    f -= __builtin_rint(f);
    const double v = f * 0x1p64;
    if (v >= 0x1p63 || v <= -0x1p63) return 1ull << 63;
    return (uint64_t)(int64_t)__builtin_round(v);          // round: half away from zero, as llround
}

__device__ __forceinline__ uint4 ch_draw(uint64_t pair, uint32_t row, uint2 key)
{
    return philox4x32_10(make_uint4((uint32_t)pair, row, (uint32_t)(pair >> 32), 0u), key);
}

// rule 19: oscillator with start phase phi and increment inc (2^-64 turns) at stream time t: (cos, sin) of P = phi + inc t
__device__ __forceinline__ float2 fade_osc(uint64_t phi, uint64_t inc, uint64_t t)
{
    float sn, cs;
    sp_sincos_phase((uint32_t)((phi + inc * t) >> 32), sn, cs);
    return make_float2(cs, sn);
}

// rule 19: the gain between the grid points G0 (at or before the sample) and G1 (32 samples later), w = (t & 31) / 32
__device__ __forceinline__ float2 fade_lerp(float2 G0, float2 G1, float w)
{
    return make_float2(G0.x + w * (G1.x - G0.x), G0.y + w * (G1.y - G0.y));
}

// rule 18: output n of a row whose drift is D = drift0 + dinc n (2^-40 samples) reads the input around i = n + (D >> 40)
__device__ __forceinline__ int64_t rs_pos(int64_t n, int64_t D) { return n + (D >> 40); }

struct ChanTile { uint32_t r; uint64_t k; int64_t rs, re; };      // row, tile of the row, row start and end

// the tile's row and its place in it (uniform: scalar loads)
__device__ __forceinline__ ChanTile ch_place(const ChanArgs& a, uint64_t tile)
{
    uint32_t r;
    uint64_t k;
    if (a.row_off) {
        uint32_t lo = 0, hi = a.n_rows;              // the last row whose first tile is <= tile: it has tiles, so it owns it
        while (hi - lo > 1) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (a.tile_base[mid] <= tile) lo = mid; else hi = mid;
        }
        r = lo;
        k = tile - a.tile_base[r];
    } else {
        r = (uint32_t)(tile / a.tiles_per_row);
        k = tile - (uint64_t)r * a.tiles_per_row;
    }
    const int64_t rs = a.row_off ? (int64_t)a.row_off[r] : (int64_t)r * (int64_t)a.row_len;
    const int64_t re = a.row_off ? (int64_t)a.row_off[r + 1] : rs + (int64_t)a.row_len;
    return {r, k, rs, re};
}

// coefficient of tap q: the tap; with FADE the gain interpolated between the grid rows g and g + L, times the tap
template <bool FADE>
__device__ __forceinline__ float2 ch_coef(const float2* tp, const float2* g, float w, uint32_t L, uint32_t q)
{
    if constexpr (FADE) return ch_mul(fade_lerp(g[q], g[L + q], w), tp[q]);
    else return tp[q];
}

// STAGE: the FIR reads its input from LDS (n_taps > 1, SRO or FADE); SRO: that input is the resampled row (rule 18), any
// n_taps; FADE: the taps are multiplied by gains that vary with the stream time (rule 19), n_taps <= CH_FADE_TAPS
template <bool STAGE, bool SRO, bool FADE>
__global__ __launch_bounds__(256)
void channel_kernel(const ChanArgs a)
{
    static_assert(STAGE || !SRO, "the resampler writes the array the FIR reads");
    static_assert(STAGE || !FADE, "the fading FIR reads its input from LDS");
    __shared__ uint64_t osc_phi[FADE ? CH_FADE_LOS + 1 : 1], osc_inc[FADE ? CH_FADE_LOS + 1 : 1];
    __shared__ float2 gg[FADE ? CH_FADE_GRID * CH_FADE_TAPS : 1];      // [grid point][tap], n_taps apart
    __shared__ float2 xs[STAGE ? CH_TILE + CH_MAX_TAPS - 1 : 1];
    __shared__ float2 tp[CH_MAX_TAPS];
    __shared__ float2 raw[SRO ? CH_RAW : 1];
    __shared__ __attribute__((aligned(16))) float tab[SRO ? (WR_RS_PHASES + 1) * WR_RS_TAPS : 1];
    const uint32_t tid = threadIdx.x;
    const ChanTile p = ch_place(a, blockIdx.x);
    const uint32_t r = p.r, L = a.n_taps;
    const int64_t rs = p.rs, re = p.re, gt = (((rs + a.shift) & ~(int64_t)1) - a.shift) + (int64_t)p.k * CH_TILE;

    // ---- stage: the taps, the input window, the gains on the grid ----
    if (tid < L) tp[tid] = a.taps[(size_t)(r % a.n_tap_sets) * L + tid];
    uint64_t q0 = 0;                                   // FADE: stream time of the tile's first grid point
    if constexpr (FADE) {
        q0 = (a.time0 + (uint64_t)(gt - rs)) & ~(uint64_t)(CH_FADE_STEP - 1);
        if (tid < CH_FADE_SINES * L || tid == CH_FADE_LOS) {
            const uint4 d = philox4x32_10(make_uint4(tid, r, 0u, 1u), make_uint2((uint32_t)a.fade_seed, (uint32_t)(a.fade_seed >> 32)));
            float sn, cs;
            sp_sincos_phase(d.x, sn, cs);
            osc_inc[tid] = (uint64_t)(int64_t)__builtin_round((double)a.doppler[r] * (double)cs * 0x1p64);      // |.| <= 2^54
            osc_phi[tid] = ((uint64_t)d.y << 32) | d.z;
        }
    }
    if constexpr (SRO) {
        const int64_t len = re - rs;
        const int64_t dinc = a.dinc[r];
        const int64_t n0 = gt - rs - (int64_t)(L - 1);            // row index of xs[0]; may be negative
        // the outputs this tile forms, [nA, nB], and the input window they read (i is non-decreasing in n)
        const int64_t nA = n0 > 0 ? n0 : 0;
        const int64_t nB = (n0 + CH_TILE + (int64_t)L - 2 < len - 1) ? n0 + CH_TILE + (int64_t)L - 2 : len - 1;
        const int64_t lo = rs_pos(nA, a.drift0 + dinc * nA) - WR_RS_CENTER;
        int64_t W = rs_pos(nB, a.drift0 + dinc * nB) + (WR_RS_TAPS - WR_RS_CENTER) - lo;      // nB < nA: nothing to form
        if (W > CH_RAW) W = CH_RAW;                               // (cannot bind: see CH_RAW)
        for (uint32_t i = tid; i < (WR_RS_PHASES + 1) * WR_RS_TAPS; i += 256) tab[i] = rs_table[i];
        for (int64_t i = tid; i < W; i += 256) {
            const int64_t m = lo + i;
            raw[i] = (m >= 0 && m < len) ? a.in[rs + m] : make_float2(0.0f, 0.0f);
        }
        __syncthreads();
        for (uint32_t t = tid; t < CH_TILE + L - 1; t += 256) {
            const int64_t n = n0 + (int64_t)t;
            float2 u = make_float2(0.0f, 0.0f);
            if (n >= 0 && n < len) {
                const int64_t D = a.drift0 + dinc * n;
                const uint64_t mu = (uint64_t)D & ((1ull << 40) - 1);
                const float frac = (float)(uint32_t)((mu >> 9) & 0xFFFFFFu) * 0x1p-24f;
                const float* t0 = tab + (uint32_t)(mu >> 33) * WR_RS_TAPS;
                const float2* x = raw + (rs_pos(n, D) - WR_RS_CENTER - lo);
#pragma unroll
                for (int q = 0; q < WR_RS_TAPS; q++) {
                    const float c = t0[q] + frac * (t0[WR_RS_TAPS + q] - t0[q]);
                    const float2 v = x[q];
                    u = q == 0 ? make_float2(c * v.x, c * v.y) : make_float2(u.x + c * v.x, u.y + c * v.y);
                }
            }
            xs[t] = u;
        }
    } else if constexpr (STAGE) {
        const int64_t s0 = gt - (int64_t)(L - 1);
        for (uint32_t i = tid; i < CH_TILE + L - 1; i += 256) {
            const int64_t g = s0 + (int64_t)i;
            xs[i] = (g >= rs && g < re) ? a.in[g] : make_float2(0.0f, 0.0f);
        }
    }
    if constexpr (FADE) {
        __syncthreads();                               // the oscillators
        const bool los = a.a_los != 0.0f;                  // k_factor > 0
        for (uint32_t e = tid; e < CH_FADE_GRID * L; e += 256) {
            const uint32_t i = e / L, l = e - i * L;
            const uint64_t t = q0 + (uint64_t)i * CH_FADE_STEP;
            float2 G = fade_osc(osc_phi[CH_FADE_SINES * l], osc_inc[CH_FADE_SINES * l], t);
#pragma unroll
            for (uint32_t k = 1; k < CH_FADE_SINES; k++)
                G = ch_add(G, fade_osc(osc_phi[CH_FADE_SINES * l + k], osc_inc[CH_FADE_SINES * l + k], t));
            G = make_float2(0.35355339f * G.x, 0.35355339f * G.y);
            if (los && l == 0) {
                const float2 o = fade_osc(osc_phi[CH_FADE_LOS], osc_inc[CH_FADE_LOS], t);
                G = make_float2(a.a_los * o.x + a.a_nlos * G.x, a.a_los * o.y + a.a_nlos * G.y);
            }
            gg[e] = G;
        }
    }
    __syncthreads();

    // ---- per pair of samples: FIR, mixer, noise, store ----
    const uint64_t inc = a.cfo ? ch_phase_inc(a.cfo[r]) : 0;
    const uint2 key = make_uint2((uint32_t)a.seed, (uint32_t)(a.seed >> 32));
    const float h = 0.70710678118654752f * a.noise;
    float4* out4 = reinterpret_cast<float4*>(a.out - a.shift);
#pragma unroll
    for (int u = 0; u < CH_TILE / 512; u++) {
        const int32_t j = 2 * (256 * u + (int32_t)tid);           // tile offset of the lane's first sample
        const int64_t g = gt + j;
        const bool in0 = g >= rs && g < re, in1 = g + 1 >= rs && g + 1 < re;
        if (!in0 && !in1) continue;

        float2 s0, s1;
        if constexpr (STAGE) {
            // the gains of both samples at their own output times t and t + 1, for every tap
            const uint64_t t0 = a.time0 + (uint64_t)(g - rs), t1 = t0 + 1;
            const float2* g0 = gg + (FADE ? (uint32_t)((t0 - q0) / CH_FADE_STEP) * L : 0);
            const float2* g1 = gg + (FADE ? (uint32_t)((t1 - q0) / CH_FADE_STEP) * L : 0);
            const float w0 = (float)(uint32_t)(t0 & (CH_FADE_STEP - 1)) * (1.0f / CH_FADE_STEP);
            const float w1 = (float)(uint32_t)(t1 & (CH_FADE_STEP - 1)) * (1.0f / CH_FADE_STEP);
            const int32_t b = j + (int32_t)L - 1;                  // xs index of the input at g
            float2 prev = xs[b + 1];
            float2 cur = xs[b];
            s0 = ch_mul(ch_coef<FADE>(tp, g0, w0, L, 0), cur);
            s1 = ch_mul(ch_coef<FADE>(tp, g1, w1, L, 0), prev);
            for (uint32_t q = 1; q < L; q++) {
                prev = cur;
                cur = xs[b - (int32_t)q];
                s0 = ch_add(s0, ch_mul(ch_coef<FADE>(tp, g0, w0, L, q), cur));
                s1 = ch_add(s1, ch_mul(ch_coef<FADE>(tp, g1, w1, L, q), prev));
            }
        } else {
            float2 x0 = make_float2(0.0f, 0.0f), x1 = x0;
            if (in0 && in1 && ((reinterpret_cast<uintptr_t>(a.in + g) & 15) == 0)) {
                const float4 v = *reinterpret_cast<const float4*>(a.in + g);
                x0 = make_float2(v.x, v.y);
                x1 = make_float2(v.z, v.w);
            } else {
                if (in0) x0 = a.in[g];
                if (in1) x1 = a.in[g + 1];
            }
            s0 = ch_mul(tp[0], x0);
            s1 = ch_mul(tp[0], x1);
        }

        // mixer: P(n) = phase0 + inc n mod 2^64, n = sample index in the row
        const uint64_t n0 = (uint64_t)(g - rs);
        const uint64_t P0 = a.phase0 + inc * n0;
        float2 y0 = ch_rotate(s0, P0, a.gain);
        float2 y1 = ch_rotate(s1, P0 + inc, a.gain);
        if (a.noise != 0.0f) {                                     // not 0 * w: a Box-Muller radius of inf would give NaN
            const uint64_t m0 = a.sample0 + n0, m1 = m0 + 1;
            const bool odd = (m0 & 1) != 0;                        // the same in every lane of the tile
            const uint4 d0 = ch_draw(m0 >> 1, r, key);
            const uint4 d1 = odd ? ch_draw(m1 >> 1, r, key) : d0;
            y0 = ch_add(y0, ch_noise(odd ? d0.z : d0.x, odd ? d0.w : d0.y, h));
            y1 = ch_add(y1, ch_noise(odd ? d1.x : d0.z, odd ? d1.y : d0.w, h));
        }

        if (in0 && in1) out4[(g + a.shift) >> 1] = make_float4(y0.x, y0.y, y1.x, y1.y);
        else if (in0) a.out[g] = y0;
        else a.out[g + 1] = y1;
    }
}

}  // namespace wr

extern "C" hipError_t wr_launch_channel(hipStream_t st, const wr::ChanArgs* args, uint64_t n_tiles)
{
    if (n_tiles == 0) return hipSuccess;
    const dim3 grid((unsigned)n_tiles), block(256);
    if (args->doppler && args->n_taps > CH_FADE_TAPS) return hipErrorInvalidValue;      // (the entry point refuses it first)
    if (args->doppler && args->dinc) hipLaunchKernelGGL((wr::channel_kernel<true, true, true>), grid, block, 0, st, *args);
    else if (args->doppler) hipLaunchKernelGGL((wr::channel_kernel<true, false, true>), grid, block, 0, st, *args);
    else if (args->dinc) hipLaunchKernelGGL((wr::channel_kernel<true, true, false>), grid, block, 0, st, *args);
    else if (args->n_taps > 1) hipLaunchKernelGGL((wr::channel_kernel<true, false, false>), grid, block, 0, st, *args);
    else hipLaunchKernelGGL((wr::channel_kernel<false, false, false>), grid, block, 0, st, *args);
    return hipGetLastError();
}

extern "C" uint32_t wr_channel_tile_samples(void) { return CH_TILE; }
extern "C" uint32_t wr_channel_fade_taps(void) { return CH_FADE_TAPS; }

extern "C" const float* wr_resample_table(uint32_t* n_phases, uint32_t* n_taps)
{
    static const float table[(WR_RS_PHASES + 1) * WR_RS_TAPS] = WR_RS_TABLE_INIT;
    *n_phases = WR_RS_PHASES;
    *n_taps = WR_RS_TAPS;
    return table;
}
