// wr_spectrum.hip -- the band survey of NUMERICS.md rule 36: windowed-FFT power rows of a stream in its native format, the
// fold of rows, and the band powers of rows.  The integer formats of rule 20 are widened on the way into the first butterfly,
// so a capture never exists as float32 in memory.
//
// spectrum_kernel: a workgroup of 256 lanes owns a tile of max(1024, N) points: 1024 / N rows side by side with N / 4 lanes per
// row, or for N = 4096 one row with four butterflies per lane and stage.  A lane holds one radix-4 butterfly of a stage.  The
// first stage reads its four samples straight from the capture (samples n, n + N/4, n + N/2, n + 3N/4 of the segment: the lanes
// of a row read neighbours), windows them and writes LDS; the middle stages work in place in LDS, a barrier between stages; the
// last stage (span 1) ends in registers, where the four powers are folded into the lane's accumulators.  Those sit at the
// digit-reversed positions 4 j + q for all of a row's avg segments; the permutation to centred natural order is done once
// per row, through LDS, so that the row leaves in whole lines.  LDS: 8 kB per tile, 32 kB at N = 4096.  The twiddles and the
// windows are read from their 4096-entry tables through the cache (32 kB and 2 x 16 kB; a stage touches every (1024 / span)-th entry).
//
// fold_kernel and bands_kernel are streaming kernels: one lane per output value, and one wave per (row, band).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wr_iq.h"
#include "wr_spectrum.h"
#include "wr_spectrum_table.h"

namespace wr {

namespace {

static_assert(WR_SPEC_ENTRIES == 4096 && WR_SPEC_TABLE_ENTRIES == WR_SPEC_ENTRIES && WR_SPEC_TILE == 4 * WR_SPEC_LANES, "table and tile geometry");

const float spec_host_twiddle[2 * WR_SPEC_ENTRIES] = WR_SPEC_TWIDDLE_INIT;
const float spec_host_hann[WR_SPEC_ENTRIES] = WR_SPEC_HANN_INIT;
const float spec_host_bh[WR_SPEC_ENTRIES] = WR_SPEC_BLACKMAN_HARRIS_INIT;
__device__ const float __attribute__((aligned(8))) spec_dev_twiddle[2 * WR_SPEC_ENTRIES] = WR_SPEC_TWIDDLE_INIT;
__device__ const float spec_dev_hann[WR_SPEC_ENTRIES] = WR_SPEC_HANN_INIT;
__device__ const float spec_dev_bh[WR_SPEC_ENTRIES] = WR_SPEC_BLACKMAN_HARRIS_INIT;

constexpr uint32_t log2_of(uint32_t n) { return n <= 1 ? 0 : 1 + log2_of(n >> 1); }

// rule 17's product with the table value first: c v
__device__ __forceinline__ float2 spec_mul(float2 c, float2 v)
{
    return make_float2(c.x * v.x - c.y * v.y, c.x * v.y + c.y * v.x);
}

// rule 4's butterfly on (a, b, c, d), then output q times T[q * step] for q = 1 .. 3 unless step == 0 (exponent 0: no multiply)
__device__ __forceinline__ void spec_bfly(float2& a, float2& b, float2& c, float2& d, uint32_t step)
{
    const float2 t0 = make_float2(a.x + c.x, a.y + c.y), t1 = make_float2(a.x - c.x, a.y - c.y);
    const float2 t2 = make_float2(b.x + d.x, b.y + d.y), t3 = make_float2(b.x - d.x, b.y - d.y);
    a = make_float2(t0.x + t2.x, t0.y + t2.y);
    b = make_float2(t1.x + t3.y, t1.y - t3.x);                // t1 - j t3
    c = make_float2(t0.x - t2.x, t0.y - t2.y);
    d = make_float2(t1.x - t3.y, t1.y + t3.x);                // t1 + j t3
    if (step) {
        const float2* T = reinterpret_cast<const float2*>(spec_dev_twiddle);
        b = spec_mul(T[step], b);
        c = spec_mul(T[2 * step], c);
        d = spec_mul(T[3 * step], d);
    }
}

// the fold of rule 36: the first value starts it
__device__ __forceinline__ float spec_fold(float a, float p, bool first, int mode)
{
    if (first) return p;
    if (mode == WIFIRX_SPEC_MAX) return (p > a || p != p) ? p : a;
    return a + p;
}

template <int FMT, uint32_t N>
__global__ __launch_bounds__(WR_SPEC_LANES)
void spectrum_kernel(const void* __restrict__ in, float scale, uint32_t hop, uint32_t avg, int window, int mode, float norm,
                     float* __restrict__ out, uint64_t n_rows)
{
    const float* win = window == WIFIRX_SPEC_HANN ? spec_dev_hann : window == WIFIRX_SPEC_BLACKMAN_HARRIS ? spec_dev_bh : nullptr;
    constexpr uint32_t P = N > WR_SPEC_TILE ? N : WR_SPEC_TILE;       // points of the tile
    constexpr uint32_t ROWS = P / N;                                  // rows of the tile
    constexpr uint32_t B = P / (4 * WR_SPEC_LANES);                   // butterflies of a lane per stage
    constexpr uint32_t Q = N / 4, LOGQ = log2_of(Q), LOGN = LOGQ + 2; // butterflies of a row per stage
    constexpr uint32_t TS = WR_SPEC_ENTRIES / N;                      // table stride of this N
    static_assert((LOGN & 1) == 0 && N >= 64 && N <= WR_SPEC_ENTRIES, "N is a power of 4");
    __shared__ __attribute__((aligned(16))) float2 buf[P];

    const uint32_t tid = threadIdx.x;
    const uint64_t row0 = (uint64_t)blockIdx.x * ROWS;                // the tile's first row
    float acc[B][4];
#pragma unroll
    for (uint32_t b = 0; b < B; b++) acc[b][0] = acc[b][1] = acc[b][2] = acc[b][3] = 0.f;

    for (uint32_t s = 0; s < avg; s++) {
        // first stage, span N / 4, from the capture: window, butterfly, twiddle W_N^(q n)
#pragma unroll
        for (uint32_t b = 0; b < B; b++) {
            const uint32_t g = tid + b * WR_SPEC_LANES, rt = g >> LOGQ, n = g & (Q - 1);
            const uint64_t row = row0 + rt;
            float2 x[4];
#pragma unroll
            for (uint32_t q = 0; q < 4; q++) {
                x[q] = make_float2(0.f, 0.f);
                if (row < n_rows) {
                    x[q] = load_sample<FMT>(in, (row * avg + s) * hop + n + q * Q, scale);
                    if (win) {
                        const float w = win[(n + q * Q) * TS];
                        x[q] = make_float2(w * x[q].x, w * x[q].y);
                    }
                }
            }
            spec_bfly(x[0], x[1], x[2], x[3], n * TS);
            float2* p = buf + rt * N + n;
#pragma unroll
            for (uint32_t q = 0; q < 4; q++) p[q * Q] = x[q];
        }
        __syncthreads();
        // middle stages, spans N / 16 .. 4, in place
#pragma unroll
        for (uint32_t lg = LOGQ - 2; lg >= 2; lg -= 2) {
            const uint32_t L = 1u << lg;
#pragma unroll
            for (uint32_t b = 0; b < B; b++) {
                const uint32_t g = tid + b * WR_SPEC_LANES, rt = g >> LOGQ, j = g & (Q - 1);
                const uint32_t n = j & (L - 1);
                float2* p = buf + rt * N + ((j >> lg) << (lg + 2)) + n;
                float2 a = p[0], bb = p[L], c = p[2 * L], d = p[3 * L];
                spec_bfly(a, bb, c, d, n * (WR_SPEC_ENTRIES / 4 >> lg));
                p[0] = a; p[L] = bb; p[2 * L] = c; p[3 * L] = d;
            }
            __syncthreads();
        }
        // last stage, span 1: no twiddle; the powers are folded where they stand
#pragma unroll
        for (uint32_t b = 0; b < B; b++) {
            const uint32_t g = tid + b * WR_SPEC_LANES;               // rt * Q + j: its points are buf[4 g .. 4 g + 3]
            const float2* p = buf + 4 * g;
            float2 y[4] = { p[0], p[1], p[2], p[3] };
            spec_bfly(y[0], y[1], y[2], y[3], 0);
#pragma unroll
            for (uint32_t q = 0; q < 4; q++) acc[b][q] = spec_fold(acc[b][q], y[q].x * y[q].x + y[q].y * y[q].y, s == 0, mode);
        }
        __syncthreads();                                              // the next segment's first stage overwrites buf
    }

    // position 4 j + q holds frequency digitrev(4 j + q); bin = frequency + N / 2 mod N; times norm; out in whole lines
    float* pb = reinterpret_cast<float*>(buf);
#pragma unroll
    for (uint32_t b = 0; b < B; b++) {
        const uint32_t g = tid + b * WR_SPEC_LANES, rt = g >> LOGQ, j = g & (Q - 1);
#pragma unroll
        for (uint32_t q = 0; q < 4; q++) {
            uint32_t i = 4 * j + q, k = 0;
#pragma unroll
            for (uint32_t d = 0; d < LOGN; d += 2) { k = (k << 2) | (i & 3); i >>= 2; }
            pb[rt * N + ((k + N / 2) & (N - 1))] = acc[b][q] * norm;
        }
    }
    __syncthreads();
    float* o = out + row0 * N;
    for (uint32_t i = tid; i < P; i += WR_SPEC_LANES)
        if (row0 + (i >> LOGN) < n_rows) o[i] = pb[i];
}

// out[q][bin] = the ascending fold of rows[q * group + g][bin], g < group; one lane per output value
__global__ __launch_bounds__(WR_SPEC_LANES)
void spectrum_fold_kernel(const float* __restrict__ rows, uint32_t log_n, uint64_t group, int mode, float* __restrict__ out,
                          uint64_t n_values)
{
    const uint64_t idx = (uint64_t)blockIdx.x * WR_SPEC_LANES + threadIdx.x;
    if (idx >= n_values) return;
    const uint64_t q = idx >> log_n, bin = idx & ((1ull << log_n) - 1);
    const float* p = rows + ((q * group) << log_n) + bin;
    float a = p[0];
    for (uint64_t g = 1; g < group; g++) a = spec_fold(a, p[g << log_n], false, mode);
    out[idx] = a;
}

// one wave per (row, band): lane l adds bins lo + l, lo + l + 64, .. below hi in ascending order from its first bin's value
// (+0 without a bin), then rule 5's xor tree over the 64 lanes in its order: lane xor 1, 2, 4, 8, 16, 32
__global__ __launch_bounds__(64)
void spectrum_bands_kernel(const float* __restrict__ rows, uint32_t n_fft, uint32_t n_bands, wr_spec_bands bands,
                           float* __restrict__ out)
{
    const uint32_t band = blockIdx.y, lane = threadIdx.x;
    const uint64_t row = blockIdx.x;
    const float* p = rows + row * n_fft;
    const uint32_t lo = bands.lo[band], hi = bands.hi[band];
    float v = 0.f;
    uint32_t i = lo + lane;
    if (i < hi) {
        v = p[i];
        for (i += 64; i < hi; i += 64) v = v + p[i];
    }
#pragma unroll
    for (int m = 1; m <= 32; m <<= 1) v = v + __shfl_xor(v, m, 64);
    if (lane == 0) out[row * n_bands + band] = v;
}

template <int FMT>
bool launch_n(uint32_t n_fft, dim3 grid, hipStream_t st, const void* in, float scale, uint32_t hop, uint32_t avg, int win,
              int mode, float norm, float* out, uint64_t n_rows)
{
    const dim3 block(WR_SPEC_LANES);
    switch (n_fft) {
    case 64: hipLaunchKernelGGL((spectrum_kernel<FMT, 64>), grid, block, 0, st, in, scale, hop, avg, win, mode, norm, out, n_rows); return true;
    case 256: hipLaunchKernelGGL((spectrum_kernel<FMT, 256>), grid, block, 0, st, in, scale, hop, avg, win, mode, norm, out, n_rows); return true;
    case 1024: hipLaunchKernelGGL((spectrum_kernel<FMT, 1024>), grid, block, 0, st, in, scale, hop, avg, win, mode, norm, out, n_rows); return true;
    case 4096: hipLaunchKernelGGL((spectrum_kernel<FMT, 4096>), grid, block, 0, st, in, scale, hop, avg, win, mode, norm, out, n_rows); return true;
    }
    return false;
}

}  // namespace

}  // namespace wr

extern "C" hipError_t wr_launch_spectrum(hipStream_t st, const void* in, int fmt, float scale, uint32_t n_fft, uint32_t hop,
                                         uint32_t avg, int window, int mode, float norm, float* rows_out, uint64_t n_rows)
{
    if (n_rows == 0) return hipSuccess;
    if (n_fft != 64 && n_fft != 256 && n_fft != 1024 && n_fft != 4096) return hipErrorInvalidValue;
    if (hop < 1 || avg < 1 || (mode != WIFIRX_SPEC_SUM && mode != WIFIRX_SPEC_MAX)) return hipErrorInvalidValue;
    if (window != WIFIRX_SPEC_RECT && window != WIFIRX_SPEC_HANN && window != WIFIRX_SPEC_BLACKMAN_HARRIS) return hipErrorInvalidValue;
    const uint64_t rows_per_tile = n_fft >= WR_SPEC_TILE ? 1 : WR_SPEC_TILE / n_fft;
    const uint64_t tiles = (n_rows + rows_per_tile - 1) / rows_per_tile;
    if (tiles > 0x7fffffffull) return hipErrorInvalidValue;
    const dim3 grid((uint32_t)tiles);
    bool known_n = false;
    const bool known = wr::iq_dispatch(fmt, [&](auto F) {
        known_n = wr::launch_n<decltype(F)::value>(n_fft, grid, st, in, scale, hop, avg, window, mode, norm, rows_out, n_rows);
    });
    return known && known_n ? hipGetLastError() : hipErrorInvalidValue;
}

extern "C" hipError_t wr_launch_spectrum_fold(hipStream_t st, const float* rows, uint32_t n_fft, uint64_t group, int mode,
                                              float* out, uint64_t n_out)
{
    if (n_out == 0) return hipSuccess;
    if (n_fft != 64 && n_fft != 256 && n_fft != 1024 && n_fft != 4096) return hipErrorInvalidValue;
    const uint32_t log_n = wr::log2_of(n_fft);
    const uint64_t values = n_out << log_n, blocks = (values + WR_SPEC_LANES - 1) / WR_SPEC_LANES;
    if (group < 1 || blocks > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(wr::spectrum_fold_kernel, dim3((uint32_t)blocks), dim3(WR_SPEC_LANES), 0, st, rows, log_n, group, mode, out, values);
    return hipGetLastError();
}

extern "C" hipError_t wr_launch_spectrum_bands(hipStream_t st, const float* rows, uint64_t n_rows, uint32_t n_fft, uint32_t n_bands,
                                               const wr_spec_bands* b, float* out)
{
    if (n_rows == 0) return hipSuccess;
    if (n_bands < 1 || n_bands > WIFIRX_SPEC_MAX_BANDS || n_rows > 0x7fffffffull) return hipErrorInvalidValue;
    for (uint32_t k = 0; k < n_bands; k++)
        if (b->lo[k] >= b->hi[k] || b->hi[k] > n_fft) return hipErrorInvalidValue;
    hipLaunchKernelGGL(wr::spectrum_bands_kernel, dim3((uint32_t)n_rows, n_bands), dim3(64), 0, st, rows, n_fft, n_bands, *b, out);
    return hipGetLastError();
}

extern "C" const float* wr_spectrum_host_hann(void) { return wr::spec_host_hann; }
extern "C" const float* wr_spectrum_host_blackman_harris(void) { return wr::spec_host_bh; }
extern "C" const float* wr_spectrum_host_twiddle(void) { return wr::spec_host_twiddle; }
