// wr_channelizer.hip -- the analysis bank of NUMERICS.md rule 21: one wideband stream of M adjacent 20 MHz channels, sampled
// at M fs, into M streams at fs.  A polyphase filter (24 taps per branch) and an M-point DFT per output; the integer formats
// of rule 20 are widened on the way into LDS, so the wideband capture is never written out as float32.
//
// One workgroup produces a tile of WR_CZ_TILE outputs per channel.  It stages the tile's WR_CZ_TILE * M input samples and the
// 23 * M in front of them in LDS, de-interleaved into M planes [q][block], so that a branch's reads are unit stride across
// the lanes.  A lane produces two adjacent outputs: their 24-tap windows share 23 of 25 blocks, which it reads as twelve
// 16-byte pieces and one 8-byte piece per branch, and it stores the two outputs of a channel as one 16-byte piece.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wr_channelizer.h"
#include "wr_bank.h"
#include "wr_iq.h"

namespace wr {

namespace {

static_assert(WR_CZ_TILE == BANK_TILE && WR_CZ_HIST == BANK_HIST && WR_CZ_HIST * 8 <= BANK_THREADS, "tile geometry");

// the host copy of the taps behind wr_channelizer_taps
const float cz_host_taps2[BANK_P * 2] = WR_CZ_TAPS2_INIT;
const float cz_host_taps4[BANK_P * 4] = WR_CZ_TAPS4_INIT;
const float cz_host_taps8[BANK_P * 8] = WR_CZ_TAPS8_INIT;

// sample e of a piece, widened by rule 20
template <int FMT>
__device__ __forceinline__ float2 piece_sample(const uint32_t (&w)[4], uint32_t e, float scale)
{
    if constexpr (FMT == WIFIRX_IQ_FC32) {
        return make_float2(__uint_as_float(w[2 * e]), __uint_as_float(w[2 * e + 1]));
    } else if constexpr (FMT == WIFIRX_IQ_SC16) {
        return make_float2((float)(int16_t)(w[e] & 0xffffu) * scale, (float)(int16_t)(w[e] >> 16) * scale);
    } else {
        const uint32_t h = (w[e >> 1] >> (16 * (e & 1))) & 0xffffu;
        return make_float2((float)(int8_t)(h & 0xffu) * scale, (float)(int8_t)(h >> 8) * scale);
    }
}

// branch constants, DFT and the final sign on the M branch sums of one output: v in, the M channels' values out
template <int M, int S>
__device__ __forceinline__ void cz_rotate(float2 (&v)[M], bool negate)
{
    float2 a[M];
#pragma unroll
    for (int j = 0; j < M; j++) {
        const int q = bank_bitrev(j, bank_log2(M));
        if (S == 0) a[j] = (q & 1) ? make_float2(-v[q].x, -v[q].y) : v[q];
        else a[j] = q == 0 ? v[q] : bank_mul(Tables<M>::branch(q), v[q]);
    }
    radix2<M, false>(a);
#pragma unroll
    for (int k = 0; k < M; k++) v[k] = negate ? make_float2(-a[k].x, -a[k].y) : a[k];
}

}  // namespace

template <int M, int S, int FMT>
__global__ __launch_bounds__(BANK_THREADS)
void channelize_kernel(const void* __restrict__ in, const void* __restrict__ hist, float scale, uint64_t n_out, uint64_t m0,
                       float2* __restrict__ out, uint64_t out_stride)
{
    constexpr uint32_t G = Format<FMT>::G;
    __shared__ __attribute__((aligned(16))) float2 plane[M * BANK_PLANE];        // [q][block - first + 23]
    const uint32_t tid = threadIdx.x;
    const uint64_t first = (uint64_t)blockIdx.x * WR_CZ_TILE;                    // the tile's first output
    const uint32_t count = n_out - first < WR_CZ_TILE ? (uint32_t)(n_out - first) : WR_CZ_TILE;      // its outputs, >= 1

    // the 23 blocks in front of the tile, one sample per lane: from the call's input, or in front of it from hist (zeros)
    if (tid < WR_CZ_HIST * M) {
        const uint64_t have = first * M;                                         // samples of `in` in front of the tile
        float2 x = make_float2(0.f, 0.f);
        if (have + tid >= WR_CZ_HIST * M) x = load_sample<FMT>(in, have + tid - WR_CZ_HIST * M, scale);
        else if (hist) x = load_sample<FMT>(hist, have + tid, scale);
        plane[(tid % M) * BANK_PLANE + tid / M] = x;
    }
    // the tile's own count * M samples in 16-byte pieces; the samples of a last, partial piece one by one
    const uint32_t n_in = count * M;
    const uint8_t* src = static_cast<const uint8_t*>(in) + first * M * Format<FMT>::BYTES;
    for (uint32_t g = tid; g * G < n_in; g += BANK_THREADS) {
        const uint32_t i0 = g * G;
        if (i0 + G <= n_in) {
            const Piece<FMT> pc = *reinterpret_cast<const Piece<FMT>*>(src + (uint64_t)i0 * Format<FMT>::BYTES);
#pragma unroll
            for (uint32_t e = 0; e < G; e++) {
                const uint32_t i = i0 + e;
                plane[(i % M) * BANK_PLANE + WR_CZ_HIST + i / M] = piece_sample<FMT>(pc.w, e, scale);
            }
        } else {
            for (uint32_t i = i0; i < n_in; i++) plane[(i % M) * BANK_PLANE + WR_CZ_HIST + i / M] = load_sample<FMT>(src, i, scale);
        }
    }
    __syncthreads();

    const uint32_t a_out = 2 * tid;                                              // this lane's outputs: a_out and a_out + 1
    if (a_out >= count) return;
    float2 va[M], vb[M];
#pragma unroll
    for (int q = 0; q < M; q++) {
        float tap[BANK_P];
#pragma unroll
        for (uint32_t p = 0; p < BANK_P; p++) {
            const float h = Tables<M>::tap(p * M + M - 1 - q);
            tap[p] = (S && (p & 1)) ? -h : h;
        }
        window_sums(&plane[q * BANK_PLANE + a_out], tap, va[q], vb[q]);
    }
    const uint64_t ma = first + a_out;
    cz_rotate<M, S>(va, S && ((m0 + ma) & 1));
    cz_rotate<M, S>(vb, S && ((m0 + ma + 1) & 1));
    if (a_out + 1 < count) {
#pragma unroll
        for (int k = 0; k < M; k++)
            *reinterpret_cast<Pair2*>(out + (uint64_t)k * out_stride + ma) = Pair2{ { va[k].x, va[k].y, vb[k].x, vb[k].y } };
    } else {
#pragma unroll
        for (int k = 0; k < M; k++) out[(uint64_t)k * out_stride + ma] = va[k];
    }
}

namespace {

template <int M, int S>
hipError_t launch_channelize(hipStream_t st, const void* in, int fmt, float scale, const void* hist, uint64_t n_out, uint64_t m0,
                             float2* out, uint64_t out_stride)
{
    const dim3 grid((uint32_t)((n_out + WR_CZ_TILE - 1) / WR_CZ_TILE)), block(BANK_THREADS);
    const bool known = iq_dispatch(fmt, [&](auto F) {
        hipLaunchKernelGGL((channelize_kernel<M, S, decltype(F)::value>), grid, block, 0, st, in, hist, scale, n_out, m0, out, out_stride);
    });
    return known ? hipGetLastError() : hipErrorInvalidValue;
}

}  // namespace

}  // namespace wr

extern "C" hipError_t wr_launch_channelize(hipStream_t st, const void* in, int fmt, float scale, const void* hist, uint32_t n_channels,
                                           int stacking, uint64_t n_out, uint64_t m0, float2* out, uint64_t out_stride)
{
    if (n_out == 0) return hipSuccess;
    if ((n_out + WR_CZ_TILE - 1) / WR_CZ_TILE > 0x7fffffffull || (stacking != 0 && stacking != 1)) return hipErrorInvalidValue;
#define WR_CZ_CASE(M_)                                                                                                        \
    if (n_channels == M_)                                                                                                     \
        return stacking ? wr::launch_channelize<M_, 1>(st, in, fmt, scale, hist, n_out, m0, out, out_stride)                  \
                        : wr::launch_channelize<M_, 0>(st, in, fmt, scale, hist, n_out, m0, out, out_stride);
    WR_CZ_CASE(2)
    WR_CZ_CASE(4)
    WR_CZ_CASE(8)
#undef WR_CZ_CASE
    return hipErrorInvalidValue;
}

extern "C" const float* wr_channelizer_taps(uint32_t n_channels)
{
    return n_channels == 2 ? wr::cz_host_taps2 : n_channels == 4 ? wr::cz_host_taps4 : n_channels == 8 ? wr::cz_host_taps8 : nullptr;
}
