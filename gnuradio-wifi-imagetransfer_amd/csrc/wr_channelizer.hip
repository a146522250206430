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
#include "wr_channelizer_table.h"

namespace wr {

namespace {

constexpr uint32_t CZ_THREADS = WR_CZ_TILE / 2;
constexpr uint32_t CZ_P = WR_CZ_TAPS_PER_BRANCH;
constexpr uint32_t CZ_PLANE = WR_CZ_TILE + WR_CZ_HIST + 1;          // float2 per plane; even, so every plane starts on 16 bytes
static_assert(CZ_P == WR_CZ_HIST + 1 && CZ_PLANE % 2 == 0 && WR_CZ_HIST * 8 <= CZ_THREADS, "tile geometry");

template <int M> struct Tables;
#define WR_CZ_TABLES(M_)                                                                      \
    __device__ const float cz_taps##M_[CZ_P * M_] = WR_CZ_TAPS##M_##_INIT;                    \
    __device__ const float cz_branch##M_[2 * M_] = WR_CZ_BRANCH##M_##_INIT;                   \
    __device__ const float cz_twiddle##M_[M_] = WR_CZ_TWIDDLE##M_##_INIT;                     \
    const float cz_host_taps##M_[CZ_P * M_] = WR_CZ_TAPS##M_##_INIT;                          \
    template <> struct Tables<M_> {                                                           \
        static __device__ __forceinline__ float tap(int i) { return cz_taps##M_[i]; }         \
        static __device__ __forceinline__ float2 branch(int q) { return make_float2(cz_branch##M_[2 * q], cz_branch##M_[2 * q + 1]); } \
        static __device__ __forceinline__ float2 twiddle(int t) { return make_float2(cz_twiddle##M_[2 * t], cz_twiddle##M_[2 * t + 1]); } \
    };
WR_CZ_TABLES(2)
WR_CZ_TABLES(4)
WR_CZ_TABLES(8)
#undef WR_CZ_TABLES

// A lane's piece of input is 16 bytes: G samples of BYTES bytes each, declared at the format's natural alignment, which is all
// a caller's buffer promises (wr_convert.hip's Piece: one 16-byte instruction, taken by the hardware at any such address).
template <int FMT> struct Format;
template <> struct Format<WIFIRX_IQ_FC32> { static constexpr uint32_t G = 2, BYTES = 8; };
template <> struct Format<WIFIRX_IQ_SC16> { static constexpr uint32_t G = 4, BYTES = 4; };
template <> struct Format<WIFIRX_IQ_SC8>  { static constexpr uint32_t G = 8, BYTES = 2; };
template <int FMT> struct __attribute__((packed, aligned(Format<FMT>::BYTES))) Piece { uint32_t w[4]; };
struct __attribute__((packed, aligned(8))) OutPair { float v[4]; };

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

// sample s of a buffer, widened by rule 20; natural alignment
template <int FMT>
__device__ __forceinline__ float2 load_sample(const void* p, uint64_t s, float scale)
{
    if constexpr (FMT == WIFIRX_IQ_FC32) {
        return static_cast<const float2*>(p)[s];
    } else if constexpr (FMT == WIFIRX_IQ_SC16) {
        const uint32_t w = static_cast<const uint32_t*>(p)[s];
        return make_float2((float)(int16_t)(w & 0xffffu) * scale, (float)(int16_t)(w >> 16) * scale);
    } else {
        const uint32_t w = static_cast<const uint16_t*>(p)[s];
        return make_float2((float)(int8_t)(w & 0xffu) * scale, (float)(int8_t)(w >> 8) * scale);
    }
}

// rule 17's plain complex product
__device__ __forceinline__ float2 cz_mul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }

constexpr int cz_bitrev(int j, int bits)
{
    int r = 0;
    for (int i = 0; i < bits; i++) r |= ((j >> i) & 1) << (bits - 1 - i);
    return r;
}
constexpr int cz_log2(int m) { return m == 2 ? 1 : m == 4 ? 2 : 3; }

// branch constants, DFT and the final sign on the M branch sums of one output: v in, the M channels' values out
template <int M, int S>
__device__ __forceinline__ void cz_rotate(float2 (&v)[M], bool negate)
{
    float2 a[M];
#pragma unroll
    for (int j = 0; j < M; j++) {
        const int q = cz_bitrev(j, cz_log2(M));
        if (S == 0) a[j] = (q & 1) ? make_float2(-v[q].x, -v[q].y) : v[q];
        else a[j] = q == 0 ? v[q] : cz_mul(Tables<M>::branch(q), v[q]);
    }
#pragma unroll
    for (int len = 2; len <= M; len *= 2) {
#pragma unroll
        for (int base = 0; base < M; base += len) {
#pragma unroll
            for (int t = 0; t < len / 2; t++) {
                const int e = t * (M / len);
                const float2 b = a[base + t + len / 2];
                const float2 x = e == 0 ? b : 4 * e == M ? make_float2(b.y, -b.x) : cz_mul(Tables<M>::twiddle(e), b);
                const float2 lo = a[base + t];
                a[base + t] = make_float2(lo.x + x.x, lo.y + x.y);
                a[base + t + len / 2] = make_float2(lo.x - x.x, lo.y - x.y);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < M; k++) v[k] = negate ? make_float2(-a[k].x, -a[k].y) : a[k];
}

}  // namespace

template <int M, int S, int FMT>
__global__ __launch_bounds__(CZ_THREADS)
void channelize_kernel(const void* __restrict__ in, const void* __restrict__ hist, float scale, uint64_t n_out, uint64_t m0,
                       float2* __restrict__ out, uint64_t out_stride)
{
    constexpr uint32_t G = Format<FMT>::G;
    __shared__ __attribute__((aligned(16))) float2 plane[M * CZ_PLANE];          // [q][block - first + 23]
    const uint32_t tid = threadIdx.x;
    const uint64_t first = (uint64_t)blockIdx.x * WR_CZ_TILE;                    // the tile's first output
    const uint32_t count = n_out - first < WR_CZ_TILE ? (uint32_t)(n_out - first) : WR_CZ_TILE;      // its outputs, >= 1

    // the 23 blocks in front of the tile, one sample per lane: from the call's input, or in front of it from hist (zeros)
    if (tid < WR_CZ_HIST * M) {
        const uint64_t have = first * M;                                         // samples of `in` in front of the tile
        float2 x = make_float2(0.f, 0.f);
        if (have + tid >= WR_CZ_HIST * M) x = load_sample<FMT>(in, have + tid - WR_CZ_HIST * M, scale);
        else if (hist) x = load_sample<FMT>(hist, have + tid, scale);
        plane[(tid % M) * CZ_PLANE + tid / M] = x;
    }
    // the tile's own count * M samples in 16-byte pieces; the samples of a last, partial piece one by one
    const uint32_t n_in = count * M;
    const uint8_t* src = static_cast<const uint8_t*>(in) + first * M * Format<FMT>::BYTES;
    for (uint32_t g = tid; g * G < n_in; g += CZ_THREADS) {
        const uint32_t i0 = g * G;
        if (i0 + G <= n_in) {
            const Piece<FMT> pc = *reinterpret_cast<const Piece<FMT>*>(src + (uint64_t)i0 * Format<FMT>::BYTES);
#pragma unroll
            for (uint32_t e = 0; e < G; e++) {
                const uint32_t i = i0 + e;
                plane[(i % M) * CZ_PLANE + WR_CZ_HIST + i / M] = piece_sample<FMT>(pc.w, e, scale);
            }
        } else {
            for (uint32_t i = i0; i < n_in; i++) plane[(i % M) * CZ_PLANE + WR_CZ_HIST + i / M] = load_sample<FMT>(src, i, scale);
        }
    }
    __syncthreads();

    const uint32_t a_out = 2 * tid;                                              // this lane's outputs: a_out and a_out + 1
    if (a_out >= count) return;
    float2 va[M], vb[M];
#pragma unroll
    for (int q = 0; q < M; q++) {
        // blocks a_out - 23 .. a_out + 1 of plane q: w[j] = block a_out - 23 + j
        float2 w[CZ_P + 1];
        const float4* p4 = reinterpret_cast<const float4*>(&plane[q * CZ_PLANE + a_out]);
#pragma unroll
        for (uint32_t j = 0; j < CZ_P / 2; j++) {
            const float4 t = p4[j];
            w[2 * j] = make_float2(t.x, t.y);
            w[2 * j + 1] = make_float2(t.z, t.w);
        }
        w[CZ_P] = plane[q * CZ_PLANE + a_out + CZ_P];
        float2 sa, sb;
#pragma unroll
        for (uint32_t p = 0; p < CZ_P; p++) {
            const float h = Tables<M>::tap(p * M + M - 1 - q);
            const float g = (S && (p & 1)) ? -h : h;
            const float2 xa = w[CZ_P - 1 - p], xb = w[CZ_P - p];
            const float2 ta = make_float2(g * xa.x, g * xa.y), tb = make_float2(g * xb.x, g * xb.y);
            sa = p == 0 ? ta : make_float2(sa.x + ta.x, sa.y + ta.y);
            sb = p == 0 ? tb : make_float2(sb.x + tb.x, sb.y + tb.y);
        }
        // Both sums exist here, and only one branch's window is in registers at a time.  Without the two lines below the
        // compiler sinks the second output's sums into the branch that stores it and keeps all M windows alive for that
        // (256 VGPRs and copies in AGPRs at M = 8).
        asm volatile("" : "+v"(sa.x), "+v"(sa.y), "+v"(sb.x), "+v"(sb.y));
        __builtin_amdgcn_sched_barrier(0);
        va[q] = sa;
        vb[q] = sb;
    }
    const uint64_t ma = first + a_out;
    cz_rotate<M, S>(va, S && ((m0 + ma) & 1));
    cz_rotate<M, S>(vb, S && ((m0 + ma + 1) & 1));
    if (a_out + 1 < count) {
#pragma unroll
        for (int k = 0; k < M; k++)
            *reinterpret_cast<OutPair*>(out + (uint64_t)k * out_stride + ma) = OutPair{ { va[k].x, va[k].y, vb[k].x, vb[k].y } };
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
    const dim3 grid((uint32_t)((n_out + WR_CZ_TILE - 1) / WR_CZ_TILE)), block(CZ_THREADS);
    if (fmt == WIFIRX_IQ_FC32) hipLaunchKernelGGL((channelize_kernel<M, S, WIFIRX_IQ_FC32>), grid, block, 0, st, in, hist, scale, n_out, m0, out, out_stride);
    else if (fmt == WIFIRX_IQ_SC16) hipLaunchKernelGGL((channelize_kernel<M, S, WIFIRX_IQ_SC16>), grid, block, 0, st, in, hist, scale, n_out, m0, out, out_stride);
    else if (fmt == WIFIRX_IQ_SC8) hipLaunchKernelGGL((channelize_kernel<M, S, WIFIRX_IQ_SC8>), grid, block, 0, st, in, hist, scale, n_out, m0, out, out_stride);
    else return hipErrorInvalidValue;
    return hipGetLastError();
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
