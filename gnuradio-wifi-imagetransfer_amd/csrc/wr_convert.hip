// wr_convert.hip -- the sample-format converters of NUMERICS.md rule 20: integer IQ pairs as the radios deliver them (sc16:
// int16 I, int16 Q; sc8: int8 I, int8 Q) to the float pairs every other kernel reads, and the quantiser that goes the other
// way (the converter between the channel and the receiver of the loop-back).  Two streaming kernels, one multiply per
// component: both are bound by memory.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wr_convert.h"
#include "wr_iq.h"

namespace wr {

namespace {

constexpr uint32_t CONV_THREADS = 256;
constexpr uint32_t CONV_BLOCKS_PER_CU = 8;

template <int FMT>
__device__ __forceinline__ void store_sample(void* p, uint64_t s, int i, int q)
{
    if constexpr (FMT == WIFIRX_IQ_SC16) static_cast<uint32_t*>(p)[s] = ((uint32_t)i & 0xffffu) | ((uint32_t)q << 16);
    else static_cast<uint16_t*>(p)[s] = (uint16_t)(((uint32_t)i & 0xffu) | (((uint32_t)q & 0xffu) << 8));
}

template <int FMT>
__device__ __forceinline__ Piece<FMT>* piece_at(void* p, uint64_t first)
{
    return reinterpret_cast<Piece<FMT>*>(static_cast<uint8_t*>(p) + first * Format<FMT>::BYTES);
}

// How a call of n samples is cut: `head` samples (0 or 1) in front bring the float side to a 16-byte boundary, `groups`
// whole pieces follow, and fewer than G samples are left behind them.  Head and rest go sample by sample.
template <int FMT>
struct Cut {
    uint64_t head, groups, rest_from;
    __host__ __device__ Cut(const void* float_side, uint64_t n)
    {
        head = ((reinterpret_cast<uintptr_t>(float_side) >> 3) & 1u) < n ? ((reinterpret_cast<uintptr_t>(float_side) >> 3) & 1u) : n;
        groups = (n - head) / Format<FMT>::G;
        rest_from = head + groups * Format<FMT>::G;
    }
};

// rule 20, quantise: one component; counts it when it clipped
__device__ __forceinline__ int quantise1(float x, float scale, float lo, float hi, uint32_t& clipped)
{
    const float t = x * scale;
    const float r = rintf(t);
    const bool nan = t != t;
    clipped += (nan || r < lo || r > hi) ? 1u : 0u;
    const float c = r < lo ? lo : r > hi ? hi : r;
    return nan ? 0 : (int)c;
}

__device__ __forceinline__ unsigned long long wave_sum64(unsigned long long v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

}  // namespace

// Widen: a lane reads the 16 bytes of a piece and stores its 2 (sc16) or 4 (sc8) 16-byte pieces of float pairs; a grid-stride
// loop over the pieces, 64-bit indices throughout.  The lanes of workgroup 0 also take the head and the rest, one sample each.
template <int FMT>
__global__ __launch_bounds__(CONV_THREADS)
void iq_widen_kernel(const void* __restrict__ src, float2* __restrict__ dst, uint64_t n, float scale)
{
    constexpr uint32_t G = Format<FMT>::G;
    const Cut<FMT> cut(dst, n);
    const uint64_t stride = (uint64_t)gridDim.x * CONV_THREADS;
    for (uint64_t g = (uint64_t)blockIdx.x * CONV_THREADS + threadIdx.x; g < cut.groups; g += stride) {
        const uint64_t first = cut.head + g * G;
        const Piece<FMT> v = *piece_at<FMT>(const_cast<void*>(src), first);
        float4* out = reinterpret_cast<float4*>(dst + first);
        const uint32_t* w = v.w;
        if constexpr (FMT == WIFIRX_IQ_SC16) {
#pragma unroll
            for (int k = 0; k < 2; k++)
                out[k] = make_float4((float)(int16_t)(w[2 * k] & 0xffffu) * scale, (float)(int16_t)(w[2 * k] >> 16) * scale,
                                     (float)(int16_t)(w[2 * k + 1] & 0xffffu) * scale, (float)(int16_t)(w[2 * k + 1] >> 16) * scale);
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++)
                out[k] = make_float4((float)(int8_t)(w[k] & 0xffu) * scale, (float)(int8_t)((w[k] >> 8) & 0xffu) * scale,
                                     (float)(int8_t)((w[k] >> 16) & 0xffu) * scale, (float)(int8_t)(w[k] >> 24) * scale);
        }
    }
    const uint64_t n_edge = cut.head + (n - cut.rest_from);       // at most 1 + G - 1 samples
    if (blockIdx.x == 0 && threadIdx.x < n_edge) {
        const uint64_t s = threadIdx.x < cut.head ? threadIdx.x : cut.rest_from + (threadIdx.x - cut.head);
        dst[s] = load_sample<FMT>(src, s, scale);
    }
}

// Quantise: the mirror image -- a lane reads 2 or 4 16-byte pieces of float pairs and stores the 16 bytes of a piece.  The
// clipped components are counted per lane, summed per wave, added per workgroup in LDS, and one 64-bit atomic add per
// workgroup goes to *count (link_stats_kernel's scheme); with count == null nothing leaves the lane.
template <int FMT>
__global__ __launch_bounds__(CONV_THREADS)
void iq_quantise_kernel(const float2* __restrict__ src, void* __restrict__ dst, uint64_t n, float scale, float lo, float hi,
                        unsigned long long* __restrict__ count)
{
    constexpr uint32_t G = Format<FMT>::G;
    __shared__ unsigned long long s_cnt;
    if (threadIdx.x == 0) s_cnt = 0;
    __syncthreads();
    const Cut<FMT> cut(src, n);
    const uint64_t stride = (uint64_t)gridDim.x * CONV_THREADS;
    unsigned long long c = 0;
    for (uint64_t g = (uint64_t)blockIdx.x * CONV_THREADS + threadIdx.x; g < cut.groups; g += stride) {
        const uint64_t first = cut.head + g * G;
        const float4* in = reinterpret_cast<const float4*>(src + first);
        float4 x[G / 2];
#pragma unroll
        for (uint32_t k = 0; k < G / 2; k++) x[k] = in[k];
        uint32_t w[4], clipped = 0;
        if constexpr (FMT == WIFIRX_IQ_SC16) {
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const float a = (k & 1) ? x[k >> 1].z : x[k >> 1].x, b = (k & 1) ? x[k >> 1].w : x[k >> 1].y;
                const int i = quantise1(a, scale, lo, hi, clipped), q = quantise1(b, scale, lo, hi, clipped);
                w[k] = ((uint32_t)i & 0xffffu) | ((uint32_t)q << 16);
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int i0 = quantise1(x[k].x, scale, lo, hi, clipped), q0 = quantise1(x[k].y, scale, lo, hi, clipped);
                const int i1 = quantise1(x[k].z, scale, lo, hi, clipped), q1 = quantise1(x[k].w, scale, lo, hi, clipped);
                w[k] = ((uint32_t)i0 & 0xffu) | (((uint32_t)q0 & 0xffu) << 8) | (((uint32_t)i1 & 0xffu) << 16) | ((uint32_t)q1 << 24);
            }
        }
        c += clipped;
        *piece_at<FMT>(dst, first) = Piece<FMT>{ { w[0], w[1], w[2], w[3] } };
    }
    const uint64_t n_edge = cut.head + (n - cut.rest_from);
    if (blockIdx.x == 0 && threadIdx.x < n_edge) {
        const uint64_t s = threadIdx.x < cut.head ? threadIdx.x : cut.rest_from + (threadIdx.x - cut.head);
        const float2 x = src[s];
        uint32_t clipped = 0;
        const int i = quantise1(x.x, scale, lo, hi, clipped), q = quantise1(x.y, scale, lo, hi, clipped);
        store_sample<FMT>(dst, s, i, q);
        c += clipped;
    }
    if (count == nullptr) return;         // (uniform: every lane of the grid takes the same way)
    c = wave_sum64(c);
    if ((threadIdx.x & 63u) == 0 && c) atomicAdd(&s_cnt, c);
    __syncthreads();
    if (threadIdx.x == 0 && s_cnt) atomicAdd(count, s_cnt);
}

namespace {

uint32_t conv_grid(uint64_t groups, uint32_t n_cu)
{
    const uint64_t want = (groups + CONV_THREADS - 1) / CONV_THREADS, cap = (uint64_t)(n_cu ? n_cu : 256u) * CONV_BLOCKS_PER_CU;
    return (uint32_t)(want < 1 ? 1 : want < cap ? want : cap);
}

template <int FMT>
hipError_t launch_widen(hipStream_t st, const void* src, uint64_t n, float scale, float2* dst, uint32_t n_cu)
{
    const Cut<FMT> cut(dst, n);
    const dim3 grid(conv_grid(cut.groups, n_cu)), block(CONV_THREADS);
    hipLaunchKernelGGL(iq_widen_kernel<FMT>, grid, block, 0, st, src, dst, n, scale);
    return hipGetLastError();
}

template <int FMT>
hipError_t launch_quantise(hipStream_t st, const float2* src, uint64_t n, float scale, uint32_t bits, void* dst,
                           unsigned long long* count, uint32_t n_cu)
{
    const Cut<FMT> cut(src, n);
    const float lo = -(float)(1u << (bits - 1)), hi = (float)((1u << (bits - 1)) - 1u);
    const dim3 grid(conv_grid(cut.groups, n_cu)), block(CONV_THREADS);
    hipLaunchKernelGGL(iq_quantise_kernel<FMT>, grid, block, 0, st, src, dst, n, scale, lo, hi, count);
    return hipGetLastError();
}

}  // namespace

}  // namespace wr

extern "C" hipError_t wr_launch_iq_widen(hipStream_t st, const void* src, int fmt, uint64_t n, float scale, float2* dst, uint32_t n_cu)
{
    if (n == 0) return hipSuccess;
    if (fmt == WIFIRX_IQ_SC16) return wr::launch_widen<WIFIRX_IQ_SC16>(st, src, n, scale, dst, n_cu);
    if (fmt == WIFIRX_IQ_SC8) return wr::launch_widen<WIFIRX_IQ_SC8>(st, src, n, scale, dst, n_cu);
    return hipErrorInvalidValue;
}

extern "C" hipError_t wr_launch_iq_quantise(hipStream_t st, const float2* src, uint64_t n, float scale, int fmt, uint32_t bits,
                                            void* dst, unsigned long long* count, uint32_t n_cu)
{
    if (n == 0) return hipSuccess;
    if (fmt == WIFIRX_IQ_SC16 && bits >= 2 && bits <= 16) return wr::launch_quantise<WIFIRX_IQ_SC16>(st, src, n, scale, bits, dst, count, n_cu);
    if (fmt == WIFIRX_IQ_SC8 && bits >= 2 && bits <= 8) return wr::launch_quantise<WIFIRX_IQ_SC8>(st, src, n, scale, bits, dst, count, n_cu);
    return hipErrorInvalidValue;
}
