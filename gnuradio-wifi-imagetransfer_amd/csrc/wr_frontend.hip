// wr_frontend.hip -- the receive front end of NUMERICS.md rule 32: DC removal and blind IQ-imbalance correction of a sample
// stream, in the launch that widens it (rule 20).  The stream is cut into blocks of 4096 samples aligned to its origin; of
// every block five INTEGER sums of the raw samples are kept, so neither the order of a reduction nor the way the stream is
// cut into calls can change a bit.  Three launches per call, none of them a chain over the blocks:
//   fe_stats_kernel   one workgroup per block touched: the call's share of the block's sums into a table
//   fe_apply_kernel   per block: the correction (d, w) from the means of the blocks in front of it -- the state's ring and the
//                     table --, then y = x - d, z = y - w conj(y) on the block's samples
//   fe_commit_kernel  ring, open block and sample count of the state
// and rx_impair_kernel, the receiver impairments of the loop-back.  All bound by memory.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "wr_frontend.h"
#include "wr_iq.h"

namespace wr {

namespace {

constexpr uint32_t FE_THREADS = 256;
constexpr uint32_t FE_BLOCKS_PER_CU = 8;
constexpr uint32_t FE_LOG2_BLOCK = 12;
constexpr uint64_t FE_BLOCK = WIFIRX_FE_BLOCK;
constexpr float    FE_CLAMP = 16777215.0f;        // 2^24 - 1
static_assert(FE_BLOCK == (1u << FE_LOG2_BLOCK) && WIFIRX_FE_RING == 64, "rule 32: blocks of 4096 samples, a ring of 64");
static_assert(sizeof(wifirx_frontend_state) == 2632, "wifirx_frontend_state is part of the ABI");

// the configuration as the kernels take it: to_fix = 2^F (float32), from_fix = 2^-F (float64), both exact
struct FeParams { uint32_t flags, dc_shift, iq_shift; float to_fix; double from_fix; };
struct FeCorr { float2 d, w; };

__host__ __device__ inline uint32_t fe_ilog2(uint64_t b) { return 63u - (uint32_t)__builtin_clzll(b); }

__host__ __device__ inline double fe_sqrt(double x)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __dsqrt_rn(x);
#else
    return std::sqrt(x);
#endif
}

__host__ __device__ inline double fe_div(double a, double b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __ddiv_rn(a, b);
#else
    return a / b;
#endif
}

// rule 32, offset and image coefficient: md = the dc window's means of (sum u, sum v), q = the iq window's five means
__host__ __device__ inline FeCorr fe_derive(const FeParams& p, const int64_t md[2], const int64_t q[5])
{
    FeCorr c;
    c.d = make_float2((float)((double)md[0] * p.from_fix), (float)((double)md[1] * p.from_fix));
    const int64_t mi = q[0], mq = q[1];
    const double P = (double)(q[2] - (mi * mi + mq * mq));
    const double Cr = (double)(q[3] - (mi * mi - mq * mq));
    const double Ci = (double)(q[4] - 2 * mi * mq);
    const double disc = P * P - (Cr * Cr + Ci * Ci);
    c.w = make_float2(0.0f, 0.0f);
    if (P > 0 && !(disc < 0)) {
        const double den = P + fe_sqrt(disc);
        c.w = make_float2((float)fe_div(Cr, den), (float)fe_div(Ci, den));
    }
    return c;
}

// a stage that is switched off uses d = 0 / w = 0
__host__ __device__ inline FeCorr fe_gate(const FeParams& p, FeCorr c)
{
    if (!(p.flags & WIFIRX_FE_DC)) c.d = make_float2(0.0f, 0.0f);
    if (!(p.flags & WIFIRX_FE_IQ)) c.w = make_float2(0.0f, 0.0f);
    return c;
}

__host__ __device__ inline FeCorr fe_initial(const FeParams& p, const wifirx_frontend_state* s)
{
    FeCorr c;
    c.d = make_float2((float)((double)s->d0[0] * p.from_fix), (float)((double)s->d0[1] * p.from_fix));
    c.w = make_float2(s->w0[0], s->w0[1]);
    return fe_gate(p, c);
}

// rule 32, statistics: one component in Q-F; NaN gives 0, everything else is clamped to +-(2^24 - 1)
__device__ __forceinline__ int32_t fe_fix(float x, float to_fix)
{
    const float t = x * to_fix;
    const float r = rintf(t);
    const float c = r < -FE_CLAMP ? -FE_CLAMP : r > FE_CLAMP ? FE_CLAMP : r;
    return t != t ? 0 : (int32_t)c;
}

__device__ __forceinline__ void fe_take(float2 x, float to_fix, int64_t (&a)[5])
{
    const int32_t u = fe_fix(x.x, to_fix), v = fe_fix(x.y, to_fix);
    const int64_t uu = (int64_t)u * u, vv = (int64_t)v * v, uv = (int64_t)u * v;
    a[0] += u;
    a[1] += v;
    a[2] += uu + vv;
    a[3] += uu - vv;
    a[4] += 2 * uv;
}

// rule 32, apply: all float32, one rounding per written operation (-ffp-contract=off)
__device__ __forceinline__ float2 fe_apply(float2 x, const FeCorr& c)
{
    const float yr = x.x - c.d.x, yi = x.y - c.d.y;
    const float cr = (yr * c.w.x) + (yi * c.w.y);
    const float ci = (yr * c.w.y) - (yi * c.w.x);
    return make_float2(yr - cr, yi - ci);
}

__device__ __forceinline__ int64_t wave_sum_i64(int64_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (int64_t)__shfl_xor((long long)v, o);
    return v;
}

// the G samples of a lane's 16-byte piece, widened by rule 20
template <int FMT>
__device__ __forceinline__ void unpack(const Piece<FMT>& v, float scale, float2 (&x)[Format<FMT>::G])
{
    const uint32_t* w = v.w;
    if constexpr (FMT == WIFIRX_IQ_FC32) {
        x[0] = make_float2(__uint_as_float(w[0]), __uint_as_float(w[1]));
        x[1] = make_float2(__uint_as_float(w[2]), __uint_as_float(w[3]));
    } else if constexpr (FMT == WIFIRX_IQ_SC16) {
#pragma unroll
        for (int k = 0; k < 4; k++) x[k] = make_float2((float)(int16_t)(w[k] & 0xffffu) * scale, (float)(int16_t)(w[k] >> 16) * scale);
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++) {
            x[2 * k] = make_float2((float)(int8_t)(w[k] & 0xffu) * scale, (float)(int8_t)((w[k] >> 8) & 0xffu) * scale);
            x[2 * k + 1] = make_float2((float)(int8_t)((w[k] >> 16) & 0xffu) * scale, (float)(int8_t)(w[k] >> 24) * scale);
        }
    }
}

template <int FMT>
__device__ __forceinline__ const Piece<FMT>* piece_at(const void* p, uint64_t first)
{
    return reinterpret_cast<const Piece<FMT>*>(static_cast<const uint8_t*>(p) + first * Format<FMT>::BYTES);
}

// The call's samples [s0, s1) of the block that row k of the table stands for: the stream origin lies `off` samples in front
// of a block boundary, so row 0 is the rest of the state's open block.  s0 >= n: the call does not reach row k.
__device__ __forceinline__ void fe_row_span(uint64_t k, uint64_t off, uint64_t n, uint64_t& s0, uint64_t& s1)
{
    s0 = k == 0 ? 0 : k * FE_BLOCK - off;
    const uint64_t e = (k + 1) * FE_BLOCK - off;
    s1 = e < n ? e : n;
}

// the five sums of block bb as the call knows it: from the table (row 0 on top of the state's open block) when the block was
// completed by this call, otherwise from the ring; shifted to means
__device__ __forceinline__ void fe_block_means(const wifirx_frontend_state* s, const int64_t* table, uint64_t b0, uint64_t bb, int64_t (&m)[5])
{
    if (bb >= b0) {
        const uint64_t k = bb - b0;
#pragma unroll
        for (int i = 0; i < 5; i++) m[i] = (table[k * 5 + i] + (k == 0 ? s->part[i] : 0)) >> FE_LOG2_BLOCK;
    } else {
#pragma unroll
        for (int i = 0; i < 5; i++) m[i] = s->ring[bb & (WIFIRX_FE_RING - 1)][i];
    }
}

}  // namespace

// Statistics: workgroup k takes the call's samples of table row k -- 256 lanes, a whole block is 16 samples per lane, read as
// 16-byte pieces, lane t the pieces t, t + 256, .. --; wave reduction, LDS, one plain store of the five sums.
template <int FMT>
__global__ __launch_bounds__(FE_THREADS)
void fe_stats_kernel(const void* __restrict__ in, uint64_t n, float scale, FeParams prm, const wifirx_frontend_state* __restrict__ state,
                     int64_t* __restrict__ table)
{
    constexpr uint32_t G = Format<FMT>::G;
    __shared__ int64_t s_sum[FE_THREADS / 64][5];
    uint64_t s0, s1;
    fe_row_span(blockIdx.x, state->n & (FE_BLOCK - 1), n, s0, s1);
    if (s0 >= n) return;                    // (uniform) the grid is sized for the worst origin
    const uint32_t len = (uint32_t)(s1 - s0), pieces = len / G, rest = len - pieces * G;
    int64_t a[5] = { 0, 0, 0, 0, 0 };
    for (uint32_t p = threadIdx.x; p < pieces; p += FE_THREADS) {
        float2 x[G];
        unpack<FMT>(*piece_at<FMT>(in, s0 + (uint64_t)p * G), scale, x);
#pragma unroll
        for (uint32_t k = 0; k < G; k++) fe_take(x[k], prm.to_fix, a);
    }
    if (threadIdx.x < rest) fe_take(load_sample<FMT>(in, s0 + (uint64_t)pieces * G + threadIdx.x, scale), prm.to_fix, a);
#pragma unroll
    for (int i = 0; i < 5; i++) a[i] = wave_sum_i64(a[i]);
    if ((threadIdx.x & 63u) == 0) {
#pragma unroll
        for (int i = 0; i < 5; i++) s_sum[threadIdx.x >> 6][i] = a[i];
    }
    __syncthreads();
    if (threadIdx.x < 5) {
        int64_t t = 0;
#pragma unroll
        for (uint32_t w = 0; w < FE_THREADS / 64; w++) t += s_sum[w][threadIdx.x];
        table[(uint64_t)blockIdx.x * 5 + threadIdx.x] = t;
    }
}

// Apply, fused with rule 20's widening: a workgroup takes table rows blockIdx.x, + gridDim.x, ...  Per row the first wave
// gathers the means of the (at most 64) blocks in front -- lane j block b - 1 - j --, sums them over the two windows, and lane 0
// derives (d, w) and hands them to the workgroup through LDS.  Then iq_widen_kernel's shape inside the row: a head sample
// where the float side is not 16-byte aligned, whole pieces, and fewer than G samples behind them.  in == out (fc32): every
// sample is read and written by the same lane.
template <int FMT>
__global__ __launch_bounds__(FE_THREADS)
void fe_apply_kernel(const void* in, float2* out, uint64_t n, float scale, FeParams prm, const wifirx_frontend_state* state,
                     const int64_t* __restrict__ table)
{
    constexpr uint32_t G = Format<FMT>::G;
    __shared__ FeCorr s_corr;
    const uint64_t n0 = state->n, off = n0 & (FE_BLOCK - 1), b0 = n0 >> FE_LOG2_BLOCK;
    const uint64_t rows = (off + n + FE_BLOCK - 1) >> FE_LOG2_BLOCK;
    for (uint64_t k = blockIdx.x; k < rows; k += gridDim.x) {
        const uint64_t b = b0 + k;
        if (threadIdx.x < 64) {
            if (b == 0) {
                if (threadIdx.x == 0) s_corr = fe_initial(prm, state);
            } else {
                const uint32_t lg = fe_ilog2(b);
                const uint32_t sd = prm.dc_shift < lg ? prm.dc_shift : lg, sq = prm.iq_shift < lg ? prm.iq_shift : lg;
                const uint32_t j = threadIdx.x;
                int64_t m[5] = { 0, 0, 0, 0, 0 };
                if (j < (1u << (sd > sq ? sd : sq))) fe_block_means(state, table, b0, b - 1 - j, m);
                int64_t md[2], q[5];
#pragma unroll
                for (int i = 0; i < 2; i++) md[i] = wave_sum_i64(j < (1u << sd) ? m[i] : 0) >> sd;
#pragma unroll
                for (int i = 0; i < 5; i++) q[i] = wave_sum_i64(j < (1u << sq) ? m[i] : 0) >> sq;
                if (j == 0) s_corr = fe_gate(prm, fe_derive(prm, md, q));
            }
        }
        __syncthreads();
        const FeCorr c = s_corr;
        uint64_t s0, s1;
        fe_row_span(k, off, n, s0, s1);
        const uint32_t len = (uint32_t)(s1 - s0);
        const uint32_t head = (uint32_t)((reinterpret_cast<uintptr_t>(out + s0) >> 3) & 1u);      // len >= 1: k < rows
        const uint32_t pieces = (len - head) / G, rest_from = head + pieces * G;
        for (uint32_t p = threadIdx.x; p < pieces; p += FE_THREADS) {
            const uint64_t first = s0 + head + (uint64_t)p * G;
            float2 x[G];
            unpack<FMT>(*piece_at<FMT>(in, first), scale, x);
            float4* o = reinterpret_cast<float4*>(out + first);
#pragma unroll
            for (uint32_t i = 0; i < G / 2; i++) {
                const float2 z0 = fe_apply(x[2 * i], c), z1 = fe_apply(x[2 * i + 1], c);
                o[i] = make_float4(z0.x, z0.y, z1.x, z1.y);
            }
        }
        const uint32_t n_edge = head + (len - rest_from);           // at most 1 + G - 1 samples
        if (threadIdx.x < n_edge) {
            const uint64_t s = s0 + (threadIdx.x < head ? 0u : rest_from + (threadIdx.x - head));
            out[s] = fe_apply(load_sample<FMT>(in, s, scale), c);
        }
        __syncthreads();                    // s_corr is rewritten by the next row
    }
}

// State: lane j owns ring slot j -- the newest block = j (mod 64) that this call completed, if any --, lane 0 the open block
// and the sample count.  Everything is read before the barrier and written behind it.
__global__ __launch_bounds__(64)
void fe_commit_kernel(wifirx_frontend_state* state, const int64_t* __restrict__ table, uint64_t n)
{
    const uint64_t n0 = state->n, b0 = n0 >> FE_LOG2_BLOCK, n1 = n0 + n, b_done = n1 >> FE_LOG2_BLOCK;     // blocks [0, b_done) are complete
    const uint32_t j = threadIdx.x;
    bool have = false;
    int64_t m[5] = { 0, 0, 0, 0, 0 }, part[5] = { 0, 0, 0, 0, 0 };
    if (b_done > b0) {
        const uint64_t last = b_done - 1, back = (last - j) & (WIFIRX_FE_RING - 1);
        if (back <= last - b0) {
            have = true;
            fe_block_means(state, table, b0, last - back, m);
        }
    }
    if (j == 0 && (n1 & (FE_BLOCK - 1))) {
        const uint64_t k = b_done - b0;     // the open block's row; row 0 continues the state's open block
#pragma unroll
        for (int i = 0; i < 5; i++) part[i] = table[k * 5 + i] + (k == 0 ? state->part[i] : 0);
    }
    __syncthreads();
    if (have) {
#pragma unroll
        for (int i = 0; i < 5; i++) state->ring[j][i] = m[i];
    }
    if (j == 0) {
#pragma unroll
        for (int i = 0; i < 5; i++) state->part[i] = part[i];
        state->n = n1;
    }
}

// Receiver impairments: out = mu x + nu conj(x) + dc.  a = x mu and b = conj(x) nu by rule 2, then (a + b) + dc per component.
// One sample per lane and step of a grid-stride loop; in == out: the same lane reads and writes a sample.
__global__ __launch_bounds__(FE_THREADS)
void rx_impair_kernel(const float2* in, float2* out, uint64_t n, float2 mu, float2 nu, float2 dc)
{
    const uint64_t stride = (uint64_t)gridDim.x * FE_THREADS;
    for (uint64_t s = (uint64_t)blockIdx.x * FE_THREADS + threadIdx.x; s < n; s += stride) {
        const float2 x = in[s];
        const float ar = __fmaf_rn(-x.y, mu.y, x.x * mu.x), ai = __fmaf_rn(x.y, mu.x, x.x * mu.y);
        const float br = __fmaf_rn(x.y, nu.y, x.x * nu.x), bi = __fmaf_rn(-x.y, nu.x, x.x * nu.y);
        out[s] = make_float2((ar + br) + dc.x, (ai + bi) + dc.y);
    }
}

namespace {

FeParams fe_params(const wifirx_frontend_cfg* cfg)
{
    return FeParams{ cfg->flags, cfg->dc_shift, cfg->iq_shift, std::ldexp(1.0f, (int)cfg->frac_bits), std::ldexp(1.0, -(int)cfg->frac_bits) };
}

template <int FMT>
hipError_t launch_frontend(hipStream_t st, const FeParams& prm, wifirx_frontend_state* state, const void* in, float scale, uint64_t n,
                           float2* out, int64_t* table, uint32_t n_cu)
{
    const uint64_t rows = wr_frontend_table_rows(n), cap = (uint64_t)(n_cu ? n_cu : 256u) * FE_BLOCKS_PER_CU;
    hipLaunchKernelGGL(fe_stats_kernel<FMT>, dim3((uint32_t)rows), dim3(FE_THREADS), 0, st, in, n, scale, prm, state, table);
    hipLaunchKernelGGL(fe_apply_kernel<FMT>, dim3((uint32_t)(rows < cap ? rows : cap)), dim3(FE_THREADS), 0, st, in, out, n, scale, prm,
                       state, table);
    hipLaunchKernelGGL(fe_commit_kernel, dim3(1), dim3(64), 0, st, state, table, n);
    return hipGetLastError();
}

}  // namespace

}  // namespace wr

extern "C" uint64_t wr_frontend_table_rows(uint64_t n) { return (n >> wr::FE_LOG2_BLOCK) + 2; }

extern "C" hipError_t wr_launch_frontend(hipStream_t st, const wifirx_frontend_cfg* cfg, wifirx_frontend_state* state, const void* in,
                                         int fmt, float scale, uint64_t n, float2* out, int64_t* table, uint32_t n_cu)
{
    if (n == 0) return hipSuccess;
    if (n > (1ull << 40)) return hipErrorInvalidValue;         // the statistics grid is one workgroup per block
    const wr::FeParams prm = wr::fe_params(cfg);
    hipError_t e = hipErrorInvalidValue;
    wr::iq_dispatch(fmt, [&](auto F) { e = wr::launch_frontend<decltype(F)::value>(st, prm, state, in, scale, n, out, table, n_cu); });
    return e;
}

// wifirx_frontend_estimate: what the block of the stream's next sample is corrected with, on the host
extern "C" void wr_frontend_estimate_host(const wifirx_frontend_cfg* cfg, const wifirx_frontend_state* s, float dc[2], float w[2])
{
    const wr::FeParams prm = wr::fe_params(cfg);
    const uint64_t b = s->n >> wr::FE_LOG2_BLOCK;
    wr::FeCorr c;
    if (b == 0) {
        c = wr::fe_initial(prm, s);
    } else {
        const uint32_t lg = wr::fe_ilog2(b);
        const uint32_t sh[2] = { prm.dc_shift < lg ? prm.dc_shift : lg, prm.iq_shift < lg ? prm.iq_shift : lg };
        int64_t sum[2][5] = {};
        for (int wdw = 0; wdw < 2; wdw++)
            for (uint64_t j = 0; j < (1ull << sh[wdw]); j++)
                for (int i = 0; i < 5; i++) sum[wdw][i] += s->ring[(b - 1 - j) & (WIFIRX_FE_RING - 1)][i];
        int64_t md[2], q[5];
        for (int i = 0; i < 2; i++) md[i] = sum[0][i] >> sh[0];
        for (int i = 0; i < 5; i++) q[i] = sum[1][i] >> sh[1];
        c = wr::fe_gate(prm, wr::fe_derive(prm, md, q));
    }
    dc[0] = c.d.x; dc[1] = c.d.y;
    w[0] = c.w.x; w[1] = c.w.y;
}

extern "C" hipError_t wr_launch_rx_impair(hipStream_t st, const float2* in, float2* out, uint64_t n, float2 mu, float2 nu, float2 dc,
                                          uint32_t n_cu)
{
    if (n == 0) return hipSuccess;
    const uint64_t want = (n + wr::FE_THREADS - 1) / wr::FE_THREADS, cap = (uint64_t)(n_cu ? n_cu : 256u) * wr::FE_BLOCKS_PER_CU;
    hipLaunchKernelGGL(wr::rx_impair_kernel, dim3((uint32_t)(want < cap ? want : cap)), dim3(wr::FE_THREADS), 0, st, in, out, n, mu, nu, dc);
    return hipGetLastError();
}
