// wr_combiner.hip -- the synthesis bank of NUMERICS.md rule 22: M streams at fs, one per adjacent 20 MHz channel, into one
// wideband stream sampled at M fs.  An M-point inverse DFT across the channels per input block and a polyphase filter
// (24 taps per branch) per output: the mirror of wr_channelizer.hip, with the same prototype; what the two share is wr_bank.h.
//
// One workgroup turns a tile of WR_CB_TILE input blocks (one sample of every channel) into WR_CB_TILE * M outputs.  A lane
// reads two adjacent samples of every row as one 16-byte piece, applies the gains and the inverse DFT in registers and
// writes the M results into M LDS planes [r][block]; lanes 0..22 do the same for the 23 blocks in front of the tile.  Then
// a lane makes the outputs of two adjacent blocks: their 24-tap windows share 23 of 25 blocks, which it reads as twelve
// 16-byte pieces and one 8-byte piece per branch, and it owns 2 M consecutive outputs, stored as M 16-byte pieces.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wr_combiner.h"
#include "wr_bank.h"

namespace wr {

static_assert(WR_CB_TILE == BANK_TILE && WR_CB_HIST == BANK_HIST && WR_CB_HIST <= BANK_THREADS, "tile geometry");

// the gains travel as kernel arguments
struct CombineGains { float g[8]; };

namespace {

// gains and the inverse DFT across the channels of one block: u_k in, V_r out
template <int M>
__device__ __forceinline__ void cb_spread(float2 (&u)[M], const CombineGains& gn, bool has_gains)
{
    float2 a[M];
#pragma unroll
    for (int j = 0; j < M; j++) {
        const int k = bank_bitrev(j, bank_log2(M));
        a[j] = has_gains ? make_float2(u[k].x * gn.g[k], u[k].y * gn.g[k]) : u[k];
    }
    radix2<M, true>(a);
#pragma unroll
    for (int r = 0; r < M; r++) u[r] = a[r];
}

// branch constant and block sign on one branch sum
template <int M, int S>
__device__ __forceinline__ float2 cb_rotate(float2 v, int r, bool negate)
{
    float2 x;
    if (S == 0) x = (r & 1) ? make_float2(-v.x, -v.y) : v;
    else x = r == 0 ? v : bank_mul(bank_conj(Tables<M>::branch(r)), v);
    return negate ? make_float2(-x.x, -x.y) : x;
}

}  // namespace

template <int M, int S>
__global__ __launch_bounds__(BANK_THREADS)
void combine_kernel(const float2* __restrict__ in, uint64_t in_stride, const float2* __restrict__ hist, CombineGains gn,
                    int has_gains, uint64_t n_in, uint64_t m0, float2* __restrict__ out)
{
    __shared__ __attribute__((aligned(16))) float2 plane[M * BANK_PLANE];        // [r][block - first + 23]
    const uint32_t tid = threadIdx.x;
    const uint64_t first = (uint64_t)blockIdx.x * WR_CB_TILE;                    // the tile's first block
    const uint32_t count = n_in - first < WR_CB_TILE ? (uint32_t)(n_in - first) : WR_CB_TILE;        // its blocks, >= 1
    const uint32_t a_blk = 2 * tid;                                              // this lane's blocks: a_blk and a_blk + 1

    // the 23 blocks in front of the tile, one per lane: from the call's rows, or in front of them from hist (zeros)
    if (tid < WR_CB_HIST) {
        float2 u[M];
#pragma unroll
        for (int k = 0; k < M; k++) {
            u[k] = make_float2(0.f, 0.f);
            if (first + tid >= WR_CB_HIST) u[k] = in[(uint64_t)k * in_stride + (first + tid - WR_CB_HIST)];
            else if (hist) u[k] = hist[(uint32_t)k * WR_CB_HIST + (uint32_t)first + tid];
        }
        cb_spread<M>(u, gn, has_gains);
#pragma unroll
        for (int r = 0; r < M; r++) plane[r * BANK_PLANE + tid] = u[r];
    }
    // the tile's own blocks, two per lane in 16-byte pieces; a last odd block sample by sample
    if (a_blk + 1 < count) {
        float2 ua[M], ub[M];
#pragma unroll
        for (int k = 0; k < M; k++) {
            const Pair2 pc = *reinterpret_cast<const Pair2*>(in + (uint64_t)k * in_stride + first + a_blk);
            ua[k] = make_float2(pc.v[0], pc.v[1]);
            ub[k] = make_float2(pc.v[2], pc.v[3]);
        }
        cb_spread<M>(ua, gn, has_gains);
        cb_spread<M>(ub, gn, has_gains);
#pragma unroll
        for (int r = 0; r < M; r++) {
            plane[r * BANK_PLANE + WR_CB_HIST + a_blk] = ua[r];
            plane[r * BANK_PLANE + WR_CB_HIST + a_blk + 1] = ub[r];
        }
    } else if (a_blk < count) {
        float2 ua[M];
#pragma unroll
        for (int k = 0; k < M; k++) ua[k] = in[(uint64_t)k * in_stride + first + a_blk];
        cb_spread<M>(ua, gn, has_gains);
#pragma unroll
        for (int r = 0; r < M; r++) plane[r * BANK_PLANE + WR_CB_HIST + a_blk] = ua[r];
    }
    __syncthreads();

    if (a_blk >= count) return;
    float2 va[M], vb[M];
#pragma unroll
    for (int r = 0; r < M; r++) {
        float tap[BANK_P];
#pragma unroll
        for (uint32_t p = 0; p < BANK_P; p++) tap[p] = (float)M * Tables<M>::tap(p * M + r);
        window_sums(&plane[r * BANK_PLANE + a_blk], tap, va[r], vb[r]);
    }
    const uint64_t ma = first + a_blk;
    const bool nega = S && ((m0 + ma) & 1), negb = S && ((m0 + ma + 1) & 1);
    float2* dst = out + ma * M;                                                  // 2 M consecutive outputs: block a_blk, then a_blk + 1
#pragma unroll
    for (int r = 0; r < M; r += 2) {
        const float2 x0 = cb_rotate<M, S>(va[r], r, nega), x1 = cb_rotate<M, S>(va[r + 1], r + 1, nega);
        *reinterpret_cast<Pair2*>(dst + r) = Pair2{ { x0.x, x0.y, x1.x, x1.y } };
    }
    if (a_blk + 1 < count) {
#pragma unroll
        for (int r = 0; r < M; r += 2) {
            const float2 x0 = cb_rotate<M, S>(vb[r], r, negb), x1 = cb_rotate<M, S>(vb[r + 1], r + 1, negb);
            *reinterpret_cast<Pair2*>(dst + M + r) = Pair2{ { x0.x, x0.y, x1.x, x1.y } };
        }
    }
}

// hist_out: the last 23 samples of (hist || in) per row, one per lane; bit patterns are copied, not values
__global__ __launch_bounds__(256)
void combine_history_kernel(const uint2* __restrict__ in, uint64_t in_stride, const uint2* __restrict__ hist, uint32_t n_channels,
                            uint64_t n_in, uint2* __restrict__ hist_out)
{
    const uint32_t t = threadIdx.x;
    if (t >= n_channels * WR_CB_HIST) return;
    const uint32_t k = t / WR_CB_HIST, j = t % WR_CB_HIST;
    uint2 x = make_uint2(0u, 0u);
    if (n_in + j >= WR_CB_HIST) x = in[(uint64_t)k * in_stride + (n_in + j - WR_CB_HIST)];
    else if (hist) x = hist[k * WR_CB_HIST + (uint32_t)n_in + j];
    hist_out[t] = x;
}

namespace {

template <int M>
hipError_t launch_combine(hipStream_t st, const float2* in, uint64_t in_stride, const CombineGains& gn, int has_gains,
                          const float2* hist, int stacking, uint64_t n_in, uint64_t m0, float2* out)
{
    const dim3 grid((uint32_t)((n_in + WR_CB_TILE - 1) / WR_CB_TILE)), block(BANK_THREADS);
    if (stacking) hipLaunchKernelGGL((combine_kernel<M, 1>), grid, block, 0, st, in, in_stride, hist, gn, has_gains, n_in, m0, out);
    else hipLaunchKernelGGL((combine_kernel<M, 0>), grid, block, 0, st, in, in_stride, hist, gn, has_gains, n_in, m0, out);
    return hipGetLastError();
}

}  // namespace

}  // namespace wr

extern "C" hipError_t wr_launch_combine(hipStream_t st, const float2* in, uint64_t in_stride, const float* gains, const float2* hist,
                                        uint32_t n_channels, int stacking, uint64_t n_in, uint64_t m0, float2* out)
{
    if (n_in == 0) return hipSuccess;
    if ((n_in + WR_CB_TILE - 1) / WR_CB_TILE > 0x7fffffffull || (stacking != 0 && stacking != 1)) return hipErrorInvalidValue;
    if (n_channels != 2 && n_channels != 4 && n_channels != 8) return hipErrorInvalidValue;
    wr::CombineGains gn;
    for (uint32_t k = 0; k < 8; k++) gn.g[k] = gains && k < n_channels ? gains[k] : 1.f;
    const int has_gains = gains != nullptr;
    if (n_channels == 2) return wr::launch_combine<2>(st, in, in_stride, gn, has_gains, hist, stacking, n_in, m0, out);
    if (n_channels == 4) return wr::launch_combine<4>(st, in, in_stride, gn, has_gains, hist, stacking, n_in, m0, out);
    return wr::launch_combine<8>(st, in, in_stride, gn, has_gains, hist, stacking, n_in, m0, out);
}

extern "C" hipError_t wr_launch_combine_history(hipStream_t st, const float2* in, uint64_t in_stride, const float2* hist,
                                                uint32_t n_channels, uint64_t n_in, float2* hist_out)
{
    if (n_channels != 2 && n_channels != 4 && n_channels != 8) return hipErrorInvalidValue;
    hipLaunchKernelGGL(wr::combine_history_kernel, dim3(1), dim3(256), 0, st, reinterpret_cast<const uint2*>(in), in_stride,
                       reinterpret_cast<const uint2*>(hist), n_channels, n_in, reinterpret_cast<uint2*>(hist_out));
    return hipGetLastError();
}
