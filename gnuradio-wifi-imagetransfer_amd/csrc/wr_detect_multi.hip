// wr_detect_multi.hip -- joint detection over up to 8 sample-synchronous antennas (NUMERICS.md rule 24): the summands of
// rule 3 -- a[n] = x[n] conj(x[n - 16]) and |x[n]|^2 -- are formed per antenna, added over the antennas by a pairwise tree,
// and go through ONE pass of rule 3's blocked window sums and its threshold comparison.  Every antenna of one radio then has
// the same triggers and the same coarse CFO; with one antenna the kernel is stream_detect_kernel bit for bit.
//
// Geometry of stream_detect_kernel (wr_kernels.hip): one wave owns WR_STREAM_SPAN tiles of 64 samples, lane <-> sample, and
// first replays the tile in front of its span for the block sums that tile hands over.  Per tile and antenna a lane makes two
// coalesced 8-byte loads (x[n], x[n - 16]); the window pass with its 15 cross-lane reads is paid once per tile, not per antenna.
// The kernel is bound by memory: per sample it reads 8 n_ant bytes (x[n - 16] comes from the caches) and writes 8 (A) + 4 (P,
// on request) + 1/8 (mask).
#include "wr_demod.h"
#include "wr_detect_multi.h"

namespace wr {

namespace {

// rule 24's tree over the antenna index: neighbours are added level by level, an odd one out moves up as it is --
// NA = 3: (s0 + s1) + s2;  NA = 8: ((s0 + s1) + (s2 + s3)) + ((s4 + s5) + (s6 + s7))
template <int NA>
__device__ __forceinline__ float tree_sum(const float (&s)[NA])
{
    float v[NA];
#pragma unroll
    for (int i = 0; i < NA; i++) v[i] = s[i];
#pragma unroll
    for (int n = NA; n > 1; n = (n + 1) / 2) {
#pragma unroll
        for (int i = 0; i < n / 2; i++) v[i] = v[2 * i] + v[2 * i + 1];
        if (n & 1) v[n / 2] = v[n - 1];
    }
    return v[0];
}

template <int NA>
__device__ __forceinline__ uint64_t detect_multi_tile(const DetectMultiArgs& a, long n0, int lane, DetectState& ps,
                                                      float& Ar, float& Ai, float& P)
{
    const long n = n0 + lane;
    float sr[NA], si[NA], sp[NA];
#pragma unroll
    for (int k = 0; k < NA; k++)
        detect_summands(load_sample(a.x[k], n, (long)a.n_samp), load_sample(a.x[k], n - 16, (long)a.n_samp), sr[k], si[k], sp[k]);
    return detect_tile_windows(tree_sum<NA>(sr), tree_sum<NA>(si), tree_sum<NA>(sp), (long)a.n_samp, n0, a.thr, lane, ps, Ar, Ai, P);
}

}  // namespace

template <int NA>
__global__ __launch_bounds__(256)
void stream_detect_multi_kernel(const DetectMultiArgs a)
{
    const int lane = threadIdx.x & 63;
    const long wave = (long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const long end = (long)(a.tile0 + a.n_tiles);
    const long first = (long)a.tile0 + wave * WR_STREAM_SPAN;
    if (first >= end) return;
    long last = first + WR_STREAM_SPAN;
    if (last > end) last = end;
    DetectState ps = detect_state_zero();
    float Ar, Ai, P;
    if (first > 0) (void)detect_multi_tile<NA>(a, (first - 1) * 64, lane, ps, Ar, Ai, P);
    for (long tl = first; tl < last; tl++) {
        const uint64_t mask = detect_multi_tile<NA>(a, tl * 64, lane, ps, Ar, Ai, P);
        const long n = tl * 64 + lane;
        if (n < (long)a.n_samp) {
            a.A[n] = make_float2(Ar, Ai);
            if (a.P) a.P[n] = P;
        }
        if (lane == 0) a.masks[tl] = mask;
    }
}

// one thread per 16-byte piece of a destination frame: 26 pieces of the csi row, then the sym_stats row
__global__ __launch_bounds__(256)
void row_gather_kernel(const GatherArgs g)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    const uint32_t k = t / 27u, j = t % 27u;
    if (k >= g.n) return;
    const uint32_t r = g.ant[k];
    const float2* csi = g.csi[0];
    const float4* stats = g.stats[0];
#pragma unroll
    for (uint32_t a = 1; a < WR_DET_MAX_ANT; a++) { csi = a == r ? g.csi[a] : csi; stats = a == r ? g.stats[a] : stats; }
    if (j < 26u) reinterpret_cast<float4*>(g.out_csi + (size_t)k * 52u)[j] = reinterpret_cast<const float4*>(csi + (size_t)k * 52u)[j];
    else g.out_stats[k] = stats[k];
}

}  // namespace wr

extern "C" hipError_t wr_launch_stream_detect_multi(hipStream_t st, const wr::DetectMultiArgs* args)
{
    if (args->n_tiles <= 0) return hipSuccess;
    if (args->n_ant < 1 || args->n_ant > WR_DET_MAX_ANT) return hipErrorInvalidValue;
    const int64_t waves = (args->n_tiles + WR_STREAM_SPAN - 1) / WR_STREAM_SPAN;
    const dim3 grid((unsigned)((waves + 3) / 4)), block(256);
    switch (args->n_ant) {
    case 1: hipLaunchKernelGGL(wr::stream_detect_multi_kernel<1>, grid, block, 0, st, *args); break;
    case 2: hipLaunchKernelGGL(wr::stream_detect_multi_kernel<2>, grid, block, 0, st, *args); break;
    case 3: hipLaunchKernelGGL(wr::stream_detect_multi_kernel<3>, grid, block, 0, st, *args); break;
    case 4: hipLaunchKernelGGL(wr::stream_detect_multi_kernel<4>, grid, block, 0, st, *args); break;
    case 5: hipLaunchKernelGGL(wr::stream_detect_multi_kernel<5>, grid, block, 0, st, *args); break;
    case 6: hipLaunchKernelGGL(wr::stream_detect_multi_kernel<6>, grid, block, 0, st, *args); break;
    case 7: hipLaunchKernelGGL(wr::stream_detect_multi_kernel<7>, grid, block, 0, st, *args); break;
    default: hipLaunchKernelGGL(wr::stream_detect_multi_kernel<8>, grid, block, 0, st, *args); break;
    }
    return hipGetLastError();
}

extern "C" hipError_t wr_launch_row_gather(hipStream_t st, const wr::GatherArgs* args)
{
    if (args->n == 0) return hipSuccess;
    const uint64_t threads = (uint64_t)args->n * 27u;
    hipLaunchKernelGGL(wr::row_gather_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, *args);
    return hipGetLastError();
}
