// wr_arb.hip -- the rational resampler of NUMERICS.md rule 34: a stream at fs_in into one at fs_out = fs_in den / num through
// a tabulated prototype (4097 entries, 128 per unit of the slower rate, linear interpolation between entries).  The integer
// formats of rule 20 are widened on the way into LDS, so a capture at any rate never exists as float32 in memory.
//
// One workgroup produces a tile of WR_ARB_TILE consecutive outputs, one per lane, so the stores are whole rows.  The tile's
// input span (at most WR_ARB_SPAN samples) is staged once in LDS; samples in front of in[0] come from hist, samples in front
// of the stream are zeros.  The 64-bit arithmetic (m num, the floor division by den) is done once per tile; a lane works in
// 32-bit integers relative to the tile's first input, and along its taps (q, r) fall by the constant 128 den = a S + b.
//
// Rule 35 (the tuner) is the same body with a rotation in the staging loop: tune_kernel runs one grid row per channel, each
// with its own phase ramp over the stream index, so K channels at any centre come out of one capture in one launch.
//
// The table is kept in LDS phase-major, T[p][t] = H[128 t + p] with rows of 33 floats, p = 0 .. 128 (row 128 is row 0
// shifted by one unit), so H[q + 1] is always T[p + 1][t].  The lanes of a decimating ratio hold q that differ by multiples
// of 128 -- one bank in the flat layout; here they are neighbours in a row -- and lanes that differ in p are 33 words apart.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <numeric>

#include "wr_arb.h"
#include "wr_arb_table.h"
#include "wr_device.h"     // sp_sincos_phase (rules 1 and 17)
#include "wr_iq.h"

namespace wr {

namespace {

static_assert(WR_ARB_ENTRIES == 2 * WR_ARB_HALF * WR_ARB_PER_UNIT + 1 && WR_ARB_PER_UNIT == 128 && WR_ARB_HALF == 16, "table geometry");
static_assert(4 * WR_ARB_HALF * 2 == WIFIRX_ARB_HIST_MAX, "32 S / den <= 128 for num <= 4 den");

constexpr uint32_t ARB_ROW = 2 * WR_ARB_HALF + 1;             // 33 floats: 32 units and one word of padding
constexpr uint32_t ARB_ROWS = WR_ARB_PER_UNIT + 1;

const float arb_host_table[WR_ARB_ENTRIES] = WR_ARB_TABLE_INIT;
__device__ const float arb_dev_table[WR_ARB_ENTRIES] = WR_ARB_TABLE_INIT;

// n / d and n % d for n < 2^23, 1 <= d <= 2048, rd = 1.0f / (float)d: the float quotient is off by at most one
__device__ __forceinline__ uint32_t div_small(uint32_t n, uint32_t d, float rd, uint32_t& rem)
{
    uint32_t q = (uint32_t)((float)n * rd);
    int32_t r = (int32_t)n - (int32_t)(q * d);
    if (r < 0) { r += (int32_t)d; q -= 1; }
    else if (r >= (int32_t)d) { r -= (int32_t)d; q += 1; }
    rem = (uint32_t)r;
    return q;
}

}  // namespace

// The one statement of rule 34 on the device: the tile blockIdx.x of a call's outputs into out.  TUNE (rule 35): every staged
// sample -- from in, from hist, a zero of a NULL history or of the front of the stream -- is first multiplied by
// exp(j 2 pi P / 2^64), P = phase0 + inc * (its stream index) mod 2^64, in rule 17's arithmetic; a channel whose inc and
// phase0 are both 0 is not rotated at all and is byte for byte the body without TUNE.
template <int FMT, bool TUNE>
__device__ __forceinline__ void arb_tile(const void* __restrict__ in, const void* __restrict__ hist, float scale, uint64_t n_in,
                                         const wr_arb_ratio& R, uint64_t j0, uint64_t m0, uint64_t n_out, float2* __restrict__ out,
                                         uint64_t inc, uint64_t phase0)
{
    __shared__ float T[ARB_ROWS * ARB_ROW];
    __shared__ __attribute__((aligned(8))) float2 xs[WR_ARB_SPAN];
    const uint32_t tid = threadIdx.x;
    const uint64_t first = (uint64_t)blockIdx.x * WR_ARB_TILE;                   // the tile's first output, of the call's
    const uint32_t count = n_out - first < WR_ARB_TILE ? (uint32_t)(n_out - first) : WR_ARB_TILE;      // its outputs, >= 1

    for (uint32_t i = tid; i < ARB_ROWS * ARB_ROW; i += WR_ARB_TILE) {
        const uint32_t p = i / ARB_ROW, t = i - p * ARB_ROW;
        T[i] = t < 2 * WR_ARB_HALF ? arb_dev_table[WR_ARB_PER_UNIT * t + p] : 0.f;
    }

    // once per tile in 64 bits: N - 16 S of the first output = (jbase - 1) den + rem0, jbase its first input
    const int64_t D0 = (int64_t)((m0 + first) * R.num) - 16 * (int64_t)R.S;
    int64_t fl = D0 / (int64_t)R.den;
    int64_t rem = D0 - fl * (int64_t)R.den;
    if (rem < 0) { rem += R.den; fl -= 1; }                                      // the floor, towards minus infinity
    const int64_t jbase = fl + 1;
    const uint32_t rem0 = (uint32_t)rem;
    const uint32_t span = (rem0 + (count - 1) * R.num + 32 * R.S) / R.den;       // inputs jbase .. jhi of the last output
    const int64_t rel = jbase - (int64_t)j0;                                     // xs[s] is in[rel + s]
    const int64_t lead = jbase < 0 ? -jbase : 0;                                 // xs[s], s < lead, lies in front of the stream
    const bool rotate = TUNE && (inc | phase0) != 0;                             // uniform over the workgroup
    const uint64_t Pbase = phase0 + inc * (uint64_t)jbase;                       // mod 2^64: jbase < 0 wraps
    for (uint32_t s = tid; s < span && s < WR_ARB_SPAN; s += WR_ARB_TILE) {
        const int64_t jj = rel + (int64_t)s;
        float2 x = make_float2(0.f, 0.f);
        if ((int64_t)s >= lead) {
            if (jj >= 0) { if ((uint64_t)jj < n_in) x = load_sample<FMT>(in, (uint64_t)jj, scale); }
            else if (hist && jj >= -(int64_t)R.HL) x = load_sample<FMT>(hist, (uint64_t)(jj + (int64_t)R.HL), scale);
        }
        if (rotate) {
            const uint64_t P = Pbase + inc * s;
            float sn, cs;
            sp_sincos_phase((uint32_t)(P >> 32), sn, cs);
            x = make_float2(x.x * cs - x.y * sn, x.x * sn + x.y * cs);
        }
        xs[s] = x;
    }
    __syncthreads();
    if (tid >= count) return;

    // this lane's output: its first input is xs[dj], B of that input is ((e mod den) + 32 S - den) * 128
    uint32_t em, r;
    const uint32_t dj = div_small(rem0 + tid * R.num, R.den, R.rden, em);
    const uint32_t taps = div_small(em + 32 * R.S, R.den, R.rden, r);
    int32_t q = (int32_t)div_small((em + 32 * R.S - R.den) * 128, R.S, R.rS, r);
    int32_t rr = (int32_t)r;
    if (dj + taps > WR_ARB_SPAN) return;                                         // cannot happen within the rule's limits
    const float2* xp = xs + dj;
    float ar = 0.f, ai = 0.f;
    for (uint32_t k = 0; k < taps; k++) {
        const uint32_t at = ((uint32_t)q & (WR_ARB_PER_UNIT - 1)) * ARB_ROW + ((uint32_t)q >> 7);
        const float h0 = T[at], h1 = T[at + ARB_ROW];
        const float frac = (float)rr * R.rS;
        const float c = h0 + frac * (h1 - h0);
        const float2 x = xp[k];
        const float tr = c * x.x, ti = c * x.y;
        if (k == 0) { ar = tr; ai = ti; }                                        // the sum starts from the first product
        else { ar = ar + tr; ai = ai + ti; }
        q -= (int32_t)R.a;
        rr -= (int32_t)R.b;
        if (rr < 0) { rr += (int32_t)R.S; q -= 1; }
    }
    if (R.num > R.den) { ar = ar * R.gain; ai = ai * R.gain; }
    out[first + tid] = make_float2(ar, ai);
}

template <int FMT>
__global__ __launch_bounds__(WR_ARB_TILE)
void arb_kernel(const void* __restrict__ in, const void* __restrict__ hist, float scale, uint64_t n_in, wr_arb_ratio R,
                uint64_t j0, uint64_t m0, uint64_t n_out, float2* __restrict__ out)
{
    arb_tile<FMT, false>(in, hist, scale, n_in, R, j0, m0, n_out, out, 0, 0);
}

// rule 35: blockIdx.y is the channel; its row starts at out + blockIdx.y * C.out_stride
template <int FMT>
__global__ __launch_bounds__(WR_ARB_TILE)
void tune_kernel(const void* __restrict__ in, const void* __restrict__ hist, float scale, uint64_t n_in, wr_arb_ratio R,
                 uint64_t j0, uint64_t m0, uint64_t n_out, float2* __restrict__ out, wr_tune_channels C)
{
    const uint32_t k = blockIdx.y;
    arb_tile<FMT, true>(in, hist, scale, n_in, R, j0, m0, n_out, out + (uint64_t)k * C.out_stride, C.inc[k], C.phase0[k]);
}

}  // namespace wr

extern "C" bool wr_arb_plan(uint32_t num, uint32_t den, wr_arb_ratio* r)
{
    if (!num || !den || !r) return false;
    const uint32_t g = std::gcd(num, den);
    num /= g;
    den /= g;
    if (den > 512 || num > 2048 || num > 4 * den || den > 4 * num) return false;
    r->num = num;
    r->den = den;
    r->S = num > den ? num : den;
    r->HL = (32 * r->S + den - 1) / den;
    r->a = 128 * den / r->S;
    r->b = 128 * den % r->S;
    r->rS = 1.0f / (float)r->S;
    r->rden = 1.0f / (float)den;
    r->gain = (float)den / (float)r->S;
    return true;
}

extern "C" uint64_t wr_arb_m_end(const wr_arb_ratio* r, uint64_t E)
{
    const int64_t v = (int64_t)(E * r->den) - 16 * (int64_t)r->S;
    return v <= 0 ? 0 : ((uint64_t)v + r->num - 1) / r->num;
}

extern "C" hipError_t wr_launch_arb(hipStream_t st, const void* in, int fmt, float scale, uint64_t n_in, const void* hist,
                                    const wr_arb_ratio* r, uint64_t j0, uint64_t m0, uint64_t n_out, float2* out)
{
    if (n_out == 0) return hipSuccess;
    const uint64_t tiles = (n_out + WR_ARB_TILE - 1) / WR_ARB_TILE;
    if (tiles > 0x7fffffffull) return hipErrorInvalidValue;
    const dim3 grid((uint32_t)tiles), block(WR_ARB_TILE);
    const bool known = wr::iq_dispatch(fmt, [&](auto F) {
        hipLaunchKernelGGL((wr::arb_kernel<decltype(F)::value>), grid, block, 0, st, in, hist, scale, n_in, *r, j0, m0, n_out, out);
    });
    return known ? hipGetLastError() : hipErrorInvalidValue;
}

extern "C" hipError_t wr_launch_tune(hipStream_t st, const void* in, int fmt, float scale, uint64_t n_in, const void* hist,
                                     const wr_arb_ratio* r, uint64_t j0, uint64_t m0, uint64_t n_out, float2* out,
                                     uint32_t n_channels, const wr_tune_channels* c)
{
    if (n_out == 0) return hipSuccess;
    const uint64_t tiles = (n_out + WR_ARB_TILE - 1) / WR_ARB_TILE;
    if (tiles > 0x7fffffffull || n_channels < 1 || n_channels > WIFIRX_TUNE_MAX_CHANNELS) return hipErrorInvalidValue;
    const dim3 grid((uint32_t)tiles, n_channels), block(WR_ARB_TILE);
    const bool known = wr::iq_dispatch(fmt, [&](auto F) {
        hipLaunchKernelGGL((wr::tune_kernel<decltype(F)::value>), grid, block, 0, st, in, hist, scale, n_in, *r, j0, m0, n_out, out, *c);
    });
    return known ? hipGetLastError() : hipErrorInvalidValue;
}

extern "C" const float* wr_arb_host_table(void) { return wr::arb_host_table; }
