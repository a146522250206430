// wr_bank.h -- what the two filter banks share on the device (internal; wr_channelizer.hip of NUMERICS.md rule 21 and
// wr_combiner.hip of rule 22): the tile geometry, rule 21's tables, the radix-2 network and the window body.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wr_channelizer_table.h"

namespace wr {

namespace {

// A workgroup works on a tile of 512 blocks (a block: one sample of every channel), two adjacent blocks per lane, with the 23
// blocks in front of the tile: M LDS planes [branch][block - first + 23] of float2, even, so every plane starts on 16 bytes.
constexpr uint32_t BANK_TILE = 512, BANK_HIST = 23;
constexpr uint32_t BANK_THREADS = BANK_TILE / 2, BANK_P = WR_CZ_TAPS_PER_BRANCH, BANK_PLANE = BANK_TILE + BANK_HIST + 1;
static_assert(BANK_P == BANK_HIST + 1 && BANK_PLANE % 2 == 0, "tile geometry");

// rule 21's tables; rule 22 uses the taps times M and the complex conjugates of the constants
template <int M> struct Tables;
#define WR_BANK_TABLES(M_)                                                                    \
    __device__ const float bank_taps##M_[BANK_P * M_] = WR_CZ_TAPS##M_##_INIT;                \
    __device__ const float bank_branch##M_[2 * M_] = WR_CZ_BRANCH##M_##_INIT;                 \
    __device__ const float bank_twiddle##M_[M_] = WR_CZ_TWIDDLE##M_##_INIT;                   \
    template <> struct Tables<M_> {                                                           \
        static __device__ __forceinline__ float tap(int i) { return bank_taps##M_[i]; }       \
        static __device__ __forceinline__ float2 branch(int q) { return make_float2(bank_branch##M_[2 * q], bank_branch##M_[2 * q + 1]); } \
        static __device__ __forceinline__ float2 twiddle(int t) { return make_float2(bank_twiddle##M_[2 * t], bank_twiddle##M_[2 * t + 1]); } \
    };
WR_BANK_TABLES(2)
WR_BANK_TABLES(4)
WR_BANK_TABLES(8)
#undef WR_BANK_TABLES

// Two float pairs as one 16-byte access, declared at the 8 bytes that a row or an interleaved stream promises (as wr_iq.h's
// Piece: one instruction, taken by the hardware at any such address).
struct __attribute__((packed, aligned(8))) Pair2 { float v[4]; };

// rule 17's plain complex product
__device__ __forceinline__ float2 bank_mul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ __forceinline__ float2 bank_conj(float2 a) { return make_float2(a.x, -a.y); }

constexpr int bank_bitrev(int j, int bits)
{
    int r = 0;
    for (int i = 0; i < bits; i++) r |= ((j >> i) & 1) << (bits - 1 - i);
    return r;
}
constexpr int bank_log2(int m) { return m == 2 ? 1 : m == 4 ? 2 : 3; }

// The M-point DFT (INV: inverse DFT, the conjugate twiddles) in place on a, which holds its input in bit-reversed order:
// radix 2, decimation in time; W = 1 is not multiplied and W = -+j is a swap and a sign.
template <int M, bool INV>
__device__ __forceinline__ void radix2(float2 (&a)[M])
{
#pragma unroll
    for (int len = 2; len <= M; len *= 2) {
#pragma unroll
        for (int base = 0; base < M; base += len) {
#pragma unroll
            for (int t = 0; t < len / 2; t++) {
                const int e = t * (M / len);
                const float2 b = a[base + t + len / 2];
                const float2 x = e == 0 ? b
                               : 4 * e == M ? (INV ? make_float2(-b.y, b.x) : make_float2(b.y, -b.x))
                                            : bank_mul(INV ? bank_conj(Tables<M>::twiddle(e)) : Tables<M>::twiddle(e), b);
                const float2 lo = a[base + t];
                a[base + t] = make_float2(lo.x + x.x, lo.y + x.y);
                a[base + t + len / 2] = make_float2(lo.x - x.x, lo.y - x.y);
            }
        }
    }
}

// The 24-tap sums of one branch for a lane's two adjacent blocks a and a + 1: row points at block a - 23 of the branch's
// plane, and the two windows share 23 of the 25 blocks a - 23 .. a + 1, read as twelve 16-byte pieces and one 8-byte piece.
// tap[p] is the caller's factor of block a - p (and a + 1 - p); the sums run in ascending p from the p = 0 product.
__device__ __forceinline__ void window_sums(const float2* row, const float (&tap)[BANK_P], float2& out_a, float2& out_b)
{
    float2 w[BANK_P + 1];                                                        // w[j] = block a - 23 + j
    const float4* p4 = reinterpret_cast<const float4*>(row);
#pragma unroll
    for (uint32_t j = 0; j < BANK_P / 2; j++) {
        const float4 t = p4[j];
        w[2 * j] = make_float2(t.x, t.y);
        w[2 * j + 1] = make_float2(t.z, t.w);
    }
    w[BANK_P] = row[BANK_P];
    float2 sa, sb;
#pragma unroll
    for (uint32_t p = 0; p < BANK_P; p++) {
        const float g = tap[p];
        const float2 xa = w[BANK_P - 1 - p], xb = w[BANK_P - p];
        const float2 ta = make_float2(g * xa.x, g * xa.y), tb = make_float2(g * xb.x, g * xb.y);
        sa = p == 0 ? ta : make_float2(sa.x + ta.x, sa.y + ta.y);
        sb = p == 0 ? tb : make_float2(sb.x + tb.x, sb.y + tb.y);
    }
    // Both sums exist here, and a caller that goes through its branches one by one has only one branch's window in registers
    // at a time.  Without the two lines below the compiler sinks the second block's sums into the branch that stores them and
    // keeps all M windows alive for that (256 VGPRs and copies in AGPRs at M = 8).
    asm volatile("" : "+v"(sa.x), "+v"(sa.y), "+v"(sb.x), "+v"(sb.y));
    __builtin_amdgcn_sched_barrier(0);
    out_a = sa;
    out_b = sb;
}

}  // namespace

}  // namespace wr
