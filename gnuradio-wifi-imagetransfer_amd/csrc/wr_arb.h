// wr_arb.h -- launch interface of the rational resampler (wr_arb.hip; internal, not the C ABI): one stream at fs_in into one
// at fs_out = fs_in * den / num, NUMERICS.md rule 34.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wifirx.h"

#define WR_ARB_TILE 256         // consecutive outputs that one workgroup produces (one per lane)
// the most input samples a tile reads: fewer than TILE * num / den + 32 S / den + 1 with num / den <= 4 and 32 S / den <= 128
#define WR_ARB_SPAN (WR_ARB_TILE * 4 + WIFIRX_ARB_HIST_MAX + 2)

// The ratio of a call in lowest terms and what the host derives from it (wr_arb_plan).
struct wr_arb_ratio {
    uint32_t num, den;          // the step num / den input samples per output sample, reduced
    uint32_t S;                 // max(num, den)
    uint32_t HL;                // ceil(32 S / den): the input samples a call takes from before its input
    uint32_t a, b;              // 128 den = a S + b, b < S: what (q, r) fall by from one tap to the next
    float rS;                   // 1.0f / (float)S
    float rden;                 // 1.0f / (float)den: the kernel's integer quotients only (they are corrected, so exact)
    float gain;                 // (float)den / (float)S; applied when num > den
};

// The channels of a tuner call (NUMERICS.md rule 35), a kernel argument by value: nothing is uploaded for a call.
struct wr_tune_channels {
    uint64_t inc[WIFIRX_TUNE_MAX_CHANNELS];       // phase increment per input sample, 2^-64 turns
    uint64_t phase0[WIFIRX_TUNE_MAX_CHANNELS];    // phase of stream sample 0
    uint64_t out_stride;                          // float pairs from one channel's row of out to the next
};

extern "C" {
// num / den reduced and checked against rule 34's limits; false outside them (or for a zero)
bool wr_arb_plan(uint32_t num, uint32_t den, wr_arb_ratio* r);
// m_end(E) = max(0, ceil((E den - 16 S) / num)) for E den < 2^62
uint64_t wr_arb_m_end(const wr_arb_ratio* r, uint64_t E);
// The outputs m0 .. m0 + n_out - 1 (n_out > 0) from the n_in samples of `fmt` at in (natural alignment; in[0] is stream sample
// j0) and the HL samples in front of them at hist (null: zeros); out is 8-byte aligned.  Device pointers that do not overlap.
// The caller has checked that every input an output reads lies in [j0 - HL, j0 + n_in) and that (m0 + n_out) num < 2^62.
hipError_t wr_launch_arb(hipStream_t st, const void* in, int fmt, float scale, uint64_t n_in, const void* hist,
                         const wr_arb_ratio* r, uint64_t j0, uint64_t m0, uint64_t n_out, float2* out);
// The same for n_channels = 1 .. 8 channels in one launch, channel k mixed by c->inc[k], c->phase0[k] on the way into LDS and
// written to out + k * c->out_stride (rule 35); the rows of out overlap nothing, each has room for n_out float pairs.
hipError_t wr_launch_tune(hipStream_t st, const void* in, int fmt, float scale, uint64_t n_in, const void* hist,
                          const wr_arb_ratio* r, uint64_t j0, uint64_t m0, uint64_t n_out, float2* out, uint32_t n_channels,
                          const wr_tune_channels* c);
// the 4097 float32 entries of the prototype (host memory, static)
const float* wr_arb_host_table(void);
}
