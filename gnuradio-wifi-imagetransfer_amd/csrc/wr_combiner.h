// wr_combiner.h -- launch interface of the synthesis bank (wr_combiner.hip; internal, not the C ABI): M channel streams at
// fs into one stream at M x fs, NUMERICS.md rule 22.  The mirror of wr_channelizer.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wifirx.h"

#define WR_CB_TILE 512          // input blocks (one sample of every channel) that one workgroup turns into 512 M outputs
#define WR_CB_HIST 23           // samples of every channel in front of a block's own that its outputs read

extern "C" {
// n_in > 0 samples of each of n_channels rows, row k at in + k * in_stride, and the 23 in front of each at hist + 23 k
// (null: zeros), into n_in * n_channels samples at out.  Device pointers, 8-byte aligned, that do not overlap.
// gains: n_channels floats in host memory (they travel as kernel arguments), or null for no multiply.
// m0: the stream index of the call's first block.
hipError_t wr_launch_combine(hipStream_t st, const float2* in, uint64_t in_stride, const float* gains, const float2* hist,
                             uint32_t n_channels, int stacking, uint64_t n_in, uint64_t m0, float2* out);
// the last 23 samples of (hist || in) of every row into hist_out + 23 k; n_in may be 0; hist null: zeros
hipError_t wr_launch_combine_history(hipStream_t st, const float2* in, uint64_t in_stride, const float2* hist,
                                     uint32_t n_channels, uint64_t n_in, float2* hist_out);
}
