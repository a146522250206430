// wr_channelizer.h -- launch interface of the analysis bank (wr_channelizer.hip; internal, not the C ABI): one wideband
// stream of M x fs into M channel streams at fs, NUMERICS.md rule 21.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wifirx.h"

#define WR_CZ_TILE 512          // outputs per channel that one workgroup produces (two per lane)
#define WR_CZ_HIST 23           // input blocks of M samples in front of an output's own block that it reads

extern "C" {
// n_out > 0 outputs per channel from the n_out * M samples of `fmt` at in (natural alignment) and the 23 * M samples in front
// of them at hist (null: zeros); channel k goes to out + k * out_stride (8-byte aligned).  Device pointers that do not overlap.
// scale: rule 20's widening factor of the integer formats.  m0: the stream index of the call's first output.
hipError_t wr_launch_channelize(hipStream_t st, const void* in, int fmt, float scale, const void* hist, uint32_t n_channels,
                                int stacking, uint64_t n_out, uint64_t m0, float2* out, uint64_t out_stride);
// the 24 * n_channels float32 taps of the prototype (host memory, static); null for n_channels outside {2, 4, 8}
const float* wr_channelizer_taps(uint32_t n_channels);
}
