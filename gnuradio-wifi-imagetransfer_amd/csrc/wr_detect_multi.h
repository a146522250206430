// wr_detect_multi.h -- launch interface of the joint detection over up to 8 sample-synchronous antennas (wr_detect_multi.hip;
// internal, not the C ABI), NUMERICS.md rule 24, and of the row gather behind the stream combiner.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wifirx.h"

#define WR_DET_MAX_ANT 8

namespace wr {

// One joint detection launch, every pointer on the device; the struct travels as the kernel's argument.  The tiles
// [tile0, tile0 + n_tiles) of 64 samples are scanned; every antenna's plane starts at the same stream index and holds n_samp
// samples.  masks [tile], A [n_samp] and P [n_samp] are indexed from the planes' first sample; nothing is written at or behind
// n_samp, and no mask word outside the scanned tiles.
struct DetectMultiArgs {
    const float2* x[WR_DET_MAX_ANT];
    int64_t       n_samp, tile0, n_tiles;
    float         thr;
    uint32_t      n_ant;            // 1 .. 8
    uint64_t*     masks;
    float2*       A;
    float*        P;                // or null
};

// Row gather: frame k's csi row (52 float pairs) and sym_stats row (one float4) are copied from antenna ant[k]'s rows.
struct GatherArgs {
    const float2*  csi[WR_DET_MAX_ANT];
    const float4*  stats[WR_DET_MAX_ANT];
    const uint8_t* ant;             // [n] values below n_ant (the host names them)
    float2*        out_csi;
    float4*        out_stats;
    uint32_t       n, n_ant;
};

}  // namespace wr

extern "C" {
hipError_t wr_launch_stream_detect_multi(hipStream_t st, const wr::DetectMultiArgs* args);
hipError_t wr_launch_row_gather(hipStream_t st, const wr::GatherArgs* args);
}
