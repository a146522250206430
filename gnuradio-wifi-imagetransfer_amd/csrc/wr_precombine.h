// wr_precombine.h -- launch interface of the pre-detection combiner (wr_precombine.hip; internal, not the C ABI): the samples
// of up to 8 antennas into one row set in front of the demodulator, NUMERICS.md rule 33.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define WR_PRE_MAX_ANT   8
#define WR_PRE_MAX_ITERS 4

namespace wr {

// one wifirx_precombine call, every pointer on the device; the struct travels as the kernel's argument, so nothing is
// uploaded.  Rows: x[a] and out [n_slots][slot_len] pairs, weights [n_slots][n_ant] pairs, stats [n_slots] rows of 16 bytes
// (float lambda, float trace, uint32 ref, uint32 flags).
struct PreArgs {
    const float2* x[WR_PRE_MAX_ANT];
    float2*       out;
    float2*       weights;      // or null
    uint2*        stats;        // or null: two per row
    uint32_t      n_ant, slot_len, n_slots, iters;
};

}  // namespace wr

extern "C" {
// n_slots > 0, n_ant = 1 .. 8, slot_len a multiple of 64, iters <= 4: one workgroup per slot
hipError_t wr_launch_precombine(hipStream_t st, const wr::PreArgs* args);
}
