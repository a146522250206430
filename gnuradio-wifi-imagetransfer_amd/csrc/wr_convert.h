// wr_convert.h -- launch interface of the sample-format converters (wr_convert.hip; internal, not the C ABI): integer IQ
// pairs (sc16 / sc8) to float pairs and back, NUMERICS.md rule 20.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wifirx.h"

// bytes of one sample (I and Q) in an integer format; 0 for anything else (WIFIRX_IQ_FC32 included: nothing to convert)
static inline uint32_t wr_iq_sample_bytes(int fmt) { return fmt == WIFIRX_IQ_SC16 ? 4u : fmt == WIFIRX_IQ_SC8 ? 2u : 0u; }

extern "C" {
// n > 0 samples of `fmt` at src (natural alignment: 4 bytes sc16, 2 bytes sc8) -> float pairs at dst (8-byte aligned), each
// component (float)q * scale.  Device pointers that do not overlap; n_cu sizes the grid.
hipError_t wr_launch_iq_widen(hipStream_t st, const void* src, int fmt, uint64_t n, float scale, float2* dst, uint32_t n_cu);
// n > 0 float pairs at src (8-byte aligned) -> samples of `fmt` at dst (natural alignment), quantised to `bits` bits.
// count: null, or a device counter the clipped components are added to (one 64-bit atomic add per workgroup).
hipError_t wr_launch_iq_quantise(hipStream_t st, const float2* src, uint64_t n, float scale, int fmt, uint32_t bits, void* dst,
                                 unsigned long long* count, uint32_t n_cu);
}
