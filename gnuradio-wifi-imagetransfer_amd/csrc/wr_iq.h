// wr_iq.h -- the sample formats of NUMERICS.md rule 20 as the kernels read them, and as their launchers pick the kernel of one
// (internal; wr_convert.hip, wr_frontend.hip, wr_channelizer.hip, wr_arb.hip, wr_spectrum.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "wifirx.h"

namespace wr {

namespace {

// A lane's piece is 16 bytes: G samples of BYTES bytes each (fc32 is a format here; the converters never instantiate it).
template <int FMT> struct Format;
template <> struct Format<WIFIRX_IQ_FC32> { static constexpr uint32_t G = 2, BYTES = 8; };
template <> struct Format<WIFIRX_IQ_SC16> { static constexpr uint32_t G = 4, BYTES = 4; };
template <> struct Format<WIFIRX_IQ_SC8>  { static constexpr uint32_t G = 8, BYTES = 2; };

// The 16 bytes of a lane's piece, declared at the format's natural alignment, which is all a caller's buffer promises: the
// compiler still moves it with one 16-byte instruction, and the hardware takes that at any such address.  (The stream places
// its own scratch copy so that the pieces lie on 16-byte boundaries, wifirx_api_stream.inc.)
template <int FMT> struct __attribute__((packed, aligned(Format<FMT>::BYTES))) Piece { uint32_t w[4]; };

// sample s of a buffer, widened by rule 20: (float)q * scale, one multiply per component; natural alignment
template <int FMT>
__device__ __forceinline__ float2 load_sample(const void* p, uint64_t s, float scale)
{
    if constexpr (FMT == WIFIRX_IQ_FC32) {
        return static_cast<const float2*>(p)[s];
    } else if constexpr (FMT == WIFIRX_IQ_SC16) {
        const uint32_t w = static_cast<const uint32_t*>(p)[s];
        return make_float2((float)(int16_t)(w & 0xffffu) * scale, (float)(int16_t)(w >> 16) * scale);
    } else {
        const uint32_t w = static_cast<const uint16_t*>(p)[s];
        return make_float2((float)(int8_t)(w & 0xffu) * scale, (float)(int8_t)(w >> 8) * scale);
    }
}

// Host side: a run-time fmt as a compile-time one.  f(std::integral_constant<int, FMT>{}) for the launchers that take all
// three formats; false for an fmt that is none of them.
template <class F>
bool iq_dispatch(int fmt, F&& f)
{
    if (fmt == WIFIRX_IQ_FC32) f(std::integral_constant<int, WIFIRX_IQ_FC32>{});
    else if (fmt == WIFIRX_IQ_SC16) f(std::integral_constant<int, WIFIRX_IQ_SC16>{});
    else if (fmt == WIFIRX_IQ_SC8) f(std::integral_constant<int, WIFIRX_IQ_SC8>{});
    else return false;
    return true;
}

}  // namespace

}  // namespace wr
