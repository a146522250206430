// wr_diversity.h -- launch interface of the receive-diversity combiner (wr_diversity.hip; internal, not the C ABI): the
// equalised points of up to 8 antennas' demodulated batches into one batch to decode, NUMERICS.md rule 23.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wifirx.h"

#define WR_DIV_MAX_ANT 8

namespace wr {

// one wifirx_diversity_combine call, every pointer on the device; the struct travels as the kernel's argument, so nothing
// is uploaded.  Rows have the layout of wifirx_out for `max_sym`: frames [n_slots], carrier [n_slots][max_sym][48][2],
// csi [n_slots][52][2], idx [n_slots][max_sym][48], llr [n_slots][max_sym * 48 * llr_bits] values.
struct DivArgs {
    const wifirx_frame* frames[WR_DIV_MAX_ANT];
    const float*        carrier[WR_DIV_MAX_ANT];
    const float*        csi[WR_DIV_MAX_ANT];
    float               gain[WR_DIV_MAX_ANT];     // g_a, looked at only when has_gain
    wifirx_frame*       out_frames;
    uint8_t*            out_idx;                  // or null
    void*               out_llr;                  // or null: float32 values, or bf16 bit patterns when llr_bf16
    float*              out_carrier;              // or null
    uint8_t*            used_mask;                // [n_slots] or null
    uint32_t            n_ant, n_slots, max_sym, llr_bits;
    uint32_t            select;                   // 1: WIFIRX_DIV_SELECT
    uint32_t            has_gain, llr_csi, llr_bf16;
};

#if defined(WR_T16_2) && defined(WR_T64_2) && defined(WR_T64_4)
// (for translation units that include wr_quad.h first: the slicer constants and c32 come from there)
// NUMERICS.md rule 7's LLRs of one point for NB bits per carrier, in the order of the row: bit 0 .. NB - 1.
template <int NB>
__device__ __forceinline__ void llr_of_point(c32 y, float (&L)[NB])
{
    const float are = __builtin_fabsf(y.re), aim = __builtin_fabsf(y.im);
    if constexpr (NB == 1) {
        L[0] = y.re;
    } else if constexpr (NB == 2) {
        L[0] = y.re; L[1] = y.im;
    } else if constexpr (NB == 4) {
        L[0] = y.re; L[1] = WR_T16_2 - are; L[2] = y.im; L[3] = WR_T16_2 - aim;
    } else {
        L[0] = y.re; L[1] = WR_T64_4 - are; L[2] = WR_T64_2 - __builtin_fabsf(are - WR_T64_4);
        L[3] = y.im; L[4] = WR_T64_4 - aim; L[5] = WR_T64_2 - __builtin_fabsf(aim - WR_T64_4);
    }
}
#endif

}  // namespace wr

extern "C" {
// n_slots > 0; n_cu sizes the capped grid
hipError_t wr_launch_diversity(hipStream_t st, const wr::DivArgs* args, uint32_t n_cu);
}
