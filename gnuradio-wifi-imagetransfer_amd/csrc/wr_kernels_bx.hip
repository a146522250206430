// wr_kernels_bx.hip -- the batch demod kernels with bf16 LLR rows for every output set but the usual one (XK = true; see
// wr_kernels_b.hip and wr_kernels_x.hip).
#include "wr_demod.h"

extern "C" hipError_t wr_launch_demod_batch_bf16_x(hipStream_t st, const float2* iq, uint32_t slot_len,
                                                   uint32_t n_slots, const wr::DemodParams* prm, const wr::DemodOut* out,
                                                   const uint64_t* slot_off)
{
    if (n_slots == 0) return hipSuccess;
    return wr::launch_demod_batch<true, true>(st, iq, slot_len, n_slots, prm, out, slot_off);
}
