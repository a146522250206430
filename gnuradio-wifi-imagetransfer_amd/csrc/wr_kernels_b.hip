// wr_kernels_b.hip -- the batch demod kernels with bf16 LLR rows (WIFIRX_P_LLR_FORMAT = WIFIRX_LLR_BF16, NUMERICS.md rule 15)
// for the contract's usual output set (XK = false); wr_kernels_bx.hip holds the instances for every other set (XK = true).
// The format is a template parameter of the instances (wr_demod.h, frames_quad), chosen here on the host: DemodParams and
// DemodOut stay as they are, so the float32 instances of wr_kernels.hip / wr_kernels_x.hip keep their kernel arguments and
// their code.  Stream mode has no bf16 instances.
#include "wr_demod.h"

extern "C" hipError_t wr_launch_demod_batch_bf16(hipStream_t st, const float2* iq, uint32_t slot_len,
                                                 uint32_t n_slots, const wr::DemodParams* prm, const wr::DemodOut* out,
                                                 const uint64_t* slot_off)
{
    if (n_slots == 0) return hipSuccess;
    if (wr_demod_wants_x(prm, out)) return wr_launch_demod_batch_bf16_x(st, iq, slot_len, n_slots, prm, out, slot_off);
    return wr::launch_demod_batch<false, true>(st, iq, slot_len, n_slots, prm, out, slot_off);
}
