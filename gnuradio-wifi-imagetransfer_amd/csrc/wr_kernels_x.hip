// wr_kernels_x.hip -- the demod kernels for every output set but the contract's usual one (XK = true, wr_demod.h): the
// reference's own set -- the equalised points of the `carrier` port (gnu_radio/IRS_AP.py:293,312-313) --, LLRs weighted by the
// channel state, the SNR probe's moments, the bit planes alone (what the stream path asks for), decisions without LLRs.
#include "wr_demod.h"

extern "C" hipError_t wr_launch_demod_batch_x(hipStream_t st, const float2* iq, uint32_t slot_len,
                                              uint32_t n_slots, const wr::DemodParams* prm, const wr::DemodOut* out,
                                              const uint64_t* slot_off)
{
    if (n_slots == 0) return hipSuccess;
    return wr::launch_demod_batch<true>(st, iq, slot_len, n_slots, prm, out, slot_off);
}

extern "C" hipError_t wr_launch_demod_stream_x(hipStream_t st, const float2* x, int64_t n_samp, const wr::StreamTrig* trig,
                                               uint32_t n_trig, const wr::DemodParams* prm, const float2* A, const wr::DemodOut* out)
{
    if (n_trig == 0) return hipSuccess;
    return wr::launch_demod_stream<true>(st, x, n_samp, trig, n_trig, prm, A, out);
}
