// wr_irs_sweep.h -- launch interface of the IRS codebook sweep (wr_irs_sweep.hip; internal, not the C ABI)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wr_irs.h"

namespace wr {

// one wifirx_irs_sweep call, every pointer on the device (NUMERICS.md rule 26).  N = n_elems, L = n_taps, K = n_codes.
struct IrsSweepArgs {
    IrsArgs        s;             // the scene, as wifirx_irs_taps has it: los_a, los_b, scale, scatter, los_d, seed, n_sets, n_taps,
                                  // n_elems, n_scatter, a_los, a_nlos, direct_gain.  s.taps_out [n_sets][L] (the winner's taps) may
                                  // be null; psi, n_psi_sets, align_bits, elems_out and codes_out are not looked at
    const float2*  codebook;      // [K][N]
    uint16_t*      best_out;      // [n_sets] the winning entry, or null
    float*         power_out;     // [n_sets][K] the power of every entry, or null
    uint32_t       n_codes;
};

}  // namespace wr

extern "C" {
hipError_t wr_launch_irs_sweep(hipStream_t st, const wr::IrsSweepArgs* args);
uint32_t   wr_irs_max_codes(void);
}
