// wr_irs_sweep.h -- launch interface of the IRS codebook sweep (wr_irs_sweep.hip; internal, not the C ABI)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wr_irs.h"

namespace wr {

// one wifirx_irs_sweep / wifirx_irs_sweep_multi call, every pointer on the device (NUMERICS.md rules 26 and 28).  K = n_codes.
struct IrsSweepArgs {
    IrsArgs        s;             // the scene; s.taps_out [M][n_sets][L] (the winner's taps) may be null; psi, n_psi_sets, align_bits,
                                  // elems_out and codes_out are not looked at
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
