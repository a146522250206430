// wr_irs_multi.h -- launch interface of the multi-antenna IRS kernels (wr_irs_multi.hip; internal, not the C ABI)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wr_irs.h"

namespace wr {

// one wifirx_irs_taps_multi call, every pointer on the device (NUMERICS.md rule 27).  M = n_ant, N = n_elems, L = n_taps.
struct IrsMultiArgs {
    IrsArgs        s;             // the scene as wifirx_irs_taps has it, with these shapes: taps_out [M][n_sets][L], los_a [M][N],
                                  // scatter [n_scatter][(M + 1) N + M] rows (w_a[M][N], w_b[N], w_d[M]), elems_out
                                  // [n_sets][L][M + 1][N] (a_0 .. a_{M-1}, b); los_d is not looked at
    const float2*  los_d;         // [M] line of sight AP antenna m -> user (D_m); always M values (zeros without a direct path)
    uint32_t       n_ant;         // 1..8
};

// one wifirx_irs_sweep_multi call (NUMERICS.md rule 28).  K = n_codes.
struct IrsSweepMultiArgs {
    IrsMultiArgs   m;             // m.s.taps_out [M][n_sets][L] (the winner's taps) may be null; psi, n_psi_sets, align_bits, elems_out
                                  // and codes_out are not looked at
    const float2*  codebook;      // [K][N]
    uint16_t*      best_out;      // [n_sets] the winning entry, or null
    float*         power_out;     // [n_sets][K] the power of every entry, or null
    uint32_t       n_codes;
};

}  // namespace wr

extern "C" {
hipError_t wr_launch_irs_multi(hipStream_t st, const wr::IrsMultiArgs* args);
hipError_t wr_launch_irs_sweep_multi(hipStream_t st, const wr::IrsSweepMultiArgs* args);
uint32_t   wr_irs_max_ant(void);
}
