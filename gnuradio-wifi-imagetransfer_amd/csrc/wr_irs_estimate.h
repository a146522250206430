// wr_irs_estimate.h -- launch interface of the pilot-based surface estimator (wr_irs_estimate.hip; internal, not the C ABI)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wr_irs.h"

namespace wr {

// one wifirx_irs_estimate call up to the decided phases, every pointer on the device (NUMERICS.md rule 29).  M = n_ant, N = n_elems,
// L = n_taps, R = M L rows per set, T = n_pilots, G = n_groups, J = G + 1.  The taps under the decided phases are a
// wr_launch_irs call on `psi_out`.
struct IrsEstimateArgs {
    IrsArgs         s;            // the scene as wifirx_irs_taps_multi has it; s.align_bits = B (0: nothing is decided), s.codes_out
                                  // [n_sets][G] or null; taps_out, psi, n_psi_sets and elems_out are not looked at
    const float2*   pilot;        // [T][G]: slot t, group g
    const uint16_t* group;        // [N] the group of element n, or null: the identity (G = N)
    const float2*   noise;        // [n_noise][T] rows of w, or null: Philox draws on the counter (t, r, rho, 3)
    float2*         obs;          // [n_sets][R][T] the observations: written by the first kernel, read by the second; never null
    float2*         est_out;      // [n_sets][R][J] the estimate, or null
    float2*         psi_out;      // [n_sets][N] the phases of the decided codes, or null
    uint32_t        n_pilots, n_groups, n_noise;
    float           sigma, kappa;
};

}  // namespace wr

extern "C" {
hipError_t wr_launch_irs_observe(hipStream_t st, const wr::IrsEstimateArgs* args);
hipError_t wr_launch_irs_despread(hipStream_t st, const wr::IrsEstimateArgs* args);
uint32_t   wr_irs_max_pilots(void);
uint32_t   wr_irs_max_groups(void);
}
