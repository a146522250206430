// wr_irs_optimize.h -- launch interface of the joint phase decision over antennas and taps (wr_irs_optimize.hip; internal, not the
// C ABI)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace wr {

#define OPT_START_REF   0          // WIFIRX_IRS_START_*: where the ascent starts
#define OPT_START_GIVEN 1
#define OPT_START_ZERO  2

// one wifirx_irs_optimize or wifirx_irs_optimize_weighted call, every pointer on the device (NUMERICS.md rules 30 and 31).
// R = n_rows, J = n_cols, G = J - 1, N = n_elems
struct IrsOptimizeArgs {
    const float2*   coef;         // [n_sets][R][J]: column 0 the direct term, column g + 1 group g (wifirx_irs_estimate's est_out)
    const uint8_t*  codes_in;     // [n_sets][G] the start codes of OPT_START_GIVEN (only their low `bits` bits count), or null
    const uint16_t* group;        // [N] the group of element n, or null: the identity (N = G); read for psi_out only
    uint8_t*        codes_out;    // [n_sets][G] or null
    float2*         psi_out;      // [n_sets][N] the phases of the final codes, or null
    float*          power_out;    // [n_sets][max_sweeps + 1] or null
    uint8_t*        sweeps_out;   // [n_sets] the number of sweeps that changed a code, or null
    uint32_t        n_sets, n_rows, n_cols, n_elems, bits, max_sweeps, start;
    int             blocked;      // the direct path is blocked: d = +0 and column 0 is not read
    uint32_t        n_weight_sets; // 1 or n_sets: set r reads row block r % n_weight_sets of `weight`
    const float*    weight;       // [n_weight_sets][R] the rows' weights (rule 31), or null: unweighted (rule 30)
};

}  // namespace wr

extern "C" {
hipError_t wr_launch_irs_optimize(hipStream_t st, const wr::IrsOptimizeArgs* args);
uint32_t   wr_irs_max_rows(void);
uint32_t   wr_irs_max_sweeps(void);
}
