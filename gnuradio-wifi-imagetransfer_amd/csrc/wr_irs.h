// wr_irs.h -- launch interface of the IRS cascade kernel (wr_irs.hip; internal, not the C ABI)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace wr {

// one wifirx_irs_taps call, every pointer on the device (NUMERICS.md rule 25).  N = n_elems, L = n_taps.
struct IrsArgs {
    float2*        taps_out;      // [n_sets][L]
    const float2*  los_a;         // [N] line of sight AP -> surface (A); not read when a_los = 0
    const float2*  los_b;         // [N] line of sight surface -> user (B); not read when a_los = 0
    const float*   scale;         // [L] s_l = (float)(sqrt(pdp_l) gain)
    const float2*  psi;           // [n_psi_sets][N]; set r uses row r % n_psi_sets.  Not read when align_bits > 0
    const float2*  scatter;       // [n_scatter][2 N + 1] rows (w_a[N], w_b[N], w_d), or null: Philox draws
    float2*        elems_out;     // [n_sets][L][2][N] the realised a_n, b_n, or null
    uint8_t*       codes_out;     // [n_sets][N] the codes of the aligned mode, or null
    float2         los_d;         // line of sight AP -> user (D)
    uint64_t       seed;          // key of the draws
    uint32_t       n_sets, n_taps, n_elems, n_psi_sets, n_scatter, align_bits;
    float          a_los, a_nlos; // sqrt(K / (K + 1)), sqrt(1 / (K + 1)); a_los = 0: k_factor = 0, neither is applied
    float          direct_gain;   // 0: the direct path is exactly +0 and nothing of it is drawn or read
};

}  // namespace wr

extern "C" {
hipError_t wr_launch_irs(hipStream_t st, const wr::IrsArgs* args);
uint32_t   wr_irs_max_elems(void);
uint32_t   wr_irs_max_taps(void);
}
