// wr_irs.h -- launch interface of the IRS cascade kernel (wr_irs.hip; internal, not the C ABI), and the scene every IRS kernel reads
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace wr {

// the scene of one wifirx_irs_taps / wifirx_irs_taps_multi call, every pointer on the device (NUMERICS.md rules 25 and 27).
// M = n_ant (1..8), N = n_elems, L = n_taps.  The shapes are the multi-antenna ones; at M = 1 they are rule 25's ([n_sets][L],
// rows of 2 N + 1, [n_sets][L][2][N]).
struct IrsArgs {
    float2*        taps_out;      // [M][n_sets][L]
    const float2*  los_a;         // [M][N] line of sight AP antenna m -> surface (A_m); not read when a_los = 0
    const float2*  los_b;         // [N] line of sight surface -> user (B); not read when a_los = 0
    const float2*  los_d;         // [M] line of sight AP antenna m -> user (D_m); always M values (zeros without a direct path)
    const float*   scale;         // [L] s_l = (float)(sqrt(pdp_l) gain)
    const float2*  psi;           // [n_psi_sets][N]; set r uses row r % n_psi_sets.  Not read when align_bits > 0
    const float2*  scatter;       // [n_scatter][(M + 1) N + M] rows (w_a[M][N], w_b[N], w_d[M]), or null: Philox draws
    float2*        elems_out;     // [n_sets][L][M + 1][N] the realised a_0 .. a_{M-1}, b, or null
    uint8_t*       codes_out;     // [n_sets][N] the codes of the aligned mode, or null
    uint64_t       seed;          // key of the draws
    uint32_t       n_ant, n_sets, n_taps, n_elems, n_psi_sets, n_scatter, align_bits;
    float          a_los, a_nlos; // sqrt(K / (K + 1)), sqrt(1 / (K + 1)); a_los = 0: k_factor = 0, neither is applied
    float          direct_gain;   // 0: the direct path is exactly +0 and nothing of it is drawn or read
};

}  // namespace wr

extern "C" {
hipError_t wr_launch_irs(hipStream_t st, const wr::IrsArgs* args);
uint32_t   wr_irs_max_elems(void);
uint32_t   wr_irs_max_taps(void);
uint32_t   wr_irs_max_ant(void);
}

// what every launcher asks of a scene (the entry points refuse these first)
inline bool irs_scene_ok(const wr::IrsArgs& s)
{
    return s.n_elems >= 1 && s.n_elems <= wr_irs_max_elems() && s.n_taps >= 1 && s.n_taps <= wr_irs_max_taps() && s.n_ant >= 1 &&
           s.n_ant <= wr_irs_max_ant() && s.n_sets <= 0x7fffffffu && s.los_d && s.n_scatter >= 1;
}
