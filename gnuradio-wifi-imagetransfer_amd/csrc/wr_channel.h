// wr_channel.h -- launch interface of the channel kernel (wr_channel.hip; internal, not the C ABI)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace wr {

// one wifirx_channel call, every pointer on the device.  Sample g of the buffers lies at in[g] / out[g].  Tiles are cut per
// row on pair-aligned output indices: tile k of row r covers [a_r + k CH_TILE, a_r + (k+1) CH_TILE) clipped to the row, with
// a_r = the row start rounded down so that (a_r + shift) is even (shift = 1 when `out` is 8 but not 16 bytes aligned).
struct ChanArgs {
    const float2*   in;
    float2*         out;
    const float2*   taps;         // [n_tap_sets][n_taps]; row r uses set r % n_tap_sets
    const float*    cfo;          // [n_rows] rad/sample, or null: 0
    const uint64_t* row_off;      // [n_rows + 1] or null: row r = [r row_len, (r+1) row_len)
    const uint64_t* tile_base;    // row_off form: [n_rows + 1] first tile of every row (tiles of row r: [tile_base[r], tile_base[r+1]))
    uint64_t        row_len, tiles_per_row;       // fixed-row form
    uint64_t        phase0, seed, sample0;
    uint32_t        n_rows, n_taps, n_tap_sets;
    int32_t         shift;
    float           gain, noise;
    const int64_t*  dinc;         // [n_rows] drift per sample in 2^-40 samples (NUMERICS.md rule 18), or null: no resampler
    int64_t         drift0;       // drift of every row's first output sample, 2^-40 samples
    const float*    doppler;      // [n_rows] Doppler in cycles per sample (NUMERICS.md rule 19), or null: no fading
    uint64_t        fade_seed;    // key of the fader's draws
    uint64_t        time0;        // stream time of every row's first output sample: the gains' grid lies on time0 + n
    float           a_los, a_nlos;      // sqrt(K / (K + 1)), sqrt(1 / (K + 1)); a_los = 0: k_factor = 0, neither is applied
};

#ifdef __HIPCC__
// rule 17: plain float32 products and sums, no fma (-ffp-contract=off keeps them apart)
__device__ __forceinline__ float2 ch_mul(float2 a, float2 b)
{
    return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}

__device__ __forceinline__ float2 ch_add(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
#endif

}  // namespace wr

extern "C" {
hipError_t wr_launch_channel(hipStream_t st, const wr::ChanArgs* args, uint64_t n_tiles);
uint32_t   wr_channel_tile_samples(void);
uint32_t   wr_channel_fade_taps(void);             // the most taps with fading
const float* wr_resample_table(uint32_t* n_phases, uint32_t* n_taps);      // host copy of the rule-18 table, [n_phases + 1][n_taps]
}
