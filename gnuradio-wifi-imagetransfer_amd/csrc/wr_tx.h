// wr_tx.h -- launch interface of the transmitter kernel (wr_tx.hip; internal, not the C ABI)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace wr {

// one wifirx_tx_batch or wifirx_tx_batch_rates call, every pointer on the device.  Output sample g lies at out[g]; the kernel writes the samples
// [g0, g1) -- the rows, back to back -- and nothing else.  shift = 1 when `out` is 8 but not 16 bytes aligned: the 16-byte
// stores then cover the samples (2 k - 1, 2 k).  v0 = the first such pair's index + shift, rounded down to even.
struct TxArgs {
    const uint8_t*  psdu;       // frame i at psdu + i * psdu_stride
    const uint32_t* len;        // [n_frames] PSDU bytes, 1..4095
    const uint8_t*  seeds;      // [n_frames] scrambler seeds 1..127, or null: (i % 127) + 1
    const uint64_t* row_off;    // [n_frames + 1] or null: row i = [i row_len, (i+1) row_len)
    const uint32_t* tile_row;   // row_off form: the row of the first sample of every tile
    float2*         out;
    uint64_t        psdu_stride, row_len;
    int64_t         g0, g1, v0, shift;
    uint32_t        n_frames, lead;
    uint32_t        enc, n_bpsc, n_cbps, n_dbps, rate_field;
    const uint8_t*  enc_v;      // [n_frames] one encoding per frame (wifirx_tx_batch_rates), or null: `enc` .. `rate_field`
};                              // hold for every frame.  With enc_v those five are not read


}  // namespace wr

extern "C" {
hipError_t wr_launch_tx(hipStream_t st, const wr::TxArgs* args);
uint32_t   wr_tx_tile_samples(void);
}
