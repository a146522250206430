// wr_link.h -- launch interface of the two ends of the device loop-back (wr_link.hip; internal, not the C ABI):
// ieee802_11.mac for a batch of payloads, and the scoring of a decoded batch against what was sent.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wifirx.h"

namespace wr {

// one wifirx_mac_batch call, every pointer on the device
struct MacArgs {
    const uint8_t*  payload;      // frame i at payload + i * payload_stride, or null: Philox bytes keyed by `seed`
    const uint32_t* len;          // [n_frames] payload lengths, or null: len_all for every frame
    uint8_t*        psdu;         // frame i at psdu + i * psdu_stride
    uint64_t        seed;
    uint32_t        payload_stride, psdu_stride, len_all, n_frames, seq0;
    uint32_t        len_max;      // longest payload of the call
    uint32_t        pitch;        // LDS row pitch in dwords (odd; holds the longest PSDU of the call at any byte alignment + 1)
    uint32_t        fpb;          // frames per workgroup (<= 64: one lane per frame runs the CRC)
    uint32_t        hdr[6];       // the 24 bytes of the MAC header with sequence number 0, little endian words
};

// one wifirx_link_stats or wifirx_link_stats_by_rate call, every pointer on the device.  Decision rows are compared as dwords: the first 2 n_bpsc n_sym
// of a frame's row for hbits (two words per coded bit of a carrier and symbol), the first 12 n_sym for idx (48 bytes per
// symbol, whatever the rate).
struct LinkArgs {
    const wifirx_frame* rx_frames;
    const wifirx_frame* ref_frames;
    const uint8_t*      rx_psdu;      // both null, or both given
    const uint8_t*      ref_psdu;
    const uint32_t*     rx_dec;       // both null, or both given: the idx rows, or the hbits rows
    const uint32_t*     ref_dec;
    uint32_t*           frame_err;    // [n_slots] or null
    uint8_t*            frame_class;  // [n_slots] or null
    unsigned long long* counts;       // [9], zeroed by the caller: the fields of wifirx_link_counts in order; by_rate: [9 * 9],
                                      // the totals and behind them the same nine per encoding 0..7 of the reference record
    uint32_t            rx_psdu_stride, ref_psdu_stride;
    uint32_t            dec_row_words;    // dwords per frame row of rx_dec / ref_dec (max_sym * 12)
    uint32_t            dec_is_hbits;
    uint32_t            max_sym, n_slots;
    uint32_t            by_rate;
};

}  // namespace wr

extern "C" {
hipError_t wr_launch_mac(hipStream_t st, const wr::MacArgs* args);
hipError_t wr_launch_link_stats(hipStream_t st, const wr::LinkArgs* args, uint32_t n_simd);
// LDS geometry of a wifirx_mac_batch call whose longest PSDU has max_psdu bytes
void       wr_mac_geometry(uint32_t max_psdu, uint32_t* pitch, uint32_t* fpb);
}
