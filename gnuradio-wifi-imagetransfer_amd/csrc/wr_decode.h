// wr_decode.h -- what the hard (wr_decode.hip) and soft (wr_decode_soft.hip) decode_mac kernels share: the rates, where a
// coded bit sits in an OFDM symbol, and the per-frame finish (descramble, bytes, CRC-32).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wifirx.h"

namespace wr {

// per rate (SIGNAL encoding 0..7): data bits per OFDM symbol, coded bits per carrier, puncturing (0 = 1/2, 1 = 2/3,
// 2 = 3/4), bit-plane words per symbol (wifirx_out.hbits: two per coded bit of a carrier).  n_dbps comes from a table in
// constant memory (one load; as a select chain it compiled to a branch tree in front of frame_steps' division, 17 more
// registers in decode_pack_kernel); the others are select chains.
constexpr int RATE_NDBPS[8] = { 24, 36, 48, 72, 96, 144, 192, 216 };
constexpr __host__ __device__ int ndbps_of(int enc) { return RATE_NDBPS[enc]; }
constexpr __host__ __device__ int nbpsc_of(int enc) { return enc < 2 ? 1 : enc < 4 ? 2 : enc < 6 ? 4 : 6; }
constexpr __host__ __device__ int punct_of(int enc) { return enc == 6 ? 1 : (enc & 1) ? 2 : 0; }
constexpr __host__ __device__ int words_per_sym(int enc) { return 2 * nbpsc_of(enc); }

// Trellis steps of a frame decode_mac accepts (n_sym * n_dbps, a multiple of 12), 0 for a frame it leaves alone.  The one
// rule for which frames get decoded: the pre-pass (decode_maxsteps_kernel, with a cap that cannot bind) counts the frames it
// accepts per rate and sets n_steps_cap to their longest trellis, decode_perm_kernel groups exactly those frames by rate,
// and every decode kernel takes exactly those frames.  So a frame the pre-pass counts is a frame the kernels decode, and
// every task of the throughput kernels (decode_kernel, decode_q_kernel, the soft kernel) holds frames of one rate -- they
// read the task's rate from its first active lane.  (The soft kernel adds two conditions, soft_frame_steps: the pre-pass
// still counts the frames it leaves alone.)
__device__ __forceinline__ int frame_steps(uint32_t flags, int enc, int len, uint32_t psdu_stride, uint32_t max_sym,
                                           uint32_t n_steps_cap)
{
    const int n_dbps = ndbps_of(enc & 7);
    const int n_sym = (16 + 8 * len + 6 + n_dbps - 1) / n_dbps;
    const bool ok = (flags & WIFIRX_F_COMPLETE) && len <= (int)psdu_stride && len <= WIFIRX_MAX_PSDU &&
                    n_sym <= WIFIRX_MAX_SYM && n_sym <= (int)max_sym && (uint32_t)(n_sym * n_dbps) <= n_steps_cap;
    return ok ? n_sym * n_dbps : 0;
}

// Where the coded bit at position `ci` of the de-punctured stream of ONE OFDM symbol was received: de-puncturing, then
// the de-interleaver, give its index among the symbol's 48 * n_bpsc coded bits (carrier * n_bpsc + bit), or -1 when the
// transmitter dropped it.  Every symbol carries 2 * n_dbps de-punctured positions and exactly 48 * n_bpsc transmitted
// bits, so the map repeats from symbol to symbol.
constexpr int coded_index(int punct, int n_bpsc, int ci)
{
    const int n_cbps = 48 * n_bpsc;
    const int s = (n_bpsc / 2) < 1 ? 1 : (n_bpsc / 2);
    int k = ci;
    if (punct == 1) {                      // 2/3: every 4th bit dropped
        const int r = ci & 3;
        if (r == 3) return -1;
        k = (ci >> 2) * 3 + r;
    } else if (punct == 2) {               // 3/4: bits 3,4 of every 6 dropped
        const int g = ci / 6, r = ci - 6 * g;
        if (r == 3 || r == 4) return -1;
        k = g * 4 + (r < 3 ? r : 3);
    }
    const int i = (n_cbps >> 4) * (k & 15) + (k >> 4);
    return s * (i / s) + (i + n_cbps - (16 * i) / n_cbps) % s;
}

constexpr __host__ __device__ int rotr6(int s, int p) { return ((s >> p) | (s << (6 - p))) & 63; }
constexpr __host__ __device__ int parity_of(int v) { return __builtin_popcount(v) & 1; }

// Per-rate tables of one OFDM symbol: entry [enc][step tt of the symbol] = entry(n_bpsc, j) of coded bit 2 tt in the low half
// and of coded bit 2 tt + 1 in the high half, where j is the bit's coded_index (-1: dropped by the transmitter, and for the
// steps past the rate's n_dbps).
constexpr int RATE_TAB_STRIDE = 216;      // steps per OFDM symbol at the highest rate
struct RateTable { uint32_t e[8 * RATE_TAB_STRIDE]; };
template <typename Entry>
constexpr RateTable make_rate_table(Entry entry)
{
    RateTable t{};
    for (int enc = 0; enc < 8; enc++)
        for (int tt = 0; tt < RATE_TAB_STRIDE; tt++) {
            const int nb = nbpsc_of(enc), pu = punct_of(enc);
            const bool in = tt < ndbps_of(enc);
            const int ja = in ? coded_index(pu, nb, 2 * tt) : -1, jb = in ? coded_index(pu, nb, 2 * tt + 1) : -1;
            t.e[enc * RATE_TAB_STRIDE + tt] = entry(nb, ja) | (entry(nb, jb) << 16);
        }
    return t;
}

// Tables of the per-frame finish (workgroup LDS, built once per workgroup): crc[k][b] = CRC-32 (reflected 0xedb88320)
// of byte b followed by k zero bytes ("slicing by 4"), scr[s] = the next 32 scrambler bits from LFSR state s.
struct FinishTables { uint32_t crc[4][256]; uint32_t scr[128]; };

__device__ __forceinline__ void build_finish_tables(FinishTables& ft)
{
    for (int e = threadIdx.x; e < 256; e += blockDim.x) {
        uint32_t c = (uint32_t)e;
#pragma unroll
        for (int k = 0; k < 8; k++) c = (c >> 1) ^ (0xedb88320u & (0u - (c & 1u)));
        ft.crc[0][e] = c;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < 256; e += blockDim.x) {
        uint32_t c = ft.crc[0][e];
        for (int k = 1; k < 4; k++) { c = (c >> 8) ^ ft.crc[0][c & 0xffu]; ft.crc[k][e] = c; }
    }
    for (int e = threadIdx.x; e < 128; e += blockDim.x) {
        int state = e;
        uint32_t w = 0;
        for (int k = 0; k < 32; k++) {
            const int fb = ((state >> 6) ^ (state >> 3)) & 1;
            state = ((state << 1) & 0x7e) | fb;
            w |= (uint32_t)fb << k;
        }
        ft.scr[e] = w;
    }
    __syncthreads();
}

// descramble (x^7+x^4+1, state from the first 7 decoded bits), bytes, CRC-32 of one frame; db = its decoded words
// (word k = decoded bits 32 k .. 32 k + 31, stride DBS dwords, two spare words behind the last one).  Four PSDU bytes per
// iteration: the 32 decoded bits from position 16 + 32 k on (a funnel shift of two decoded words), the 32 scrambler bits
// from the table (the state after them is their last seven, reversed), CRC by four table look-ups.  Bytes leave four at a
// time when the row is dword-aligned (wave-uniform `dword_ok`).
template <int DBS = 128>
__device__ __forceinline__ void finish_frame(const uint32_t* __restrict__ db, int psdu_len, uint8_t* __restrict__ psdu,
                                             bool dword_ok, wifirx_frame* __restrict__ rec, uint32_t flags,
                                             const FinishTables& ft)
{
    uint32_t cur = db[0];
    int state = 0;
#pragma unroll
    for (int i = 0; i < 7; i++) state |= (int)((cur >> i) & 1) << (6 - i);
    // positions 7..15 belong to the SERVICE field: advance the scrambler
#pragma unroll
    for (int i = 7; i < 16; i++) {
        int fb = ((state >> 6) ^ (state >> 3)) & 1;
        state = ((state << 1) & 0x7e) | fb;
    }
    uint32_t crc = 0xffffffffu;
    uint32_t nxt = db[DBS];
    const int n_words = psdu_len >> 2;
    for (int k = 0; k < n_words; k++) {
        const uint32_t nn = db[(size_t)(k + 2) * DBS];                     // spare words behind the last one keep this in range
        const uint32_t sc = ft.scr[state];
        state = (int)(__builtin_bitreverse32(sc) & 0x7fu);
        const uint32_t d = __builtin_amdgcn_alignbit(nxt, cur, 16) ^ sc;    // positions 16 + 32 k .. + 31, descrambled
        cur = nxt; nxt = nn;
        if (dword_ok) *reinterpret_cast<uint32_t*>(psdu + 4 * k) = d;
        else { psdu[4 * k] = (uint8_t)d; psdu[4 * k + 1] = (uint8_t)(d >> 8); psdu[4 * k + 2] = (uint8_t)(d >> 16); psdu[4 * k + 3] = (uint8_t)(d >> 24); }
        const uint32_t x = crc ^ d;
        crc = ft.crc[3][x & 0xffu] ^ ft.crc[2][(x >> 8) & 0xffu] ^ ft.crc[1][(x >> 16) & 0xffu] ^ ft.crc[0][x >> 24];
    }
    {   // the last one to three bytes
        const uint32_t sc = ft.scr[state];
        const uint32_t d = __builtin_amdgcn_alignbit(nxt, cur, 16) ^ sc;
        for (int b = 4 * n_words; b < psdu_len; b++) {
            const uint32_t byte = (d >> (8 * (b & 3))) & 0xffu;
            psdu[b] = (uint8_t)byte;
            crc = (crc >> 8) ^ ft.crc[0][(crc ^ byte) & 0xffu];
        }
    }
    crc = ~crc;
    uint32_t fl = flags | WIFIRX_F_DECODED;
    if (psdu_len >= 4 && crc == 558161692u) fl |= WIFIRX_F_CRC_OK; else fl &= ~WIFIRX_F_CRC_OK;
    rec->flags = fl;
}

}  // namespace wr
