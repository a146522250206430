// wr_tx.hip -- the TX half of the reference's wifi_phy_hier block on the device (gnu_radio/wifi_phy_hier.grc:279-479,570-586):
// scrambler, (133,171) encoder, puncturing, interleaver, constellation map, SIGNAL symbol, pilots, the 4 sync words,
// IFFT-64 with the 1/sqrt(52) window and the cyclic prefixer (CP 16, roll-off 2), for a batch of PSDUs at one encoding.
// What it computes is wifirx/txgen.py's encode_psdus in the float32 arithmetic of NUMERICS.md rule 16.
//
// Work split: the output (every row, padding included) is cut into tiles of TX_TILE consecutive samples; one workgroup
// owns one tile.  It first lists the (frame, OFDM symbol) pairs whose samples fall into the tile -- every symbol of a frame
// is independent work: the coded bits of data symbol q depend only on the data bits q N_DBPS - 6 .. (q+1) N_DBPS - 1, and
// the scrambler bit of position t is bit t mod 127 of the seed's period --, builds each in 16 lanes (lane r holds the FFT
// inputs r + 16 j, the layout of the receive kernels' FFT, wr_quad.h) into LDS, and then writes the tile with one 16-byte
// store per lane and pair of samples, zeros included.
//
// Two kinds of instance.  tx_kernel<NB, false>: every frame at the call's encoding (NB its bits per carrier), that
// encoding's row of the bit map and its constellation axis in LDS.  tx_kernel<6, true>: one encoding per frame
// (TxArgs::enc_v); the rate is a property of the row (TxRowMix), the bit loops run at the widest symbol with the guards the
// SIGNAL symbol already needs, and the bit map is read from constant memory (see the kernel's comment).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "wr_quad.h"      // bfly4_reg, the twiddle table and the spec's complex product (rule 4)
#include "wr_tx.h"

namespace wr {

#define TX_TILE   2048     // samples per workgroup (1024 pairs: four 16-byte stores per lane of a 256-lane group)
#define TX_ROWS   8        // rows one tile can touch: rows hold at least one frame (>= 481 samples): k rows need
                           // (k - 2) 481 < TX_TILE, so at most 6
#define TX_SLOTS  38       // symbols one tile needs: <= TX_TILE / 80 + 2 per row touched = 25.6 + 12 (6 rows at most)
#define TX_PBUF   1040     // PSDU bytes they read: <= (37 * 216 + 6 * 6) / 8 + 2 * 6 = 1016 (6 rows at most)
// With one encoding per frame the three bounds stand as they are.  TX_ROWS: the shortest frame of any encoding is one data
// symbol, 6 * 80 + 1 = 481 samples (1..23 bytes at 64-QAM 3/4; every other encoding needs more symbols for the same bytes),
// so a mix cannot put more rows into a tile than a batch of such frames.  TX_SLOTS counts symbols by the 80 samples each
// takes, whatever it carries.  TX_PBUF: the symbols a tile needs of one row are consecutive and read N_DBPS + 6 bits each
// behind one another, rounded outwards to bytes once per row; 216 is the largest N_DBPS, so rows at other encodings read less.
#define TX_NTW    46       // twiddles the FFT uses: W64^e, e = q r (stage 1) and 4 q (r & 3) (stage 2) <= 45

// scrambler x^7 + x^4 + 1: period of the state 0x7F (bits 0..126, then repeated so that any 32 consecutive bits are one
// unaligned read) and, per seed, the position in that period where the state equals the seed.  The pilot polarity
// p_n = 1 - 2 P[n] is the same sequence (txgen.polarity_sequence starts in state 0x7F too).
struct TxScramble {
    uint32_t pp[6];
    uint8_t  off[128];
};

constexpr TxScramble make_tx_scramble()
{
    TxScramble t{};
    uint32_t state = 0x7F;
    for (int i = 0; i < 127; i++) {
        t.off[state] = (uint8_t)i;
        const uint32_t fb = ((state >> 6) ^ (state >> 3)) & 1u;
        for (int q = i; q < 192; q += 127) t.pp[q >> 5] |= fb << (q & 31);
        state = ((state << 1) & 0x7Eu) | fb;
    }
    return t;
}

__constant__ TxScramble kTxScr = make_tx_scramble();

// sync words (txgen.sync_words): the integer patterns of the short and long training sequence on sub-carriers -26..26,
// as bit masks over k + 26 (compile-time constants: no memory access)
constexpr int8_t kSts[53] = { 0, 0, 1, 0, 0, 0, -1, 0, 0, 0, 1, 0, 0, 0, -1, 0, 0, 0, -1, 0, 0, 0, 1, 0, 0, 0, 0,
                                 0, 0, 0, -1, 0, 0, 0, -1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0 };
constexpr int8_t kLts[53] = { 1, 1, -1, -1, 1, 1, -1, 1, -1, 1, 1, 1, 1, 1, 1, -1, -1, 1, 1, -1, 1, -1, 1, 1, 1, 1, 0,
                                 1, -1, -1, 1, 1, -1, 1, -1, 1, -1, -1, -1, -1, -1, 1, 1, -1, -1, 1, -1, 1, -1, 1, 1, 1, 1 };

constexpr uint64_t sync_mask(const int8_t (&v)[53], int want)
{
    uint64_t m = 0;
    for (int k = 0; k < 53; k++) m |= (uint64_t)(v[k] == want) << k;
    return m;
}
constexpr uint64_t TX_STS_POS = sync_mask(kSts, 1), TX_STS_NEG = sync_mask(kSts, -1);
constexpr uint64_t TX_LTS_POS = sync_mask(kLts, 1), TX_LTS_NEG = sync_mask(kLts, -1);

// one axis of txgen.constellation_points, float32 roundings of the float64 levels, indexed by the axis key (the index bits
// of that axis, first transmitted bit = bit 0)
__constant__ float kAxis2[2]  = { -0x1.6a09e6p-1f, 0x1.6a09e6p-1f };                                       // sqrt(1/2) * {-1, 1}
__constant__ float kAxis4[4]  = { -0x1.e5b9d2p-1f, 0x1.e5b9d2p-1f, -0x1.43d136p-2f, 0x1.43d136p-2f };     // sqrt(1/10) * {-3, 3, -1, 1}
__constant__ float kAxis6[8]  = { -0x1.1482f8p+0f, 0x1.1482f8p+0f, -0x1.3c0366p-3f, 0x1.3c0366p-3f,       // sqrt(1/42) * {-7, 7, -1, 1,
                                  -0x1.8b043ep-1f, 0x1.8b043ep-1f, -0x1.da0518p-2f, 0x1.da0518p-2f };     //                -5, 5, -3, 3}
#define TX_STS_LEVEL 0x1.78d262p+0f     // (float) sqrt(13/6)
#define TX_SCALE     0x1.1c01aap-3f     // (float) (1/sqrt(52))

struct TxRow {             // one row the tile touches
    int64_t  rs, fs;       // first sample of the row, of its frame
    uint32_t flen, s_lo, slot, cnt;      // frame samples; first symbol the tile needs, its LDS slot, symbols needed
    uint32_t frame, len, seed, n_tot;
    uint32_t b_lo, b_n, boff;            // PSDU bytes [b_lo, b_lo + b_n) the tile's data symbols read, at pbuf[boff]
    int32_t  rs_rel, fs_rel, sbase;      // rs, fs relative to the tile's first sample (clamped to +-2^30); slot - s_lo
};

struct TxRowMix : TxRow {  // ... and its rate, where every frame has its own
    uint32_t enc, n_bpsc, n_dbps, rate_field;
};

__device__ __forceinline__ uint32_t parity7(uint32_t v) { return __builtin_popcount(v) & 1u; }

// Where coded bit `pos` (interleaved order) of an OFDM symbol comes from: de-interleave (802.11 17.3.5.7), de-puncture ->
// index m of the rate-1/2 mother code inside the symbol = output m & 1 (A, B) of the encoder at the symbol's data bit m >> 1.
// Rows 0..7: the encodings (WIFIRX_BPSK_1_2 ..); row 8: the SIGNAL symbol (BPSK 1/2).
struct TxBitMap {
    uint16_t m[9][288];
};

constexpr TxBitMap make_tx_bitmap()
{
    TxBitMap t{};
    constexpr uint32_t n_bpsc_of[9] = { 1, 1, 2, 2, 4, 4, 6, 6, 1 };
    constexpr uint32_t rate_of[9] = { 0, 2, 0, 2, 0, 2, 1, 2, 0 };      // 0 = 1/2, 1 = 2/3, 2 = 3/4
    for (int e = 0; e < 9; e++) {
        const uint32_t n_bpsc = n_bpsc_of[e], n_cbps = 48 * n_bpsc, s = n_bpsc > 1 ? n_bpsc / 2 : 1;
        for (uint32_t pos = 0; pos < n_cbps; pos++) {
            const uint32_t i = s * (pos / s) + (pos + (16 * pos) / n_cbps) % s;
            const uint32_t k = 16 * i - (n_cbps - 1) * ((16 * i) / n_cbps);
            uint32_t m = k;
            if (rate_of[e] == 2) m = 6 * (k / 4) + (k % 4 == 3 ? 5 : k % 4);     // 3/4: keep 0,1,2,5 of 6
            else if (rate_of[e] == 1) m = 4 * (k / 3) + k % 3;                   // 2/3: keep 0,1,2 of 4
            t.m[e][pos] = (uint16_t)m;
        }
    }
    return t;
}

__constant__ TxBitMap kTxMap = make_tx_bitmap();


// NB = bits per sub-carrier of the call's encoding: the bit loops unroll, so that a symbol's table and window reads go
// out together instead of one LDS round trip after the other.
// MIX (NB = 6): one encoding per frame.  LDS is full (seven workgroups per CU leave 23 405 bytes each) and the nine rows of
// kTxMap are 5 184 bytes, so this instance reads the map where it lies, in constant memory: the index is per lane, so these
// are vector loads, and the whole table stays in the CU's cache (it is read by every workgroup).  Its LDS copy (672 bytes) goes
// and the three constellation axes (14 floats: 2 | 4 | 8, at axis + 0, 2 and 6) and four words per row come, so the seven
// workgroups per CU stay.  A wave builds four symbols at once, one per group of 16 lanes, and with rows of different
// encodings in a tile it runs the unrolled bit loops at the width of the widest, the others masked by `b < n_bpsc`.
template <int NB, bool MIX>
__global__ __launch_bounds__(256, 7)     // 7 waves per SIMD (72 registers): seven workgroups per CU, as the LDS allows
void tx_kernel(TxArgs a)
{
    static_assert(!MIX || NB == 6, "the mixed instance runs at the widest symbol");
    using Row = typename std::conditional<MIX, TxRowMix, TxRow>::type;
    __shared__ float2   sym[TX_SLOTS][64];     // time-domain symbols (also the FFT's transpose space)
    __shared__ uint32_t win[16][8];            // data-bit window of the symbol each group of 16 lanes builds
    __shared__ uint16_t bmap[MIX ? 2 : 288 + 48];      // kTxMap rows of the call's encoding and of SIGNAL (MIX: not used)
    __shared__ float    axis[MIX ? 14 : 8];    // one axis of the call's constellation; MIX: of the three
    __shared__ float2   twd[TX_NTW];
    __shared__ uint32_t scr_pp[6];
    __shared__ uint8_t  scr_off[128];
    __shared__ uint8_t  pbuf[TX_PBUF];         // the PSDU bytes of the tile's data symbols
    __shared__ Row      rows[TX_ROWS];
    __shared__ uint32_t n_rows_s, n_tasks_s;

    const int tid = threadIdx.x;
    const uint64_t tile = blockIdx.x;
    const int64_t v_lo = a.v0 + (int64_t)tile * TX_TILE;                  // pair-aligned sample index + a.shift
    const int64_t g_lo = v_lo - a.shift < a.g0 ? a.g0 : v_lo - a.shift;
    const int64_t g_hi = v_lo + TX_TILE - a.shift > a.g1 ? a.g1 : v_lo + TX_TILE - a.shift;

    if constexpr (!MIX) {
        for (uint32_t i = tid; i < a.n_cbps; i += 256) bmap[i] = kTxMap.m[a.enc][i];
        if (tid < 48) bmap[288 + tid] = kTxMap.m[8][tid];
    }
    if (tid < TX_NTW) twd[tid] = make_float2(WR_TWIDDLE64[2 * tid], WR_TWIDDLE64[2 * tid + 1]);
    if (tid < 6) scr_pp[tid] = kTxScr.pp[tid];
    if (tid < 128) scr_off[tid] = kTxScr.off[tid];
    if constexpr (MIX) {
        if (tid < 14) axis[tid] = tid < 2 ? kAxis2[tid] : tid < 6 ? kAxis4[tid - 2] : kAxis6[tid - 6];
    } else {
        if (tid < (1 << (a.n_bpsc >> 1)) && a.n_bpsc > 1) axis[tid] = a.n_bpsc == 2 ? kAxis2[tid] : a.n_bpsc == 4 ? kAxis4[tid] : kAxis6[tid];
    }

    // ---- the rows of the tile and the symbols it needs of each (lanes 0..7 of wave 0, one row each) ----
    if (tid < 64) {
        const uint32_t r0 = a.row_off ? a.tile_row[tile] : (uint32_t)((uint64_t)g_lo / a.row_len);
        const uint32_t r = r0 + (uint32_t)tid;
        Row e{};
        uint32_t n_dbps = a.n_dbps;
        bool in = tid < TX_ROWS && r < a.n_frames;
        if (in) {
            e.rs = a.row_off ? (int64_t)a.row_off[r] : (int64_t)r * (int64_t)a.row_len;
            in = e.rs < g_hi;
        }
        if (in) {
            e.frame = r;
            e.len = a.len[r];
            e.seed = a.seeds ? a.seeds[r] : r % 127u + 1u;
            if constexpr (MIX) {
                // the rate of the row from its encoding (the host has checked enc <= 7): N_BPSC 1 1 2 2 4 4 6 6; N_DBPS =
                // 48 N_BPSC times 1/2 (even), 3/4 (odd) or 2/3 (64-QAM 2/3); RATE 0xD 0xF 0x5 0x7 0x9 0xB 0x1 0x3
                e.enc = a.enc_v[r] & 7u;
                e.n_bpsc = e.enc >= 6 ? 6u : 1u << (e.enc >> 1);
                e.n_dbps = e.enc == 6 ? 192u : (e.enc & 1) ? 36u * e.n_bpsc : 24u * e.n_bpsc;
                e.rate_field = (0x31B975FDu >> (4 * e.enc)) & 0xFu;
                n_dbps = e.n_dbps;
            }
            e.n_tot = 5 + (16 + 8 * e.len + 6 + n_dbps - 1) / n_dbps;
            e.flen = e.n_tot * 80 + 1;
            e.fs = e.rs + a.lead;
            const int64_t lo = g_lo > e.fs ? g_lo : e.fs, hi = g_hi < e.fs + e.flen ? g_hi : e.fs + e.flen;
            if (lo < hi) {
                const uint32_t m_lo = (uint32_t)(lo - e.fs), m_hi = (uint32_t)(hi - e.fs);
                e.s_lo = m_lo ? (m_lo - 1) / 80 : 0;                       // sample 80 s needs symbol s - 1 (roll-off)
                const uint32_t s_hi = min(e.n_tot - 1, (m_hi - 1) / 80);  // the trailing sample n_tot * 80 needs the last
                e.cnt = s_hi - e.s_lo + 1;
                if (s_hi >= 5) {                                           // data symbols d_lo .. d_hi read data bits
                    const int32_t d_lo = (int32_t)max(e.s_lo, 5u) - 5, d_hi = (int32_t)s_hi - 5;   // d N_DBPS - 6 ..
                    const int32_t q_lo = max(0, (d_lo * (int32_t)n_dbps - 22) >> 3);                // (d + 1) N_DBPS - 1
                    const int32_t q_hi = min((int32_t)e.len, (((d_hi + 1) * (int32_t)n_dbps - 17) >> 3) + 1);
                    e.b_lo = (uint32_t)q_lo;
                    e.b_n = q_hi > q_lo ? (uint32_t)(q_hi - q_lo) : 0;
                }
            }
        }
        uint32_t incl = e.cnt, bincl = e.b_n;                             // inclusive prefix sums over the 8 lanes
#pragma unroll
        for (int d = 1; d < TX_ROWS; d <<= 1) {
            const uint32_t o = __shfl_up(incl, d, 64), bo = __shfl_up(bincl, d, 64);
            if ((tid & 63) >= d) { incl += o; bincl += bo; }
        }
        e.slot = incl - e.cnt;
        e.sbase = (int32_t)e.slot - (int32_t)e.s_lo;
        e.rs_rel = (int32_t)max(min(e.rs - g_lo, (int64_t)1 << 30), -((int64_t)1 << 30));
        e.fs_rel = (int32_t)max(min(e.fs - g_lo, (int64_t)1 << 30), -((int64_t)1 << 30));
        e.boff = bincl - e.b_n;
        if (e.boff + e.b_n > TX_PBUF) e.b_n = e.boff < TX_PBUF ? TX_PBUF - e.boff : 0;     // (cannot happen: see TX_PBUF)
        const uint64_t in_mask = __ballot(in);
        const uint32_t total = __shfl(incl, TX_ROWS - 1, 64);          // (every lane of the wave takes part)
        if (in) rows[tid] = e;
        if (tid == 0) {
            n_rows_s = (uint32_t)__popcll(in_mask);
            n_tasks_s = min(total, (uint32_t)TX_SLOTS);
        }
    }
    __syncthreads();
    const uint32_t n_rows = n_rows_s, n_tasks = n_tasks_s;
    for (uint32_t ei = 0; ei < n_rows; ei++) {                          // the PSDU bytes, row by row
        const Row& e = rows[ei];
        const uint8_t* p = a.psdu + (uint64_t)e.frame * a.psdu_stride + e.b_lo;
        for (uint32_t k = tid; k < e.b_n; k += 256) pbuf[e.boff + k] = p[k];
    }
    __syncthreads();

    // ---- build the symbols: group of 16 lanes = one (frame, symbol) ----
    const int grp = tid >> 4, r = tid & 15;
    int cj[4];                                   // data carrier of the lane's bin j (0 for the other bins)
    bool dj[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int i = r + 16 * ((j + 2) & 3);
        dj[j] = i >= 6 && i <= 58 && i != 11 && i != 25 && i != 32 && i != 39 && i != 53;
        cj[j] = dj[j] ? i - 6 - (i > 11) - (i > 25) - (i > 32) - (i > 39) - (i > 53) : 0;
    }
    for (uint32_t base = 0; base < n_tasks; base += 16) {
        const uint32_t task = base + grp;
        if (task < n_tasks) {
            uint32_t ei = 0;
            while (ei + 1 < n_rows && rows[ei + 1].slot <= task) ei++;
            const Row e = rows[ei];                              // (a copy: one set of LDS reads)
            const uint32_t s = e.s_lo + task - e.slot;
            const bool sig = s == 4;
            uint32_t n_bpsc, n_dbps, rate_field;
            const uint16_t* bm;
            const float* ax;
            if constexpr (MIX) {
                n_bpsc = sig ? 1 : e.n_bpsc;
                n_dbps = e.n_dbps;
                rate_field = e.rate_field;
                bm = kTxMap.m[sig ? 8 : e.enc];
                ax = axis + (e.n_bpsc == 6 ? 6 : e.n_bpsc == 4 ? 2 : 0);
            } else {
                n_bpsc = sig ? 1 : NB;
                n_dbps = a.n_dbps;
                rate_field = a.rate_field;
                bm = sig ? bmap + 288 : bmap;
                ax = axis;
            }
            uint32_t* w = win[grp];
            if (s >= 4 && r < 8) {                                       // the symbol's data-bit window, word r
                uint32_t word = 0;
                if (sig) {
                    // SIGNAL: RATE (4 bits, MSB first) | 0 | LENGTH (12 bits, LSB first) | even parity | 6 zero tail bits
                    const uint32_t rf = rate_field;
                    uint32_t b = ((rf >> 3) & 1) | ((rf >> 2) & 1) << 1 | ((rf >> 1) & 1) << 2 | (rf & 1) << 3 | e.len << 5;
                    b |= (uint32_t)(__builtin_popcount(b) & 1) << 17;
                    word = r == 0 ? b << 6 : 0;
                } else {
                    const int32_t t0 = (int32_t)((s - 5) * n_dbps) - 6 + 32 * r;       // data bit of bit 0 of the word
                    // PSDU bits (LSB first) behind the 16 SERVICE bits; bytes outside the PSDU read as 0
                    const int32_t bq = (t0 - 16) >> 3, sh = (t0 - 16) - 8 * bq;
                    uint64_t raw = 0;                                    // (bytes outside b_lo .. read as 0: such bits
#pragma unroll                                                           //  lie outside the symbol's window)
                    for (int k = 0; k < 5; k++) {
                        const uint32_t q = (uint32_t)(bq + k - (int32_t)e.b_lo);
                        const uint32_t byte = pbuf[min(e.boff + q, (uint32_t)TX_PBUF - 1)];     // (in bounds, used or not)
                        raw |= (uint64_t)(q < e.b_n ? byte : 0u) << (8 * k);
                    }
                    const uint32_t ps = ((uint32_t)(t0 + 127) + scr_off[e.seed]) % 127u;
                    const uint32_t pw = ps >> 5, po = ps & 31;
                    const uint32_t scr = __builtin_amdgcn_alignbit(scr_pp[pw + 1], scr_pp[pw], po);
                    word = (uint32_t)(raw >> sh) ^ scr;
                    if (t0 < 0) word &= ~0u << (-t0);                            // the encoder starts in state 0
                    const int32_t q0 = 16 + 8 * (int32_t)e.len - t0;                 // tail bits: zero after scrambling
                    if (q0 > -6 && q0 < 32) word &= ~(uint32_t)(q0 >= 0 ? 0x3Full << q0 : 0x3Full >> -q0);
                }
                w[r] = word;
            }
            __builtin_amdgcn_wave_barrier();
            float2* sl = sym[task];
            const uint32_t half = n_bpsc >> 1, hmask = (1u << half) - 1;
            uint32_t idx[4] = { 0, 0, 0, 0 };
            if (s >= 4) {                                        // the constellation indices of the lane's data bins
                uint32_t mm[4][NB];
#pragma unroll
                for (int j = 0; j < 4; j++)
#pragma unroll
                    for (int b = 0; b < NB; b++) mm[j][b] = bm[cj[j] * n_bpsc + (b < (int)n_bpsc ? b : 0)];
#pragma unroll
                for (int j = 0; j < 4; j++)
#pragma unroll
                    for (int b = 0; b < NB; b++) {
                        const uint32_t m = mm[j][b], t = m >> 1, wi = t >> 5;
                        const uint32_t f = __builtin_amdgcn_alignbit(w[wi + 1], w[wi], t & 31);
                        // field bit p = data bit t - 6 + p: A = d0^d2^d3^d5^d6 -> bits 6,4,3,1,0; B = d0^d1^d2^d3^d6 -> 6,5,4,3,0
                        if (b < (int)n_bpsc) idx[j] |= parity7(f & ((m & 1) ? 0x79u : 0x5Bu)) << b;
                    }
            }
            c32 v[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int i = r + 16 * ((j + 2) & 3);            // shifted bin of FFT input r + 16 j (ifftshift)
                const int k = i - 32;
                c32 X = { 0.0f, 0.0f };
                if (s < 4) {
                    if (k >= -26 && k <= 26) {
                        if (s < 2) {
                            const float q = ((TX_STS_POS >> (k + 26)) & 1) ? TX_STS_LEVEL : ((TX_STS_NEG >> (k + 26)) & 1) ? -TX_STS_LEVEL : 0.0f;
                            X = { q, q };
                        } else {
                            const float l = ((TX_LTS_POS >> (k + 26)) & 1) ? 1.0f : ((TX_LTS_NEG >> (k + 26)) & 1) ? -1.0f : 0.0f;
                            if (s == 3 || (k & 3) == 0) X = { l, 0.0f };
                            else if ((k & 3) == 1) X = { 0.0f, -l };              // LTS advanced by 16 samples: l (-j)^k
                            else if ((k & 3) == 2) X = { -l, 0.0f };
                            else X = { 0.0f, l };
                        }
                    }
                } else if (i == 11 || i == 25 || i == 39 || i == 53) {
                    const bool neg = ((scr_pp[((s - 4) % 127) >> 5] >> (((s - 4) % 127) & 31)) & 1) ^ (i == 53);
                    X = { neg ? -1.0f : 1.0f, 0.0f };
                } else if (dj[j]) {
                    if (n_bpsc == 1) X = { idx[j] ? 1.0f : -1.0f, 0.0f };
                    else X = { ax[idx[j] & hmask], ax[idx[j] >> half] };
                }
                v[j] = { X.re, -X.im };                          // the IFFT as conj(FFT(conj(.)))
            }
            // ---- FFT-64, NUMERICS.md rule 4: three radix-4 DIF stages (spans 16, 4, 1), twiddle W64^(q n step) ----
            bfly4_reg(v[0], v[1], v[2], v[3]);
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const float2 tw = twd[q * r];
                const c32 y = sp_cmul(v[q], c32{ tw.x, tw.y });
                sl[r + 16 * q] = make_float2(y.re, y.im);
            }
            __builtin_amdgcn_wave_barrier();
            const int b2 = 16 * (r >> 2) + (r & 3);
#pragma unroll
            for (int q = 0; q < 4; q++) { const float2 t = sl[b2 + 4 * q]; v[q] = { t.x, t.y }; }
            bfly4_reg(v[0], v[1], v[2], v[3]);
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const float2 tw = twd[q * (r & 3) * 4];
                const c32 y = sp_cmul(v[q], c32{ tw.x, tw.y });
                sl[b2 + 4 * q] = make_float2(y.re, y.im);
            }
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int q = 0; q < 4; q++) { const float2 t = sl[4 * r + q]; v[q] = { t.x, t.y }; }
            __builtin_amdgcn_wave_barrier();
            bfly4_reg(v[0], v[1], v[2], v[3]);
            // position 4 r + q holds X[k], k = (r >> 2) + 4 (r & 3) + 16 q: time sample k = conj(X[k]) / sqrt(52)
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const c32 y = sp_cmul(v[q], c32{ twd[0].x, twd[0].y });
                sl[(r >> 2) + 4 * (r & 3) + 16 * q] = make_float2(y.re * TX_SCALE, -y.im * TX_SCALE);
            }
        }
    }
    __syncthreads();

    // ---- the tile's stores: pair p of the tile = samples v_lo + 2 p, +1 (minus the shift), one 16-byte store ----
    // sample x of the tile (relative to g_lo); the selects instead of branches: a wave's 128 samples span two symbols
    auto sample = [&](int32_t x) -> float2 {
        uint32_t ei = 0;
        while (ei + 1 < n_rows && rows[ei + 1].rs_rel <= x) ei++;
        const Row& e = rows[ei];
        const int32_t m = x - e.fs_rel;
        const bool in = n_rows != 0 && m >= 0 && m < (int32_t)e.flen;
        const uint32_t mu = in ? (uint32_t)m : 0, s = mu / 80, j = mu - 80 * s;
        const int32_t so = min(max(e.sbase + (int32_t)min(s, e.n_tot - 1), 0), TX_SLOTS - 1);   // own symbol (the last one
        const int32_t sp = min(max(e.sbase + (int32_t)s - 1, 0), TX_SLOTS - 1);                //  for the trailing sample)
        const float2 o = sym[so][j == 0 ? 48 : j < 16 ? 48 + j : j - 16];
        const float2 p = sym[sp][0];
        float2 r = o;
        if (j == 0) {                       // roll-off: 0.5 own + 0.5 the previous symbol's continuation; frame edges half
            if (s == 0) r = make_float2(0.5f * o.x, 0.5f * o.y);
            else if (s == e.n_tot) r = make_float2(0.5f * p.x, 0.5f * p.y);
            else r = make_float2(0.5f * o.x + 0.5f * p.x, 0.5f * o.y + 0.5f * p.y);
        }
        return in ? r : make_float2(0.0f, 0.0f);
    };
    float4* out4 = reinterpret_cast<float4*>(a.out - a.shift);
    const int32_t x0 = (int32_t)(v_lo - a.shift - g_lo), x_end = (int32_t)(g_hi - g_lo);      // x0 = 0 or -1
#pragma unroll
    for (int u = 0; u < TX_TILE / 512; u++) {
        const int32_t x = x0 + 2 * (256 * u + tid);
        const bool in0 = x >= 0 && x < x_end, in1 = x + 1 >= 0 && x + 1 < x_end;
        if (in0 && in1) {
            const float2 y0 = sample(x), y1 = sample(x + 1);
            out4[(v_lo >> 1) + 256 * u + tid] = make_float4(y0.x, y0.y, y1.x, y1.y);
        } else if (in0) {
            a.out[g_lo + x] = sample(x);
        } else if (in1) {
            a.out[g_lo + x + 1] = sample(x + 1);
        }
    }
}

}  // namespace wr

extern "C" hipError_t wr_launch_tx(hipStream_t st, const wr::TxArgs* args)
{
    if (args->g1 <= args->g0) return hipSuccess;
    const uint64_t n_tiles = ((uint64_t)(args->g1 + args->shift - args->v0) + TX_TILE - 1) / TX_TILE;
    const dim3 grid((unsigned)n_tiles), block(256);
    if (args->enc_v) {
        hipLaunchKernelGGL((wr::tx_kernel<6, true>), grid, block, 0, st, *args);
        return hipGetLastError();
    }
    switch (args->n_bpsc) {
    case 1: hipLaunchKernelGGL((wr::tx_kernel<1, false>), grid, block, 0, st, *args); break;
    case 2: hipLaunchKernelGGL((wr::tx_kernel<2, false>), grid, block, 0, st, *args); break;
    case 4: hipLaunchKernelGGL((wr::tx_kernel<4, false>), grid, block, 0, st, *args); break;
    default: hipLaunchKernelGGL((wr::tx_kernel<6, false>), grid, block, 0, st, *args); break;
    }
    return hipGetLastError();
}

extern "C" uint32_t wr_tx_tile_samples(void) { return TX_TILE; }
