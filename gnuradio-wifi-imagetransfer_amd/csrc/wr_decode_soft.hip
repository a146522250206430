// wr_decode_soft.hip -- soft-decision decode_mac (NUMERICS.md rule 14): Viterbi K=7 (133,171) on the demodulator's
// LLRs instead of its hard decisions, then descramble and CRC-32 as the hard path does (wr_decode.hip).
//
// One wavefront decodes 64 frames of ONE rate, one frame per lane.  The 64 path metrics of a lane's frame are float32
// in 64 VGPRs, updated in place with the register rotation of decode_kernel (the state <-> register map turns by one
// bit per step and is the identity again after six, so the add-compare-select is unrolled over six steps).  A state's
// decision is the contract's comparison itself: v_cmp_lt_f32 (m1 < m0) into VCC, v_cndmask_b32 picks the survivor's
// metric, v_addc_co_u32 (acc + acc + VCC) drops the decision into the lane's 32-bit accumulator -- three instructions per
// state besides the two adds, and no NaN can ever decide (the +inf start metrics compare, they are never subtracted).
//
// The LLRs of the current OFDM symbol of every lane's frame are staged in LDS as rows of 64 lanes (row j = LLR j of the
// symbol, 256 bytes): each lane reads its own symbol contiguously in float4s, and a trellis step then reads coded bits A
// and B of all 64 frames from the two rows a per-rate table names (wave-uniform: scalar loads).  The kernel is
// instantiated per bits-per-carrier class (NB = 1, 2, 4, 6 rows of 48), so that the LDS of a workgroup (one wave) is what
// its rate needs: 12 / 24 / 48 / 72 kB + 4.5 kB of finish tables.
//
// bf16 rows (WIFIRX_LLR_BF16, NUMERICS.md rule 15; BF = true): the same kernel with the rows staged as the 16-bit values
// themselves -- 6 / 12 / 24 / 36 kB --, still loaded as 16-byte vectors contiguous per lane; a trellis step widens the two
// values it reads (exactly: a shift by 16) and goes on with rule 14 unchanged.
//
// The host groups the decodable frames by rate (decode_perm_kernel of wr_decode.hip: runs that start on 64-frame task
// boundaries) and launches each class over its range of tasks.  Survivor bits: 8 bytes per step and lane in the handle's
// decode scratch; trace-back, descramble and CRC follow per lane.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "wifirx.h"
#include "wr_kernels.h"
#include "wr_decode.h"

namespace wr {
namespace soft {

#define WR_SOFT_NORM_STEPS 24          // the common minimum leaves the metrics before every step t > 0, t % 24 == 0
#define WR_SOFT_PUNCT 0xffffu          // table entry of a coded bit the transmitter dropped

// [enc][step of the symbol]: the LLR index (coded_index: carrier * n_bpsc + bit) of coded bit A | that of B << 16
constexpr uint32_t llr_of_coded(int, int j) { return j < 0 ? WR_SOFT_PUNCT : (uint32_t)j; }
__constant__ const RateTable WR_SOFT_TABLE = make_rate_table(llr_of_coded);

// trellis steps of a frame the soft decoder takes (the hard decoder's rule, WIFIRX_F_LLR, and LLR rows wide enough for
// the rate), 0 for a frame it leaves alone
__device__ __forceinline__ int soft_frame_steps(uint32_t flags, int enc, int len, uint32_t psdu_stride, uint32_t max_sym,
                                                uint32_t llr_bits, uint32_t n_steps_cap)
{
    if (!(flags & WIFIRX_F_LLR) || (uint32_t)nbpsc_of(enc & 7) > llr_bits) return 0;
    return frame_steps(flags, enc, len, psdu_stride, max_sym, n_steps_cap);
}

// One state of the add-compare-select: m = (c1 < c0) ? c1 : c0, and the decision (c1 < c0) shifted into acc from below.
__device__ __forceinline__ void acs_state(float c0, float c1, float& m, uint32_t& acc)
{
    asm("v_cmp_lt_f32 vcc, %2, %3\n\t"
        "v_cndmask_b32 %0, %3, %2, vcc\n\t"
        "v_addc_co_u32 %1, vcc, %1, %1, vcc"
        : "=v"(m), "+v"(acc)
        : "v"(c1), "v"(c0)
        : "vcc");
}

// one trellis step at register phase P: logical state s lives in pm[rotr6(s, P)].  bm[2 a + b]: branch metric of a
// transition whose expected coded pair is (a, b).  acc[0] / acc[1]: the decisions of states 0..31 / 32..63, state s in
// bit 31 - (s & 31).
template <int P>
__device__ __forceinline__ void acs_step(float (&pm)[64], const float (&bm)[4], uint32_t (&acc)[2])
{
#pragma unroll
    for (int j = 0; j < 32; j++) {
        const int a = parity_of((j << 1) & 0155), b = parity_of((j << 1) & 0117);
        const float m = bm[2 * a + b], mb = bm[2 * (a ^ 1) + (b ^ 1)];
        const int r0 = rotr6(j, P), r1 = rotr6(j + 32, P);
        const float p0 = pm[r0], p1 = pm[r1];
        // state 2j (input bit 0): from j with m (candidate 0), from j+32 with mb (candidate 1); state 2j+1: swapped
        const float c00 = p0 + m, c01 = p1 + mb, c10 = p0 + mb, c11 = p1 + m;
        acs_state(c00, c01, pm[r0], acc[j >> 4]);      // = register of logical state 2j at phase P+1
        acs_state(c10, c11, pm[r1], acc[j >> 4]);      // = register of logical state 2j+1 at phase P+1
    }
}

// Tasks [task_lo, task_hi) of 64 frames each (grid-stride over n_waves_total waves, one wave per workgroup); frame k of
// task T is perm[64 T + k] (0xffffffff: none), or slot 64 T + k without a permutation.  Every task holds frames of one
// rate whose bits per carrier are NB.  BF: llr_all holds bf16 values (uint16_t) instead of floats.
template <int NB, bool BF = false>
__global__ __launch_bounds__(64)
void decode_soft_kernel(uint32_t n_slots, uint32_t max_sym, uint32_t llr_bits, wifirx_frame* __restrict__ frames,
                        const float* __restrict__ llr_all, uint8_t* __restrict__ psdu_all, uint32_t psdu_stride,
                        uint8_t* __restrict__ scratch, size_t scratch_stride, uint32_t n_steps_cap, uint32_t n_waves_total,
                        const uint32_t* __restrict__ perm, uint32_t n_virtual, uint32_t task_lo, uint32_t task_hi)
{
    constexpr int N_CBPS = 48 * NB;
    typedef std::conditional_t<BF, uint16_t, float> row_t;
    __shared__ row_t rows[N_CBPS * 64];          // LLR j of the current symbol of lane l's frame at rows[64 j + l]
    __shared__ FinishTables ft;
    build_finish_tables(ft);
    const int lane = threadIdx.x;
    const uint32_t wave = blockIdx.x;
    row_t* roww = rows + lane;
    uint8_t* const slice = scratch + (size_t)wave * scratch_stride;                              // (layout: wr_kernels.h)
    uint32_t* surv = reinterpret_cast<uint32_t*>(slice);                                         // [step][lane][2]
    uint32_t* dbits = reinterpret_cast<uint32_t*>(slice + dec_soft_dbits_at(n_steps_cap));       // [word][lane]
    const size_t row_stride = (size_t)max_sym * 48 * llr_bits;      // values per frame

    for (uint32_t task = task_lo + wave; task < task_hi; task += n_waves_total) {
        const uint32_t v = task * 64u + (uint32_t)lane;
        uint32_t slot = 0xffffffffu;
        if (v < n_virtual) slot = perm ? perm[v] : v;
        int n_data = 0, enc = 0;
        if (slot < n_slots) {
            enc = frames[slot].encoding & 7;
            n_data = soft_frame_steps(frames[slot].flags, enc, frames[slot].psdu_len, psdu_stride, max_sym, llr_bits, n_steps_cap);
        } else {
            slot = 0;
        }
        // the task's rate: that of its first frame; the host's grouping makes it every frame's (a frame of another rate
        // would be left alone rather than decoded with the wrong tables)
        const uint64_t act = __ballot(n_data > 0);
        if (act == 0) continue;
        const int enc_u = __builtin_amdgcn_readlane(enc, (int)__builtin_ctzll(act));
        if (nbpsc_of(enc_u) != NB) continue;                 // wave-uniform; not this instance's class
        if (enc != enc_u) n_data = 0;
        int n_max = n_data;
#pragma unroll
        for (int k = 1; k < 64; k <<= 1) {
            int o = __shfl_xor(n_max, k, 64);
            n_max = o > n_max ? o : n_max;
        }
        n_max = __builtin_amdgcn_readfirstlane(n_max);
        const int nd_u = ndbps_of(enc_u);
        const float4* src = BF ? reinterpret_cast<const float4*>(reinterpret_cast<const uint16_t*>(llr_all) + (size_t)slot * row_stride)
                               : reinterpret_cast<const float4*>(llr_all + (size_t)slot * row_stride);

        // ---- add-compare-select ----
        float pm[64];
#pragma unroll
        for (int s = 0; s < 64; s++) pm[s] = s == 0 ? 0.0f : __builtin_inff();
        int best = 0;
        int tt_u = 0, sym_u = 0, since_norm = 0;            // wave-uniform: step within the symbol, symbol, steps since the minimum left
        for (int tg = 0; tg < n_max; tg += 6) {
            if (since_norm == WR_SOFT_NORM_STEPS) {
                // subtract the common minimum (register phase 0 here)
                since_norm = 0;
                float mn = pm[0];
#pragma unroll
                for (int s = 1; s < 64; s++) mn = fminf(mn, pm[s]);
#pragma unroll
                for (int s = 0; s < 64; s++) pm[s] = pm[s] - mn;
            }
            since_norm += 6;
            if (tt_u == nd_u) { tt_u = 0; sym_u++; }
            if (BF && tt_u == 0 && tg < n_data) {
                // the same for bf16 rows: eight values per 16-byte load, 6 / 12 / 24 / 36 loads per symbol
                constexpr int NV = N_CBPS / 8, CH = NV < 12 ? NV : 12;
                const float4* sp = src + (size_t)sym_u * NV;
#pragma unroll
                for (int c = 0; c < NV; c += CH) {
                    uint4 x[CH];
#pragma unroll
                    for (int k = 0; k < CH; k++) x[k] = __builtin_bit_cast(uint4, sp[c + k]);
#pragma unroll
                    for (int k = 0; k < CH; k++) {
                        const uint32_t w[4] = { x[k].x, x[k].y, x[k].z, x[k].w };
#pragma unroll
                        for (int i = 0; i < 4; i++) {
                            roww[(8 * (c + k) + 2 * i) * 64] = (uint16_t)w[i];
                            roww[(8 * (c + k) + 2 * i + 1) * 64] = (uint16_t)(w[i] >> 16);
                        }
                    }
                }
            } else
            if (tt_u == 0 && tg < n_data) {
                // a new OFDM symbol: its 48 NB LLRs, global (float4, contiguous per lane) -> the lane's column of the rows
                const float4* sp = src + (size_t)sym_u * (N_CBPS / 4);
#pragma unroll
                for (int c = 0; c < N_CBPS / 4; c += 12) {
                    float4 x[12];
#pragma unroll
                    for (int k = 0; k < 12; k++) x[k] = sp[c + k];
#pragma unroll
                    for (int k = 0; k < 12; k++) {
                        roww[(4 * (c + k) + 0) * 64] = (row_t)x[k].x;
                        roww[(4 * (c + k) + 1) * 64] = (row_t)x[k].y;
                        roww[(4 * (c + k) + 2) * 64] = (row_t)x[k].z;
                        roww[(4 * (c + k) + 3) * 64] = (row_t)x[k].w;
                    }
                }
            }
            const uint32_t* te = WR_SOFT_TABLE.e + (enc_u * RATE_TAB_STRIDE + tt_u);      // wave-uniform: scalar loads
// an LLR as the trellis reads it: float32 rows as they are, bf16 rows widened (exactly: the 16 bits above 16 zero bits)
#define WR_SOFT_ROW(v) (BF ? __uint_as_float((uint32_t)(v) << 16) : (v))
#define WR_SOFT_STEP(P)                                                                                   \
            {                                                                                             \
                const uint32_t e = te[P];                                                                 \
                const uint32_t ea = e & 0xffffu, eb = e >> 16;                                            \
                float la = WR_SOFT_ROW(roww[(ea == WR_SOFT_PUNCT ? 0u : ea) * 64]);                       \
                float lb = WR_SOFT_ROW(roww[(eb == WR_SOFT_PUNCT ? 0u : eb) * 64]);                       \
                if (ea == WR_SOFT_PUNCT || !__builtin_isfinite(la)) la = 0.0f;                            \
                if (eb == WR_SOFT_PUNCT || !__builtin_isfinite(lb)) lb = 0.0f;                            \
                const float a0 = fmaxf(la, 0.0f), a1 = fmaxf(-la, 0.0f);                                  \
                const float b0 = fmaxf(lb, 0.0f), b1 = fmaxf(-lb, 0.0f);                                  \
                const float bm[4] = { a0 + b0, a0 + b1, a1 + b0, a1 + b1 };                               \
                uint32_t acc[2] = { 0u, 0u };                                                             \
                acs_step<P>(pm, bm, acc);                                                                 \
                *reinterpret_cast<uint2*>(surv + ((size_t)(tg + P) * 64 + lane) * 2) = make_uint2(acc[0], acc[1]); \
            }
            WR_SOFT_STEP(0) WR_SOFT_STEP(1) WR_SOFT_STEP(2) WR_SOFT_STEP(3) WR_SOFT_STEP(4) WR_SOFT_STEP(5)
#undef WR_SOFT_STEP
#undef WR_SOFT_ROW
            {
                const bool end = tg + 6 == n_data;
                if (__any(end)) {
                    // a frame just ended (register phase 0 again): smallest metric, lowest state
                    float bv = pm[0];
                    int bs = 0;
#pragma unroll
                    for (int s = 1; s < 64; s++)
                        if (pm[s] < bv) { bv = pm[s]; bs = s; }
                    if (end) best = bs;
                }
            }
            tt_u += 6;
        }
        __threadfence_block();
        // ---- trace-back: 32 decoded bits per word, words stored [word][lane]; the survivor rows are loaded ahead ----
        {
            int st = best;
            uint32_t word = 0;
            for (int t1 = n_max - 1; t1 >= 0; t1 -= 16) {
                uint2 r[16];
#pragma unroll
                for (int k = 0; k < 16; k++) {
                    const int t = t1 - k < 0 ? 0 : t1 - k;      // rows below n_max were all written: no branch around the loads
                    r[k] = *reinterpret_cast<const uint2*>(surv + ((size_t)t * 64 + lane) * 2);
                }
#pragma unroll
                for (int k = 0; k < 16; k++) {
                    const int t = t1 - k;
                    if (t >= 0 && t < n_data) {
                        word |= (uint32_t)(st & 1) << (t & 31);
                        const uint64_t w = ((uint64_t)r[k].x << 32) | r[k].y;         // state s in bit 63 - s
                        const uint32_t hb = (uint32_t)(w >> (63 - st)) & 1u;
                        st = (st >> 1) | (int)(hb << 5);
                        if ((t & 31) == 0) { dbits[(size_t)(t >> 5) * 64 + lane] = word; word = 0; }
                    }
                }
            }
        }
        __threadfence_block();
        // ---- descramble, bytes, CRC-32 ----
        if (n_data > 0)
            finish_frame<64>(dbits + lane, frames[slot].psdu_len, psdu_all + (size_t)slot * psdu_stride,
                         ((reinterpret_cast<uintptr_t>(psdu_all) | psdu_stride) & 3) == 0, frames + slot, frames[slot].flags, ft);
    }
}

}  // namespace soft
}  // namespace wr

extern "C" hipError_t wr_launch_decode_soft(hipStream_t st, int nb, uint32_t n_slots, uint32_t max_sym, uint32_t llr_bits,
                                            wifirx_frame* frames, const float* llr, uint8_t* psdu, uint32_t psdu_stride,
                                            uint8_t* scratch, size_t scratch_stride, uint32_t n_steps_cap, uint32_t n_waves,
                                            const uint32_t* perm, uint32_t n_virtual, uint32_t task_lo, uint32_t task_hi)
{
    if (n_slots == 0 || n_waves == 0 || task_hi <= task_lo) return hipSuccess;
    if (!perm) n_virtual = n_slots;
#define WR_LAUNCH_SOFT(NB) hipLaunchKernelGGL(wr::soft::decode_soft_kernel<NB>, dim3(n_waves), dim3(64), 0, st, n_slots, max_sym, \
                                              llr_bits, frames, llr, psdu, psdu_stride, scratch, scratch_stride, n_steps_cap, n_waves, \
                                              perm, n_virtual, task_lo, task_hi)
    switch (nb) {
    case 1: WR_LAUNCH_SOFT(1); break;
    case 2: WR_LAUNCH_SOFT(2); break;
    case 4: WR_LAUNCH_SOFT(4); break;
    case 6: WR_LAUNCH_SOFT(6); break;
    default: return hipErrorInvalidValue;
    }
#undef WR_LAUNCH_SOFT
    return hipGetLastError();
}

extern "C" hipError_t wr_launch_decode_soft_bf16(hipStream_t st, int nb, uint32_t n_slots, uint32_t max_sym, uint32_t llr_bits,
                                                 wifirx_frame* frames, const uint16_t* llr, uint8_t* psdu, uint32_t psdu_stride,
                                                 uint8_t* scratch, size_t scratch_stride, uint32_t n_steps_cap, uint32_t n_waves,
                                                 const uint32_t* perm, uint32_t n_virtual, uint32_t task_lo, uint32_t task_hi)
{
    if (n_slots == 0 || n_waves == 0 || task_hi <= task_lo) return hipSuccess;
    if (!perm) n_virtual = n_slots;
    const float* llr_f = reinterpret_cast<const float*>(llr);      // (the kernel's parameter; BF reads it as uint16_t)
#define WR_LAUNCH_SOFT(NB) hipLaunchKernelGGL((wr::soft::decode_soft_kernel<NB, true>), dim3(n_waves), dim3(64), 0, st, n_slots, max_sym, \
                                              llr_bits, frames, llr_f, psdu, psdu_stride, scratch, scratch_stride, n_steps_cap, n_waves, \
                                              perm, n_virtual, task_lo, task_hi)
    switch (nb) {
    case 1: WR_LAUNCH_SOFT(1); break;
    case 2: WR_LAUNCH_SOFT(2); break;
    case 4: WR_LAUNCH_SOFT(4); break;
    case 6: WR_LAUNCH_SOFT(6); break;
    default: return hipErrorInvalidValue;
    }
#undef WR_LAUNCH_SOFT
    return hipGetLastError();
}
