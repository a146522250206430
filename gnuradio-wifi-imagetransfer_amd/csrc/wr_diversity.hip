// wr_diversity.hip -- receive diversity (NUMERICS.md rule 23): the equalised points of up to 8 antennas' batches, slot for
// slot the same transmissions, become one batch of points, decisions and LLRs for decode_mac -- maximal-ratio combining
// with the |H|^2 of each antenna's LS estimate as the weight (rule 12's), or selection of the antenna with the best SNR.
//
// One wave per slot, four waves per workgroup, a capped grid striding over the slots.  A wave
//   1. reads the A records (the same address in every lane; the words move to scalar registers) and settles the reference
//      antenna r and the contributing set C: wave-uniform, so every later branch on them is a scalar branch;
//   2. lanes 0..47, one data carrier each: the weights w_a, their sum W, the normalised u_a = w_a / W and W_eff into the
//      wave's own piece of LDS (9 x 48 floats); a carrier that falls back to selection carries u_r = -1 (a true u is
//      never negative);
//   3. streams the slot's contiguous n_sym x 48 points, four consecutive points per lane (48 = 12 x 4: a lane's four stay
//      inside one symbol): two 16-byte loads per contributing antenna, two 16-byte stores of points, one dword of
//      decisions, n_bpsc 16-byte stores of LLRs (bf16: half as many bytes).
// The kernel is bound by memory: per point it moves 8 |C| + 8 bytes of points, 1 of decisions and 4 n_bpsc of LLRs.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wr_quad.h"      // decide(), the slicer constants, bf16_pk, fma_
#include "wr_diversity.h"

namespace wr {

namespace {

constexpr uint32_t DIV_WAVES = 4;
constexpr uint32_t DIV_THREADS = 64 * DIV_WAVES;
constexpr uint32_t DIV_BLOCKS_PER_CU = 8;
constexpr uint32_t DIV_LDS_FLOATS = (WR_DIV_MAX_ANT + 1) * 48;      // u_a[k], a = 0..7, and W_eff[k] behind them

typedef float    div_f4 __attribute__((ext_vector_type(4)));
typedef uint32_t div_u4 __attribute__((ext_vector_type(4)));
typedef uint32_t div_u2 __attribute__((ext_vector_type(2)));

// a value that every lane of the wave holds alike, moved to a scalar register: what depends on it branches on the scalar side
__device__ __forceinline__ uint32_t uniform(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

// the occupied index (0..51, pilots at 5, 19, 32, 46) of data carrier k = 0..47
__device__ __forceinline__ int occupied_of(int k) { return k + (k >= 5) + (k >= 18) + (k >= 30) + (k >= 43); }

__device__ __forceinline__ int n_bpsc_of(uint32_t enc) { return enc < 2 ? 1 : enc < 4 ? 2 : enc < 6 ? 4 : 6; }

// What step 1 settled for a slot; every member is wave-uniform.
struct DivSlot {
    uint32_t cmask;       // bit a: antenna a contributes
    int      r, c0;       // the reference antenna; the lowest contributing one
    bool     single;      // |C| = 1: every carrier is the reference antenna's
    uint32_t n_sym;
    size_t   row;         // the slot's first point: slot * max_sym * 48
};

// step 3 for NB bits per carrier; BF: bf16 LLR rows
template <int NB, bool BF>
__device__ __forceinline__ void div_stream(const DivArgs& A, const DivSlot& S, const float* lds, int lane, bool want_llr)
{
    const uint32_t groups = S.n_sym * 12u;
#pragma unroll 1
    for (uint32_t g = (uint32_t)lane; g < groups; g += 64u) {
        const uint32_t k0 = (g % 12u) * 4u;
        const size_t p = S.row + (size_t)g * 4u;
        c32 acc[4] = { { 0.0f, 0.0f }, { 0.0f, 0.0f }, { 0.0f, 0.0f }, { 0.0f, 0.0f } }, yr[4] = { { 0.0f, 0.0f }, { 0.0f, 0.0f }, { 0.0f, 0.0f }, { 0.0f, 0.0f } };
#pragma unroll
        for (int a = 0; a < WR_DIV_MAX_ANT; a++) {
            if (!((S.cmask >> a) & 1u)) continue;                    // scalar branch
            const div_f4* cp = reinterpret_cast<const div_f4*>(A.carrier[a] + 2 * p);
            const div_f4 v0 = cp[0], v1 = cp[1];
            const c32 y[4] = { { v0.x, v0.y }, { v0.z, v0.w }, { v1.x, v1.y }, { v1.z, v1.w } };
            if (a == S.r) {
#pragma unroll
                for (int j = 0; j < 4; j++) yr[j] = y[j];
            }
            if (!S.single) {
                const div_f4 u4 = *reinterpret_cast<const div_f4*>(lds + 48 * a + k0);
                const float u[4] = { u4.x, u4.y, u4.z, u4.w };
                if (a == S.c0) {
#pragma unroll
                    for (int j = 0; j < 4; j++) acc[j] = { u[j] * y[j].re, u[j] * y[j].im };
                } else {
#pragma unroll
                    for (int j = 0; j < 4; j++) acc[j] = { fma_(u[j], y[j].re, acc[j].re), fma_(u[j], y[j].im, acc[j].im) };
                }
            }
        }
        c32 Y[4];
        if (S.single) {
#pragma unroll
            for (int j = 0; j < 4; j++) Y[j] = yr[j];
        } else {
            const div_f4 ur4 = *reinterpret_cast<const div_f4*>(lds + 48 * S.r + k0);
            const float ur[4] = { ur4.x, ur4.y, ur4.z, ur4.w };
#pragma unroll
            for (int j = 0; j < 4; j++) Y[j] = ur[j] < 0.0f ? yr[j] : acc[j];      // -1: the carrier fell back to selection
        }
        if (A.out_carrier) {
            div_f4* op = reinterpret_cast<div_f4*>(A.out_carrier + 2 * p);
            __builtin_nontemporal_store(div_f4{ Y[0].re, Y[0].im, Y[1].re, Y[1].im }, op);
            __builtin_nontemporal_store(div_f4{ Y[2].re, Y[2].im, Y[3].re, Y[3].im }, op + 1);
        }
        if (A.out_idx)
            *reinterpret_cast<uint32_t*>(A.out_idx + p) = (uint32_t)decide(Y[0], NB) | ((uint32_t)decide(Y[1], NB) << 8) |
                                                           ((uint32_t)decide(Y[2], NB) << 16) | ((uint32_t)decide(Y[3], NB) << 24);
        if (want_llr) {
            float V[4 * NB];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                float L[NB];
                llr_of_point<NB>(Y[j], L);
#pragma unroll
                for (int b = 0; b < NB; b++) V[NB * j + b] = L[b];
            }
            if (A.llr_csi) {
                const div_f4 w4 = *reinterpret_cast<const div_f4*>(lds + 48 * WR_DIV_MAX_ANT + k0);
                const float w[4] = { w4.x, w4.y, w4.z, w4.w };
#pragma unroll
                for (int j = 0; j < 4; j++)
#pragma unroll
                    for (int b = 0; b < NB; b++) V[NB * j + b] = V[NB * j + b] * w[j];
            }
            // the group's first value: (slot row + point) * n_bpsc, rows of max_sym * 48 * llr_bits values
            const size_t e = (S.row * A.llr_bits) + (size_t)g * (4u * NB);
            if constexpr (BF) {
                uint16_t* lp = reinterpret_cast<uint16_t*>(A.out_llr) + e;
                if constexpr (NB == 1) {
                    __builtin_nontemporal_store(div_u2{ bf16_pk(V[0], V[1]), bf16_pk(V[2], V[3]) }, reinterpret_cast<div_u2*>(lp));
                } else {
#pragma unroll
                    for (int j = 0; j < NB / 2; j++)
                        __builtin_nontemporal_store(div_u4{ bf16_pk(V[8 * j], V[8 * j + 1]), bf16_pk(V[8 * j + 2], V[8 * j + 3]),
                                                            bf16_pk(V[8 * j + 4], V[8 * j + 5]), bf16_pk(V[8 * j + 6], V[8 * j + 7]) },
                                                    reinterpret_cast<div_u4*>(lp) + j);
                }
            } else {
                div_f4* lp = reinterpret_cast<div_f4*>(reinterpret_cast<float*>(A.out_llr) + e);
#pragma unroll
                for (int j = 0; j < NB; j++)
                    __builtin_nontemporal_store(div_f4{ V[4 * j], V[4 * j + 1], V[4 * j + 2], V[4 * j + 3] }, lp + j);
            }
        }
    }
}

}  // namespace

__global__ __launch_bounds__(DIV_THREADS)
void diversity_kernel(const DivArgs A)
{
    __shared__ __attribute__((aligned(16))) float s_lds[DIV_WAVES * DIV_LDS_FLOATS];
    const int lane = (int)(threadIdx.x & 63u);
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    float* lds = s_lds + wave * DIV_LDS_FLOATS;
    const uint32_t stride = gridDim.x * DIV_WAVES;
#pragma unroll 1
    for (uint32_t slot = blockIdx.x * DIV_WAVES + wave; slot < A.n_slots; slot += stride) {
        // 1. the records: usable antennas, the reference antenna, the contributing set
        uint32_t usable = 0, key[WR_DIV_MAX_ANT], nsym[WR_DIV_MAX_ANT];
        int r = -1;
        float best = 0.0f;
#pragma unroll
        for (int a = 0; a < WR_DIV_MAX_ANT; a++) {
            key[a] = 0; nsym[a] = 0;
            if ((uint32_t)a >= A.n_ant) continue;
            // (whole dwords of the 32-byte record, the same address in every lane: word 5 = snr_db, word 6 =
            // psdu_len | encoding << 16 | n_bpsc << 24, word 7 = n_sym | n_sym_out << 16)
            const uint32_t* f = reinterpret_cast<const uint32_t*>(A.frames[a] + slot);
            const uint32_t flags = uniform(f[0]), w6 = uniform(f[6]), enc = (w6 >> 16) & 0xffu, ns = uniform(f[7]) & 0xffffu;
            const float snr = __uint_as_float(uniform(f[5]));
            key[a] = enc | ((w6 & 0xffffu) << 8);
            nsym[a] = ns;
            // (a record whose rate or length cannot have come from the demod of this row layout is not usable: nothing is
            // read or written outside the rows)
            const bool ok = (flags & (WIFIRX_F_SIGNAL | WIFIRX_F_COMPLETE)) == (WIFIRX_F_SIGNAL | WIFIRX_F_COMPLETE) && enc <= 7u && ns <= A.max_sym;
            if (ok) {
                usable |= 1u << a;
                if (r < 0 || snr > best) { r = a; best = snr; }
            }
        }
        if (r < 0) {
            // no antenna is usable: antenna 0's record, marked as without symbols; nothing else of the slot is written
            if (lane == 0) {
                const div_u4* fp = reinterpret_cast<const div_u4*>(A.frames[0] + slot);
                div_u4 lo = fp[0];
                const div_u4 hi = fp[1];
                lo.x &= ~(WIFIRX_F_COMPLETE | WIFIRX_F_LLR | WIFIRX_F_DECODED | WIFIRX_F_CRC_OK);
                div_u4* op = reinterpret_cast<div_u4*>(A.out_frames + slot);
                op[0] = lo; op[1] = hi;
                if (A.used_mask) A.used_mask[slot] = 0;
            }
            continue;
        }
        uint32_t keyr = 0;
        DivSlot S;
        S.n_sym = 0;
#pragma unroll
        for (int a = 0; a < WR_DIV_MAX_ANT; a++) { keyr = a == r ? key[a] : keyr; S.n_sym = a == r ? nsym[a] : S.n_sym; }
        S.cmask = 0;
#pragma unroll
        for (int a = 0; a < WR_DIV_MAX_ANT; a++) S.cmask |= (((usable >> a) & 1u) && key[a] == keyr) ? 1u << a : 0u;
        if (A.select) S.cmask = 1u << r;
        S.r = r;
        S.c0 = (int)__builtin_ctz(S.cmask);
        S.single = (S.cmask & (S.cmask - 1u)) == 0u;
        S.row = (size_t)slot * A.max_sym * 48u;
        const int nb = n_bpsc_of(keyr & 0xffu);
        const bool want_llr = A.out_llr != nullptr && (uint32_t)nb <= A.llr_bits;

        // 2. weights, once per data carrier
        __builtin_amdgcn_wave_barrier();                 // the previous slot's reads of the piece are done
        if (lane < 48 && (!S.single || (want_llr && A.llr_csi))) {
            const size_t hrow = (size_t)slot * 52u + (size_t)occupied_of(lane);
            float w[WR_DIV_MAX_ANT], W = 0.0f, wr_ = 0.0f;
#pragma unroll
            for (int a = 0; a < WR_DIV_MAX_ANT; a++) {
                w[a] = 0.0f;
                if (!((S.cmask >> a) & 1u)) continue;
                const float2 H = reinterpret_cast<const float2*>(A.csi[a])[hrow];
                float wa = fma_(H.y, H.y, H.x * H.x);
                if (A.has_gain) wa = wa * A.gain[a];
                w[a] = wa;
                W = a == S.c0 ? wa : W + wa;
                wr_ = a == r ? wa : wr_;
            }
            const bool fb = S.single || !(W > 0.0f && W < __builtin_inff());     // not finite, or not > 0
            if (!S.single) {
#pragma unroll
                for (int a = 0; a < WR_DIV_MAX_ANT; a++) {
                    if (!((S.cmask >> a) & 1u)) continue;
                    lds[48 * a + lane] = fb ? (a == r ? -1.0f : 0.0f) : w[a] / W;
                }
            }
            lds[48 * WR_DIV_MAX_ANT + lane] = fb ? wr_ : W;
        }
        __builtin_amdgcn_wave_barrier();

        // 3. the points
        if (A.llr_bf16) {
            if (nb == 1) div_stream<1, true>(A, S, lds, lane, want_llr);
            else if (nb == 2) div_stream<2, true>(A, S, lds, lane, want_llr);
            else if (nb == 4) div_stream<4, true>(A, S, lds, lane, want_llr);
            else div_stream<6, true>(A, S, lds, lane, want_llr);
        } else {
            if (nb == 1) div_stream<1, false>(A, S, lds, lane, want_llr);
            else if (nb == 2) div_stream<2, false>(A, S, lds, lane, want_llr);
            else if (nb == 4) div_stream<4, false>(A, S, lds, lane, want_llr);
            else div_stream<6, false>(A, S, lds, lane, want_llr);
        }

        // the record: the reference antenna's, not yet decoded
        if (lane == 0) {
            const wifirx_frame* fr = A.frames[0] + slot;
#pragma unroll
            for (int a = 1; a < WR_DIV_MAX_ANT; a++) fr = a == r ? A.frames[a] + slot : fr;
            const div_u4* fp = reinterpret_cast<const div_u4*>(fr);
            div_u4 lo = fp[0];
            const div_u4 hi = fp[1];
            lo.x &= ~(WIFIRX_F_LLR | WIFIRX_F_DECODED | WIFIRX_F_CRC_OK);
            if (want_llr) lo.x |= WIFIRX_F_LLR;
            div_u4* op = reinterpret_cast<div_u4*>(A.out_frames + slot);
            op[0] = lo; op[1] = hi;
            if (A.used_mask) A.used_mask[slot] = (uint8_t)S.cmask;
        }
    }
}

}  // namespace wr

extern "C" hipError_t wr_launch_diversity(hipStream_t st, const wr::DivArgs* args, uint32_t n_cu)
{
    if (args->n_slots == 0) return hipSuccess;
    const uint64_t want = ((uint64_t)args->n_slots + wr::DIV_WAVES - 1) / wr::DIV_WAVES;
    const uint64_t cap = (uint64_t)(n_cu ? n_cu : 256u) * wr::DIV_BLOCKS_PER_CU;
    const dim3 grid((uint32_t)(want < cap ? want : cap)), block(wr::DIV_THREADS);
    hipLaunchKernelGGL(wr::diversity_kernel, grid, block, 0, st, *args);
    return hipGetLastError();
}
