// wr_link.hip -- the two ends of the loop-back on the device (gnu_radio/IRS_tranceiver.py: strobe -> ieee802_11.mac -> PHY ...
// -> decode_mac): mac_kernel frames a batch of payloads the way ieee802_11.mac does, link_stats_kernel scores a decoded batch
// against what was sent and leaves nine integers.  Integer arithmetic only: both are exact, whatever the order of execution.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wr_decode.h"      // FinishTables: the CRC-32 tables of decode_mac's finish
#include "wr_link.h"
#include "wr_rng.h"

namespace wr {

namespace {

constexpr uint32_t LINK_THREADS = 256;
constexpr uint32_t MAC_THREADS = 256;
constexpr uint32_t MAC_MAX_FPB = 64;

// Walks the items (f, q), q < width, of a workgroup in steps of MAC_THREADS without a division per item.
struct Walk {
    uint32_t f, q, df, dq, width;
    __device__ Walk(uint32_t tid, uint32_t w) : f(tid / w), q(tid % w), df(MAC_THREADS / w), dq(MAC_THREADS % w), width(w) {}
    __device__ void next()
    {
        f += df;
        q += dq;
        if (q >= width) { q -= width; f++; }
    }
};

// A byte row of `extent` readable bytes at any alignment, as dwords: dword k of the row = two aligned loads and a funnel
// shift.  An aligned dword is loaded only where it holds a byte of the row, so nothing outside the aligned dwords that overlap
// the row is read; what a dword holds behind byte `extent` is whatever lies there, and the caller masks it.
struct ByteRow {
    const uint32_t* base;
    uint32_t sh, end;       // byte offset of the row in its first aligned dword; sh + extent
    __device__ ByteRow(const uint8_t* row, uint32_t extent)
        : base(reinterpret_cast<const uint32_t*>(row - (reinterpret_cast<uintptr_t>(row) & 3u))),
          sh((uint32_t)(reinterpret_cast<uintptr_t>(row) & 3u)), end(sh + extent) {}
    __device__ uint32_t word(uint32_t k) const
    {
        const uint32_t lo = 4 * k < end ? base[k] : 0u;
        const uint32_t hi = (sh != 0 && 4 * (k + 1) < end) ? base[k + 1] : 0u;
        return __builtin_amdgcn_alignbit(hi, lo, 8 * sh);
    }
};

}  // namespace

// ---- ieee802_11.mac over a batch ---------------------------------------------------------------------------------------
// A workgroup takes a.fpb consecutive frames.  Their PSDUs are built in LDS, row f at the byte alignment its row has in global
// memory (byte p of the PSDU at byte (row address & 3) + p of the LDS row), so that the aligned dwords of the two coincide:
// header and payload are written by all lanes, one lane per frame then runs the slice-by-4 CRC over its LDS row with the
// tables of decode_mac's finish (the pitch is odd: the lanes of a wave read their rows from different banks) and appends the
// FCS, and all lanes store the rows as aligned dwords, bytes at the two edges of a row.  Nothing outside
// [row, row + 24 + len + 4) is written.  Six workgroups share a CU (24 KB of LDS each at 294 bytes) and overlap their phases;
// larger or persistent workgroups and slicing by 8 measured slower.
__global__ __launch_bounds__(MAC_THREADS)
void mac_kernel(const MacArgs a)
{
    __shared__ FinishTables ft;
    __shared__ uint32_t s_len[MAC_MAX_FPB], s_sh[MAC_MAX_FPB];
    __shared__ __attribute__((aligned(4))) uint8_t s_hdr[24];
    extern __shared__ __attribute__((aligned(16))) uint32_t rows[];
    const uint32_t tid = threadIdx.x;
    const uint32_t pitch = a.pitch, pitch_b = 4 * a.pitch;
    uint8_t* rb = reinterpret_cast<uint8_t*>(rows);

    build_finish_tables(ft);
    if (tid < 6)      // (a select chain: a lane-indexed read of the kernel arguments would go through scratch memory)
        reinterpret_cast<uint32_t*>(s_hdr)[tid] = tid == 0 ? a.hdr[0] : tid == 1 ? a.hdr[1] : tid == 2 ? a.hdr[2] : tid == 3 ? a.hdr[3]
                                                  : tid == 4 ? a.hdr[4] : a.hdr[5];
    const uint32_t f0 = blockIdx.x * a.fpb;
    const uint32_t nf = min(a.fpb, a.n_frames - f0);
    if (tid < nf) {
        s_len[tid] = a.len ? a.len[f0 + tid] : a.len_all;
        s_sh[tid] = (uint32_t)(reinterpret_cast<uintptr_t>(a.psdu + (uint64_t)(f0 + tid) * a.psdu_stride) & 3u);
    }
    __syncthreads();

    // header: 24 bytes per frame, the sequence number in bytes 22, 23
    for (Walk w(tid, 24); w.f < nf; w.next()) {
        const uint32_t seq = ((a.seq0 + f0 + w.f) & 0xFFFu) << 4;
        const uint32_t v = w.q == 22 ? (seq & 0xFFu) : w.q == 23 ? (seq >> 8) : s_hdr[w.q];
        rb[w.f * pitch_b + s_sh[w.f] + w.q] = (uint8_t)v;
    }
    // payload
    if (a.payload) {
        // lane per dword of a payload, whatever the alignment of the two rows; the last, partial one byte by byte.  The
        // loop is bound by the latency of a load followed by a store: four loads are in flight per lane
        const uint32_t width = max((a.len_max + 3u) >> 2, 1u);
        for (Walk w(tid, width); w.f < nf;) {
            uint32_t v[4], off[4], cnt[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                cnt[u] = 0;
                if (w.f < nf) {
                    const uint32_t len = s_len[w.f];
                    if (4 * w.q < len) {
                        cnt[u] = min(len - 4 * w.q, 4u);
                        off[u] = w.f * pitch_b + s_sh[w.f] + 24 + 4 * w.q;
                        v[u] = ByteRow(a.payload + (uint64_t)(f0 + w.f) * a.payload_stride, len).word(w.q);
                    }
                }
                w.next();
            }
#pragma unroll
            for (int u = 0; u < 4; u++) {
                if (cnt[u] == 4 && (off[u] & 3u) == 0) rows[off[u] >> 2] = v[u];
                else
                    for (uint32_t k = 0; k < cnt[u]; k++) rb[off[u] + k] = (uint8_t)(v[u] >> (8 * k));
            }
        }
    } else {
        // lane per Philox block: bytes 16 j .. 16 j + 15 of frame i = the words of philox4x32_10((j, i, 0, 0), seed)
        const uint32_t n_blk = max((a.len_max + 15u) >> 4, 1u);
        const uint2 key = make_uint2((uint32_t)a.seed, (uint32_t)(a.seed >> 32));
        for (Walk w(tid, n_blk); w.f < nf; w.next()) {
            const uint32_t len = s_len[w.f], p0 = 16 * w.q;
            if (p0 >= len) continue;
            const uint4 r = philox4x32_10(make_uint4(w.q, f0 + w.f, 0u, 0u), key);
            const uint32_t v[4] = { r.x, r.y, r.z, r.w };
            const uint32_t off = w.f * pitch_b + s_sh[w.f] + 24 + p0;
            if (p0 + 16 <= len && (off & 3u) == 0) {
#pragma unroll
                for (int k = 0; k < 4; k++) rows[(off >> 2) + k] = v[k];
            } else if (p0 + 16 <= len && (off & 1u) == 0) {
                uint16_t* rh = reinterpret_cast<uint16_t*>(rb + off);
#pragma unroll
                for (int k = 0; k < 8; k++) rh[k] = (uint16_t)(v[k >> 1] >> (16 * (k & 1)));
            } else {
#pragma unroll
                for (int k = 0; k < 16; k++)
                    if (p0 + k < len) rb[off + k] = (uint8_t)(v[k >> 2] >> (8 * (k & 3)));
            }
        }
    }
    __syncthreads();

    // CRC-32 of header + payload, one lane per frame; the FCS behind them, little endian
    if (tid < nf) {
        const uint32_t body = 24 + s_len[tid], sh8 = 8 * s_sh[tid];
        const uint32_t* r = rows + tid * pitch;
        uint32_t crc = 0xffffffffu, w0 = r[0];
        const uint32_t n_words = body >> 2;
        for (uint32_t k = 0; k < n_words; k++) {
            const uint32_t w1 = r[k + 1];
            const uint32_t x = crc ^ __builtin_amdgcn_alignbit(w1, w0, sh8);
            w0 = w1;
            crc = ft.crc[3][x & 0xffu] ^ ft.crc[2][(x >> 8) & 0xffu] ^ ft.crc[1][(x >> 16) & 0xffu] ^ ft.crc[0][x >> 24];
        }
        const uint32_t d = __builtin_amdgcn_alignbit(r[n_words + 1], w0, sh8);
        for (uint32_t b = 0; b < (body & 3u); b++) crc = (crc >> 8) ^ ft.crc[0][(crc ^ (d >> (8 * b))) & 0xffu];
        crc = ~crc;
        uint8_t* fcs = rb + tid * pitch_b + s_sh[tid] + body;
#pragma unroll
        for (int b = 0; b < 4; b++) fcs[b] = (uint8_t)(crc >> (8 * b));
    }
    __syncthreads();

    // rows out: aligned dwords inside a row, bytes where a dword straddles one of its ends
    for (Walk w(tid, pitch); w.f < nf; w.next()) {
        const uint32_t lo = s_sh[w.f], hi = lo + 24 + s_len[w.f] + 4, b0 = 4 * w.q;
        if (b0 + 4 <= lo || b0 >= hi) continue;
        uint8_t* p = a.psdu + (uint64_t)(f0 + w.f) * a.psdu_stride - lo + b0;      // 4-byte aligned
        const uint32_t v = rows[w.f * pitch + w.q];
        if (b0 >= lo && b0 + 4 <= hi) {
            *reinterpret_cast<uint32_t*>(p) = v;
        } else {
#pragma unroll
            for (int b = 0; b < 4; b++)
                if (b0 + b >= lo && b0 + b < hi) p[b] = (uint8_t)(v >> (8 * b));
        }
    }
}

// ---- scoring a decoded batch ------------------------------------------------------------------------------------------
namespace {

__device__ __forceinline__ uint32_t wave_sum(uint32_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

enum { LC_FRAMES, LC_REF, LC_GOOD, LC_CRC, LC_PSDU_OK, LC_CRC_WRONG, LC_BITS, LC_ERR, LC_ERR_SQ, LC_N };

}  // namespace

// One wave per frame (the frame index is wave-uniform: the records come through scalar loads), 16 bytes of decisions and 4
// bytes of each PSDU per lane and load.  What a frame needs is known only from its records, but where its rows lie is not:
// the first 64 loads of every row are issued together with the record loads and masked afterwards (a frame of config 3
// has 33 of decisions and 74 of PSDU), so that a wave waits for memory once per frame, not twice.  Counters are kept per
// wave, added per workgroup in LDS, then one 64-bit atomic add per counter and workgroup.
// BY_RATE (wifirx_link_stats_by_rate): the same counters once more per encoding of the reference record, behind the totals
// (a.counts[LC_N (1 + e) + i]).  A frame's nine contributions go from lanes 0..8 of its wave into the workgroup's LDS row of
// its rate with one atomic instruction per frame -- eight more sets of per-wave counters would not fit the registers --, and
// the rows into global memory at the end like the totals.
template <bool BY_RATE>
__global__ __launch_bounds__(LINK_THREADS)
void link_stats_kernel(const LinkArgs a)
{
    __shared__ unsigned long long s_cnt[BY_RATE ? 9 * LC_N : LC_N];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    if (tid < (BY_RATE ? 9 * LC_N : LC_N)) s_cnt[tid] = 0;
    __syncthreads();

    unsigned long long c[LC_N] = {};
    const uint32_t n_waves = gridDim.x * (LINK_THREADS / 64);
    const bool have_psdu = a.rx_psdu != nullptr, have_dec = a.rx_dec != nullptr;
    for (uint32_t f = blockIdx.x * (LINK_THREADS / 64) + wave; f < a.n_slots; f += n_waves) {
        // the first 64 loads of the rows, whatever the records will say (inside the rows: they are allocated in full)
        const uint4* p4 = reinterpret_cast<const uint4*>(a.rx_dec + (uint64_t)f * a.dec_row_words);
        const uint4* q4 = reinterpret_cast<const uint4*>(a.ref_dec + (uint64_t)f * a.dec_row_words);
        uint4 x0 = make_uint4(0, 0, 0, 0), y0 = x0;
        if (have_dec && lane < (a.dec_row_words >> 2)) { x0 = p4[lane]; y0 = q4[lane]; }
        const ByteRow pr(a.rx_psdu + (uint64_t)f * a.rx_psdu_stride, a.rx_psdu_stride);
        const ByteRow qr(a.ref_psdu + (uint64_t)f * a.ref_psdu_stride, a.ref_psdu_stride);
        uint32_t pw0 = 0, qw0 = 0;
        if (have_psdu) { pw0 = pr.word(lane); qw0 = qr.word(lane); }

        const wifirx_frame rx = a.rx_frames[f];
        const wifirx_frame rf = a.ref_frames[f];
        const bool ref_c = (rf.flags & WIFIRX_F_COMPLETE) != 0;
        const uint32_t n_sym = rx.n_sym, len = rx.psdu_len;
        const bool good = ref_c && (rx.flags & WIFIRX_F_COMPLETE) && rx.encoding == rf.encoding && rx.encoding < 8 &&
                          len == rf.psdu_len && n_sym == rf.n_sym && n_sym <= a.max_sym;
        const bool crc_ok = ref_c && (rx.flags & WIFIRX_F_CRC_OK) && have_psdu;
        bool psdu_ok = false;
        if (crc_ok && len == rf.psdu_len && len <= a.rx_psdu_stride && len <= a.ref_psdu_stride) {
            const uint32_t n_words = (len + 3) >> 2;
            const uint32_t last = (len & 3u) ? (1u << (8 * (len & 3u))) - 1u : 0xffffffffu;
            bool diff = lane < n_words && ((pw0 ^ qw0) & (lane + 1 == n_words ? last : 0xffffffffu)) != 0;
            for (uint32_t k = lane + 64; k < n_words; k += 64)
                diff |= ((pr.word(k) ^ qr.word(k)) & (k + 1 == n_words ? last : 0xffffffffu)) != 0;
            psdu_ok = __ballot(diff) == 0;
        }
        uint32_t e = 0xffffffffu;
        unsigned long long f_bits = 0;
        if (good && have_dec) {
            const uint32_t nb = (uint32_t)nbpsc_of(rx.encoding);
            const uint32_t n_words = (a.dec_is_hbits ? 2 * nb : 12u) * n_sym, n_quads = n_words >> 2;
            const uint32_t* p = reinterpret_cast<const uint32_t*>(p4);
            const uint32_t* q = reinterpret_cast<const uint32_t*>(q4);
            uint32_t s = lane < n_quads ? __popc(x0.x ^ y0.x) + __popc(x0.y ^ y0.y) + __popc(x0.z ^ y0.z) + __popc(x0.w ^ y0.w) : 0u;
            for (uint32_t k = lane + 64; k < n_quads; k += 64) {
                const uint4 x = p4[k], y = q4[k];
                s += __popc(x.x ^ y.x) + __popc(x.y ^ y.y) + __popc(x.z ^ y.z) + __popc(x.w ^ y.w);
            }
            const uint32_t t = (n_words & ~3u) + lane;
            if (lane < 3 && t < n_words) s += __popc(p[t] ^ q[t]);
            e = wave_sum(s);
            f_bits = (unsigned long long)n_sym * 48u * nb;
            c[LC_BITS] += f_bits;
            c[LC_ERR] += e;
            c[LC_ERR_SQ] += (unsigned long long)e * e;
        }
        c[LC_FRAMES] += 1;
        c[LC_REF] += ref_c;
        c[LC_GOOD] += good;
        c[LC_CRC] += crc_ok;
        c[LC_PSDU_OK] += psdu_ok;
        c[LC_CRC_WRONG] += crc_ok && !psdu_ok;
        if constexpr (BY_RATE) {
            if (ref_c && rf.encoding < 8 && lane < LC_N) {      // (a reference record that is not complete lands in no rate)
                const bool scored = f_bits != 0;
                const unsigned long long v = lane == LC_FRAMES || lane == LC_REF ? 1ull : lane == LC_GOOD ? (unsigned long long)good
                    : lane == LC_CRC ? (unsigned long long)crc_ok : lane == LC_PSDU_OK ? (unsigned long long)psdu_ok
                    : lane == LC_CRC_WRONG ? (unsigned long long)(crc_ok && !psdu_ok) : lane == LC_BITS ? f_bits
                    : !scored ? 0ull : lane == LC_ERR ? (unsigned long long)e : (unsigned long long)e * e;
                if (v) atomicAdd(&s_cnt[LC_N * (1 + rf.encoding) + lane], v);
            }
        }
        if (lane == 0) {
            if (a.frame_err) a.frame_err[f] = e;
            if (a.frame_class) a.frame_class[f] = (uint8_t)((good ? 1 : 0) | (crc_ok ? 2 : 0) | (psdu_ok ? 4 : 0) | (ref_c ? 8 : 0));
        }
    }
    if (lane == 0)
#pragma unroll
        for (int i = 0; i < LC_N; i++)
            if (c[i]) atomicAdd(&s_cnt[i], c[i]);
    __syncthreads();
    if (tid < (BY_RATE ? 9 * LC_N : LC_N) && s_cnt[tid]) atomicAdd(&a.counts[tid], s_cnt[tid]);
}

}  // namespace wr

extern "C" void wr_mac_geometry(uint32_t max_psdu, uint32_t* pitch, uint32_t* fpb)
{
    // a row holds up to 3 bytes of alignment + the PSDU, and one dword more for the CRC loop's look-ahead
    const uint32_t p = ((max_psdu + 3 + 3) / 4 + 1) | 1u;
    *pitch = p;
    *fpb = p <= 160 ? wr::MAC_MAX_FPB : wr::MAC_MAX_FPB / 2;     // rows of a group: at most 40 KB, 49 KB for the longest PSDUs
}

extern "C" hipError_t wr_launch_mac(hipStream_t st, const wr::MacArgs* args)
{
    if (args->n_frames == 0) return hipSuccess;
    // one group per workgroup: with 24 KB of LDS each at config 3's 294 bytes, six of them share a CU and overlap their phases
    const dim3 grid((args->n_frames + args->fpb - 1) / args->fpb), block(wr::MAC_THREADS);
    hipLaunchKernelGGL(wr::mac_kernel, grid, block, (size_t)args->fpb * args->pitch * 4, st, *args);
    return hipGetLastError();
}

extern "C" hipError_t wr_launch_link_stats(hipStream_t st, const wr::LinkArgs* args, uint32_t n_simd)
{
    if (args->n_slots == 0) return hipSuccess;
    const uint32_t per = wr::LINK_THREADS / 64;
    const uint32_t want = (args->n_slots + per - 1) / per, cap = 2 * (n_simd ? n_simd : 1024u);      // 8 waves per SIMD
    const dim3 grid(want < cap ? want : cap), block(wr::LINK_THREADS);
    if (args->by_rate) hipLaunchKernelGGL(wr::link_stats_kernel<true>, grid, block, 0, st, *args);
    else hipLaunchKernelGGL(wr::link_stats_kernel<false>, grid, block, 0, st, *args);
    return hipGetLastError();
}
