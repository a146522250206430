// box_probe -- the same-run, same-process yardstick of bench.py (libboxprobe.so; measurement tooling, NOT part of the
// product ABI: nothing under gnuradio-wifi-imagetransfer_amd/ links or loads it).
//
// The boxes of the pool differ: round 3's driver box ran the store-heavy legs of wr::demod_batch_kernel 12-19 % slower
// than the builder's boxes, and a memory floor quoted from another machine's profile file says nothing about the kernel
// that was just timed.  bench.py therefore calls boxprobe_run() on ITS OWN device buffers (the batch's samples, its idx /
// LLR / carrier rows) right after the timed region and reports, for THIS box in THIS process:
//   out[0] stream_ms     a float4 stream: one 4-kB piece per workgroup, the kernel's read : write byte mix
//   out[1] stream_bytes  the bytes that stream moved (read + written)
//   out[2] combined_ms   the demod kernel's own global loads and stores -- same addresses, order, wave organisation (one
//                        wave = four slots, lane r of a row holds bins r + 16 j, rows written as whole 16-byte pieces),
//                        preamble reads included, no arithmetic: the kernel's memory floor on this box
//   out[3] symbols_ms    the same without the preamble reads
//   out[4] loads_ms      the symbol loop's loads alone
//   out[5] stores_ms     the symbol loop's stores alone
//   out[6] pattern_bytes the bytes the lanes of `combined` move
//   out[7], out[8]       combined / stores alone with plain (temporal) loads and stores
//   out[9], out[10]      combined / stores alone with everything streaming, the decisions' dwords too
// every time the best of `reps` launches after one warm-up launch, HIP events on the null stream.
// The rows it writes are garbage: bench.py calls it after its parity checks.
//   hipcc --offload-arch=gfx950 -O3 -shared -fPIC tools/box_probe.hip -o tools/libboxprobe.so
#include <hip/hip_runtime.h>
#include <stdint.h>

#ifndef BOXPROBE_SRC_SHA
#define BOXPROBE_SRC_SHA "unknown"
#endif

// the symbol loop's loads and stores as the kernel issues them (csrc/wr_quad.h: load_global_f2, store_piece -- both non-temporal)
#ifndef BOXPROBE_NT_LOADS
#define BOXPROBE_NT_LOADS 1
#endif
#ifndef BOXPROBE_NT_STORES
#define BOXPROBE_NT_STORES 1
#endif

typedef float v4f __attribute__((ext_vector_type(4)));
typedef float v2f __attribute__((ext_vector_type(2)));

namespace {

// NT: 1 = as the kernel issues them (streaming sample loads and 16-byte pieces, the decisions' dwords plain: csrc/wr_quad.h
// store_word), 0 = all plain, 2 = everything streaming, the decisions' dwords too
template <int NT> __device__ __forceinline__ float2 ld_sample(const float2* p)
{
    if (NT != 0 && BOXPROBE_NT_LOADS) {
        const v2f v = __builtin_nontemporal_load(reinterpret_cast<const v2f*>(p));
        return make_float2(v.x, v.y);
    }
    return *p;
}
template <int NT> __device__ __forceinline__ void st_piece(char* p, v4f v)
{
    if (NT != 0 && BOXPROBE_NT_STORES) __builtin_nontemporal_store(v, reinterpret_cast<v4f*>(p));
    else *reinterpret_cast<v4f*>(p) = v;
}
template <int NT> __device__ __forceinline__ void st_word(uint8_t* p, uint32_t v)
{
    if (NT == 2 && BOXPROBE_NT_STORES) __builtin_nontemporal_store(v, reinterpret_cast<uint32_t*>(p));
    else *reinterpret_cast<uint32_t*>(p) = v;
}

// NB: bits per sub-carrier (1, 2, 4, 6); CAR: the equalised points leave too (384 B per symbol and frame)
template <int NB, int PRE, int LD, int ST, int CAR, int NT>
__global__ __launch_bounds__(64, 4) void pattern(const float2* __restrict__ x, uint32_t n_slots, int slot_len, int lead,
                                                 int n_sym, uint8_t* __restrict__ idx, float* __restrict__ llr,
                                                 float2* __restrict__ car, float* sink)
{
    const int lane = threadIdx.x & 63, row = lane >> 4, r = lane & 15;
    const uint32_t slot = blockIdx.x * 4 + row;
    if (slot >= n_slots) return;
    const float2* xs = x + (size_t)slot * slot_len;
    float acc = 0.0f;
    if (PRE) {
        // detection: row = slot, blocks of 16 samples up to the trigger (a few samples behind the start of the short preamble);
        // then, per slot by the whole wave, 384 samples from the trigger - 16 on
        const int n_blk = (lead + 64) / 16;
        for (int m = 0; m < n_blk; m++) { const float2 a = xs[16 * m + r]; acc += a.x + a.y; }
        for (int f = 0; f < 4; f++) {
            if (slot - row + f >= n_slots) break;
            const float2* xf = x + (size_t)(slot - row + f) * slot_len;
            for (int p = 0; p < 6; p++) { const float2 a = xf[lead + 16 + 64 * p + lane]; acc += a.x + a.y; }
        }
    }
    constexpr int NK = (12 * NB + 15) / 16, TAIL = 12 * NB - 16 * (NK - 1);
    uint8_t* ip = idx + (size_t)slot * n_sym * 48;
    char* lp = reinterpret_cast<char*>(llr) + (size_t)slot * n_sym * (192 * NB) + 16 * r;
    char* cp = reinterpret_cast<char*>(car) + (size_t)slot * n_sym * 384 + 16 * r;
    const int lts = lead + 192;
    for (int s = 0; s < n_sym + 3; s++) {
        const int off = lts + (s < 2 ? 64 * s : 128 + 80 * (s - 2) + 16);
        float2 v[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            v[j] = make_float2((float)s, (float)j);
            if (LD) v[j] = ld_sample<NT>(xs + off + r + 16 * j);
        }
        if (s >= 3 && ST) {
            const int q = s - 3;
            const v4f w = { v[0].x + v[2].y, v[1].y + v[3].x, v[2].x + v[0].y, v[3].y + v[1].x };     // every loaded component is used
            char* d = lp + (size_t)q * (192 * NB);
#pragma unroll
            for (int k = 0; k < NK; k++)
                if (k < NK - 1 || r < TAIL) st_piece<NT>(d + 256 * k, w);
            if (r < 12) st_word<NT>(ip + q * 48 + 4 * r, __float_as_uint(w.x + w.y));
            if (CAR) {
                char* c = cp + (size_t)q * 384;
                st_piece<NT>(c, w);
                if (r < 8) st_piece<NT>(c + 256, w);
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++) acc += v[j].x + v[j].y;
        }
    }
    if (acc == 12345.678f) sink[0] = acc;
}

// each workgroup owns one contiguous 4-kB piece; wr_num of every wr_den workgroups write theirs to dst
__global__ __launch_bounds__(256) void stream(const v4f* __restrict__ src, v4f* __restrict__ dst, size_t n, int wr_num, int wr_den)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const v4f v = src[i];
    if ((int)(blockIdx.x % wr_den) < wr_num) dst[i] = v;
    else if (v.x + v.y + v.z + v.w == 12345.678f) dst[0] = v;
}

template <typename F> float best_of(F&& launch, int reps, hipEvent_t e0, hipEvent_t e1)
{
    float best = 1e30f;
    for (int it = 0; it <= reps; it++) {
        (void)hipEventRecord(e0, 0);
        launch();
        (void)hipEventRecord(e1, 0);
        (void)hipEventSynchronize(e1);
        float ms = 0.0f;
        (void)hipEventElapsedTime(&ms, e0, e1);
        if (it > 0 && ms < best) best = ms;
    }
    return best;
}

template <int NB, int CAR>
void run_patterns(const float2* x, uint32_t n, int slot_len, int lead, int n_sym, uint8_t* idx, float* llr, float2* car,
                  float* sink, int reps, hipEvent_t e0, hipEvent_t e1, double* out)
{
    const dim3 g((n + 3) / 4), b(64);
#define BP_RUN(PRE, LD, ST, NT) best_of([&] { hipLaunchKernelGGL((pattern<NB, PRE, LD, ST, CAR, NT>), g, b, 0, 0, x, n, slot_len, lead, n_sym, idx, llr, car, sink); }, reps, e0, e1)
    out[2] = BP_RUN(1, 1, 1, 1);
    out[3] = BP_RUN(0, 1, 1, 1);
    out[4] = BP_RUN(0, 1, 0, 1);
    out[5] = BP_RUN(0, 0, 1, 1);
    // what the streaming (non-temporal) forms are worth on THIS box: the same patterns with plain loads and stores, and with
    // the decisions' dwords (48 bytes per row: never a whole line) streaming too
    out[7] = BP_RUN(1, 1, 1, 0);
    out[8] = BP_RUN(0, 0, 1, 0);
    out[9] = BP_RUN(1, 1, 1, 2);
    out[10] = BP_RUN(0, 0, 1, 2);
#undef BP_RUN
}

}  // namespace

extern "C" const char* boxprobe_src_sha(void) { return BOXPROBE_SRC_SHA; }

// x: n_slots x slot_len complex64 (device); idx: n_slots x n_sym x 48 bytes; llr: n_slots x n_sym x 48 x n_bpsc floats;
// car: n_slots x n_sym x 48 complex64 or null.  Returns 0 or a hipError_t.
extern "C" int boxprobe_run(const void* x, void* idx, void* llr, void* car, uint32_t n_slots, int slot_len, int lead,
                            int n_sym, int n_bpsc, int reps, double* out)
{
    if (!x || !idx || !llr || !out || n_slots == 0 || reps < 1) return (int)hipErrorInvalidValue;
    if (n_bpsc != 1 && n_bpsc != 2 && n_bpsc != 4 && n_bpsc != 6) return (int)hipErrorInvalidValue;
    if (lead + 192 + 128 + 80 * (n_sym + 1) > slot_len) return (int)hipErrorInvalidValue;      // the pattern must stay inside a slot
    hipEvent_t e0, e1;
    float* sink = nullptr;
    if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) return (int)hipGetLastError();
    if (hipMalloc(&sink, 4) != hipSuccess) return (int)hipGetLastError();
    (void)hipDeviceSynchronize();
    const double rd_sym = (double)n_slots * (n_sym + 3) * 512.0;
    const double rd_pre = (double)n_slots * ((lead + 64) / 16 * 128.0 + 6 * 512.0);
    const double wr = (double)n_slots * n_sym * (48.0 * (1 + 4 * n_bpsc) + (car ? 384.0 : 0.0));
    out[6] = rd_sym + rd_pre + wr;
    // the stream: read rd bytes of x, write the kernel's share of them into llr (at most what llr holds)
    {
        const double rd = rd_sym + rd_pre;
        const size_t n16 = (size_t)(rd / 16.0);
        const size_t cap16 = (size_t)n_slots * n_sym * 48 * n_bpsc / 4;          // float4s in llr
        const int den = 64;
        int num = (int)(wr / rd * den + 0.5);
        if (num > den) num = den;
        // piece i of x is read and, for num of every den workgroups, written to piece i of llr: the stream is as long as the
        // shorter of the two buffers allows (the samples are n_slots x slot_len x 8 bytes, the LLR rows n_slots x n_sym x 192 n_bpsc)
        const size_t x16 = (size_t)n_slots * (size_t)slot_len * 8 / 16;
        size_t n_run = n16 < cap16 ? n16 : cap16;
        if (n_run > x16) n_run = x16;
        const unsigned blocks_run = (unsigned)((n_run + 255) / 256);
        out[0] = best_of([&] { hipLaunchKernelGGL(stream, dim3(blocks_run), dim3(256), 0, 0, reinterpret_cast<const v4f*>(x),
                                                  reinterpret_cast<v4f*>(llr), n_run, num, den); }, reps, e0, e1);
        out[1] = (double)n_run * 16.0 * (1.0 + (double)num / den);
    }
    const float2* xs = reinterpret_cast<const float2*>(x);
    uint8_t* ip = reinterpret_cast<uint8_t*>(idx);
    float* lp = reinterpret_cast<float*>(llr);
    float2* cp = reinterpret_cast<float2*>(car);
#define BP_NB(NB)                                                                                                \
    { if (car) run_patterns<NB, 1>(xs, n_slots, slot_len, lead, n_sym, ip, lp, cp, sink, reps, e0, e1, out);      \
      else     run_patterns<NB, 0>(xs, n_slots, slot_len, lead, n_sym, ip, lp, cp, sink, reps, e0, e1, out); }
    switch (n_bpsc) {
    case 1: BP_NB(1) break;
    case 2: BP_NB(2) break;
    case 4: BP_NB(4) break;
    default: BP_NB(6) break;
    }
#undef BP_NB
    const hipError_t err = hipDeviceSynchronize();
    (void)hipFree(sink);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    return (int)(err != hipSuccess ? err : hipGetLastError());
}
