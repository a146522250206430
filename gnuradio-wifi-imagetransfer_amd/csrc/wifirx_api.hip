// wifirx_api.hip -- implementation of the C ABI in include/wifirx.h on top of the HIP kernels.
// Host side only: handles, the per-handle HIP stream, workspaces, host<->device staging.
// No CPU compute fallback exists: every entry point needs a gfx950 device.
#include <hip/hip_runtime.h>
#include <emmintrin.h>      // SSE2 streaming stores of the staging copy (x86-64 baseline)

#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <condition_variable>
#include <deque>
#include <memory>
#include <mutex>
#include <new>
#include <optional>
#include <thread>
#include <string>
#include <vector>

#include "wifirx.h"
#include "wr_kernels.h"
#include "wr_tx.h"
#include "wr_channel.h"
#include "wr_irs.h"
#include "wr_irs_sweep.h"
#include "wr_irs_estimate.h"
#include "wr_irs_optimize.h"
#include "wr_link.h"
#include "wr_convert.h"
#include "wr_frontend.h"
#include "wr_channelizer.h"
#include "wr_combiner.h"
#include "wr_arb.h"
#include "wr_arb_table.h"
#include "wr_spectrum.h"
#include "wr_diversity.h"
#include "wr_precombine.h"
#include "wr_detect_multi.h"

// The stream's per-frame outputs (stream_outs, wifirx_api_stream.inc) and the host copy of a batch of them, shared by its
// frames: output o of frame k is the width[o] bytes at blob[off[o] + k * width[o]] (width 0: the handle did not produce o).
// A PolledFrame is a finished frame of the stream: its record and its row k of the batch it came with.
enum StreamOutput { SO_PSDU, SO_IDX, SO_CAR, SO_CSI, SO_STATS, SO_N };
// A batch of the diversity stream also carries, per frame k, used[k] = the contributing antennas and ant[k * n_ant + a] =
// antenna a's own record (n_ant = 0: a batch of the single stream).
struct StreamBatch {
    std::vector<uint8_t> blob; size_t off[SO_N], width[SO_N];
    uint32_t n_ant; std::vector<uint8_t> used; std::vector<wifirx_frame> ant;
};
struct PolledFrame { wifirx_frame fr; std::shared_ptr<const StreamBatch> batch; uint32_t k; };

struct PendingTrig {
    int64_t pos;        // absolute stream index of the trigger
    float   cfo;        // coarse CFO, valid once the frame kernel has seen the trigger (have_cfo)
    bool    have_cfo;
};

namespace {

int oom(wifirx_handle* h, const char* what, hipError_t e);

// An owning device (hipMalloc) or pinned host (hipHostMalloc) allocation: freed by its destructor, moved, never copied.
template <bool Pinned>
struct Buffer {
    void*  p = nullptr;
    size_t bytes = 0;

    Buffer() = default;
    Buffer(const Buffer&) = delete;
    Buffer& operator=(const Buffer&) = delete;
    Buffer(Buffer&& o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
    Buffer& operator=(Buffer&& o) noexcept
    {
        if (this != &o) { reset(); std::swap(p, o.p); std::swap(bytes, o.bytes); }
        return *this;
    }
    ~Buffer() { reset(); }

    template <class T> T* as() const { return static_cast<T*>(p); }
    void reset()
    {
        if (p) (void)(Pinned ? hipHostFree(p) : hipFree(p));
        p = nullptr;
        bytes = 0;
    }
    // exactly `n` bytes; what the buffer held is freed first, and a failure leaves it empty
    int alloc(wifirx_handle* h, size_t n, const char* what)
    {
        reset();
        hipError_t e = Pinned ? hipHostMalloc(&p, n, hipHostMallocDefault) : hipMalloc(&p, n);
        if (e != hipSuccess) { p = nullptr; return oom(h, what, e); }
        bytes = n;
        return WIFIRX_OK;
    }
    // at least `need` bytes: a device buffer grows to exactly `need`, a pinned one to half as much again
    int reserve(wifirx_handle* h, size_t need)
    {
        if (bytes >= need) return WIFIRX_OK;
        return Pinned ? alloc(h, need + need / 2, "hipHostMalloc") : alloc(h, need, "hipMalloc");
    }
};
using DevBuf = Buffer<false>;
using PinnedBuf = Buffer<true>;

// wifirx_set_param's settings beyond the wifirx_config
struct Tunables {
    int32_t  llr_csi = 0;                              // WIFIRX_P_LLR_CSI
    int32_t  llr_format = WIFIRX_LLR_F32;              // WIFIRX_P_LLR_FORMAT: the LLR rows of the batch calls (stream mode keeps float32)
    int32_t  stream_want_idx = 1;                      // WIFIRX_P_STREAM_IDX
    int32_t  stream_soft = 0;                          // WIFIRX_P_STREAM_SOFT: stream batches decoded from LLRs (wifirx_decode_batch_soft)
    int64_t  stream_batch = 0;                         // WIFIRX_P_STREAM_BATCH
    uint32_t decode_small_max = WR_DECODE_SMALL_MAX;   // WIFIRX_P_DECODE_SMALL_MAX
};

// Environment overrides and test hooks, read once by wifirx_create (read_environment)
struct Environment {
    uint32_t decode_fpw = 0;        // WIFIRX_DECODE_FPW (tests): frames per wave of the throughput decoder
    int      decode_ovl = -1;       // WIFIRX_DECODE_OVL (tests): 0 = trace-back behind each task, 2 = speculative walks under the task's own add-compare-select; -1: by batch size
    int      decode_q = -1;         // WIFIRX_DECODE_Q (tests): 1 / 0 = always / never the four-frames-per-lane decoder; -1: by batch size
    int      fail_alloc = 0, alloc_count = 0;      // WIFIRX_TEST_FAIL_ALLOC (allocation-failure tests)
    size_t   decode_budget = 0;                    // WIFIRX_TEST_DECODE_BUDGET: bytes of survivor scratch a decode call may hold (tests)
    int      fail_decode_scratch = 0;              // WIFIRX_TEST_FAIL_DECODE_SCRATCH: the next k scratch allocations fail (tests)
    int      fail_carry = 0, carry_count = 0;      // WIFIRX_TEST_FAIL_CARRY (a failure behind the commit of a stream pass)
};

// batch staging (host-buffer path only)
struct Staging {
    DevBuf iq, frames, idx, llr, car, csi, stats, hbits;
    DevBuf off;                     // slot offsets of wifirx_demod_batch_v
    DevBuf tx_psdu, tx_meta;        // wifirx_tx_batch: host PSDUs; lengths, seeds, row offsets
    DevBuf ch_meta;                 // wifirx_channel: host taps, phase increments, row offsets, tile bases
    DevBuf irs_meta;                // wifirx_irs_taps: line-of-sight vectors, tap scales, host psi
    DevBuf irs_obs, irs_psi;        // wifirx_irs_estimate: the observations without an obs_out; the decided phases for the taps
    DevBuf link_meta, link_payload; // wifirx_mac_batch: payload lengths; host payloads
    DevBuf link_counts;             // wifirx_link_stats: the nine counters
    DevBuf iq_clipped;              // wifirx_iq_from_f32: the counter of clipped components
    DevBuf fe_table;                // wifirx_frontend and the stream's front end: the block sums of a call
};

// decode workspace
struct DecodeWork {
    DevBuf scratch, max;
    DevBuf perm;                    // decode_mac over several rates: frames grouped by rate
    DevBuf hbits;                   // decode_mac over `idx` alone: its bit planes (wifirx_out.hbits form)
};

// stream mode (wifirx_api_stream.inc), of both kinds of stream: the single stream is a stream of one sample plane, the
// diversity stream one of div.n_ant planes that fill, are scanned and are carried together
struct StreamState {
    DevBuf   sbuf;                  // the sample planes, plane a at sbuf + a * sbuf_cap samples (stream_plane)
    DevBuf   native;                // host input in an integer format: every plane's chunk of a pass, widened from here into the planes
    DevBuf   above, A;              // the detection side buffers, sized by sbuf_cap too
    int64_t  sbuf_cap = 0;          // samples a plane holds
    int64_t  sbase = 0;             // absolute index of a plane's first sample (multiple of 64)
    int64_t  sfill = 0;             // valid samples in every plane
    int64_t  sdetected = 0;         // absolute index up to which triggers have been selected
    int64_t  sprocessed = 0;        // absolute index up to which pushes have been processed
    int64_t  last_trig = -(1ll << 40);
    std::vector<PendingTrig> pending;
    std::deque<PolledFrame>  queue;
    std::atomic<uint32_t> n_queued{0};  // frames waiting for wifirx_poll (wifirx_queued: read without the lock)
    DevBuf   trig, frames, idx, car, psdu, csi, stats, hbits;     // output rows of out_cap triggers
    uint32_t out_cap = 0;
    DevBuf   llr;                   // WIFIRX_P_STREAM_SOFT: LLR rows of the triggers (6 bits per carrier reserved)
    DevBuf   pack;                  // stream outputs, rows cut to their filled width
    PinnedBuf host;                 // pinned landing zone of the packed outputs
    bool     dead = false;          // the carry step failed after it had begun to move the sample planes
    std::string dead_msg;
    size_t   push_consumed = 0;     // wifirx_push_consumed
    bool     single = false;        // wifirx_push / wifirx_push_iq has handed in samples: no wifirx_push_diversity on this handle
    bool     fe_on = false;         // wifirx_stream_frontend: the front end (NUMERICS.md rule 32) runs on the samples a pass appends
    wifirx_frontend_cfg fe_cfg{};
    DevBuf   fe_state, fe_saved;    // its state, and the state in front of the current pass (what StreamRollback puts back)
    bool     fe_dirty = false;      // the current pass has advanced fe_state
};

// the diversity stream (wifirx_api_stream_div.inc): what its frames step keeps beside the StreamState, whose pass it shares
// with the single stream.  n_ant is the StreamState's plane count, and the st.* output rows are the combined set.
struct DivStream {
    uint32_t n_ant = 0;             // fixed by the handle's first wifirx_push_diversity; 0: none yet
    uint32_t cap = 0;               // triggers the per-antenna rows hold
    DevBuf   frames, car, csi, stats;   // n_ant sets of frame-kernel rows, set a at cap rows times a
    DevBuf   used, src;             // per trigger: the contributing antennas (the combiner's), the antenna of the csi / sym_stats rows
};

// A batch handed to the worker: `n` samples of format `fmt` (WIFIRX_IQ_*; `scale` widens the integer ones) at `ptr` (a ring
// buffer), and whether it ends with a flush
struct Job { const void* ptr; size_t n; bool flush; int fmt; float scale; };

// Host-buffer stream path (what a GNU Radio work() drives; wifirx_api_stream.inc): pushes are copied into one of two
// pinned staging buffers of one batch each; a full one is handed to the worker thread, which runs the device pipeline
// for it while the caller fills the other.  `mu` guards the job and retry slots, the frame queue, the statistics and the
// dead flag.
struct Worker {
    mutable std::mutex      mu;
    std::condition_variable cv;
    std::thread             thread;     // joinable while the worker runs
    bool    stop = false, busy = false;
    std::optional<Job> job;
    std::optional<Job> retry;           // the failed batch is still staged (its ring buffer untouched): the next push / flush re-submits it
    int     rc = 0;                     std::string err;     // first failure of a batch, reported by the next call
    std::string err_local;              // the worker's own error text (only the worker writes it; h->err belongs to the caller's thread)
    PinnedBuf ring[2];                  size_t ring_cap = 0, ring_fill = 0;   int ring_cur = 0;
    int     ring_fmt = WIFIRX_IQ_FC32;  float ring_scale = 1.0f;            // format of the samples staged in ring[ring_cur]
};

}  // namespace

// Members are released by their destructors: wifirx_destroy joins the worker and makes the device current first, and
// destroys the HIP stream after them.
struct wifirx_handle {
    wifirx_config cfg;
    Tunables      tune;
    Environment   env;
    int           device = 0;
    uint32_t      n_simd = 1024;    // SIMDs of the device (4 per CU): sizes the speculative trace-back's launch
    uint32_t      n_cu = 256;       // CUs of the device: sizes the grids of the format converters
    hipStream_t   stream = nullptr;
    std::string   err;
    wifirx_stats  stats{};
    Staging       stage;
    DecodeWork    dec;
    StreamState   st;
    DivStream     div;
    Worker        w;
};

namespace {

thread_local std::string g_err;
thread_local bool t_is_worker = false;      // set by the handle's stream worker thread

// h->err is written by the caller's thread only (one handle = calls serialised by the caller); the stream worker keeps
// its text in w.err_local until the caller's next push / flush takes it over (stream_worker_take_error).
int fail(wifirx_handle* h, int code, const std::string& msg)
{
    if (h) { if (t_is_worker) h->w.err_local = msg; else h->err = msg; }
    g_err = msg;
    return code;
}

#define HIP_TRY(h, expr)                                                                       \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return fail(h, WIFIRX_EHIP, std::string(#expr) + ": " + hipGetErrorString(e_));   \
    } while (0)

// A failed allocation: HIP keeps the last non-success code until it is read (hipGetLastError), and the launch wrappers of
// wr_kernels.hip / wr_decode.hip end in `return hipGetLastError()` -- a later launch that went fine would report this allocation's
// hipErrorOutOfMemory.  Every ENOMEM path reads it away.
int oom(wifirx_handle* h, const char* what, hipError_t e)
{
    (void)hipGetLastError();
    return fail(h, WIFIRX_ENOMEM, std::string(what) + ": " + hipGetErrorString(e));
}

// The environment overrides (tests, measurement); returns the stream priority WIFIRX_STREAM_PRIORITY asks for.
int read_environment(wifirx_handle* h)
{
    Environment& v = h->env;
    if (const char* e = std::getenv("WIFIRX_DECODE_SMALL_MAX")) h->tune.decode_small_max = (uint32_t)std::strtoul(e, nullptr, 10);   // tests pick the decode kernel with this
    if (const char* e = std::getenv("WIFIRX_DECODE_FPW")) v.decode_fpw = (uint32_t)std::strtoul(e, nullptr, 10);
    if (const char* e = std::getenv("WIFIRX_DECODE_Q")) v.decode_q = std::atoi(e) != 0;
    if (const char* e = std::getenv("WIFIRX_DECODE_OVL")) { const int m = std::atoi(e); if (m == 0 || m == 2) v.decode_ovl = m; }
    if (const char* e = std::getenv("WIFIRX_TEST_FAIL_ALLOC")) v.fail_alloc = std::atoi(e);
    if (const char* e = std::getenv("WIFIRX_TEST_FAIL_CARRY")) v.fail_carry = std::atoi(e);
    if (const char* e = std::getenv("WIFIRX_TEST_DECODE_BUDGET")) v.decode_budget = (size_t)std::strtoull(e, nullptr, 10);
    if (const char* e = std::getenv("WIFIRX_TEST_FAIL_DECODE_SCRATCH")) v.fail_decode_scratch = std::atoi(e);
    // WIFIRX_STREAM_PRIORITY = high | low (measurement: two handles whose kernels share the GPU, tools/coresident_probe.py)
    int prio = 0, prio_lo = 0, prio_hi = 0;
    if (const char* e = std::getenv("WIFIRX_STREAM_PRIORITY")) {
        if (hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi) == hipSuccess) prio = e[0] == 'h' ? prio_hi : e[0] == 'l' ? prio_lo : 0;
        else (void)hipGetLastError();
    }
    return prio;
}

wr::DemodParams params_of(const wifirx_handle* h)
{
    wr::DemodParams p;
    p.bandwidth = h->cfg.bandwidth;
    p.frequency = h->cfg.frequency;
    p.threshold = h->cfg.sensitivity;
    p.min_plateau = h->cfg.min_plateau;
    p.max_sym = h->cfg.max_sym;
    p.llr_bits = h->cfg.llr_bits;
    p.chan_est = h->cfg.chan_est;
    p.llr_csi = h->tune.llr_csi;
    return p;
}

}  // namespace

static void stream_worker_stop(wifirx_handle* h);
static void stream_worker_wait_idle(wifirx_handle* h);

extern "C" {

int wifirx_abi_version(void) { return WIFIRX_ABI_VERSION; }

const char* wifirx_last_error(const wifirx_handle* h) { return h ? h->err.c_str() : g_err.c_str(); }

int wifirx_create(const wifirx_config* cfg, wifirx_handle** out)
{
    if (!cfg || !out) return fail(nullptr, WIFIRX_EINVAL, "null argument");
    *out = nullptr;
    if (cfg->abi_version != WIFIRX_ABI_VERSION) return fail(nullptr, WIFIRX_EINVAL, "abi_version mismatch");
    if (cfg->max_sym == 0 || cfg->max_sym > WIFIRX_MAX_SYM) return fail(nullptr, WIFIRX_EINVAL, "max_sym out of range");
    if (!(cfg->llr_bits == 0 || cfg->llr_bits == 1 || cfg->llr_bits == 2 || cfg->llr_bits == 4 || cfg->llr_bits == 6))
        return fail(nullptr, WIFIRX_EINVAL, "llr_bits must be 0,1,2,4,6");
    if (cfg->chan_est < WIFIRX_EQ_LS || cfg->chan_est > WIFIRX_EQ_STA)
        return fail(nullptr, WIFIRX_EINVAL, "chan_est must be one of WIFIRX_EQ_LS, LMS, COMB, STA");
    if (!(cfg->bandwidth > 0) || !(cfg->frequency > 0)) return fail(nullptr, WIFIRX_EINVAL, "bandwidth/frequency must be > 0");
    if (cfg->min_plateau < 0 || cfg->min_plateau > 32) return fail(nullptr, WIFIRX_EINVAL, "min_plateau out of range");
    // the detect phase compares squares (NUMERICS.md rule 3): a negative threshold would act as its magnitude
    if (!(cfg->sensitivity >= 0)) return fail(nullptr, WIFIRX_EINVAL, "sensitivity must be >= 0");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(nullptr, WIFIRX_ENODEV, "no HIP device: libwifirx has no CPU fallback");
    if (cfg->device < 0 || cfg->device >= ndev) return fail(nullptr, WIFIRX_ENODEV, "device ordinal out of range");
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, cfg->device) != hipSuccess) return fail(nullptr, WIFIRX_ENODEV, "hipGetDeviceProperties failed");
    if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0)
        return fail(nullptr, WIFIRX_ENODEV, std::string("kernels are built for gfx950 only, device is ") + prop.gcnArchName);
    wifirx_handle* h = new (std::nothrow) wifirx_handle();
    if (!h) return fail(nullptr, WIFIRX_ENOMEM, "out of host memory");
    h->cfg = *cfg;
    h->device = cfg->device;
    h->n_simd = 4u * (uint32_t)prop.multiProcessorCount;
    h->n_cu = (uint32_t)prop.multiProcessorCount;
    const int prio = read_environment(h);
    if (hipSetDevice(h->device) != hipSuccess || hipStreamCreateWithPriority(&h->stream, hipStreamNonBlocking, prio) != hipSuccess) {
        delete h;
        return fail(nullptr, WIFIRX_EHIP, "hipStreamCreate failed");
    }
    *out = h;
    return WIFIRX_OK;
}

int wifirx_destroy(wifirx_handle* h)
{
    if (!h) return WIFIRX_EINVAL;
    stream_worker_stop(h);                  // the worker uses the buffers
    (void)hipSetDevice(h->device);          // the buffers free themselves on the handle's device
    hipStream_t stream = h->stream;
    if (stream) (void)hipStreamSynchronize(stream);
    delete h;
    if (stream) (void)hipStreamDestroy(stream);
    return WIFIRX_OK;
}

int wifirx_set_param(wifirx_handle* h, int id, double value)
{
    if (!h) return WIFIRX_EINVAL;
    if (!std::isfinite(value)) return fail(h, WIFIRX_EINVAL, "parameter value must be finite");
    stream_worker_wait_idle(h);            // a batch in flight keeps the parameters it started with
    switch (id) {
    case WIFIRX_P_BANDWIDTH:
        if (!(value > 0)) return fail(h, WIFIRX_EINVAL, "bandwidth must be > 0");
        h->cfg.bandwidth = value;
        return WIFIRX_OK;
    case WIFIRX_P_FREQUENCY:
        if (!(value > 0)) return fail(h, WIFIRX_EINVAL, "frequency must be > 0");
        h->cfg.frequency = value;
        return WIFIRX_OK;
    case WIFIRX_P_SENSITIVITY:
        if (!(value >= 0)) return fail(h, WIFIRX_EINVAL, "sensitivity must be >= 0");      // squared comparison, NUMERICS.md rule 3
        h->cfg.sensitivity = (float)value;
        return WIFIRX_OK;
    case WIFIRX_P_CHAN_EST:
        if (value < WIFIRX_EQ_LS || value > WIFIRX_EQ_STA || value != std::floor(value))
            return fail(h, WIFIRX_EINVAL, "chan_est must be one of WIFIRX_EQ_LS, LMS, COMB, STA");
        h->cfg.chan_est = (int)value;
        return WIFIRX_OK;
    case WIFIRX_P_LLR_CSI:
        h->tune.llr_csi = value != 0;
        return WIFIRX_OK;
    case WIFIRX_P_STREAM_IDX:
        h->tune.stream_want_idx = value != 0;
        return WIFIRX_OK;
    case WIFIRX_P_STREAM_SOFT:
        if (value != 0 && value != 1) return fail(h, WIFIRX_EINVAL, "WIFIRX_P_STREAM_SOFT must be 0 or 1");
        h->tune.stream_soft = (int32_t)value;
        return WIFIRX_OK;
    case WIFIRX_P_LLR_FORMAT:
        if (value != WIFIRX_LLR_F32 && value != WIFIRX_LLR_BF16)
            return fail(h, WIFIRX_EINVAL, "WIFIRX_P_LLR_FORMAT must be WIFIRX_LLR_F32 (0) or WIFIRX_LLR_BF16 (1)");
        h->tune.llr_format = (int32_t)value;
        return WIFIRX_OK;
    case WIFIRX_P_DECODE_SMALL_MAX:
        if (!(value >= 0) || value > 4e9) return fail(h, WIFIRX_EINVAL, "decode threshold out of range");
        h->tune.decode_small_max = (uint32_t)value;
        return WIFIRX_OK;
    case WIFIRX_P_STREAM_BATCH:
        // two pinned staging buffers of one batch each: at most 2^27 samples (1 GiB) per buffer
        if (!(value >= 0) || value > (double)WIFIRX_STREAM_BATCH_MAX) return fail(h, WIFIRX_EINVAL, "stream batch out of range (0 .. WIFIRX_STREAM_BATCH_MAX)");
        h->tune.stream_batch = (int64_t)value;
        return WIFIRX_OK;
    default:
        return fail(h, WIFIRX_EINVAL, "unknown parameter id");
    }
}

int wifirx_get_stats(const wifirx_handle* h, wifirx_stats* st)
{
    if (!h || !st) return WIFIRX_EINVAL;
    std::lock_guard<std::mutex> lk(h->w.mu);
    *st = h->stats;
    return WIFIRX_OK;
}

void* wifirx_stream(wifirx_handle* h) { return h ? (void*)h->stream : nullptr; }

int wifirx_sync(wifirx_handle* h)
{
    if (!h) return WIFIRX_EINVAL;
    stream_worker_wait_idle(h);
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return WIFIRX_OK;
}

int wifirx_dev_alloc(wifirx_handle* h, size_t bytes, void** out)
{
    if (!h || !out) return WIFIRX_EINVAL;
    HIP_TRY(h, hipSetDevice(h->device));
    hipError_t e = hipMalloc(out, bytes);
    if (e != hipSuccess) return oom(h, "hipMalloc", e);
    return WIFIRX_OK;
}

int wifirx_dev_free(wifirx_handle* h, void* p)
{
    if (!h) return WIFIRX_EINVAL;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipFree(p));
    return WIFIRX_OK;
}

int wifirx_memcpy_h2d(wifirx_handle* h, void* dst, const void* src, size_t bytes)
{
    if (!h) return WIFIRX_EINVAL;
    stream_worker_wait_idle(h);
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return WIFIRX_OK;
}

int wifirx_memcpy_d2h(wifirx_handle* h, void* dst, const void* src, size_t bytes)
{
    if (!h) return WIFIRX_EINVAL;
    stream_worker_wait_idle(h);
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return WIFIRX_OK;
}

// ---- batch mode -----------------------------------------------------------------------------

// bytes of one LLR value in the handle's batch format (WIFIRX_P_LLR_FORMAT)
static size_t llr_value_bytes(const wifirx_handle* h) { return h->tune.llr_format == WIFIRX_LLR_BF16 ? 2 : sizeof(float); }

// the demod launch of the handle's LLR format: the float32 and the bf16 rows are written by kernel instances of their own
static hipError_t launch_demod_batch_fmt(const wifirx_handle* h, const float2* iq, uint32_t slot_len, uint32_t n_slots,
                                         const wr::DemodParams* prm, const wr::DemodOut* out, const uint64_t* slot_off)
{
    if (h->tune.llr_format == WIFIRX_LLR_BF16) return wr_launch_demod_batch_bf16(h->stream, iq, slot_len, n_slots, prm, out, slot_off);
    return wr_launch_demod_batch(h->stream, iq, slot_len, n_slots, prm, out, slot_off);
}

static int check_batch(wifirx_handle* h, uint32_t slot_len, uint32_t n_slots, const wifirx_out* out)
{
    if (!h || !out) return WIFIRX_EINVAL;
    if (!out->frames) return fail(h, WIFIRX_EINVAL, "out->frames is required");
    if (slot_len == 0) return fail(h, WIFIRX_EINVAL, "slot_len must be > 0");
    if (slot_len > 0x7fffffffu) return fail(h, WIFIRX_ERANGE, "slot longer than 2^31 - 1 samples");
    if (h->cfg.max_batch && n_slots > h->cfg.max_batch) return fail(h, WIFIRX_ERANGE, "n_slots exceeds max_batch");
    if (h->cfg.max_slot_len && slot_len > h->cfg.max_slot_len) return fail(h, WIFIRX_ERANGE, "slot_len exceeds max_slot_len");
    if (out->llr && h->cfg.llr_bits == 0) return fail(h, WIFIRX_EINVAL, "llr requested but llr_bits == 0");
    if (out->on_device && (reinterpret_cast<uintptr_t>(out->hbits) & 15)) return fail(h, WIFIRX_EINVAL, "out->hbits must be 16-byte aligned");
    return WIFIRX_OK;
}

static int demod_batch_impl(wifirx_handle* h, const float* iq, int iq_on_device, uint32_t slot_len,
                            uint32_t n_slots, const wifirx_out* out, const uint64_t* slot_off_host);

int wifirx_demod_batch(wifirx_handle* h, const float* iq, int iq_on_device, uint32_t slot_len,
                       uint32_t n_slots, const wifirx_out* out)
{
    return demod_batch_impl(h, iq, iq_on_device, slot_len, n_slots, out, nullptr);
}

int wifirx_demod_batch_v(wifirx_handle* h, const float* iq, int iq_on_device, const uint64_t* slot_off,
                         uint32_t n_slots, const wifirx_out* out)
{
    if (!h) return WIFIRX_EINVAL;
    if (!slot_off) return fail(h, WIFIRX_EINVAL, "slot_off is null");
    uint64_t longest = 1;
    for (uint32_t k = 0; k < n_slots; k++) {
        if (slot_off[k + 1] < slot_off[k]) return fail(h, WIFIRX_EINVAL, "slot_off must not decrease");
        if (slot_off[k + 1] - slot_off[k] > 0x7fffffffu) return fail(h, WIFIRX_ERANGE, "slot longer than 2^31 - 1 samples");
        longest = std::max<uint64_t>(longest, slot_off[k + 1] - slot_off[k]);
    }
    return demod_batch_impl(h, iq, iq_on_device, (uint32_t)longest, n_slots, out, slot_off);
}

static int demod_batch_impl(wifirx_handle* h, const float* iq, int iq_on_device, uint32_t slot_len,
                            uint32_t n_slots, const wifirx_out* out, const uint64_t* slot_off_host)
{
    int rc = check_batch(h, slot_len, n_slots, out);
    if (rc) return rc;
    if (!iq) return fail(h, WIFIRX_EINVAL, "iq is null");
    if (n_slots == 0) return WIFIRX_OK;
    stream_worker_wait_idle(h);            // a stream batch in flight uses the handle's stream and workspaces
    HIP_TRY(h, hipSetDevice(h->device));
    const wr::DemodParams prm = params_of(h);
    const size_t n_iq = slot_off_host ? (size_t)(slot_off_host[n_slots] - slot_off_host[0]) + (size_t)slot_off_host[0]
                                      : (size_t)slot_len * n_slots;
    const uint64_t* d_off = nullptr;
    if (slot_off_host) {
        if ((rc = h->stage.off.reserve(h, ((size_t)n_slots + 1) * sizeof(uint64_t)))) return rc;
        HIP_TRY(h, hipMemcpyAsync(h->stage.off.p, slot_off_host, ((size_t)n_slots + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, h->stream));
        d_off = h->stage.off.as<const uint64_t>();
    }
    const size_t idx_n = (size_t)n_slots * h->cfg.max_sym * 48;
    const float2* d_iq = reinterpret_cast<const float2*>(iq);
    if (!iq_on_device) {
        if ((rc = h->stage.iq.reserve(h, n_iq * sizeof(float2)))) return rc;
        HIP_TRY(h, hipMemcpyAsync(h->stage.iq.p, iq, n_iq * sizeof(float2), hipMemcpyHostToDevice, h->stream));
        d_iq = h->stage.iq.as<const float2>();
    }
    // the outputs: the caller's buffer, the staging buffer that stands in for it when it is on the host, its bytes, and
    // whether that staging buffer is zero-filled first; `dev` is what the kernel writes
    struct Staged { void* user; DevBuf& stage; size_t bytes; bool zero; void* dev = nullptr; };
    Staged so[] = {
        { out->frames,    h->stage.frames, n_slots * sizeof(wifirx_frame), false },
        { out->idx,       h->stage.idx,    idx_n, true },
        { out->llr,       h->stage.llr,    idx_n * h->cfg.llr_bits * llr_value_bytes(h), true },
        { out->carrier,   h->stage.car,    idx_n * sizeof(float2), true },
        { out->csi,       h->stage.csi,    (size_t)n_slots * 52 * sizeof(float2), true },
        { out->sym_stats, h->stage.stats,  (size_t)n_slots * sizeof(float4), false },
        { out->hbits,     h->stage.hbits,  idx_n, true },
    };
    for (Staged& s : so) {
        s.dev = s.user;
        if (out->on_device || !s.user) continue;
        if ((rc = s.stage.reserve(h, s.bytes))) return rc;
        s.dev = s.stage.p;
        if (s.zero) HIP_TRY(h, hipMemsetAsync(s.dev, 0, s.bytes, h->stream));
    }
    const wr::DemodOut dout = { static_cast<wifirx_frame*>(so[0].dev), static_cast<uint8_t*>(so[1].dev), static_cast<float*>(so[2].dev),
                                static_cast<float2*>(so[3].dev), static_cast<float2*>(so[4].dev), static_cast<float4*>(so[5].dev),
                                static_cast<uint32_t*>(so[6].dev) };
    HIP_TRY(h, launch_demod_batch_fmt(h, d_iq, slot_len, n_slots, &prm, &dout, d_off));
    h->stats.samples_in += n_iq;
    if (!out->on_device) {
        for (const Staged& s : so)
            if (s.user) HIP_TRY(h, hipMemcpyAsync(s.user, s.dev, s.bytes, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        for (uint32_t i = 0; i < n_slots; i++) {
            uint32_t f = out->frames[i].flags;
            h->stats.frames_detected += (f & WIFIRX_F_DETECTED) != 0;
            h->stats.frames_signal_ok += (f & WIFIRX_F_SIGNAL) != 0;
            h->stats.frames_complete += (f & WIFIRX_F_COMPLETE) != 0;
        }
    }
    return WIFIRX_OK;
}

int wifirx_time_demod(wifirx_handle* h, const float* iq_dev, uint32_t slot_len, uint32_t n_slots,
                      const wifirx_out* out, int iters, float* ms_mean)
{
    int rc = check_batch(h, slot_len, n_slots, out);
    if (rc) return rc;
    if (!iq_dev || !ms_mean || iters <= 0 || !out->on_device) return fail(h, WIFIRX_EINVAL, "device buffers and iters > 0 required");
    stream_worker_wait_idle(h);
    HIP_TRY(h, hipSetDevice(h->device));
    const wr::DemodParams prm = params_of(h);
    struct Events {                       // destroyed on every exit
        hipEvent_t e0 = nullptr, e1 = nullptr;
        ~Events() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
    } ev;
    HIP_TRY(h, hipEventCreate(&ev.e0));
    HIP_TRY(h, hipEventCreate(&ev.e1));
    double total = 0;
    for (int i = 0; i < iters; i++) {
        HIP_TRY(h, hipEventRecord(ev.e0, h->stream));
        const wr::DemodOut dout = { out->frames, out->idx, out->llr, reinterpret_cast<float2*>(out->carrier),
                                    reinterpret_cast<float2*>(out->csi), reinterpret_cast<float4*>(out->sym_stats), out->hbits };
        HIP_TRY(h, launch_demod_batch_fmt(h, reinterpret_cast<const float2*>(iq_dev), slot_len, n_slots, &prm, &dout, nullptr));
        HIP_TRY(h, hipEventRecord(ev.e1, h->stream));
        HIP_TRY(h, hipEventSynchronize(ev.e1));
        float ms = 0;
        HIP_TRY(h, hipEventElapsedTime(&ms, ev.e0, ev.e1));
        total += ms;
    }
    *ms_mean = (float)(total / iters);
    return WIFIRX_OK;
}

int wifirx_synth_slots(wifirx_handle* h, const float* templates, int templates_on_device, uint32_t n_templates,
                       uint32_t frame_len, float* slots, uint32_t slot_len, uint32_t n_slots, uint32_t lead,
                       float snr_db, float cfo_max, uint64_t seed, float* cfo_out)
{
    if (!h || !templates || !slots) return WIFIRX_EINVAL;
    if (n_templates == 0 || frame_len == 0) return fail(h, WIFIRX_EINVAL, "empty templates");
    if (slot_len % 2) return fail(h, WIFIRX_EINVAL, "slot_len must be even");
    stream_worker_wait_idle(h);
    HIP_TRY(h, hipSetDevice(h->device));
    const float2* d_t = reinterpret_cast<const float2*>(templates);
    DevBuf tmp;                             // freed on return, after the synchronisation below
    if (!templates_on_device) {
        size_t bytes = (size_t)n_templates * frame_len * sizeof(float2);
        if (int rc = tmp.alloc(h, bytes, "hipMalloc(templates)")) return rc;
        hipError_t e = hipMemcpyAsync(tmp.p, templates, bytes, hipMemcpyHostToDevice, h->stream);
        if (e != hipSuccess) return fail(h, WIFIRX_EHIP, std::string("template upload: ") + hipGetErrorString(e));
        d_t = tmp.as<const float2>();
    }
    // snr_db = NaN: the noiseless channel (gain 1, no AWGN) -- what txgen.impair(snr_db=None) is on the host
    const bool noiseless = std::isnan(snr_db);
    float gain = noiseless ? 1.0f : std::sqrt(std::pow(10.0f, snr_db / 10.0f));
    hipError_t e = wr_launch_synth(h->stream, d_t, n_templates, frame_len, reinterpret_cast<float2*>(slots), slot_len,
                                   n_slots, lead, gain, noiseless ? 0.0f : 1.0f, cfo_max, seed, cfo_out);
    hipError_t e2 = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) return fail(h, WIFIRX_EHIP, std::string("synth launch: ") + hipGetErrorString(e));
    if (e2 != hipSuccess) return fail(h, WIFIRX_EHIP, std::string("synth sync: ") + hipGetErrorString(e2));
    return WIFIRX_OK;
}

}  // extern "C"

#include "wifirx_api_decode.inc"
#include "wifirx_api_ingest.inc"
#include "wifirx_api_frontend.inc"
#include "wifirx_api_stream.inc"
#include "wifirx_api_tx.inc"
#include "wifirx_api_channel.inc"
#include "wifirx_api_irs.inc"
#include "wifirx_api_link.inc"
#include "wifirx_api_convert.inc"
#include "wifirx_api_bank.inc"
#include "wifirx_api_arb.inc"
#include "wifirx_api_tune.inc"
#include "wifirx_api_spectrum.inc"
#include "wifirx_api_diversity.inc"
#include "wifirx_api_precombine.inc"
#include "wifirx_api_stream_div.inc"
