// Stream mode: what a GNU Radio block's work() drives.  The continuous input is kept in a device
// buffer; every push runs (1) the detection kernel over the new samples, (2) the sync_short
// state machine on the host over the 1-bit-per-sample plateau masks (a few bytes per tile),
// (3) the per-frame kernel + decode_mac for every trigger whose samples are present, and queues
// the finished frames for wifirx_poll.  Samples that a still-pending trigger needs, plus the
// detection history, are carried over to the next push.
// A stream is a stream of `planes` sample planes: one for wifirx_push / wifirx_push_iq, n_ant for the diversity stream
// (wifirx_api_stream_div.inc), whose pass is the same pass with a joint detection launch and a frames step of its own.

namespace {

const int64_t kHistory = 256;     // samples kept in front of the detection frontier (2 tiles + delay 16, rounded)

// What a push varies in a pass (stream_process): per plane the input pointer, the samples' format and scale and the side they
// are on, whether the pass ends the stream; for the diversity frames step the combining mode and the antennas' gains.
struct StreamCall { const void* const* iq; int fmt; float scale; int iq_on_device; bool flush; int mode; const float* ant_gain; };

// The sample planes: 1, or the antennas of a diversity stream; plane a at sbuf + a * sbuf_cap samples
uint32_t stream_planes(const wifirx_handle* h) { return h->div.n_ant ? h->div.n_ant : 1; }
float2* stream_plane(const wifirx_handle* h, uint32_t a) { return h->st.sbuf.as<float2>() + (size_t)a * (size_t)h->st.sbuf_cap; }

// Test hook for the allocation-failure paths (tests/test_gpu_stream.py): a handle created with
// WIFIRX_TEST_FAIL_ALLOC=<k> in the environment fails its k-th stream-mode allocation (counted from 1) once.
int stream_alloc(wifirx_handle* h, DevBuf& b, size_t bytes, const char* what)
{
    if (h->env.fail_alloc > 0 && ++h->env.alloc_count == h->env.fail_alloc) { b.reset(); return oom(h, what, hipErrorOutOfMemory); }
    return b.alloc(h, bytes, what);
}

// Grows the sample planes (one allocation) and the two detection side buffers together, to `need` samples a plane.  All
// three are allocated before anything of the handle changes: after a failure the old buffers and capacities are still in
// place and a later push starts over.
int stream_reserve(wifirx_handle* h, int64_t need)
{
    StreamState& s = h->st;
    if (need <= s.sbuf_cap) return WIFIRX_OK;
    const uint32_t planes = stream_planes(h);
    int64_t cap = std::max<int64_t>(need + need / 2, 1 << 16);
    cap = (cap + 63) / 64 * 64;
    DevBuf nb, n_above, n_A;
    const char* what = "hipMalloc(stream buffers)";
    int rc = stream_alloc(h, nb, (size_t)planes * (size_t)cap * sizeof(float2), what);
    if (!rc) rc = stream_alloc(h, n_above, (size_t)(cap / 64 + 2) * sizeof(uint64_t), what);
    if (!rc) rc = stream_alloc(h, n_A, (size_t)cap * sizeof(float2), what);
    if (rc) return rc;
    hipError_t e = hipSuccess;
    for (uint32_t a = 0; a < planes && e == hipSuccess && s.sbuf.p && s.sfill > 0; a++)      // the filled part, plane by plane to the new pitch
        e = hipMemcpyAsync(nb.as<float2>() + (size_t)a * (size_t)cap, stream_plane(h, a), (size_t)s.sfill * sizeof(float2),
                           hipMemcpyDeviceToDevice, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) return fail(h, WIFIRX_EHIP, std::string("stream buffer move: ") + hipGetErrorString(e));
    s.sbuf = std::move(nb);
    s.above = std::move(n_above);
    s.A = std::move(n_A);
    s.sbuf_cap = cap;
    return WIFIRX_OK;
}

// Host input in an integer format: room for a pass's samples as they come, every plane's chunk (grows like the sample buffer)
int stream_native_reserve(wifirx_handle* h, size_t need)
{
    if (h->st.native.bytes >= need) return WIFIRX_OK;
    return stream_alloc(h, h->st.native, need + need / 2, "hipMalloc(stream native samples)");
}

// Output rows of the frame kernel + decode_mac for up to `n` triggers.  The capacity is zero while the buffers are
// being replaced, so a failed allocation leaves "no buffers, capacity 0" and the next push allocates again.
int stream_out_reserve(wifirx_handle* h, uint32_t n)
{
    StreamState& s = h->st;
    if (n <= s.out_cap) return WIFIRX_OK;
    uint32_t cap = std::max<uint32_t>(n * 2, 64);
    const size_t per = (size_t)h->cfg.max_sym * 48;
    // no LLR rows here: wifirx_poll has no LLR output; with WIFIRX_P_STREAM_SOFT the decoder's rows come from stream_llr_reserve
    struct { DevBuf& b; size_t bytes; } req[] = {
        { s.trig, cap * sizeof(wr::StreamTrig) },
        { s.frames, cap * sizeof(wifirx_frame) },
        { s.idx, cap * per },
        { s.car, h->cfg.want_carrier ? cap * per * sizeof(float2) : 0 },
        { s.psdu, (size_t)cap * 2048 },
        { s.csi, (size_t)cap * 52 * sizeof(float2) },
        { s.stats, (size_t)cap * sizeof(float4) },
        { s.hbits, cap * per },                 // the decisions as bit planes: what decode_mac reads
    };
    s.out_cap = 0;
    for (auto& r : req) r.b.reset();
    for (auto& r : req) {
        if (!r.bytes) continue;
        if (int rc = stream_alloc(h, r.b, r.bytes, "hipMalloc(stream outputs)")) {
            for (auto& q : req) q.b.reset();
            return rc;
        }
    }
    s.out_cap = cap;
    return WIFIRX_OK;
}

// WIFIRX_P_STREAM_SOFT: LLR rows for the out_cap triggers the other rows hold (max_sym * 48 * 6 floats each), kept while
// the handle lives; allocated only once the mode is on
static int stream_llr_reserve(wifirx_handle* h)
{
    const size_t need = (size_t)h->st.out_cap * h->cfg.max_sym * 48 * 6 * sizeof(float);
    if (h->st.llr.bytes >= need) return WIFIRX_OK;
    return stream_alloc(h, h->st.llr, need, "hipMalloc(stream LLR rows)");
}

// The stream's per-frame outputs, in the order of StreamBatch and wifirx_poll_out: the device rows of out_cap triggers,
// the bytes of a row (a caller's row is as long; psdu: psdu_stride), whether this handle produces the output, whether it
// is zero-filled before the frame kernel, and the bytes of a frame's row worth bringing back (null: the whole row).
struct StreamOut {
    const DevBuf* dev; size_t pitch; bool produced, zero; size_t (*filled)(const wifirx_frame&);
    size_t bytes(const wifirx_frame& f) const { return filled ? filled(f) : pitch; }
};

std::array<StreamOut, SO_N> stream_outs(const wifirx_handle* h)
{
    const StreamState& s = h->st;
    const size_t per = (size_t)h->cfg.max_sym * 48;
    return {{
        { &s.psdu, 2048, true, false, [](const wifirx_frame& f) { return (f.flags & WIFIRX_F_DECODED) ? std::min<size_t>(f.psdu_len, 2048) : 0; } },
        { &s.idx, per, h->tune.stream_want_idx != 0, true, [](const wifirx_frame& f) { return (size_t)f.n_sym_out * 48; } },
        { &s.car, per * sizeof(float2), h->cfg.want_carrier != 0, true, [](const wifirx_frame& f) { return f.n_sym_out * 48 * sizeof(float2); } },
        { &s.csi, 52 * sizeof(float2), true, true, nullptr },
        { &s.stats, sizeof(float4), true, false, nullptr },
    }};
}

// What a pass of the stream pipeline changes before its results are queued; put back when the pass fails, so that a
// failed push has consumed nothing (include/wifirx.h, WIFIRX_P_STREAM_BATCH: ERRORS) and can simply be repeated.
struct StreamRollback {
    wifirx_handle* h;
    bool     armed = true;
    int64_t  sfill, sprocessed, sdetected, last_trig;
    size_t   n_pending;
    uint64_t samples_in, frames_detected;
    explicit StreamRollback(wifirx_handle* hh) : h(hh), sfill(hh->st.sfill), sprocessed(hh->st.sprocessed), sdetected(hh->st.sdetected),
        last_trig(hh->st.last_trig), n_pending(hh->st.pending.size())
    {
        h->st.fe_dirty = false;
        std::lock_guard<std::mutex> lk(h->w.mu);
        samples_in = h->stats.samples_in;
        frames_detected = h->stats.frames_detected;
    }
    ~StreamRollback()
    {
        if (!armed) return;
        h->st.sfill = sfill; h->st.sprocessed = sprocessed; h->st.sdetected = sdetected; h->st.last_trig = last_trig;
        h->st.pending.resize(n_pending);
        // the front end's state as it was in front of the pass (stream_frontend_run saved it), behind whatever the pass queued.
        // Should this copy itself fail, the state no longer matches the samples the caller repeats: the stream is dead.
        if (h->st.fe_dirty && (hipMemcpyAsync(h->st.fe_state.p, h->st.fe_saved.p, sizeof(wifirx_frontend_state), hipMemcpyDeviceToDevice,
                                              h->stream) != hipSuccess || hipStreamSynchronize(h->stream) != hipSuccess)) {
            (void)hipGetLastError();
            std::lock_guard<std::mutex> lk(h->w.mu);
            h->st.dead = true;
            h->st.dead_msg = "the stream's front-end state could not be restored after a failed pass (destroy the handle)";
        }
        h->st.fe_dirty = false;
        std::lock_guard<std::mutex> lk(h->w.mu);
        h->stats.samples_in = samples_in;
        h->stats.frames_detected = frames_detected;
    }
};

// WIFIRX_TRACE: stage times of every push on stderr
struct StageClock {
    std::chrono::steady_clock::time_point t_prev = std::chrono::steady_clock::now();
    void operator()(const char* what)
    {
        static const bool trace = std::getenv("WIFIRX_TRACE") != nullptr;
        if (!trace) return;
        auto t = std::chrono::steady_clock::now();
        std::fprintf(stderr, "[wifirx_push] %-28s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(t - t_prev).count());
        t_prev = t;
    }
};

// What the frames phase hands to the queue step: per pending trigger its record and whether no more samples can come
// (a diversity pass, wifirx_api_stream_div.inc, adds: hold[k] = an antenna's record of trigger k still waits for samples;
// per frame the contributing antennas and the n_ant antennas' own records, which travel with the batch)
struct FramePass {
    std::vector<wifirx_frame> fr; std::vector<char> final_; std::shared_ptr<const StreamBatch> batch;
    std::vector<char> hold; std::vector<uint8_t> used; std::vector<wifirx_frame> ant; uint32_t n_ant = 0;
};

}  // namespace

// The sync_short state machine over the plateau masks of the tiles from t_first on (the first one is mask history when
// t_first > 0): appends to st.pending and moves the detection frontier to the end of the buffer.  A trigger needs
// min_plateau+1 samples above the threshold in a row and > MIN_GAP since the last.  Shared by the single stream and the
// diversity stream, whose masks come from the joint detection.
static void stream_select_triggers(wifirx_handle* h, const std::vector<uint64_t>& masks, int64_t t_first, StageClock& stage)
{
    StreamState& st = h->st;
    const int64_t end_abs = st.sbase + st.sfill, n_tiles = (int64_t)masks.size();
    uint64_t n_new_trig = 0;
    for (int64_t tl = 0; tl < n_tiles; tl++) {
        uint64_t m = masks[(size_t)tl], prev = tl > 0 ? masks[(size_t)tl - 1] : 0;
        if (!m) continue;               // no sample of the tile above the threshold: no plateau can end in it (most tiles: 0.17 -> 0.03 ms per 4 M samples)
        uint64_t hit = m;
        for (int j = 1; j <= h->cfg.min_plateau; j++) hit &= (m << j) | (j < 64 ? (prev >> (64 - j)) : 0);
        const int64_t tile_abs = st.sbase + (t_first + tl) * 64;
        while (hit) {
            int l = __builtin_ctzll(hit);
            hit &= hit - 1;
            int64_t pos = tile_abs + l;
            if (pos < st.sdetected || pos >= end_abs) continue;
            if (pos - st.last_trig <= WIFIRX_MIN_GAP) continue;
            st.pending.push_back({ pos, 0.0f, false });
            st.last_trig = pos;
            n_new_trig++;
        }
    }
    st.sdetected = end_abs;
    { std::lock_guard<std::mutex> lk(h->w.mu); h->stats.frames_detected += n_new_trig; }
    stage("host state machine");
}

// Detect: (1) detection over the tiles with not yet scanned samples (plus one tile of mask history) -- of a diversity stream
// the joint detection over its planes (NUMERICS.md rule 24), whatever n_ant; (2) the sync_short state machine
// (stream_select_triggers) appends to st.pending
static int stream_detect(wifirx_handle* h, StageClock& stage)
{
    StreamState& st = h->st;
    const int64_t end_abs = st.sbase + st.sfill;
    if (end_abs <= st.sdetected) return WIFIRX_OK;
    int64_t t_first = (st.sdetected - st.sbase) / 64;
    if (t_first > 0) t_first -= 1;
    const int64_t n_tiles = (st.sfill + 63) / 64 - t_first;
    if (h->div.n_ant) {
        wr::DetectMultiArgs args{};
        for (uint32_t a = 0; a < h->div.n_ant; a++) args.x[a] = stream_plane(h, a);
        args.n_samp = st.sfill;
        args.tile0 = t_first;
        args.n_tiles = n_tiles;
        args.thr = h->cfg.sensitivity;
        args.n_ant = h->div.n_ant;
        args.masks = st.above.as<uint64_t>();
        args.A = st.A.as<float2>();
        HIP_TRY(h, wr_launch_stream_detect_multi(h->stream, &args));
    } else {
        HIP_TRY(h, wr_launch_stream_detect(h->stream, st.sbuf.as<float2>(), st.sfill, t_first, n_tiles, h->cfg.sensitivity,
                                           st.above.as<uint64_t>(), st.A.as<float2>()));
    }
    std::vector<uint64_t> masks((size_t)n_tiles);
    HIP_TRY(h, hipMemcpyAsync(masks.data(), st.above.as<uint64_t>() + t_first,
                              (size_t)n_tiles * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    stage("input copy + detect + masks");
    stream_select_triggers(h, masks, t_first, stage);
    return WIFIRX_OK;
}

// The triggers of a pass as the frame kernel takes them: position in the buffer, the samples that belong to the trigger, the
// coarse CFO of an earlier pass; p.final_[k] = no more samples can come for trigger k (next trigger / MAX_SAMPLES / flush)
static std::vector<wr::StreamTrig> stream_trig_rows(wifirx_handle* h, bool flush, FramePass& p)
{
    StreamState& st = h->st;
    const uint32_t np = (uint32_t)st.pending.size();
    const int64_t end_abs = st.sbase + st.sfill;
    std::vector<wr::StreamTrig> trig(np);
    for (uint32_t k = 0; k < np; k++) {
        const int64_t pos = st.pending[k].pos;
        int64_t L = end_abs - (pos - 16);
        bool fin = flush;
        if (k + 1 < np && st.pending[k + 1].pos - pos <= L) { L = st.pending[k + 1].pos - pos; fin = true; }
        if (L >= WIFIRX_MAX_SAMPLES) { L = WIFIRX_MAX_SAMPLES; fin = true; }
        // 383 samples are enough for the LTS search only when the 384th cannot come: it takes part in stage 1's exponent
        // maximum (NUMERICS.md rule 6), so a search without it could give a record that depends on where a push ends.
        // One sample fewer and the frame waits (DETECTED | TRUNCATED) like any other whose window is still on its way.
        if (!fin && L == WIFIRX_SYNC_LENGTH + 63) L -= 1;
        trig[k].pos = pos - st.sbase;
        trig[k].usable = L;
        trig[k].cfo = st.pending[k].cfo;        // A[] of an earlier push is gone: reuse the value
        trig[k].pad = st.pending[k].have_cfo;   // the device computed when it first saw the trigger
        p.final_.push_back(fin);
    }
    return trig;
}

// The outputs of a pass to the host, p.fr (the records, already here) saying how much of every output row (max_sym symbols,
// 2048 bytes) is worth bringing back.  Each output's rows are cut to the batch's widest filled row and packed on the device,
// then leave in one piece for a pinned host buffer: a 2-D copy to pageable memory goes row by row and costs milliseconds.
static int stream_pack_outputs(wifirx_handle* h, const std::array<StreamOut, SO_N>& outs, StageClock& stage, FramePass& p)
{
    StreamState& st = h->st;
    const uint32_t np = (uint32_t)p.fr.size();
    int rc;
    auto b = std::make_shared<StreamBatch>();
    size_t total = 0;
    for (int i = 0; i < SO_N; i++) {         // (widths start at 0: make_shared value-initialises)
        for (uint32_t k = 0; outs[i].produced && k < np; k++) b->width[i] = std::max(b->width[i], outs[i].bytes(p.fr[k]));
        b->off[i] = total;
        total += (np * b->width[i] + 15) / 16 * 16;
    }
    if ((rc = st.pack.reserve(h, total)) || (rc = st.host.reserve(h, total))) return rc;
    for (int i = 0; i < SO_N; i++) {
        const size_t w = b->width[i];
        uint8_t* dst = st.pack.as<uint8_t>() + b->off[i];
        if (w && outs[i].filled) HIP_TRY(h, hipMemcpy2DAsync(dst, w, outs[i].dev->p, outs[i].pitch, w, np, hipMemcpyDeviceToDevice, h->stream));
        else if (w) HIP_TRY(h, hipMemcpyAsync(dst, outs[i].dev->p, np * w, hipMemcpyDeviceToDevice, h->stream));     // fixed rows: packed already
    }
    HIP_TRY(h, hipMemcpyAsync(st.host.p, st.pack.p, total, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    stage("outputs to host");
    b->blob.assign(st.host.as<const uint8_t>(), st.host.as<const uint8_t>() + total);     // shared by the batch's frames
    b->n_ant = p.n_ant;
    b->used = std::move(p.used);
    b->ant = std::move(p.ant);
    p.batch = std::move(b);
    return WIFIRX_OK;
}

// What both frames steps begin with (stream_frames_begin): the pending triggers, WIFIRX_P_STREAM_SOFT, the frame kernel's
// parameters, the table of outputs, the decoder's LLR rows (null: hard decisions); the rows the trigger upload reads, which
// live until the step has waited for the stream
struct FramesBegin {
    uint32_t np = 0; bool soft = false; wr::DemodParams prm{}; std::array<StreamOut, SO_N> outs{}; float* d_llr = nullptr;
    std::vector<wr::StreamTrig> trig;
};

// The prologue of a frames step: the output rows (`out_reserve`: the stream's, or with the antennas' behind them) and the LLR rows
// for the pending triggers, the triggers to the device, zeros in the produced outputs that want them.  np = 0: nothing to do.
static int stream_frames_begin(wifirx_handle* h, int (*out_reserve)(wifirx_handle*, uint32_t), bool flush, FramePass& p, FramesBegin& f)
{
    StreamState& st = h->st;
    f.np = (uint32_t)st.pending.size();
    if (!f.np) return WIFIRX_OK;
    int rc;
    if ((rc = out_reserve(h, f.np))) return rc;
    f.soft = h->tune.stream_soft != 0;
    if (f.soft && (rc = stream_llr_reserve(h))) return rc;
    f.trig = stream_trig_rows(h, flush, p);
    f.prm = params_of(h);
    if (f.soft) f.prm.llr_bits = 6;             // the stream's own LLR rows: every rate fits, whatever cfg.llr_bits says
    HIP_TRY(h, hipMemcpyAsync(st.trig.p, f.trig.data(), f.np * sizeof(wr::StreamTrig), hipMemcpyHostToDevice, h->stream));
    f.outs = stream_outs(h);
    for (const StreamOut& so : f.outs)
        if (so.produced && so.zero) HIP_TRY(h, hipMemsetAsync(so.dev->p, 0, f.np * so.pitch, h->stream));
    f.d_llr = f.soft ? st.llr.as<float>() : nullptr;
    return WIFIRX_OK;
}

// Frames: (3) the frame kernel + decode_mac over every pending trigger whose samples are (partly) here; records, outputs
static int stream_frames(wifirx_handle* h, bool flush, StageClock& stage, FramePass& p)
{
    StreamState& st = h->st;
    FramesBegin f;
    int rc = stream_frames_begin(h, stream_out_reserve, flush, p, f);
    if (rc || !f.np) return rc;
    const uint32_t np = f.np;
    // hard decisions as bytes only when the caller polls them (WIFIRX_P_STREAM_IDX); decode_mac reads the bit planes
    uint8_t* d_idx = f.outs[SO_IDX].produced ? st.idx.as<uint8_t>() : nullptr;
    const wr::DemodOut dout = { st.frames.as<wifirx_frame>(), d_idx, f.d_llr, st.car.as<float2>(), st.csi.as<float2>(),
                                st.stats.as<float4>(), st.hbits.as<uint32_t>() };
    HIP_TRY(h, wr_launch_demod_stream(h->stream, st.sbuf.as<float2>(), st.sfill, st.trig.as<wr::StreamTrig>(), np,
                                      &f.prm, st.A.as<float2>(), &dout));
    const wifirx_out o = { st.frames.as<wifirx_frame>(), d_idx, f.d_llr, nullptr, st.psdu.as<uint8_t>(), 2048, 1,
                           nullptr, nullptr, st.hbits.as<uint32_t>() };
    stage("enqueue frame kernel");
    if ((rc = f.soft ? decode_batch_soft_impl(h, np, &o, 6, false) : decode_batch_impl(h, np, &o))) return rc;
    stage("frame kernel + decode_mac");
    // the frame records first: they say how much of every output row is worth bringing back (stream_pack_outputs)
    p.fr.resize(np);
    HIP_TRY(h, hipMemcpyAsync(p.fr.data(), st.frames.p, np * sizeof(wifirx_frame), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return stream_pack_outputs(h, f.outs, stage, p);
}

// Queue: the settled frames go to wifirx_poll, the others stay pending with the coarse CFO the device found (cannot fail)
static void stream_queue(wifirx_handle* h, const FramePass& p, StageClock& stage)
{
    StreamState& st = h->st;
    if (p.fr.empty()) return;
    std::vector<PendingTrig> keep;
    std::lock_guard<std::mutex> lk(h->w.mu);            // queue + statistics
    for (uint32_t k = 0; k < p.fr.size(); k++) {
        wifirx_frame f = p.fr[k];
        const bool complete = (f.flags & WIFIRX_F_COMPLETE) != 0;
        const bool truncated = (f.flags & WIFIRX_F_TRUNCATED) != 0;
        // a frame is settled when it is complete, when it failed for a reason more samples cannot
        // cure, or when no more samples can come (next trigger / MAX_SAMPLES / flush)
        // (a diversity pass: when every antenna's record is complete or failed so -- p.hold)
        const bool waits = p.hold.empty() ? !(complete || !truncated) : p.hold[k] != 0;
        if (waits && !p.final_[k]) {
            keep.push_back({ st.pending[k].pos, f.cfo_coarse, true });
            continue;
        }
        f.trigger = (int32_t)(st.pending[k].pos & 0x7fffffff);
        h->stats.frames_signal_ok += (f.flags & WIFIRX_F_SIGNAL) != 0;
        h->stats.frames_complete += complete;
        h->stats.frames_crc_ok += (f.flags & WIFIRX_F_CRC_OK) != 0;
        h->stats.frames_dropped += (f.flags & WIFIRX_F_CRC_OK) == 0;
        st.queue.push_back(PolledFrame{ f, p.batch, k });
    }
    st.n_queued.store((uint32_t)st.queue.size(), std::memory_order_release);
    st.pending.swap(keep);
    stage("queue frames");
}

// Carry: (4) samples a pending trigger still needs + the detection history, in every plane.  It runs behind the commit
// (frames queued, fill and frontier advanced) and reports no error, which every caller reads as "nothing was consumed, hand
// the samples in again" -- that would double them (include/wifirx.h, WIFIRX_P_STREAM_BATCH: ERRORS).  A failure before a
// plane has been touched leaves base and fill as they are (the next pass moves them); one after the move began leaves
// planes that cannot be trusted: the stream is marked dead and every later push says so (WIFIRX_EDEAD, never "retry").
static void stream_carry(wifirx_handle* h, StageClock& stage)
{
    StreamState& st = h->st;
    int64_t keep_from = st.sdetected - kHistory;
    if (!st.pending.empty()) keep_from = std::min(keep_from, st.pending.front().pos - 16);
    if (keep_from < st.sbase) keep_from = st.sbase;
    keep_from = keep_from / 64 * 64;
    if (keep_from > st.sbase) {
        const int64_t off = keep_from - st.sbase, left = st.sfill - off;
        hipError_t ce = hipSuccess;
        bool touched = false;
        // test hook (tests/test_gpu_stream.py): WIFIRX_TEST_FAIL_CARRY=<k> fails the k-th carry before / =-<k> after the move began
        if (h->env.fail_carry != 0 && ++h->env.carry_count == std::abs(h->env.fail_carry)) {
            ce = hipErrorUnknown;
            touched = h->env.fail_carry < 0;
        }
        for (uint32_t a = 0; a < stream_planes(h) && ce == hipSuccess && left > 0; a++) {
            // overlapping move: stage through the A buffer (a plane's capacity, free between pushes)
            ce = hipMemcpyAsync(st.A.p, stream_plane(h, a) + off, (size_t)left * sizeof(float2), hipMemcpyDeviceToDevice, h->stream);
            if (ce == hipSuccess) {
                touched = true;
                ce = hipMemcpyAsync(stream_plane(h, a), st.A.p, (size_t)left * sizeof(float2), hipMemcpyDeviceToDevice, h->stream);
            }
        }
        if (ce == hipSuccess) ce = hipStreamSynchronize(h->stream);
        if (ce == hipSuccess) {
            st.sbase = keep_from;
            st.sfill = left > 0 ? left : 0;
        } else if (touched) {
            std::lock_guard<std::mutex> lk(h->w.mu);
            st.dead = true;
            st.dead_msg = std::string("stream sample buffer lost in the carry step: ") + hipGetErrorString(ce) +
                          " (frames up to here were delivered; destroy the handle)";
        } else {
            (void)hipGetLastError();        // nothing was moved: the next pass carries from the same base
        }
    }
    stage("carry");
}

// Ingest: `n` more samples of format c.fmt into every plane at sfill.  Integer samples (NUMERICS.md rule 20) are widened into
// the plane by a launch: from the caller's device buffer, or from the plane's chunk of the native scratch (at a * pitch +
// native_off), which host samples cross the bus into as they come.  With the front end on (rule 32; wifirx_push_diversity
// refuses it: one plane) it takes the place of the widening, or runs in place on the float pairs.
static int stream_ingest(wifirx_handle* h, const StreamCall& c, size_t n, size_t native_off, size_t pitch)
{
    StreamState& st = h->st;
    const uint32_t bps = wr_iq_sample_bytes(c.fmt);     // 0: float pairs
    int rc;
    for (uint32_t a = 0; n && a < stream_planes(h); a++) {
        float2* const d_new = stream_plane(h, a) + st.sfill;
        if (bps) {
            const void* d_native = c.iq[a];
            if (!c.iq_on_device) {
                uint8_t* const chunk = st.native.as<uint8_t>() + a * pitch + native_off;
                HIP_TRY(h, hipMemcpyAsync(chunk, c.iq[a], n * bps, hipMemcpyHostToDevice, h->stream));
                d_native = chunk;
            }
            if (st.fe_on) { if ((rc = stream_frontend_run(h, d_native, c.fmt, c.scale, n, d_new))) return rc; }
            else HIP_TRY(h, wr_launch_iq_widen(h->stream, d_native, c.fmt, n, c.scale, d_new, h->n_cu));
        } else {
            HIP_TRY(h, hipMemcpyAsync(d_new, c.iq[a], n * sizeof(float2), c.iq_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, h->stream));
            if (st.fe_on && (rc = stream_frontend_run(h, d_new, WIFIRX_IQ_FC32, 1.0f, n, d_new))) return rc;
        }
    }
    if (n) {
        st.sfill += (int64_t)n;
        { std::lock_guard<std::mutex> lk(h->w.mu); h->stats.samples_in += n; }
    }
    return WIFIRX_OK;
}

static int div_frames(wifirx_handle* h, const StreamCall& c, StageClock& stage, FramePass& p);      // wifirx_api_stream_div.inc

// One pass of the stream pipeline over `n` more samples of every plane (what every push was before the staging ring existed):
// ingest, detect, frames (the diversity stream's own step for its kind), queue, carry.
// All or nothing: on an error return the handle's stream state is what it was before the call.
static int stream_process(wifirx_handle* h, const StreamCall& c, size_t n)
{
    StageClock stage;
    StreamState& st = h->st;
    { std::lock_guard<std::mutex> lk(h->w.mu); if (st.dead) return fail(h, WIFIRX_EDEAD, st.dead_msg); }   // (repeating will not help)
    HIP_TRY(h, hipSetDevice(h->device));
    int rc = stream_reserve(h, st.sfill + (int64_t)n + 64);
    if (rc) return rc;
    const uint32_t bps = wr_iq_sample_bytes(c.fmt);
    // a plane's scratch copy starts where its first whole 16-byte piece, behind the widen kernel's head sample, is 16-byte aligned
    const size_t native_off = bps ? (16 - (size_t)(st.sfill & 1) * bps) & 15 : 0;
    const size_t pitch = (native_off + n * bps + 63) / 64 * 64;
    if (n && bps && !c.iq_on_device && (rc = stream_native_reserve(h, (stream_planes(h) - 1) * pitch + native_off + n * bps))) return rc;
    if ((rc = stream_frontend_reserve(h, n))) return rc;
    StreamRollback undo(h);
    if ((rc = stream_ingest(h, c, n, native_off, pitch))) return rc;
    stage("reserve + enqueue input copy");
    const bool run = c.flush || h->tune.stream_batch <= 0 || st.sbase + st.sfill - st.sprocessed >= h->tune.stream_batch;
    if (!run) HIP_TRY(h, hipStreamSynchronize(h->stream));     // keep collecting (WIFIRX_P_STREAM_BATCH); the caller may reuse its buffers
    else st.sprocessed = st.sbase + st.sfill;
    FramePass pass;
    if (run && (rc = stream_detect(h, stage))) return rc;
    if (run && (rc = h->div.n_ant ? div_frames(h, c, stage, pass) : stream_frames(h, c.flush, stage, pass))) return rc;
    undo.armed = false;                 // the commit: the samples are consumed and the frames queued below; nothing after it fails
    if (run) {
        stream_queue(h, pass, stage);
        stream_carry(h, stage);
    }
    return WIFIRX_OK;
}

// ---- the worker thread of the host-buffer path ------------------------------------------------------------------
static void stream_worker_main(wifirx_handle* h)
{
    t_is_worker = true;
    Worker& w = h->w;
    std::unique_lock<std::mutex> lk(w.mu);
    for (;;) {
        w.cv.wait(lk, [&] { return w.job || w.stop; });
        if (!w.job) return;                                 // stop requested, nothing queued
        const Job job = *w.job;
        w.job.reset();
        lk.unlock();
        int rc;
        try {
            rc = stream_process(h, StreamCall{ &job.ptr, job.fmt, job.scale, 0, job.flush, 0, nullptr }, job.n);
        } catch (const std::exception& e) {          // nothing may escape a thread (or the C boundary)
            rc = WIFIRX_ENOMEM;
            w.err_local = std::string("stream worker: ") + e.what();
        }
        lk.lock();
        if (rc != WIFIRX_OK) {
            if (w.rc == WIFIRX_OK) { w.rc = rc; w.err = w.err_local; }
            // stream_process is all or nothing: the batch is still whole in its staging buffer (the caller fills the other
            // one and cannot hand that over before this one is settled) -- keep it for another attempt
            w.retry = job;
        }
        w.busy = false;
        w.cv.notify_all();
    }
}

static void stream_worker_wait_idle(wifirx_handle* h)
{
    if (!h->w.thread.joinable()) return;
    std::unique_lock<std::mutex> lk(h->w.mu);
    h->w.cv.wait(lk, [&] { return !h->w.busy; });
}

static void stream_worker_stop(wifirx_handle* h)
{
    Worker& w = h->w;
    if (!w.thread.joinable()) return;
    {
        std::unique_lock<std::mutex> lk(w.mu);
        w.cv.wait(lk, [&] { return !w.busy; });
        w.stop = true;
        w.cv.notify_all();
    }
    w.thread.join();
}

// the failure of an earlier batch, if any (reported once, by the next push / flush)
static int stream_worker_take_error(wifirx_handle* h)
{
    std::lock_guard<std::mutex> lk(h->w.mu);
    const int rc = h->w.rc;
    if (rc != WIFIRX_OK) { h->err = h->w.err; h->w.rc = WIFIRX_OK; }
    return rc;
}

// A batch that failed on the worker is submitted again (same buffer, same samples) and waited for: it must be through
// before anything behind it in the stream.  Returns its result.
static int stream_resubmit_failed(wifirx_handle* h)
{
    Worker& w = h->w;
    {
        std::unique_lock<std::mutex> lk(w.mu);
        if (!w.retry) return WIFIRX_OK;                     // the usual case: no wait -- the worker may be busy with a good batch
        w.cv.wait(lk, [&] { return !w.busy; });            // (a failed batch leaves the worker idle)
        w.job = w.retry;
        w.retry.reset();
        w.busy = true;
        w.cv.notify_all();
    }
    stream_worker_wait_idle(h);
    return stream_worker_take_error(h);
}

// hand the current staging buffer to the worker (waits until the previous batch has left the device pipeline)
static int stream_submit(wifirx_handle* h, bool flush)
{
    Worker& w = h->w;
    {
        std::unique_lock<std::mutex> lk(w.mu);
        w.cv.wait(lk, [&] { return !w.busy; });
        w.job = Job{ w.ring[w.ring_cur].p, w.ring_fill, flush, w.ring_fmt, w.ring_scale };
        w.busy = true;
        w.cv.notify_all();
    }
    w.ring_cur ^= 1;
    w.ring_fill = 0;
    return WIFIRX_OK;
}

// Copy of a work() chunk into the pinned staging buffer with streaming (non-temporal) stores: the buffer is written
// once and then read by the DMA engine only, so the lines need neither be fetched for ownership nor stay in the caches
// of the core that runs the scheduler thread.  Whole 64-byte lines at a time; the fence orders the stores before the
// hand-over to the worker thread.
static void stage_copy(void* dst_, const void* src_, size_t bytes)
{
    uint8_t* dst = static_cast<uint8_t*>(dst_);
    const uint8_t* src = static_cast<const uint8_t*>(src_);
    if (bytes < 256) { std::memcpy(dst, src, bytes); return; }
    const size_t head = (64 - (reinterpret_cast<uintptr_t>(dst) & 63)) & 63;
    if (head) { std::memcpy(dst, src, head); dst += head; src += head; bytes -= head; }
    const size_t lines = bytes / 64;
    for (size_t i = 0; i < lines; i++) {
        const __m128i a = _mm_loadu_si128(reinterpret_cast<const __m128i*>(src) + 0);
        const __m128i b = _mm_loadu_si128(reinterpret_cast<const __m128i*>(src) + 1);
        const __m128i c = _mm_loadu_si128(reinterpret_cast<const __m128i*>(src) + 2);
        const __m128i d = _mm_loadu_si128(reinterpret_cast<const __m128i*>(src) + 3);
        _mm_stream_si128(reinterpret_cast<__m128i*>(dst) + 0, a);
        _mm_stream_si128(reinterpret_cast<__m128i*>(dst) + 1, b);
        _mm_stream_si128(reinterpret_cast<__m128i*>(dst) + 2, c);
        _mm_stream_si128(reinterpret_cast<__m128i*>(dst) + 3, d);
        src += 64;
        dst += 64;
    }
    _mm_sfence();
    if (bytes & 63) std::memcpy(dst, src, bytes & 63);
}

// Everything staged or in flight goes through the pipeline before the mode / batch size changes: the batch that failed
// earlier (if any), then the partly filled staging buffer as a short batch.  On a failure the batch concerned stays
// staged (the worker's retry slot) and the next call starts with it again.
static int stream_drain_staged(wifirx_handle* h)
{
    if (!h->w.thread.joinable()) return WIFIRX_OK;
    int rc = stream_resubmit_failed(h);
    if (rc) return rc;
    if (h->w.ring_fill) stream_submit(h, false);
    stream_worker_wait_idle(h);
    return stream_worker_take_error(h);
}

// wifirx_push and wifirx_push_iq behind their checks: `n` samples of format `fmt` (n = 0: flush)
static int stream_push(wifirx_handle* h, const void* iq, size_t n, int fmt, float scale, int iq_on_device)
{
    h->st.push_consumed = 0;
    if (n > 0 && !iq) return fail(h, WIFIRX_EINVAL, "iq is null");
    // the two kinds of stream share the queue and the absolute sample index: one handle cannot mix them
    if (h->div.n_ant) return fail(h, WIFIRX_EINVAL, "the handle's stream is a diversity stream (wifirx_push_diversity)");
    if (n > 0) h->st.single = true;
    const bool flush = (n == 0);
    // Device input, or no batching: the pipeline runs in the caller's thread, as one pass per push.
    if (iq_on_device || h->tune.stream_batch <= 0) {
        const int drc = stream_drain_staged(h);                   // samples staged before the mode changed
        if (drc) return drc;
        try {
            const int rc = stream_process(h, StreamCall{ &iq, fmt, scale, iq_on_device, flush, 0, nullptr }, n);
            if (rc == WIFIRX_OK) h->st.push_consumed = n;
            return rc;
        } catch (const std::exception& e) {
            return fail(h, WIFIRX_ENOMEM, std::string("wifirx_push: ") + e.what());
        }
    }
    // Host input with batching: copy into the pinned staging buffer; a full buffer (one batch) goes to the worker.
    // The failure of an earlier batch is reported once, by this call, before it takes anything; the call after it
    // submits that batch again (it is still staged) and goes on.  Samples that were staged belong to the stream: the
    // library runs them again itself, the caller never repeats them (wifirx_push_consumed).
    int rc = stream_worker_take_error(h);
    if (rc) return rc;
    if ((rc = stream_resubmit_failed(h))) return rc;
    Worker& w = h->w;
    const size_t cap = (size_t)h->tune.stream_batch;
    if (w.ring_cap != cap) {
        if ((rc = stream_drain_staged(h))) return rc;           // what was staged under the old batch size runs as a short batch
        HIP_TRY(h, hipSetDevice(h->device));
        for (PinnedBuf& r : w.ring) r.reset();
        w.ring_cap = 0;
        for (PinnedBuf& r : w.ring) {
            if ((rc = r.alloc(h, cap * sizeof(float2), "hipHostMalloc(staging)"))) {
                for (PinnedBuf& q : w.ring) q.reset();
                return rc;
            }
        }
        w.ring_cap = cap;
        w.ring_cur = 0;
    }
    // one format and scale per staged batch: what is staged in another runs first, as a short batch (the ring's bytes were
    // sized for float pairs, the widest format)
    const uint32_t bps = fmt == WIFIRX_IQ_FC32 ? (uint32_t)sizeof(float2) : wr_iq_sample_bytes(fmt);
    if (n && (w.ring_fmt != fmt || (fmt != WIFIRX_IQ_FC32 && w.ring_scale != scale))) {
        if (w.ring_fill && (rc = stream_drain_staged(h))) return rc;
        w.ring_fmt = fmt;
        w.ring_scale = scale;
    }
    if (!w.thread.joinable()) {
        w.stop = false;
        try {
            w.thread = std::thread(stream_worker_main, h);
        } catch (const std::exception& e) {
            return fail(h, WIFIRX_ENOMEM, std::string("cannot start the stream worker thread: ") + e.what());
        }
    }
    const uint8_t* src = static_cast<const uint8_t*>(iq);
    for (;;) {
        if (w.ring_fill == cap) {
            // hand-over.  The batch before this one must be through first (the worker takes one at a time); if it failed
            // it stays in the retry slot, this full buffer stays staged, and the call stops here: what it has staged so
            // far is consumed, the rest is the caller's to push again.
            stream_worker_wait_idle(h);
            if ((rc = stream_worker_take_error(h))) return rc;
            stream_submit(h, false);
        }
        if (!n) break;
        const size_t take = std::min(n, cap - w.ring_fill);
        stage_copy(w.ring[w.ring_cur].as<uint8_t>() + w.ring_fill * bps, src, take * bps);
        w.ring_fill += take;
        h->st.push_consumed += take;
        src += take * bps;
        n -= take;
    }
    if (flush) {
        stream_submit(h, true);                 // whatever is staged (possibly nothing) + settle the pending frames
        stream_worker_wait_idle(h);
        return stream_worker_take_error(h);     // on a failure the flush batch stays staged (retry slot): flush again
    }
    return WIFIRX_OK;
}

extern "C" int wifirx_push(wifirx_handle* h, const float* iq, size_t n, int iq_on_device)
{
    if (!h) return WIFIRX_EINVAL;
    return stream_push(h, iq, n, WIFIRX_IQ_FC32, 1.0f, iq_on_device);
}

extern "C" uint32_t wifirx_queued(const wifirx_handle* h) { return h ? h->st.n_queued.load(std::memory_order_acquire) : 0; }

extern "C" size_t wifirx_push_consumed(const wifirx_handle* h) { return h ? h->st.push_consumed : 0; }

extern "C" int wifirx_poll(wifirx_handle* h, wifirx_frame* frames, uint8_t* psdu, uint32_t psdu_stride,
                           uint8_t* idx, float* carrier, uint32_t cap, uint32_t* n_out)
{
    const wifirx_poll_out o = { frames, psdu, psdu_stride, 0, idx, carrier, nullptr, nullptr };
    return wifirx_poll_ex(h, &o, cap, n_out);
}

extern "C" int wifirx_poll_csi(wifirx_handle* h, wifirx_frame* frames, uint8_t* psdu, uint32_t psdu_stride,
                               uint8_t* idx, float* carrier, float* csi, uint32_t cap, uint32_t* n_out)
{
    const wifirx_poll_out o = { frames, psdu, psdu_stride, 0, idx, carrier, csi, nullptr };
    return wifirx_poll_ex(h, &o, cap, n_out);
}

// wifirx_poll_ex and wifirx_poll_diversity: the latter also delivers, per frame, the contributing antennas and the antennas' own
// records (zeros for the frames of a single stream)
static int stream_poll(wifirx_handle* h, const wifirx_poll_out* out, uint8_t* used_mask, wifirx_frame* ant_frames,
                       uint32_t n_ant, uint32_t cap, uint32_t* n_out)
{
    if (!h || !n_out || !out) return WIFIRX_EINVAL;
    *n_out = 0;
    if (cap && !out->frames) return fail(h, WIFIRX_EINVAL, "frames is null");
    uint8_t* const dst[SO_N] = { out->psdu, out->idx, reinterpret_cast<uint8_t*>(out->carrier),
                                 reinterpret_cast<uint8_t*>(out->csi), reinterpret_cast<uint8_t*>(out->sym_stats) };
    const std::array<StreamOut, SO_N> outs = stream_outs(h);
    uint32_t n = 0;
    std::lock_guard<std::mutex> lk(h->w.mu);
    while (n < cap && !h->st.queue.empty()) {
        const PolledFrame& pf = h->st.queue.front();
        const StreamBatch& b = *pf.batch;
        out->frames[n] = pf.fr;
        // the caller's row: what the frame filled, as far as its batch brought it back; zeros behind it
        for (int o = 0; o < SO_N; o++) {
            if (!dst[o]) continue;
            const size_t row = o == SO_PSDU ? out->psdu_stride : outs[o].pitch;
            const size_t c = std::min({ outs[o].bytes(pf.fr), b.width[o], row });
            if (c) std::memcpy(dst[o] + n * row, b.blob.data() + b.off[o] + pf.k * b.width[o], c);
            std::memset(dst[o] + n * row + c, 0, row - c);
        }
        if (used_mask) used_mask[n] = pf.k < b.used.size() ? b.used[pf.k] : 0;
        for (uint32_t a = 0; ant_frames && a < n_ant; a++) {
            if (a < b.n_ant) ant_frames[(size_t)n * n_ant + a] = b.ant[(size_t)pf.k * b.n_ant + a];
            else std::memset(&ant_frames[(size_t)n * n_ant + a], 0, sizeof(wifirx_frame));
        }
        h->st.queue.pop_front();
        n++;
    }
    h->st.n_queued.store((uint32_t)h->st.queue.size(), std::memory_order_release);
    *n_out = n;
    return WIFIRX_OK;
}

extern "C" int wifirx_poll_ex(wifirx_handle* h, const wifirx_poll_out* out, uint32_t cap, uint32_t* n_out)
{
    return stream_poll(h, out, nullptr, nullptr, 0, cap, n_out);
}
