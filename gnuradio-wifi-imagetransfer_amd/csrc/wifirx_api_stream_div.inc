// Stream-mode receive diversity: the stream pipeline for the n_ant sample-synchronous antennas of one radio.  Detection runs
// once, on the sum of the antennas' autocorrelations and powers (NUMERICS.md rule 24, wr_detect_multi.hip), so every antenna
// gets the same triggers and the same coarse CFO and slot i of every antenna is the same transmission by construction.
// The pass is stream_process (wifirx_api_stream.inc) over n_ant sample planes: its reserve, ingest, joint detection, host state
// machine, queue and carry, and its all-or-nothing contract.  What this file adds is the frames step of such a pass
// (div_frames): one frame-kernel launch per antenna on that antenna's plane with the same triggers and the joint A, the
// combiner (rule 23, wr_diversity.hip) over the n_ant row sets, decode_mac on the combined rows; and the entry points.
// Everything runs in the caller's thread on the handle's stream: the pinned ring and the worker of the single stream are not
// built for n_ant host streams.  The st.* output rows are the combined set; DivStream holds the antennas' own rows.

namespace {

// the combined rows (stream_out_reserve) and the antennas' own rows for up to `n` triggers
int div_out_reserve(wifirx_handle* h, uint32_t n)
{
    DivStream& d = h->div;
    if (int rc = stream_out_reserve(h, n)) return rc;
    if (n <= d.cap) return WIFIRX_OK;
    const uint32_t cap = h->st.out_cap;
    const size_t per = (size_t)h->cfg.max_sym * 48, rows = (size_t)d.n_ant * cap;
    struct { DevBuf& b; size_t bytes; } req[] = {
        { d.frames, rows * sizeof(wifirx_frame) }, { d.car, rows * per * sizeof(float2) }, { d.csi, rows * 52 * sizeof(float2) },
        { d.stats, rows * sizeof(float4) }, { d.used, (size_t)cap }, { d.src, (size_t)cap },
    };
    d.cap = 0;
    for (auto& r : req) r.b.reset();
    for (auto& r : req) {
        if (int rc = stream_alloc(h, r.b, r.bytes, "hipMalloc(diversity stream rows)")) {
            for (auto& q : req) q.b.reset();
            return rc;
        }
    }
    d.cap = cap;
    return WIFIRX_OK;
}

bool div_usable(const wifirx_handle* h, const wifirx_frame& f)
{
    const uint32_t need = WIFIRX_F_SIGNAL | WIFIRX_F_COMPLETE;
    return (f.flags & need) == need && f.encoding <= 7 && f.n_sym <= h->cfg.max_sym;
}

}  // namespace

// Frames: per antenna the frame kernel over every pending trigger, the combiner, decode_mac on the combined rows; records, outputs
static int div_frames(wifirx_handle* h, const StreamCall& c, StageClock& stage, FramePass& p)
{
    StreamState& st = h->st;
    DivStream& d = h->div;
    FramesBegin f;
    int rc = stream_frames_begin(h, div_out_reserve, c.flush, p, f);
    if (rc || !f.np) return rc;
    const uint32_t np = f.np, A = d.n_ant;
    const size_t per = (size_t)h->cfg.max_sym * 48;
    if (!f.outs[SO_IDX].produced) HIP_TRY(h, hipMemsetAsync(st.idx.p, 0, np * per, h->stream));       // the decoder reads them all the same
    wr::DivArgs args{};
    for (uint32_t a = 0; a < A; a++) {
        const size_t row0 = (size_t)a * d.cap;
        // (a csi row is written once SYNC is set: zeros otherwise, as in the single stream)
        HIP_TRY(h, hipMemsetAsync(d.csi.as<float2>() + row0 * 52, 0, (size_t)np * 52 * sizeof(float2), h->stream));
        const wr::DemodOut dout = { d.frames.as<wifirx_frame>() + row0, nullptr, nullptr, d.car.as<float2>() + row0 * per,
                                    d.csi.as<float2>() + row0 * 52, d.stats.as<float4>() + row0, nullptr };
        HIP_TRY(h, wr_launch_demod_stream(h->stream, stream_plane(h, a), st.sfill, st.trig.as<wr::StreamTrig>(), np, &f.prm, st.A.as<float2>(), &dout));
        args.frames[a] = dout.frames;
        args.carrier[a] = reinterpret_cast<const float*>(dout.carrier);
        args.csi[a] = reinterpret_cast<const float*>(dout.csi);
        args.gain[a] = c.ant_gain ? c.ant_gain[a] : 1.0f;
    }
    args.out_frames = st.frames.as<wifirx_frame>();
    args.out_idx = st.idx.as<uint8_t>();
    args.out_llr = f.d_llr;
    args.out_carrier = h->cfg.want_carrier ? st.car.as<float>() : nullptr;
    args.used_mask = d.used.as<uint8_t>();
    args.n_ant = A;
    args.n_slots = np;
    args.max_sym = h->cfg.max_sym;
    args.llr_bits = f.prm.llr_bits;
    args.select = c.mode == WIFIRX_DIV_SELECT;
    args.has_gain = c.ant_gain != nullptr;
    args.llr_csi = h->tune.llr_csi != 0;
    args.llr_bf16 = 0;                          // stream mode keeps float32
    HIP_TRY(h, wr_launch_diversity(h->stream, &args, h->n_cu));
    stage("enqueue frame kernels + combiner");
    // hbits stays NULL: the decoder packs the planes from idx, as it does behind the batch combiner
    const wifirx_out o = { st.frames.as<wifirx_frame>(), st.idx.as<uint8_t>(), f.d_llr, nullptr, st.psdu.as<uint8_t>(), 2048, 1,
                           nullptr, nullptr, nullptr };
    if ((rc = f.soft ? decode_batch_soft_impl(h, np, &o, 6, false) : decode_batch_impl(h, np, &o))) return rc;
    stage("frame kernels + combiner + decode_mac");
    // the records: the combined ones, every antenna's own, the contributing antennas
    p.fr.resize(np);
    std::vector<wifirx_frame> ant((size_t)A * np);
    p.used.resize(np);
    HIP_TRY(h, hipMemcpyAsync(p.fr.data(), st.frames.p, np * sizeof(wifirx_frame), hipMemcpyDeviceToHost, h->stream));
    for (uint32_t a = 0; a < A; a++)
        HIP_TRY(h, hipMemcpyAsync(ant.data() + (size_t)a * np, d.frames.as<wifirx_frame>() + (size_t)a * d.cap, np * sizeof(wifirx_frame),
                                  hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipMemcpyAsync(p.used.data(), d.used.p, np, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    // The csi and sym_stats rows are the reference antenna's: the lowest usable antenna whose snr_db equals the combined
    // record's (antenna 0 where none is usable: its record is the one delivered).  The host names it, the device gathers.
    std::vector<uint8_t> src(np, 0);
    p.ant.resize((size_t)np * A);
    p.hold.assign(np, 0);
    p.n_ant = A;
    for (uint32_t k = 0; k < np; k++) {
        bool found = false;
        for (uint32_t a = 0; a < A; a++) {
            wifirx_frame f = ant[(size_t)a * np + k];
            if (!found && div_usable(h, f) && std::memcmp(&f.snr_db, &p.fr[k].snr_db, sizeof(float)) == 0) { src[k] = (uint8_t)a; found = true; }
            if (!(f.flags & WIFIRX_F_COMPLETE) && (f.flags & WIFIRX_F_TRUNCATED)) p.hold[k] = 1;       // this antenna still waits for samples
            f.trigger = (int32_t)(st.pending[k].pos & 0x7fffffff);
            p.ant[(size_t)k * A + a] = f;
        }
    }
    HIP_TRY(h, hipMemcpyAsync(d.src.p, src.data(), np, hipMemcpyHostToDevice, h->stream));
    wr::GatherArgs g{};
    for (uint32_t a = 0; a < A; a++) {
        g.csi[a] = d.csi.as<float2>() + (size_t)a * d.cap * 52;
        g.stats[a] = d.stats.as<float4>() + (size_t)a * d.cap;
    }
    g.ant = d.src.as<uint8_t>();
    g.out_csi = st.csi.as<float2>();
    g.out_stats = st.stats.as<float4>();
    g.n = np;
    g.n_ant = A;
    HIP_TRY(h, wr_launch_row_gather(h->stream, &g));
    return stream_pack_outputs(h, f.outs, stage, p);       // (waits: src stays alive until then)
}

extern "C" int wifirx_push_diversity(wifirx_handle* h, const wifirx_div_stream* cfg, const void* const* iq, size_t n)
{
    if (!h) return WIFIRX_EINVAL;
    if (!cfg || !iq) return fail(h, WIFIRX_EINVAL, "cfg and iq are required");
    if (cfg->n_ant < 1 || cfg->n_ant > WR_DET_MAX_ANT) return fail(h, WIFIRX_EINVAL, "n_ant must be 1 .. 8");
    if (h->div.n_ant && cfg->n_ant != h->div.n_ant) return fail(h, WIFIRX_EINVAL, "n_ant differs from the handle's first wifirx_push_diversity");
    if (h->st.single) return fail(h, WIFIRX_EINVAL, "the handle's stream has taken samples through wifirx_push / wifirx_push_iq");
    if (h->st.fe_on) return fail(h, WIFIRX_EINVAL, "the handle's front end is on (wifirx_stream_frontend): the diversity stream has none");
    if (cfg->mode != WIFIRX_DIV_MRC && cfg->mode != WIFIRX_DIV_SELECT) return fail(h, WIFIRX_EINVAL, "mode must be WIFIRX_DIV_MRC or WIFIRX_DIV_SELECT");
    uint32_t bps;
    if (int rc = iq_check_format(h, cfg->fmt, cfg->scale, true, &bps)) return rc;
    for (uint32_t a = 0; a < cfg->n_ant; a++) {
        if (cfg->ant_gain && !(std::isfinite(cfg->ant_gain[a]) && cfg->ant_gain[a] >= 0.0f)) return fail(h, WIFIRX_EINVAL, "ant_gain must be finite and >= 0");
        if (n > 0 && !iq[a]) return fail(h, WIFIRX_EINVAL, "iq[a] is null");
        const uintptr_t align = cfg->fmt != WIFIRX_IQ_FC32 || cfg->iq_on_device ? bps : 1;       // float pairs on the host: any address
        if (reinterpret_cast<uintptr_t>(iq[a]) & (align - 1)) return fail(h, WIFIRX_EINVAL, "iq[a] is misaligned (float pairs on the device: 8 bytes; sc16: 4; sc8: 2)");
    }
    if (n > (size_t)1 << 40) return fail(h, WIFIRX_EINVAL, "n out of range");
    h->div.n_ant = cfg->n_ant;
    try {
        return stream_process(h, StreamCall{ iq, cfg->fmt, cfg->scale, cfg->iq_on_device, n == 0, cfg->mode, cfg->ant_gain }, n);
    } catch (const std::exception& e) {
        return fail(h, WIFIRX_ENOMEM, std::string("wifirx_push_diversity: ") + e.what());
    }
}

extern "C" int wifirx_poll_diversity(wifirx_handle* h, const wifirx_poll_out* out, uint8_t* used_mask, wifirx_frame* ant_frames,
                                     uint32_t cap, uint32_t* n_out)
{
    return stream_poll(h, out, used_mask, ant_frames, h ? h->div.n_ant : 0, cap, n_out);
}

extern "C" int wifirx_detect_multi(wifirx_handle* h, uint32_t n_ant, const float* const* iq_dev, uint64_t n, float threshold,
                                   uint64_t* masks_dev, float* A_dev, float* P_dev)
{
    if (!h) return WIFIRX_EINVAL;
    if (!iq_dev) return fail(h, WIFIRX_EINVAL, "iq_dev is required");
    if (n_ant < 1 || n_ant > WR_DET_MAX_ANT) return fail(h, WIFIRX_EINVAL, "n_ant must be 1 .. 8");
    if (!(threshold >= 0)) return fail(h, WIFIRX_EINVAL, "threshold must be >= 0");       // squared comparison, NUMERICS.md rule 3
    if (n > 0 && (!masks_dev || !A_dev)) return fail(h, WIFIRX_EINVAL, "masks_dev and A_dev are required");
    if (n > (uint64_t)1 << 40) return fail(h, WIFIRX_EINVAL, "n out of range");
    auto misaligned = [](const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; };
    if (misaligned(masks_dev, 8) || misaligned(A_dev, 8) || misaligned(P_dev, 4)) return fail(h, WIFIRX_EINVAL, "misaligned buffer (masks, A: 8 bytes; P: 4)");
    wr::DetectMultiArgs args{};
    for (uint32_t a = 0; a < n_ant; a++) {
        if (n > 0 && !iq_dev[a]) return fail(h, WIFIRX_EINVAL, "iq_dev[a] is null");
        if (misaligned(iq_dev[a], 8)) return fail(h, WIFIRX_EINVAL, "iq_dev[a] is misaligned (float pairs: 8 bytes)");
        args.x[a] = reinterpret_cast<const float2*>(iq_dev[a]);
    }
    if (n == 0) return WIFIRX_OK;
    args.n_samp = (int64_t)n;
    args.tile0 = 0;
    args.n_tiles = (int64_t)((n + 63) / 64);
    args.thr = threshold;
    args.n_ant = n_ant;
    args.masks = masks_dev;
    args.A = reinterpret_cast<float2*>(A_dev);
    args.P = P_dev;
    stream_worker_wait_idle(h);
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, wr_launch_stream_detect_multi(h->stream, &args));
    return WIFIRX_OK;
}
