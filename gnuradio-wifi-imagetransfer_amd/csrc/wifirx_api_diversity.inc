// receive diversity (NUMERICS.md rule 23): the combiner between A demodulated batches and one batch to decode (wr_diversity.hip)

extern "C" int wifirx_diversity_combine(wifirx_handle* h, uint32_t n_ant, const wifirx_out* in, uint32_t n_slots, int mode,
                                        const float* ant_gain, const wifirx_out* out, uint8_t* used_mask)
{
    if (!h) return WIFIRX_EINVAL;
    if (!in || !out || !out->frames) return fail(h, WIFIRX_EINVAL, "in, out and out->frames are required");
    if (n_ant < 1 || n_ant > WR_DIV_MAX_ANT) return fail(h, WIFIRX_EINVAL, "n_ant must be 1 .. 8");
    if (mode != WIFIRX_DIV_MRC && mode != WIFIRX_DIV_SELECT) return fail(h, WIFIRX_EINVAL, "mode must be WIFIRX_DIV_MRC or WIFIRX_DIV_SELECT");
    if (!out->on_device) return fail(h, WIFIRX_EINVAL, "device buffers only (on_device = 1)");
    if (out->hbits) return fail(h, WIFIRX_EINVAL, "out->hbits must be NULL: the combiner does not produce the planes");
    if (out->llr && h->cfg.llr_bits == 0) return fail(h, WIFIRX_EINVAL, "out->llr on a handle with llr_bits = 0");
    auto misaligned = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; };
    if (misaligned(out->frames) || misaligned(out->idx) || misaligned(out->llr) || misaligned(out->carrier))
        return fail(h, WIFIRX_EINVAL, "misaligned output buffer (frames, idx, llr, carrier: 16 bytes)");
    const void* outs[5] = { out->frames, out->idx, out->llr, out->carrier, used_mask };
    for (uint32_t a = 0; a < n_ant; a++) {
        if (!in[a].on_device) return fail(h, WIFIRX_EINVAL, "device buffers only (on_device = 1)");
        if (!in[a].frames || !in[a].carrier || !in[a].csi) return fail(h, WIFIRX_EINVAL, "every antenna needs frames, carrier and csi");
        if (misaligned(in[a].frames) || misaligned(in[a].carrier) || misaligned(in[a].csi))
            return fail(h, WIFIRX_EINVAL, "misaligned input buffer (frames, carrier, csi: 16 bytes)");
        if (ant_gain && !(std::isfinite(ant_gain[a]) && ant_gain[a] >= 0.0f)) return fail(h, WIFIRX_EINVAL, "ant_gain must be finite and >= 0");
        const void* ins[3] = { in[a].frames, in[a].carrier, in[a].csi };
        for (const void* o : outs)
            for (const void* i : ins)
                if (o && o == i) return fail(h, WIFIRX_EINVAL, "an output buffer is an input buffer");
    }
    if (h->cfg.max_batch && n_slots > h->cfg.max_batch) return fail(h, WIFIRX_ERANGE, "n_slots exceeds max_batch");
    if (n_slots == 0) return WIFIRX_OK;
    wr::DivArgs args{};
    for (uint32_t a = 0; a < n_ant; a++) {
        args.frames[a] = in[a].frames;
        args.carrier[a] = in[a].carrier;
        args.csi[a] = in[a].csi;
        args.gain[a] = ant_gain ? ant_gain[a] : 1.0f;
    }
    args.out_frames = out->frames;
    args.out_idx = out->idx;
    args.out_llr = out->llr;
    args.out_carrier = out->carrier;
    args.used_mask = used_mask;
    args.n_ant = n_ant;
    args.n_slots = n_slots;
    args.max_sym = h->cfg.max_sym;
    args.llr_bits = h->cfg.llr_bits;
    args.select = mode == WIFIRX_DIV_SELECT;
    args.has_gain = ant_gain != nullptr;
    args.llr_csi = h->tune.llr_csi != 0;
    args.llr_bf16 = h->tune.llr_format == WIFIRX_LLR_BF16;
    stream_worker_wait_idle(h);
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, wr_launch_diversity(h->stream, &args, h->n_cu));     // the host arrays travel as kernel arguments
    return WIFIRX_OK;
}
