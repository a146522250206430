// pre-detection combining (NUMERICS.md rule 33): A antennas' sample rows into the one row set the demod reads (wr_precombine.hip)

extern "C" int wifirx_precombine(wifirx_handle* h, uint32_t n_ant, const float* const* iq_dev, uint32_t slot_len, uint32_t n_slots,
                                 uint32_t iters, float* out_dev, float* weights_dev, void* stats_dev)
{
    if (!h) return WIFIRX_EINVAL;
    if (!iq_dev || !out_dev) return fail(h, WIFIRX_EINVAL, "iq_dev and out_dev are required");
    if (n_ant < 1 || n_ant > WR_PRE_MAX_ANT) return fail(h, WIFIRX_EINVAL, "n_ant must be 1 .. 8");
    if (slot_len < 64 || slot_len > 65536 || (slot_len & 63)) return fail(h, WIFIRX_EINVAL, "slot_len must be a multiple of 64 in 64 .. 65536");
    if (iters > WR_PRE_MAX_ITERS) return fail(h, WIFIRX_EINVAL, "iters must be 0 .. 4");
    auto misaligned = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) != 0; };
    if (misaligned(out_dev) || misaligned(weights_dev) || misaligned(stats_dev))
        return fail(h, WIFIRX_EINVAL, "misaligned output buffer (out, weights, stats: 8 bytes)");
    for (uint32_t a = 0; a < n_ant; a++) {
        if (!iq_dev[a]) return fail(h, WIFIRX_EINVAL, "every antenna needs its samples");
        if (misaligned(iq_dev[a])) return fail(h, WIFIRX_EINVAL, "misaligned input buffer (8 bytes)");
        if (iq_dev[a] == out_dev) return fail(h, WIFIRX_EINVAL, "out_dev is an input buffer");
    }
    if (h->cfg.max_batch && n_slots > h->cfg.max_batch) return fail(h, WIFIRX_ERANGE, "n_slots exceeds max_batch");
    if (n_slots == 0) return WIFIRX_OK;
    wr::PreArgs args{};
    for (uint32_t a = 0; a < n_ant; a++) args.x[a] = reinterpret_cast<const float2*>(iq_dev[a]);
    args.out = reinterpret_cast<float2*>(out_dev);
    args.weights = reinterpret_cast<float2*>(weights_dev);
    args.stats = reinterpret_cast<uint2*>(stats_dev);
    args.n_ant = n_ant;
    args.slot_len = slot_len;
    args.n_slots = n_slots;
    args.iters = iters;
    stream_worker_wait_idle(h);
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, wr_launch_precombine(h->stream, &args));              // the host array travels as kernel arguments
    return WIFIRX_OK;
}
