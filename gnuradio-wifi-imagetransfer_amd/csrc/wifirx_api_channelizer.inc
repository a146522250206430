// wideband ingest (NUMERICS.md rule 21): the analysis bank on device buffers (wr_channelizer.hip) and its prototype

namespace {

// do the byte ranges [a, a + na) and [b, b + nb) share a byte?  (an empty range shares none)
bool ranges_overlap(const void* a, uint64_t na, const void* b, uint64_t nb)
{
    const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
    return na && nb && pa < pb + nb && pb < pa + na;
}

}  // namespace

extern "C" int wifirx_channelize(wifirx_handle* h, const void* in, int fmt, float scale, const void* hist, void* hist_out,
                                 uint32_t n_channels, int stacking, uint64_t n_out, uint64_t m0, float* out, uint64_t out_stride)
{
    if (!h) return WIFIRX_EINVAL;
    if (n_out && (!in || !out)) return fail(h, WIFIRX_EINVAL, "in and out are required");
    const uint32_t bps = fmt == WIFIRX_IQ_FC32 ? 8u : wr_iq_sample_bytes(fmt);
    if (!bps) return fail(h, WIFIRX_EINVAL, "fmt must be WIFIRX_IQ_FC32, WIFIRX_IQ_SC16 or WIFIRX_IQ_SC8");
    if (fmt != WIFIRX_IQ_FC32 && (!std::isfinite(scale) || !(scale > 0))) return fail(h, WIFIRX_EINVAL, "scale must be finite and > 0");
    if (n_channels != 2 && n_channels != 4 && n_channels != 8) return fail(h, WIFIRX_EINVAL, "n_channels must be 2, 4 or 8");
    if (stacking != 0 && stacking != 1) return fail(h, WIFIRX_EINVAL, "stacking must be 0 or 1");
    const uintptr_t align = bps - 1;
    if ((reinterpret_cast<uintptr_t>(in) & align) || (reinterpret_cast<uintptr_t>(hist) & align) ||
        (reinterpret_cast<uintptr_t>(hist_out) & align) || (reinterpret_cast<uintptr_t>(out) & 7))
        return fail(h, WIFIRX_EINVAL, "misaligned buffer (out: 8 bytes; in, hist, hist_out: fc32 8, sc16 4, sc8 2)");
    if (n_out > (1ull << 40)) return fail(h, WIFIRX_ERANGE, "n_out out of range");
    if (out_stride < n_out || out_stride > (1ull << 44)) return fail(h, WIFIRX_ERANGE, "out_stride must be n_out .. 2^44");
    const uint64_t M = n_channels, in_bytes = n_out * M * bps, hist_bytes = (uint64_t)WR_CZ_HIST * M * bps;
    const uint64_t out_bytes = n_out ? ((M - 1) * out_stride + n_out) * 8 : 0;        // first byte of row 0 to the last of row M - 1
    const uint64_t hin_bytes = hist ? hist_bytes : 0, hout_bytes = hist_out ? hist_bytes : 0;
    if (ranges_overlap(in, in_bytes, out, out_bytes) || ranges_overlap(hist, hin_bytes, out, out_bytes) ||
        ranges_overlap(hist_out, hout_bytes, out, out_bytes) || ranges_overlap(hist_out, hout_bytes, in, in_bytes) ||
        ranges_overlap(hist_out, hout_bytes, hist, hin_bytes) || ranges_overlap(hist, hin_bytes, in, in_bytes))
        return fail(h, WIFIRX_EINVAL, "in, hist, hist_out and out must not overlap");
    if (n_out == 0 && !hist_out) return WIFIRX_OK;
    stream_worker_wait_idle(h);
    HIP_TRY(h, hipSetDevice(h->device));
    if (n_out)
        HIP_TRY(h, wr_launch_channelize(h->stream, in, fmt, scale, hist, n_channels, stacking, n_out, m0, reinterpret_cast<float2*>(out), out_stride));
    if (hist_out) {
        // the last 23 M samples of (hist || in), queued behind the kernel: `keep` bytes of hist's tail, then in's tail
        uint8_t* dst = static_cast<uint8_t*>(hist_out);
        const uint64_t from_in = std::min(in_bytes, hist_bytes), keep = hist_bytes - from_in;
        if (keep && hist) HIP_TRY(h, hipMemcpyAsync(dst, static_cast<const uint8_t*>(hist) + from_in, keep, hipMemcpyDeviceToDevice, h->stream));
        else if (keep) HIP_TRY(h, hipMemsetAsync(dst, 0, keep, h->stream));
        if (from_in)
            HIP_TRY(h, hipMemcpyAsync(dst + keep, static_cast<const uint8_t*>(in) + (in_bytes - from_in), from_in, hipMemcpyDeviceToDevice, h->stream));
    }
    return WIFIRX_OK;
}

extern "C" int wifirx_channelizer_table(uint32_t n_channels, const float** taps, uint32_t* n_taps)
{
    const float* t = wr_channelizer_taps(n_channels);
    if (!t || !taps || !n_taps) return WIFIRX_EINVAL;
    *taps = t;
    *n_taps = WR_CZ_HIST * n_channels + n_channels;
    return WIFIRX_OK;
}
