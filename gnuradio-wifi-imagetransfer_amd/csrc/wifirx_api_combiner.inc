// wideband transmit (NUMERICS.md rule 22): the synthesis bank on device buffers (wr_combiner.hip)

extern "C" int wifirx_combine(wifirx_handle* h, const float* in, uint64_t in_stride, const float* gains, const float* hist,
                              float* hist_out, uint32_t n_channels, int stacking, uint64_t n_in, uint64_t m0, float* out)
{
    if (!h) return WIFIRX_EINVAL;
    if (n_in && (!in || !out)) return fail(h, WIFIRX_EINVAL, "in and out are required");
    if (n_channels != 2 && n_channels != 4 && n_channels != 8) return fail(h, WIFIRX_EINVAL, "n_channels must be 2, 4 or 8");
    if (stacking != 0 && stacking != 1) return fail(h, WIFIRX_EINVAL, "stacking must be 0 or 1");
    for (uint32_t k = 0; gains && k < n_channels; k++)
        if (!std::isfinite(gains[k])) return fail(h, WIFIRX_EINVAL, "gains must be finite");
    if ((reinterpret_cast<uintptr_t>(in) & 7) || (reinterpret_cast<uintptr_t>(hist) & 7) ||
        (reinterpret_cast<uintptr_t>(hist_out) & 7) || (reinterpret_cast<uintptr_t>(out) & 7))
        return fail(h, WIFIRX_EINVAL, "misaligned buffer (in, hist, hist_out, out: 8 bytes)");
    if (n_in > (1ull << 40)) return fail(h, WIFIRX_ERANGE, "n_in out of range");
    if (in_stride < n_in || in_stride > (1ull << 44)) return fail(h, WIFIRX_ERANGE, "in_stride must be n_in .. 2^44");
    const uint64_t M = n_channels, out_bytes = n_in * M * 8, hist_bytes = (uint64_t)WR_CB_HIST * M * 8;
    const uint64_t in_bytes = n_in ? ((M - 1) * in_stride + n_in) * 8 : 0;           // first byte of row 0 to the last of row M - 1
    const uint64_t hin_bytes = hist ? hist_bytes : 0, hout_bytes = hist_out ? hist_bytes : 0;
    if (ranges_overlap(in, in_bytes, out, out_bytes) || ranges_overlap(hist, hin_bytes, out, out_bytes) ||
        ranges_overlap(hist_out, hout_bytes, out, out_bytes) || ranges_overlap(hist_out, hout_bytes, in, in_bytes) ||
        ranges_overlap(hist_out, hout_bytes, hist, hin_bytes) || ranges_overlap(hist, hin_bytes, in, in_bytes))
        return fail(h, WIFIRX_EINVAL, "in, hist, hist_out and out must not overlap");
    if (n_in == 0 && !hist_out) return WIFIRX_OK;
    stream_worker_wait_idle(h);
    HIP_TRY(h, hipSetDevice(h->device));
    if (n_in)
        HIP_TRY(h, wr_launch_combine(h->stream, reinterpret_cast<const float2*>(in), in_stride, gains, reinterpret_cast<const float2*>(hist),
                                     n_channels, stacking, n_in, m0, reinterpret_cast<float2*>(out)));
    if (hist_out)   // the last 23 samples of (hist || in) of every row, queued behind the kernel
        HIP_TRY(h, wr_launch_combine_history(h->stream, reinterpret_cast<const float2*>(in), in_stride,
                                             reinterpret_cast<const float2*>(hist), n_channels, n_in, reinterpret_cast<float2*>(hist_out)));
    return WIFIRX_OK;
}
