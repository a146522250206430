// the filter banks on device buffers: wideband ingest (NUMERICS.md rule 21: the analysis bank, wr_channelizer.hip, and its
// prototype) and wideband transmit (rule 22: the synthesis bank, wr_combiner.hip)

namespace {

static_assert(WR_CZ_HIST == WR_CB_HIST, "one history length for both banks");

// The buffers of a bank call.  `wide`: one interleaved stream of n * M samples of bps bytes, aligned to bps, as are hist and
// hist_out of 23 * M such samples each.  `rows`: M rows of n float pairs, `stride` pairs apart, aligned to 8 bytes.  No two
// of the four may share a byte.  side ("in" or "out") is what the caller calls its rows; misaligned is its text for that.
int bank_check(wifirx_handle* h, const void* wide, uint32_t bps, const void* rows, uint64_t stride, uint64_t n, uint64_t M,
               const void* hist, const void* hist_out, const std::string& side, const char* misaligned)
{
    const uintptr_t align = bps - 1;
    if ((reinterpret_cast<uintptr_t>(wide) & align) || (reinterpret_cast<uintptr_t>(hist) & align) ||
        (reinterpret_cast<uintptr_t>(hist_out) & align) || (reinterpret_cast<uintptr_t>(rows) & 7))
        return fail(h, WIFIRX_EINVAL, misaligned);
    if (n > (1ull << 40)) return fail(h, WIFIRX_ERANGE, "n_" + side + " out of range");
    if (stride < n || stride > (1ull << 44)) return fail(h, WIFIRX_ERANGE, side + "_stride must be n_" + side + " .. 2^44");
    const uint64_t hist_bytes = (uint64_t)WR_CZ_HIST * M * bps;
    const ByteRange r[4] = {
        { wide, n * M * bps }, { rows, n ? ((M - 1) * stride + n) * 8 : 0 },         // first byte of row 0 to the last of row M - 1
        { hist, hist ? hist_bytes : 0 }, { hist_out, hist_out ? hist_bytes : 0 } };
    if (any_overlap(r)) return fail(h, WIFIRX_EINVAL, "in, hist, hist_out and out must not overlap");
    return WIFIRX_OK;
}

}  // namespace

extern "C" int wifirx_channelize(wifirx_handle* h, const void* in, int fmt, float scale, const void* hist, void* hist_out,
                                 uint32_t n_channels, int stacking, uint64_t n_out, uint64_t m0, float* out, uint64_t out_stride)
{
    if (!h) return WIFIRX_EINVAL;
    if (n_out && (!in || !out)) return fail(h, WIFIRX_EINVAL, "in and out are required");
    uint32_t bps;
    if (int rc = iq_check_format(h, fmt, scale, true, &bps)) return rc;
    if (n_channels != 2 && n_channels != 4 && n_channels != 8) return fail(h, WIFIRX_EINVAL, "n_channels must be 2, 4 or 8");
    if (stacking != 0 && stacking != 1) return fail(h, WIFIRX_EINVAL, "stacking must be 0 or 1");
    if (const int rc = bank_check(h, in, bps, out, out_stride, n_out, n_channels, hist, hist_out, "out",
                                  "misaligned buffer (out: 8 bytes; in, hist, hist_out: fc32 8, sc16 4, sc8 2)"))
        return rc;
    if (n_out == 0 && !hist_out) return WIFIRX_OK;
    stream_worker_wait_idle(h);
    HIP_TRY(h, hipSetDevice(h->device));
    if (n_out)
        HIP_TRY(h, wr_launch_channelize(h->stream, in, fmt, scale, hist, n_channels, stacking, n_out, m0, reinterpret_cast<float2*>(out), out_stride));
    // the last 23 M samples of (hist || in)
    return hist_out ? queue_hist_tail(h, in, n_out * n_channels * bps, hist, hist_out, (uint64_t)WR_CZ_HIST * n_channels * bps) : WIFIRX_OK;
}

extern "C" int wifirx_channelizer_table(uint32_t n_channels, const float** taps, uint32_t* n_taps)
{
    const float* t = wr_channelizer_taps(n_channels);
    if (!t || !taps || !n_taps) return WIFIRX_EINVAL;
    *taps = t;
    *n_taps = WR_CZ_HIST * n_channels + n_channels;
    return WIFIRX_OK;
}

extern "C" int wifirx_combine(wifirx_handle* h, const float* in, uint64_t in_stride, const float* gains, const float* hist,
                              float* hist_out, uint32_t n_channels, int stacking, uint64_t n_in, uint64_t m0, float* out)
{
    if (!h) return WIFIRX_EINVAL;
    if (n_in && (!in || !out)) return fail(h, WIFIRX_EINVAL, "in and out are required");
    if (n_channels != 2 && n_channels != 4 && n_channels != 8) return fail(h, WIFIRX_EINVAL, "n_channels must be 2, 4 or 8");
    if (stacking != 0 && stacking != 1) return fail(h, WIFIRX_EINVAL, "stacking must be 0 or 1");
    for (uint32_t k = 0; gains && k < n_channels; k++)
        if (!std::isfinite(gains[k])) return fail(h, WIFIRX_EINVAL, "gains must be finite");
    if (const int rc = bank_check(h, out, 8, in, in_stride, n_in, n_channels, hist, hist_out, "in",
                                  "misaligned buffer (in, hist, hist_out, out: 8 bytes)"))
        return rc;
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
