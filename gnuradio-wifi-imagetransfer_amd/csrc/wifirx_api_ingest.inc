// what the calls in front of the demodulator share (the converters, the front end, the banks, the resampler, the tuner and the
// streams' entry points): the check of a sample format, the byte ranges of a call's buffers, and the history a call hands on

namespace {

// fmt and scale of rule 20's formats; *bps = bytes per sample.  fc32_ok: float pairs are a format of the call (8 bytes, and
// scale is not looked at)
int iq_check_format(wifirx_handle* h, int fmt, float scale, bool fc32_ok, uint32_t* bps)
{
    *bps = fc32_ok && fmt == WIFIRX_IQ_FC32 ? 8u : wr_iq_sample_bytes(fmt);
    if (!*bps)
        return fail(h, WIFIRX_EINVAL, fc32_ok ? "fmt must be WIFIRX_IQ_FC32, WIFIRX_IQ_SC16 or WIFIRX_IQ_SC8" : "fmt must be WIFIRX_IQ_SC16 or WIFIRX_IQ_SC8");
    if (fmt != WIFIRX_IQ_FC32 && (!std::isfinite(scale) || !(scale > 0))) return fail(h, WIFIRX_EINVAL, "scale must be finite and > 0");
    return WIFIRX_OK;
}

// do the byte ranges [a, a + na) and [b, b + nb) share a byte?  (an empty range shares none)
bool ranges_overlap(const void* a, uint64_t na, const void* b, uint64_t nb)
{
    const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
    return na && nb && pa < pb + nb && pb < pa + na;
}

struct ByteRange { const void* p; uint64_t bytes; };

// do any two of the N ranges share a byte?
template <size_t N>
bool any_overlap(const ByteRange (&r)[N])
{
    for (size_t a = 0; a < N; a++)
        for (size_t b = a + 1; b < N; b++)
            if (ranges_overlap(r[a].p, r[a].bytes, r[b].p, r[b].bytes)) return true;
    return false;
}

// hist_out = the last hist_bytes of (hist || in), queued behind the call's kernel: `keep` bytes of hist's tail (zeros for a
// NULL hist), then in's tail
int queue_hist_tail(wifirx_handle* h, const void* in, uint64_t in_bytes, const void* hist, void* hist_out, uint64_t hist_bytes)
{
    uint8_t* dst = static_cast<uint8_t*>(hist_out);
    const uint64_t from_in = std::min(in_bytes, hist_bytes), keep = hist_bytes - from_in;
    if (keep && hist) HIP_TRY(h, hipMemcpyAsync(dst, static_cast<const uint8_t*>(hist) + from_in, keep, hipMemcpyDeviceToDevice, h->stream));
    else if (keep) HIP_TRY(h, hipMemsetAsync(dst, 0, keep, h->stream));
    if (from_in)
        HIP_TRY(h, hipMemcpyAsync(dst + keep, static_cast<const uint8_t*>(in) + (in_bytes - from_in), from_in, hipMemcpyDeviceToDevice, h->stream));
    return WIFIRX_OK;
}

}  // namespace
