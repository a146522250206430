// sample formats (NUMERICS.md rule 20): the two converters on device buffers (wr_convert.hip), and the stream's entry point
// for samples that arrive as integers (the stream side is stream_push, wifirx_api_stream.inc)

namespace {

// what both converters check before anything is queued: `ints` is the integer side, `floats` the float side
int check_convert(wifirx_handle* h, const void* ints, const void* floats, int fmt, uint64_t n, float scale)
{
    if (!ints || !floats) return fail(h, WIFIRX_EINVAL, "src and dst are required");
    uint32_t bps;
    if (int rc = iq_check_format(h, fmt, scale, false, &bps)) return rc;
    const uintptr_t pi = reinterpret_cast<uintptr_t>(ints), pf = reinterpret_cast<uintptr_t>(floats);
    if ((pi & (bps - 1)) || (pf & 7)) return fail(h, WIFIRX_EINVAL, "misaligned buffer (float pairs: 8 bytes; sc16: 4; sc8: 2)");
    if (n > (UINT64_MAX >> 4)) return fail(h, WIFIRX_EINVAL, "n out of range");
    if (ranges_overlap(ints, n * bps, floats, n * 8)) return fail(h, WIFIRX_EINVAL, "src and dst overlap");
    return WIFIRX_OK;
}

}  // namespace

extern "C" int wifirx_iq_to_f32(wifirx_handle* h, const void* src, int fmt, uint64_t n, float scale, float* dst)
{
    if (!h) return WIFIRX_EINVAL;
    if (int rc = check_convert(h, src, dst, fmt, n, scale)) return rc;
    if (n == 0) return WIFIRX_OK;
    stream_worker_wait_idle(h);
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, wr_launch_iq_widen(h->stream, src, fmt, n, scale, reinterpret_cast<float2*>(dst), h->n_cu));
    return WIFIRX_OK;
}

extern "C" int wifirx_iq_from_f32(wifirx_handle* h, const float* src, uint64_t n, float scale, int fmt, uint32_t bits,
                                  void* dst, uint64_t* clipped)
{
    if (!h) return WIFIRX_EINVAL;
    if (int rc = check_convert(h, dst, src, fmt, n, scale)) return rc;
    if (bits < 2 || bits > (fmt == WIFIRX_IQ_SC16 ? 16u : 8u)) return fail(h, WIFIRX_EINVAL, "bits must be 2..16 (sc16) or 2..8 (sc8)");
    if (n == 0) {
        if (clipped) *clipped = 0;
        return WIFIRX_OK;
    }
    stream_worker_wait_idle(h);
    HIP_TRY(h, hipSetDevice(h->device));
    unsigned long long* d_count = nullptr;
    if (clipped) {
        if (int rc = h->stage.iq_clipped.reserve(h, sizeof(unsigned long long))) return rc;
        d_count = h->stage.iq_clipped.as<unsigned long long>();
        HIP_TRY(h, hipMemsetAsync(d_count, 0, sizeof(unsigned long long), h->stream));
    }
    HIP_TRY(h, wr_launch_iq_quantise(h->stream, reinterpret_cast<const float2*>(src), n, scale, fmt, bits, dst, d_count, h->n_cu));
    if (clipped) {
        unsigned long long got = 0;
        HIP_TRY(h, hipMemcpyAsync(&got, d_count, sizeof(got), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        *clipped = got;
    }
    return WIFIRX_OK;
}

extern "C" int wifirx_push_iq(wifirx_handle* h, const void* iq, size_t n, int fmt, float scale, int iq_on_device)
{
    if (!h) return WIFIRX_EINVAL;
    if (fmt == WIFIRX_IQ_FC32) return wifirx_push(h, static_cast<const float*>(iq), n, iq_on_device);
    h->st.push_consumed = 0;
    uint32_t bps;
    if (int rc = iq_check_format(h, fmt, scale, true, &bps)) return rc;         // (float pairs have gone to wifirx_push)
    if (reinterpret_cast<uintptr_t>(iq) & (bps - 1)) return fail(h, WIFIRX_EINVAL, "iq is misaligned (sc16: 4 bytes; sc8: 2)");
    return stream_push(h, iq, n, fmt, scale, iq_on_device);
}
