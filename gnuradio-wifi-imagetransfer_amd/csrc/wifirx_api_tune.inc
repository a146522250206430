// the tuner on device buffers (NUMERICS.md rule 35; wr_arb.hip, tune_kernel): K channels at any centre out of one capture,
// each mixed by rule 17's fixed-point phase ramp on the way into rule 34's sum.  The checks and the counting are
// wifirx_arb_resample's (wifirx_api_arb.inc), the history's copies every ingest call's (wifirx_api_ingest.inc).

extern "C" int wifirx_tune_inc(double offset_hz, double sample_rate, uint64_t* inc)
{
    if (!inc || !std::isfinite(offset_hz) || !std::isfinite(sample_rate) || !(sample_rate > 0)) return WIFIRX_EINVAL;
    double t = offset_hz / sample_rate;
    t -= std::rint(t);                                       // exact: |t| <= 1/2
    const double v = t * 0x1p64;
    if (v >= 0x1p63 || v <= -0x1p63) { *inc = 1ull << 63; return WIFIRX_OK; }
    *inc = (uint64_t)(-std::llround(v));
    return WIFIRX_OK;
}

extern "C" int wifirx_tune(wifirx_handle* h, const void* in, int fmt, float scale, uint64_t n_in, const void* hist, void* hist_out,
                           uint32_t num, uint32_t den, uint32_t n_channels, const uint64_t* inc, const uint64_t* phase0,
                           uint64_t j0, uint64_t m0, float* out, uint64_t out_stride, uint64_t* n_out)
{
    if (!h) return WIFIRX_EINVAL;
    if (n_channels < 1 || n_channels > WIFIRX_TUNE_MAX_CHANNELS) return fail(h, WIFIRX_EINVAL, "n_channels must be 1 .. 8");
    if (!inc) return fail(h, WIFIRX_EINVAL, "inc is required");
    arb_call c;
    if (int rc = arb_check_call(h, in, fmt, scale, n_in, hist, hist_out, num, den, j0, m0, out, out_stride, n_out, &c)) return rc;
    if (out_stride >= ARB_INDEX_LIMIT / (8 * WIFIRX_TUNE_MAX_CHANNELS))
        return fail(h, WIFIRX_ERANGE, "out_stride must stay below 2^56");
    if (int rc = arb_check_buffers(h, c, in, hist, hist_out, out, out ? n_channels * out_stride * 8 : 0, j0, m0)) return rc;
    wr_tune_channels ch = {};
    for (uint32_t k = 0; k < n_channels; k++) {
        ch.inc[k] = inc[k];
        ch.phase0[k] = phase0 ? phase0[k] : 0;
    }
    ch.out_stride = out_stride;
    *n_out = c.n;
    if (c.n == 0 && !hist_out) return WIFIRX_OK;
    stream_worker_wait_idle(h);
    HIP_TRY(h, hipSetDevice(h->device));
    if (c.n)
        HIP_TRY(h, wr_launch_tune(h->stream, in, fmt, scale, n_in, hist, &c.r, j0, m0, c.n, reinterpret_cast<float2*>(out),
                                  n_channels, &ch));
    return hist_out ? queue_hist_tail(h, in, c.in_bytes, hist, hist_out, c.hist_bytes) : WIFIRX_OK;
}
