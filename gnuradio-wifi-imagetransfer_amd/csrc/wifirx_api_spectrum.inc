// the band survey on device buffers (NUMERICS.md rule 36; wr_spectrum.hip): windowed-FFT power rows of a stream in its native
// format, the fold of rows, the band powers of rows, and the host arithmetic of a band's bins.  Every argument is checked
// before a device is looked for, as wifirx_tune does.

namespace {

constexpr uint64_t SPEC_INDEX_LIMIT = 1ull << 62;            // n_in stays below it, so no sample's byte offset overflows
constexpr uint64_t SPEC_ROWS_LIMIT = 1ull << 40;             // rows of a fold: rows * n_fft * 4 bytes stay below 2^54

bool spec_n_ok(uint32_t n_fft) { return n_fft == 64 || n_fft == 256 || n_fft == 1024 || n_fft == 4096; }
bool spec_mode_ok(int mode) { return mode == WIFIRX_SPEC_SUM || mode == WIFIRX_SPEC_MAX; }

// rule 36's counting; false for arguments outside the rule
bool spec_count(uint32_t n_fft, uint32_t hop, uint32_t avg, uint64_t n_in, uint64_t* n_rows, uint64_t* consumed)
{
    if (!spec_n_ok(n_fft) || hop < 1 || hop > WIFIRX_SPEC_MAX_HOP || avg < 1 || avg > WIFIRX_SPEC_MAX_HOP) return false;
    const uint64_t S = n_in >= n_fft ? (n_in - n_fft) / hop + 1 : 0;
    *n_rows = S / avg;
    *consumed = *n_rows * avg * hop;                         // <= S hop <= n_in - n_fft + hop < 2^62 + 2^20
    return true;
}

}  // namespace

extern "C" int wifirx_spectrum_count(uint32_t n_fft, uint32_t hop, uint32_t avg, uint64_t n_in, uint64_t* n_rows, uint64_t* consumed)
{
    if (!n_rows || !consumed) return WIFIRX_EINVAL;
    uint64_t r, c;
    if (!spec_count(n_fft, hop, avg, n_in, &r, &c)) return WIFIRX_EINVAL;
    if (n_in >= SPEC_INDEX_LIMIT) return WIFIRX_ERANGE;
    *n_rows = r;
    *consumed = c;
    return WIFIRX_OK;
}

extern "C" int wifirx_spectrum_band(double offset_hz, double width_hz, double sample_rate, uint32_t n_fft, uint32_t* lo, uint32_t* hi)
{
    if (!lo || !hi || !spec_n_ok(n_fft)) return WIFIRX_EINVAL;
    if (!std::isfinite(offset_hz) || !std::isfinite(width_hz) || !std::isfinite(sample_rate) || !(sample_rate > 0) || !(width_hz > 0))
        return WIFIRX_EINVAL;
    const double a = std::ceil((offset_hz - width_hz / 2) * n_fft / sample_rate);
    const double b = std::ceil((offset_hz + width_hz / 2) * n_fft / sample_rate);
    const double half = n_fft / 2;
    if (!(a >= -half) || !(b <= half) || !(a < b)) return WIFIRX_ERANGE;
    *lo = (uint32_t)(int64_t)(a + half);
    *hi = (uint32_t)(int64_t)(b + half);
    return WIFIRX_OK;
}

extern "C" int wifirx_spectrum_table(const float** hann, const float** blackman_harris, const float** twiddle, uint32_t* n_entries)
{
    if (!hann || !blackman_harris || !twiddle || !n_entries) return WIFIRX_EINVAL;
    *hann = wr_spectrum_host_hann();
    *blackman_harris = wr_spectrum_host_blackman_harris();
    *twiddle = wr_spectrum_host_twiddle();
    *n_entries = WR_SPEC_ENTRIES;
    return WIFIRX_OK;
}

extern "C" int wifirx_spectrum(wifirx_handle* h, const void* in, int fmt, float scale, uint64_t n_in, uint32_t n_fft, uint32_t hop,
                               uint32_t avg, int window, int mode, float norm, float* rows_out, uint64_t rows_cap, uint64_t* n_rows)
{
    if (!h) return WIFIRX_EINVAL;
    if (!n_rows) return fail(h, WIFIRX_EINVAL, "n_rows is required");
    if (n_in && !in) return fail(h, WIFIRX_EINVAL, "in is required");
    uint32_t bps;
    if (int rc = iq_check_format(h, fmt, scale, true, &bps)) return rc;
    if (window != WIFIRX_SPEC_RECT && window != WIFIRX_SPEC_HANN && window != WIFIRX_SPEC_BLACKMAN_HARRIS)
        return fail(h, WIFIRX_EINVAL, "window must be WIFIRX_SPEC_RECT, WIFIRX_SPEC_HANN or WIFIRX_SPEC_BLACKMAN_HARRIS");
    if (!spec_mode_ok(mode)) return fail(h, WIFIRX_EINVAL, "mode must be WIFIRX_SPEC_SUM or WIFIRX_SPEC_MAX");
    uint64_t rows, consumed;
    if (!spec_count(n_fft, hop, avg, n_in, &rows, &consumed))
        return fail(h, WIFIRX_EINVAL, "n_fft must be 64, 256, 1024 or 4096; hop and avg 1 .. 2^20");
    if (n_in >= SPEC_INDEX_LIMIT) return fail(h, WIFIRX_ERANGE, "n_in must stay below 2^62");
    if ((reinterpret_cast<uintptr_t>(in) & (bps - 1)) || (reinterpret_cast<uintptr_t>(rows_out) & 3))
        return fail(h, WIFIRX_EINVAL, "misaligned buffer (rows_out: 4 bytes; in: fc32 8, sc16 4, sc8 2)");
    if (rows && !rows_out) return fail(h, WIFIRX_EINVAL, "rows_out is required");
    if (rows > rows_cap) return fail(h, WIFIRX_ERANGE, "rows_cap is smaller than n_rows (wifirx_spectrum_count)");
    const uint64_t rows_per_tile = n_fft >= WR_SPEC_TILE ? 1 : WR_SPEC_TILE / n_fft;
    if ((rows + rows_per_tile - 1) / rows_per_tile > 0x7fffffffull) return fail(h, WIFIRX_ERANGE, "too many rows for one call");
    if (ranges_overlap(in, n_in * bps, rows_out, rows * n_fft * 4)) return fail(h, WIFIRX_EINVAL, "in and rows_out must not overlap");
    *n_rows = rows;
    if (rows == 0) return WIFIRX_OK;
    stream_worker_wait_idle(h);
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, wr_launch_spectrum(h->stream, in, fmt, scale, n_fft, hop, avg, window, mode, norm, rows_out, rows));
    return WIFIRX_OK;
}

extern "C" int wifirx_spectrum_fold(wifirx_handle* h, const float* rows, uint64_t n_rows, uint32_t n_fft, uint64_t group, int mode,
                                    float* out, uint64_t out_cap, uint64_t* n_out)
{
    if (!h) return WIFIRX_EINVAL;
    if (!n_out) return fail(h, WIFIRX_EINVAL, "n_out is required");
    if (!spec_n_ok(n_fft)) return fail(h, WIFIRX_EINVAL, "n_fft must be 64, 256, 1024 or 4096");
    if (!spec_mode_ok(mode)) return fail(h, WIFIRX_EINVAL, "mode must be WIFIRX_SPEC_SUM or WIFIRX_SPEC_MAX");
    if (group < 1) return fail(h, WIFIRX_EINVAL, "group must be at least 1");
    if (n_rows >= SPEC_ROWS_LIMIT) return fail(h, WIFIRX_ERANGE, "n_rows must stay below 2^40");
    const uint64_t made = n_rows / group;
    if (made && (!rows || !out)) return fail(h, WIFIRX_EINVAL, "rows and out are required");
    if ((reinterpret_cast<uintptr_t>(rows) & 3) || (reinterpret_cast<uintptr_t>(out) & 3))
        return fail(h, WIFIRX_EINVAL, "misaligned buffer (rows, out: 4 bytes)");
    if (made > out_cap) return fail(h, WIFIRX_ERANGE, "out_cap is smaller than n_out = n_rows / group");
    if (ranges_overlap(rows, made * group * n_fft * 4, out, made * n_fft * 4)) return fail(h, WIFIRX_EINVAL, "rows and out must not overlap");
    *n_out = made;
    if (made == 0) return WIFIRX_OK;
    stream_worker_wait_idle(h);
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, wr_launch_spectrum_fold(h->stream, rows, n_fft, group, mode, out, made));
    return WIFIRX_OK;
}

extern "C" int wifirx_spectrum_bands(wifirx_handle* h, const float* rows, uint64_t n_rows, uint32_t n_fft, uint32_t n_bands,
                                     const uint32_t* lo, const uint32_t* hi, float* out)
{
    if (!h) return WIFIRX_EINVAL;
    if (!rows || !out || !lo || !hi) return fail(h, WIFIRX_EINVAL, "rows, out, lo and hi are required");
    if (!spec_n_ok(n_fft)) return fail(h, WIFIRX_EINVAL, "n_fft must be 64, 256, 1024 or 4096");
    if (n_bands < 1 || n_bands > WIFIRX_SPEC_MAX_BANDS) return fail(h, WIFIRX_EINVAL, "n_bands must be 1 .. 16");
    wr_spec_bands b = {};
    for (uint32_t k = 0; k < n_bands; k++) {
        if (lo[k] >= hi[k] || hi[k] > n_fft) return fail(h, WIFIRX_EINVAL, "a band must hold lo < hi <= n_fft");
        b.lo[k] = lo[k];
        b.hi[k] = hi[k];
    }
    if ((reinterpret_cast<uintptr_t>(rows) & 3) || (reinterpret_cast<uintptr_t>(out) & 3))
        return fail(h, WIFIRX_EINVAL, "misaligned buffer (rows, out: 4 bytes)");
    if (n_rows > 0x7fffffffull) return fail(h, WIFIRX_ERANGE, "n_rows must stay below 2^31");
    if (ranges_overlap(rows, n_rows * n_fft * 4, out, n_rows * n_bands * 4)) return fail(h, WIFIRX_EINVAL, "rows and out must not overlap");
    if (n_rows == 0) return WIFIRX_OK;
    stream_worker_wait_idle(h);
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, wr_launch_spectrum_bands(h->stream, rows, n_rows, n_fft, n_bands, &b, out));
    return WIFIRX_OK;
}
