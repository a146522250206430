// channel entry points: channels.channel_model over rows of device samples (wr_channel.hip)

// wifirx_channel (sro == NULL: drift0 is not looked at), wifirx_channel_sro and wifirx_channel_fading (doppler == NULL:
// k_factor, fade_seed and time0 are not looked at)
static int channel_call(wifirx_handle* h, const float* in, float* out, uint64_t samples_cap,
                        const uint64_t* row_off, uint64_t row_len, uint32_t n_rows,
                        const float* taps, int taps_on_device, uint32_t n_taps, uint32_t n_tap_sets,
                        const float* cfo, uint64_t phase0, const float* sro, int64_t drift0, float gain, float noise_voltage,
                        uint64_t seed, uint64_t sample0,
                        const float* doppler = nullptr, float k_factor = 0.0f, uint64_t fade_seed = 0, uint64_t time0 = 0)
{
    if (!h) return WIFIRX_EINVAL;
    if (!in || !out || !taps) return fail(h, WIFIRX_EINVAL, "in, out and taps are required");
    if ((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out)) & 7)
        return fail(h, WIFIRX_EINVAL, "in and out must be 8-byte aligned (complex64)");
    if (taps_on_device && (reinterpret_cast<uintptr_t>(taps) & 7)) return fail(h, WIFIRX_EINVAL, "device taps must be 8-byte aligned");
    if (n_taps < 1 || n_taps > 64) return fail(h, WIFIRX_EINVAL, "n_taps must be 1..64");
    if (n_tap_sets == 0) return fail(h, WIFIRX_EINVAL, "n_tap_sets must be >= 1");
    if (!std::isfinite(gain) || !std::isfinite(noise_voltage)) return fail(h, WIFIRX_EINVAL, "gain and noise_voltage must be finite");
    if (n_rows == 0) return WIFIRX_OK;
    if (cfo)
        for (uint32_t r = 0; r < n_rows; r++)
            if (!std::isfinite(cfo[r])) return fail(h, WIFIRX_EINVAL, "cfo must be finite");
    if (sro)
        for (uint32_t r = 0; r < n_rows; r++)
            if (!(std::fabs(sro[r]) <= 0x1p-8f)) return fail(h, WIFIRX_EINVAL, "sro must be finite and at most 2^-8 in magnitude");
    if (sro && in == out) return fail(h, WIFIRX_EINVAL, "in place is not possible with a sample-rate offset");
    if (doppler) {
        // rule 19: the interpolation of the gains between grid points is good to sqrt(8) (2 pi fd 32)^2 / 8, 1.4e-2 at 2^-10
        for (uint32_t r = 0; r < n_rows; r++)
            if (!(doppler[r] >= 0.0f && doppler[r] <= 0x1p-10f))
                return fail(h, WIFIRX_EINVAL, "doppler must be finite, not negative and at most 2^-10 cycles per sample");
        if (!(std::isfinite(k_factor) && k_factor >= 0.0f)) return fail(h, WIFIRX_EINVAL, "k_factor must be finite and not negative");
        if (n_taps > wr_channel_fade_taps()) return fail(h, WIFIRX_EINVAL, "n_taps must be 1..16 with fading");
        if (in == out) return fail(h, WIFIRX_EINVAL, "in place is not possible with fading");
    }
    if (row_off)
        for (uint32_t r = 0; r < n_rows; r++)
            if (row_off[r + 1] < row_off[r]) return fail(h, WIFIRX_EINVAL, "row_off must not decrease");
    if (!row_off && row_len > samples_cap / n_rows) return fail(h, WIFIRX_ERANGE, "rows exceed samples_cap");
    const uint64_t g0 = row_off ? row_off[0] : 0;
    const uint64_t g1 = row_off ? row_off[n_rows] : row_len * n_rows;
    if (g1 > samples_cap) return fail(h, WIFIRX_ERANGE, "rows exceed samples_cap");
    if (g1 > g0) {
        const uintptr_t i0 = reinterpret_cast<uintptr_t>(in) + 8 * g0, i1 = reinterpret_cast<uintptr_t>(in) + 8 * g1;
        const uintptr_t o0 = reinterpret_cast<uintptr_t>(out) + 8 * g0, o1 = reinterpret_cast<uintptr_t>(out) + 8 * g1;
        if (i0 < o1 && o0 < i1 && !(n_taps == 1 && in == out))
            return fail(h, WIFIRX_EINVAL, "in and out overlap: only in == out with one tap is allowed");
    }
    // rule 18: dinc_r = llround(sro_r 2^40) (exact in double: a float32 times a power of two), |dinc| <= 2^32; the drift
    // D(n) = drift0 + dinc n of every sample of every row must stay below 2^62 in magnitude
    std::vector<int64_t> dinc;
    if (sro) {
        dinc.resize(n_rows);
        uint64_t longest = row_off ? 0 : row_len, worst = 0;
        for (uint32_t r = 0; r < n_rows; r++) {
            dinc[r] = std::llround((double)sro[r] * 0x1p40);
            worst = std::max<uint64_t>(worst, (uint64_t)std::llabs(dinc[r]));
            if (row_off) longest = std::max(longest, row_off[r + 1] - row_off[r]);
        }
        const unsigned __int128 reach = (unsigned __int128)(drift0 < 0 ? 0 - (uint64_t)drift0 : (uint64_t)drift0) +
                                        (unsigned __int128)worst * longest;
        if (reach >= ((unsigned __int128)1 << 62)) return fail(h, WIFIRX_ERANGE, "|drift0| + |dinc| * (longest row) must stay below 2^62");
    }

    wr::ChanArgs a{};
    a.shift = (int32_t)((reinterpret_cast<uintptr_t>(out) >> 3) & 1);
    const uint64_t tile = wr_channel_tile_samples();
    // tiles of a row: [a_r, row end) in steps of `tile`, a_r = the row start or the sample before it (pair alignment)
    uint64_t n_tiles = 0;
    std::vector<uint64_t> tile_base;
    if (row_off) {
        tile_base.resize((size_t)n_rows + 1);
        for (uint32_t r = 0; r < n_rows; r++) {
            tile_base[r] = n_tiles;
            const uint64_t rs = row_off[r], re = row_off[r + 1];
            if (re > rs) n_tiles += (re - rs + ((rs + a.shift) & 1) + tile - 1) / tile;
        }
        tile_base[n_rows] = n_tiles;
    } else if (row_len) {
        const uint64_t d = (row_len & 1) ? 1 : (uint64_t)a.shift;
        a.tiles_per_row = (row_len + d + tile - 1) / tile;
        n_tiles = a.tiles_per_row * n_rows;
    }
    if (n_tiles > 0x7fffffffull) return fail(h, WIFIRX_ERANGE, "more than 2^31 - 1 tiles of output");
    stream_worker_wait_idle(h);
    HIP_TRY(h, hipSetDevice(h->device));

    // one upload of what the host holds: taps | cfo | row offsets | tile bases (row_off form) | drift increments (sro) |
    // Doppler (fading)
    const size_t taps_bytes = 8ull * n_taps * n_tap_sets;
    const size_t o_taps = 0, o_cfo = o_taps + (taps_on_device ? 0 : taps_bytes);
    const size_t o_row = o_cfo + (cfo ? (4ull * n_rows + 7) & ~7ull : 0);
    const size_t o_tile = o_row + (row_off ? 8ull * (n_rows + 1) : 0);
    const size_t o_dinc = o_tile + (row_off ? 8ull * (n_rows + 1) : 0);
    const size_t o_dop = o_dinc + (sro ? 8ull * n_rows : 0);
    const size_t meta_bytes = o_dop + (doppler ? 4ull * n_rows : 0);
    uint8_t* dm = nullptr;
    if (meta_bytes) {
        std::vector<uint8_t> meta(meta_bytes);      // (the phase increments are derived on the device: wr_channel.hip)
        if (!taps_on_device) std::memcpy(meta.data() + o_taps, taps, taps_bytes);
        if (cfo) std::memcpy(meta.data() + o_cfo, cfo, 4ull * n_rows);
        if (row_off) {
            std::memcpy(meta.data() + o_row, row_off, 8ull * (n_rows + 1));
            std::memcpy(meta.data() + o_tile, tile_base.data(), 8ull * (n_rows + 1));
        }
        if (sro) std::memcpy(meta.data() + o_dinc, dinc.data(), 8ull * n_rows);
        if (doppler) std::memcpy(meta.data() + o_dop, doppler, 4ull * n_rows);
        int rc = h->stage.ch_meta.reserve(h, meta_bytes);
        if (rc) return rc;
        HIP_TRY(h, hipMemcpyAsync(h->stage.ch_meta.p, meta.data(), meta_bytes, hipMemcpyHostToDevice, h->stream));
        // the host arrays (the caller's and `meta`) may go once this returns: wait for the copy, not for the kernel
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        dm = h->stage.ch_meta.as<uint8_t>();
    }

    a.in = reinterpret_cast<const float2*>(in);
    a.out = reinterpret_cast<float2*>(out);
    a.taps = taps_on_device ? reinterpret_cast<const float2*>(taps) : reinterpret_cast<const float2*>(dm + o_taps);
    a.cfo = cfo ? reinterpret_cast<const float*>(dm + o_cfo) : nullptr;
    a.row_off = row_off ? reinterpret_cast<const uint64_t*>(dm + o_row) : nullptr;
    a.tile_base = row_off ? reinterpret_cast<const uint64_t*>(dm + o_tile) : nullptr;
    a.row_len = row_len;
    a.phase0 = phase0;
    a.seed = seed;
    a.sample0 = sample0;
    a.n_rows = n_rows;
    a.n_taps = n_taps;
    a.n_tap_sets = n_tap_sets;
    a.gain = gain;
    a.noise = noise_voltage;
    a.dinc = sro ? reinterpret_cast<const int64_t*>(dm + o_dinc) : nullptr;
    a.drift0 = sro ? drift0 : 0;
    if (doppler) {
        a.doppler = reinterpret_cast<const float*>(dm + o_dop);
        a.fade_seed = fade_seed;
        a.time0 = time0;
        if (k_factor > 0.0f) {                      // formed in double; k_factor = 0: neither is applied (a_los = 0 says so)
            a.a_los = (float)std::sqrt((double)k_factor / ((double)k_factor + 1.0));
            a.a_nlos = (float)std::sqrt(1.0 / ((double)k_factor + 1.0));
        }
    }
    HIP_TRY(h, wr_launch_channel(h->stream, &a, n_tiles));
    return WIFIRX_OK;
}

extern "C" int wifirx_channel(wifirx_handle* h, const float* in, float* out, uint64_t samples_cap,
                              const uint64_t* row_off, uint64_t row_len, uint32_t n_rows,
                              const float* taps, int taps_on_device, uint32_t n_taps, uint32_t n_tap_sets,
                              const float* cfo, uint64_t phase0, float gain, float noise_voltage,
                              uint64_t seed, uint64_t sample0)
{
    return channel_call(h, in, out, samples_cap, row_off, row_len, n_rows, taps, taps_on_device, n_taps, n_tap_sets, cfo, phase0,
                        nullptr, 0, gain, noise_voltage, seed, sample0);
}

extern "C" int wifirx_channel_sro(wifirx_handle* h, const float* in, float* out, uint64_t samples_cap,
                                  const uint64_t* row_off, uint64_t row_len, uint32_t n_rows,
                                  const float* taps, int taps_on_device, uint32_t n_taps, uint32_t n_tap_sets,
                                  const float* cfo, uint64_t phase0, const float* sro, int64_t drift0,
                                  float gain, float noise_voltage, uint64_t seed, uint64_t sample0)
{
    return channel_call(h, in, out, samples_cap, row_off, row_len, n_rows, taps, taps_on_device, n_taps, n_tap_sets, cfo, phase0,
                        sro, drift0, gain, noise_voltage, seed, sample0);
}

extern "C" int wifirx_channel_fading(wifirx_handle* h, const float* in, float* out, uint64_t samples_cap,
                                     const uint64_t* row_off, uint64_t row_len, uint32_t n_rows,
                                     const float* taps, int taps_on_device, uint32_t n_taps, uint32_t n_tap_sets,
                                     const float* cfo, uint64_t phase0, const float* sro, int64_t drift0,
                                     float gain, float noise_voltage, uint64_t seed, uint64_t sample0,
                                     const float* doppler, float k_factor, uint64_t fade_seed, uint64_t time0)
{
    return channel_call(h, in, out, samples_cap, row_off, row_len, n_rows, taps, taps_on_device, n_taps, n_tap_sets, cfo, phase0,
                        sro, drift0, gain, noise_voltage, seed, sample0, doppler, k_factor, fade_seed, time0);
}

extern "C" int wifirx_resampler_table(const float** taps, uint32_t* n_phases, uint32_t* n_taps)
{
    uint32_t phases, width;
    const float* table = wr_resample_table(&phases, &width);
    if (taps) *taps = table;
    if (n_phases) *n_phases = phases;
    if (n_taps) *n_taps = width;
    return WIFIRX_OK;
}
