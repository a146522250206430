// channel entry points: channels.channel_model over rows of device samples (wr_channel.hip)

// the arguments of wifirx_channel_fading, the widest entry point, in its order (sro == NULL: drift0 is not looked at;
// doppler == NULL: k_factor, fade_seed and time0 are not looked at)
struct ChanCall {
    const float* in; float* out; uint64_t samples_cap; const uint64_t* row_off; uint64_t row_len; uint32_t n_rows;
    const float* taps; int taps_on_device; uint32_t n_taps, n_tap_sets; const float* cfo; uint64_t phase0; const float* sro;
    int64_t drift0; float gain, noise_voltage; uint64_t seed, sample0; const float* doppler; float k_factor; uint64_t fade_seed, time0;
};

// the argument checks; n_rows == 0 ends them, and the call, with WIFIRX_OK
static int channel_check(wifirx_handle* h, const ChanCall& c)
{
    if (!c.in || !c.out || !c.taps) return fail(h, WIFIRX_EINVAL, "in, out and taps are required");
    if ((reinterpret_cast<uintptr_t>(c.in) | reinterpret_cast<uintptr_t>(c.out)) & 7)
        return fail(h, WIFIRX_EINVAL, "in and out must be 8-byte aligned (complex64)");
    if (c.taps_on_device && (reinterpret_cast<uintptr_t>(c.taps) & 7)) return fail(h, WIFIRX_EINVAL, "device taps must be 8-byte aligned");
    if (c.n_taps < 1 || c.n_taps > 64) return fail(h, WIFIRX_EINVAL, "n_taps must be 1..64");
    if (c.n_tap_sets == 0) return fail(h, WIFIRX_EINVAL, "n_tap_sets must be >= 1");
    if (!std::isfinite(c.gain) || !std::isfinite(c.noise_voltage)) return fail(h, WIFIRX_EINVAL, "gain and noise_voltage must be finite");
    if (c.n_rows == 0) return WIFIRX_OK;
    if (c.cfo)
        for (uint32_t r = 0; r < c.n_rows; r++)
            if (!std::isfinite(c.cfo[r])) return fail(h, WIFIRX_EINVAL, "cfo must be finite");
    if (c.sro)
        for (uint32_t r = 0; r < c.n_rows; r++)
            if (!(std::fabs(c.sro[r]) <= 0x1p-8f)) return fail(h, WIFIRX_EINVAL, "sro must be finite and at most 2^-8 in magnitude");
    if (c.sro && c.in == c.out) return fail(h, WIFIRX_EINVAL, "in place is not possible with a sample-rate offset");
    if (c.doppler) {
        // rule 19: the interpolation of the gains between grid points is good to sqrt(8) (2 pi fd 32)^2 / 8, 1.4e-2 at 2^-10
        for (uint32_t r = 0; r < c.n_rows; r++)
            if (!(c.doppler[r] >= 0.0f && c.doppler[r] <= 0x1p-10f))
                return fail(h, WIFIRX_EINVAL, "doppler must be finite, not negative and at most 2^-10 cycles per sample");
        if (!(std::isfinite(c.k_factor) && c.k_factor >= 0.0f)) return fail(h, WIFIRX_EINVAL, "k_factor must be finite and not negative");
        if (c.n_taps > wr_channel_fade_taps()) return fail(h, WIFIRX_EINVAL, "n_taps must be 1..16 with fading");
        if (c.in == c.out) return fail(h, WIFIRX_EINVAL, "in place is not possible with fading");
    }
    if (c.row_off)
        for (uint32_t r = 0; r < c.n_rows; r++)
            if (c.row_off[r + 1] < c.row_off[r]) return fail(h, WIFIRX_EINVAL, "row_off must not decrease");
    if (!c.row_off && c.row_len > c.samples_cap / c.n_rows) return fail(h, WIFIRX_ERANGE, "rows exceed samples_cap");
    const uint64_t g0 = c.row_off ? c.row_off[0] : 0;
    const uint64_t g1 = c.row_off ? c.row_off[c.n_rows] : c.row_len * c.n_rows;
    if (g1 > c.samples_cap) return fail(h, WIFIRX_ERANGE, "rows exceed samples_cap");
    if (g1 > g0) {
        const uintptr_t i0 = reinterpret_cast<uintptr_t>(c.in) + 8 * g0, i1 = reinterpret_cast<uintptr_t>(c.in) + 8 * g1;
        const uintptr_t o0 = reinterpret_cast<uintptr_t>(c.out) + 8 * g0, o1 = reinterpret_cast<uintptr_t>(c.out) + 8 * g1;
        if (i0 < o1 && o0 < i1 && !(c.n_taps == 1 && c.in == c.out))
            return fail(h, WIFIRX_EINVAL, "in and out overlap: only in == out with one tap is allowed");
    }
    return WIFIRX_OK;
}

// rule 18: dinc_r = llround(sro_r 2^40) (exact in double: a float32 times a power of two), |dinc| <= 2^32; the drift
// D(n) = drift0 + dinc n of every sample of every row must stay below 2^62 in magnitude
static int channel_drift(wifirx_handle* h, const ChanCall& c, std::vector<int64_t>& dinc)
{
    dinc.resize(c.n_rows);
    uint64_t longest = c.row_off ? 0 : c.row_len, worst = 0;
    for (uint32_t r = 0; r < c.n_rows; r++) {
        dinc[r] = std::llround((double)c.sro[r] * 0x1p40);
        worst = std::max<uint64_t>(worst, (uint64_t)std::llabs(dinc[r]));
        if (c.row_off) longest = std::max(longest, c.row_off[r + 1] - c.row_off[r]);
    }
    const unsigned __int128 reach = (unsigned __int128)(c.drift0 < 0 ? 0 - (uint64_t)c.drift0 : (uint64_t)c.drift0) +
                                    (unsigned __int128)worst * longest;
    if (reach >= ((unsigned __int128)1 << 62)) return fail(h, WIFIRX_ERANGE, "|drift0| + |dinc| * (longest row) must stay below 2^62");
    return WIFIRX_OK;
}

// tiles of a row: [a_r, row end) in steps of `tile`, a_r = the row start or the sample before it (pair alignment, a.shift).
// Returns their number; row_off form: tile_base = the first tile of every row, fixed rows: a.tiles_per_row
static uint64_t channel_tiles(const ChanCall& c, wr::ChanArgs& a, std::vector<uint64_t>& tile_base)
{
    const uint64_t tile = wr_channel_tile_samples();
    uint64_t n_tiles = 0;
    if (c.row_off) {
        tile_base.resize((size_t)c.n_rows + 1);
        for (uint32_t r = 0; r < c.n_rows; r++) {
            tile_base[r] = n_tiles;
            const uint64_t rs = c.row_off[r], re = c.row_off[r + 1];
            if (re > rs) n_tiles += (re - rs + ((rs + a.shift) & 1) + tile - 1) / tile;
        }
        tile_base[c.n_rows] = n_tiles;
    } else if (c.row_len) {
        const uint64_t d = (c.row_len & 1) ? 1 : (uint64_t)a.shift;
        a.tiles_per_row = (c.row_len + d + tile - 1) / tile;
        n_tiles = a.tiles_per_row * c.n_rows;
    }
    return n_tiles;
}

static int channel_call(wifirx_handle* h, const ChanCall& c)
{
    if (!h) return WIFIRX_EINVAL;
    int rc = channel_check(h, c);
    if (rc || c.n_rows == 0) return rc;
    std::vector<int64_t> dinc;
    if (c.sro && (rc = channel_drift(h, c, dinc))) return rc;
    wr::ChanArgs a{};
    a.shift = (int32_t)((reinterpret_cast<uintptr_t>(c.out) >> 3) & 1);
    std::vector<uint64_t> tile_base;
    const uint64_t n_tiles = channel_tiles(c, a, tile_base);
    if (n_tiles > 0x7fffffffull) return fail(h, WIFIRX_ERANGE, "more than 2^31 - 1 tiles of output");
    stream_worker_wait_idle(h);
    HIP_TRY(h, hipSetDevice(h->device));
    // one upload of what the host holds (the phase increments are derived on the device: wr_channel.hip): add() appends an
    // array to `meta` at 8-byte alignment and notes which device pointer of `a` is to name it once the copy has its place
    std::vector<uint8_t> meta;
    std::vector<std::pair<void*, size_t>> named;      // (the pointer to set, the offset of its array)
    auto add = [&](void* dev_ptr, const void* host, size_t bytes) {
        const size_t off = (meta.size() + 7) & ~(size_t)7;
        meta.resize(off + bytes);
        std::memcpy(meta.data() + off, host, bytes);
        named.emplace_back(dev_ptr, off);
    };
    a.taps = reinterpret_cast<const float2*>(c.taps);
    if (!c.taps_on_device) add(&a.taps, c.taps, 8ull * c.n_taps * c.n_tap_sets);
    if (c.cfo) add(&a.cfo, c.cfo, 4ull * c.n_rows);
    if (c.row_off) add(&a.row_off, c.row_off, 8ull * (c.n_rows + 1));
    if (c.row_off) add(&a.tile_base, tile_base.data(), 8ull * (c.n_rows + 1));
    if (c.sro) add(&a.dinc, dinc.data(), 8ull * c.n_rows);
    if (c.doppler) add(&a.doppler, c.doppler, 4ull * c.n_rows);
    if (const size_t meta_bytes = meta.size()) {
        if ((rc = h->stage.ch_meta.reserve(h, meta_bytes))) return rc;
        HIP_TRY(h, hipMemcpyAsync(h->stage.ch_meta.p, meta.data(), meta_bytes, hipMemcpyHostToDevice, h->stream));
        // the host arrays (the caller's and `meta`) may go once this returns: wait for the copy, not for the kernel
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        for (const auto& n : named) {
            const uint8_t* dev = h->stage.ch_meta.as<uint8_t>() + n.second;
            std::memcpy(n.first, &dev, sizeof dev);      // (every one is an object pointer: one representation)
        }
    }
    a.in = reinterpret_cast<const float2*>(c.in);
    a.out = reinterpret_cast<float2*>(c.out);
    a.row_len = c.row_len;
    a.phase0 = c.phase0;
    a.seed = c.seed;
    a.sample0 = c.sample0;
    a.n_rows = c.n_rows;
    a.n_taps = c.n_taps;
    a.n_tap_sets = c.n_tap_sets;
    a.gain = c.gain;
    a.noise = c.noise_voltage;
    a.drift0 = c.sro ? c.drift0 : 0;
    if (c.doppler) {
        a.fade_seed = c.fade_seed;
        a.time0 = c.time0;
        if (c.k_factor > 0.0f) {                    // formed in double; k_factor = 0: neither is applied (a_los = 0 says so)
            a.a_los = (float)std::sqrt((double)c.k_factor / ((double)c.k_factor + 1.0));
            a.a_nlos = (float)std::sqrt(1.0 / ((double)c.k_factor + 1.0));
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
    return channel_call(h, {in, out, samples_cap, row_off, row_len, n_rows, taps, taps_on_device, n_taps, n_tap_sets, cfo, phase0,
                            nullptr, 0, gain, noise_voltage, seed, sample0, nullptr, 0.0f, 0, 0});
}

extern "C" int wifirx_channel_sro(wifirx_handle* h, const float* in, float* out, uint64_t samples_cap,
                                  const uint64_t* row_off, uint64_t row_len, uint32_t n_rows,
                                  const float* taps, int taps_on_device, uint32_t n_taps, uint32_t n_tap_sets,
                                  const float* cfo, uint64_t phase0, const float* sro, int64_t drift0,
                                  float gain, float noise_voltage, uint64_t seed, uint64_t sample0)
{
    return channel_call(h, {in, out, samples_cap, row_off, row_len, n_rows, taps, taps_on_device, n_taps, n_tap_sets, cfo, phase0,
                            sro, drift0, gain, noise_voltage, seed, sample0, nullptr, 0.0f, 0, 0});
}

extern "C" int wifirx_channel_fading(wifirx_handle* h, const float* in, float* out, uint64_t samples_cap,
                                     const uint64_t* row_off, uint64_t row_len, uint32_t n_rows,
                                     const float* taps, int taps_on_device, uint32_t n_taps, uint32_t n_tap_sets,
                                     const float* cfo, uint64_t phase0, const float* sro, int64_t drift0,
                                     float gain, float noise_voltage, uint64_t seed, uint64_t sample0,
                                     const float* doppler, float k_factor, uint64_t fade_seed, uint64_t time0)
{
    return channel_call(h, {in, out, samples_cap, row_off, row_len, n_rows, taps, taps_on_device, n_taps, n_tap_sets, cfo, phase0,
                            sro, drift0, gain, noise_voltage, seed, sample0, doppler, k_factor, fade_seed, time0});
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
