// IRS entry point: the tap sets of a reflecting surface's cascade channel, made on the device (wr_irs.hip, NUMERICS.md rule 25)

extern "C" int wifirx_irs_taps(wifirx_handle* h, float* taps_out, uint32_t n_sets, uint32_t n_taps, const float* pdp, float gain,
                               uint32_t n_elems, const float* los_b2r, const float* los_r2u, const float* los_b2u,
                               float k_factor, float direct_gain,
                               const float* psi, int psi_on_device, uint32_t n_psi_sets, uint32_t align_bits,
                               const float* scatter, uint32_t n_scatter, uint64_t irs_seed,
                               float* elems_out, uint8_t* codes_out)
{
    if (!h) return WIFIRX_EINVAL;
    // ---- the argument checks, before anything is queued ----
    if (!taps_out || !pdp || !los_b2r || !los_r2u) return fail(h, WIFIRX_EINVAL, "taps_out, pdp, los_b2r and los_r2u are required");
    if (n_elems < 1 || n_elems > wr_irs_max_elems()) return fail(h, WIFIRX_EINVAL, "n_elems must be 1..4096");
    if (n_taps < 1 || n_taps > wr_irs_max_taps()) return fail(h, WIFIRX_EINVAL, "n_taps must be 1..16");
    if (align_bits > 3) return fail(h, WIFIRX_EINVAL, "align_bits must be 0..3");
    if (!std::isfinite(gain) || !std::isfinite(direct_gain)) return fail(h, WIFIRX_EINVAL, "gain and direct_gain must be finite");
    if (!(std::isfinite(k_factor) && k_factor >= 0.0f)) return fail(h, WIFIRX_EINVAL, "k_factor must be finite and not negative");
    if (direct_gain != 0.0f && !los_b2u) return fail(h, WIFIRX_EINVAL, "los_b2u is required with a direct path");
    if (align_bits == 0 && !psi) return fail(h, WIFIRX_EINVAL, "psi is required when align_bits is 0");
    if (align_bits == 0 && n_psi_sets == 0) return fail(h, WIFIRX_EINVAL, "n_psi_sets must be >= 1 when align_bits is 0");
    if (align_bits == 0 && codes_out) return fail(h, WIFIRX_EINVAL, "codes_out needs align_bits 1..3");
    if (scatter && n_scatter == 0) return fail(h, WIFIRX_EINVAL, "n_scatter must be >= 1 with scatter");
    const auto addr = [](const void* p) { return reinterpret_cast<uintptr_t>(p); };
    const bool psi_read = align_bits == 0;
    if ((addr(taps_out) | addr(scatter) | addr(elems_out) | (psi_read && psi_on_device ? addr(psi) : 0)) & 7)
        return fail(h, WIFIRX_EINVAL, "taps_out, scatter, elems_out and device psi must be 8-byte aligned (complex64)");
    if ((addr(pdp) | addr(los_b2r) | addr(los_r2u) | addr(los_b2u) | (psi_read && !psi_on_device ? addr(psi) : 0)) & 3)
        return fail(h, WIFIRX_EINVAL, "the host arrays must be 4-byte aligned (float32)");
    for (uint32_t l = 0; l < n_taps; l++)
        if (!(std::isfinite(pdp[l]) && pdp[l] >= 0.0f)) return fail(h, WIFIRX_EINVAL, "pdp must be finite and not negative");
    if (n_sets == 0) return WIFIRX_OK;
    if (n_sets > 0x7fffffffu) return fail(h, WIFIRX_ERANGE, "more than 2^31 - 1 tap sets");
    const bool host_psi = psi_read && !psi_on_device;
    if (host_psi && (uint64_t)n_psi_sets * n_elems * 8 > (1ull << 31)) return fail(h, WIFIRX_ERANGE, "host psi above 2 GiB");

    stream_worker_wait_idle(h);
    HIP_TRY(h, hipSetDevice(h->device));
    wr::IrsArgs a{};
    // one upload of what the host holds, as channel_call does it: add() appends an array to `meta` at 8-byte alignment and
    // notes which device pointer of `a` is to name it once the copy has its place
    std::vector<uint8_t> meta;
    std::vector<std::pair<void*, size_t>> named;
    auto add = [&](void* dev_ptr, const void* host, size_t bytes) {
        const size_t off = (meta.size() + 7) & ~(size_t)7;
        meta.resize(off + bytes);
        std::memcpy(meta.data() + off, host, bytes);
        named.emplace_back(dev_ptr, off);
    };
    std::vector<float> scale(n_taps);                  // s_l = (float)(sqrt(pdp_l) gain), formed in double
    for (uint32_t l = 0; l < n_taps; l++) scale[l] = (float)(std::sqrt((double)pdp[l]) * (double)gain);
    add(&a.los_a, los_b2r, 8ull * n_elems);
    add(&a.los_b, los_r2u, 8ull * n_elems);
    add(&a.scale, scale.data(), 4ull * n_taps);
    a.psi = reinterpret_cast<const float2*>(psi);
    if (host_psi) add(&a.psi, psi, 8ull * n_psi_sets * n_elems);
    int rc;
    if ((rc = h->stage.irs_meta.reserve(h, meta.size()))) return rc;
    HIP_TRY(h, hipMemcpyAsync(h->stage.irs_meta.p, meta.data(), meta.size(), hipMemcpyHostToDevice, h->stream));
    // the host arrays (the caller's and `meta`) may go once this returns: wait for the copy, not for the kernel
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    for (const auto& n : named) {
        const uint8_t* dev = h->stage.irs_meta.as<uint8_t>() + n.second;
        std::memcpy(n.first, &dev, sizeof dev);
    }
    a.taps_out = reinterpret_cast<float2*>(taps_out);
    a.scatter = reinterpret_cast<const float2*>(scatter);
    a.elems_out = reinterpret_cast<float2*>(elems_out);
    a.codes_out = codes_out;
    if (direct_gain != 0.0f) a.los_d = make_float2(los_b2u[0], los_b2u[1]);
    a.seed = irs_seed;
    a.n_sets = n_sets;
    a.n_taps = n_taps;
    a.n_elems = n_elems;
    a.n_psi_sets = psi_read ? n_psi_sets : 1;
    a.n_scatter = scatter ? n_scatter : 1;
    a.align_bits = align_bits;
    if (k_factor > 0.0f) {                              // formed in double; k_factor = 0: neither is applied (a_los = 0 says so)
        a.a_los = (float)std::sqrt((double)k_factor / ((double)k_factor + 1.0));
        a.a_nlos = (float)std::sqrt(1.0 / ((double)k_factor + 1.0));
    }
    a.direct_gain = direct_gain;
    HIP_TRY(h, wr_launch_irs(h->stream, &a));
    return WIFIRX_OK;
}

// beam training over a codebook: the same scene, K configurations, the best one per set (wr_irs_sweep.hip, NUMERICS.md rule 26)
extern "C" int wifirx_irs_sweep(wifirx_handle* h, float* taps_out, uint32_t n_sets, uint32_t n_taps, const float* pdp, float gain,
                                uint32_t n_elems, const float* los_b2r, const float* los_r2u, const float* los_b2u,
                                float k_factor, float direct_gain,
                                const float* codebook, int codebook_on_device, uint32_t n_codes,
                                const float* scatter, uint32_t n_scatter, uint64_t irs_seed,
                                uint16_t* best_out, float* power_out)
{
    if (!h) return WIFIRX_EINVAL;
    // ---- the argument checks, before anything is queued ----
    if (!pdp || !los_b2r || !los_r2u || !codebook) return fail(h, WIFIRX_EINVAL, "pdp, los_b2r, los_r2u and codebook are required");
    if (!taps_out && !best_out && !power_out) return fail(h, WIFIRX_EINVAL, "one of taps_out, best_out and power_out is required");
    if (n_elems < 1 || n_elems > wr_irs_max_elems()) return fail(h, WIFIRX_EINVAL, "n_elems must be 1..4096");
    if (n_taps < 1 || n_taps > wr_irs_max_taps()) return fail(h, WIFIRX_EINVAL, "n_taps must be 1..16");
    if (n_codes < 1 || n_codes > wr_irs_max_codes()) return fail(h, WIFIRX_EINVAL, "n_codes must be 1..1024");
    if (!std::isfinite(gain) || !std::isfinite(direct_gain)) return fail(h, WIFIRX_EINVAL, "gain and direct_gain must be finite");
    if (!(std::isfinite(k_factor) && k_factor >= 0.0f)) return fail(h, WIFIRX_EINVAL, "k_factor must be finite and not negative");
    if (direct_gain != 0.0f && !los_b2u) return fail(h, WIFIRX_EINVAL, "los_b2u is required with a direct path");
    if (scatter && n_scatter == 0) return fail(h, WIFIRX_EINVAL, "n_scatter must be >= 1 with scatter");
    const auto addr = [](const void* p) { return reinterpret_cast<uintptr_t>(p); };
    if ((addr(taps_out) | addr(scatter) | (codebook_on_device ? addr(codebook) : 0)) & 7)
        return fail(h, WIFIRX_EINVAL, "taps_out, scatter and a device codebook must be 8-byte aligned (complex64)");
    if ((addr(pdp) | addr(los_b2r) | addr(los_r2u) | addr(los_b2u) | addr(power_out) | (codebook_on_device ? 0 : addr(codebook))) & 3)
        return fail(h, WIFIRX_EINVAL, "the host arrays and power_out must be 4-byte aligned (float32)");
    if (addr(best_out) & 1) return fail(h, WIFIRX_EINVAL, "best_out must be 2-byte aligned (uint16)");
    for (uint32_t l = 0; l < n_taps; l++)
        if (!(std::isfinite(pdp[l]) && pdp[l] >= 0.0f)) return fail(h, WIFIRX_EINVAL, "pdp must be finite and not negative");
    if (n_sets == 0) return WIFIRX_OK;
    if (n_sets > 0x7fffffffu) return fail(h, WIFIRX_ERANGE, "more than 2^31 - 1 tap sets");

    stream_worker_wait_idle(h);
    HIP_TRY(h, hipSetDevice(h->device));
    wr::IrsSweepArgs a{};
    // one upload of what the host holds, as wifirx_irs_taps does it
    std::vector<uint8_t> meta;
    std::vector<std::pair<void*, size_t>> named;
    auto add = [&](void* dev_ptr, const void* host, size_t bytes) {
        const size_t off = (meta.size() + 7) & ~(size_t)7;
        meta.resize(off + bytes);
        std::memcpy(meta.data() + off, host, bytes);
        named.emplace_back(dev_ptr, off);
    };
    std::vector<float> scale(n_taps);                  // s_l = (float)(sqrt(pdp_l) gain), formed in double
    for (uint32_t l = 0; l < n_taps; l++) scale[l] = (float)(std::sqrt((double)pdp[l]) * (double)gain);
    add(&a.s.los_a, los_b2r, 8ull * n_elems);
    add(&a.s.los_b, los_r2u, 8ull * n_elems);
    add(&a.s.scale, scale.data(), 4ull * n_taps);
    a.codebook = reinterpret_cast<const float2*>(codebook);
    if (!codebook_on_device) add(&a.codebook, codebook, 8ull * n_codes * n_elems);
    int rc;
    if ((rc = h->stage.irs_meta.reserve(h, meta.size()))) return rc;
    HIP_TRY(h, hipMemcpyAsync(h->stage.irs_meta.p, meta.data(), meta.size(), hipMemcpyHostToDevice, h->stream));
    // the host arrays (the caller's and `meta`) may go once this returns: wait for the copy, not for the kernel
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    for (const auto& n : named) {
        const uint8_t* dev = h->stage.irs_meta.as<uint8_t>() + n.second;
        std::memcpy(n.first, &dev, sizeof dev);
    }
    a.s.taps_out = reinterpret_cast<float2*>(taps_out);
    a.s.scatter = reinterpret_cast<const float2*>(scatter);
    if (direct_gain != 0.0f) a.s.los_d = make_float2(los_b2u[0], los_b2u[1]);
    a.s.seed = irs_seed;
    a.s.n_sets = n_sets;
    a.s.n_taps = n_taps;
    a.s.n_elems = n_elems;
    a.s.n_psi_sets = 1;
    a.s.n_scatter = scatter ? n_scatter : 1;
    if (k_factor > 0.0f) {                              // formed in double; k_factor = 0: neither is applied (a_los = 0 says so)
        a.s.a_los = (float)std::sqrt((double)k_factor / ((double)k_factor + 1.0));
        a.s.a_nlos = (float)std::sqrt(1.0 / ((double)k_factor + 1.0));
    }
    a.s.direct_gain = direct_gain;
    a.best_out = best_out;
    a.power_out = power_out;
    a.n_codes = n_codes;
    HIP_TRY(h, wr_launch_irs_sweep(h->stream, &a));
    return WIFIRX_OK;
}

// ---- the surface behind an AP of n_ant antennas (wr_irs_multi.hip, NUMERICS.md rules 27 and 28) ----

// the checks of the scene that wifirx_irs_taps_multi and wifirx_irs_sweep_multi share, in wifirx_irs_taps' order and words
static int irs_multi_check(wifirx_handle* h, uint32_t n_ant, uint32_t n_taps, const float* pdp, float gain, uint32_t n_elems,
                           const float* los_b2u, float k_factor, float direct_gain, const float* scatter, uint32_t n_scatter)
{
    if (n_ant < 1 || n_ant > wr_irs_max_ant()) return fail(h, WIFIRX_EINVAL, "n_ant must be 1..8");
    if (n_elems < 1 || n_elems > wr_irs_max_elems()) return fail(h, WIFIRX_EINVAL, "n_elems must be 1..4096");
    if (n_taps < 1 || n_taps > wr_irs_max_taps()) return fail(h, WIFIRX_EINVAL, "n_taps must be 1..16");
    if (!std::isfinite(gain) || !std::isfinite(direct_gain)) return fail(h, WIFIRX_EINVAL, "gain and direct_gain must be finite");
    if (!(std::isfinite(k_factor) && k_factor >= 0.0f)) return fail(h, WIFIRX_EINVAL, "k_factor must be finite and not negative");
    if (direct_gain != 0.0f && !los_b2u) return fail(h, WIFIRX_EINVAL, "los_b2u is required with a direct path");
    if (scatter && n_scatter == 0) return fail(h, WIFIRX_EINVAL, "n_scatter must be >= 1 with scatter");
    return WIFIRX_OK;
}

// one upload of what the host holds, as wifirx_irs_taps does it: add() appends an array at 8-byte alignment and notes which
// device pointer is to name it; send() copies, waits for the copy (not for a kernel) and sets the pointers
struct IrsMeta {
    std::vector<uint8_t> meta;
    std::vector<std::pair<void*, size_t>> named;
    void add(void* dev_ptr, const void* host, size_t bytes)
    {
        const size_t off = (meta.size() + 7) & ~(size_t)7;
        meta.resize(off + bytes);
        std::memcpy(meta.data() + off, host, bytes);
        named.emplace_back(dev_ptr, off);
    }
    int send(wifirx_handle* h)
    {
        int rc;
        if ((rc = h->stage.irs_meta.reserve(h, meta.size()))) return rc;
        HIP_TRY(h, hipMemcpyAsync(h->stage.irs_meta.p, meta.data(), meta.size(), hipMemcpyHostToDevice, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        for (const auto& n : named) {
            const uint8_t* dev = h->stage.irs_meta.as<uint8_t>() + n.second;
            std::memcpy(n.first, &dev, sizeof dev);
        }
        return WIFIRX_OK;
    }
};

// the scene's host arrays into `up` and its scalars into `a` (the pointers of `a` are set by up.send())
static void irs_multi_scene(wr::IrsMultiArgs& a, IrsMeta& up, std::vector<float>& scale, std::vector<float>& los_d, uint32_t n_ant,
                            uint32_t n_sets, uint32_t n_taps, const float* pdp, float gain, uint32_t n_elems, const float* los_b2r,
                            const float* los_r2u, const float* los_b2u, float k_factor, float direct_gain, const float* scatter,
                            uint32_t n_scatter, uint64_t irs_seed)
{
    scale.resize(n_taps);                               // s_l = (float)(sqrt(pdp_l) gain), formed in double
    for (uint32_t l = 0; l < n_taps; l++) scale[l] = (float)(std::sqrt((double)pdp[l]) * (double)gain);
    los_d.assign(2 * (size_t)n_ant, 0.0f);              // D_m; zeros where nothing of the direct path is read
    if (direct_gain != 0.0f) std::memcpy(los_d.data(), los_b2u, 8 * (size_t)n_ant);
    up.add(&a.s.los_a, los_b2r, 8ull * n_ant * n_elems);
    up.add(&a.s.los_b, los_r2u, 8ull * n_elems);
    up.add(&a.s.scale, scale.data(), 4ull * n_taps);
    up.add(&a.los_d, los_d.data(), 8ull * n_ant);
    a.s.scatter = reinterpret_cast<const float2*>(scatter);
    a.s.seed = irs_seed;
    a.s.n_sets = n_sets;
    a.s.n_taps = n_taps;
    a.s.n_elems = n_elems;
    a.s.n_psi_sets = 1;
    a.s.n_scatter = scatter ? n_scatter : 1;
    if (k_factor > 0.0f) {                              // formed in double; k_factor = 0: neither is applied (a_los = 0 says so)
        a.s.a_los = (float)std::sqrt((double)k_factor / ((double)k_factor + 1.0));
        a.s.a_nlos = (float)std::sqrt(1.0 / ((double)k_factor + 1.0));
    }
    a.s.direct_gain = direct_gain;
    a.n_ant = n_ant;
}

extern "C" int wifirx_irs_taps_multi(wifirx_handle* h, float* taps_out, uint32_t n_ant, uint32_t n_sets, uint32_t n_taps,
                                     const float* pdp, float gain, uint32_t n_elems,
                                     const float* los_b2r, const float* los_r2u, const float* los_b2u,
                                     float k_factor, float direct_gain,
                                     const float* psi, int psi_on_device, uint32_t n_psi_sets, uint32_t align_bits,
                                     const float* scatter, uint32_t n_scatter, uint64_t irs_seed,
                                     float* elems_out, uint8_t* codes_out)
{
    if (!h) return WIFIRX_EINVAL;
    // ---- the argument checks, before anything is queued ----
    if (!taps_out || !pdp || !los_b2r || !los_r2u) return fail(h, WIFIRX_EINVAL, "taps_out, pdp, los_b2r and los_r2u are required");
    if (align_bits > 3) return fail(h, WIFIRX_EINVAL, "align_bits must be 0..3");
    int rc;
    if ((rc = irs_multi_check(h, n_ant, n_taps, pdp, gain, n_elems, los_b2u, k_factor, direct_gain, scatter, n_scatter))) return rc;
    if (align_bits == 0 && !psi) return fail(h, WIFIRX_EINVAL, "psi is required when align_bits is 0");
    if (align_bits == 0 && n_psi_sets == 0) return fail(h, WIFIRX_EINVAL, "n_psi_sets must be >= 1 when align_bits is 0");
    if (align_bits == 0 && codes_out) return fail(h, WIFIRX_EINVAL, "codes_out needs align_bits 1..3");
    const auto addr = [](const void* p) { return reinterpret_cast<uintptr_t>(p); };
    const bool psi_read = align_bits == 0;
    if ((addr(taps_out) | addr(scatter) | addr(elems_out) | (psi_read && psi_on_device ? addr(psi) : 0)) & 7)
        return fail(h, WIFIRX_EINVAL, "taps_out, scatter, elems_out and device psi must be 8-byte aligned (complex64)");
    if ((addr(pdp) | addr(los_b2r) | addr(los_r2u) | addr(los_b2u) | (psi_read && !psi_on_device ? addr(psi) : 0)) & 3)
        return fail(h, WIFIRX_EINVAL, "the host arrays must be 4-byte aligned (float32)");
    for (uint32_t l = 0; l < n_taps; l++)
        if (!(std::isfinite(pdp[l]) && pdp[l] >= 0.0f)) return fail(h, WIFIRX_EINVAL, "pdp must be finite and not negative");
    if (n_sets == 0) return WIFIRX_OK;
    if (n_sets > 0x7fffffffu) return fail(h, WIFIRX_ERANGE, "more than 2^31 - 1 tap sets");
    const bool host_psi = psi_read && !psi_on_device;
    if (host_psi && (uint64_t)n_psi_sets * n_elems * 8 > (1ull << 31)) return fail(h, WIFIRX_ERANGE, "host psi above 2 GiB");

    stream_worker_wait_idle(h);
    HIP_TRY(h, hipSetDevice(h->device));
    wr::IrsMultiArgs a{};
    IrsMeta up;
    std::vector<float> scale, los_d;
    irs_multi_scene(a, up, scale, los_d, n_ant, n_sets, n_taps, pdp, gain, n_elems, los_b2r, los_r2u, los_b2u, k_factor, direct_gain,
                    scatter, n_scatter, irs_seed);
    a.s.psi = reinterpret_cast<const float2*>(psi);
    if (host_psi) up.add(&a.s.psi, psi, 8ull * n_psi_sets * n_elems);
    // the host arrays (the caller's and the staging vectors) may go once this returns
    if ((rc = up.send(h))) return rc;
    a.s.taps_out = reinterpret_cast<float2*>(taps_out);
    a.s.elems_out = reinterpret_cast<float2*>(elems_out);
    a.s.codes_out = codes_out;
    a.s.n_psi_sets = psi_read ? n_psi_sets : 1;
    a.s.align_bits = align_bits;
    HIP_TRY(h, wr_launch_irs_multi(h->stream, &a));
    return WIFIRX_OK;
}

extern "C" int wifirx_irs_sweep_multi(wifirx_handle* h, float* taps_out, uint32_t n_ant, uint32_t n_sets, uint32_t n_taps,
                                      const float* pdp, float gain, uint32_t n_elems,
                                      const float* los_b2r, const float* los_r2u, const float* los_b2u,
                                      float k_factor, float direct_gain,
                                      const float* codebook, int codebook_on_device, uint32_t n_codes,
                                      const float* scatter, uint32_t n_scatter, uint64_t irs_seed,
                                      uint16_t* best_out, float* power_out)
{
    if (!h) return WIFIRX_EINVAL;
    // ---- the argument checks, before anything is queued ----
    if (!pdp || !los_b2r || !los_r2u || !codebook) return fail(h, WIFIRX_EINVAL, "pdp, los_b2r, los_r2u and codebook are required");
    if (!taps_out && !best_out && !power_out) return fail(h, WIFIRX_EINVAL, "one of taps_out, best_out and power_out is required");
    if (n_codes < 1 || n_codes > wr_irs_max_codes()) return fail(h, WIFIRX_EINVAL, "n_codes must be 1..1024");
    int rc;
    if ((rc = irs_multi_check(h, n_ant, n_taps, pdp, gain, n_elems, los_b2u, k_factor, direct_gain, scatter, n_scatter))) return rc;
    const auto addr = [](const void* p) { return reinterpret_cast<uintptr_t>(p); };
    if ((addr(taps_out) | addr(scatter) | (codebook_on_device ? addr(codebook) : 0)) & 7)
        return fail(h, WIFIRX_EINVAL, "taps_out, scatter and a device codebook must be 8-byte aligned (complex64)");
    if ((addr(pdp) | addr(los_b2r) | addr(los_r2u) | addr(los_b2u) | addr(power_out) | (codebook_on_device ? 0 : addr(codebook))) & 3)
        return fail(h, WIFIRX_EINVAL, "the host arrays and power_out must be 4-byte aligned (float32)");
    if (addr(best_out) & 1) return fail(h, WIFIRX_EINVAL, "best_out must be 2-byte aligned (uint16)");
    for (uint32_t l = 0; l < n_taps; l++)
        if (!(std::isfinite(pdp[l]) && pdp[l] >= 0.0f)) return fail(h, WIFIRX_EINVAL, "pdp must be finite and not negative");
    if (n_sets == 0) return WIFIRX_OK;
    if (n_sets > 0x7fffffffu) return fail(h, WIFIRX_ERANGE, "more than 2^31 - 1 tap sets");

    stream_worker_wait_idle(h);
    HIP_TRY(h, hipSetDevice(h->device));
    wr::IrsSweepMultiArgs a{};
    IrsMeta up;
    std::vector<float> scale, los_d;
    irs_multi_scene(a.m, up, scale, los_d, n_ant, n_sets, n_taps, pdp, gain, n_elems, los_b2r, los_r2u, los_b2u, k_factor,
                    direct_gain, scatter, n_scatter, irs_seed);
    a.codebook = reinterpret_cast<const float2*>(codebook);
    if (!codebook_on_device) up.add(&a.codebook, codebook, 8ull * n_codes * n_elems);
    if ((rc = up.send(h))) return rc;
    a.m.s.taps_out = reinterpret_cast<float2*>(taps_out);
    a.best_out = best_out;
    a.power_out = power_out;
    a.n_codes = n_codes;
    HIP_TRY(h, wr_launch_irs_sweep_multi(h->stream, &a));
    return WIFIRX_OK;
}

// ---- the surface configured from noisy pilot observations (wr_irs_estimate.hip, NUMERICS.md rule 29) ----

extern "C" int wifirx_irs_estimate(wifirx_handle* h, float* taps_out, uint32_t n_ant, uint32_t n_sets, uint32_t n_taps,
                                   const float* pdp, float gain, uint32_t n_elems,
                                   const float* los_b2r, const float* los_r2u, const float* los_b2u, float k_factor, float direct_gain,
                                   const float* pilot, int pilot_on_device, uint32_t n_pilots, uint32_t n_groups, const uint16_t* group,
                                   float noise_sigma, float est_scale, uint32_t align_bits,
                                   const float* scatter, uint32_t n_scatter, const float* noise, uint32_t n_noise, uint64_t irs_seed,
                                   float* est_out, uint8_t* codes_out, float* obs_out)
{
    if (!h) return WIFIRX_EINVAL;
    // ---- the argument checks, before anything is queued ----
    if (!pdp || !los_b2r || !los_r2u || !pilot) return fail(h, WIFIRX_EINVAL, "pdp, los_b2r, los_r2u and pilot are required");
    if (!taps_out && !est_out && !codes_out && !obs_out)
        return fail(h, WIFIRX_EINVAL, "one of taps_out, est_out, codes_out and obs_out is required");
    if (align_bits > 3) return fail(h, WIFIRX_EINVAL, "align_bits must be 0..3");
    if (align_bits == 0 && (taps_out || codes_out)) return fail(h, WIFIRX_EINVAL, "taps_out and codes_out need align_bits 1..3");
    int rc;
    if ((rc = irs_multi_check(h, n_ant, n_taps, pdp, gain, n_elems, los_b2u, k_factor, direct_gain, scatter, n_scatter))) return rc;
    if (n_pilots < 1 || n_pilots > wr_irs_max_pilots()) return fail(h, WIFIRX_EINVAL, "n_pilots must be 1..1024");
    if (n_groups < 1 || n_groups > std::min(n_elems, wr_irs_max_groups())) return fail(h, WIFIRX_EINVAL, "n_groups must be 1..min(n_elems, 1023)");
    if (!group && n_groups != n_elems) return fail(h, WIFIRX_EINVAL, "group is required when n_groups differs from n_elems");
    if (!(std::isfinite(noise_sigma) && noise_sigma >= 0.0f)) return fail(h, WIFIRX_EINVAL, "noise_sigma must be finite and not negative");
    if (!std::isfinite(est_scale)) return fail(h, WIFIRX_EINVAL, "est_scale must be finite");
    if (noise && n_noise == 0) return fail(h, WIFIRX_EINVAL, "n_noise must be >= 1 with noise");
    const auto addr = [](const void* p) { return reinterpret_cast<uintptr_t>(p); };
    if ((addr(taps_out) | addr(scatter) | addr(noise) | addr(est_out) | addr(obs_out) | (pilot_on_device ? addr(pilot) : 0)) & 7)
        return fail(h, WIFIRX_EINVAL, "taps_out, est_out, obs_out, scatter, noise and a device pilot must be 8-byte aligned (complex64)");
    if ((addr(pdp) | addr(los_b2r) | addr(los_r2u) | addr(los_b2u) | (pilot_on_device ? 0 : addr(pilot))) & 3)
        return fail(h, WIFIRX_EINVAL, "the host arrays must be 4-byte aligned (float32)");
    if (addr(group) & 1) return fail(h, WIFIRX_EINVAL, "group must be 2-byte aligned (uint16)");
    for (uint32_t l = 0; l < n_taps; l++)
        if (!(std::isfinite(pdp[l]) && pdp[l] >= 0.0f)) return fail(h, WIFIRX_EINVAL, "pdp must be finite and not negative");
    if (group)
        for (uint32_t n = 0; n < n_elems; n++)
            if (group[n] >= n_groups) return fail(h, WIFIRX_EINVAL, "a group value is not below n_groups");
    if (n_sets == 0) return WIFIRX_OK;
    if (n_sets > 0x7fffffffu) return fail(h, WIFIRX_ERANGE, "more than 2^31 - 1 tap sets");
    const uint64_t rows = (uint64_t)n_sets * n_ant * n_taps;
    if ((rows + 15) / 16 > 0x7fffffffu) return fail(h, WIFIRX_ERANGE, "more than 2^31 - 1 tiles of 16 rows");

    stream_worker_wait_idle(h);
    HIP_TRY(h, hipSetDevice(h->device));
    wr::IrsEstimateArgs a{};
    IrsMeta up;
    std::vector<float> scale, los_d;
    irs_multi_scene(a.m, up, scale, los_d, n_ant, n_sets, n_taps, pdp, gain, n_elems, los_b2r, los_r2u, los_b2u, k_factor,
                    direct_gain, scatter, n_scatter, irs_seed);
    a.pilot = reinterpret_cast<const float2*>(pilot);
    if (!pilot_on_device) up.add(&a.pilot, pilot, 8ull * n_pilots * n_groups);
    if (group) up.add(&a.group, group, 2ull * n_elems);
    // the scratch is reserved before the upload is queued: a failed allocation queues nothing
    a.obs = reinterpret_cast<float2*>(obs_out);
    if (!obs_out && (taps_out || est_out || codes_out)) {
        if ((rc = h->stage.irs_obs.reserve(h, rows * n_pilots * 8))) return rc;
        a.obs = h->stage.irs_obs.as<float2>();
    }
    if (taps_out) {
        if ((rc = h->stage.irs_psi.reserve(h, 8ull * n_sets * n_elems))) return rc;
        a.psi_out = h->stage.irs_psi.as<float2>();
    }
    // the host arrays (the caller's and the staging vectors) may go once this returns
    if ((rc = up.send(h))) return rc;
    a.noise = reinterpret_cast<const float2*>(noise);
    a.est_out = reinterpret_cast<float2*>(est_out);
    a.m.s.codes_out = codes_out;
    a.m.s.align_bits = align_bits;
    a.n_pilots = n_pilots;
    a.n_groups = n_groups;
    a.n_noise = noise ? n_noise : 1;
    a.sigma = noise_sigma;
    a.kappa = est_scale;
    HIP_TRY(h, wr_launch_irs_observe(h->stream, &a));
    if (!taps_out && !est_out && !codes_out) return WIFIRX_OK;
    HIP_TRY(h, wr_launch_irs_despread(h->stream, &a));
    if (!taps_out) return WIFIRX_OK;
    // the taps of the TRUE elements under the decided phases: rule 27's kernel on the phases the decision pass wrote
    wr::IrsMultiArgs t = a.m;
    t.s.taps_out = reinterpret_cast<float2*>(taps_out);
    t.s.psi = a.psi_out;
    t.s.n_psi_sets = n_sets;
    t.s.align_bits = 0;
    t.s.codes_out = nullptr;
    t.s.elems_out = nullptr;
    HIP_TRY(h, wr_launch_irs_multi(h->stream, &t));
    return WIFIRX_OK;
}

// ---- the joint phase decision over antennas and taps (wr_irs_optimize.hip, NUMERICS.md rule 30) ----

// the body of wifirx_irs_optimize (weighted = false: weight, weight_on_device and n_weight_sets are not looked at) and of
// wifirx_irs_optimize_weighted (NUMERICS.md rule 31)
static int irs_optimize_call(wifirx_handle* h, const float* coef, uint32_t n_sets, uint32_t n_rows, uint32_t n_cols, bool weighted,
                             const float* weight, int weight_on_device, uint32_t n_weight_sets,
                             uint32_t bits, uint32_t max_sweeps, int start, int direct_blocked, const uint8_t* codes_in,
                             uint32_t n_elems, const uint16_t* group,
                             uint8_t* codes_out, float* psi_out, float* power_out, uint8_t* sweeps_out)
{
    if (!h) return WIFIRX_EINVAL;
    // ---- the argument checks, before anything is queued ----
    if (!coef) return fail(h, WIFIRX_EINVAL, "coef is required");
    if (!codes_out && !psi_out) return fail(h, WIFIRX_EINVAL, "one of codes_out and psi_out is required");
    if (n_rows < 1 || n_rows > wr_irs_max_rows()) return fail(h, WIFIRX_EINVAL, "n_rows must be 1..128");
    if (n_cols < 2 || n_cols > wr_irs_max_groups() + 1) return fail(h, WIFIRX_EINVAL, "n_cols must be 2..1024");
    if (bits < 1 || bits > 3) return fail(h, WIFIRX_EINVAL, "bits must be 1..3");
    if (max_sweeps > wr_irs_max_sweeps()) return fail(h, WIFIRX_EINVAL, "max_sweeps must be 0..16");
    if (start != WIFIRX_IRS_START_REF && start != WIFIRX_IRS_START_GIVEN && start != WIFIRX_IRS_START_ZERO)
        return fail(h, WIFIRX_EINVAL, "start must be WIFIRX_IRS_START_REF, _GIVEN or _ZERO");
    if (start == WIFIRX_IRS_START_GIVEN && !codes_in) return fail(h, WIFIRX_EINVAL, "codes_in is required with WIFIRX_IRS_START_GIVEN");
    const uint32_t n_groups = n_cols - 1;
    if (psi_out) {
        if (n_elems < 1 || n_elems > wr_irs_max_elems()) return fail(h, WIFIRX_EINVAL, "n_elems must be 1..4096 with psi_out");
        if (!group && n_elems != n_groups) return fail(h, WIFIRX_EINVAL, "group is required when n_elems differs from n_cols - 1");
    }
    const auto addr = [](const void* p) { return reinterpret_cast<uintptr_t>(p); };
    if ((addr(coef) | addr(psi_out)) & 7) return fail(h, WIFIRX_EINVAL, "coef and psi_out must be 8-byte aligned (complex64)");
    if (addr(power_out) & 3) return fail(h, WIFIRX_EINVAL, "power_out must be 4-byte aligned (float32)");
    if (psi_out && (addr(group) & 1)) return fail(h, WIFIRX_EINVAL, "group must be 2-byte aligned (uint16)");
    if (psi_out && group)
        for (uint32_t n = 0; n < n_elems; n++)
            if (group[n] >= n_groups) return fail(h, WIFIRX_EINVAL, "a group value is not below n_cols - 1");
    const bool host_weight = weighted && !weight_on_device;
    if (weighted) {
        if (!weight) return fail(h, WIFIRX_EINVAL, "weight is required");
        if (n_weight_sets != 1 && n_weight_sets != n_sets) return fail(h, WIFIRX_EINVAL, "n_weight_sets must be 1 or n_sets");
        if (host_weight && n_weight_sets != 1) return fail(h, WIFIRX_EINVAL, "host weights are one row block: n_weight_sets must be 1");
        if (addr(weight) & 3) return fail(h, WIFIRX_EINVAL, "weight must be 4-byte aligned (float32)");
        if (host_weight)
            for (uint32_t r = 0; r < n_rows; r++)
                if (!std::isfinite(weight[r])) return fail(h, WIFIRX_EINVAL, "a host weight is not finite");
    }
    if (n_sets == 0) return WIFIRX_OK;
    if (n_sets > 0x7fffffffu) return fail(h, WIFIRX_ERANGE, "more than 2^31 - 1 sets");

    stream_worker_wait_idle(h);
    HIP_TRY(h, hipSetDevice(h->device));
    wr::IrsOptimizeArgs a{};
    a.weight = weighted ? weight : nullptr;
    a.n_weight_sets = weighted ? n_weight_sets : 1;
    if ((psi_out && group) || host_weight) {            // the one upload: the group map, as wifirx_irs_estimate sends it, and
        IrsMeta up;                                     // the host weights
        int rc;
        if (psi_out && group) up.add(&a.group, group, 2ull * n_elems);
        if (host_weight) up.add(&a.weight, weight, 4ull * n_rows);
        if ((rc = up.send(h))) return rc;
    }
    a.coef = reinterpret_cast<const float2*>(coef);
    a.codes_in = start == WIFIRX_IRS_START_GIVEN ? codes_in : nullptr;
    a.codes_out = codes_out;
    a.psi_out = reinterpret_cast<float2*>(psi_out);
    a.power_out = power_out;
    a.sweeps_out = sweeps_out;
    a.n_sets = n_sets;
    a.n_rows = n_rows;
    a.n_cols = n_cols;
    a.n_elems = psi_out ? n_elems : 0;
    a.bits = bits;
    a.max_sweeps = max_sweeps;
    a.start = (uint32_t)start;
    a.blocked = direct_blocked != 0;
    HIP_TRY(h, wr_launch_irs_optimize(h->stream, &a));
    return WIFIRX_OK;
}

extern "C" int wifirx_irs_optimize(wifirx_handle* h, const float* coef, uint32_t n_sets, uint32_t n_rows, uint32_t n_cols,
                                   uint32_t bits, uint32_t max_sweeps, int start, int direct_blocked, const uint8_t* codes_in,
                                   uint32_t n_elems, const uint16_t* group,
                                   uint8_t* codes_out, float* psi_out, float* power_out, uint8_t* sweeps_out)
{
    return irs_optimize_call(h, coef, n_sets, n_rows, n_cols, false, nullptr, 0, 1, bits, max_sweeps, start, direct_blocked,
                             codes_in, n_elems, group, codes_out, psi_out, power_out, sweeps_out);
}

// ---- the same decision with a signed weight on every row (NUMERICS.md rule 31) ----

extern "C" int wifirx_irs_optimize_weighted(wifirx_handle* h, const float* coef, uint32_t n_sets, uint32_t n_rows, uint32_t n_cols,
                                            const float* weight, int weight_on_device, uint32_t n_weight_sets,
                                            uint32_t bits, uint32_t max_sweeps, int start, int direct_blocked, const uint8_t* codes_in,
                                            uint32_t n_elems, const uint16_t* group,
                                            uint8_t* codes_out, float* psi_out, float* power_out, uint8_t* sweeps_out)
{
    return irs_optimize_call(h, coef, n_sets, n_rows, n_cols, true, weight, weight_on_device, n_weight_sets, bits, max_sweeps, start,
                             direct_blocked, codes_in, n_elems, group, codes_out, psi_out, power_out, sweeps_out);
}
