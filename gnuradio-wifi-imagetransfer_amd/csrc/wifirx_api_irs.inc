// IRS entry points: the reflecting surface behind an AP of n_ant = 1..8 antennas, made on the device -- its cascade channel
// (wr_irs.hip, NUMERICS.md rules 25 and 27), its beam training over a codebook (wr_irs_sweep.hip, rules 26 and 28), its
// configuration from pilot observations (wr_irs_estimate.hip, rule 29) -- and the joint phase decision (wr_irs_optimize.hip, rules
// 30 and 31).  The one-antenna entry points are the multi-antenna ones at n_ant = 1.

// the scene arguments of an entry point, as they were passed
struct IrsScene {
    uint32_t     n_ant, n_sets, n_taps;
    const float* pdp;
    float        gain;
    uint32_t     n_elems;
    const float *los_b2r, *los_r2u, *los_b2u;
    float        k_factor, direct_gain;
    const float* scatter;
    uint32_t     n_scatter;
    uint64_t     irs_seed;
};

static uintptr_t irs_addr(const void* p) { return reinterpret_cast<uintptr_t>(p); }

// the checks of the scene's numbers, which follow the entry point's required pointers (align_bits: 0 where the call has none)
static int irs_scene_check(wifirx_handle* h, const IrsScene& c, uint32_t align_bits)
{
    if (c.n_ant < 1 || c.n_ant > wr_irs_max_ant()) return fail(h, WIFIRX_EINVAL, "n_ant must be 1..8");
    if (c.n_elems < 1 || c.n_elems > wr_irs_max_elems()) return fail(h, WIFIRX_EINVAL, "n_elems must be 1..4096");
    if (c.n_taps < 1 || c.n_taps > wr_irs_max_taps()) return fail(h, WIFIRX_EINVAL, "n_taps must be 1..16");
    if (align_bits > 3) return fail(h, WIFIRX_EINVAL, "align_bits must be 0..3");
    if (!std::isfinite(c.gain) || !std::isfinite(c.direct_gain)) return fail(h, WIFIRX_EINVAL, "gain and direct_gain must be finite");
    if (!(std::isfinite(c.k_factor) && c.k_factor >= 0.0f)) return fail(h, WIFIRX_EINVAL, "k_factor must be finite and not negative");
    if (c.direct_gain != 0.0f && !c.los_b2u) return fail(h, WIFIRX_EINVAL, "los_b2u is required with a direct path");
    return WIFIRX_OK;
}

// ... and the checks that follow the entry point's own: the scatter rows, the alignment of the scene's arrays and of the call's
// own (at8, at4, at2: their addresses OR-ed, for elements of 8, 4 and 2 bytes; msg8, msg4, msg2: the call's words), and the pdp
static int irs_layout_check(wifirx_handle* h, const IrsScene& c, uintptr_t at8, const char* msg8, uintptr_t at4, const char* msg4,
                            uintptr_t at2 = 0, const char* msg2 = "")
{
    if (c.scatter && c.n_scatter == 0) return fail(h, WIFIRX_EINVAL, "n_scatter must be >= 1 with scatter");
    if ((at8 | irs_addr(c.scatter)) & 7) return fail(h, WIFIRX_EINVAL, msg8);
    if ((at4 | irs_addr(c.pdp) | irs_addr(c.los_b2r) | irs_addr(c.los_r2u) | irs_addr(c.los_b2u)) & 3) return fail(h, WIFIRX_EINVAL, msg4);
    if (at2 & 1) return fail(h, WIFIRX_EINVAL, msg2);
    for (uint32_t l = 0; l < c.n_taps; l++)
        if (!(std::isfinite(c.pdp[l]) && c.pdp[l] >= 0.0f)) return fail(h, WIFIRX_EINVAL, "pdp must be finite and not negative");
    return WIFIRX_OK;
}

// one upload of what the host holds, as channel_call does it: add() appends an array at 8-byte alignment and notes which
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
static void irs_scene_fill(wr::IrsArgs& a, IrsMeta& up, std::vector<float>& scale, std::vector<float>& los_d, const IrsScene& c)
{
    scale.resize(c.n_taps);                             // s_l = (float)(sqrt(pdp_l) gain), formed in double
    for (uint32_t l = 0; l < c.n_taps; l++) scale[l] = (float)(std::sqrt((double)c.pdp[l]) * (double)c.gain);
    los_d.assign(2 * (size_t)c.n_ant, 0.0f);            // D_m; zeros where nothing of the direct path is read
    if (c.direct_gain != 0.0f) std::memcpy(los_d.data(), c.los_b2u, 8 * (size_t)c.n_ant);
    up.add(&a.los_a, c.los_b2r, 8ull * c.n_ant * c.n_elems);
    up.add(&a.los_b, c.los_r2u, 8ull * c.n_elems);
    up.add(&a.scale, scale.data(), 4ull * c.n_taps);
    up.add(&a.los_d, los_d.data(), 8ull * c.n_ant);
    a.scatter = reinterpret_cast<const float2*>(c.scatter);
    a.seed = c.irs_seed;
    a.n_ant = c.n_ant;
    a.n_sets = c.n_sets;
    a.n_taps = c.n_taps;
    a.n_elems = c.n_elems;
    a.n_psi_sets = 1;
    a.n_scatter = c.scatter ? c.n_scatter : 1;
    if (c.k_factor > 0.0f) {                            // formed in double; k_factor = 0: neither is applied (a_los = 0 says so)
        a.a_los = (float)std::sqrt((double)c.k_factor / ((double)c.k_factor + 1.0));
        a.a_nlos = (float)std::sqrt(1.0 / ((double)c.k_factor + 1.0));
    }
    a.direct_gain = c.direct_gain;
}

// ---- the cascade channel's tap sets (wr_irs.hip, NUMERICS.md rules 25 and 27) ----

extern "C" int wifirx_irs_taps_multi(wifirx_handle* h, float* taps_out, uint32_t n_ant, uint32_t n_sets, uint32_t n_taps,
                                     const float* pdp, float gain, uint32_t n_elems,
                                     const float* los_b2r, const float* los_r2u, const float* los_b2u,
                                     float k_factor, float direct_gain,
                                     const float* psi, int psi_on_device, uint32_t n_psi_sets, uint32_t align_bits,
                                     const float* scatter, uint32_t n_scatter, uint64_t irs_seed,
                                     float* elems_out, uint8_t* codes_out)
{
    if (!h) return WIFIRX_EINVAL;
    const IrsScene c{n_ant, n_sets, n_taps, pdp, gain, n_elems, los_b2r, los_r2u, los_b2u, k_factor, direct_gain, scatter, n_scatter, irs_seed};
    // ---- the argument checks, before anything is queued ----
    if (!taps_out || !pdp || !los_b2r || !los_r2u) return fail(h, WIFIRX_EINVAL, "taps_out, pdp, los_b2r and los_r2u are required");
    int rc;
    if ((rc = irs_scene_check(h, c, align_bits))) return rc;
    if (align_bits == 0 && !psi) return fail(h, WIFIRX_EINVAL, "psi is required when align_bits is 0");
    if (align_bits == 0 && n_psi_sets == 0) return fail(h, WIFIRX_EINVAL, "n_psi_sets must be >= 1 when align_bits is 0");
    if (align_bits == 0 && codes_out) return fail(h, WIFIRX_EINVAL, "codes_out needs align_bits 1..3");
    const bool psi_read = align_bits == 0, host_psi = psi_read && !psi_on_device;
    if ((rc = irs_layout_check(h, c, irs_addr(taps_out) | irs_addr(elems_out) | (psi_read && psi_on_device ? irs_addr(psi) : 0),
                               "taps_out, scatter, elems_out and device psi must be 8-byte aligned (complex64)",
                               host_psi ? irs_addr(psi) : 0, "the host arrays must be 4-byte aligned (float32)")))
        return rc;
    if (n_sets == 0) return WIFIRX_OK;
    if (n_sets > 0x7fffffffu) return fail(h, WIFIRX_ERANGE, "more than 2^31 - 1 tap sets");
    if (host_psi && (uint64_t)n_psi_sets * n_elems * 8 > (1ull << 31)) return fail(h, WIFIRX_ERANGE, "host psi above 2 GiB");

    stream_worker_wait_idle(h);
    HIP_TRY(h, hipSetDevice(h->device));
    wr::IrsArgs a{};
    IrsMeta up;
    std::vector<float> scale, los_d;
    irs_scene_fill(a, up, scale, los_d, c);
    a.psi = reinterpret_cast<const float2*>(psi);
    if (host_psi) up.add(&a.psi, psi, 8ull * n_psi_sets * n_elems);
    // the host arrays (the caller's and the staging vectors) may go once this returns
    if ((rc = up.send(h))) return rc;
    a.taps_out = reinterpret_cast<float2*>(taps_out);
    a.elems_out = reinterpret_cast<float2*>(elems_out);
    a.codes_out = codes_out;
    a.n_psi_sets = psi_read ? n_psi_sets : 1;
    a.align_bits = align_bits;
    HIP_TRY(h, wr_launch_irs(h->stream, &a));
    return WIFIRX_OK;
}

extern "C" int wifirx_irs_taps(wifirx_handle* h, float* taps_out, uint32_t n_sets, uint32_t n_taps, const float* pdp, float gain,
                               uint32_t n_elems, const float* los_b2r, const float* los_r2u, const float* los_b2u,
                               float k_factor, float direct_gain,
                               const float* psi, int psi_on_device, uint32_t n_psi_sets, uint32_t align_bits,
                               const float* scatter, uint32_t n_scatter, uint64_t irs_seed,
                               float* elems_out, uint8_t* codes_out)
{
    return wifirx_irs_taps_multi(h, taps_out, 1, n_sets, n_taps, pdp, gain, n_elems, los_b2r, los_r2u, los_b2u, k_factor, direct_gain,
                                 psi, psi_on_device, n_psi_sets, align_bits, scatter, n_scatter, irs_seed, elems_out, codes_out);
}

// ---- beam training over a codebook: the same scene, K configurations, the best one per set (wr_irs_sweep.hip, NUMERICS.md rules
// 26 and 28) ----

extern "C" int wifirx_irs_sweep_multi(wifirx_handle* h, float* taps_out, uint32_t n_ant, uint32_t n_sets, uint32_t n_taps,
                                      const float* pdp, float gain, uint32_t n_elems,
                                      const float* los_b2r, const float* los_r2u, const float* los_b2u,
                                      float k_factor, float direct_gain,
                                      const float* codebook, int codebook_on_device, uint32_t n_codes,
                                      const float* scatter, uint32_t n_scatter, uint64_t irs_seed,
                                      uint16_t* best_out, float* power_out)
{
    if (!h) return WIFIRX_EINVAL;
    const IrsScene c{n_ant, n_sets, n_taps, pdp, gain, n_elems, los_b2r, los_r2u, los_b2u, k_factor, direct_gain, scatter, n_scatter, irs_seed};
    // ---- the argument checks, before anything is queued ----
    if (!pdp || !los_b2r || !los_r2u || !codebook) return fail(h, WIFIRX_EINVAL, "pdp, los_b2r, los_r2u and codebook are required");
    if (!taps_out && !best_out && !power_out) return fail(h, WIFIRX_EINVAL, "one of taps_out, best_out and power_out is required");
    int rc;
    if ((rc = irs_scene_check(h, c, 0))) return rc;
    if (n_codes < 1 || n_codes > wr_irs_max_codes()) return fail(h, WIFIRX_EINVAL, "n_codes must be 1..1024");
    if ((rc = irs_layout_check(h, c, irs_addr(taps_out) | (codebook_on_device ? irs_addr(codebook) : 0),
                               "taps_out, scatter and a device codebook must be 8-byte aligned (complex64)",
                               irs_addr(power_out) | (codebook_on_device ? 0 : irs_addr(codebook)),
                               "the host arrays and power_out must be 4-byte aligned (float32)",
                               irs_addr(best_out), "best_out must be 2-byte aligned (uint16)")))
        return rc;
    if (n_sets == 0) return WIFIRX_OK;
    if (n_sets > 0x7fffffffu) return fail(h, WIFIRX_ERANGE, "more than 2^31 - 1 tap sets");

    stream_worker_wait_idle(h);
    HIP_TRY(h, hipSetDevice(h->device));
    wr::IrsSweepArgs a{};
    IrsMeta up;
    std::vector<float> scale, los_d;
    irs_scene_fill(a.s, up, scale, los_d, c);
    a.codebook = reinterpret_cast<const float2*>(codebook);
    if (!codebook_on_device) up.add(&a.codebook, codebook, 8ull * n_codes * n_elems);
    // the host arrays (the caller's and the staging vectors) may go once this returns
    if ((rc = up.send(h))) return rc;
    a.s.taps_out = reinterpret_cast<float2*>(taps_out);
    a.best_out = best_out;
    a.power_out = power_out;
    a.n_codes = n_codes;
    HIP_TRY(h, wr_launch_irs_sweep(h->stream, &a));
    return WIFIRX_OK;
}

extern "C" int wifirx_irs_sweep(wifirx_handle* h, float* taps_out, uint32_t n_sets, uint32_t n_taps, const float* pdp, float gain,
                                uint32_t n_elems, const float* los_b2r, const float* los_r2u, const float* los_b2u,
                                float k_factor, float direct_gain,
                                const float* codebook, int codebook_on_device, uint32_t n_codes,
                                const float* scatter, uint32_t n_scatter, uint64_t irs_seed,
                                uint16_t* best_out, float* power_out)
{
    return wifirx_irs_sweep_multi(h, taps_out, 1, n_sets, n_taps, pdp, gain, n_elems, los_b2r, los_r2u, los_b2u, k_factor, direct_gain,
                                  codebook, codebook_on_device, n_codes, scatter, n_scatter, irs_seed, best_out, power_out);
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
    const IrsScene c{n_ant, n_sets, n_taps, pdp, gain, n_elems, los_b2r, los_r2u, los_b2u, k_factor, direct_gain, scatter, n_scatter, irs_seed};
    // ---- the argument checks, before anything is queued ----
    if (!pdp || !los_b2r || !los_r2u || !pilot) return fail(h, WIFIRX_EINVAL, "pdp, los_b2r, los_r2u and pilot are required");
    if (!taps_out && !est_out && !codes_out && !obs_out)
        return fail(h, WIFIRX_EINVAL, "one of taps_out, est_out, codes_out and obs_out is required");
    int rc;
    if ((rc = irs_scene_check(h, c, align_bits))) return rc;
    if (align_bits == 0 && (taps_out || codes_out)) return fail(h, WIFIRX_EINVAL, "taps_out and codes_out need align_bits 1..3");
    if (n_pilots < 1 || n_pilots > wr_irs_max_pilots()) return fail(h, WIFIRX_EINVAL, "n_pilots must be 1..1024");
    if (n_groups < 1 || n_groups > std::min(n_elems, wr_irs_max_groups())) return fail(h, WIFIRX_EINVAL, "n_groups must be 1..min(n_elems, 1023)");
    if (!group && n_groups != n_elems) return fail(h, WIFIRX_EINVAL, "group is required when n_groups differs from n_elems");
    if (!(std::isfinite(noise_sigma) && noise_sigma >= 0.0f)) return fail(h, WIFIRX_EINVAL, "noise_sigma must be finite and not negative");
    if (!std::isfinite(est_scale)) return fail(h, WIFIRX_EINVAL, "est_scale must be finite");
    if (noise && n_noise == 0) return fail(h, WIFIRX_EINVAL, "n_noise must be >= 1 with noise");
    if ((rc = irs_layout_check(h, c, irs_addr(taps_out) | irs_addr(noise) | irs_addr(est_out) | irs_addr(obs_out) | (pilot_on_device ? irs_addr(pilot) : 0),
                               "taps_out, est_out, obs_out, scatter, noise and a device pilot must be 8-byte aligned (complex64)",
                               pilot_on_device ? 0 : irs_addr(pilot), "the host arrays must be 4-byte aligned (float32)",
                               irs_addr(group), "group must be 2-byte aligned (uint16)")))
        return rc;
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
    irs_scene_fill(a.s, up, scale, los_d, c);
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
    a.s.codes_out = codes_out;
    a.s.align_bits = align_bits;
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
    wr::IrsArgs t = a.s;
    t.taps_out = reinterpret_cast<float2*>(taps_out);
    t.psi = a.psi_out;
    t.n_psi_sets = n_sets;
    t.align_bits = 0;
    t.codes_out = nullptr;
    t.elems_out = nullptr;
    HIP_TRY(h, wr_launch_irs(h->stream, &t));
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
