// receive front end (NUMERICS.md rule 32; wr_frontend.hip): the call on device buffers, the host estimate, the receiver
// impairments of the loop-back, and the stream's switch.  The stream side is stream_frontend_run below, which stream_ingest
// (wifirx_api_stream.inc) calls on the samples it appends.

extern "C" void wr_frontend_estimate_host(const wifirx_frontend_cfg* cfg, const wifirx_frontend_state* s, float dc[2], float w[2]);
static int stream_drain_staged(wifirx_handle* h);

namespace {

int check_frontend_cfg(wifirx_handle* h, const wifirx_frontend_cfg* cfg)
{
    if (!cfg) return fail(h, WIFIRX_EINVAL, "cfg is required");
    if (cfg->flags & ~(WIFIRX_FE_DC | WIFIRX_FE_IQ)) return fail(h, WIFIRX_EINVAL, "flags must be a combination of WIFIRX_FE_DC and WIFIRX_FE_IQ");
    if (cfg->frac_bits > 30) return fail(h, WIFIRX_EINVAL, "frac_bits must be 0 .. 30");
    if (cfg->dc_shift > 6 || cfg->iq_shift > 6) return fail(h, WIFIRX_EINVAL, "dc_shift and iq_shift must be 0 .. 6");
    return WIFIRX_OK;
}

// what wifirx_frontend checks before anything is queued
int check_frontend(wifirx_handle* h, const wifirx_frontend_cfg* cfg, const wifirx_frontend_state* state, const void* in, int fmt,
                   float scale, uint64_t n, const float* out)
{
    if (int rc = check_frontend_cfg(h, cfg)) return rc;
    if (!state || !in || !out) return fail(h, WIFIRX_EINVAL, "state_dev, in and out are required");
    uint32_t bps;
    if (int rc = iq_check_format(h, fmt, scale, true, &bps)) return rc;
    const uintptr_t pi = reinterpret_cast<uintptr_t>(in), po = reinterpret_cast<uintptr_t>(out), ps = reinterpret_cast<uintptr_t>(state);
    if ((pi & (bps - 1)) || (po & 7) || (ps & 7))
        return fail(h, WIFIRX_EINVAL, "misaligned buffer (float pairs and the state: 8 bytes; sc16: 4; sc8: 2)");
    if (n > (1ull << 40)) return fail(h, WIFIRX_EINVAL, "n out of range (at most 2^40 samples per call)");
    if (!(fmt == WIFIRX_IQ_FC32 && pi == po) && ranges_overlap(in, n * bps, out, n * 8))
        return fail(h, WIFIRX_EINVAL, "in and out overlap (only in == out, for WIFIRX_IQ_FC32, is allowed)");
    if (ranges_overlap(state, sizeof(wifirx_frontend_state), in, n * bps) || ranges_overlap(state, sizeof(wifirx_frontend_state), out, n * 8))
        return fail(h, WIFIRX_EINVAL, "the state overlaps in or out");
    return WIFIRX_OK;
}

// the launches of one call, with the handle's table of block sums behind them
int frontend_run(wifirx_handle* h, const wifirx_frontend_cfg* cfg, wifirx_frontend_state* state, const void* in, int fmt, float scale,
                 uint64_t n, float2* out)
{
    if (int rc = h->stage.fe_table.reserve(h, (size_t)wr_frontend_table_rows(n) * 5 * sizeof(int64_t))) return rc;
    HIP_TRY(h, wr_launch_frontend(h->stream, cfg, state, in, fmt, scale, n, out, h->stage.fe_table.as<int64_t>(), h->n_cu));
    return WIFIRX_OK;
}

// Stream mode: room for the table of a pass of n samples (an allocation: in front of the pass's StreamRollback)
int stream_frontend_reserve(wifirx_handle* h, size_t n)
{
    if (!h->st.fe_on || !n) return WIFIRX_OK;
    return h->stage.fe_table.reserve(h, (size_t)wr_frontend_table_rows(n) * 5 * sizeof(int64_t));
}

// Stream mode: the front end over the n samples a pass appends at sbuf + sfill, `in` being where they are read from (the
// native samples, or sbuf + sfill itself for float pairs).  The state is saved first; StreamRollback puts it back.
int stream_frontend_run(wifirx_handle* h, const void* in, int fmt, float scale, size_t n, float2* out)
{
    StreamState& st = h->st;
    HIP_TRY(h, hipMemcpyAsync(st.fe_saved.p, st.fe_state.p, sizeof(wifirx_frontend_state), hipMemcpyDeviceToDevice, h->stream));
    st.fe_dirty = true;
    HIP_TRY(h, wr_launch_frontend(h->stream, &st.fe_cfg, st.fe_state.as<wifirx_frontend_state>(), in, fmt, scale, n, out,
                                  h->stage.fe_table.as<int64_t>(), h->n_cu));
    return WIFIRX_OK;
}

}  // namespace

extern "C" int wifirx_frontend(wifirx_handle* h, const wifirx_frontend_cfg* cfg, wifirx_frontend_state* state_dev, const void* in,
                               int fmt, float scale, uint64_t n, float* out)
{
    if (!h) return WIFIRX_EINVAL;
    if (int rc = check_frontend(h, cfg, state_dev, in, fmt, scale, n, out)) return rc;
    if (n == 0) return WIFIRX_OK;
    stream_worker_wait_idle(h);
    HIP_TRY(h, hipSetDevice(h->device));
    return frontend_run(h, cfg, state_dev, in, fmt, scale, n, reinterpret_cast<float2*>(out));
}

extern "C" int wifirx_frontend_estimate(const wifirx_frontend_cfg* cfg, const wifirx_frontend_state* state_host, float dc[2], float w[2])
{
    if (!state_host || !dc || !w) return fail(nullptr, WIFIRX_EINVAL, "null argument");
    if (int rc = check_frontend_cfg(nullptr, cfg)) return rc;
    wr_frontend_estimate_host(cfg, state_host, dc, w);
    return WIFIRX_OK;
}

extern "C" int wifirx_rx_impair(wifirx_handle* h, const float* in, float* out, uint64_t n, const float mu[2], const float nu[2],
                                const float dc[2])
{
    if (!h) return WIFIRX_EINVAL;
    if (!in || !out || !mu || !nu || !dc) return fail(h, WIFIRX_EINVAL, "in, out, mu, nu and dc are required");
    for (int i = 0; i < 2; i++)
        if (!std::isfinite(mu[i]) || !std::isfinite(nu[i]) || !std::isfinite(dc[i])) return fail(h, WIFIRX_EINVAL, "mu, nu and dc must be finite");
    const uintptr_t pi = reinterpret_cast<uintptr_t>(in), po = reinterpret_cast<uintptr_t>(out);
    if ((pi & 7) || (po & 7)) return fail(h, WIFIRX_EINVAL, "misaligned buffer (float pairs: 8 bytes)");
    if (n > (1ull << 40)) return fail(h, WIFIRX_EINVAL, "n out of range (at most 2^40 samples per call)");
    if (pi != po && ranges_overlap(in, n * 8, out, n * 8)) return fail(h, WIFIRX_EINVAL, "in and out overlap (only in == out is allowed)");
    if (n == 0) return WIFIRX_OK;
    stream_worker_wait_idle(h);
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, wr_launch_rx_impair(h->stream, reinterpret_cast<const float2*>(in), reinterpret_cast<float2*>(out), n,
                                   make_float2(mu[0], mu[1]), make_float2(nu[0], nu[1]), make_float2(dc[0], dc[1]), h->n_cu));
    return WIFIRX_OK;
}

extern "C" int wifirx_stream_frontend(wifirx_handle* h, const wifirx_frontend_cfg* cfg, const wifirx_frontend_state* init)
{
    if (!h) return WIFIRX_EINVAL;
    if (cfg) {
        if (int rc = check_frontend_cfg(h, cfg)) return rc;
        if (h->div.n_ant) return fail(h, WIFIRX_EINVAL, "the handle's stream is a diversity stream: it has no front end");
    }
    if (int rc = stream_drain_staged(h)) return rc;        // samples staged under the old setting run under it
    HIP_TRY(h, hipSetDevice(h->device));
    StreamState& st = h->st;
    if (!cfg) {
        st.fe_on = false;
        return WIFIRX_OK;
    }
    if (!st.fe_state.p) {
        if (int rc = st.fe_state.alloc(h, sizeof(wifirx_frontend_state), "hipMalloc(front-end state)")) return rc;
        if (int rc = st.fe_saved.alloc(h, sizeof(wifirx_frontend_state), "hipMalloc(front-end state)")) { st.fe_state.reset(); return rc; }
    }
    if (init) HIP_TRY(h, hipMemcpyAsync(st.fe_state.p, init, sizeof(wifirx_frontend_state), hipMemcpyHostToDevice, h->stream));
    else HIP_TRY(h, hipMemsetAsync(st.fe_state.p, 0, sizeof(wifirx_frontend_state), h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));            // *init may be reused
    st.fe_cfg = *cfg;
    st.fe_on = true;
    return WIFIRX_OK;
}

extern "C" int wifirx_stream_frontend_state(wifirx_handle* h, wifirx_frontend_state* out_host)
{
    if (!h) return WIFIRX_EINVAL;
    if (!out_host) return fail(h, WIFIRX_EINVAL, "out_host is required");
    if (!h->st.fe_on) return fail(h, WIFIRX_EINVAL, "the handle's front end is off");
    stream_worker_wait_idle(h);
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipMemcpyAsync(out_host, h->st.fe_state.p, sizeof(wifirx_frontend_state), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return WIFIRX_OK;
}
