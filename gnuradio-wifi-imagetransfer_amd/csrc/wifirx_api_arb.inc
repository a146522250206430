// the rational resampler on device buffers (NUMERICS.md rule 34; wr_arb.hip): a capture at any rate into the channel rate,
// or a stream at the channel rate into a converter's

namespace {

static_assert(WIFIRX_ARB_HIST_MAX == 128, "rule 34: HL = ceil(32 S / den) <= 128");

constexpr uint64_t ARB_INDEX_LIMIT = 1ull << 62;             // (j0 + n_in) den and (m0 + n_out) num stay below it

// n_out of a call, rule 34's counting: m0 .. m_end(j0 + n_in) - 1.  false: (j0 + n_in) den or (m0 + n_out) num >= 2^62
bool arb_count(const wr_arb_ratio& r, uint64_t j0, uint64_t n_in, uint64_t m0, uint64_t* n_out)
{
    const unsigned __int128 E = (unsigned __int128)j0 + n_in;
    if (E * r.den >= ARB_INDEX_LIMIT) return false;
    const uint64_t end = wr_arb_m_end(&r, (uint64_t)E);
    *n_out = end > m0 ? end - m0 : 0;
    return ((unsigned __int128)m0 + *n_out) * r.num < ARB_INDEX_LIMIT;
}

// What wifirx_arb_resample and wifirx_tune share.  A call's checked arguments:
struct arb_call {
    wr_arb_ratio r;
    uint32_t bps;                    // bytes per input sample
    uint64_t n;                      // outputs (per channel)
    uint64_t in_bytes, hist_bytes;
};

// every check that needs no output buffer: the arguments, the ratio, the alignment, the counting; `room` float pairs per row
int arb_check_call(wifirx_handle* h, const void* in, int fmt, float scale, uint64_t n_in, const void* hist, const void* hist_out,
                   uint32_t num, uint32_t den, uint64_t j0, uint64_t m0, const float* out, uint64_t room, const uint64_t* n_out,
                   arb_call* c)
{
    if (!n_out) return fail(h, WIFIRX_EINVAL, "n_out is required");
    if (n_in && !in) return fail(h, WIFIRX_EINVAL, "in is required");
    if (int rc = iq_check_format(h, fmt, scale, true, &c->bps)) return rc;
    if (!wr_arb_plan(num, den, &c->r))
        return fail(h, WIFIRX_EINVAL, "num / den must reduce to 1 <= den <= 512, 1 <= num <= 2048, num <= 4 den, den <= 4 num");
    const uintptr_t align = c->bps - 1;
    if ((reinterpret_cast<uintptr_t>(in) & align) || (reinterpret_cast<uintptr_t>(hist) & align) ||
        (reinterpret_cast<uintptr_t>(hist_out) & align) || (reinterpret_cast<uintptr_t>(out) & 7))
        return fail(h, WIFIRX_EINVAL, "misaligned buffer (out: 8 bytes; in, hist, hist_out: fc32 8, sc16 4, sc8 2)");
    c->n = 0;
    if (!arb_count(c->r, j0, n_in, m0, &c->n))
        return fail(h, WIFIRX_ERANGE, "(j0 + n_in) den and (m0 + n_out) num must stay below 2^62");
    if (c->n && !out) return fail(h, WIFIRX_EINVAL, "out is required");
    if (c->n > room) return fail(h, WIFIRX_ERANGE, "out_cap (out_stride) is smaller than n_out (wifirx_arb_count)");
    if ((c->n + WR_ARB_TILE - 1) / WR_ARB_TILE > 0x7fffffffull) return fail(h, WIFIRX_ERANGE, "too many outputs for one call");
    c->in_bytes = n_in * c->bps;
    c->hist_bytes = (uint64_t)c->r.HL * c->bps;
    return WIFIRX_OK;
}

// no overlap among in, hist, hist_out and the out_bytes of out; the history reaches the call's first output
int arb_check_buffers(wifirx_handle* h, const arb_call& c, const void* in, const void* hist, const void* hist_out, const float* out,
                      uint64_t out_bytes, uint64_t j0, uint64_t m0)
{
    const wr_arb_ratio& r = c.r;
    const ByteRange buf[4] = { { in, c.in_bytes }, { out, out_bytes }, { hist, hist ? c.hist_bytes : 0 }, { hist_out, hist_out ? c.hist_bytes : 0 } };
    if (any_overlap(buf)) return fail(h, WIFIRX_EINVAL, "in, hist, hist_out and out must not overlap");
    if (c.n) {
        // jlo(m0) = floor((m0 num - 16 S) / den) + 1 must not lie in front of the history
        const int64_t D = (int64_t)(m0 * r.num) - 16 * (int64_t)r.S;
        int64_t fl = D / (int64_t)r.den;
        if (D - fl * (int64_t)r.den < 0) fl -= 1;
        if (fl + 1 < (int64_t)j0 - (int64_t)r.HL)
            return fail(h, WIFIRX_EINVAL, "the history does not reach output m0: its first input lies in front of j0 - hist_len");
    }
    return WIFIRX_OK;
}

}  // namespace

extern "C" int wifirx_arb_hist(uint32_t num, uint32_t den, uint32_t* hist_len)
{
    wr_arb_ratio r;
    if (!hist_len || !wr_arb_plan(num, den, &r)) return WIFIRX_EINVAL;
    *hist_len = r.HL;
    return WIFIRX_OK;
}

extern "C" int wifirx_arb_count(uint32_t num, uint32_t den, uint64_t j0, uint64_t n_in, uint64_t m0, uint64_t* n_out)
{
    wr_arb_ratio r;
    if (!n_out || !wr_arb_plan(num, den, &r)) return WIFIRX_EINVAL;
    return arb_count(r, j0, n_in, m0, n_out) ? WIFIRX_OK : WIFIRX_ERANGE;
}

extern "C" int wifirx_arb_table(const float** table, uint32_t* n_entries, uint32_t* per_unit)
{
    if (!table || !n_entries || !per_unit) return WIFIRX_EINVAL;
    *table = wr_arb_host_table();
    *n_entries = WR_ARB_ENTRIES;
    *per_unit = WR_ARB_PER_UNIT;
    return WIFIRX_OK;
}

extern "C" int wifirx_arb_resample(wifirx_handle* h, const void* in, int fmt, float scale, uint64_t n_in, const void* hist,
                                   void* hist_out, uint32_t num, uint32_t den, uint64_t j0, uint64_t m0, float* out,
                                   uint64_t out_cap, uint64_t* n_out)
{
    if (!h) return WIFIRX_EINVAL;
    arb_call c;
    if (int rc = arb_check_call(h, in, fmt, scale, n_in, hist, hist_out, num, den, j0, m0, out, out_cap, n_out, &c)) return rc;
    if (int rc = arb_check_buffers(h, c, in, hist, hist_out, out, c.n * 8, j0, m0)) return rc;
    *n_out = c.n;
    if (c.n == 0 && !hist_out) return WIFIRX_OK;
    stream_worker_wait_idle(h);
    HIP_TRY(h, hipSetDevice(h->device));
    if (c.n)
        HIP_TRY(h, wr_launch_arb(h->stream, in, fmt, scale, n_in, hist, &c.r, j0, m0, c.n, reinterpret_cast<float2*>(out)));
    return hist_out ? queue_hist_tail(h, in, c.in_bytes, hist, hist_out, c.hist_bytes) : WIFIRX_OK;
}
