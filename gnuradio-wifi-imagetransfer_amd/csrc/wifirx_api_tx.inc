// transmitter entry point: PSDUs -> time-domain rows on the device (wr_tx.hip)

namespace {

struct TxRate { uint32_t n_bpsc, n_cbps, n_dbps, rate_field; };
constexpr TxRate kTxRates[8] = {
    { 1, 48, 24, 0x0D }, { 1, 48, 36, 0x0F }, { 2, 96, 48, 0x05 }, { 2, 96, 72, 0x07 },
    { 4, 192, 96, 0x09 }, { 4, 192, 144, 0x0B }, { 6, 288, 192, 0x01 }, { 6, 288, 216, 0x03 },
};

}  // namespace

namespace {

// both transmitter entry points: every frame at `encoding`, or (enc_v != null) frame i at enc_v[i], checked by the caller
int tx_batch_impl(wifirx_handle* h, int encoding, const uint8_t* enc_v, const uint8_t* psdu, int psdu_on_device,
                  uint32_t psdu_stride, const uint32_t* psdu_len, const uint8_t* seeds, uint32_t n_frames, float* samples,
                  uint64_t samples_cap, const uint64_t* row_off, uint64_t row_len, uint32_t lead)
{
    if (n_frames == 0) return WIFIRX_OK;
    if (!psdu || !psdu_len || !samples) return fail(h, WIFIRX_EINVAL, "psdu, psdu_len and samples are required");
    if (reinterpret_cast<uintptr_t>(samples) & 7) return fail(h, WIFIRX_EINVAL, "samples must be 8-byte aligned (complex64)");
    const TxRate& rt = kTxRates[encoding];
    uint64_t psdu_extent = 0;
    for (uint32_t i = 0; i < n_frames; i++) {
        if (psdu_len[i] == 0 || psdu_len[i] > 4095) return fail(h, WIFIRX_EINVAL, "psdu_len must be 1..4095");
        if (psdu_len[i] > psdu_stride) return fail(h, WIFIRX_EINVAL, "psdu_stride is shorter than a PSDU");
        if (seeds && (seeds[i] == 0 || seeds[i] > 127)) return fail(h, WIFIRX_EINVAL, "scrambler seeds must be 1..127");
        psdu_extent = std::max<uint64_t>(psdu_extent, (uint64_t)i * psdu_stride + psdu_len[i]);
    }
    if (row_off)
        for (uint32_t i = 0; i < n_frames; i++)
            if (row_off[i + 1] < row_off[i]) return fail(h, WIFIRX_EINVAL, "row_off must not decrease");
    auto frame_len = [&](uint32_t len, uint32_t n_dbps) -> uint64_t {
        return (5ull + (16ull + 8ull * len + 6 + n_dbps - 1) / n_dbps) * 80 + 1;
    };
    for (uint32_t i = 0; i < n_frames; i++) {
        const uint64_t have = row_off ? row_off[i + 1] - row_off[i] : row_len;
        const uint32_t n_dbps = enc_v ? kTxRates[enc_v[i]].n_dbps : rt.n_dbps;
        if (have < (uint64_t)lead + frame_len(psdu_len[i], n_dbps)) return fail(h, WIFIRX_ERANGE, "a frame plus lead does not fit its row");
    }
    const uint64_t g0 = row_off ? row_off[0] : 0;
    if (!row_off && row_len > samples_cap / n_frames) return fail(h, WIFIRX_ERANGE, "rows exceed samples_cap");
    const uint64_t g1 = row_off ? row_off[n_frames] : row_len * n_frames;
    if (g1 > samples_cap) return fail(h, WIFIRX_ERANGE, "rows exceed samples_cap");
    stream_worker_wait_idle(h);
    HIP_TRY(h, hipSetDevice(h->device));

    wr::TxArgs a{};
    a.shift = (int64_t)((reinterpret_cast<uintptr_t>(samples) >> 3) & 1);
    a.g0 = (int64_t)g0;
    a.g1 = (int64_t)g1;
    a.v0 = (a.g0 + a.shift) & ~(int64_t)1;
    const uint64_t tile = wr_tx_tile_samples();
    const uint64_t n_tiles = ((uint64_t)(a.g1 + a.shift - a.v0) + tile - 1) / tile;
    if (n_tiles > 0x7fffffffull) return fail(h, WIFIRX_ERANGE, "more than 2^31 - 1 tiles of output");

    // one upload of what the host holds: lengths | seeds | encodings | row offsets | first row of every tile (row_off form)
    const size_t o_len = 0, o_seed = o_len + 4ull * n_frames, o_enc = o_seed + n_frames;
    const size_t o_row = (o_enc + (enc_v ? n_frames : 0) + 7) & ~size_t(7);
    const size_t o_tile = o_row + (row_off ? 8ull * (n_frames + 1) : 0);
    const size_t meta_bytes = o_tile + (row_off ? 4ull * n_tiles : 0);
    std::vector<uint8_t> meta(meta_bytes);
    std::memcpy(meta.data() + o_len, psdu_len, 4ull * n_frames);
    if (seeds) std::memcpy(meta.data() + o_seed, seeds, n_frames);
    if (enc_v) std::memcpy(meta.data() + o_enc, enc_v, n_frames);
    if (row_off) {
        std::memcpy(meta.data() + o_row, row_off, 8ull * (n_frames + 1));
        uint32_t* tr = reinterpret_cast<uint32_t*>(meta.data() + o_tile);
        uint32_t r = 0;
        for (uint64_t t = 0; t < n_tiles; t++) {
            const int64_t g_lo = std::max<int64_t>(a.g0, a.v0 + (int64_t)(t * tile) - a.shift);
            while (r + 1 < n_frames && (int64_t)row_off[r + 1] <= g_lo) r++;
            tr[t] = r;
        }
    }
    int rc = h->stage.tx_meta.reserve(h, meta_bytes);
    if (rc) return rc;
    HIP_TRY(h, hipMemcpyAsync(h->stage.tx_meta.p, meta.data(), meta_bytes, hipMemcpyHostToDevice, h->stream));
    const uint8_t* d_psdu = psdu;
    if (!psdu_on_device) {
        if ((rc = h->stage.tx_psdu.reserve(h, psdu_extent))) return rc;
        HIP_TRY(h, hipMemcpyAsync(h->stage.tx_psdu.p, psdu, psdu_extent, hipMemcpyHostToDevice, h->stream));
        d_psdu = h->stage.tx_psdu.as<const uint8_t>();
    }
    // the host arrays (the caller's and `meta`) may go once this returns: wait for the copies, not for the kernel
    HIP_TRY(h, hipStreamSynchronize(h->stream));

    uint8_t* dm = h->stage.tx_meta.as<uint8_t>();
    a.psdu = d_psdu;
    a.len = reinterpret_cast<const uint32_t*>(dm + o_len);
    a.seeds = seeds ? dm + o_seed : nullptr;
    a.row_off = row_off ? reinterpret_cast<const uint64_t*>(dm + o_row) : nullptr;
    a.tile_row = row_off ? reinterpret_cast<const uint32_t*>(dm + o_tile) : nullptr;
    a.out = reinterpret_cast<float2*>(samples);
    a.psdu_stride = psdu_stride;
    a.row_len = row_len;
    a.n_frames = n_frames;
    a.lead = lead;
    a.n_bpsc = rt.n_bpsc;
    a.n_cbps = rt.n_cbps;
    a.n_dbps = rt.n_dbps;
    a.enc = (uint32_t)encoding;
    a.rate_field = rt.rate_field;
    a.enc_v = enc_v ? dm + o_enc : nullptr;
    HIP_TRY(h, wr_launch_tx(h->stream, &a));
    return WIFIRX_OK;
}

}  // namespace

extern "C" int wifirx_tx_batch(wifirx_handle* h, int encoding, const uint8_t* psdu, int psdu_on_device, uint32_t psdu_stride,
                               const uint32_t* psdu_len, const uint8_t* seeds, uint32_t n_frames, float* samples,
                               uint64_t samples_cap, const uint64_t* row_off, uint64_t row_len, uint32_t lead)
{
    if (!h) return WIFIRX_EINVAL;
    if (encoding < WIFIRX_BPSK_1_2 || encoding > WIFIRX_64QAM_3_4) return fail(h, WIFIRX_EINVAL, "unknown encoding");
    return tx_batch_impl(h, encoding, nullptr, psdu, psdu_on_device, psdu_stride, psdu_len, seeds, n_frames, samples,
                         samples_cap, row_off, row_len, lead);
}

extern "C" int wifirx_tx_batch_rates(wifirx_handle* h, const uint8_t* encoding, const uint8_t* psdu, int psdu_on_device,
                                     uint32_t psdu_stride, const uint32_t* psdu_len, const uint8_t* seeds, uint32_t n_frames,
                                     float* samples, uint64_t samples_cap, const uint64_t* row_off, uint64_t row_len,
                                     uint32_t lead)
{
    if (!h) return WIFIRX_EINVAL;
    if (n_frames == 0) return WIFIRX_OK;
    if (!encoding) return fail(h, WIFIRX_EINVAL, "encoding is required");
    bool uniform = true;
    for (uint32_t i = 0; i < n_frames; i++) {
        if (encoding[i] > WIFIRX_64QAM_3_4) return fail(h, WIFIRX_EINVAL, "unknown encoding");
        uniform &= encoding[i] == encoding[0];
    }
    // one encoding for all: the single-encoding instance, which keeps that encoding's tables in LDS
    return tx_batch_impl(h, encoding[0], uniform ? nullptr : encoding, psdu, psdu_on_device, psdu_stride, psdu_len, seeds,
                         n_frames, samples, samples_cap, row_off, row_len, lead);
}
