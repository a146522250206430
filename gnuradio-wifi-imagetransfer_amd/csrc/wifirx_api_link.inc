// the two ends of the device loop-back: ieee802_11.mac for a batch, and the scoring of a decoded batch (wr_link.hip)

extern "C" int wifirx_mac_batch(wifirx_handle* h, const uint8_t* payload, int payload_on_device, uint32_t payload_stride,
                                const uint32_t* payload_len, uint32_t n_frames, const uint8_t* addr, uint32_t seq0,
                                uint64_t payload_seed, uint8_t* psdu, uint32_t psdu_stride)
{
    if (!h) return WIFIRX_EINVAL;
    if (n_frames == 0) return WIFIRX_OK;
    if (!psdu) return fail(h, WIFIRX_EINVAL, "psdu is required");
    constexpr uint32_t kMaxPayload = WIFIRX_MAX_PSDU - 28;
    uint32_t len_max = 0;
    uint64_t payload_extent = 0;
    for (uint32_t i = 0; i < n_frames; i++) {
        const uint32_t len = payload_len ? payload_len[i] : payload_stride;
        if (len > kMaxPayload) return fail(h, WIFIRX_EINVAL, "payload_len must be at most 1500");
        if (payload && len > payload_stride) return fail(h, WIFIRX_EINVAL, "payload_stride is shorter than a payload");
        len_max = std::max(len_max, len);
        if (len) payload_extent = std::max<uint64_t>(payload_extent, (uint64_t)i * payload_stride + len);
        if (!payload_len) break;        // one length for all: checked once
    }
    if (!payload_len && len_max) payload_extent = (uint64_t)(n_frames - 1) * payload_stride + len_max;
    if (psdu_stride < 28 + len_max) return fail(h, WIFIRX_ERANGE, "psdu_stride is shorter than a PSDU");
    if (payload_len)
        for (uint32_t i = 0; i < n_frames; i++)
            if (psdu_stride < 28 + payload_len[i]) return fail(h, WIFIRX_ERANGE, "psdu_stride is shorter than a PSDU");
    stream_worker_wait_idle(h);
    HIP_TRY(h, hipSetDevice(h->device));

    wr::MacArgs a{};
    bool uploaded = false;
    if (payload_len) {
        if (int rc = h->stage.link_meta.reserve(h, 4ull * n_frames)) return rc;
        HIP_TRY(h, hipMemcpyAsync(h->stage.link_meta.p, payload_len, 4ull * n_frames, hipMemcpyHostToDevice, h->stream));
        a.len = h->stage.link_meta.as<const uint32_t>();
        uploaded = true;
    }
    a.payload = payload;
    if (payload && !payload_on_device && payload_extent) {
        if (int rc = h->stage.link_payload.reserve(h, payload_extent)) return rc;
        HIP_TRY(h, hipMemcpyAsync(h->stage.link_payload.p, payload, payload_extent, hipMemcpyHostToDevice, h->stream));
        a.payload = h->stage.link_payload.as<const uint8_t>();
        uploaded = true;
    }
    // the caller's host arrays may go once this returns: wait for the copies, not for the kernel
    if (uploaded) HIP_TRY(h, hipStreamSynchronize(h->stream));

    // the reference's flowgraphs: src 0x23.., dst 0x42.., bss 0xff.. (gnu_radio/IRS_user.py:192); addr1 = dst, addr2 = src, addr3 = bss
    uint8_t hdr[24] = { 0x08, 0x00, 0x00, 0x00, 0x42, 0x42, 0x42, 0x42, 0x42, 0x42, 0x23, 0x23, 0x23, 0x23, 0x23, 0x23,
                        0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0x00, 0x00 };
    if (addr) std::memcpy(hdr + 4, addr, 18);
    std::memcpy(a.hdr, hdr, 24);
    a.psdu = psdu;
    a.seed = payload_seed;
    a.payload_stride = payload_stride;
    a.psdu_stride = psdu_stride;
    a.len_all = payload_len ? 0 : payload_stride;
    a.len_max = len_max;
    a.n_frames = n_frames;
    a.seq0 = seq0;
    wr_mac_geometry(28 + len_max, &a.pitch, &a.fpb);
    HIP_TRY(h, wr_launch_mac(h->stream, &a));
    return WIFIRX_OK;
}

namespace {

// both scoring entry points: the totals into `counts` (if given), the counters per reference encoding into by_rate[8] (if given)
int link_stats_impl(wifirx_handle* h, uint32_t n_slots, const wifirx_out* rx, const wifirx_out* ref, uint32_t* frame_err,
                    uint8_t* frame_class, wifirx_link_counts* counts, wifirx_link_counts* by_rate)
{
    if (!rx->frames || !ref->frames) return fail(h, WIFIRX_EINVAL, "rx->frames and ref->frames are required");
    if (!rx->on_device || !ref->on_device) return fail(h, WIFIRX_EINVAL, "rx and ref must be device buffers");
    if (reinterpret_cast<uintptr_t>(frame_err) & 3) return fail(h, WIFIRX_EINVAL, "frame_err must be 4-byte aligned");

    wr::LinkArgs a{};
    a.rx_frames = rx->frames;
    a.ref_frames = ref->frames;
    if (rx->psdu && ref->psdu) {
        a.rx_psdu = rx->psdu;
        a.ref_psdu = ref->psdu;
        a.rx_psdu_stride = rx->psdu_stride;
        a.ref_psdu_stride = ref->psdu_stride;
    }
    // the transmitted and the received decisions in the same form: the bit planes when both sides have them, else `idx`
    if (rx->hbits && ref->hbits) {
        a.rx_dec = rx->hbits;
        a.ref_dec = ref->hbits;
        a.dec_is_hbits = 1;
    } else if (rx->idx && ref->idx) {
        a.rx_dec = reinterpret_cast<const uint32_t*>(rx->idx);
        a.ref_dec = reinterpret_cast<const uint32_t*>(ref->idx);
    }
    if ((reinterpret_cast<uintptr_t>(a.rx_dec) | reinterpret_cast<uintptr_t>(a.ref_dec)) & 15)
        return fail(h, WIFIRX_EINVAL, "the idx / hbits buffers must be 16-byte aligned");
    a.dec_row_words = h->cfg.max_sym * 12;
    a.max_sym = h->cfg.max_sym;
    a.n_slots = n_slots;
    a.frame_err = frame_err;
    a.frame_class = frame_class;
    stream_worker_wait_idle(h);
    HIP_TRY(h, hipSetDevice(h->device));
    // totals | by_rate[8] in one device buffer: one zeroing, one copy back
    const size_t n_sets = by_rate ? 9 : 1;
    wifirx_link_counts got[9];
    if (int rc = h->stage.link_counts.reserve(h, n_sets * sizeof(wifirx_link_counts))) return rc;
    a.counts = h->stage.link_counts.as<unsigned long long>();
    a.by_rate = by_rate ? 1 : 0;
    HIP_TRY(h, hipMemsetAsync(h->stage.link_counts.p, 0, n_sets * sizeof(wifirx_link_counts), h->stream));
    HIP_TRY(h, wr_launch_link_stats(h->stream, &a, h->n_simd));
    HIP_TRY(h, hipMemcpyAsync(got, h->stage.link_counts.p, n_sets * sizeof(wifirx_link_counts), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (counts) *counts = got[0];
    if (by_rate) std::memcpy(by_rate, got + 1, 8 * sizeof(wifirx_link_counts));
    return WIFIRX_OK;
}

}  // namespace

extern "C" int wifirx_link_stats(wifirx_handle* h, uint32_t n_slots, const wifirx_out* rx, const wifirx_out* ref,
                                 uint32_t* frame_err, uint8_t* frame_class, wifirx_link_counts* counts)
{
    if (!h) return WIFIRX_EINVAL;
    if (!rx || !ref || !counts) return fail(h, WIFIRX_EINVAL, "rx, ref and counts are required");
    return link_stats_impl(h, n_slots, rx, ref, frame_err, frame_class, counts, nullptr);
}

extern "C" int wifirx_link_stats_by_rate(wifirx_handle* h, uint32_t n_slots, const wifirx_out* rx, const wifirx_out* ref,
                                         uint32_t* frame_err, uint8_t* frame_class, wifirx_link_counts* total,
                                         wifirx_link_counts* by_rate)
{
    if (!h) return WIFIRX_EINVAL;
    if (!rx || !ref || !by_rate) return fail(h, WIFIRX_EINVAL, "rx, ref and by_rate are required");
    return link_stats_impl(h, n_slots, rx, ref, frame_err, frame_class, total, by_rate);
}
