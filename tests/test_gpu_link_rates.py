"""wifirx_link_stats_by_rate (wr_link.hip, link_stats_kernel<true>): the nine counters per encoding of the reference record,
against tests/rates_ref.py on the same buffers -- a hand-made batch that hits every class at every rate, and the device
loop-back over a batch that mixes the eight rates (wifirx_tx_batch_rates)."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import link_ref
import rates_ref
from wifirx import capi, txgen

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LEAD, TAIL, PSDU_LEN = 160, 240, 294
CFO_20PPM = 2 * np.pi * 20e-6 * 5.89e9 / 20e6


def upload_side(rx, side):
    d = {k: rx.alloc(v.nbytes).upload(v) for k, v in side.items() if v is not None}
    if "psdu" in d:
        d["psdu_stride"] = side["psdu"].shape[1]
    return d


def counters(d):
    return {k: d[k] for k in link_ref.COUNTERS}


def check(rx, n, d_rx, d_ref, h_rx, h_ref, max_sym):
    """device totals and by_rate == the host statement on the same buffers; totals == wifirx_link_stats; the sums hold"""
    r = rx.link_stats(n, d_rx, d_ref, by_rate=True)
    total, by_rate = rates_ref.link_stats_by_rate(h_rx, h_ref, max_sym)
    assert counters(r) == total
    assert counters(r) == counters(rx.link_stats(n, d_rx, d_ref))
    assert len(r["by_rate"]) == 8
    for e in range(8):
        assert counters(r["by_rate"][e]) == by_rate[e], e
        assert r["by_rate"][e]["frames"] == r["by_rate"][e]["frames_ref"]
    rates_ref.check_sums(counters(r), [counters(b) for b in r["by_rate"]])
    return r


def test_by_rate_hand_made():
    rng = np.random.default_rng(2027)
    n, max_sym = 6000, 16
    rx = capi.WifiRx(max_sym=max_sym, llr_bits=0, device=0)
    classes, enc = rng.integers(0, len(link_ref.CLASSES), n), rng.integers(0, 8, n)
    h_rx, h_ref = link_ref.hand_made_batch(rng, classes, enc, rng.choice([1, 7, max_sym], n), max_sym, rx_stride=64, ref_stride=59)
    d_rx, d_ref = upload_side(rx, h_rx), upload_side(rx, h_ref)
    pick = lambda d, *keys: {k: v for k, v in d.items() if k in keys or k in ("frames", "psdu_stride")}
    sub = lambda side, *keys: {k: (v if k in keys or k == "frames" else None) for k, v in side.items()}
    try:
        r = check(rx, n, d_rx, d_ref, h_rx, h_ref, max_sym)
        r2 = check(rx, n, pick(d_rx, "psdu", "idx"), pick(d_ref, "psdu", "idx"), sub(h_rx, "psdu", "idx"),
                   sub(h_ref, "psdu", "idx"), max_sym)
        assert [counters(b) for b in r["by_rate"]] == [counters(b) for b in r2["by_rate"]]
        incomplete = link_ref.CLASSES.index("ref_incomplete")
        for e in range(8):
            assert r["by_rate"][e]["frames"] == int(((enc == e) & (classes != incomplete)).sum())
            assert r["by_rate"][e]["coded_bit_errors"] > 0 and r["by_rate"][e]["frames_psdu_ok"] > 0
        # per-frame outputs are those of wifirx_link_stats; fewer frames than a workgroup's waves; total = NULL
        a = rx.link_stats(n, d_rx, d_ref, per_frame=True, by_rate=True)
        b = rx.link_stats(n, d_rx, d_ref, per_frame=True)
        try:
            for k in ("frame_err", "frame_class"):
                dt = np.uint32 if k == "frame_err" else np.uint8
                assert np.array_equal(a[k].download(dt, n), b[k].download(dt, n))
        finally:
            for x in (a, b):
                x["frame_err"].free()
                x["frame_class"].free()
        for m in (0, 1, 3):
            cut = lambda side: {k: v[:m] for k, v in side.items()}
            got = rx.link_stats(m, d_rx, d_ref, by_rate=True)
            total, by_rate = rates_ref.link_stats_by_rate(cut(h_rx), cut(h_ref), max_sym)
            assert counters(got) == total and [counters(x) for x in got["by_rate"]] == by_rate
        rates = (capi.LinkCounts * 8)()
        o_rx, o_ref = rx._out_struct(d_rx), rx._out_struct(d_ref)
        lib = capi.lib()
        assert lib.wifirx_link_stats_by_rate(rx._h, n, C.byref(o_rx), C.byref(o_ref), None, None, None, rates) == capi.OK
        assert [{k: int(getattr(rates[e], k)) for k in link_ref.COUNTERS} for e in range(8)] == [counters(x) for x in r["by_rate"]]
        assert lib.wifirx_link_stats_by_rate(rx._h, n, C.byref(o_rx), C.byref(o_ref), None, None, None, None) == capi.EINVAL
    finally:
        rx.free_out(d_rx)
        rx.free_out(d_ref)
        rx.close()


def test_by_rate_on_the_device_loop_back_at_20_db():
    """8 x 8192 frames of 294 bytes (wifirx_mac_batch), encodings cycling, row_off rows -> wifirx_tx_batch_rates ->
    wifirx_channel (sv_taps.npy sets, CFO in +-20 ppm, gain for 20 dB) -> demod (LS) + decode_mac; reference = the demod of the
    clean rows.  Device counters = the host bookkeeping of the downloaded buffers, with hbits and with idx only."""
    n, snr, seed = 8 * 8192, 20, 1
    enc = (np.arange(n) % 8).astype(np.uint8)
    flen = np.array([txgen.frame_samples(PSDU_LEN, e) for e in range(8)])
    assert flen.tolist() == [8321, 5681, 4401, 3041, 2401, 1761, 1441, 1281]
    max_sym = txgen.n_sym_for(PSDU_LEN, 0)
    assert max_sym == 99
    rows = LEAD + flen[enc] + TAIL
    rows += rows & 1
    row_off = np.concatenate([[0], np.cumsum(rows)]).astype(np.uint64)
    total = int(row_off[-1])
    taps = np.load(os.path.join(GOLD, "sv_taps.npy")).astype(np.complex64)
    rx = capi.WifiRx(max_sym=max_sym, llr_bits=0, chan_est=capi.EQ_LS, device=0)
    d_psdu, clean, iq = rx.alloc(n * PSDU_LEN), rx.alloc(total * 8), rx.alloc(total * 8)
    ref = rx.alloc_out(n, want_hbits=True)
    ref["psdu"], ref["psdu_stride"] = d_psdu, PSDU_LEN
    dev = rx.alloc_out(n, psdu_stride=304, want_hbits=True)
    try:
        rx.mac_batch_dev(d_psdu.ptr, PSDU_LEN, n, None, payload_len=PSDU_LEN - 28, payload_seed=seed)
        rx.tx_batch_dev(clean.ptr, total, d_psdu.ptr, enc, psdu_len=np.full(n, PSDU_LEN, np.uint32), psdu_stride=PSDU_LEN,
                        lead=LEAD, row_off=row_off)
        rx.demod_batch_var_dev(clean.ptr, row_off, ref)
        cfo = np.random.default_rng(1000 * snr + seed).uniform(-CFO_20PPM, CFO_20PPM, n).astype(np.float32)
        rx.channel_dev(clean.ptr, iq.ptr, total, n, row_off=row_off, taps=taps, cfo=cfo, gain=math.sqrt(10 ** (snr / 10)),
                       noise_voltage=1.0, seed=9000 + snr + (seed << 32))
        rx.demod_batch_var_dev(iq.ptr, row_off, dev)
        rx.decode_batch_dev(n, dev)
        rx.sync()
        h_ref, h_rx = rx.download_out(ref, n), rx.download_out(dev, n)
        assert ((h_ref["frames"]["flags"] & capi.F_COMPLETE) != 0).all()
        assert np.array_equal(h_ref["frames"]["encoding"], enc)
        r = check(rx, n, dev, ref, h_rx, h_ref, max_sym)
        pick = lambda d: {k: v for k, v in d.items() if k != "hbits"}
        r_idx = check(rx, n, pick(dev), pick(ref), pick(h_rx), pick(h_ref), max_sym)
        assert counters(r) == counters(r_idx) and [counters(b) for b in r["by_rate"]] == [counters(b) for b in r_idx["by_rate"]]
        for e in range(8):
            b = r["by_rate"][e]
            assert b["frames_ref"] == 8192, e
            print("encoding %d at %d dB: %s" % (e, snr, counters(b)))
        b7 = r["by_rate"][7]
        assert b7["frames_good"] > 0 and b7["frames_psdu_ok"] > 0 and b7["coded_bit_errors"] > 0
    finally:
        rx.free_out(dev)
        rx.free_out(ref)                                               # frees d_psdu with it
        clean.free()
        iq.free()
        rx.close()
