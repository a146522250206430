"""The receive resampler in front of the receiver, on the device: a wifirx_tx_batch stream taken up to a capture rate and down
again by wifirx_arb_resample decodes to the transmitted PSDUs (float32, and sc16 through the device quantiser);
block.wifi_phy_rx_resampled publishes the PDUs of a wifi_phy_rx fed tests/arb_ref.py's samples; block.arb_resampler in
chunks equals WifiRx.arb_resample of the whole stream."""
import numpy as np
import pytest

import arb_ref as ar
import convert_ref as cr
from wifirx import block, capi, grshim, txgen

pytestmark = pytest.mark.gpu

BW = 20e6
N_FRAMES, PLEN, ENC, LEAD, TAIL = 16, 1000, 7, 160, 240


def loop(up, down, fmt):
    """16 frames of 64-QAM 3/4 built on the device, no noise: `up` then `down` (through `fmt` in between), then
    wifirx_push(iq_on_device = 1); returns (transmitted PSDUs, poll() of the stream)"""
    psdus = txgen.make_psdus(N_FRAMES, PLEN, seed=91)
    row = LEAD + txgen.frame_samples(PLEN, ENC) + TAIL
    n = N_FRAMES * row
    n_up = ar.count(up[0], up[1], 0, n, 0)
    n_back = ar.count(down[0], down[1], 0, n_up, 0)
    rx = capi.WifiRx(bandwidth=BW, max_sym=txgen.n_sym_for(PLEN, ENC))
    bufs = [rx.alloc(n * 8), rx.alloc(n_up * 8), rx.alloc(n_up * 4), rx.alloc(n_back * 8)]
    d_tx, d_up, d_q, d_back = bufs
    try:
        rx.tx_batch_dev(d_tx.ptr, n, psdus, ENC, lead=LEAD, row_len=row)
        assert rx.arb_resample_dev(d_tx.ptr, "fc32", n, up[0], up[1], d_up.ptr, n_up) == n_up
        if fmt == "fc32":
            got = rx.arb_resample_dev(d_up.ptr, "fc32", n_up, down[0], down[1], d_back.ptr, n_back)
        else:
            # full scale 8 times the frames' unit RMS: nothing clips
            assert rx.iq_from_f32_dev(d_up.ptr, n_up, fmt, d_q.ptr, scale=4096.0, count=True) == 0
            got = rx.arb_resample_dev(d_q.ptr, fmt, n_up, down[0], down[1], d_back.ptr, n_back, scale=1.0 / 4096.0)
        assert got == n_back
        rx.sync()                                             # device input: the producer has finished
        rx._check(capi.lib().wifirx_push(rx._h, d_back.ptr, n_back, 1))
        rx.flush()
        return psdus, rx.poll(cap=64)
    finally:
        for b in bufs:
            b.free()
        rx.close()


def check_loop(up, down, fmt):
    psdus, r = loop(up, down, fmt)
    assert len(r["frames"]) == N_FRAMES
    assert ((r["frames"]["flags"] & capi.F_CRC_OK) != 0).all()
    assert (r["frames"]["psdu_len"] == PLEN).all() and (r["frames"]["encoding"] == ENC).all()
    assert np.array_equal(r["psdu"][:, :PLEN], psdus)


def test_device_loop_through_25_msps():
    check_loop((4, 5), (5, 4), "fc32")


def test_device_loop_through_30_72_msps_as_sc16():
    check_loop((125, 192), (192, 125), "sc16")


# ---- the blocks -----------------------------------------------------------------------------------------------------------

def capture_25():
    """a 25 MS/s capture of three frames at 20 MHz with noise, and rule 34's 20 MS/s samples of it behind the flush zeros"""
    rng = np.random.default_rng(92)
    parts = [np.zeros(1237, np.complex128)]
    psdus = []
    for j, (enc, plen) in enumerate(((7, 611), (2, 135), (5, 1000))):
        psdu = txgen.make_psdus(1, plen, seed=920 + j, seq0=j)
        tx = txgen.encode_psdus(psdu, enc, seeds=[3 + j])
        cfo = rng.uniform(-0.03, 0.03)
        parts += [tx.samples[0] * np.exp(1j * cfo * np.arange(tx.samples.shape[1])) * np.sqrt(10 ** 3.0), np.zeros(901 + 173 * j, np.complex128)]
        psdus.append(psdu[0])
    x = np.concatenate(parts)
    x = x + (rng.standard_normal(len(x)) + 1j * rng.standard_normal(len(x))) * np.sqrt(0.5)
    cap = ar.stream(x.astype(np.complex64), 4, 5, n_out=len(x) * 5 // 4)
    flushed = np.concatenate([cap, np.zeros(20, np.complex64)])           # stop(): ceil(16 S / den) zeros
    want = cr.to_complex(ar.resample(cr.pairs(flushed), 5, 4))
    return cap, want, psdus


def run_block(blk, items, chunk):
    pdus = []
    try:
        grshim.msg_connect(blk, "mac_out", grshim.sink_block(pdus.append), "in")
        assert grshim.run_stream(blk, items, chunk=chunk) == len(items)
        return pdus, blk.stats()
    finally:
        blk.close()


def test_resampled_receiver_publishes_what_the_receiver_makes_of_the_rules_samples():
    cap, want, psdus = capture_25()
    ref, ref_stats = run_block(block.wifi_phy_rx(bandwidth=BW, publish_carrier=False, batch_samples=8192), want, 4096)
    assert len(ref) == len(psdus)
    for chunk in (8192, 1000):
        blk = block.wifi_phy_rx_resampled(sample_rate=25e6, bandwidth=BW, publish_carrier=False, batch_samples=8192)
        assert (blk.num, blk.den) == (5, 4)
        got, stats = run_block(blk, cap, chunk)
        assert len(got) == len(ref), chunk
        assert stats == ref_stats, chunk
        for (gm, gb), (wm, wb), p in zip(got, ref, psdus):
            assert gm == wm, chunk
            assert np.array_equal(gb, wb) and np.array_equal(gb, p[:-4]), chunk


@pytest.mark.parametrize("rates,fmt", [((25e6, 20e6), "fc32"), ((20e6, 30.72e6), "sc16"), ((80e6, 20e6), "sc8")])
def test_resampler_block_in_chunks_is_the_whole_stream(rates, fmt):
    rng = np.random.default_rng(93)
    n = 20000
    if fmt == "fc32":
        x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    else:
        info = np.iinfo(capi.IQ_DTYPE[capi.IQ_FORMATS[fmt]])
        x = rng.integers(info.min, info.max + 1, (n, 2)).astype(capi.IQ_DTYPE[capi.IQ_FORMATS[fmt]])
    num, den = capi.arb_ratio(*rates)
    rx = capi.WifiRx(max_sym=1)
    blk = block.arb_resampler(rates[0], rates[1], sample_format=fmt)
    try:
        assert (blk.num, blk.den) == (num, den)
        whole = rx.arb_resample(x, num, den, fmt=fmt)
        parts, pos, room = [], 0, np.empty(700, np.complex64)
        for chunk in (1, 3, 1000, 64, 8192) * 50:
            if pos >= n:
                break
            made = blk.work([x[pos:pos + chunk]], [room])
            assert made <= len(room) and 0 < blk.consumed <= chunk
            parts.append(room[:made].copy())
            pos += blk.consumed
        assert pos == n
        got = np.concatenate(parts)
        assert got.shape == whole.shape and np.array_equal(got.view(np.uint32), whole.view(np.uint32))
        blk.stop()
        total = len(got) + len(blk.tail)
        assert total == ar.count(num, den, 0, n + -((-16 * max(num, den)) // den), 0) >= n * den // num
        flushed = rx.arb_resample(x, num, den, fmt=fmt, n_out=total)
        assert np.array_equal(np.concatenate([got, blk.tail]).view(np.uint32), flushed.view(np.uint32))
    finally:
        blk.close()
        rx.close()
