"""The wideband loop on the device: per channel wifirx_tx_batch and wifirx_channel make the narrowband rows, wifirx_combine
joins them (NUMERICS.md rule 22), wifirx_iq_from_f32 quantises to sc16, wifirx_channelize splits them again and M streams
receive them.  The narrowband rows are downloaded and are the reference chain's input (tests/combine_ref.py, convert_ref.py,
channelizer_ref.py, the oracle), so the device noise generator's tolerance never enters: everything behind them is equal bit
for bit."""
import numpy as np
import pytest

import channelizer_ref as zr
import combine_ref as cb
import convert_ref as cr
import wideband_scene as ws
from wifirx import capi

pytestmark = pytest.mark.gpu

BW = 20e6
LEAD = 100


def run(M, s, seed):
    from oracle import oracle as orc
    chans, n = ws.layout(M, seed)
    freqs = [5.21e9 + zr.centre(k, M, s) * M * BW for k in range(M)]
    rx = capi.WifiRx(max_sym=1, device=0)
    chan_rx = []
    bufs = [rx.alloc(n * 8), rx.alloc(M * n * 8), rx.alloc(M * n * 8), rx.alloc(M * n * 4), rx.alloc(M * n * 8)]
    d_tx, d_rows, d_wide, d_q, d_ch = bufs
    try:
        # the narrowband rows: frames at their offsets, then one tap, the channel's CFO, 30 dB of gain and unit noise
        for k, frames in enumerate(chans):
            d_tx.upload(np.zeros(n, np.complex64))
            row_off = [f[0] - LEAD for f in frames] + [n]
            rx.tx_batch_dev(d_tx.ptr, n, [f[2].tobytes() for f in frames], frames[0][1], seeds=[f[3] for f in frames], lead=LEAD,
                            row_off=row_off)
            rx.channel_dev(d_tx.ptr, d_rows.ptr + 8 * k * n, n, 1, row_len=n, taps=(1.0,), cfo=frames[0][4],
                           gain=float(np.sqrt(10 ** (ws.SNR_DB / 10))), noise_voltage=1.0, seed=seed * 10 + k)
        u = d_rows.download(np.complex64, M * n).reshape(M, n)
        assert np.isfinite(u.view(np.float32)).all()
        # the reference chain on those rows
        wide = cb.combine(u, M, s)
        scale_q = cr.full_scale(wide, 12.0, cr.SC16)
        q, clipped = cr.quantise(cr.pairs(wide), scale_q, cr.SC16)
        scale = np.float32(1.0 / float(scale_q))
        rows = zr.analyse_format(q, cr.SC16, scale, M, s)
        # the device chain
        rx.combine_dev(d_rows.ptr, n, n, M, s, d_wide.ptr)
        got_clipped = rx.iq_from_f32_dev(d_wide.ptr, n * M, cr.SC16, d_q.ptr, scale=float(scale_q), count=True)
        rx.channelize_dev(d_q.ptr, cr.SC16, n, M, s, d_ch.ptr, n, scale=float(scale))
        rx.sync()                                             # the channels' handles read the rows on their own streams
        assert np.array_equal(d_wide.download(np.complex64, n * M).view(np.uint32), wide.view(np.uint32)), "the wide stream"
        assert got_clipped == clipped
        assert np.array_equal(d_q.download(np.int16, 2 * n * M).reshape(-1, 2), q)
        for k in range(M):
            r = capi.WifiRx(bandwidth=BW, frequency=freqs[k], max_sym=511)
            chan_rx.append(r)
            r._check(capi.lib().wifirx_push(r._h, d_ch.ptr + 8 * k * n, n, 1))
            r.flush()
            got = r.poll(cap=64, want_idx=True)
            prm = orc.make_params(bandwidth=BW, frequency=freqs[k], max_sym=511)
            o = orc.demod_stream(np.asarray(rows[k]), prm, cap=64)
            opsdu = orc.decode_batch(o["frames"], o["idx"], prm, psdu_stride=2048)
            assert np.array_equal(got["frames"], o["frames"]), k
            assert len(got["frames"]) == len(chans[k]) and ((got["frames"]["flags"] & capi.F_CRC_OK) != 0).all(), k
            for i, frame in enumerate(chans[k]):
                ns, L = int(got["frames"]["n_sym_out"][i]), int(got["frames"]["psdu_len"][i])
                assert np.array_equal(got["idx"][i, :ns], o["idx"][i, :ns]) and np.array_equal(got["psdu"][i, :L], opsdu[i, :L]), (k, i)
                assert L == len(frame[2]) and np.array_equal(got["psdu"][i, :L], frame[2]), (k, i)
    finally:
        for r in chan_rx:
            r.close()
        for b in bufs:
            b.free()
        rx.close()


def test_four_channels_odd_stacking():
    run(4, 1, seed=3)


def test_two_channels_even_stacking():
    run(2, 0, seed=4)
