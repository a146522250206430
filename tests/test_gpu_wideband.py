"""block.wifi_phy_rx_wideband: a wideband capture through the device's analysis bank and M receive chains publishes, per channel,
the PDUs of a wifi_phy_rx fed tests/channelizer_ref.py's samples for that channel -- whose records are the oracle's."""
import functools

import numpy as np
import pytest

import channelizer_ref as zr
import convert_ref as cr
from wifirx import block, capi, grshim, txgen

pytestmark = pytest.mark.gpu

BW = 20e6
SNR_DB = 30.0
CFO_MAX = 2e-5 * 5.2e9 / 20e6 * 2 * np.pi          # 20 ppm, rad per channel sample


@functools.lru_cache(maxsize=None)
def scene(M, s, fmt, seed):
    """(samples in the format, scale, PSDUs per channel, rule-21 rows of the reference [M, n]): two frames per channel, one
    encoding per channel, PSDU lengths and gaps that fit no grid, noise of unit variance per channel bandwidth"""
    rng = np.random.default_rng(seed)
    encs = (0, 3, 5, 7, 2, 4, 6, 1)[:M]
    plens = ((61, 135), (77, 203), (93, 58), (149, 111), (64, 65), (66, 67), (68, 69), (70, 71))[:M]
    streams, psdus = [], []
    for k in range(M):
        parts = [np.zeros(1237 + 211 * k + int(rng.integers(0, 97)), np.complex128)]
        mine = []
        for j, plen in enumerate(plens[k]):
            psdu = txgen.make_psdus(1, plen, seed=seed * 100 + 10 * k + j, seq0=j)
            tx = txgen.encode_psdus(psdu, encs[k], seeds=[1 + 2 * k + j])
            cfo = rng.uniform(-CFO_MAX, CFO_MAX)
            sig = tx.samples[0] * np.exp(1j * cfo * np.arange(tx.samples.shape[1])) * np.sqrt(10 ** (SNR_DB / 10))
            parts += [sig, np.zeros(901 + 173 * j + 59 * k + int(rng.integers(0, 131)), np.complex128)]
            mine.append(psdu[0])
        streams.append(np.concatenate(parts))
        psdus.append(tuple(mine))
    n = max(len(v) for v in streams) + 333
    streams = [np.concatenate([v, np.zeros(n - len(v), np.complex128)]) for v in streams]
    wide = zr.synthesise(streams, M, s)
    wide = wide + (rng.standard_normal(n * M) + 1j * rng.standard_normal(n * M)) * np.sqrt(0.5 * M)
    x = wide.astype(np.complex64)
    if fmt == cr.FC32:
        q, scale = cr.pairs(x), 1.0
    else:
        scale_q = cr.full_scale(x, 12.0, fmt)
        q, _ = cr.quantise(cr.pairs(x), scale_q, fmt)
        scale = np.float32(1.0 / float(scale_q))
    rows = zr.analyse_format(q, fmt, scale, M, s)
    q.setflags(write=False)
    rows.setflags(write=False)
    return q, scale, tuple(psdus), rows


def run_wideband(M, s, fmt, q, scale, chunk):
    pdus = []
    blk = block.wifi_phy_rx_wideband(M, s, 5.21e9, bandwidth=BW, sample_format=fmt, sample_scale=scale, publish_carrier=False,
                                     batch_samples=8192)
    try:
        grshim.msg_connect(blk, "mac_out", grshim.sink_block(pdus.append), "in")
        items = q if fmt != cr.FC32 else cr.to_complex(q)
        assert grshim.run_stream(blk, items, chunk=chunk) == len(items)
        return pdus, blk.frequencies, blk.stats()
    finally:
        blk.close()


def run_single(samples, frequency):
    pdus = []
    blk = block.wifi_phy_rx(bandwidth=BW, frequency=frequency, publish_carrier=False, batch_samples=8192)
    try:
        grshim.msg_connect(blk, "mac_out", grshim.sink_block(pdus.append), "in")
        assert grshim.run_stream(blk, samples, chunk=4096) == len(samples)
        return pdus, blk.stats()
    finally:
        blk.close()


def stream_records(samples, frequency):
    """the same samples through wifirx_push on a handle of their own: records and PSDUs"""
    rx = capi.WifiRx(bandwidth=BW, frequency=frequency, max_sym=511)
    try:
        rx.push(samples)
        rx.flush()
        return rx.poll(cap=64, want_idx=True)
    finally:
        rx.close()


def check(M, s, fmt, chunk, seed):
    from oracle import oracle as orc
    q, scale, psdus, rows = scene(M, s, fmt, seed)
    got, freqs, stats = run_wideband(M, s, fmt, q, scale, chunk or len(q))
    assert freqs == [5.21e9 + zr.centre(k, M, s) * M * BW for k in range(M)]
    for k in range(M):
        mine = [(m, b) for m, b in got if m["channel"] == k]
        want, st = run_single(rows[k], freqs[k])
        assert len(mine) == len(want) == len(psdus[k]), (k, len(mine), len(want))
        assert stats[k] == st, k
        for (gm, gb), (wm, wb), p in zip(mine, want, psdus[k]):
            assert gm == dict(wm, channel=k) and gm["freq"] == freqs[k], k
            assert np.array_equal(gb, wb) and np.array_equal(gb, p[:-4]), k
        # and the records of those samples are the oracle's
        prm = orc.make_params(bandwidth=BW, frequency=freqs[k], max_sym=511)
        o = orc.demod_stream(np.asarray(rows[k]), prm, cap=64)
        opsdu = orc.decode_batch(o["frames"], o["idx"], prm, psdu_stride=2048)
        r = stream_records(np.asarray(rows[k]), freqs[k])
        assert np.array_equal(r["frames"], o["frames"]), k
        assert ((r["frames"]["flags"] & capi.F_CRC_OK) != 0).all() and len(r["frames"]) == len(psdus[k]), k
        for i in range(len(r["frames"])):
            ns, L = int(r["frames"]["n_sym_out"][i]), int(r["frames"]["psdu_len"][i])
            assert np.array_equal(r["idx"][i, :ns], o["idx"][i, :ns]) and np.array_equal(r["psdu"][i, :L], opsdu[i, :L]), (k, i)


def test_four_channels_sc16_in_work_chunks():
    check(4, 1, cr.SC16, 8192, seed=3)


def test_two_channels_even_stacking_fc32_in_one_chunk():
    check(2, 0, cr.FC32, None, seed=4)
