"""block.wifi_phy_rx_tuned: channels 1 / 6 / 11 out of one 80 MS/s capture through the device's tuner and three receive chains
publish, per channel, the PDUs of a wifi_phy_rx fed tests/tune_ref.py's samples for that channel; ``channel`` and ``freq`` are
in the dictionaries; the capture ends inside the resampler's delay of the last frame, so stop() delivers it."""
import functools

import numpy as np
import pytest

import arb_ref as ar
import convert_ref as cr
import tune_ref as tr
from wifirx import block, grshim

pytestmark = pytest.mark.gpu

BW, FC = 20e6, 2.437e9
ENC, PLEN, SNR_DB, N_FRAMES = 7, 300, 28.0, 2
FLUSH = 64                                                    # ceil(16 S / den) at 4/1


@functools.lru_cache(maxsize=None)
def scene(fmt):
    """(items in the format, scale, PSDUs per channel, rule 35's rows [3, n] behind the flush zeros).  The capture ends two
    channel samples behind the last frame of channel 2, which is rolled furthest: 14 of its samples are still inside the
    resampler when the capture is over"""
    wide, psdus, _ = tr.three_channel_scene(ENC, PLEN, SNR_DB, n_frames=N_FRAMES)
    wide = wide[:len(wide) - 4 * (240 - 200 - 2)]
    if fmt == cr.FC32:
        q, scale = cr.pairs(wide), 1.0
    else:
        scale_q = cr.full_scale(wide, 12.0, fmt)
        q, _ = cr.quantise(cr.pairs(wide), scale_q, fmt)
        scale = np.float32(1.0 / float(scale_q))
    flushed = np.concatenate([q, np.zeros((FLUSH, 2), q.dtype)])
    rows = tr.tune_format(flushed, fmt, scale, 4, 1, tr.scene_incs())
    rows = np.stack([cr.to_complex(r) for r in rows])
    q.setflags(write=False)
    rows.setflags(write=False)
    return q, scale, psdus, rows


def run_single(samples, frequency):
    pdus = []
    blk = block.wifi_phy_rx(bandwidth=BW, frequency=frequency, publish_carrier=False, batch_samples=8192)
    try:
        grshim.msg_connect(blk, "mac_out", grshim.sink_block(pdus.append), "in")
        assert grshim.run_stream(blk, samples, chunk=4096) == len(samples)
        return pdus, blk.stats()
    finally:
        blk.close()


@functools.lru_cache(maxsize=None)
def reference(fmt):
    q, scale, psdus, rows = scene(fmt)
    return [run_single(rows[k], FC + off) for k, off in enumerate(tr.SCENE_OFFSETS)]


@pytest.mark.parametrize("chunk", [8192, 1000])
@pytest.mark.parametrize("fmt", [cr.FC32, cr.SC16], ids=["fc32", "sc16"])
def test_tuned_receiver_publishes_what_the_receiver_makes_of_the_rules_samples(fmt, chunk):
    q, scale, psdus, rows = scene(fmt)
    assert rows.shape[1] == ar.count(4, 1, 0, len(q) + FLUSH, 0)
    want = reference(fmt)
    pdus = []
    blk = block.wifi_phy_rx_tuned(80e6, offsets=tr.SCENE_OFFSETS, center_frequency=FC, bandwidth=BW, sample_format=fmt,
                                  sample_scale=scale, publish_carrier=False, batch_samples=8192)
    try:
        assert (blk.num, blk.den) == (4, 1) and blk.incs == tr.scene_incs()
        assert blk.frequencies == [FC - 25e6, FC, FC + 25e6]
        grshim.msg_connect(blk, "mac_out", grshim.sink_block(pdus.append), "in")
        items = q if fmt != cr.FC32 else cr.to_complex(q)
        assert grshim.run_stream(blk, items, chunk=chunk, finish=False) == len(items)
        before = sum(1 for m, _ in pdus if m["channel"] == 2)
        blk.stop()
        stats = blk.stats()
    finally:
        blk.close()
    assert before < N_FRAMES                                  # the last frame's end was still inside the resampler
    for k in range(3):
        mine = [(m, b) for m, b in pdus if m["channel"] == k]
        ref, st = want[k]
        assert len(mine) == len(ref) == N_FRAMES, (k, len(mine), len(ref))
        assert stats[k] == st, k
        for (gm, gb), (wm, wb), p in zip(mine, ref, psdus[k]):
            assert gm == dict(wm, channel=k) and gm["freq"] == FC + tr.SCENE_OFFSETS[k], k
            assert np.array_equal(gb, wb) and np.array_equal(gb, p[:-4]), k
