"""The band survey end to end on tests/spectrum_scene.py: the scene's margins on the restatement alone, the device's rows and
band powers bit for bit, spectrum.busy_channels finding exactly the two outer candidates, wifi_phy_rx_tuned opened on them
decoding every frame that it decodes when given the offsets by hand; and spectrum_probe publishing, for a stream pushed in
uneven chunks, the rows of one call on the whole stream."""
import numpy as np
import pytest

import spectrum_ref as sr
import spectrum_scene as sc
from bank_helpers import same_bits
from wifirx import block, capi, grshim, spectrum

pytestmark = pytest.mark.gpu

FC = 2.437e9


def db_above_floor(band_rows):
    """per band: its largest row over the lowest floor of all bands, in dB"""
    db = spectrum.to_db(band_rows)
    return db.max(axis=0) - db.min(axis=0).min()


def test_the_scene_is_not_marginal():
    """on the restatement alone: busy bands stand at least 15 dB above the floor, the idle band at most 5 dB"""
    rows, band_rows = sc.survey()
    assert rows.shape[0] >= 40 and sc.bands() == [(16, 80), (96, 160), (176, 240)]
    up = db_above_floor(band_rows)
    print("largest row above the floor, dB:", up)
    assert up[0] >= 15.0 and up[2] >= 15.0 and up[1] <= 5.0
    assert spectrum.busy_channels(band_rows, 10.0) == [0, 2]


@pytest.fixture(scope="module")
def rx():
    r = capi.WifiRx(max_sym=1, device=0)
    yield r
    r.close()


def test_device_rows_and_band_rows_equal_the_restatement(rx):
    q, scale, _ = sc.scene()
    rows, band_rows = sc.survey()
    got = rx.spectrum(q, sc.N_FFT, sc.HOP, sc.AVG, "blackman_harris", "sum", 1.0, fmt=sc.FMT, scale=float(scale))
    assert same_bits(got, rows)
    got_bands = rx.spectrum_bands(got, sc.bands())
    assert same_bits(got_bands, band_rows)
    assert [sc.CANDIDATES[k] for k in spectrum.busy_channels(got_bands, 10.0)] == list(sc.BUSY)
    # a Welch spectrum of the whole capture: the fold of all rows
    whole = rx.spectrum_fold(got, None, "sum")
    assert same_bits(whole, sr.fold(rows, rows.shape[0], sr.SUM))


def run_tuned(q, scale, offsets):
    pdus = []
    blk = block.wifi_phy_rx_tuned(sc.RATE, offsets=offsets, center_frequency=FC, sample_format=sc.FMT, sample_scale=float(scale),
                                  publish_carrier=False, batch_samples=8192)
    try:
        grshim.msg_connect(blk, "mac_out", grshim.sink_block(pdus.append), "in")
        assert grshim.run_stream(blk, q, chunk=8192) == len(q)
    finally:
        blk.close()
    return [grshim.to_python(m) for m in pdus]


def test_probe_then_tuned_receiver_decodes_every_frame(rx):
    q, scale, psdus = sc.scene()
    probe = block.spectrum_probe(sc.RATE, n_fft=sc.N_FFT, hop=sc.HOP, avg=sc.AVG, offsets=sc.CANDIDATES, width=sc.WIDTH,
                                 center_frequency=FC, sample_format=sc.FMT, sample_scale=float(scale), norm=1.0)
    try:
        assert grshim.run_stream(probe, q, chunk=5000) == len(q)
        busy = probe.busy_offsets(10.0)
        assert same_bits(np.stack(probe.band_rows), sc.survey()[1])
    finally:
        probe.close()
    assert busy == list(sc.BUSY)
    found, by_hand = run_tuned(q, scale, busy), run_tuned(q, scale, (-25e6, 25e6))
    for k, off in enumerate(sc.BUSY):
        mine = [(m, b) for m, b in found if m["channel"] == k]
        ref = [(m, b) for m, b in by_hand if m["channel"] == k]
        assert len(mine) == len(ref) == sc.N_FRAMES, (k, len(mine), len(ref))
        for (gm, gb), (wm, wb), p in zip(mine, ref, psdus[off]):
            assert gm == wm and gm["freq"] == FC + off
            assert np.array_equal(gb, wb) and np.array_equal(gb, p[:-4]), k


def test_probe_publishes_the_rows_of_one_call_on_the_whole_stream():
    q, scale, _ = sc.scene()
    q = q[:20000]
    n_fft, hop, avg = 256, 100, 3
    pdus = []
    probe = block.spectrum_probe(sc.RATE, n_fft=n_fft, hop=hop, avg=avg, window="hann", mode="max", offsets=(-25e6, 25e6),
                                 center_frequency=FC, sample_format=sc.FMT, sample_scale=float(scale))
    try:
        grshim.msg_connect(probe, "spectrum", grshim.sink_block(pdus.append), "in")
        pos = 0
        for n in (1, 255, 299, 300, 7, 4096, 1, 10000, 5041):
            assert probe.work([q[pos:pos + n]], []) == n
            pos += n
        assert pos == len(q)
        norm = probe.norm
        assert norm == spectrum.norm(n_fft, "hann", 1)
    finally:
        probe.close()
    want = sr.spectrum_format(q, sc.FMT, scale, n_fft, hop, avg, sr.HANN, sr.MAX, norm)
    msgs = [grshim.to_python(m) for m in pdus]
    assert len(msgs) == want.shape[0] == sr.count(n_fft, hop, avg, len(q))[0] > 50
    edges = [sr.band(off, 20e6, sc.RATE, n_fft) for off in (-25e6, 25e6)]
    band = sr.bands(want, edges)
    for r, (meta, vec) in enumerate(msgs):
        assert vec.dtype == np.float32 and same_bits(np.asarray(vec), want[r]), r
        assert meta["row_index"] == r and meta["n_fft"] == n_fft and meta["sample_rate"] == sc.RATE and meta["center_frequency"] == FC
        assert np.array_equal(meta["band_power_db"], spectrum.to_db(band[r]))
