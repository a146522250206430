#!/usr/bin/env python3
"""TX side of BASELINE.json config 1 without an SDR: image -> pieces in the reference's wire format
(upload_image_udp.py:19-34) -> ieee802_11.mac framing -> 802.11a frames (wifirx.txgen, CPU) -> x0.5 gain and
packet_pad2(100, 1000) as in gnu_radio/IRS_user.py:193-196 -> unit-variance AWGN at the given SNR ->
interleaved float32 I/Q file (GNU Radio file_sink format) that examples/irs_ap_file_rx.py receives.  With --format sc16 / sc8
the samples are quantised on the host (NUMERICS.md rule 20) with full scale --backoff-db above their RMS and written as
int16 / int8 pairs: a UHD sc16 recording, or what hackrf_transfer writes; the scale that widens them again is printed.

    python examples/make_iq_file.py image.png out.c64 [--encoding 0] [--snr 20] [--pieces 1000]
    python examples/make_iq_file.py kodim01 out.sc8 --format sc8 --backoff-db 12
    python examples/make_iq_file.py kodim01 wide.sc16 --format sc16 --channels 4 [--stacking 1]
    python examples/make_iq_file.py kodim01 cap25.sc16 --format sc16 --sample-rate 25e6
    python examples/make_iq_file.py kodim01 band.sc16 --format sc16 --sample-rate 80e6 --offsets=-25e6,0,25e6

--channels M (2, 4 or 8): a wideband capture at M times the channel rate for examples/wideband_file_rx.py.  The frames are
dealt round-robin to M streams (frame k goes to channel k mod M), every stream is up-sampled by M with a float64 FFT, shifted
to its channel's centre and the streams are summed (txgen.synthesise_wideband, NUMERICS.md rule 21); the noise then has unit
variance per channel bandwidth, so --snr means per channel what it means without --channels.

--sample-rate R (one channel): a capture at R samples per second of the 20 MS/s stream, for examples/arb_file_rx.py -- 25e6,
30.72e6, 40e6, 61.44e6, 80e6, or any rate whose ratio to 20e6 capi.arb_ratio takes.  The stream is up-sampled by NUMERICS.md
rule 34, on the device (wifirx_arb_resample) when the library finds one and by the rule's NumPy restatement
(tests/arb_ref.py) otherwise: the two give the same bytes.  The noise is added at the capture rate with unit variance per
20 MHz, so --snr keeps its meaning.

--offsets F0,F1,.. (with --sample-rate R): up to 8 channels centred F0, F1, .. Hz above the capture's centre, for
examples/tuned_file_rx.py -- channels 1 / 6 / 11 of the 2.4 GHz band around 2437 MHz are --sample-rate 80e6
--offsets=-25e6,0,25e6.  The frames are dealt round-robin to the channels, every stream is up-sampled to R as above, mixed to
its offset in float64 and the streams are summed; |offset| + 10 MHz must stay inside R / 2.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gnuradio-wifi-imagetransfer_amd"))
from wifirx import app, capi, txgen  # noqa: E402


def upsample(x, rate, bandwidth=20e6):
    """the complex64 stream x at `bandwidth` samples per second -> at `rate`, by NUMERICS.md rule 34, flushed with zeros so
    that every instant of x comes out"""
    num, den = capi.arb_ratio(bandwidth, rate)
    n_out = len(x) * den // num
    try:
        rx = capi.WifiRx(max_sym=1)
    except capi.WifiRxError:
        rx = None
    if rx is not None:
        try:
            print("rule 34 on the device: %d/%d" % (num, den))
            return rx.arb_resample(x, num, den, n_out=n_out)
        finally:
            rx.close()
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import arb_ref
    import convert_ref
    print("rule 34 by tests/arb_ref.py (no device): %d/%d" % (num, den))
    v = convert_ref.pairs(np.concatenate([x, np.zeros(arb_ref.flush_inputs(num, den, len(x), n_out), np.complex64)]))
    hist, j0, m0, parts = None, 0, 0, []
    for a in range(0, len(v), 1 << 18):                       # in calls of 2^18 samples: the same bytes, less memory
        piece = v[a:a + (1 << 18)]
        y = arb_ref.resample(piece, num, den, hist, j0, m0)
        hist, j0, m0 = arb_ref.next_history(piece, hist, num, den), j0 + len(piece), m0 + len(y)
        parts.append(y)
    return convert_ref.to_complex(np.concatenate(parts))[:n_out]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("image", help="PNG/JPEG (resized to 300x300 like the reference) or 'kodim01'..'kodim23' from tests/golden")
    ap.add_argument("out")
    ap.add_argument("--encoding", type=int, default=0)
    ap.add_argument("--snr", type=float, default=20.0)
    ap.add_argument("--pieces", type=int, default=0, help="first N pieces only (0 = all 2700)")
    ap.add_argument("--format", choices=("fc32", "sc16", "sc8"), default="fc32")
    ap.add_argument("--backoff-db", type=float, default=12.0, help="integer formats: full scale above the RMS of the samples")
    ap.add_argument("--channels", type=int, choices=(1, 2, 4, 8), default=1, help="adjacent channels in one wideband capture")
    ap.add_argument("--stacking", type=int, choices=(0, 1), default=1, help="--channels: 1 = centres at odd multiples of half the "
                    "channel width, 0 = at whole multiples")
    ap.add_argument("--sample-rate", type=float, default=None, help="one channel: the capture's rate in samples per second "
                    "(default: the channel's 20e6)")
    ap.add_argument("--offsets", default=None, help="with --sample-rate: comma-separated centres of up to 8 channels in Hz above "
                    "the capture's centre; the frames are dealt round-robin to them")
    a = ap.parse_args()
    if a.sample_rate is not None and a.channels != 1:
        ap.error("--sample-rate is for one channel")
    offsets = [float(v) for v in a.offsets.split(",")] if a.offsets else []
    if offsets and (a.sample_rate is None or a.channels != 1):
        ap.error("--offsets needs --sample-rate and no --channels")
    if len(offsets) > capi.TUNE_MAX_CHANNELS or any(abs(f) + 10e6 > (a.sample_rate or 0) / 2 for f in offsets):
        ap.error("--offsets: at most 8 channels, each with |offset| + 10 MHz inside half the sample rate")
    gold = os.path.join(ROOT, "tests", "golden", "kodim_300.npz")
    if os.path.exists(a.image):
        from PIL import Image
        img = np.array(Image.open(a.image).convert("RGB").resize((300, 300)), dtype=np.uint8)
    else:
        img = np.load(gold)[a.image]
    pieces = app.detach_image_sorted(img)
    if a.pieces:
        pieces = pieces[:a.pieces]
    payloads = [app.pack_piece(p) for p in pieces]
    groups = {}
    for k, p in enumerate(payloads):
        groups.setdefault(len(p), []).append(k)
    bursts = [None] * len(payloads)
    g = np.float32(np.sqrt(10 ** (a.snr / 10)))
    for _, ks in groups.items():
        psdus = np.stack([np.frombuffer(txgen.mac_frame(payloads[k], seq=k), dtype=np.uint8) for k in ks])
        tx = txgen.encode_psdus(psdus, a.encoding, seeds=[(k % 127) + 1 for k in ks])
        for row, k in enumerate(ks):
            bursts[k] = tx.samples[row] * g
    M = a.channels
    padded = [np.concatenate([np.zeros(100, np.complex64), b, np.zeros(1000, np.complex64)]) for b in bursts]
    rng = np.random.default_rng(0)
    if M == 1:
        x = np.concatenate(padded)
    else:
        streams = [np.concatenate(padded[k::M] or [np.zeros(0, np.complex64)]) for k in range(M)]
        n = max(len(v) for v in streams)
        x = txgen.synthesise_wideband([np.concatenate([v, np.zeros(n - len(v), np.complex64)]) for v in streams], M, a.stacking)
    over = 1.0                                                # the capture's rate over the channel's
    if offsets:
        streams = [np.concatenate(padded[k::len(offsets)] or [np.zeros(0, np.complex64)]) for k in range(len(offsets))]
        n = max(len(v) for v in streams)
        x = 0.0
        for v, f in zip(streams, offsets):
            up = upsample(np.concatenate([v, np.zeros(n - len(v), np.complex64)]).astype(np.complex64), a.sample_rate)
            x = x + up.astype(np.complex128) * np.exp(2j * np.pi * np.mod(f / a.sample_rate * np.arange(len(up)), 1.0))
        over = a.sample_rate / 20e6
    elif a.sample_rate is not None and a.sample_rate != 20e6:
        x = upsample(np.asarray(x, dtype=np.complex64), a.sample_rate)
        over = a.sample_rate / 20e6
    x = (x + (rng.standard_normal(x.size) + 1j * rng.standard_normal(x.size)) * np.sqrt(0.5 * M * over)).astype(np.complex64)
    if a.format != "fc32":
        scale = txgen.iq_full_scale(x, a.backoff_db, a.format)
        q, clipped = txgen.quantise_iq(x, a.format, scale)
        q.tofile(a.out)
        print("%s, full scale %.1f dB above the RMS: %d of %d components clipped; receive with --format %s --scale %.9g"
              % (a.format, a.backoff_db, clipped, q.size, a.format, 1.0 / float(scale)))
        x = q
    else:
        x.tofile(a.out)
    print("%d frames, %d samples (%.1f MB) -> %s" % (len(bursts), len(x), x.nbytes / 1e6, a.out))


if __name__ == "__main__":
    main()
