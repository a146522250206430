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

--channels M (2, 4 or 8): a wideband capture at M times the channel rate for examples/wideband_file_rx.py.  The frames are
dealt round-robin to M streams (frame k goes to channel k mod M), every stream is up-sampled by M with a float64 FFT, shifted
to its channel's centre and the streams are summed (txgen.synthesise_wideband, NUMERICS.md rule 21); the noise then has unit
variance per channel bandwidth, so --snr means per channel what it means without --channels.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gnuradio-wifi-imagetransfer_amd"))
from wifirx import app, txgen  # noqa: E402


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
    a = ap.parse_args()
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
    x = (x + (rng.standard_normal(x.size) + 1j * rng.standard_normal(x.size)) * np.sqrt(0.5 * M)).astype(np.complex64)
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
