#!/usr/bin/env python3
"""A recording that holds several 20 MHz channels at centres of their own -- channels 1 / 6 / 11 of the 2.4 GHz band, 25 MHz
apart, in one 80 MS/s capture around 2437 MHz -- through `wifi_phy_rx_tuned`: the file's samples go to the device as they
are, one wifirx_tune per chunk mixes every channel down and brings it to the channel rate there (NUMERICS.md rule 35), and
one receive chain per channel publishes the PDUs.

    python examples/make_iq_file.py kodim01 band.sc16 --format sc16 --sample-rate 80e6 --offsets=-25e6,0,25e6 --pieces 300
    python examples/tuned_file_rx.py band.sc16 --sample-rate 80e6 --offsets=-25e6,0,25e6 --format sc16 --scale S [--out out.png]

Prints the counters per channel; with --out the image pieces of all channels are drawn into a file.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gnuradio-wifi-imagetransfer_amd"))
from wifirx import app, block, grshim  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("iq")
    ap.add_argument("--sample-rate", type=float, required=True, help="of the file, in samples per second")
    ap.add_argument("--offsets", default="-25e6,0,25e6", help="comma-separated channel centres in Hz above the capture's centre")
    ap.add_argument("--center-frequency", type=float, default=2.437e9)
    ap.add_argument("--bandwidth", type=float, default=20e6, help="of a channel: the rate the receivers run at")
    ap.add_argument("--chan-est", type=int, default=block.LS)
    ap.add_argument("--chunk", type=int, default=1 << 20)
    ap.add_argument("--format", choices=("fc32", "sc16", "sc8"), default="fc32")
    ap.add_argument("--scale", type=float, default=None, help="integer formats: value of one integer step")
    ap.add_argument("--out", default=None, help="draw the image pieces into this file")
    a = ap.parse_args()
    if a.format == "fc32":
        x = np.fromfile(a.iq, dtype=np.complex64)
    else:
        x = np.fromfile(a.iq, dtype=np.int16 if a.format == "sc16" else np.int8)
        x = x[:x.size // 2 * 2].reshape(-1, 2)
    offsets = [float(v) for v in a.offsets.split(",")]
    img = np.zeros((300, 300, 3), np.uint8)
    pdus, drawn = [0] * len(offsets), [0]

    def on_piece(data):
        app.redraw_image(app.load_piece(data), img)
        drawn[0] += 1

    def on_pdu(pdu):
        meta, _ = grshim.to_python(pdu)
        pdus[meta["channel"]] += 1

    rx = block.wifi_phy_rx_tuned(a.sample_rate, offsets=offsets, center_frequency=a.center_frequency, bandwidth=a.bandwidth,
                                 chan_est=a.chan_est, publish_carrier=False, sample_format=a.format, sample_scale=a.scale)
    grshim.msg_connect(rx, "mac_out", grshim.sink_block(on_pdu), "in")
    if a.out:
        grshim.msg_connect(rx, "mac_out", app.extract_pics(sink=on_piece), "MAC")
    grshim.run_stream(rx, x, chunk=a.chunk)
    print("%d samples at %.2f MS/s, ratio %d/%d, %d channels" % (len(x), a.sample_rate / 1e6, rx.num, rx.den, len(offsets)))
    for k, st in enumerate(rx.stats()):
        print("channel %d at %.1f MHz: %d samples, frames detected %d, PDUs %d"
              % (k, rx.frequencies[k] / 1e6, st["samples_in"], st["frames_detected"], pdus[k]))
    rx.close()
    if a.out:
        from PIL import Image
        Image.fromarray(img).save(a.out)
        print("pieces drawn %d -> %s" % (drawn[0], a.out))


if __name__ == "__main__":
    main()
