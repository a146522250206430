#!/usr/bin/env python3
"""A recording of one 20 MHz channel made at another rate -- 25, 30.72, 40, 50, 61.44 or 80 MS/s, as many radios write it --
through `wifi_phy_rx_resampled`: the file's samples go to the device as they are, wifirx_arb_resample brings them to the
channel rate there (NUMERICS.md rule 34) and one receive chain publishes the PDUs.

    python examples/make_iq_file.py kodim01 cap25.sc16 --format sc16 --sample-rate 25e6 --pieces 200
    python examples/arb_file_rx.py cap25.sc16 --sample-rate 25e6 --format sc16 --scale S [--out out.png]

Prints the stream's counters; with --out the image pieces are drawn into a file.
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
    ap.add_argument("--bandwidth", type=float, default=20e6, help="of the channel: the rate the receiver runs at")
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
    img = np.zeros((300, 300, 3), np.uint8)
    pdus, drawn = [0], [0]

    def on_piece(data):
        app.redraw_image(app.load_piece(data), img)
        drawn[0] += 1

    def on_pdu(pdu):
        pdus[0] += 1

    rx = block.wifi_phy_rx_resampled(a.sample_rate, bandwidth=a.bandwidth, chan_est=a.chan_est, publish_carrier=False,
                                     sample_format=a.format, sample_scale=a.scale)
    grshim.msg_connect(rx, "mac_out", grshim.sink_block(on_pdu), "in")
    if a.out:
        grshim.msg_connect(rx, "mac_out", app.extract_pics(sink=on_piece), "MAC")
    grshim.run_stream(rx, x, chunk=a.chunk)
    st = rx.stats()
    print("%d samples at %.2f MS/s, ratio %d/%d -> %d samples at %.0f MS/s: frames detected %d, PDUs %d"
          % (len(x), a.sample_rate / 1e6, rx.num, rx.den, st["samples_in"], a.bandwidth / 1e6, st["frames_detected"], pdus[0]))
    rx.close()
    if a.out:
        from PIL import Image
        Image.fromarray(img).save(a.out)
        print("pieces drawn %d -> %s" % (drawn[0], a.out))


if __name__ == "__main__":
    main()
