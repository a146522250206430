#!/usr/bin/env python3
"""A wideband recording -- 2, 4 or 8 adjacent 20 MHz channels in one I/Q file, as a USRP at 40 / 80 / 160 MS/s writes it --
through `wifi_phy_rx_wideband`: the file's samples go to the device as they are, wifirx_channelize splits them there
(NUMERICS.md rule 21) and one receive chain per channel publishes its PDUs, each marked with its channel.

    python examples/make_iq_file.py kodim01 wide.sc16 --format sc16 --channels 4 --pieces 200
    python examples/wideband_file_rx.py wide.sc16 --channels 4 --format sc16 --scale S [--out out.png]

Prints the PDUs per channel; with --out the pieces of every channel are drawn into one image (make_iq_file.py deals the
frames of one image round-robin to the channels).
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
    ap.add_argument("--channels", type=int, choices=(2, 4, 8), default=4)
    ap.add_argument("--stacking", type=int, choices=(0, 1), default=1)
    ap.add_argument("--center-frequency", type=float, default=5.21e9)
    ap.add_argument("--bandwidth", type=float, default=20e6, help="of one channel; the file is sampled at channels times this")
    ap.add_argument("--chan-est", type=int, default=block.LS)
    ap.add_argument("--chunk", type=int, default=1 << 20)
    ap.add_argument("--format", choices=("fc32", "sc16", "sc8"), default="fc32")
    ap.add_argument("--scale", type=float, default=None, help="integer formats: value of one integer step")
    ap.add_argument("--dc-block", action="store_true", help="DC removal on every channel stream, behind the bank (NUMERICS.md rule 32)")
    ap.add_argument("--iq-correct", action="store_true", help="blind IQ-imbalance correction on every channel stream (NUMERICS.md rule 32)")
    ap.add_argument("--out", default=None, help="draw the image pieces of all channels into this file")
    a = ap.parse_args()
    if a.format == "fc32":
        x = np.fromfile(a.iq, dtype=np.complex64)
    else:
        x = np.fromfile(a.iq, dtype=np.int16 if a.format == "sc16" else np.int8)
        x = x[:x.size // 2 * 2].reshape(-1, 2)
    img = np.zeros((300, 300, 3), np.uint8)
    per_channel = [0] * a.channels
    drawn = [0]

    def on_piece(data):
        app.redraw_image(app.load_piece(data), img)
        drawn[0] += 1

    pics = app.extract_pics(sink=on_piece)

    def on_pdu(pdu):
        per_channel[pdu[0]["channel"]] += 1

    rx = block.wifi_phy_rx_wideband(a.channels, a.stacking, a.center_frequency, bandwidth=a.bandwidth, chan_est=a.chan_est,
                                    publish_carrier=False, sample_format=a.format, sample_scale=a.scale, dc_block=a.dc_block,
                                    iq_correct=a.iq_correct)
    grshim.msg_connect(rx, "mac_out", grshim.sink_block(on_pdu), "in")
    if a.out:
        grshim.msg_connect(rx, "mac_out", pics, "MAC")
    grshim.run_stream(rx, x, chunk=a.chunk)
    for k, (st, f) in enumerate(zip(rx.stats(), rx.frequencies)):
        print("channel %d at %.1f MHz: samples %d, frames detected %d, PDUs %d" % (k, f / 1e6, st["samples_in"], st["frames_detected"], per_channel[k]))
    rx.close()
    if a.out:
        from PIL import Image
        Image.fromarray(img).save(a.out)
        print("pieces drawn %d -> %s" % (drawn[0], a.out))


if __name__ == "__main__":
    main()
