#!/usr/bin/env python3
"""Survey a recording before tuning to it: `spectrum_probe` makes power rows of the file's samples on the device, in the file's
own format (wifirx_spectrum, NUMERICS.md rule 36), sums them over the candidate channels (wifirx_spectrum_bands), the host
decides which candidates are busy (`spectrum.busy_channels`), and `wifi_phy_rx_tuned` is opened on those alone.

    python examples/make_iq_file.py kodim01 band.sc16 --format sc16 --sample-rate 80e6 --offsets=-25e6,25e6 --pieces 300
    python examples/scan_tuned_file_rx.py band.sc16 --sample-rate 80e6 --candidates=-25e6,0,25e6 --format sc16 --scale S

Prints the band powers' range per candidate, the busy centres, and the counters of the channels received.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gnuradio-wifi-imagetransfer_amd"))
from wifirx import block, grshim, spectrum  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("iq")
    ap.add_argument("--sample-rate", type=float, required=True, help="of the file, in samples per second")
    ap.add_argument("--candidates", default="-25e6,0,25e6", help="comma-separated candidate centres in Hz above the capture's centre")
    ap.add_argument("--center-frequency", type=float, default=2.437e9)
    ap.add_argument("--bandwidth", type=float, default=20e6, help="of a channel: the candidates' width and the receivers' rate")
    ap.add_argument("--n-fft", type=int, default=256)
    ap.add_argument("--avg", type=int, default=4)
    ap.add_argument("--margin-db", type=float, default=10.0)
    ap.add_argument("--chunk", type=int, default=1 << 20)
    ap.add_argument("--format", choices=("fc32", "sc16", "sc8"), default="fc32")
    ap.add_argument("--scale", type=float, default=None, help="integer formats: value of one integer step")
    a = ap.parse_args()
    if a.format == "fc32":
        x = np.fromfile(a.iq, dtype=np.complex64)
    else:
        x = np.fromfile(a.iq, dtype=np.int16 if a.format == "sc16" else np.int8)
        x = x[:x.size // 2 * 2].reshape(-1, 2)
    candidates = [float(v) for v in a.candidates.split(",")]

    probe = block.spectrum_probe(a.sample_rate, n_fft=a.n_fft, avg=a.avg, offsets=candidates, width=a.bandwidth,
                                 center_frequency=a.center_frequency, sample_format=a.format, sample_scale=a.scale)
    grshim.run_stream(probe, x, chunk=a.chunk)
    rows = np.stack(probe.band_rows) if probe.band_rows else np.zeros((0, len(candidates)))
    busy = probe.busy_offsets(a.margin_db)
    probe.close()
    print("%d samples at %.2f MS/s: %d rows of %d bins" % (len(x), a.sample_rate / 1e6, len(rows), a.n_fft))
    for k, off in enumerate(candidates):
        if len(rows):
            db = spectrum.to_db(rows[:, k])
            print("candidate %+.1f MHz: %.1f .. %.1f dB%s" % (off / 1e6, db.min(), db.max(), "  busy" if off in busy else ""))
    if not busy:
        print("no busy channel")
        return
    pdus = [0] * len(busy)

    def on_pdu(pdu):
        meta, _ = grshim.to_python(pdu)
        pdus[meta["channel"]] += 1

    rx = block.wifi_phy_rx_tuned(a.sample_rate, offsets=busy, center_frequency=a.center_frequency, bandwidth=a.bandwidth,
                                 publish_carrier=False, sample_format=a.format, sample_scale=a.scale)
    grshim.msg_connect(rx, "mac_out", grshim.sink_block(on_pdu), "in")
    grshim.run_stream(rx, x, chunk=a.chunk)
    for k, st in enumerate(rx.stats()):
        print("channel %d at %.1f MHz: frames detected %d, PDUs %d" % (k, rx.frequencies[k] / 1e6, st["frames_detected"], pdus[k]))
    rx.close()


if __name__ == "__main__":
    main()
