#!/usr/bin/env python3
"""Throughput of the drop-in path: wifi_phy_rx.work() fed with host chunks the way a GNU Radio scheduler feeds it.

    python tools/host_path_bench.py [frames=6000]

Two streams: config-2-like (QPSK-1/2, 294 B, one frame per 4608 samples) and config-1-like (BPSK-1/2, 294 B,
packet_pad2 gaps: 9420 samples per frame); work() chunk sizes 8192 / 32768 / 131072 items; batch sizes 2^20 / 2^22.
Prints one JSON line per case: Gsample/s through work() incl. PDU construction and a list-append consumer.

    python tools/host_path_bench.py --format [frames=6000] [--out profiles/host_path_formats.json]

--format: the same work() loop with fc32, sc16 and sc8 items (wifi_phy_rx(sample_format=...); the integer streams are the
float stream quantised on the host with full scale 12 dB above its RMS, NUMERICS.md rule 20), on the config-2-like stream with
batch 2^22 and chunks of 131072 items: three blocks in one process, five rounds alternating between them, the median of each
and its ratio to fc32.

    python tools/host_path_bench.py --wideband M [frames=600] [--format sc16] [--out profiles/host_path_wideband.json]

--wideband M: wifi_phy_rx_wideband.work() on a capture of M config-2-like streams synthesised on the host (float64 FFT
up-sampling, NUMERICS.md rule 21) and quantised to the format, in chunks of 524288 wideband items: wideband samples per second,
the median of five rounds, beside M times the single-channel figure recorded in profiles/host_path_formats.json."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gnuradio-wifi-imagetransfer_amd"))
from wifirx import block, grshim, txgen  # noqa: E402


def make_stream(enc, n_frames, period, lead, snr_db=20.0, seed=3):
    """snr_db None: the frames at unit power without noise (the wideband synthesis adds its own)"""
    tx = txgen.encode_psdus(txgen.make_psdus(64, 294, seed=seed), enc)
    flen = tx.samples.shape[1]
    assert lead + flen <= period
    g = np.float32(1.0 if snr_db is None else np.sqrt(10 ** (snr_db / 10)))
    x = np.zeros((n_frames, period), np.complex64)
    x[:, lead:lead + flen] = tx.samples[np.arange(n_frames) % 64] * g
    rng = np.random.default_rng(seed)
    x = x.reshape(-1)
    if snr_db is None:
        return x, tx.n_sym
    x += ((rng.standard_normal(x.size) + 1j * rng.standard_normal(x.size)) * np.sqrt(0.5)).astype(np.complex64)
    return x, tx.n_sym


def formats_main(argv):
    out = None
    if "--out" in argv:
        out = argv[argv.index("--out") + 1]
        argv = [v for i, v in enumerate(argv) if v != "--out" and (i == 0 or argv[i - 1] != "--out")]
    n_frames = int(argv[0]) if argv else 6000
    period, chunk, batch, rounds = 4608, 131072, 1 << 22, 5
    x, n_sym = make_stream(2, n_frames, period, 160)
    streams = {"fc32": (x, None)}
    for fmt in ("sc16", "sc8"):
        scale = txgen.iq_full_scale(x, 12.0, fmt)
        streams[fmt] = (txgen.quantise_iq(x, fmt, scale)[0], 1.0 / float(scale))
    blocks, got = {}, {}
    for fmt, (samples, scale) in streams.items():
        blocks[fmt] = block.wifi_phy_rx(bandwidth=20e6, frequency=5.89e9, max_sym=n_sym, publish_carrier=False, batch_samples=batch,
                                        sample_format=fmt, sample_scale=scale)
        got[fmt] = []
        grshim.msg_connect(blocks[fmt], "mac_out", grshim.sink_block(got[fmt].append), "in")
        grshim.run_stream(blocks[fmt], samples[:period * 300], chunk=chunk)           # warm-up
    n0 = {fmt: len(g) for fmt, g in got.items()}
    rate = {fmt: [] for fmt in streams}
    for _ in range(rounds):
        for fmt, (samples, _) in streams.items():
            t = time.perf_counter()
            grshim.run_stream(blocks[fmt], samples, chunk=chunk)
            rate[fmt].append(len(samples) / (time.perf_counter() - t) / 1e9)
    med = {fmt: float(np.median(v)) for fmt, v in rate.items()}
    res = {"workload": "wifi_phy_rx.work() on the config-2-like stream (QPSK 1/2, 294 B, one frame per 4608 samples, %d frames, 20 dB), "
                       "batch_samples 2^22, work() chunks of %d items; PDU construction and a list-append consumer included" % (n_frames, chunk),
           "method": "three blocks (fc32, sc16, sc8 items) in one process, %d rounds alternating between them, medians; the integer "
                     "streams are the float stream quantised on the host, full scale 12 dB above its RMS" % rounds,
           "host_bytes_per_sample": {"fc32": 8, "sc16": 4, "sc8": 2},
           "gsamples_per_s": med, "gsamples_per_s_rounds": rate, "ratio_to_fc32": {fmt: med[fmt] / med["fc32"] for fmt in med},
           "pdus_per_round": {fmt: (len(got[fmt]) - n0[fmt]) // rounds for fmt in got}, "frames": n_frames}
    print(json.dumps(res), flush=True)
    if out:
        with open(out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    for b in blocks.values():
        b.close()


def wideband_main(argv):
    def option(name, default):
        if name in argv:
            i = argv.index(name)
            value = argv[i + 1]
            del argv[i:i + 2]
            return value
        return default
    M = int(option("--wideband", "4"))
    out, fmt = option("--out", None), option("--format", "sc16")
    n_frames = int(argv[0]) if argv else 600
    period, chunk, batch, rounds, stacking = 4608, 524288, 1 << 22, 5, 1
    streams, n_sym = [], 0
    for k in range(M):
        v, n_sym = make_stream(2, n_frames, period, 96 + 8 * k, snr_db=None, seed=3 + k)
        streams.append(v)
    wide = txgen.synthesise_wideband(streams, M, stacking) * np.sqrt(10 ** (20.0 / 10))
    del streams
    rng = np.random.default_rng(9)
    x = wide.astype(np.complex64)
    del wide
    x += ((rng.standard_normal(x.size) + 1j * rng.standard_normal(x.size)) * np.sqrt(0.5 * M)).astype(np.complex64)
    scale = None
    if fmt != "fc32":
        scale_q = txgen.iq_full_scale(x, 12.0, fmt)
        x, scale = txgen.quantise_iq(x, fmt, scale_q)[0], 1.0 / float(scale_q)
    blk = block.wifi_phy_rx_wideband(M, stacking, 5.21e9, bandwidth=20e6, sample_format=fmt, sample_scale=scale, max_sym=n_sym,
                                     publish_carrier=False, batch_samples=batch)
    got = []
    grshim.msg_connect(blk, "mac_out", grshim.sink_block(got.append), "in")
    grshim.run_stream(blk, x[:period * M * 100], chunk=chunk)                 # warm-up
    n0, rate = len(got), []
    for _ in range(rounds):
        t = time.perf_counter()
        grshim.run_stream(blk, x, chunk=chunk)
        rate.append(len(x) / (time.perf_counter() - t) / 1e9)
    single = None
    try:
        with open(os.path.join(ROOT, "profiles", "host_path_formats.json")) as f:
            single = json.load(f)["gsamples_per_s"]["fc32"]
    except (OSError, KeyError, ValueError):
        pass
    med = float(np.median(rate))
    res = {"workload": "wifi_phy_rx_wideband.work(): %d channels (stacking 1), each the config-2-like stream (QPSK 1/2, 294 B, one frame "
                       "per 4608 channel samples, %d frames, 20 dB), %s items, batch_samples 2^22 per channel, work() chunks of %d wideband "
                       "items; PDU construction and a list-append consumer included" % (M, n_frames, fmt, chunk),
           "method": "one block, %d rounds over the capture, the median; the figure beside it is the fc32 work() rate of the "
                     "single-channel block recorded in profiles/host_path_formats.json (the channels' streams arrive as float32 on the "
                     "device), times the number of channels" % rounds,
           "n_channels": M, "format": fmt, "wideband_gsamples_per_s": med, "wideband_gsamples_per_s_rounds": rate,
           "single_channel_fc32_gsamples_per_s": single, "n_channels_times_single": None if single is None else M * single,
           "ratio_to_n_channels_times_single": None if single is None else med / (M * single),
           "pdus_per_round": (len(got) - n0) // rounds, "frames_per_channel": n_frames}
    print(json.dumps(res), flush=True)
    if out:
        with open(out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    blk.close()


def main():
    if "--wideband" in sys.argv[1:]:
        return wideband_main(list(sys.argv[1:]))
    if "--format" in sys.argv[1:]:
        return formats_main([v for v in sys.argv[1:] if v != "--format"])
    n_frames = int(sys.argv[1]) if len(sys.argv) > 1 else 6000
    for name, enc, period, lead in (("config-2-like", 2, 4608, 160), ("config-1-like", 0, 9420, 100)):
        x, n_sym = make_stream(enc, n_frames, period, lead)
        for batch in (1 << 20, 1 << 22):
            for chunk in (8192, 32768, 131072):
                blk = block.wifi_phy_rx(bandwidth=20e6, frequency=5.89e9, max_sym=n_sym, publish_carrier=False,
                                        batch_samples=batch)
                got = []
                grshim.msg_connect(blk, "mac_out", grshim.sink_block(got.append), "in")
                grshim.run_stream(blk, x[:period * 300], chunk=chunk)             # warm-up
                n0 = len(got)
                best = 0.0
                for _ in range(2):
                    t = time.perf_counter()
                    grshim.run_stream(blk, x, chunk=chunk)
                    dt = time.perf_counter() - t
                    best = max(best, x.size / dt / 1e9)
                print(json.dumps({"stream": name, "batch_samples": batch, "work_chunk": chunk, "gsamples_per_s": round(best, 3),
                                  "pdus": (len(got) - n0) // 2, "frames": n_frames}), flush=True)
                blk.close()


if __name__ == "__main__":
    main()
