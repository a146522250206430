"""Time wifirx_channel at config 2's geometry (1 M rows of 4608 samples: 36.9 GB read, 36.9 GB written) with HIP events on the
handle's stream after a warm-up: one tap and the 8-tap sets of tests/golden/sv_taps.npy, per-row CFO, unit noise.  In the same
process, against a device-to-device hipMemcpyAsync of the same bytes and wifirx_synth_slots on the same geometry (which only
writes).  Prints one JSON line, writes it to --out when given.

--sro adds wifirx_channel_sro on the same rows with the sample clock locked to the carrier, sro = -cfo bw / (2 pi fc) per
row (NUMERICS.md rule 18), one tap and 8 taps, and a hipMemsetAsync of the output bytes, beside the calls without sro.

--fading adds wifirx_channel_fading on the same rows with the same 8-tap sets, a Doppler of 1e-4 cycles per sample on every
row and K = 10 (NUMERICS.md rule 19), and -- to say where its time goes -- the static and the fading 8-tap call without noise.

    python tools/channel_bench.py [--iters 3] [--out profiles/channel_config2.json]
    python tools/channel_bench.py --sro [--out profiles/channel_sro_config2.json]
    python tools/channel_bench.py --fading [--out profiles/channel_fading_config2.json]"""
import argparse
import ctypes as C
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gnuradio-wifi-imagetransfer_amd")]

from wifirx import capi  # noqa: E402

N, ROW = 1_000_000, 4608


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--rows", type=int, default=N)
    ap.add_argument("--sro", action="store_true", help="also time wifirx_channel_sro (locked sample clock) and a memset")
    ap.add_argument("--fading", action="store_true", help="also time wifirx_channel_fading (8 taps, Doppler 1e-4, K = 10)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n = a.rows
    hip = C.CDLL("libamdhip64.so")
    rx = capi.WifiRx(max_sym=1, device=0)
    st = C.c_void_p(rx.stream_ptr())
    ev0, ev1 = C.c_void_p(), C.c_void_p()
    assert hip.hipEventCreate(C.byref(ev0)) == 0 and hip.hipEventCreate(C.byref(ev1)) == 0
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipMemsetAsync.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]

    nbytes = n * ROW * 8
    d_in = rx.alloc(nbytes)
    d_out = rx.alloc(nbytes)
    rng = np.random.default_rng(1)
    tmpl = ((rng.standard_normal((64, 4401)) + 1j * rng.standard_normal((64, 4401))) * 0.3).astype(np.complex64)
    taps8 = np.load(os.path.join(ROOT, "tests", "golden", "sv_taps.npy")).astype(np.complex64)
    cfo = rng.uniform(-0.037, 0.037, n).astype(np.float32)
    gain = math.sqrt(10 ** 2.0)
    d_taps8 = rx.alloc(taps8.nbytes).upload(taps8)
    d_tap1 = rx.alloc(8).upload(np.ones(1, np.complex64))

    def timed(fn):
        ms = []
        for _ in range(a.iters):
            assert hip.hipEventRecord(ev0, st) == 0
            fn()
            assert hip.hipEventRecord(ev1, st) == 0
            assert hip.hipEventSynchronize(ev1) == 0
            t = C.c_float()
            assert hip.hipEventElapsedTime(C.byref(t), ev0, ev1) == 0
            ms.append(t.value)
        return ms

    runs = {
        "channel_L1": lambda: rx.channel_dev(d_in.ptr, d_out.ptr, n * ROW, n, row_len=ROW, taps=(1.0,), cfo=cfo, gain=gain,
                                             noise_voltage=1.0, seed=7),
        "channel_L8": lambda: rx.channel_dev(d_in.ptr, d_out.ptr, n * ROW, n, row_len=ROW, taps=taps8, cfo=cfo, gain=gain,
                                             noise_voltage=1.0, seed=7),
        # the kernel alone: device taps, no CFO array -- nothing to upload (the kernel does the same work with inc = 0)
        "kernel_L1": lambda: rx.channel_dev(d_in.ptr, d_out.ptr, n * ROW, n, row_len=ROW, taps=d_tap1.ptr, n_taps=1,
                                            gain=gain, noise_voltage=1.0, seed=7),
        "kernel_L8": lambda: rx.channel_dev(d_in.ptr, d_out.ptr, n * ROW, n, row_len=ROW, taps=d_taps8.ptr, n_taps=8,
                                            n_tap_sets=taps8.shape[0], gain=gain, noise_voltage=1.0, seed=7),
        "memcpy_d2d": lambda: hip.hipMemcpyAsync(d_out.ptr, d_in.ptr, nbytes, 3, st),
        "synth_slots": lambda: rx.synth_slots(tmpl, d_out.ptr, ROW, n, 160, 20.0, 0.037, 7),
    }
    if a.sro:
        sro = capi.locked_sro(cfo)
        runs.update({
            "channel_sro_L1": lambda: rx.channel_dev(d_in.ptr, d_out.ptr, n * ROW, n, row_len=ROW, taps=(1.0,), cfo=cfo, sro=sro,
                                                     gain=gain, noise_voltage=1.0, seed=7),
            "channel_sro_L8": lambda: rx.channel_dev(d_in.ptr, d_out.ptr, n * ROW, n, row_len=ROW, taps=taps8, cfo=cfo, sro=sro,
                                                     gain=gain, noise_voltage=1.0, seed=7),
            "memset": lambda: hip.hipMemsetAsync(d_out.ptr, 0, nbytes, st),
        })
    if a.fading:
        fd = np.full(n, 1e-4, np.float32)
        fade = dict(doppler=fd, k_factor=10.0, fade_seed=19)
        runs.update({
            "channel_fading_L8": lambda: rx.channel_dev(d_in.ptr, d_out.ptr, n * ROW, n, row_len=ROW, taps=taps8, cfo=cfo, gain=gain,
                                                        noise_voltage=1.0, seed=7, **fade),
            "channel_L8_quiet": lambda: rx.channel_dev(d_in.ptr, d_out.ptr, n * ROW, n, row_len=ROW, taps=taps8, cfo=cfo, gain=gain,
                                                       noise_voltage=0.0),
            "channel_fading_L8_quiet": lambda: rx.channel_dev(d_in.ptr, d_out.ptr, n * ROW, n, row_len=ROW, taps=taps8, cfo=cfo,
                                                              gain=gain, noise_voltage=0.0, **fade),
        })
    rx.synth_slots(tmpl, d_in.ptr, ROW, n, 160, 20.0, 0.037, 3)        # the input: config 2's slots
    for fn in runs.values():                                            # warm-up of each
        fn()
    rx.sync()
    ms = {k: [] for k in runs}
    for _ in range(2):                                                  # alternate them, twice
        for k, fn in runs.items():
            ms[k] += timed(fn)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    res = dict(workload="wifirx_channel config 2: %d rows of %d samples, per-row CFO, noise_voltage 1" % (n, ROW),
               bytes_read=nbytes, bytes_written=nbytes, ms=ms, ms_median=med,
               GBps_read_plus_write={k: 2 * nbytes / med[k] / 1e6 for k in ("channel_L1", "channel_L8", "kernel_L1", "kernel_L8",
                                                                             "memcpy_d2d")},
               synth_slots_GBps_written=nbytes / med["synth_slots"] / 1e6,
               ratio_to_memcpy={k: med[k] / med["memcpy_d2d"] for k in ("channel_L1", "channel_L8", "kernel_L1", "kernel_L8",
                                                                         "synth_slots")},
               aim_ratio_L8=1.25,
               note="channel_* cover the whole call on the handle's stream: the upload of the host arrays (4 MB of CFO; "
                    "64 KB of taps for L8), then the kernel; kernel_* pass device taps and no CFO array (no upload)")
    if a.sro:
        res["sro"] = dict(what="wifirx_channel_sro, sro = -cfo * 20e6 / (2 pi 5.89e9) per row, drift0 = 0; the whole call "
                               "(upload of 4 MB of CFO and 8 MB of drift increments, then the kernel)",
                          ms_median={k: med[k] for k in ("channel_sro_L1", "channel_sro_L8", "memset")},
                          ratio_to_channel_without_sro={"L1": med["channel_sro_L1"] / med["channel_L1"],
                                                        "L8": med["channel_sro_L8"] / med["channel_L8"]},
                          Gsamples_per_s={k: n * ROW / med[k] / 1e6 for k in ("channel_sro_L1", "channel_sro_L8")},
                          memset_GBps_written=nbytes / med["memset"] / 1e6)
    if a.fading:
        res["fading"] = dict(what="wifirx_channel_fading, 8 taps (sv_taps.npy sets), doppler 1e-4 cycles per sample on every row, "
                                  "k_factor 10, time0 0; the whole call (upload of 4 MB of CFO and 4 MB of Doppler, then the kernel)",
                             ms_median={k: med[k] for k in ("channel_fading_L8", "channel_L8", "memcpy_d2d", "channel_fading_L8_quiet",
                                                            "channel_L8_quiet")},
                             ratio_to_static_L8=med["channel_fading_L8"] / med["channel_L8"],
                             ratio_to_memcpy=med["channel_fading_L8"] / med["memcpy_d2d"],
                             ratio_to_static_L8_without_noise=med["channel_fading_L8_quiet"] / med["channel_L8_quiet"],
                             ms_added_by_fading={"with_noise": med["channel_fading_L8"] - med["channel_L8"],
                                                 "without_noise": med["channel_fading_L8_quiet"] - med["channel_L8_quiet"]},
                             Gsamples_per_s=n * ROW / med["channel_fading_L8"] / 1e6)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    d_in.free(); d_out.free(); d_taps8.free(); d_tap1.free(); rx.close()


if __name__ == "__main__":
    main()
