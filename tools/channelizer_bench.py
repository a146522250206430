"""Time wifirx_channelize (NUMERICS.md rule 21) for M = 2, 4, 8 channels in the three sample formats on 2^28 input samples,
stacking 1, without hist and hist_out (one kernel per call), with HIP events on the handle's stream after a warm-up,
alternating in one process with device-to-device hipMemcpyAsync calls that move as many bytes as each call reads + writes
(tools/convert_bench.py's method and yardstick).  A timed window holds enough repetitions to last about 0.1 s; the figures are
per call, medians over the windows.  The project's aim for streaming kernels is 1.3 x the equal-bytes copy (DESIGN.md section
9d).  Prints one JSON line, writes it to --out when given.

    python tools/channelizer_bench.py [--log2-samples 28] [--windows 10] [--out profiles/channelizer_config.json]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gnuradio-wifi-imagetransfer_amd")]

from wifirx import capi  # noqa: E402

AIM = 1.3
FORMATS = (("fc32", capi.IQ_FC32, 8), ("sc16", capi.IQ_SC16, 4), ("sc8", capi.IQ_SC8, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-samples", type=int, default=28)
    ap.add_argument("--windows", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n = 1 << a.log2_samples
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    rx = capi.WifiRx(max_sym=1, device=0)
    st = C.c_void_p(rx.stream_ptr())
    ev0, ev1 = C.c_void_p(), C.c_void_p()
    assert hip.hipEventCreate(C.byref(ev0)) == 0 and hip.hipEventCreate(C.byref(ev1)) == 0
    lib = capi.lib()

    d_in = {"fc32": rx.alloc(n * 8), "sc16": rx.alloc(n * 4), "sc8": rx.alloc(n * 2)}
    d_out = rx.alloc(n * 8)
    # Gaussian float samples, built on the device from one uploaded block; the integer inputs are their quantisations
    blk = min(1 << 22, n)
    d_in["fc32"].upload(np.random.default_rng(1).standard_normal(2 * blk).astype(np.float32))
    have = blk
    while have < n:
        step = min(have, n - have)
        assert hip.hipMemcpyAsync(d_in["fc32"].ptr + have * 8, d_in["fc32"].ptr, step * 8, 3, st) == 0
        rx.sync()
        have += step
    for name, fmt, _ in FORMATS[1:]:
        bits = capi.IQ_MAX_BITS[fmt]
        assert lib.wifirx_iq_from_f32(rx._h, d_in["fc32"].ptr, n, float(np.float32(2.0 ** (bits - 1) / 4.0)), fmt, bits, d_in[name].ptr, None) == 0
    rx.sync()

    scratch = rx.alloc(n * 16)                  # the copies' own buffer: as many bytes as the largest call moves
    ops, copies = {}, {}
    for M in capi.CHANNELIZER_CHANNELS:
        for name, fmt, bps in FORMATS:
            nbytes = n * (bps + 8)
            ops["M%d_%s" % (M, name)] = (lambda M=M, fmt=fmt, name=name: lib.wifirx_channelize(
                rx._h, d_in[name].ptr, fmt, 2.0 ** -7, None, None, M, 1, n // M, 0, d_out.ptr, n // M), nbytes)
            copies[nbytes] = lambda half=nbytes // 2: hip.hipMemcpyAsync(scratch.ptr + half, scratch.ptr, half, 3, st)

    def window(fn, reps):
        assert hip.hipEventRecord(ev0, st) == 0
        for _ in range(reps):
            assert fn() == 0
        assert hip.hipEventRecord(ev1, st) == 0
        assert hip.hipEventSynchronize(ev1) == 0
        t = C.c_float()
        assert hip.hipEventElapsedTime(C.byref(t), ev0, ev1) == 0
        return t.value / reps

    runs = {name: fn for name, (fn, _) in ops.items()}
    runs.update({"memcpy_%d" % b: fn for b, fn in copies.items()})
    reps = {}
    for name, fn in runs.items():
        window(fn, 2)
        reps[name] = max(int(np.ceil(100.0 / max(window(fn, 3), 1e-3))), 3)
    ms = {k: [] for k in runs}
    for _ in range(a.windows):
        for name, fn in runs.items():
            ms[name].append(window(fn, reps[name]))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    ratio = {name: med[name] / med["memcpy_%d" % b] for name, (_, b) in ops.items()}
    res = dict(workload="2^%d input samples per call, stacking 1, hist = hist_out = NULL: one kernel per call" % a.log2_samples,
               bytes_read_plus_written={name: b for name, (_, b) in ops.items()}, reps_per_window=reps, windows=a.windows,
               ms_windows=ms, ms={name: med[name] for name in ops}, memcpy_d2d_ms={str(b): med["memcpy_%d" % b] for b in copies},
               GBps={name: b / med[name] / 1e6 for name, (_, b) in ops.items()},
               input_gsamples_per_s={name: n / med[name] / 1e6 for name in ops},
               ratio_to_memcpy=ratio, aim_ratio=AIM, meets_aim={name: bool(r <= AIM) for name, r in ratio.items()},
               note="every figure is per call, HIP events around a window of calls, medians of the windows, kernels and copies "
                    "alternating in one process; the memcpy of an entry moves half its byte count (it reads and writes each "
                    "byte it moves)")
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    for d in list(d_in.values()) + [d_out, scratch]:
        d.free()
    rx.close()


if __name__ == "__main__":
    main()
