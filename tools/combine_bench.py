"""Time wifirx_combine (NUMERICS.md rule 22) for M = 2, 4, 8 channels, with and without gains, on 2^28 output samples,
stacking 1, without hist and hist_out (one kernel per call), with HIP events on the handle's stream after a warm-up,
alternating in one process with device-to-device hipMemcpyAsync calls that move as many bytes as each call reads + writes
(tools/channelizer_bench.py's method and yardstick, unchanged).  A timed window holds enough repetitions to last about 0.1 s;
the figures are per call, medians over the windows.  The project's aim for streaming kernels is 1.3 x the equal-bytes copy
(DESIGN.md section 9d).  Prints one JSON line, writes it to --out when given.

    python tools/combine_bench.py [--log2-samples 28] [--windows 10] [--out profiles/combine_config.json]"""
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

    d_in, d_out = rx.alloc(n * 8), rx.alloc(n * 8)
    # Gaussian float samples, built on the device from one uploaded block; M rows of n / M samples are the same n samples
    blk = min(1 << 22, n)
    d_in.upload(np.random.default_rng(1).standard_normal(2 * blk).astype(np.float32))
    have = blk
    while have < n:
        step = min(have, n - have)
        assert hip.hipMemcpyAsync(d_in.ptr + have * 8, d_in.ptr, step * 8, 3, st) == 0
        rx.sync()
        have += step

    nbytes = n * 16                             # every call reads n samples and writes n samples of 8 bytes
    scratch = rx.alloc(nbytes)                  # the copies' own buffer
    ops = {}
    for M in capi.CHANNELIZER_CHANNELS:
        g = (C.c_float * M)(*[0.5 + 0.25 * k for k in range(M)])
        ops["M%d" % M] = lambda M=M: lib.wifirx_combine(rx._h, d_in.ptr, n // M, None, None, None, M, 1, n // M, 0, d_out.ptr)
        ops["M%d_gains" % M] = lambda M=M, g=g: lib.wifirx_combine(rx._h, d_in.ptr, n // M, g, None, None, M, 1, n // M, 0, d_out.ptr)
    copy = lambda half=nbytes // 2: hip.hipMemcpyAsync(scratch.ptr + half, scratch.ptr, half, 3, st)

    def window(fn, reps):
        assert hip.hipEventRecord(ev0, st) == 0
        for _ in range(reps):
            assert fn() == 0
        assert hip.hipEventRecord(ev1, st) == 0
        assert hip.hipEventSynchronize(ev1) == 0
        t = C.c_float()
        assert hip.hipEventElapsedTime(C.byref(t), ev0, ev1) == 0
        return t.value / reps

    runs = dict(ops)
    runs["memcpy_%d" % nbytes] = copy
    reps = {}
    for name, fn in runs.items():
        window(fn, 2)
        reps[name] = max(int(np.ceil(100.0 / max(window(fn, 3), 1e-3))), 3)
    ms = {k: [] for k in runs}
    for _ in range(a.windows):
        for name, fn in runs.items():
            ms[name].append(window(fn, reps[name]))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    ratio = {name: med[name] / med["memcpy_%d" % nbytes] for name in ops}
    res = dict(workload="2^%d output samples per call, stacking 1, hist = hist_out = NULL: one kernel per call" % a.log2_samples,
               bytes_read_plus_written={name: nbytes for name in ops}, reps_per_window=reps, windows=a.windows,
               ms_windows=ms, ms={name: med[name] for name in ops}, memcpy_d2d_ms={str(nbytes): med["memcpy_%d" % nbytes]},
               GBps={name: nbytes / med[name] / 1e6 for name in ops},
               output_gsamples_per_s={name: n / med[name] / 1e6 for name in ops},
               ratio_to_memcpy=ratio, aim_ratio=AIM, meets_aim={name: bool(r <= AIM) for name, r in ratio.items()},
               note="every figure is per call, HIP events around a window of calls, medians of the windows, kernels and copies "
                    "alternating in one process; the memcpy moves half the byte count (it reads and writes each byte it moves)")
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    for d in (d_in, d_out, scratch):
        d.free()
    rx.close()


if __name__ == "__main__":
    main()
