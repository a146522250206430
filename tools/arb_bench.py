"""Time wifirx_arb_resample (NUMERICS.md rule 34) on 2^26 input samples for the ratios 5/4, 192/125, 2/1, 4/1 and 4/5 and the
formats fc32 and sc16, with HIP events on the handle's stream after a warm-up, alternating in one process with a
device-to-device hipMemcpyAsync that moves as many bytes as the call must read and write at least: bytes per input sample *
n_in + 8 * n_out (tools/combine_bench.py's yardstick: the copy moves half the count, since it reads and writes each byte it
moves).

A timed window holds enough repetitions to last about 0.1 s; the figures are per call, medians over the windows.  Nothing is
asserted.  Prints one JSON line, writes it to --out when given.

    python tools/arb_bench.py [--log2-n 26] [--windows 10] [--out profiles/arb_config.json]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gnuradio-wifi-imagetransfer_amd")]

from wifirx import capi  # noqa: E402

RATIOS = ((5, 4), (192, 125), (2, 1), (4, 1), (4, 5))
FORMATS = (("fc32", 8), ("sc16", 4))


def device_name():
    try:
        import torch
        p = torch.cuda.get_device_properties(0)
        return "%s (%s, %d CUs)" % (p.name, getattr(p, "gcnArchName", "?"), p.multi_processor_count)
    except Exception as e:
        return "unknown (%s)" % e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-n", type=int, default=26, help="input samples per call, as a power of two")
    ap.add_argument("--windows", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n_in = 1 << a.log2_n
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipMemsetAsync.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    rx = capi.WifiRx(max_sym=1, device=0)
    st = C.c_void_p(rx.stream_ptr())
    ev0, ev1 = C.c_void_p(), C.c_void_p()
    assert hip.hipEventCreate(C.byref(ev0)) == 0 and hip.hipEventCreate(C.byref(ev1)) == 0

    n_out = {r: capi.arb_count(r[0], r[1], 0, n_in, 0) for r in RATIOS}
    d_in, d_out = rx.alloc(n_in * 8), rx.alloc(max(n_out.values()) * 8)
    # every byte 0x3c: the float 0.0115 and the int16 15420, finite in both formats; the kernel has no branch on the data
    assert hip.hipMemsetAsync(d_in.ptr, 0x3C, n_in * 8, st) == 0
    rx.sync()
    runs, floor = {}, {}
    for num, den in RATIOS:
        for fmt, bps in FORMATS:
            key = "%d/%d %s" % (num, den, fmt)
            floor[key] = bps * n_in + 8 * n_out[(num, den)]
            runs[key] = lambda num=num, den=den, fmt=fmt: 0 * rx.arb_resample_dev(d_in.ptr, fmt, n_in, num, den, d_out.ptr, n_out[(num, den)])
    scratch = rx.alloc(max(floor.values()))                  # the copies' own buffer
    for key in list(floor):
        runs["memcpy " + key] = lambda half=floor[key] // 2: hip.hipMemcpyAsync(scratch.ptr + half, scratch.ptr, half, 3, st)

    def window(fn, reps):
        assert hip.hipEventRecord(ev0, st) == 0
        for _ in range(reps):
            assert fn() == 0
        assert hip.hipEventRecord(ev1, st) == 0
        assert hip.hipEventSynchronize(ev1) == 0
        t = C.c_float()
        assert hip.hipEventElapsedTime(C.byref(t), ev0, ev1) == 0
        return t.value / reps

    reps = {}
    for name, fn in runs.items():
        window(fn, 2)
        reps[name] = max(int(np.ceil(100.0 / max(window(fn, 3), 1e-3))), 3)
    ms = {k: [] for k in runs}
    for _ in range(a.windows):
        for name, fn in runs.items():
            ms[name].append(window(fn, reps[name]))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    table = {}
    for key in floor:
        t, c = med[key], med["memcpy " + key]
        num, den = (int(v) for v in key.split()[0].split("/"))
        taps = 32 * max(num, den) / den
        table[key] = dict(ms=t, memcpy_d2d_ms=c, ratio_to_memcpy=t / c, TBps_at_floor_bytes=floor[key] / t / 1e9,
                          n_out=n_out[(num, den)], taps_per_output=taps, giga_taps_per_s=n_out[(num, den)] * taps / t / 1e6)
    res = dict(workload="wifirx_arb_resample on %d input samples from the start of a stream, no hist_out" % n_in,
               device=device_name(), n_in=n_in, by_ratio_and_format=table, floor_bytes=floor, reps_per_window=reps,
               windows=a.windows, ms_windows=ms,
               note="every figure is per call, HIP events around a window of calls, medians of the windows, calls and copies alternating in "
                    "one process; floor bytes = bytes per input sample * n_in + 8 * n_out; the memcpy moves half that count")
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    for b in (d_in, d_out, scratch):
        b.free()
    rx.close()


if __name__ == "__main__":
    main()
