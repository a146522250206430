"""Time wifirx_spectrum (NUMERICS.md rule 36) on a capture of 2^28 samples per format, for n_fft = 256, 1024 and 4096 and
hop = n_fft and n_fft / 2 (Blackman-Harris, SUM, avg 16), against the cheapest pass over the same input in the same process:
wifirx_iq_to_f32 for sc16 / sc8, a device-to-device copy for fc32.  HIP events on the handle's stream after a warm-up, the
calls alternating in one process (tools/tune_bench.py's method).

A timed window holds enough repetitions to last about 0.1 s; the figures are per call, medians over the windows.  Nothing is
asserted and no ratio is promised.  Prints one JSON line, writes it to --out when given.

    python tools/spectrum_bench.py [--log2-n 28] [--windows 5] [--out profiles/spectrum_config.json]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gnuradio-wifi-imagetransfer_amd")]

from wifirx import capi  # noqa: E402

N_FFT = (256, 1024, 4096)
FORMATS = ("fc32", "sc16", "sc8")
BPS = {"fc32": 8, "sc16": 4, "sc8": 2}
AVG = 16


def device_name():
    try:
        import torch
        p = torch.cuda.get_device_properties(0)
        return "%s (%s, %d CUs)" % (p.name, getattr(p, "gcnArchName", "?"), p.multi_processor_count)
    except Exception as e:
        return "unknown (%s)" % e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-n", type=int, default=28, help="input samples per call, as a power of two")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n_in = 1 << a.log2_n
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemsetAsync.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    rx = capi.WifiRx(max_sym=1, device=0)
    st = C.c_void_p(rx.stream_ptr())
    ev0, ev1 = C.c_void_p(), C.c_void_p()
    assert hip.hipEventCreate(C.byref(ev0)) == 0 and hip.hipEventCreate(C.byref(ev1)) == 0

    rows_cap = {(n, h): capi.spectrum_count(n, n // h, AVG, n_in)[0] for n in N_FFT for h in (1, 2)}
    d_in, d_f32 = rx.alloc(n_in * 8), rx.alloc(n_in * 8)
    d_rows = rx.alloc(max(r * n for (n, _), r in rows_cap.items()) * 4)
    # every byte 0x3c: the float 0.0115, the int16 15420 and the int8 60, finite in every format; no kernel branches on the data
    assert hip.hipMemsetAsync(d_in.ptr, 0x3C, n_in * 8, st) == 0
    rx.sync()

    def copy():
        return hip.hipMemcpyAsync(d_f32.ptr, d_in.ptr, n_in * 8, 3, st)          # hipMemcpyDeviceToDevice

    runs = {}
    for fmt in FORMATS:
        if fmt == "fc32":
            runs["copy fc32"] = copy
        else:
            runs["iq_to_f32 " + fmt] = lambda fmt=fmt: rx.iq_to_f32_dev(d_in.ptr, fmt, n_in, d_f32.ptr) or 0
        for n in N_FFT:
            for h in (1, 2):
                runs["spectrum %s n_fft %d hop %d" % (fmt, n, n // h)] = lambda fmt=fmt, n=n, h=h: 0 * rx.spectrum_dev(
                    d_in.ptr, fmt, n_in, n, n // h, AVG, d_rows.ptr, rows_cap[(n, h)], "blackman_harris", "sum", 1.0)

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
    for fmt in FORMATS:
        base_name = "copy fc32" if fmt == "fc32" else "iq_to_f32 " + fmt
        base = med[base_name]
        for n in N_FFT:
            for h in (1, 2):
                t = med["spectrum %s n_fft %d hop %d" % (fmt, n, n // h)]
                table["%s n_fft %d hop %d" % (fmt, n, n // h)] = dict(
                    spectrum_ms=t, baseline=base_name, baseline_ms=base, ratio=t / base, rows=rows_cap[(n, h)],
                    msamples_in_per_s=n_in / t / 1e3, gbytes_in_per_s=n_in * BPS[fmt] / t / 1e6)
    res = dict(workload="one wifirx_spectrum call (blackman_harris, sum, avg %d) on %d input samples against wifirx_iq_to_f32 "
                        "(sc16, sc8) or a device-to-device copy (fc32) of the same input" % (AVG, n_in),
               device=device_name(), n_in=n_in, avg=AVG, windows=a.windows, by_format_n_fft_and_hop=table,
               note="every figure is per call, HIP events around a window of calls, medians of the windows, all calls "
                    "alternating in one process; no ratio is promised")
    print(json.dumps(dict(res, reps_per_window=reps, ms_windows=ms)))
    if a.out:                                                  # the medians, one line per case
        head = {k: v for k, v in res.items() if k != "by_format_n_fft_and_hop"}
        rows = ",\n".join("  %s: %s" % (json.dumps(k), json.dumps(v)) for k, v in table.items())
        with open(a.out, "w") as f:
            f.write(json.dumps(head, indent=1)[:-2] + ',\n "by_format_n_fft_and_hop": {\n' + rows + "\n }\n}\n")
    for b in (d_in, d_f32, d_rows):
        b.free()
    rx.close()


if __name__ == "__main__":
    main()
