"""Time one wifirx_tune call with K = 3 channels (NUMERICS.md rule 35) against three wifirx_arb_resample calls (rule 34) on the
same capture of 2^24 input samples, for the ratios 4/1 and 1/1 and the formats fc32 and sc16, with HIP events on the handle's
stream after a warm-up, the two alternating in one process (tools/arb_bench.py's method).  The three resampler calls do
strictly less work: no rotation, and they write the same bytes.  The channels are those of the 2.4 GHz band in an 80 MS/s
capture, -25 / 0 / +25 MHz, so the middle row of the tuner call is not rotated; --all-rotated gives it an increment too.

A timed window holds enough repetitions to last about 0.1 s; the figures are per call (per three calls), medians over the
windows.  Nothing is asserted.  Prints one JSON line, writes it to --out when given.

    python tools/tune_bench.py [--log2-n 24] [--windows 10] [--out profiles/tune_config.json]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gnuradio-wifi-imagetransfer_amd")]

from wifirx import capi  # noqa: E402

RATIOS = ((4, 1), (1, 1))
FORMATS = ("fc32", "sc16")
K = 3
EXPECTED = {(4, 1): 1.15, (1, 1): 1.5}                       # from instruction counts: +8 % / +33 % and +-3 % between boxes


def device_name():
    try:
        import torch
        p = torch.cuda.get_device_properties(0)
        return "%s (%s, %d CUs)" % (p.name, getattr(p, "gcnArchName", "?"), p.multi_processor_count)
    except Exception as e:
        return "unknown (%s)" % e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-n", type=int, default=24, help="input samples per call, as a power of two")
    ap.add_argument("--windows", type=int, default=10)
    ap.add_argument("--all-rotated", action="store_true", help="a small increment for the middle channel as well")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n_in = 1 << a.log2_n
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemsetAsync.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    rx = capi.WifiRx(max_sym=1, device=0)
    st = C.c_void_p(rx.stream_ptr())
    ev0, ev1 = C.c_void_p(), C.c_void_p()
    assert hip.hipEventCreate(C.byref(ev0)) == 0 and hip.hipEventCreate(C.byref(ev1)) == 0

    incs = [capi.tune_inc(-25e6, 80e6), 1 << 40 if a.all_rotated else 0, capi.tune_inc(25e6, 80e6)]
    n_out = {r: capi.arb_count(r[0], r[1], 0, n_in, 0) for r in RATIOS}
    stride = max(n_out.values())
    d_in, d_out = rx.alloc(n_in * 8), rx.alloc(K * stride * 8)
    # every byte 0x3c: the float 0.0115 and the int16 15420, finite in both formats; the kernel has no branch on the data
    assert hip.hipMemsetAsync(d_in.ptr, 0x3C, n_in * 8, st) == 0
    rx.sync()

    def three(num, den, fmt):
        for k in range(K):
            rx.arb_resample_dev(d_in.ptr, fmt, n_in, num, den, d_out.ptr + 8 * k * stride, stride)
        return 0

    runs = {}
    for num, den in RATIOS:
        for fmt in FORMATS:
            key = "%d/%d %s" % (num, den, fmt)
            runs["tune " + key] = lambda num=num, den=den, fmt=fmt: 0 * rx.tune_dev(d_in.ptr, fmt, n_in, num, den, incs, d_out.ptr, stride)
            runs["3 x arb " + key] = lambda num=num, den=den, fmt=fmt: three(num, den, fmt)

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
    for num, den in RATIOS:
        for fmt in FORMATS:
            key = "%d/%d %s" % (num, den, fmt)
            t, c = med["tune " + key], med["3 x arb " + key]
            table[key] = dict(tune_ms=t, three_arb_ms=c, ratio=t / c, expected_at_most=EXPECTED[(num, den)],
                              n_out_per_channel=n_out[(num, den)], msamples_in_per_s=n_in / t / 1e3)
    res = dict(workload="one wifirx_tune call, K = 3 (-25 / 0 / +25 MHz of 80 MS/s%s), against three wifirx_arb_resample calls on "
                        "the same %d input samples from the start of a stream, no hist_out" % (", the middle one rotated too" if a.all_rotated else "", n_in),
               device=device_name(), n_in=n_in, channels=K, incs=["%016x" % v for v in incs], by_ratio_and_format=table,
               reps_per_window=reps, windows=a.windows, ms_windows=ms,
               note="every figure is per tuner call or per three resampler calls, HIP events around a window of calls, medians of the "
                    "windows, the two alternating in one process")
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    for b in (d_in, d_out):
        b.free()
    rx.close()


if __name__ == "__main__":
    main()
