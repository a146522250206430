"""Time wifirx_frontend (NUMERICS.md rule 32: statistics, apply fused with the widening, state) against wifirx_iq_to_f32 (rule
20's widening alone) on the same 2^28 samples, per format, in one process: HIP events on the handle's stream after a
warm-up, the two alternating, a timed window holding enough calls to last about 0.1 s, medians over the windows
(tools/convert_bench.py's method).  For fc32 there is nothing to widen: the yardstick is a device-to-device hipMemcpyAsync
of the samples.  The front end reads its input twice and writes once where the yardstick reads and writes once, so the byte
ratio is (2 b + 8) / (b + 8) for b bytes per input sample: 1.33 for sc16, 1.2 for sc8, 1.5 for fc32.  No time is promised;
the measured ratio is recorded with the device it was measured on.  Prints one JSON line, writes it to --out when given.

    python tools/frontend_bench.py [--log2-samples 28] [--windows 5] [--out profiles/frontend_config.json]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gnuradio-wifi-imagetransfer_amd")]

from wifirx import capi  # noqa: E402

BPS = {"fc32": 8, "sc16": 4, "sc8": 2}


def device_name():
    try:
        import torch
        p = torch.cuda.get_device_properties(0)
        return "%s (%s, %d CUs)" % (p.name, getattr(p, "gcnArchName", "?"), p.multi_processor_count)
    except Exception as e:
        return "unknown (%s)" % e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-samples", type=int, default=28)
    ap.add_argument("--windows", type=int, default=5)
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

    d_f, d_out, d_i, d_st = rx.alloc(n * 8), rx.alloc(n * 8), rx.alloc(n * 4), rx.alloc(capi.FE_STATE_DTYPE.itemsize)
    # Gaussian float samples with an offset, built on the device from one uploaded block
    blk = min(1 << 22, n)
    seedling = (np.random.default_rng(1).standard_normal(2 * blk) + 0.25).astype(np.float32)
    d_f.upload(seedling)
    have = blk
    while have < n:
        step = min(have, n - have)
        assert hip.hipMemcpyAsync(d_f.ptr + have * 8, d_f.ptr, step * 8, 3, st) == 0
        rx.sync()
        have += step
    d_st.upload(np.zeros(1, capi.FE_STATE_DTYPE))
    cfg = capi.frontend_cfg(dc=True, iq=True)

    def window(fn, reps):
        assert hip.hipEventRecord(ev0, st) == 0
        for _ in range(reps):
            assert fn() == 0
        assert hip.hipEventRecord(ev1, st) == 0
        assert hip.hipEventSynchronize(ev1) == 0
        t = C.c_float()
        assert hip.hipEventElapsedTime(C.byref(t), ev0, ev1) == 0
        return t.value / reps

    res_fmt = {}
    for name in ("sc16", "sc8", "fc32"):
        fmt, bps = capi.IQ_FORMATS[name], BPS[name]
        if name == "fc32":
            src, scale = d_f.ptr, 1.0
            base = lambda: hip.hipMemcpyAsync(d_out.ptr, d_f.ptr, n * 8, 3, st)
            base_name = "hipMemcpyAsync device to device, n * 8 bytes"
        else:
            bits = capi.IQ_MAX_BITS[fmt]
            scale_q = float(np.float32(2.0 ** (bits - 1) / 4.0))      # full scale at 4 sigma
            assert lib.wifirx_iq_from_f32(rx._h, d_f.ptr, n, scale_q, fmt, bits, d_i.ptr, None) == 0
            rx.sync()
            src, scale = d_i.ptr, 1.0 / scale_q
            base = lambda fmt=fmt, scale=scale: lib.wifirx_iq_to_f32(rx._h, d_i.ptr, fmt, n, scale, d_out.ptr)
            base_name = "wifirx_iq_to_f32"
        fe = lambda src=src, fmt=fmt, scale=scale: lib.wifirx_frontend(rx._h, C.byref(cfg), d_st.ptr, src, fmt, scale, n, d_out.ptr)
        runs = {"frontend": fe, "baseline": base}
        reps = {}
        for k, fn in runs.items():
            window(fn, 2)
            reps[k] = max(int(np.ceil(100.0 / max(window(fn, 3), 1e-3))), 3)
        ms = {k: [] for k in runs}
        for _ in range(a.windows):
            for k, fn in runs.items():
                ms[k].append(window(fn, reps[k]))
        med = {k: float(np.median(v)) for k, v in ms.items()}
        res_fmt[name] = dict(baseline=base_name, ms_windows=ms, reps_per_window=reps, frontend_ms=med["frontend"], baseline_ms=med["baseline"],
                             ratio=med["frontend"] / med["baseline"], byte_ratio=(2 * bps + 8) / (bps + 8),
                             frontend_GBps=n * (2 * bps + 8) / med["frontend"] / 1e6, baseline_GBps=n * (bps + 8) / med["baseline"] / 1e6,
                             gsamples_per_s=n / med["frontend"] / 1e6)
    res = dict(workload="2^%d samples per call, both stages on (the arithmetic does not depend on the flags), the state carried from "
                        "call to call on the device" % a.log2_samples,
               device=device_name(), formats=res_fmt,
               note="per call, HIP events around a window of calls, medians of the windows, front end and yardstick alternating in "
                    "one process.  The front end is three launches (statistics: read; apply: read + write; state); byte_ratio "
                    "is what its traffic alone predicts against one read and one write")
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    for d in (d_f, d_out, d_i, d_st):
        d.free()
    rx.close()


if __name__ == "__main__":
    main()
