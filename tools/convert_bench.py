"""Time the two sample-format kernels (wifirx_iq_to_f32, wifirx_iq_from_f32 without a counter; NUMERICS.md rule 20) in both
integer formats on 2^28 samples, with HIP events on the handle's stream after a warm-up, alternating in one process with
device-to-device hipMemcpyAsync calls that move as many bytes as each kernel reads + writes (tools/link_bench.py's method).
A timed window holds enough repetitions to last about 0.1 s; the figures are per call, medians over the windows.  The project's
aim for streaming kernels is 1.3 x the equal-bytes copy.  Prints one JSON line, writes it to --out
when given.

    python tools/convert_bench.py [--log2-samples 28] [--windows 5] [--out profiles/convert_formats.json]"""
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
BPS = {"sc16": 4, "sc8": 2}
BITS = {"sc16": 16, "sc8": 8}


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

    d_f, d_i = rx.alloc(n * 8), rx.alloc(n * 4)
    # Gaussian float samples, built on the device from one uploaded block (a 2 GiB host array is not needed for a timing)
    blk = 1 << 22
    seedling = np.random.default_rng(1).standard_normal(2 * min(blk, n)).astype(np.float32)
    d_f.upload(seedling)
    have = min(blk, n)
    while have < n:
        step = min(have, n - have)
        assert hip.hipMemcpyAsync(d_f.ptr + have * 8, d_f.ptr, step * 8, 3, st) == 0
        rx.sync()
        have += step

    scratch = rx.alloc(n * 12)                  # the copies' own buffer: as many bytes as the larger kernel moves
    ops, copies = {}, {}
    for name, fmt in (("sc16", capi.IQ_SC16), ("sc8", capi.IQ_SC8)):
        bps = BPS[name]
        bits = BITS[name]
        scale_q = float(np.float32(2.0 ** (bits - 1) / 4.0))      # full scale at 4 sigma
        assert lib.wifirx_iq_from_f32(rx._h, d_f.ptr, n, scale_q, fmt, bits, d_i.ptr, None) == 0      # real integers to widen
        rx.sync()
        nbytes = n * (8 + bps)
        ops["widen_" + name] = (lambda fmt=fmt, s=1.0 / scale_q: lib.wifirx_iq_to_f32(rx._h, d_i.ptr, fmt, n, s, d_f.ptr), nbytes)
        ops["quantise_" + name] = (lambda fmt=fmt, s=scale_q, b=bits: lib.wifirx_iq_from_f32(rx._h, d_f.ptr, n, s, fmt, b, d_i.ptr, None),
                                   nbytes)
        half = nbytes // 2
        copies[nbytes] = lambda half=half: hip.hipMemcpyAsync(scratch.ptr + half, scratch.ptr, half, 3, st)

    def window(fn, reps):
        assert hip.hipEventRecord(ev0, st) == 0
        for _ in range(reps):
            assert fn() == 0
        assert hip.hipEventRecord(ev1, st) == 0
        assert hip.hipEventSynchronize(ev1) == 0
        t = C.c_float()
        assert hip.hipEventElapsedTime(C.byref(t), ev0, ev1) == 0
        return t.value / reps

    # the kernels rewrite each other's buffers (a widen writes d_f, which the quantisers read): any finite values serve a timing
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
    res = dict(workload="2^%d samples per call; quantise without a counter (clipped = NULL), bits = the container's" % a.log2_samples,
               bytes_read_plus_written={name: b for name, (_, b) in ops.items()}, reps_per_window=reps, ms_windows=ms,
               ms={name: med[name] for name in ops}, memcpy_d2d_ms={str(b): med["memcpy_%d" % b] for b in copies},
               GBps={name: b / med[name] / 1e6 for name, (_, b) in ops.items()},
               gsamples_per_s={name: n / med[name] / 1e6 for name in ops},
               ratio_to_memcpy=ratio, aim_ratio=AIM, meets_aim={name: bool(r <= AIM) for name, r in ratio.items()},
               note="every figure is per call, HIP events around a window of calls, medians of the windows, kernels and copies "
                    "alternating in one process; the memcpy of an entry moves half its byte count (it reads and writes each "
                    "byte it moves)")
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    for d in (d_f, d_i, scratch):
        d.free()
    rx.close()


if __name__ == "__main__":
    main()
