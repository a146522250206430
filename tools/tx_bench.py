"""Time wifirx_tx_batch at config 2's geometry (1 M frames, 294-byte PSDUs, QPSK 1/2, 4608-sample rows, lead 160: 36.9 GB
written) with HIP events on the handle's stream after a warm-up, against a device memset of the same buffer in the same
process; the NumPy transmitter (txgen) on 10 k frames for scale.  Prints one JSON line, writes it to --out when given.

    python tools/tx_bench.py [--iters 5] [--out profiles/tx_batch_config2.json]

--rates times wifirx_tx_batch_rates instead: the same PSDUs with the eight encodings cycling (frame i at encoding i % 8), in
row_off rows of lead + frame rounded up to even, against the sum of eight wifirx_tx_batch calls, each over the frames of one
encoding in row_off rows of the same lengths (the same symbols and bytes written, no wave holds two rates), and a memset of
the same bytes; then encodings 0 and 7 alternating against its two single-encoding calls.  One process, the calls that are
compared alternating, medians.

    python tools/tx_bench.py --rates [--iters 5] [--out profiles/tx_rates_config2.json]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gnuradio-wifi-imagetransfer_amd")]

from wifirx import capi, txgen  # noqa: E402

N, L, ENC, ROW, LEAD = 1_000_000, 294, 2, 4608, 160


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--frames", type=int, default=N)
    ap.add_argument("--out", default=None)
    ap.add_argument("--rates", action="store_true", help="time the call with one encoding per frame")
    a = ap.parse_args()
    if a.rates:
        return rates_main(a)
    n = a.frames
    hip = C.CDLL("libamdhip64.so")
    rx = capi.WifiRx(max_sym=1, device=0)
    st = C.c_void_p(rx.stream_ptr())
    ev0, ev1 = C.c_void_p(), C.c_void_p()
    assert hip.hipEventCreate(C.byref(ev0)) == 0 and hip.hipEventCreate(C.byref(ev1)) == 0
    hip.hipMemsetAsync.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]

    rng = np.random.default_rng(1)
    p = rng.integers(0, 256, size=(n, L), dtype=np.uint8)
    d_psdu = rx.alloc(p.nbytes).upload(p)
    lens = np.full(n, L, np.uint32)
    out = rx.alloc(n * ROW * 8)
    nbytes = n * ROW * 8

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

    tx = lambda: rx.tx_batch_dev(out.ptr, n * ROW, d_psdu.ptr, ENC, psdu_len=lens, psdu_stride=L, row_len=ROW, lead=LEAD)
    ms_set = lambda: hip.hipMemsetAsync(out.ptr, 0, nbytes, st)
    tx(); ms_set(); rx.sync()                                     # warm-up of both
    t_tx, t_set = [], []
    for _ in range(2):                                             # alternate the two, twice
        t_tx += timed(tx)
        t_set += timed(ms_set)
    tx()                                                           # the memsets came last: build the rows once more
    rx.sync()
    # correctness of what was timed: a few rows against txgen
    rows = np.empty((3, ROW), np.complex64)
    for k, f in enumerate((0, n // 2, n - 1)):
        rx._check(capi.lib().wifirx_memcpy_d2h(rx._h, rows[k].ctypes.data_as(C.c_void_p), out.ptr + f * ROW * 8, ROW * 8))
    ref = txgen.encode_psdus(p[[0, n // 2, n - 1]], ENC, seeds=[1, (n // 2) % 127 + 1, (n - 1) % 127 + 1]).samples
    err = float(np.abs(rows[:, LEAD:LEAD + ref.shape[1]] - ref).max())
    t0 = time.perf_counter()
    txgen.encode_psdus(txgen.make_psdus(10_000, L, seed=3), ENC)
    cpu_s = time.perf_counter() - t0
    med_tx, med_set = float(np.median(t_tx)), float(np.median(t_set))
    res = dict(workload="wifirx_tx_batch config 2: %d frames, %d B PSDUs, QPSK 1/2, rows of %d samples, lead %d" % (n, L, ROW, LEAD),
               bytes_written=nbytes, tx_ms=t_tx, memset_ms=t_set, tx_ms_median=med_tx, memset_ms_median=med_set,
               tx_GBps=nbytes / med_tx / 1e6, memset_GBps=nbytes / med_set / 1e6, ratio_to_memset=med_tx / med_set,
               aim_ratio=1.3, max_abs_err_vs_txgen=err, txgen_cpu_frames_per_s=10_000 / cpu_s,
               gpu_frames_per_s=n / (med_tx / 1e3),
               note="tx_ms covers the whole call on the handle's stream: the upload of the 4 MB length array, then the kernel")
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    out.free(); d_psdu.free(); rx.close()


def rates_main(a):
    n = a.frames - a.frames % 8
    hip = C.CDLL("libamdhip64.so")
    rx = capi.WifiRx(max_sym=1, device=0)
    st = C.c_void_p(rx.stream_ptr())
    ev0, ev1 = C.c_void_p(), C.c_void_p()
    assert hip.hipEventCreate(C.byref(ev0)) == 0 and hip.hipEventCreate(C.byref(ev1)) == 0
    hip.hipMemsetAsync.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]

    def timed(fn):
        assert hip.hipEventRecord(ev0, st) == 0
        fn()
        assert hip.hipEventRecord(ev1, st) == 0
        assert hip.hipEventSynchronize(ev1) == 0
        t = C.c_float()
        assert hip.hipEventElapsedTime(C.byref(t), ev0, ev1) == 0
        return t.value

    rng = np.random.default_rng(1)
    p = rng.integers(0, 256, size=(n, L), dtype=np.uint8)
    d_psdu = rx.alloc(p.nbytes).upload(p)
    flen = np.array([txgen.frame_samples(L, e) for e in range(8)])
    row_of = LEAD + flen + ((LEAD + flen) & 1)
    mixes = []
    for name, cycle in (("encodings 0..7 cycling", list(range(8))), ("encodings 0 and 7 alternating", [0, 7])):
        k = len(cycle)
        enc = np.array(cycle * (n // k), np.uint8)
        row_off = np.concatenate([[0], np.cumsum(row_of[enc])]).astype(np.uint64)
        total = int(row_off[-1])
        out = rx.alloc(total * 8)
        lens = np.full(n, L, np.uint32)
        mixed = lambda: rx.tx_batch_dev(out.ptr, total, d_psdu.ptr, enc, psdu_len=lens, psdu_stride=L, lead=LEAD, row_off=row_off)
        # the frames of one encoding: every k-th PSDU (stride k L), rows of that encoding's length, in a region of their own
        singles, base = [], 0
        for j, e in enumerate(cycle):
            m = n // k
            ro = (np.arange(m + 1, dtype=np.uint64) * np.uint64(row_of[e]))
            singles.append(dict(ptr=out.ptr + base * 8, cap=m * int(row_of[e]), psdu=d_psdu.ptr + j * L, e=e, ro=ro,
                                lens=np.full(m, L, np.uint32)))
            base += m * int(row_of[e])
        assert base == total

        def one(sg):
            rx.tx_batch_dev(sg["ptr"], sg["cap"], sg["psdu"], sg["e"], psdu_len=sg["lens"], psdu_stride=k * L, lead=LEAD, row_off=sg["ro"])

        def split():
            for sg in singles:
                one(sg)

        ms_set = lambda: hip.hipMemsetAsync(out.ptr, 0, total * 8, st)
        mixed(); split(); ms_set(); rx.sync()                      # warm-up of all three
        t_mix, t_split, t_set, t_each = [], [], [], {e: [] for e in cycle}
        for _ in range(a.iters):                                   # alternating
            t_mix.append(timed(mixed))
            t_split.append(timed(split))
            t_set.append(timed(ms_set))
        for _ in range(a.iters):                                   # the single-encoding calls one by one, for the table
            for sg in singles:
                t_each[sg["e"]].append(timed(lambda: one(sg)))
        # correctness of what was timed: rows of the mixed call against txgen, one per encoding at both ends of the batch
        mixed(); rx.sync()
        err = 0.0
        for f in list(range(k)) + list(range(n - k, n)):
            row = np.empty(int(row_of[enc[f]]), np.complex64)
            rx._check(capi.lib().wifirx_memcpy_d2h(rx._h, row.ctypes.data_as(C.c_void_p), out.ptr + int(row_off[f]) * 8, row.nbytes))
            ref = txgen.encode_psdus(p[f:f + 1], int(enc[f]), seeds=[f % 127 + 1]).samples[0]
            err = max(err, float(np.abs(row[LEAD:LEAD + ref.size] - ref).max()), float(np.abs(row[:LEAD]).max(initial=0.0)),
                      float(np.abs(row[LEAD + ref.size:]).max(initial=0.0)))
        out.free()
        med = lambda v: float(np.median(v))
        mixes.append(dict(mix=name, frames=n, bytes_written=total * 8, mixed_ms=t_mix, split_ms=t_split, memset_ms=t_set,
                          mixed_ms_median=med(t_mix), split_ms_median=med(t_split), memset_ms_median=med(t_set),
                          mixed_TBps=total * 8 / med(t_mix) / 1e9, split_TBps=total * 8 / med(t_split) / 1e9,
                          ratio_to_split=med(t_mix) / med(t_split), ratio_to_memset=med(t_mix) / med(t_set),
                          single_call_ms_median={str(e): med(v) for e, v in t_each.items()},
                          max_abs_err_vs_txgen=err))
    res = dict(workload="wifirx_tx_batch_rates: %d frames, %d B PSDUs, row_off rows of lead %d + frame rounded up to even" % (n, L, LEAD),
               aim_ratio_to_split=1.25, mixes=mixes,
               method="HIP events on the handle's stream around each call (upload of the host arrays, then the kernel) after a "
                      "warm-up; mixed call, the single-encoding calls back to back and a memset alternating in one process; "
                      "medians of %d" % a.iters)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    d_psdu.free(); rx.close()


if __name__ == "__main__":
    main()
