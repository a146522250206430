"""Time wifirx_tx_batch at config 2's geometry (1 M frames, 294-byte PSDUs, QPSK 1/2, 4608-sample rows, lead 160: 36.9 GB
written) with HIP events on the handle's stream after a warm-up, against a device memset of the same buffer in the same
process; the NumPy transmitter (txgen) on 10 k frames for scale.  Prints one JSON line, writes it to --out when given.

    python tools/tx_bench.py [--iters 5] [--out profiles/tx_batch_config2.json]"""
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
    a = ap.parse_args()
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


if __name__ == "__main__":
    main()
