"""Time wifirx_irs_sweep -- Philox scatter, k_factor 10, direct path on, a 2-bit DFT codebook held on the device -- at
(sets, L, N, K) = (65536, 3, 256, 256), (65536, 8, 64, 256) and (16384, 3, 256, 1024), with HIP events on the handle's stream
after a warm-up; and, at the first shape, on the same box in the same process, the only route there was before it: K calls of
wifirx_irs_taps, one per codebook entry (psi = that entry, on the device), which draw every element K times.  Every call covers
the whole entry point (the upload of the line-of-sight vectors and the scales, a few kB, then the kernel).  Medians of 6 runs.
Prints one JSON line, writes it to --out when given.

    python tools/irs_sweep_bench.py [--iters 3] [--out profiles/irs_sweep_config.json]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gnuradio-wifi-imagetransfer_amd")]

from wifirx import capi, irs  # noqa: E402

SHAPES = [(65536, 3, 256, 256), (65536, 8, 64, 256), (16384, 3, 256, 1024)]
BITS, K_FACTOR, PEAK_TF = 2, 10.0, 157.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    hip = C.CDLL("libamdhip64.so")
    rx = capi.WifiRx(max_sym=1, device=0)
    st = C.c_void_p(rx.stream_ptr())
    ev0, ev1 = C.c_void_p(), C.c_void_p()
    assert hip.hipEventCreate(C.byref(ev0)) == 0 and hip.hipEventCreate(C.byref(ev1)) == 0
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]

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

    runs, bufs, flop = {}, [], {}
    for n, L, N, K in SHAPES:
        S = int(round(N ** 0.5))
        over = int(round((K / N) ** 0.5))
        b2r, r2u, b2u = irs.los(S, [0.015, 0.015, 0], [S * 0.015, S * 0.015, 4.5], [S * 0.015 + 0.3, S * 0.015 - 0.2, 1.0])
        cb = irs.dft_codebook(S, b2r, over=over, bits=BITS)
        assert cb.shape == (K, N)
        pdp = np.exp(-np.arange(L) / 2.0)
        pdp = (pdp / pdp.sum()).astype(np.float32)
        d_cb, d_taps, d_best = rx.alloc(cb.nbytes).upload(cb), rx.alloc(n * L * 8), rx.alloc(n * 2)
        bufs += [d_cb, d_taps, d_best]
        kw = dict(gain=1.0 / N ** 0.5, k_factor=K_FACTOR, seed=7)
        name = "sweep_sets%d_L%d_N%d_K%d" % (n, L, N, K)
        flop[name] = 8.0 * N * K * n * L
        runs[name] = (lambda v=(d_taps, n, pdp, b2r, r2u, b2u, d_cb, K, d_best), kw=kw:
                      rx.irs_sweep_dev(v[0], v[1], v[2], v[3], v[4], v[5], codebook=v[6], n_codes=v[7], best_ptr=v[8], **kw))
        if (n, L, N, K) == SHAPES[0]:
            def k_calls(v=(d_taps, n, pdp, b2r, r2u, b2u, d_cb, K, N), kw=kw):
                for k in range(v[7]):
                    rx.irs_taps_dev(v[0], v[1], v[2], v[3], v[4], v[5], psi=v[6].ptr + 8 * v[8] * k, n_psi_sets=1, **kw)
            runs["k_calls_of_irs_taps_sets%d_L%d_N%d_K%d" % (n, L, N, K)] = k_calls
    for fn in runs.values():                                            # warm-up of each
        fn()
    rx.sync()
    ms = {k: [] for k in runs}
    for _ in range(2):                                                  # alternate them, twice
        for k, fn in runs.items():
            ms[k] += timed(fn)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    first = "sets%d_L%d_N%d_K%d" % SHAPES[0]
    tf = {k: flop[k] / (med[k] * 1e-3) / 1e12 for k in flop}
    res = dict(workload="wifirx_irs_sweep: Philox scatter, k_factor %g, direct path on, %d-bit DFT codebook on the device; taps and "
                        "winners written, powers not" % (K_FACTOR, BITS),
               shapes="sets, L, N, K", ms=ms, ms_median=med,
               f32_TFLOPs={k: v for k, v in tf.items()}, flop_count="8 N K per set and tap",
               fraction_of_f32_matrix_peak={k: v / PEAK_TF for k, v in tf.items()}, matrix_peak_TFLOPs=PEAK_TF,
               ratio_k_calls_to_sweep=med["k_calls_of_irs_taps_" + first] / med["sweep_" + first],
               note="the K calls are the route the library offered before wifirx_irs_sweep: one wifirx_irs_taps call per entry, "
                    "each drawing all elements again and each with its own small upload and stream synchronisation; they "
                    "produce K tap sets per draw and no winner (the powers and the argmax would come on top)")
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    for b in bufs:
        b.free()
    rx.close()


if __name__ == "__main__":
    main()
