"""Time wifirx_irs_taps_multi and wifirx_irs_sweep_multi -- Philox scatter, k_factor 10, direct path on, given 2-bit phases / a
2-bit DFT codebook held on the device -- against the only route there was before them, on the same box in the same process: M
calls of wifirx_irs_taps / wifirx_irs_sweep at the same (sets, L, N, K).  Those M calls draw a different channel (an independent
surface-to-user leg per antenna); they are the time yardstick only.  HIP events on the handle's stream around the whole call (the
upload of the line-of-sight vectors and the scales, then the kernel), the median of six after a warm-up.

Shapes: sets 65536, L = 3, N = 256, M = 2, 4, 8 for both calls (the sweep with K = 256), and for the sweep sets 65536, L = 8,
N = 64, K = 256 with M = 2 (16 rows: one full tile) and M = 4 (32 rows: two tiles).  TFLOP/s of the sweep: 8 N K M flops per set
and tap, against the 157 TFLOP/s float32 matrix peak of DESIGN.md section 9k.  Prints one JSON line, writes it to --out when given.

    python tools/irs_multi_bench.py [--iters 6] [--out profiles/irs_multi_config.json]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gnuradio-wifi-imagetransfer_amd")]

from wifirx import capi, irs  # noqa: E402

#          sets   L  N    K    M
TAPS = [(65536, 3, 256, None, M) for M in (2, 4, 8)]
SWEEP = [(65536, 3, 256, 256, M) for M in (2, 4, 8)] + [(65536, 8, 64, 256, M) for M in (2, 4)]
BITS, K_FACTOR, PEAK_TF = 2, 10.0, 157.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=6)
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
        fn()                                                    # the warm-up
        rx.sync()
        ms = []
        for _ in range(a.iters):
            assert hip.hipEventRecord(ev0, st) == 0
            fn()
            assert hip.hipEventRecord(ev1, st) == 0
            assert hip.hipEventSynchronize(ev1) == 0
            t = C.c_float()
            assert hip.hipEventElapsedTime(C.byref(t), ev0, ev1) == 0
            ms.append(t.value)
        return {"ms": ms, "median_ms": float(np.median(ms))}

    rows = []
    for n, L, N, K, M in TAPS + SWEEP:
        S = int(round(N ** 0.5))
        pos = ([0.015, 0.015, 0], [S * 0.015, S * 0.015, 4.5], [S * 0.015 + 0.3, S * 0.015 - 0.2, 1.0])
        b2r, r2u, b2u = irs.los(S, *pos, antennas=M)
        pdp = np.exp(-np.arange(L) / 2.0)
        pdp = (pdp / pdp.sum()).astype(np.float32)
        kw = dict(gain=1.0 / S, k_factor=K_FACTOR, seed=7)
        taps, best = rx.alloc(M * n * L * 8), rx.alloc(n * 2)
        if K is None:
            psi = irs.random_psi(N, BITS, 3)
            d_psi = rx.alloc(psi.nbytes).upload(psi)
            multi = timed(lambda: rx.irs_taps_multi_dev(taps, n, pdp, b2r, r2u, b2u, psi=d_psi, n_psi_sets=1, **kw))
            single = timed(lambda: [rx.irs_taps_dev(taps.ptr + m * n * L * 8, n, pdp, b2r[m], r2u, b2u[m], psi=d_psi, n_psi_sets=1, **kw)
                                    for m in range(M)])
            d_psi.free()
            row = {"call": "wifirx_irs_taps_multi", "against": "%d calls of wifirx_irs_taps" % M}
        else:
            cb = irs.dft_codebook(S, b2r[0], over=int(round((K / N) ** 0.5)), bits=BITS)
            assert cb.shape == (K, N)
            d_cb = rx.alloc(cb.nbytes).upload(cb)
            multi = timed(lambda: rx.irs_sweep_multi_dev(taps, n, pdp, b2r, r2u, b2u, codebook=d_cb, n_codes=K, best_ptr=best, **kw))
            single = timed(lambda: [rx.irs_sweep_dev(taps.ptr + m * n * L * 8, n, pdp, b2r[m], r2u, b2u[m], codebook=d_cb, n_codes=K,
                                                     best_ptr=best, **kw) for m in range(M)])
            d_cb.free()
            flop = 8.0 * N * K * M * n * L
            row = {"call": "wifirx_irs_sweep_multi", "against": "%d calls of wifirx_irs_sweep" % M, "n_codes": K, "rows_per_set": M * L,
                   "row_tiles_per_set": -(-M * L // 16), "flop": flop, "tflops": flop / (multi["median_ms"] * 1e-3) / 1e12,
                   "fraction_of_peak": flop / (multi["median_ms"] * 1e-3) / 1e12 / PEAK_TF,
                   "tflops_single_calls": flop / (single["median_ms"] * 1e-3) / 1e12}
        row.update(n_sets=n, n_taps=L, n_elems=N, n_ant=M, multi=multi, single_calls=single,
                   ratio_multi_over_single=multi["median_ms"] / single["median_ms"])
        rows.append(row)
        print(json.dumps({k: row[k] for k in ("call", "n_taps", "n_elems", "n_ant", "ratio_multi_over_single")} |
                         {"multi_ms": multi["median_ms"], "single_ms": single["median_ms"]}), file=sys.stderr)
        taps.free()
        best.free()
    rx.close()
    res = {"what": __doc__.split("\n\n")[0].replace("\n", " "), "iters": a.iters, "bits": BITS, "k_factor": K_FACTOR, "peak_tflops_f32_matrix": PEAK_TF,
           "runs": rows}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
