"""Time wifirx_irs_estimate -- Philox scatter and noise, k_factor 0, direct path on, every element its own group, the 257 DFT pilots
held on the device, 2-bit codes, all three launches (observe, de-spread and decide, taps) -- against wifirx_irs_sweep_multi at
K = T on the same scene with the group-expanded pilots as its codebook, on the same box in the same process.  The observation is
the sweep's GEMM; at G = N the de-spread has the same flop count, so a ratio of 2 is what counting expects.  HIP events on the
handle's stream around the whole call (the upload of the host arrays, then the kernels), the median of ten after a warm-up of each
shape; the window per shape is the ten calls.

Shapes: sets 4096, L = 8, N = G = 256, T = 257, M = 1 and 4.  The observations (sets * M * L * T complex64) go to the handle's
scratch, as a caller without an obs_out has them.  Prints one JSON line, writes it to --out when given.

    python tools/irs_estimate_bench.py [--iters 10] [--out profiles/irs_estimate_config.json]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gnuradio-wifi-imagetransfer_amd")]

from wifirx import capi, irs  # noqa: E402

#         sets  L  N    M
SHAPES = [(4096, 8, 256, M) for M in (1, 4)]
BITS, SIGMA = 2, 1.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
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
        return {"ms": ms, "median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms))}

    rows = []
    for n, L, N, M in SHAPES:
        S = int(round(N ** 0.5))
        pos = ([0.015, 0.015, 0], [S * 0.015, S * 0.015, 4.5], [S * 0.015 + 0.3, S * 0.015 - 0.2, 1.0])
        b2r, r2u, b2u = irs.los(S, *pos, antennas=M)
        pdp = np.exp(-np.arange(L) / 2.0)
        pdp = (pdp / pdp.sum()).astype(np.float32)
        pl = irs.dft_pilots(N)
        T = pl.shape[0]
        kw = dict(gain=1.0 / S, k_factor=0.0, seed=7)
        taps, best, codes, obs = rx.alloc(M * n * L * 8), rx.alloc(n * 2), rx.alloc(n * N), rx.alloc(n * M * L * T * 8)
        d_pl = rx.alloc(pl.nbytes).upload(pl)
        est = timed(lambda: rx.irs_estimate_dev(taps, n, pdp, b2r, r2u, b2u, pilots=d_pl, n_pilots=T, n_groups=N, sigma=SIGMA,
                                                est_scale=irs.est_scale(T), align_bits=BITS, codes_ptr=codes, **kw))
        observe = timed(lambda: rx.irs_estimate_dev(None, n, pdp, b2r, r2u, b2u, pilots=d_pl, n_pilots=T, n_groups=N, sigma=SIGMA,
                                                    obs_ptr=obs, **kw))
        sweep = timed(lambda: rx.irs_sweep_multi_dev(taps, n, pdp, b2r, r2u, b2u, codebook=d_pl, n_codes=T, best_ptr=best, **kw))
        flop_gemm = 8.0 * N * T * M * n * L                     # one complex GEMM of [M L sets, N] by [N, T]
        flop_est = flop_gemm + 8.0 * T * (N + 1) * M * n * L
        row = {"n_sets": n, "n_taps": L, "n_elems": N, "n_groups": N, "n_pilots": T, "n_ant": M, "rows_per_set": M * L,
               "estimate": est, "observe_alone": observe, "sweep_multi_at_K_equal_T": sweep,
               "ratio_estimate_over_sweep": est["median_ms"] / sweep["median_ms"],
               "ratio_observe_over_sweep": observe["median_ms"] / sweep["median_ms"],
               "flop_estimate": flop_est, "flop_sweep": flop_gemm,
               "tflops_estimate": flop_est / (est["median_ms"] * 1e-3) / 1e12,
               "tflops_sweep": flop_gemm / (sweep["median_ms"] * 1e-3) / 1e12,
               "obs_scratch_bytes": n * M * L * T * 8}
        rows.append(row)
        print(json.dumps({k: row[k] for k in ("n_ant", "ratio_estimate_over_sweep", "ratio_observe_over_sweep", "tflops_estimate",
                                              "tflops_sweep")} | {"estimate_ms": est["median_ms"], "sweep_ms": sweep["median_ms"]}),
              file=sys.stderr)
        for b in (taps, best, codes, obs, d_pl):
            b.free()
    rx.close()
    res = {"what": __doc__.split("\n\n")[0].replace("\n", " "), "iters": a.iters, "bits": BITS, "sigma": SIGMA, "runs": rows}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
