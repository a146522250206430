"""Time wifirx_irs_optimize -- 4096 sets, 2-bit codes, at most 4 sweeps from the estimate's own decision, codes and phases written --
on the est_out of a wifirx_irs_estimate call (Philox scatter and noise, k_factor 0, direct path on, every element its own group, the
N + 1 DFT pilots, sigma 1), against that whole wifirx_irs_estimate call (observe, de-spread and decide, taps) at the same shape, on
the same box in the same process.  HIP events on the handle's stream around the whole call, the median of ten after a warm-up of
each shape.

A wave owns a set and runs a dependent chain of (sweeps + 1) G steps, each of which ends in the six-level butterfly and the argmax,
so the call is bound by that chain's latency and by how many waves a SIMD holds, not by the bytes of the coefficient matrix: the
rows of the result give the time per step of the chain and the bytes per second the reads amount to.

Shapes (M, L, N): (1, 1, 64), (4, 1, 64), (4, 8, 64), (4, 8, 256).  Prints one JSON line, writes it to --out when given.

--weights times wifirx_irs_optimize_weighted (NUMERICS.md rule 31) beside wifirx_irs_optimize on the same coefficients in the same
process: host weights (1, -0.5, ..) per antenna, which ride in the call's one upload, and the same weights as a device buffer of
one row block; the chain of a step grows by two multiplies and a select.  --old-lib PATH also times wifirx_irs_optimize of another
build of the library (the parent commit's), loaded beside this one, on the same device buffers through a handle of its own.

    python tools/irs_optimize_bench.py [--iters 10] [--out profiles/irs_optimize_config.json]
    python tools/irs_optimize_bench.py --weights [--old-lib PATH] [--out profiles/irs_optimize_w_config.json]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gnuradio-wifi-imagetransfer_amd")]

from wifirx import capi, irs  # noqa: E402

#         M  L  N
SHAPES = [(1, 1, 64), (4, 1, 64), (4, 8, 64), (4, 8, 256)]
SETS, BITS, SWEEPS, SIGMA = 4096, 2, 4, 1.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--weights", action="store_true", help="time wifirx_irs_optimize_weighted beside wifirx_irs_optimize")
    ap.add_argument("--old-lib", default=None, help="another build of libwifirx.so whose wifirx_irs_optimize is timed too")
    a = ap.parse_args()
    hip = C.CDLL("libamdhip64.so")
    rx = capi.WifiRx(max_sym=1, device=0)
    st = C.c_void_p(rx.stream_ptr())
    ev0, ev1 = C.c_void_p(), C.c_void_p()
    assert hip.hipEventCreate(C.byref(ev0)) == 0 and hip.hipEventCreate(C.byref(ev1)) == 0
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]

    old = old_h = old_st = None
    if a.old_lib:                                               # a handle of the other build, on a stream of its own
        old, old_h = C.CDLL(os.path.abspath(a.old_lib)), C.c_void_p()
        old.wifirx_create.argtypes = [C.POINTER(capi.Config), C.POINTER(C.c_void_p)]
        old.wifirx_stream.restype, old.wifirx_stream.argtypes = C.c_void_p, [C.c_void_p]
        old.wifirx_destroy.argtypes = old.wifirx_sync.argtypes = [C.c_void_p]
        old.wifirx_irs_optimize.argtypes = capi.lib().wifirx_irs_optimize.argtypes
        assert old.wifirx_create(C.byref(rx.cfg), C.byref(old_h)) == 0
        old_st = C.c_void_p(old.wifirx_stream(old_h))

    def timed(fn, st=st, sync=rx.sync):
        fn()                                                    # the warm-up
        sync()
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

    rows, n = [], SETS
    for M, L, N in SHAPES:
        S = int(round(N ** 0.5))
        pos = ([0.015, 0.015, 0], [S * 0.015, S * 0.015, 4.5], [S * 0.015 + 0.3, S * 0.015 - 0.2, 1.0])
        b2r, r2u, b2u = irs.los(S, *pos, antennas=M)
        pdp = np.exp(-np.arange(L) / 2.0)
        pdp = (pdp / pdp.sum()).astype(np.float32)
        pl = irs.dft_pilots(N)
        T, R, J = pl.shape[0], M * L, N + 1
        kw = dict(gain=1.0 / S, k_factor=0.0, seed=7, pilots=None, n_pilots=T, n_groups=N, sigma=SIGMA, est_scale=irs.est_scale(T))
        taps, codes, coef, psi = rx.alloc(M * n * L * 8), rx.alloc(n * N), rx.alloc(n * R * J * 8), rx.alloc(n * N * 8)
        power, sweeps = rx.alloc(n * (SWEEPS + 1) * 4), rx.alloc(n)
        kw["pilots"] = rx.alloc(pl.nbytes).upload(pl)
        est = timed(lambda: rx.irs_estimate_dev(taps, n, pdp, b2r, r2u, b2u, align_bits=BITS, codes_ptr=codes, est_ptr=coef, **kw))
        opt = timed(lambda: rx.irs_optimize_dev(coef, n, R, J, bits=BITS, max_sweeps=SWEEPS, codes_ptr=codes, psi_ptr=psi))
        extra = {}
        if a.weights:
            w = irs.row_weights(M, L, tap=irs.tap_weights(L, penalty=0.5))
            d_w = rx.alloc(w.nbytes).upload(w)
            okw = dict(bits=BITS, max_sweeps=SWEEPS, codes_ptr=codes, psi_ptr=psi)
            host = timed(lambda: rx.irs_optimize_dev(coef, n, R, J, weights=w, **okw))
            dev = timed(lambda: rx.irs_optimize_dev(coef, n, R, J, weights_ptr=d_w, **okw))
            again = timed(lambda: rx.irs_optimize_dev(coef, n, R, J, **okw))     # the unweighted call once more, behind the two
            extra = {"weights": w.tolist(), "weighted_host_weights": host, "weighted_device_weights": dev,
                     "optimize_again": again, "ratio_weighted_host_over_optimize": host["median_ms"] / opt["median_ms"],
                     "ratio_weighted_device_over_optimize": dev["median_ms"] / opt["median_ms"]}
            d_w.free()
        if old is not None:
            call = lambda: old.wifirx_irs_optimize(old_h, coef.ptr, n, R, J, BITS, SWEEPS, capi.IRS_START_REF, 0, None, N, None,
                                                   codes.ptr, psi.ptr, None, None)
            assert call() == 0
            was = timed(call, old_st, lambda: old.wifirx_sync(old_h))
            extra |= {"optimize_of_old_lib": was, "ratio_optimize_over_old_lib": opt["median_ms"] / was["median_ms"]}
        rx.irs_optimize_dev(coef, n, R, J, bits=BITS, max_sweeps=SWEEPS, codes_ptr=codes, power_ptr=power, sweeps_ptr=sweeps)
        done = sweeps.download(np.uint8, n).astype(np.float64)
        pw = power.download(np.float32, n * (SWEEPS + 1)).reshape(n, SWEEPS + 1).astype(np.float64)
        passes = float(np.minimum(done + 1, SWEEPS).mean()) + 1          # the start pass, the sweeps that changed a code, the one that did not
        sec = opt["median_ms"] * 1e-3
        row = {"n_sets": n, "n_ant": M, "n_taps": L, "n_elems": N, "rows_per_set": R, "cols": J, "max_sweeps": SWEEPS,
               "optimize": opt, "estimate_whole_call": est, "ratio_optimize_over_estimate": opt["median_ms"] / est["median_ms"],
               "sweeps_that_changed_a_code_mean": float(done.mean()), "passes_over_the_matrix_mean": passes,
               "power_ratio_last_over_start": float(pw[:, -1].sum() / pw[:, 0].sum()),
               "coef_bytes": n * R * J * 8, "read_gb_per_s": n * R * J * 8 * passes / sec / 1e9,
               "ns_per_step_of_a_wave": sec / (passes * N) * 1e9, "waves": n} | extra
        rows.append(row)
        print(json.dumps({k: row[k] for k in ("n_ant", "n_taps", "n_elems", "ratio_optimize_over_estimate", "read_gb_per_s",
                                              "ns_per_step_of_a_wave", "power_ratio_last_over_start")}
                         | {"optimize_ms": opt["median_ms"], "estimate_ms": est["median_ms"]}
                         | {k: v for k, v in extra.items() if k.startswith("ratio")}), file=sys.stderr)
        for b in (taps, codes, coef, psi, power, sweeps, kw["pilots"]):
            b.free()
    if old is not None:
        old.wifirx_destroy(old_h)
    rx.close()
    res = {"what": __doc__.split("\n\n")[0].replace("\n", " "), "iters": a.iters, "bits": BITS, "sigma": SIGMA, "runs": rows}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
