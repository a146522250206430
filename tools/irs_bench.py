"""Time wifirx_irs_taps at config 3's geometry -- 1 M tap sets of 8 taps, Philox scatter, K = 10 -- for surfaces of 64, 256
and 1024 elements, with given phases and with align_bits = 2, with HIP events on the handle's stream after a warm-up.  Every
call covers the whole entry point: the upload of the line-of-sight vectors, the scales and host psi (a few kB), then the
kernel.  On the same box, the NumPy restatement (tests/irs_ref.py) on 1024 sets.  There is no earlier kernel to compare with.
Prints one JSON line, writes it to --out when given.

    python tools/irs_bench.py [--iters 3] [--sets 1000000] [--out profiles/irs_config3.json]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gnuradio-wifi-imagetransfer_amd"), os.path.join(ROOT, "tests")]

from wifirx import capi, irs  # noqa: E402

SETS, L, SIZES, BITS, K = 1_000_000, 8, (64, 256, 1024), 2, 10.0
HOST_SETS = 1024


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--sets", type=int, default=SETS)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n = a.sets
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

    pdp = np.exp(-np.arange(L) / 2.0)
    pdp = (pdp / pdp.sum()).astype(np.float32)
    d_taps = rx.alloc(n * L * 8)
    runs, scenes = {}, {}
    for N in SIZES:
        S = int(round(N ** 0.5))
        b2r, r2u, b2u = irs.los(S, [0.015, 0.015, 0], [S * 0.015, S * 0.015, 4.5], [S * 0.015 + 0.3, S * 0.015 - 0.2, 1.0])
        psi = irs.random_psi(N, BITS, N)
        scenes[N] = (b2r, r2u, b2u, psi)
        common = dict(gain=1.0 / N ** 0.5, k_factor=K, seed=7)
        runs["given_psi_N%d" % N] = (lambda s=scenes[N], kw=common: rx.irs_taps_dev(d_taps, n, pdp, s[0], s[1], s[2], psi=s[3], **kw))
        runs["align2_N%d" % N] = (lambda s=scenes[N], kw=common: rx.irs_taps_dev(d_taps, n, pdp, s[0], s[1], s[2], align_bits=BITS, **kw))
    for fn in runs.values():                                            # warm-up of each
        fn()
    rx.sync()
    ms = {k: [] for k in runs}
    for _ in range(2):                                                  # alternate them, twice
        for k, fn in runs.items():
            ms[k] += timed(fn)
    med = {k: float(np.median(v)) for k, v in ms.items()}

    import irs_ref
    host = {}
    for N in SIZES:
        b2r, r2u, b2u, psi = scenes[N]
        for name, kw in (("given_psi", dict(psi=psi)), ("align2", dict(align_bits=BITS))):
            t0 = time.perf_counter()
            irs_ref.irs_taps(HOST_SETS, pdp, b2r, r2u, b2u, gain=1.0 / N ** 0.5, k_factor=K, seed=7, **kw)
            host["%s_N%d" % (name, N)] = (time.perf_counter() - t0) * 1e3

    def elems(k):
        return int(k.rsplit("N", 1)[1]) * L * n

    res = dict(workload="wifirx_irs_taps config 3: %d tap sets of %d taps, Philox scatter, k_factor %g, direct path on" % (n, L, K),
               bytes_written=n * L * 8, ms=ms, ms_median=med,
               Gelements_per_s={k: elems(k) / med[k] / 1e6 for k in med},
               ratio_align2_to_given={"N%d" % N: med["align2_N%d" % N] / med["given_psi_N%d" % N] for N in SIZES},
               numpy_restatement=dict(sets=HOST_SETS, ms=host,
                                      Melements_per_s={k: int(k.rsplit("N", 1)[1]) * L * HOST_SETS / v / 1e3 for k, v in host.items()}),
               note="every call covers the upload of the host arrays (line-of-sight vectors, scales, psi: at most 25 kB) and the "
                    "kernel; an element is one (a_n, b_n) pair: a Philox draw, two Box-Mullers, the mix, two complex products")
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    d_taps.free()
    rx.close()


if __name__ == "__main__":
    main()
