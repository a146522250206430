"""Time wifirx_diversity_combine (NUMERICS.md rule 23) at config 2's geometry -- QPSK 1/2, 50 data symbols per frame, 2 LLRs
per carrier -- for A = 2 and 4 antennas, maximal-ratio combining and selection, with every output (points, decisions, LLRs)
and with what a decoder needs (decisions, LLRs), on host-built rows (every antenna usable, random points and estimates), with
HIP events on the handle's stream after a warm-up, alternating in one process with device-to-device hipMemcpyAsync calls that
move as many bytes as the call reads + writes (tools/combine_bench.py's method and yardstick).  A timed window holds enough
repetitions to last about 0.1 s; the figures are per call, medians over the windows.  No ratio is asserted.  Prints one JSON
line, writes it to --out when given.

    python tools/diversity_bench.py [--frames 262144] [--windows 10] [--out profiles/diversity_config2.json]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gnuradio-wifi-imagetransfer_amd")]

from wifirx import capi  # noqa: E402

N_SYM, ENC, N_BPSC, PSDU_LEN = 50, 2, 2, 294
BLOCK = 4096                                    # frames made on the host; the device repeats them
GOOD = capi.F_DETECTED | capi.F_SYNC | capi.F_SIGNAL | capi.F_COMPLETE


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=262144)
    ap.add_argument("--windows", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n = a.frames - a.frames % BLOCK
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    rx = capi.WifiRx(max_sym=N_SYM, llr_bits=N_BPSC, want_carrier=True, device=0)
    st = C.c_void_p(rx.stream_ptr())
    ev0, ev1 = C.c_void_p(), C.c_void_p()
    assert hip.hipEventCreate(C.byref(ev0)) == 0 and hip.hipEventCreate(C.byref(ev1)) == 0
    lib = capi.lib()
    car_b, csi_b, idx_b, llr_b = N_SYM * 48 * 8, 52 * 8, N_SYM * 48, N_SYM * 48 * N_BPSC * 4

    def repeated(block: np.ndarray, per_frame: int):
        """a device buffer of n frames: the block of BLOCK frames, doubled on the device until it is full"""
        d = rx.alloc(n * per_frame)
        d.upload(block)
        have = BLOCK
        while have < n:
            step = min(have, n - have)
            assert hip.hipMemcpyAsync(d.ptr + have * per_frame, d.ptr, step * per_frame, 3, st) == 0
            rx.sync()
            have += step
        return d

    rng = np.random.default_rng(1)
    ins = []
    for ant in range(4):
        f = np.zeros(BLOCK, capi.FRAME_DTYPE)
        f["flags"], f["snr_db"] = GOOD, rng.uniform(5, 25, BLOCK)
        f["psdu_len"], f["encoding"], f["n_bpsc"], f["n_sym"], f["n_sym_out"] = PSDU_LEN, ENC, N_BPSC, N_SYM, N_SYM
        ins.append(dict(frames=repeated(f, 32),
                        carrier=repeated(rng.normal(0, 0.7, (BLOCK, N_SYM * 48 * 2)).astype(np.float32), car_b),
                        csi=repeated(rng.normal(0, 1, (BLOCK, 104)).astype(np.float32), csi_b)))
    out = dict(frames=rx.alloc(n * 32), idx=rx.alloc(n * idx_b), llr=rx.alloc(n * llr_b), carrier=rx.alloc(n * car_b))
    mask = rx.alloc(n)

    ops, nbytes = {}, {}
    for A in (2, 4):
        arr = (capi.Out * A)(*[rx._out_struct(d) for d in ins[:A]])
        for mode, mname in ((capi.DIV_MRC, "mrc"), (capi.DIV_SELECT, "select")):
            for oname, keys in (("all_outputs", ("frames", "idx", "llr", "carrier")), ("idx_llr", ("frames", "idx", "llr"))):
                o = rx._out_struct({k: out[k] for k in keys})
                name = "A%d_%s_%s" % (A, mname, oname)
                ops[name] = lambda A=A, arr=arr, mode=mode, o=o: lib.wifirx_diversity_combine(rx._h, A, arr, n, mode, None, C.byref(o), mask.ptr)
                contributing = A if mode == capi.DIV_MRC else 1
                nbytes[name] = n * (A * 32 + contributing * (car_b + csi_b) + 32 + 1 + idx_b + llr_b + (car_b if "carrier" in keys else 0))
    sizes = sorted(set(nbytes.values()))
    scratch = rx.alloc(max(sizes))                 # the copies' own buffer
    copies = {"memcpy_%d" % b: (lambda half=b // 2: hip.hipMemcpyAsync(scratch.ptr + half, scratch.ptr, half, 3, st)) for b in sizes}

    def window(fn, reps):
        assert hip.hipEventRecord(ev0, st) == 0
        for _ in range(reps):
            assert fn() == 0
        assert hip.hipEventRecord(ev1, st) == 0
        assert hip.hipEventSynchronize(ev1) == 0
        t = C.c_float()
        assert hip.hipEventElapsedTime(C.byref(t), ev0, ev1) == 0
        return t.value / reps

    runs = dict(ops)
    runs.update(copies)
    reps = {}
    for name, fn in runs.items():
        window(fn, 2)
        reps[name] = max(int(np.ceil(100.0 / max(window(fn, 3), 1e-3))), 3)
    ms = {k: [] for k in runs}
    for _ in range(a.windows):
        for name, fn in runs.items():
            ms[name].append(window(fn, reps[name]))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    ratio = {name: med[name] / med["memcpy_%d" % nbytes[name]] for name in ops}
    res = dict(workload="config 2's geometry: %d frames per antenna, QPSK 1/2, %d data symbols, 2 LLRs per carrier (float32); host-built rows, "
                        "every antenna usable; all_outputs = points + decisions + LLRs, idx_llr = decisions + LLRs" % (n, N_SYM),
               bytes_read_plus_written=nbytes, reps_per_window=reps, windows=a.windows, ms_windows=ms,
               ms={name: med[name] for name in ops}, memcpy_d2d_ms={str(b): med["memcpy_%d" % b] for b in sizes},
               GBps={name: nbytes[name] / med[name] / 1e6 for name in ops},
               frames_per_s={name: n / med[name] * 1e3 for name in ops}, ratio_to_memcpy=ratio,
               note="every figure is per call, HIP events around a window of calls, medians of the windows, kernels and copies "
                    "alternating in one process; the memcpy moves half the byte count (it reads and writes each byte it moves); "
                    "bytes = A records + per contributing antenna its points and estimates + the outputs written")
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    for d in ins + [out]:
        for v in d.values():
            v.free()
    mask.free()
    scratch.free()
    rx.close()


if __name__ == "__main__":
    main()
