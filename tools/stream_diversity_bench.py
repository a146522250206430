"""Two measurements of stream-mode receive diversity (NUMERICS.md rule 24, wifirx_push_diversity).  Nobody had measured either,
so no aim is fixed and no ratio is asserted.  Prints one JSON line, writes it to --out when given.

1. The joint detection kernel (wifirx_detect_multi) for A = 1, 2, 4, 8 antennas over --samples samples per antenna (default
   64 M) of unit-variance noise, HIP events on the handle's stream after a warm-up, alternating in one process with a
   device-to-device hipMemcpyAsync that moves as many bytes as the call reads + writes (tools/diversity_bench.py's method and
   yardstick: the copy moves half the count, it reads and writes each byte it moves).  Medians of --windows windows; kernel /
   copy is reported, and a straight line through the four times: its slope is what an antenna costs (two 8-byte loads per
   sample and three summands), its intercept what does not depend on A (the window pass with its cross-lane reads, the stores).

2. Samples to PDUs: a device-resident stream of config-2 frames (294 bytes, QPSK 1/2; --frames of them, built on the device
   by wifirx_tx_batch and wifirx_channel at --snr dB, an independent noise seed per antenna) through push_diversity for A = 2
   and 4, next to ONE wifirx_push stream of one antenna, in the same process, alternating, wall-clock time from the push to
   the last polled frame.  Medians of --passes passes after a warm-up pass.

    python tools/stream_diversity_bench.py [--samples 67108864] [--windows 10] [--frames 2048] [--out profiles/stream_diversity.json]"""
import argparse
import ctypes as C
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gnuradio-wifi-imagetransfer_amd")]

from wifirx import capi, txgen  # noqa: E402

BLOCK = 1 << 20                                 # samples made on the host per antenna; the device repeats them
ENC, PLEN, LEAD, TAIL = 2, 294, 160, 79


def detect_part(a, hip):
    n = a.samples - a.samples % BLOCK
    rx = capi.WifiRx(max_sym=1, device=0)
    st = C.c_void_p(rx.stream_ptr())
    ev0, ev1 = C.c_void_p(), C.c_void_p()
    assert hip.hipEventCreate(C.byref(ev0)) == 0 and hip.hipEventCreate(C.byref(ev1)) == 0
    rng = np.random.default_rng(2)
    planes = []
    for _ in range(8):
        d = rx.alloc(n * 8)
        d.upload(((rng.standard_normal(BLOCK) + 1j * rng.standard_normal(BLOCK)) * np.sqrt(0.5)).astype(np.complex64))
        have = BLOCK
        while have < n:
            step = min(have, n - have)
            assert hip.hipMemcpyAsync(d.ptr + have * 8, d.ptr, step * 8, 3, st) == 0
            rx.sync()
            have += step
        planes.append(d)
    d_A, d_m = rx.alloc(n * 8), rx.alloc((n // 64 + 2) * 8)
    nbytes = {A: A * 8 * n + 8 * n + n // 8 for A in (1, 2, 4, 8)}
    scratch = rx.alloc(max(nbytes.values()))
    runs = {}
    for A in (1, 2, 4, 8):
        ptrs = [p.ptr for p in planes[:A]]
        runs["detect_A%d" % A] = lambda ptrs=ptrs: rx.detect_multi_dev(ptrs, n, 0.56, d_m.ptr, d_A.ptr) or 0
        runs["memcpy_A%d" % A] = lambda half=nbytes[A] // 2: hip.hipMemcpyAsync(scratch.ptr + half, scratch.ptr, half, 3, st)

    def window(fn, reps):
        assert hip.hipEventRecord(ev0, st) == 0
        for _ in range(reps):
            assert fn() == 0
        assert hip.hipEventRecord(ev1, st) == 0
        assert hip.hipEventSynchronize(ev1) == 0
        t = C.c_float()
        assert hip.hipEventElapsedTime(C.byref(t), ev0, ev1) == 0
        return t.value / reps

    reps = {}
    for name, fn in runs.items():
        window(fn, 2)
        reps[name] = max(int(np.ceil(100.0 / max(window(fn, 3), 1e-3))), 3)
    ms = {k: [] for k in runs}
    for _ in range(a.windows):
        for name, fn in runs.items():
            ms[name].append(window(fn, reps[name]))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    As = np.array([1, 2, 4, 8], dtype=np.float64)
    t = np.array([med["detect_A%d" % A] for A in (1, 2, 4, 8)])
    slope, intercept = np.polyfit(As, t, 1)
    res = dict(samples_per_antenna=n, bytes_read_plus_written={str(A): nbytes[A] for A in nbytes}, reps_per_window=reps, windows=a.windows,
               ms_windows=ms, ms={str(A): med["detect_A%d" % A] for A in (1, 2, 4, 8)},
               memcpy_d2d_ms={str(A): med["memcpy_A%d" % A] for A in (1, 2, 4, 8)},
               ratio_to_memcpy={str(A): med["detect_A%d" % A] / med["memcpy_A%d" % A] for A in (1, 2, 4, 8)},
               GBps={str(A): nbytes[A] / med["detect_A%d" % A] / 1e6 for A in (1, 2, 4, 8)},
               Gsamples_per_s_per_antenna={str(A): n / med["detect_A%d" % A] / 1e6 for A in (1, 2, 4, 8)},
               line_through_the_times=dict(ms_per_antenna=float(slope), ms_independent_of_antennas=float(intercept),
                                           ms_of_8_bytes_per_sample_at_the_copy_rate=float(8 * n / (nbytes[8] / med["memcpy_A8"]))),
               note="per call; HIP events around a window of calls, medians of the windows, kernels and copies alternating in one process; "
                    "bytes = A planes read + A written + the masks (P not requested); x[n - 16] is counted once, it comes from the caches")
    for d in planes + [d_A, d_m, scratch]:
        d.free()
    rx.close()
    return res


def stream_part(a):
    n = a.frames
    n_sym = txgen.n_sym_for(PLEN, ENC)
    slot = LEAD + txgen.frame_samples(PLEN, ENC) + TAIL
    slot += slot & 1
    total = n * slot
    gen = capi.WifiRx(max_sym=n_sym, device=0)
    psdus = txgen.make_psdus(n, PLEN, seed=31)
    d_psdu = gen.alloc(n * PLEN).upload(psdus)
    tx = gen.alloc(total * 8)
    ant = [gen.alloc(total * 8) for _ in range(4)]
    gen.tx_batch_dev(tx.ptr, total, d_psdu.ptr, ENC, psdu_len=np.full(n, PLEN, np.uint32), psdu_stride=PLEN, lead=LEAD, row_len=slot)
    for k, d in enumerate(ant):
        gen.channel_dev(tx.ptr, d.ptr, total, n, row_len=slot, gain=math.sqrt(10 ** (a.snr / 10)), noise_voltage=1.0, seed=700 + k)
    gen.sync()

    def make(A):
        rx = capi.WifiRx(max_sym=n_sym, device=0)
        rx.set_param(capi.P_STREAM_IDX, 0)              # PDUs only, as the block runs it
        return rx

    handles = {"single": make(1), "A2": make(2), "A4": make(4)}

    def one(name):
        rx = handles[name]
        t0 = time.perf_counter()
        if name == "single":
            rx._check(capi.lib().wifirx_push(rx._h, ant[0].ptr, total, 1))
            rx.flush()
            poll = rx.poll
        else:
            A = int(name[1:])
            rx.push_diversity_dev([d.ptr for d in ant[:A]], total)
            rx.flush_diversity()
            poll = rx.poll_diversity
        ok = 0
        while True:
            r = poll(cap=1024, psdu_stride=320)
            if len(r["frames"]) == 0:
                break
            ok += int(np.count_nonzero(r["frames"]["flags"] & capi.F_CRC_OK))
        return (time.perf_counter() - t0) * 1e3, ok

    for name in handles:
        one(name)                                       # warm-up: the handle's buffers are allocated here
    ms, ok = {k: [] for k in handles}, {}
    for _ in range(a.passes):
        for name in handles:
            t, ok[name] = one(name)
            ms[name].append(t)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    res = dict(workload="%d config-2 frames (294 B, QPSK 1/2, %d data symbols) at %g dB, %d samples per antenna, device-resident; "
                        "one push of the whole stream, a flush, every frame polled; hard decode, decisions not polled" % (n, n_sym, a.snr, total),
               passes=a.passes, ms_passes=ms, ms=med, frames_crc_ok=ok,
               Msamples_per_s_per_antenna={k: total / med[k] / 1e3 for k in med}, frames_per_s={k: n / med[k] * 1e3 for k in med},
               ratio_to_single={k: med[k] / med["single"] for k in med},
               note="wall-clock time of the caller's thread, medians of the passes, the three streams alternating in one process")
    for rx in handles.values():
        rx.close()
    for d in ant + [tx, d_psdu]:
        d.free()
    gen.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=1 << 26)
    ap.add_argument("--windows", type=int, default=10)
    ap.add_argument("--frames", type=int, default=2048)
    ap.add_argument("--snr", type=float, default=20.0)
    ap.add_argument("--passes", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    res = dict(detect=detect_part(a, hip), stream=stream_part(a))
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
