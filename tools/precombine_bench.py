"""Time wifirx_precombine (NUMERICS.md rule 33) at config 2's geometry -- rows of 4608 samples holding one QPSK-1/2 frame of 294
bytes each, made on the device (wifirx_tx_batch, then one flat Rayleigh wifirx_channel_fading call per antenna at 15 dB) -- for
A = 2, 4 and 8 antennas, with HIP events on the handle's stream after a warm-up, alternating in one process with

  * a device-to-device hipMemcpyAsync that moves as many bytes as the call must read and write at least, 8 (A + 1) per sample
    (tools/combine_bench.py's yardstick: the copy moves half the count, since it reads and writes each byte it moves), and
  * what the call replaces: one more wifirx_demod_batch launch per further antenna (points and estimates written, as rule 23
    needs them) and the wifirx_diversity_combine pass over A antennas (decisions and LLRs out).

A timed window holds enough repetitions to last about 0.1 s; the figures are per call, medians over the windows.  Nothing is
asserted.  Prints one JSON line, writes it to --out when given.

    python tools/precombine_bench.py [--frames 32768] [--windows 10] [--iters 2] [--out profiles/precombine_config.json]"""
import argparse
import ctypes as C
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gnuradio-wifi-imagetransfer_amd")]

from wifirx import capi, txgen  # noqa: E402

SLOT, LEAD, ENC, PSDU_LEN, SNR_DB = 4608, 160, 2, 294, 15.0
COUNTS = (2, 4, 8)


def device_name():
    try:
        import torch
        p = torch.cuda.get_device_properties(0)
        return "%s (%s, %d CUs)" % (p.name, getattr(p, "gcnArchName", "?"), p.multi_processor_count)
    except Exception as e:
        return "unknown (%s)" % e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32768, help="slots per antenna (8 antennas and the output: 332 KB per slot)")
    ap.add_argument("--windows", type=int, default=10)
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n = a.frames
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    n_sym = txgen.n_sym_for(PSDU_LEN, ENC)
    rx = capi.WifiRx(max_sym=n_sym, llr_bits=2, want_carrier=True, device=0)
    st = C.c_void_p(rx.stream_ptr())
    ev0, ev1 = C.c_void_p(), C.c_void_p()
    assert hip.hipEventCreate(C.byref(ev0)) == 0 and hip.hipEventCreate(C.byref(ev1)) == 0
    row_b = SLOT * 8

    d_psdu, tx = rx.alloc(n * PSDU_LEN), rx.alloc(n * row_b)
    rx.mac_batch_dev(d_psdu.ptr, PSDU_LEN, n, None, payload_len=PSDU_LEN - 28, payload_seed=1)
    rx.tx_batch_dev(tx.ptr, n * SLOT, d_psdu.ptr, ENC, psdu_len=np.full(n, PSDU_LEN, np.uint32), psdu_stride=PSDU_LEN, lead=LEAD, row_len=SLOT)
    iqs = [rx.alloc(n * row_b) for _ in range(COUNTS[-1])]
    for ant, iq in enumerate(iqs):
        rx.channel_dev(tx.ptr, iq.ptr, n * SLOT, n, row_len=SLOT, gain=math.sqrt(10 ** (SNR_DB / 10)), noise_voltage=1.0, seed=700 + ant,
                       doppler=0.0, fade_seed=40 + ant)
    rx.sync()
    tx.free()
    y, d_w, d_s = rx.alloc(n * row_b), rx.alloc(n * COUNTS[-1] * 8), rx.alloc(n * 16)
    ins = [rx.alloc_out(n, want_csi=True) for _ in range(COUNTS[-1])]
    out = rx.alloc_out(n)
    for ant, dev in enumerate(ins):                 # rule 23's inputs, once; the timed demod below is antenna 0's
        rx.demod_batch_dev(iqs[ant].ptr, SLOT, n, dev)
    rx.sync()

    def call(fn, *args):
        fn(*args)
        return 0

    ops, nbytes = {}, {}
    ops["demod"] = lambda: call(rx.demod_batch_dev, iqs[0].ptr, SLOT, n, ins[0])
    for A in COUNTS:
        ptrs = [b.ptr for b in iqs[:A]]
        ops["precombine_A%d" % A] = lambda A=A, ptrs=ptrs: call(rx.precombine_dev, ptrs, SLOT, n, y.ptr, a.iters, d_w.ptr, d_s.ptr)
        nbytes["precombine_A%d" % A] = n * row_b * (A + 1)
        ops["mrc_A%d" % A] = lambda A=A: call(rx.diversity_combine_dev, ins[:A], n, dict(frames=out["frames"], idx=out["idx"], llr=out["llr"]), capi.DIV_MRC)
    scratch = rx.alloc(max(nbytes.values()))        # the copies' own buffer
    copies = {"memcpy_A%d" % A: (lambda half=nbytes["precombine_A%d" % A] // 2: hip.hipMemcpyAsync(scratch.ptr + half, scratch.ptr, half, 3, st))
              for A in COUNTS}

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
    stats = d_s.download(capi.PRE_STATS_DTYPE, n)
    by_A = {}
    for A in COUNTS:
        t, floor = med["precombine_A%d" % A], nbytes["precombine_A%d" % A]
        replaced = (A - 1) * med["demod"] + med["mrc_A%d" % A]
        by_A[str(A)] = dict(ms=t, memcpy_d2d_ms=med["memcpy_A%d" % A], ratio_to_memcpy=t / med["memcpy_A%d" % A],
                            GBps_at_floor_bytes=floor / t / 1e6, GBps_if_second_read_misses=n * row_b * (2 * A + 1) / t / 1e6,
                            complex_macs_per_s=n * SLOT * (A * (A + 1) // 2 + A) / t * 1e3,
                            ms_per_million_slots=t / n * 1e6, replaced_ms=replaced, replaced_over_precombine=replaced / t,
                            mrc_ms=med["mrc_A%d" % A])
    res = dict(workload="config 2's geometry: %d slots of %d samples per antenna, one QPSK-1/2 frame of %d bytes each, flat Rayleigh at %g dB; "
                        "%d power iterations; weights and stats written" % (n, SLOT, PSDU_LEN, SNR_DB, a.iters),
               device=device_name(), frames=n, iters=a.iters, demod_ms=med["demod"], demod_ms_per_million_slots=med["demod"] / n * 1e6,
               by_antennas=by_A, floor_bytes=nbytes, reps_per_window=reps, windows=a.windows, ms_windows=ms,
               degenerate_slots_last_call=int((stats["flags"] != 0).sum()),
               note="every figure is per call, HIP events around a window of calls, medians of the windows, kernels and copies alternating in one "
                    "process; floor bytes = 8 (A + 1) per sample (every input read once from memory, the second read from cache, the output "
                    "written); the memcpy moves half that count; replaced = (A - 1) demod launches + the rule-23 pass over A antennas")
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    for d in ins + [out]:
        rx.free_out(d)
    for b in iqs + [y, d_w, d_s, scratch, d_psdu]:
        b.free()
    rx.close()


if __name__ == "__main__":
    main()
