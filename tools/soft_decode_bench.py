#!/usr/bin/env python3
"""Hard vs soft-decision decode_mac in ONE process: python tools/soft_decode_bench.py [--frames 1000000] [--rounds 5]
[--out profiles/soft_decode_bench.json]

Config 2 geometry (QPSK 1/2, PSDU 294 B, slots of 4608 samples synthesised on the device at --snr dB): one demod writes
the records, the bit planes and the LLRs (llr_bits 2: 19.2 GB at a million frames -- the batch is cut to what 60 % of the
free device memory holds); then every round decodes the same batch with wifirx_decode_batch and with
wifirx_decode_batch_soft (wall time of the call + sync, ms; round 0 is the allocations and is dropped).  Afterwards the
frame error points of profiles/soft_decode_cpu_fer.json run through the device (demod + soft decode, llr_csi 0 / 1) and
are reported beside the CPU record.  Run it under `timeout -k 10 <s>`; any failed call ends it with the exception."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "gnuradio-wifi-imagetransfer_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)


def free_bytes():
    """hipMemGetInfo of the HIP runtime libwifirx.so already loaded (a second runtime, e.g. torch's, must not come in)"""
    hip = C.CDLL("libamdhip64.so", mode=C.RTLD_GLOBAL)
    free, total = C.c_size_t(0), C.c_size_t(0)
    if hip.hipMemGetInfo(C.byref(free), C.byref(total)) != 0:
        raise RuntimeError("hipMemGetInfo failed")
    return int(free.value)


def time_decode(capi, rx, n, frames0, b, out, soft):
    b["frames"].upload(frames0)                       # the records as the demod left them (decode sets flags in them)
    rx.sync()
    t = time.perf_counter()
    f = capi.lib().wifirx_decode_batch_soft if soft else capi.lib().wifirx_decode_batch
    rx._check(f(rx._h, n, C.byref(out)))
    rx.sync()
    ms = (time.perf_counter() - t) * 1e3
    fr = b["frames"].download(np.uint8, n * 32).view(capi.FRAME_DTYPE)
    return ms, int(((fr["flags"] & capi.F_CRC_OK) != 0).sum())


def fer_points(capi, n_rec):
    import soft_fer_points as sfp
    with open(sfp.OUT) as f:
        rec = json.load(f)
    res = []
    for (g, snr), p in zip(sfp.POINTS, rec["points"]):
        x, slot_len, max_sym, tx = sfp.point_frames(g, snr, rec["frames_per_point"])
        n = tx.shape[0]
        row = {"geometry": g, "snr_db": snr, "frames": n, "cpu_record": {k: p[k] for k in p if k.endswith("_delivered")}}
        for csi, tag in ((0, "soft"), (1, "soft_csi")):
            rx = capi.WifiRx(max_sym=max_sym, llr_bits=6, device=0)
            rx.set_param(capi.P_LLR_CSI, csi)
            r = rx.demod_batch(x, slot_len, decode=True, psdu_stride=320, soft=True)
            rx.close()
            row["gpu_" + tag + "_delivered"] = int(sfp.delivered(r["frames"], r["psdu"], tx).sum())
        row["gpu_equals_cpu"] = all(row["gpu_%s_delivered" % t] == p["%s_delivered" % t] for t in ("soft", "soft_csi"))
        row["hard_fer_cpu"] = p["hard_fer"]
        row["soft_csi_fer_gpu"] = 1.0 - row["gpu_soft_csi_delivered"] / n
        res.append(row)
        print(json.dumps(row), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1000000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--snr", type=float, default=20.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "soft_decode_bench.json"))
    a = ap.parse_args()
    from wifirx import capi, txgen
    tx = txgen.encode_psdus(txgen.make_psdus(64, 294, seed=5), 2)
    ms_sym = tx.n_sym
    slot, stride = 4608, 320
    per_frame = slot * 8 + 32 + ms_sym * 48 + ms_sym * 48 * 2 * 4 + stride
    rx = capi.WifiRx(max_sym=ms_sym, llr_bits=2, device=0)
    n = min(a.frames, int(0.6 * free_bytes()) // per_frame)
    iq = rx.alloc(n * slot * 8)
    rx.synth_slots(tx.samples, iq.ptr, slot, n, 160, a.snr, 0.037, 99)
    b = dict(frames=rx.alloc(n * 32), hbits=rx.alloc(n * ms_sym * 48), llr=rx.alloc(n * ms_sym * 48 * 2 * 4),
             psdu=rx.alloc(n * stride))
    out = capi.Out(b["frames"].ptr, None, b["llr"].ptr, None, b["psdu"].ptr, stride, 1, None, None, b["hbits"].ptr)
    rx._check(capi.lib().wifirx_demod_batch(rx._h, iq.ptr, 1, slot, n, C.byref(out)))
    rx.sync()
    iq.free()
    fr0 = b["frames"].download(np.uint8, n * 32).copy()
    hard, soft = [], []
    for rnd in range(a.rounds + 1):
        mh, ch = time_decode(capi, rx, n, fr0, b, out, False)
        ms, cs = time_decode(capi, rx, n, fr0, b, out, True)
        print("round %d: hard %.3f ms (crc ok %d)   soft %.3f ms (crc ok %d)" % (rnd, mh, ch, ms, cs), flush=True)
        if rnd:
            hard.append(mh)
            soft.append(ms)
    res = {"frames": n, "snr_db": a.snr, "geometry": "config 2: QPSK 1/2, 294 B, %d symbols" % ms_sym,
           "hard_ms": hard, "soft_ms": soft, "hard_ms_median": float(np.median(hard)), "soft_ms_median": float(np.median(soft)),
           "hard_ms_per_1M_frames": float(np.median(hard)) * 1e6 / n, "soft_ms_per_1M_frames": float(np.median(soft)) * 1e6 / n,
           "crc_ok_hard": ch, "crc_ok_soft": cs}
    for k in b.values():
        k.free()
    rx.close()
    print(json.dumps(res), flush=True)
    res["fer_points"] = fer_points(capi, n)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
