#!/usr/bin/env python3
"""float32 against bf16 LLR rows (WIFIRX_P_LLR_FORMAT, NUMERICS.md rule 15) in ONE process, on the same device batch:

    python tools/llr_bf16_bench.py [--frames 1000000] [--rounds 5] [--out profiles/llr_bf16_bench.json]

* the demod kernel time (wifirx_time_demod, 3 launches per round) on config 2 (QPSK 1/2, 294 B, slot 4608, llr_bits 2) and
  on the config-3 geometry (64-QAM 3/4, 294 B, slot 1472, AWGN 20 dB, llr_bits 6), the usual output set (records,
  decisions, LLRs); the formats alternate round by round (round 0 is dropped);
* wifirx_decode_batch_soft on config 2 over the rows of each format, against wifirx_decode_batch (call + sync, ms);
* the code-object metadata (VGPRs, spills, LDS, scratch) of every demod and soft-decoder instance of the library.
Slots are synthesised on the device (wifirx_synth_slots); the batch is cut to what 60 % of the free device memory holds.
Run it under `timeout -k 10 <s>`; any failed call ends it with the exception."""
import argparse
import ctypes as C
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gnuradio-wifi-imagetransfer_amd"))
LIB = os.path.join(ROOT, "gnuradio-wifi-imagetransfer_amd", "wifirx", "libwifirx.so")
LLVM = "/opt/rocm/lib/llvm/bin"


def free_bytes():
    """hipMemGetInfo of the HIP runtime libwifirx.so already loaded"""
    hip = C.CDLL("libamdhip64.so", mode=C.RTLD_GLOBAL)
    free, total = C.c_size_t(0), C.c_size_t(0)
    if hip.hipMemGetInfo(C.byref(free), C.byref(total)) != 0:
        raise RuntimeError("hipMemGetInfo failed")
    return int(free.value)


def kernel_resources():
    """{kernel: {vgpr_count, vgpr_spill_count, group_segment_fixed_size, private_segment_fixed_size, ...}} of the demod batch
    and soft-decoder instances, from the code objects' metadata notes"""
    res = {}
    with tempfile.TemporaryDirectory() as tmp:
        fat, cp = os.path.join(tmp, "fat.bin"), os.path.join(tmp, "lib.so")
        shutil.copyfile(LIB, cp)
        subprocess.check_call(["objcopy", "--dump-section", ".hip_fatbin=" + fat, cp, os.path.join(tmp, "out.so")],
                              stderr=subprocess.DEVNULL)
        data = open(fat, "rb").read()
        starts = [m.start() for m in re.finditer(b"__CLANG_OFFLOAD_BUNDLE__", data)]
        for n, (a, b) in enumerate(zip(starts, starts[1:] + [len(data)])):
            part, co = os.path.join(tmp, "p%d" % n), os.path.join(tmp, "co%d" % n)
            with open(part, "wb") as f:
                f.write(data[a:b])
            subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o",
                                   "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + part, "--output=" + co])
            notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True, capture_output=True,
                                   text=True).stdout
            cur = {}
            for line in notes.splitlines():
                if re.match(r"^  - \.", line):
                    cur = {}
                m = re.match(r"^  (?:- |  )\.name:\s+(\S+)", line)
                if m and re.search(r"demod_batch_kernel|decode_soft_kernel", m.group(1)) and not m.group(1).endswith(".kd"):
                    res[m.group(1)] = cur
                m = re.match(r"^  (?:- |  )\.(vgpr_count|sgpr_count|vgpr_spill_count|sgpr_spill_count|group_segment_fixed_size|"
                             r"private_segment_fixed_size):\s+(\d+)", line)
                if m:
                    cur[m.group(1)] = int(m.group(2))
    return res


def demod_times(capi, rx, iq_ptr, slot, n, out, rounds):
    t = {"f32": [], "bf16": []}
    for rnd in range(rounds + 1):
        for fmt, v in (("f32", capi.LLR_F32), ("bf16", capi.LLR_BF16)):
            rx.set_param(capi.P_LLR_FORMAT, v)
            ms = C.c_float(0)
            rx._check(capi.lib().wifirx_time_demod(rx._h, iq_ptr, slot, n, C.byref(out), 3, C.byref(ms)))
            if rnd:
                t[fmt].append(float(ms.value))
        print("round %d: %s" % (rnd, {k: v[-1:] for k, v in t.items()}), flush=True)
    return {"ms_f32": t["f32"], "ms_bf16": t["bf16"], "ms_f32_median": float(np.median(t["f32"])),
            "ms_bf16_median": float(np.median(t["bf16"])),
            "bf16_vs_f32": float(np.median(t["bf16"]) / np.median(t["f32"]) - 1.0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1000000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "llr_bf16_bench.json"))
    a = ap.parse_args()
    from wifirx import capi, txgen
    res = {"provenance": "python tools/llr_bf16_bench.py --frames %d --rounds %d" % (a.frames, a.rounds)}

    # ---- config 2: demod and decode ----
    tx = txgen.encode_psdus(txgen.make_psdus(64, 294, seed=5), 2)
    ms_sym, slot, stride, lb = tx.n_sym, 4608, 320, 2
    per_frame = slot * 8 + 32 + ms_sym * 48 * 2 + ms_sym * 48 * lb * 4 + stride
    rx = capi.WifiRx(max_sym=ms_sym, llr_bits=lb, device=0)
    n = min(a.frames, int(0.6 * free_bytes()) // per_frame)
    iq = rx.alloc(n * slot * 8)
    rx.synth_slots(tx.samples, iq.ptr, slot, n, 160, 20.0, 0.037, 99)
    b = dict(frames=rx.alloc(n * 32), idx=rx.alloc(n * ms_sym * 48), hbits=rx.alloc(n * ms_sym * 48),
             llr=rx.alloc(n * ms_sym * 48 * lb * 4), psdu=rx.alloc(n * stride))
    out = capi.Out(b["frames"].ptr, b["idx"].ptr, b["llr"].ptr, None, None, 0, 1, None, None, None)
    res["config2_demod"] = dict(frames=n, slot_len=slot, n_sym=ms_sym, llr_bits=lb,
                                llr_bytes_per_frame_f32=ms_sym * 48 * lb * 4, llr_bytes_per_frame_bf16=ms_sym * 48 * lb * 2,
                                **demod_times(capi, rx, iq.ptr, slot, n, out, a.rounds))
    print(json.dumps(res["config2_demod"]), flush=True)
    # decode: the rows of both formats side by side (float32 in b["llr"], bf16 in a buffer of their own) from one demod of
    # each format; then hard, soft on float32 and soft on bf16 rows alternately, from the same records
    llr16 = rx.alloc(n * ms_sym * 48 * lb * 2)
    dout = capi.Out(b["frames"].ptr, None, b["llr"].ptr, None, b["psdu"].ptr, stride, 1, None, None, b["hbits"].ptr)
    out16 = capi.Out(b["frames"].ptr, None, llr16.ptr, None, b["psdu"].ptr, stride, 1, None, None, b["hbits"].ptr)
    dec = {"hard": [], "soft_f32": [], "soft_bf16": []}
    crc = {}
    fr0 = {}
    for fmt, v, o in (("bf16", capi.LLR_BF16, out16), ("f32", capi.LLR_F32, dout)):
        rx.set_param(capi.P_LLR_FORMAT, v)
        rx._check(capi.lib().wifirx_demod_batch(rx._h, iq.ptr, 1, slot, n, C.byref(o)))
        rx.sync()
        fr0[fmt] = b["frames"].download(np.uint8, n * 32).copy()
    assert np.array_equal(fr0["f32"], fr0["bf16"])
    iq.free()

    def timed(f, o, fmt):
        b["frames"].upload(fr0["f32"])
        rx.set_param(capi.P_LLR_FORMAT, fmt)
        rx.sync()
        t = time.perf_counter()
        rx._check(f(rx._h, n, C.byref(o)))
        rx.sync()
        ms = (time.perf_counter() - t) * 1e3
        fr = b["frames"].download(np.uint8, n * 32).view(capi.FRAME_DTYPE)
        return ms, int(((fr["flags"] & capi.F_CRC_OK) != 0).sum())

    for rnd in range(a.rounds + 1):
        row = {}
        row["hard"] = timed(capi.lib().wifirx_decode_batch, dout, capi.LLR_F32)
        row["soft_f32"] = timed(capi.lib().wifirx_decode_batch_soft, dout, capi.LLR_F32)
        row["soft_bf16"] = timed(capi.lib().wifirx_decode_batch_soft, out16, capi.LLR_BF16)
        print("decode round %d: %s" % (rnd, row), flush=True)
        if rnd:
            for k, (ms, c) in row.items():
                dec[k].append(ms)
                crc[k] = c
    res["config2_decode"] = dict(frames=n, **{k + "_ms": v for k, v in dec.items()},
                                 **{k + "_ms_median": float(np.median(v)) for k, v in dec.items()},
                                 **{"crc_ok_" + k: v for k, v in crc.items()})
    print(json.dumps(res["config2_decode"]), flush=True)
    for k in b.values():
        k.free()
    llr16.free()
    rx.close()

    # ---- config-3 geometry: demod ----
    tx = txgen.encode_psdus(txgen.make_psdus(64, 294, seed=6), 7)
    ms_sym, slot, lb = tx.n_sym, 1472, 6
    per_frame = slot * 8 + 32 + ms_sym * 48 + ms_sym * 48 * lb * 4
    rx = capi.WifiRx(max_sym=ms_sym, llr_bits=lb, device=0)
    n = min(a.frames, int(0.6 * free_bytes()) // per_frame)
    iq = rx.alloc(n * slot * 8)
    rx.synth_slots(tx.samples, iq.ptr, slot, n, 160, 20.0, 0.0, 98)
    b = dict(frames=rx.alloc(n * 32), idx=rx.alloc(n * ms_sym * 48), llr=rx.alloc(n * ms_sym * 48 * lb * 4))
    out = capi.Out(b["frames"].ptr, b["idx"].ptr, b["llr"].ptr, None, None, 0, 1, None, None, None)
    res["config3_geometry_demod"] = dict(frames=n, slot_len=slot, n_sym=ms_sym, llr_bits=lb,
                                         llr_bytes_per_frame_f32=ms_sym * 48 * lb * 4,
                                         llr_bytes_per_frame_bf16=ms_sym * 48 * lb * 2,
                                         **demod_times(capi, rx, iq.ptr, slot, n, out, a.rounds))
    print(json.dumps(res["config3_geometry_demod"]), flush=True)
    for k in list(b.values()) + [iq]:
        k.free()
    rx.close()

    try:
        res["kernel_resources"] = kernel_resources()
    except (OSError, subprocess.CalledProcessError) as e:
        res["kernel_resources"] = "not read: %s" % e
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
