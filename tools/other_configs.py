#!/usr/bin/env python3
"""The demod and decode_mac kernels on frame geometries other than bench.py's config 2: device-resident batches
generated like bench.py's (host templates -> Philox AWGN + CFO on the GPU), kernel time by HIP events, throughput
and the algorithmic-bytes fraction of the 8 TB/s roofline (SURVEY.md 8(d) formula).  Prints one JSON line.

    python tools/other_configs.py [frames=1000000]
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gnuradio-wifi-imagetransfer_amd"))
from wifirx import capi, txgen  # noqa: E402

CASES = [   # name, encoding, PSDU bytes, slot length
    ("config 3 geometry: 64-QAM 3/4, 294 B, slot 1472", 7, 294, 1472),
    ("config 1 geometry: BPSK 1/2, 294 B, slot 8576", 0, 294, 8576),
    ("16-QAM 1/2, 1000 B, slot 7424", 4, 1000, 7424),
    ("config 2: QPSK 1/2, 294 B, slot 4608", 2, 294, 4608),
]


def main():
    n_frames = int(sys.argv[1]) if len(sys.argv) > 1 else 1000000
    res = []
    only = os.environ.get("WIFIRX_ONLY_CASE")          # A/B runs: one geometry, demod only
    for name, enc, plen, slot_len in ((CASES if only is None else [CASES[int(only)]]) if not os.environ.get("WIFIRX_ONLY_EQ") else []):
        n_sym = txgen.n_sym_for(plen, enc)
        n_bpsc = txgen.RATE_TABLE[enc][0]
        tx = txgen.encode_psdus(txgen.make_psdus(256, plen, seed=5), enc)
        assert 160 + tx.samples.shape[1] <= slot_len
        rx = capi.WifiRx(max_sym=n_sym, llr_bits=n_bpsc)
        slots = rx.alloc(n_frames * slot_len * 8)
        dev = rx.alloc_out(n_frames, psdu_stride=((plen + 63) // 64) * 64, want_hbits=True)
        rx.synth_slots(tx.samples, slots.ptr, slot_len, n_frames, 160, 25.0, 0.037, 77)
        # the contract's outputs (idx, LLRs, records) first; then the same kernel also writing the bit planes decode_mac reads
        planes = dev.pop("hbits")
        dev["hbits"] = None
        # every figure of this script: the best of three means of three launches, after two warm-up launches (the first
        # case of a process otherwise carries the clock ramp: 7.65 vs 7.28 ms on the same box)
        rx.time_demod(slots.ptr, slot_len, n_frames, dev, iters=2)
        ms = min(rx.time_demod(slots.ptr, slot_len, n_frames, dev, iters=3) for _ in range(3))
        dev["hbits"] = planes
        rx.time_demod(slots.ptr, slot_len, n_frames, dev, iters=1)
        ms_planes = min(rx.time_demod(slots.ptr, slot_len, n_frames, dev, iters=3) for _ in range(3))
        rx.decode_batch_dev(n_frames, dev); rx.sync()
        t = time.perf_counter()
        rx.decode_batch_dev(n_frames, dev); rx.sync()
        dec_ms = (time.perf_counter() - t) * 1e3
        fr = dev["frames"].download(capi.FRAME_DTYPE, n_frames)
        bpf = 8 * slot_len + 48 * n_sym * (1 + 4 * n_bpsc) + 32
        res.append({"case": name, "frames": n_frames, "n_sym": n_sym, "demod_ms": ms,
                    "gsamples_per_s": n_frames * slot_len / ms / 1e6, "algorithmic_bytes_per_frame": bpf,
                    "roofline_frac": bpf * n_frames / (ms * 1e-3) / 8e12, "demod_with_planes_ms": ms_planes, "decode_mac_ms": dec_ms,
                    "crc_ok": int(((fr["flags"] & capi.F_CRC_OK) != 0).sum())})
        rx.free_out(dev); slots.free(); rx.close()
    if only is not None:
        print(json.dumps({"cases": res, "equalisers": []}))
        return
    # several rates in one batch (decode_mac groups the frames by rate): QPSK-1/2 and 16-QAM-3/4 frames alternate
    if not os.environ.get("WIFIRX_ONLY_EQ"):
        plen, slot_len = 294, 4608
        ta = txgen.encode_psdus(txgen.make_psdus(128, plen, seed=5), 2)
        tb = txgen.encode_psdus(txgen.make_psdus(128, plen, seed=6), 5)
        flen = max(ta.samples.shape[1], tb.samples.shape[1])
        tmpl = np.zeros((256, flen), np.complex64)
        tmpl[0::2, :ta.samples.shape[1]] = ta.samples
        tmpl[1::2, :tb.samples.shape[1]] = tb.samples
        n_sym = max(ta.n_sym, tb.n_sym)
        rx = capi.WifiRx(max_sym=n_sym, llr_bits=4)
        slots = rx.alloc(n_frames * slot_len * 8)
        dev = rx.alloc_out(n_frames, psdu_stride=320, want_hbits=True)
        rx.synth_slots(tmpl, slots.ptr, slot_len, n_frames, 160, 25.0, 0.037, 77)
        rx.time_demod(slots.ptr, slot_len, n_frames, dev, iters=2)
        ms = min(rx.time_demod(slots.ptr, slot_len, n_frames, dev, iters=3) for _ in range(3))
        rx.decode_batch_dev(n_frames, dev); rx.sync()
        t = time.perf_counter()
        rx.decode_batch_dev(n_frames, dev); rx.sync()
        dec_ms = (time.perf_counter() - t) * 1e3
        fr = dev["frames"].download(capi.FRAME_DTYPE, n_frames)
        res.append({"case": "mixed rates: QPSK 1/2 and 16-QAM 3/4 frames alternate, 294 B, slot 4608", "frames": n_frames,
                    "n_sym": [int(ta.n_sym), int(tb.n_sym)], "demod_ms": ms, "gsamples_per_s": n_frames * slot_len / ms / 1e6,
                    "decode_mac_ms": dec_ms, "crc_ok": int(((fr["flags"] & capi.F_CRC_OK) != 0).sum())})
        rx.free_out(dev); slots.free(); rx.close()
    # the other equalisers on config 2's geometry (their kernel instances are parity-tested, not tuned)
    eqs = []
    for name, enc, plen, slot_len in (CASES[-1], CASES[0]):
      n_sym, n_bpsc = txgen.n_sym_for(plen, enc), txgen.RATE_TABLE[enc][0]
      tx = txgen.encode_psdus(txgen.make_psdus(256, plen, seed=5), enc)
      for ce, en in enumerate(("LS", "LMS", "COMB", "STA")):
        rx = capi.WifiRx(max_sym=n_sym, llr_bits=n_bpsc, chan_est=ce)
        slots = rx.alloc(n_frames * slot_len * 8)
        dev = rx.alloc_out(n_frames, psdu_stride=320)
        rx.synth_slots(tx.samples, slots.ptr, slot_len, n_frames, 160, 25.0, 0.037, 77)
        rx.time_demod(slots.ptr, slot_len, n_frames, dev, iters=2)
        ms = min(rx.time_demod(slots.ptr, slot_len, n_frames, dev, iters=3) for _ in range(3))     # the best of three means of three
        eqs.append({"geometry": name, "chan_est": en, "demod_ms": ms, "gsamples_per_s": n_frames * slot_len / ms / 1e6})
        rx.free_out(dev); slots.free(); rx.close()
    for e in eqs:
        ls = [x for x in eqs if x["geometry"] == e["geometry"] and x["chan_est"] == "LS"][0]
        e["vs_LS"] = e["demod_ms"] / ls["demod_ms"]
    if os.environ.get("WIFIRX_ONLY_EQ"):
        res = []
    print(json.dumps({"cases": res, "equalisers": eqs}))


if __name__ == "__main__":
    main()
