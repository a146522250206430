#!/usr/bin/env python3
"""Hard vs soft decode_mac frame error rates on the CPU: the oracle demodulates (llr_bits = 6, llr_csi 0 and 1), the
oracle's decode_batch gives the hard result, tests/soft_viterbi_ref.py the soft one (NUMERICS.md rule 14).

    python tests/soft_fer_points.py [frames_per_point=2000]       # writes profiles/soft_decode_cpu_fer.json

Points: BASELINE config 3 (64-QAM 3/4, PSDU 294 B, SV multipath tests/golden/sv_taps.npy, LS, CFO in +-20 ppm) at 20, 25,
30 dB -- the frames of tests/golden/make_config3_ber_table.py --, and QPSK 1/2 on AWGN near its hard FER of 0.5.
tests/test_soft_decode_ref.py reruns the points and checks the counts; tests/test_gpu_soft_decode.py checks the device
against them.  A frame counts as delivered when its CRC is good and its PSDU is the transmitted one.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "gnuradio-wifi-imagetransfer_amd"), os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

from wifirx import txgen  # noqa: E402  (NumPy transmitter)

import soft_viterbi_ref as ref  # noqa: E402

CFO_20PPM = 2 * np.pi * 20e-6 * 5.89e9 / 20e6
POINTS = [("config3_sv", 20.0), ("config3_sv", 25.0), ("config3_sv", 30.0), ("qpsk12_awgn", 6.5)]
OUT = os.path.join(ROOT, "profiles", "soft_decode_cpu_fer.json")


def point_frames(geometry: str, snr_db: float, n: int):
    """(iq [n * slot_len] complex64, slot_len, max_sym, transmitted PSDUs [n][len]) of one point, seeded by the point."""
    lead = 160
    if geometry == "config3_sv":
        taps = np.load(os.path.join(ROOT, "tests", "golden", "sv_taps.npy"))
        n_t = taps.shape[0]
        psdu = txgen.make_psdus(n_t, 294, seed=31)
        tx = txgen.encode_psdus(psdu, 7)
        faded = txgen.impair(tx.samples, None, cfo=0.0, lead=0, total=tx.samples.shape[1] + 8, taps=taps)
        tmpl = np.arange(n) % n_t
        slot_len = 1472
        rng = np.random.default_rng(7000 + int(snr_db))
        x = txgen.impair(faded[tmpl], float(snr_db), cfo=rng.uniform(-CFO_20PPM, CFO_20PPM, n), lead=lead,
                         total=slot_len, seed=9000 + int(snr_db))
        return x.reshape(-1), slot_len, tx.n_sym, psdu[tmpl]
    if geometry == "qpsk12_awgn":
        psdu = txgen.make_psdus(n, 294, seed=77)
        tx = txgen.encode_psdus(psdu, 2)
        slot_len = ((lead + tx.samples.shape[1] + 320 + 63) // 64) * 64
        rng = np.random.default_rng(7100 + int(10 * snr_db))
        x = txgen.impair(tx.samples, float(snr_db), cfo=rng.uniform(-CFO_20PPM, CFO_20PPM, n), lead=lead,
                         total=slot_len, seed=9100 + int(10 * snr_db))
        return x.reshape(-1), slot_len, tx.n_sym, psdu
    raise ValueError(geometry)


def delivered(frames, psdu, tx_psdu):
    ln = tx_psdu.shape[1]
    return ((frames["flags"] & ref.F_CRC_OK) != 0) & (frames["psdu_len"] == ln) & (psdu[:, :ln] == tx_psdu).all(axis=1)


def run_point(orc, geometry: str, snr_db: float, n: int, threads=None) -> dict:
    threads = threads or os.cpu_count() or 1
    x, slot_len, max_sym, tx_psdu = point_frames(geometry, snr_db, n)
    r = {"geometry": geometry, "snr_db": snr_db, "frames": n}
    for csi in (0, 1):
        prm = orc.make_params(max_sym=max_sym, llr_bits=6, llr_csi=csi)
        o = orc.demod_batch(x, slot_len, prm, n_threads=threads)
        if csi == 0:
            fr_h = o["frames"].copy()
            hp = orc.decode_batch(fr_h, o["idx"], prm, psdu_stride=320, n_threads=threads)
            ok = delivered(fr_h, hp, tx_psdu)
            r["hard_crc_ok"] = int(((fr_h["flags"] & ref.F_CRC_OK) != 0).sum())
            r["hard_delivered"] = int(ok.sum())
        fr_s, sp = ref.decode_batch(o["frames"], o["llr"], max_sym, psdu_stride=320)
        tag = "soft_csi" if csi else "soft"
        ok = delivered(fr_s, sp, tx_psdu)
        r[tag + "_crc_ok"] = int(((fr_s["flags"] & ref.F_CRC_OK) != 0).sum())
        r[tag + "_delivered"] = int(ok.sum())
    for tag in ("hard", "soft", "soft_csi"):
        r[tag + "_fer"] = 1.0 - r[tag + "_delivered"] / n
    return r


def main():
    from oracle import oracle as orc
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
    pts = []
    for g, snr in POINTS:
        pts.append(run_point(orc, g, snr, n))
        print(json.dumps(pts[-1]), file=sys.stderr)
    out = {"provenance": "python tests/soft_fer_points.py %d: the ORACLE's demod (SPEC mode, llr_bits 6, llr_csi 0 / 1) "
                         "on the CPU, hard = oracle decode_batch, soft = tests/soft_viterbi_ref.py (NUMERICS.md rule 14); "
                         "delivered = CRC good and PSDU equal to the transmitted one" % n,
           "frames_per_point": n, "points": pts}
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
