"""The reference's loop-back (gnu_radio/IRS_tranceiver.py: TX -> x gain -> channel_model -> RX) on the device at config 3's
geometry: distinct PSDUs -> wifirx_tx_batch (fixed rows of 1472 samples, lead 160) -> wifirx_channel (the 8-tap sets of
tests/golden/sv_taps.npy cycling, CFO uniform in +-20 ppm of 5.89 GHz at 20 MHz, gain sqrt(10^(snr/10)), noise_voltage 1)
-> demod (LS) -> decode_mac, hard and soft.  Per SNR point: FER of both decoders and the coded BER of the hard decisions
(against the decisions on the clean TX rows), the quantities of tests/golden/config3_ber_table.json (host channel, CPU oracle).
Prints one JSON line, writes it to --out when given.

    python tools/loopback_per.py [--frames 1000000] [--snr 5 10 15 20 25 30] [--out profiles/loopback_per_config3.json]"""
import argparse
import json
import math
import os
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gnuradio-wifi-imagetransfer_amd")]

from wifirx import capi, txgen  # noqa: E402

SLOT, LEAD, ENC, PSDU_LEN = 1472, 160, 7, 294
CFO_20PPM = 2 * np.pi * 20e-6 * 5.89e9 / 20e6
POPCOUNT6 = np.array([bin(v).count("1") for v in range(256)], np.uint8)


def psdus(n, seed):
    """n distinct PSDUs: the MAC header of txgen.mac_frame with the frame number as sequence, random payload, FCS"""
    rng = np.random.Generator(np.random.PCG64(seed))
    out = np.empty((n, PSDU_LEN), dtype=np.uint8)
    out[:, :24] = np.frombuffer(txgen.mac_frame(b"", seq=0)[:24], dtype=np.uint8)
    seq = (np.arange(n) & 0xFFF) << 4
    out[:, 22] = seq & 0xFF
    out[:, 23] = seq >> 8
    out[:, 24:PSDU_LEN - 4] = rng.integers(0, 256, size=(n, PSDU_LEN - 28), dtype=np.uint8)
    crc = np.fromiter((zlib.crc32(row) for row in out[:, :PSDU_LEN - 4]), dtype=np.uint32, count=n)
    out[:, PSDU_LEN - 4:] = crc.view(np.uint8).reshape(n, 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1_000_000)
    ap.add_argument("--snr", type=float, nargs="+", default=[5, 10, 15, 20, 25, 30])
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n = a.frames
    n_sym = txgen.n_sym_for(PSDU_LEN, ENC)
    nb = txgen.RATE_TABLE[ENC][0]
    taps = np.load(os.path.join(ROOT, "tests", "golden", "sv_taps.npy")).astype(np.complex64)
    rx = capi.WifiRx(max_sym=n_sym, llr_bits=nb, chan_est=capi.EQ_LS, device=0)
    p = psdus(n, a.seed)
    d_psdu = rx.alloc(p.nbytes).upload(p)
    rows = rx.alloc(n * SLOT * 8)
    iq = rx.alloc(n * SLOT * 8)
    rx.tx_batch_dev(rows.ptr, n * SLOT, d_psdu.ptr, ENC, psdu_len=np.full(n, PSDU_LEN, np.uint32), psdu_stride=PSDU_LEN,
                    lead=LEAD, row_len=SLOT)
    d_psdu.free()
    dev = rx.alloc_out(n, psdu_stride=304, want_hbits=True)
    # the transmitted decisions: the demodulator on the clean rows
    rx.demod_batch_dev(rows.ptr, SLOT, n, dev)
    rx.sync()
    fr0 = dev["frames"].download(capi.FRAME_DTYPE, n)
    assert ((fr0["flags"] & capi.F_COMPLETE) != 0).all(), "a clean frame was not demodulated"
    idx_tx = dev["idx"].download(np.uint8, n * n_sym * 48).reshape(n, -1)
    points = []
    for snr in a.snr:
        t0 = time.perf_counter()
        cfo = np.random.default_rng(int(1000 * snr) + a.seed).uniform(-CFO_20PPM, CFO_20PPM, n).astype(np.float32)
        rx.channel_dev(rows.ptr, iq.ptr, n * SLOT, n, row_len=SLOT, taps=taps, cfo=cfo, gain=math.sqrt(10 ** (snr / 10)),
                       noise_voltage=1.0, seed=9000 + int(snr) + (a.seed << 32))
        rx.demod_batch_dev(iq.ptr, SLOT, n, dev)
        rx.decode_batch_dev(n, dev)
        rx.sync()
        fr = dev["frames"].download(capi.FRAME_DTYPE, n)
        got = dev["psdu"].download(np.uint8, n * 304).reshape(n, 304)[:, :PSDU_LEN]
        ok_hard = ((fr["flags"] & capi.F_CRC_OK) != 0) & (got == p).all(axis=1)
        good = ((fr["flags"] & capi.F_COMPLETE) != 0) & (fr["encoding"] == ENC) & (fr["psdu_len"] == PSDU_LEN)
        idx = dev["idx"].download(np.uint8, n * n_sym * 48).reshape(n, -1)
        per_frame = POPCOUNT6[idx[good] ^ idx_tx[good]].sum(axis=1, dtype=np.int64) / float(n_sym * 48 * nb)
        rx.decode_batch_soft_dev(n, dev)
        rx.sync()
        fr_s = dev["frames"].download(capi.FRAME_DTYPE, n)
        got = dev["psdu"].download(np.uint8, n * 304).reshape(n, 304)[:, :PSDU_LEN]
        ok_soft = ((fr_s["flags"] & capi.F_CRC_OK) != 0) & (got == p).all(axis=1)
        points.append({"snr_db": snr, "frames": n, "detected_and_signal_ok": float(good.mean()),
                       "coded_ber": float(per_frame.mean()), "coded_ber_se": float(per_frame.std() / np.sqrt(max(per_frame.size, 1))),
                       "fer": float(1.0 - ok_hard.mean()), "fer_soft": float(1.0 - ok_soft.mean()),
                       "crc_ok_wrong_psdu": int((((fr["flags"] & capi.F_CRC_OK) != 0) & ~ok_hard).sum()),
                       "seconds": time.perf_counter() - t0})
        print(json.dumps(points[-1]), file=sys.stderr)
    rx.free_out(dev)
    rows.free(); iq.free(); rx.close()
    res = {"workload": "loop-back on the device, config 3: %d distinct frames per point, 64-QAM 3/4, PSDU 294 B, rows of 1472, "
                       "lead 160, sv_taps.npy sets cycling, CFO uniform in +-20 ppm, LS; hard and soft decode_mac" % n,
           "points": points}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
