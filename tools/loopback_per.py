"""The reference's loop-back (gnu_radio/IRS_tranceiver.py: mac -> TX -> x gain -> channel_model -> RX -> decode_mac) on the device at
config 3's geometry, without a per-frame array crossing PCIe: wifirx_mac_batch (Philox payloads made on the device, 294-byte
PSDUs) -> wifirx_tx_batch (fixed rows of 1472 samples, lead 160) -> wifirx_channel (the 8-tap sets of tests/golden/sv_taps.npy
cycling, CFO uniform in +-20 ppm of 5.89 GHz at 20 MHz, gain sqrt(10^(snr/10)), noise_voltage 1) -> demod (LS) -> decode_mac,
hard and soft -> wifirx_link_stats against the PSDUs sent and the decisions on the clean TX rows.  Per SNR point: FER of both
decoders and the coded BER of the hard decisions, the quantities of tests/golden/config3_ber_table.json (host channel, CPU
oracle), and the raw counters.  --host-stats also downloads the buffers, keeps the books in NumPy and asserts that both agree.
Prints one JSON line, writes it to --out when given.

    python tools/loopback_per.py [--frames 1000000] [--snr 5 10 15 20 25 30] [--host-stats] [--out profiles/loopback_per_config3_device_stats.json]"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gnuradio-wifi-imagetransfer_amd")]

from wifirx import capi, txgen  # noqa: E402

SLOT, LEAD, ENC, PSDU_LEN = 1472, 160, 7, 294
CFO_20PPM = 2 * np.pi * 20e-6 * 5.89e9 / 20e6
POPCOUNT6 = np.array([bin(v).count("1") for v in range(256)], np.uint8)
COUNTERS = [k for k, _ in capi.LinkCounts._fields_]


def host_stats(rx, dev, n, n_sym, nb, p, idx_tx):
    """the bookkeeping on the host: downloads the records, the PSDU rows and the decisions of the batch"""
    fr = dev["frames"].download(capi.FRAME_DTYPE, n)
    got = dev["psdu"].download(np.uint8, n * 304).reshape(n, 304)[:, :PSDU_LEN]
    crc = (fr["flags"] & capi.F_CRC_OK) != 0
    ok = crc & (got == p).all(axis=1)
    good = ((fr["flags"] & capi.F_COMPLETE) != 0) & (fr["encoding"] == ENC) & (fr["psdu_len"] == PSDU_LEN)
    idx = dev["idx"].download(np.uint8, n * n_sym * 48).reshape(n, -1)
    e = POPCOUNT6[idx[good] ^ idx_tx[good]].sum(axis=1, dtype=np.int64)
    per_frame = e / float(n_sym * 48 * nb)
    return dict(frames=n, frames_ref=n, frames_good=int(good.sum()), frames_crc_ok=int(crc.sum()), frames_psdu_ok=int(ok.sum()),
                frames_crc_ok_wrong=int((crc & ~ok).sum()), coded_bits=int(good.sum()) * n_sym * 48 * nb,
                coded_bit_errors=int(e.sum()), coded_bit_errors_sq=int((e * e).sum()),
                coded_ber=float(per_frame.mean()), coded_ber_se=float(per_frame.std() / np.sqrt(max(per_frame.size, 1))),
                fer=float(1.0 - ok.mean()))


def check_host(r, hs, what):
    assert {k: r[k] for k in COUNTERS} == {k: hs[k] for k in COUNTERS}, (what, r, hs)
    for k in ("fer", "coded_ber", "coded_ber_se"):
        assert abs(r[k] - hs[k]) <= 1e-12 * max(abs(hs[k]), 1e-300) + 1e-15, (what, k, r[k], hs[k])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1_000_000)
    ap.add_argument("--snr", type=float, nargs="+", default=[5, 10, 15, 20, 25, 30])
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--host-stats", action="store_true", help="also keep the books in NumPy and assert they agree")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n = a.frames
    n_sym = txgen.n_sym_for(PSDU_LEN, ENC)
    nb = txgen.RATE_TABLE[ENC][0]
    taps = np.load(os.path.join(ROOT, "tests", "golden", "sv_taps.npy")).astype(np.complex64)
    rx = capi.WifiRx(max_sym=n_sym, llr_bits=nb, chan_est=capi.EQ_LS, device=0)
    t_all = time.perf_counter()
    d_psdu = rx.alloc(n * PSDU_LEN)
    rows = rx.alloc(n * SLOT * 8)
    iq = rx.alloc(n * SLOT * 8)
    rx.mac_batch_dev(d_psdu.ptr, PSDU_LEN, n, None, payload_len=PSDU_LEN - 28, payload_seed=a.seed)
    rx.tx_batch_dev(rows.ptr, n * SLOT, d_psdu.ptr, ENC, psdu_len=np.full(n, PSDU_LEN, np.uint32), psdu_stride=PSDU_LEN,
                    lead=LEAD, row_len=SLOT)
    dev = rx.alloc_out(n, psdu_stride=304, want_hbits=True)
    # what was sent: the PSDUs, and the demodulator's records and decisions on the clean rows
    ref = dict(frames=rx.alloc(n * 32).upload(np.zeros(n * 32, np.uint8)), idx=rx.alloc(n * n_sym * 48), hbits=rx.alloc(n * n_sym * 48), psdu=d_psdu,
               psdu_stride=PSDU_LEN)
    rx.demod_batch_dev(rows.ptr, SLOT, n, ref)
    assert rx.link_stats(n, ref, ref)["frames_ref"] == n, "a clean frame was not demodulated"
    if a.host_stats:
        p = d_psdu.download(np.uint8, n * PSDU_LEN).reshape(n, PSDU_LEN)
        idx_tx = ref["idx"].download(np.uint8, n * n_sym * 48).reshape(n, -1)
    points = []
    for snr in a.snr:
        t0 = time.perf_counter()
        cfo = np.random.default_rng(int(1000 * snr) + a.seed).uniform(-CFO_20PPM, CFO_20PPM, n).astype(np.float32)
        rx.channel_dev(rows.ptr, iq.ptr, n * SLOT, n, row_len=SLOT, taps=taps, cfo=cfo, gain=math.sqrt(10 ** (snr / 10)),
                       noise_voltage=1.0, seed=9000 + int(snr) + (a.seed << 32))
        rx.demod_batch_dev(iq.ptr, SLOT, n, dev)
        rx.decode_batch_dev(n, dev)
        hard = rx.link_stats(n, dev, ref)
        if a.host_stats:
            check_host(hard, host_stats(rx, dev, n, n_sym, nb, p, idx_tx), "hard")
        rx.decode_batch_soft_dev(n, dev)
        soft = rx.link_stats(n, dev, ref)
        if a.host_stats:
            check_host(soft, host_stats(rx, dev, n, n_sym, nb, p, idx_tx), "soft")
        points.append({"snr_db": snr, "frames": n, "detected_and_signal_ok": hard["frames_good"] / n,
                       "coded_ber": hard["coded_ber"], "coded_ber_se": hard["coded_ber_se"],
                       "fer": hard["fer"], "fer_soft": soft["fer"], "crc_ok_wrong_psdu": hard["frames_crc_ok_wrong"],
                       "seconds": time.perf_counter() - t0,
                       "counts": {k: hard[k] for k in COUNTERS}, "counts_soft": {k: soft[k] for k in COUNTERS}})
        print(json.dumps(points[-1]), file=sys.stderr)
    seconds_total = time.perf_counter() - t_all
    rx.free_out(ref)
    rx.free_out(dev)
    rows.free(); iq.free(); rx.close()
    res = {"workload": "loop-back on the device, config 3: %d distinct frames per point (wifirx_mac_batch, Philox payloads), 64-QAM 3/4, PSDU 294 B, rows of 1472, "
                       "lead 160, sv_taps.npy sets cycling, CFO uniform in +-20 ppm, LS; hard and soft decode_mac" % n,
           "stats": "wifirx_link_stats on the device" + (", checked against the NumPy bookkeeping" if a.host_stats else ""),
           "seconds_total": seconds_total, "points": points}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
