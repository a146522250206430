"""The operating point of the end-to-end diversity test (tests/test_gpu_diversity.py::test_diversity_gain) and the host chain
that chose it: txgen -> fading_ref.channel -> oracle demod -> diversity_ref -> the oracle's decode_mac.

2048 QPSK-1/2 frames of 100 bytes through a flat Rayleigh channel with doppler = 0 -- one static complex gain per row and
antenna (NUMERICS.md rule 19) --, A = 2 antennas that differ in fade_seed and noise seed, one mean SNR.  The single-antenna FER
has to lie between 0.1 and 0.5 there.  Rayleigh outage with a threshold near 6.5 dB suggested about 12 dB; the host chain
settles it (profiles/diversity_operating_point.json holds the point and the counts).

    python tests/diversity_point.py [--frames 2048] [--snr 12] [--out profiles/diversity_operating_point.json]"""
import math
import os
import sys

import numpy as np

N, ENC, PLEN, LEAD, TAIL = 2048, 2, 100, 160, 79
SNR_DB = 12.0
N_ANT = 2
PSDU_SEED = 23
SEEDS = ((9100, 11), (9200, 12))       # (noise seed, fade_seed) of antenna 0, 1


def geometry():
    from wifirx import txgen
    n_sym = txgen.n_sym_for(PLEN, ENC)
    slot = LEAD + txgen.frame_samples(PLEN, ENC) + TAIL
    return n_sym, slot + (slot & 1)


def host_chain(n=N, snr_db=SNR_DB):
    """the counts of the host chain: lost frames (of n) of each antenna alone, of SELECT and of MRC, hard decisions"""
    import diversity_ref as dr
    import fading_ref
    from oracle import oracle as orc
    from wifirx import txgen
    n_sym, slot = geometry()
    psdus = txgen.make_psdus(n, PLEN, seed=PSDU_SEED)
    tx = txgen.encode_psdus(psdus, ENC)
    rows = np.zeros((n, slot), np.complex64)
    rows[:, LEAD:LEAD + tx.samples.shape[1]] = tx.samples
    prm = orc.make_params(max_sym=n_sym, llr_bits=2)
    ant = []
    for seed, fade_seed in SEEDS[:N_ANT]:
        y = fading_ref.channel(rows, taps=(1.0,), gain=math.sqrt(10 ** (snr_db / 10)), noise_voltage=1.0, seed=seed, doppler=0.0,
                               fade_seed=fade_seed)
        ant.append(orc.demod_batch(y, slot, prm, want_eq=True, want_csi=True, n_threads=8))

    def lost(frames, idx):
        fr = frames.copy()
        got = orc.decode_batch(fr, idx, prm, psdu_stride=112, n_threads=8)
        ok = ((fr["flags"] & 0x40) != 0) & (fr["psdu_len"] == PLEN) & (got[:, :PLEN] == psdus).all(axis=1)
        wrong = int((((fr["flags"] & 0x40) != 0) & ~ok).sum())
        return int(n - ok.sum()), wrong

    res = {"frames": n, "snr_db": snr_db, "single": [], "crc_ok_wrong": 0}
    for o in ant:
        l, w = lost(o["frames"], o["idx"])
        res["single"].append(l)
        res["crc_ok_wrong"] += w
    for name, mode in (("select", dr.SELECT), ("mrc", dr.MRC)):
        out = dr.new_outputs(n, n_sym, 2, fill=0)
        dr.combine([o["frames"] for o in ant], [o["eq"] for o in ant], [o["csi"] for o in ant], n_sym, 2, out, mode=mode)
        l, w = lost(out["frames"], out["idx"])
        res[name] = l
        res["crc_ok_wrong"] += w
    res["fer_single"] = [l / n for l in res["single"]]
    return res


if __name__ == "__main__":
    import argparse
    import json
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [ROOT, os.path.join(ROOT, "gnuradio-wifi-imagetransfer_amd")]
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=N)
    ap.add_argument("--snr", type=float, nargs="+", default=[SNR_DB])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pts = [host_chain(a.frames, s) for s in a.snr]
    rec = {"what": "host chain of tests/diversity_point.py: lost frames of %d QPSK-1/2 frames of %d bytes, flat Rayleigh, doppler 0, "
                   "hard decode_mac: each antenna alone, selection, maximal-ratio combining (NUMERICS.md rule 23)" % (a.frames, PLEN),
           "chosen_snr_db": SNR_DB, "prediction": "Rayleigh outage with a threshold near 6.5 dB suggested about 12 dB (not a measurement)",
           "points": pts}
    print(json.dumps(rec))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")
