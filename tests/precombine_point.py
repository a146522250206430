"""The two operating points of the end-to-end pre-detection combining tests (tests/test_gpu_precombine.py::test_gain_at_two_antennas
and ::test_gain_at_four_antennas) and the host chain that settles them: txgen -> fading_ref.channel -> precombine_ref (NUMERICS.md
rule 33, the rule's own arithmetic) -> oracle demod -> the oracle's decode_mac, next to diversity_ref (rule 23) on the A single-
antenna demods.

The scene is that of tests/diversity_point.py -- 2048 QPSK-1/2 frames of 100 bytes, flat Rayleigh with doppler = 0 (one static
complex gain per row and antenna), its PSDU seed and its seeds for antennas 0 and 1 -- with two more antennas for A = 4 and the
slot lengthened to the next multiple of 64 samples, which rule 33 asks for.

    python tests/precombine_point.py [--frames 2048] [--out profiles/precombine_operating_point.json]"""
import math
import os
import sys

import numpy as np

import diversity_point as dp

N, ENC, PLEN, LEAD = dp.N, dp.ENC, dp.PLEN, dp.LEAD
PSDU_SEED = dp.PSDU_SEED
SEEDS = dp.SEEDS + ((9300, 13), (9400, 14))     # (noise seed, fade_seed) of antenna 0 .. 3
ITERS = 2
# the assertion each point carries, and the margin the host chain has to leave on it (a factor of two)
POINTS = {"a2": dict(n_ant=2, snr_db=12.0),     # pre-detection combining loses at most half of the better single antenna's frames
          "a4": dict(n_ant=4, snr_db=8.0)}      # pre-detection combining loses no more frames than rule 23's MRC


def geometry():
    n_sym, slot = dp.geometry()
    return n_sym, (slot + 63) // 64 * 64


def host_chain(n_ant, snr_db, n=N, iters=ITERS):
    """lost frames (of n), hard decisions: each antenna alone, rule 23's MRC over the A demods, rule 33 and one demod"""
    import diversity_ref as dr
    import fading_ref
    import precombine_ref as pr
    from oracle import oracle as orc
    from wifirx import txgen
    n_sym, slot = geometry()
    psdus = txgen.make_psdus(n, PLEN, seed=PSDU_SEED)
    tx = txgen.encode_psdus(psdus, ENC)
    rows = np.zeros((n, slot), np.complex64)
    rows[:, LEAD:LEAD + tx.samples.shape[1]] = tx.samples
    prm = orc.make_params(max_sym=n_sym, llr_bits=2)
    xs = [fading_ref.channel(rows, taps=(1.0,), gain=math.sqrt(10 ** (snr_db / 10)), noise_voltage=1.0, seed=seed, doppler=0.0,
                             fade_seed=fade_seed) for seed, fade_seed in SEEDS[:n_ant]]
    ant = [orc.demod_batch(x, slot, prm, want_eq=True, want_csi=True, n_threads=8) for x in xs]

    def lost(frames, idx):
        fr = frames.copy()
        got = orc.decode_batch(fr, idx, prm, psdu_stride=112, n_threads=8)
        ok = ((fr["flags"] & 0x40) != 0) & (fr["psdu_len"] == PLEN) & (got[:, :PLEN] == psdus).all(axis=1)
        return int(n - ok.sum()), int((((fr["flags"] & 0x40) != 0) & ~ok).sum())

    res = {"frames": n, "n_ant": n_ant, "snr_db": snr_db, "iters": iters, "slot_len": slot, "single": [], "crc_ok_wrong": 0}
    for o in ant:
        l, w = lost(o["frames"], o["idx"])
        res["single"].append(l)
        res["crc_ok_wrong"] += w
    out = dr.new_outputs(n, n_sym, 2, fill=0)
    dr.combine([o["frames"] for o in ant], [o["eq"] for o in ant], [o["csi"] for o in ant], n_sym, 2, out, mode=dr.MRC)
    res["mrc"], w = lost(out["frames"], out["idx"])
    res["crc_ok_wrong"] += w
    y, _, st = pr.combine(xs, slot, iters)
    o = orc.demod_batch(y, slot, prm, want_eq=True, n_threads=8)
    res["precombine"], w = lost(o["frames"], o["idx"])
    res["crc_ok_wrong"] += w
    res["degenerate_slots"] = int((st["flags"] != 0).sum())
    return res


if __name__ == "__main__":
    import argparse
    import json
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [ROOT, os.path.join(ROOT, "gnuradio-wifi-imagetransfer_amd")]
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=N)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pts = {k: host_chain(p["n_ant"], p["snr_db"], a.frames) for k, p in POINTS.items()}
    rec = {"what": "host chain of tests/precombine_point.py: lost frames of %d QPSK-1/2 frames of %d bytes, flat Rayleigh, doppler 0, hard "
                   "decode_mac: each antenna alone, rule 23's MRC over the A demods, pre-detection combining (NUMERICS.md rule 33, "
                   "tests/precombine_ref.py, %d power iterations) and one demod" % (a.frames, PLEN, ITERS),
           "assertions": {"a2": "2 * precombine <= min(single); margin wanted: 4 * precombine <= min(single)",
                          "a4": "precombine <= mrc; margin wanted: 2 * precombine <= mrc"},
           "points": pts}
    print(json.dumps(rec))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")
