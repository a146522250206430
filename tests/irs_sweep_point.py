"""The operating point of the end-to-end beam-training test (tests/test_gpu_irs_sweep.py::test_training_closes_a_link_a_random_
configuration_cannot) and the host chain that chose it: txgen -> irs_sweep_ref.irs_sweep / irs_ref.irs_taps ->
channel_ref.channel -> the oracle's demod and decode_mac.

256 QPSK-1/2 frames of 100 bytes, one tap (pdp = {1}), an 8 x 8 surface (N = 64) in the geometry of tools/loopback_per.py --irs,
Rician scatter with k_factor = 3, the direct path blocked, noise_voltage 1 and a transmit gain of sqrt(snr): `snr` is the SNR of
ONE unit-power path.  Two arms with 2-bit phases: `random`, one fixed random configuration, and `sweep`, the winner of
irs.dft_codebook(8, los_b2r, over=2, bits=2) (256 entries) per draw (NUMERICS.md rule 26).  The point is accepted only if
the host chain gives at most 64 of 256 frames for the random arm and at least 250 for the sweep arm; the prediction was about
-22 dB (random near +2 dB in the mean, sweep near +10 dB), and the SNR is stepped by 1 dB from there until both hold
(profiles/irs_sweep_operating_point.json holds the point and the counts of every step looked at).

    python tests/irs_sweep_point.py [--snr -22] [--out profiles/irs_sweep_operating_point.json]"""
import math
import os
import sys

import numpy as np

from irs_point import ENC, LEAD, N_FRAMES, PLEN, TAIL, geometry     # the same frames in the same slots

SNR_DB = -22.0
SCALE, BITS, OVER, K_FACTOR = 8, 2, 2, 3.0
N_ELEMS = SCALE * SCALE
PSDU_SEED, NOISE_SEED, IRS_SEED, PSI_SEED = 31, 9300, 41, 43
ARMS = ("random", "sweep")
RANDOM_AT_MOST, SWEEP_AT_LEAST = 64, 250


def scene():
    """(los_b2r, los_r2u) of the surface in front of the AP, as tools/loopback_per.py --irs places it"""
    from wifirx import irs
    S = SCALE
    b2r, r2u, _ = irs.los(S, [0.015, 0.015, 0], [S * 0.015, S * 0.015, 4.5], [S * 0.015 + 0.3, S * 0.015 - 0.2, 1.0])
    return b2r.astype(np.complex64), r2u.astype(np.complex64)


def surface(arm):
    """keywords of irs_taps (random) / irs_sweep (sweep), restatement and device alike"""
    from wifirx import irs
    kw = dict(k_factor=K_FACTOR, direct_gain=0.0, seed=IRS_SEED)
    if arm == "sweep":
        kw["codebook"] = irs.dft_codebook(SCALE, scene()[0], over=OVER, bits=BITS)
    else:
        kw["psi"] = irs.random_psi(N_ELEMS, BITS, PSI_SEED)
    return kw


def host_taps(arm, n=N_FRAMES):
    import irs_ref
    import irs_sweep_ref
    b2r, r2u = scene()
    if arm == "sweep":
        return irs_sweep_ref.irs_sweep(n, [1.0], b2r, r2u, None, **surface(arm))
    return irs_ref.irs_taps(n, [1.0], b2r, r2u, None, **surface(arm))


def host_chain(snr_db=SNR_DB, n=N_FRAMES, taps=None):
    """FCS-good frames (of n) of the two arms on the host"""
    import channel_ref
    from oracle import oracle as orc
    from wifirx import txgen
    n_sym, slot = geometry()
    psdus = txgen.make_psdus(n, PLEN, seed=PSDU_SEED)
    tx = txgen.encode_psdus(psdus, ENC)
    rows = np.zeros((n, slot), np.complex64)
    rows[:, LEAD:LEAD + tx.samples.shape[1]] = tx.samples
    prm = orc.make_params(max_sym=n_sym, llr_bits=0)
    res = {"frames": n, "snr_db": snr_db, "n_elems": N_ELEMS, "bits": BITS, "k_factor": K_FACTOR, "codebook": "dft_codebook(8, los_b2r, over=2, bits=2)"}
    for arm in ARMS:
        t = (taps or {}).get(arm)
        if t is None:
            t = host_taps(arm, n)
        y = channel_ref.channel(rows, taps=t["taps"], gain=math.sqrt(10 ** (snr_db / 10)), noise_voltage=1.0, seed=NOISE_SEED)
        o = orc.demod_batch(y, slot, prm, n_threads=8)
        fr = o["frames"].copy()
        got = orc.decode_batch(fr, o["idx"], prm, psdu_stride=112, n_threads=8)
        ok = ((fr["flags"] & 0x40) != 0) & (fr["psdu_len"] == PLEN) & (got[:, :PLEN] == psdus).all(axis=1)
        res[arm] = int(ok.sum())
        res[arm + "_detected"] = int(((fr["flags"] & 1) != 0).sum())
        res[arm + "_mean_tap_power"] = float((np.abs(t["taps"].astype(np.complex128)) ** 2).mean())
        if arm == "sweep":
            res["sweep_distinct_winners"] = int(np.unique(t["best"]).size)
    res["accepted"] = bool(res["random"] <= RANDOM_AT_MOST and res["sweep"] >= SWEEP_AT_LEAST)
    return res


if __name__ == "__main__":
    import argparse
    import json
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [ROOT, os.path.join(ROOT, "gnuradio-wifi-imagetransfer_amd")]
    ap = argparse.ArgumentParser()
    ap.add_argument("--snr", type=float, nargs="+", default=[SNR_DB])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    taps = {arm: host_taps(arm) for arm in ARMS}                # the taps do not depend on the SNR
    rec = {"what": "host chain of tests/irs_sweep_point.py: FCS-good frames of %d QPSK-1/2 frames of %d bytes at an SNR per unit-power "
                   "path over %d elements, k_factor %g, direct path blocked: one fixed random %d-bit configuration / the winner of a "
                   "256-entry 2-bit DFT codebook per draw (NUMERICS.md rule 26)" % (N_FRAMES, PLEN, N_ELEMS, K_FACTOR, BITS),
           "accept": "random <= %d and sweep >= %d of %d" % (RANDOM_AT_MOST, SWEEP_AT_LEAST, N_FRAMES),
           "chosen_snr_db": SNR_DB, "prediction": "about -22 dB: random near +2 dB in the mean, sweep near +10 dB (a sketch, not a measurement)",
           "points": [host_chain(s, taps=taps) for s in a.snr]}
    print(json.dumps(rec))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")
