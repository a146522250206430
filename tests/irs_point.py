"""The operating point of the end-to-end surface test (tests/test_gpu_irs.py::test_surface_closes_a_link_the_direct_path_cannot)
and the host chain that chose it: txgen -> irs_ref.irs_taps -> channel_ref.channel -> the oracle's demod and decode_mac.

256 QPSK-1/2 frames of 100 bytes, one tap (pdp = {1}), Rayleigh scatter (k_factor = 0), noise_voltage 1 and a transmit
gain of sqrt(snr): `snr` is the SNR of ONE unit-power path, which is what the direct path alone ("N = 0": one flat tap of 1)
and every element path a_n, b_n have.  The point has to lie where the direct path alone decodes no frame.  With the direct
path blocked, N = 64 elements aligned to 2 bits per draw lift the link by about (N pi/4 sinc(pi/4))^2 = 2048 (33 dB) and
keep every frame; random phases lift it by N = 64 (18 dB) in the mean but leave it Rayleigh, so frames in the fades are lost.
Detection needs S / (S + N) above 0.56 (about +1 dB) and QPSK 1/2 about 5 dB, which suggested -6 dB: nothing is found at
-6 dB, the genie arm runs near 27 dB and the random arm near 12 dB in the mean.  The host chain settles it
(profiles/irs_operating_point.json holds the point and the counts).

    python tests/irs_point.py [--snr -6] [--out profiles/irs_operating_point.json]"""
import math
import os
import sys

import numpy as np

N_FRAMES, ENC, PLEN, LEAD, TAIL = 256, 2, 100, 160, 79
SNR_DB = -6.0
N_ELEMS, BITS = 64, 2
PSDU_SEED, NOISE_SEED, IRS_SEED, PSI_SEED = 31, 9300, 41, 43
ARMS = ("direct", "genie", "random")


def geometry():
    from wifirx import txgen
    slot = LEAD + txgen.frame_samples(PLEN, ENC) + TAIL
    return txgen.n_sym_for(PLEN, ENC), slot + (slot & 1)


def surface(arm):
    """keywords of irs_taps (restatement and device alike) for the two arms with a surface"""
    from wifirx import irs
    kw = dict(k_factor=0.0, direct_gain=0.0, seed=IRS_SEED)
    if arm == "genie":
        kw["align_bits"] = BITS
    else:
        kw["psi"] = irs.random_psi(N_ELEMS, BITS, PSI_SEED)
    return kw


def host_chain(snr_db=SNR_DB, n=N_FRAMES):
    """FCS-good frames (of n) of the three arms on the host"""
    import channel_ref
    import irs_ref
    from oracle import oracle as orc
    from wifirx import txgen
    n_sym, slot = geometry()
    psdus = txgen.make_psdus(n, PLEN, seed=PSDU_SEED)
    tx = txgen.encode_psdus(psdus, ENC)
    rows = np.zeros((n, slot), np.complex64)
    rows[:, LEAD:LEAD + tx.samples.shape[1]] = tx.samples
    prm = orc.make_params(max_sym=n_sym, llr_bits=0)
    one = np.ones(N_ELEMS, np.complex64)
    res = {"frames": n, "snr_db": snr_db, "n_elems": N_ELEMS, "bits": BITS}
    for arm in ARMS:
        taps = np.ones((1, 1), np.complex64) if arm == "direct" else irs_ref.irs_taps(n, [1.0], one, one, None, **surface(arm))["taps"]
        y = channel_ref.channel(rows, taps=taps, gain=math.sqrt(10 ** (snr_db / 10)), noise_voltage=1.0, seed=NOISE_SEED)
        o = orc.demod_batch(y, slot, prm, n_threads=8)
        fr = o["frames"].copy()
        got = orc.decode_batch(fr, o["idx"], prm, psdu_stride=112, n_threads=8)
        ok = ((fr["flags"] & 0x40) != 0) & (fr["psdu_len"] == PLEN) & (got[:, :PLEN] == psdus).all(axis=1)
        res[arm] = int(ok.sum())
        res[arm + "_detected"] = int(((fr["flags"] & 1) != 0).sum())
        res[arm + "_mean_tap_power"] = float((np.abs(taps.astype(np.complex128)) ** 2).mean())
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
    rec = {"what": "host chain of tests/irs_point.py: FCS-good frames of %d QPSK-1/2 frames of %d bytes at an SNR per unit-power path: "
                   "the direct path alone, and with it blocked %d elements aligned to %d bits per draw / with random %d-bit phases "
                   "(NUMERICS.md rule 25)" % (N_FRAMES, PLEN, N_ELEMS, BITS, BITS),
           "chosen_snr_db": SNR_DB, "prediction": "detection needs about +1 dB and QPSK 1/2 about 5 dB, the aligned surface adds 33 dB, "
                                                  "the random one 18 dB in the mean: -6 dB (not a measurement)",
           "points": [host_chain(s) for s in a.snr]}
    print(json.dumps(rec))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")
