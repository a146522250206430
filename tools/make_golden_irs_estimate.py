#!/usr/bin/env python3
"""Record the reference's pilot-based channel estimator as a fixture: tests/golden/irs_estimate_reference.npz.

Runs only where the reference tree exists (its path is the one argument); utils/channel.py is imported from it at run time, and
only what it computed is written.  For J = 5 and 17 coefficients (the direct path and J - 1 groups), A = 1 and 4 AP antennas and
four NumPy seeds the file holds, as complex128 / float64:

  Pilot_J{J}               Channel.DFT_matrix(J): [J, J], unitary
  H_J{J}_A{A}              [4, A, J]: the channel rows that are estimated, seeded complex Gaussians of variance 1
  noise_J{J}_A{A}          [4, A, J]: Channel(J, A, J).noise(sqrt(sigma2)) after the same seed
  y_J{J}_A{A}              [4, A, J]: y_rx = H Pilot + noise
  Hest_J{J}_A{A}           [4, A, J]: Channel.CH_est(y_rx, sigma2, Pilot)
  sigma2, seeds            the noise variances per seed [4] and the seeds
"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "..", "tests", "golden", "irs_estimate_reference.npz")
SEEDS = np.arange(301, 305)
SIGMA2 = np.array([0.0, 0.01, 0.25, 1.0])
COEFFS = (5, 17)
ANTENNAS = (1, 4)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("reference", help="root of the reference tree")
    args = ap.parse_args()
    sys.path.insert(0, args.reference)
    from utils.channel import Channel                            # (the module seeds NumPy with 0 at import)

    out = {"seeds": SEEDS, "sigma2": SIGMA2}
    for J in COEFFS:
        for A in ANTENNAS:
            ch = Channel(J, A, J)
            pilot = np.asarray(ch.DFT_matrix(J))
            out["Pilot_J%d" % J] = pilot
            H, W, Y, E = [], [], [], []
            for s, s2 in zip(SEEDS, SIGMA2):
                rng = np.random.default_rng(int(s))
                h = (rng.standard_normal((A, J)) + 1j * rng.standard_normal((A, J))) / np.sqrt(2.0)
                np.random.seed(int(s))
                w = np.asarray(ch.noise(np.sqrt(s2)))
                y = h @ pilot + w
                H.append(h), W.append(w), Y.append(y), E.append(np.asarray(ch.CH_est(y, s2, pilot)))
            tag = "J%d_A%d" % (J, A)
            out["H_" + tag], out["noise_" + tag], out["y_" + tag], out["Hest_" + tag] = map(np.array, (H, W, Y, E))
    out = {k: (np.asarray(v, dtype=np.complex128) if np.iscomplexobj(v) else np.asarray(v)) for k, v in out.items()}
    np.savez_compressed(OUT, **out)
    print("wrote %s: %d arrays, %d bytes" % (OUT, len(out), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
