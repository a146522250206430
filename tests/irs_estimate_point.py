"""The operating point of the end-to-end test of the pilot-trained surface
(tests/test_gpu_irs_estimate.py::test_trained_surface_between_random_and_genie) and the host restatement that chose it.

256 tap sets of one tap behind an 8 x 8 surface (N = 64, every element its own group), one AP antenna, pure scattering
(k_factor = 0: no steering codebook helps here), the direct path blocked, 2-bit phases, the 65-point DFT pilots of
wifirx.irs.dft_pilots and the least-squares scale 1 / T.  For every sigma of GRID the restatement (tests/irs_estimate_ref.py,
NUMERICS.md rule 29) trains the surface from its noisy estimate, and the channel power sum_r |t_r|^2 under the decided codes is
set against the genie's (rule 27's align_bits on the true elements) and against one random 2-bit configuration.  With the
direct path blocked both align to the positive real axis, so at sigma = 0 the codes and the power are the genie's.  The chosen sigma
is the grid value whose ratio to the genie is nearest 0.8; profiles/irs_estimate_operating_point.json holds every step.

The ratio R = sum P_est / sum P_genie is a ratio of means over the 256 sets; its standard error is that of the mean of
P_est - R P_genie divided by the mean of P_genie (the first-order error of a ratio).  The device draws the same counters through
its own logf / sincosf (rule 25's 1e-5), so its ratio is held to R +- 5 standard errors, not to R's digits.

    python tests/irs_estimate_point.py [--out profiles/irs_estimate_operating_point.json]"""
import json
import math
import os
import sys

import numpy as np

N_SETS, SCALE, BITS = 256, 8, 2
N_ELEMS = SCALE * SCALE
IRS_SEED, PSI_SEED = 61, 7
SIGMA = 3.5
TARGET = 0.8
GRID = (0.0, 1.0, 2.0, 3.0, 3.5, 4.0, 4.5, 5.0, 6.0)
PDP = (1.0,)


def scene():
    """the arguments both sides share: (pdp, los_b2r [1, N], los_r2u [N]) -- not looked at with k_factor = 0 -- and the keywords"""
    one = np.ones(N_ELEMS, np.complex64)
    return (PDP, one[None], one), dict(k_factor=0.0, direct_gain=0.0, seed=IRS_SEED)


def pilots():
    from wifirx import irs
    pl = irs.dft_pilots(N_ELEMS)
    return pl, irs.est_scale(pl.shape[0])


def power(taps):
    """the channel power of every set: taps [M, n_sets, L] -> float64 [n_sets]"""
    t = np.asarray(taps, dtype=np.complex128)
    return (np.abs(t) ** 2).sum(axis=(0, 2))


def ratio(p, p_genie):
    """(R, its standard error) of the ratio of means"""
    r = float(p.sum() / p_genie.sum())
    se = float(np.std(p - r * p_genie, ddof=1) / math.sqrt(p.size) / p_genie.mean())
    return r, se


def host_point(sigma):
    import irs_estimate_ref as er
    import irs_multi_ref as mr
    from wifirx import irs
    (pdp, a, b), kw = scene()
    pl, kappa = pilots()
    est = er.irs_estimate(N_SETS, pdp, a, b, None, pilots=pl, sigma=sigma, est_scale=kappa, align_bits=BITS, **kw)
    genie = mr.irs_taps_multi(N_SETS, pdp, a, b, None, align_bits=BITS, **kw)
    rand = mr.irs_taps_multi(N_SETS, pdp, a, b, None, psi=irs.random_psi(N_ELEMS, BITS, PSI_SEED), **kw)
    p_est, p_gen, p_rnd = power(est["taps"]), power(genie["taps"]), power(rand["taps"])
    r, se = ratio(p_est, p_gen)
    return {"sigma": sigma, "ratio": r, "ratio_se": se, "random_ratio": ratio(p_rnd, p_gen)[0],
            "codes_differing": int((est["codes"] != genie["codes"]).sum()), "mean_power_genie": float(p_gen.mean())}


def main(argv):
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [here, os.path.join(here, ".."), os.path.join(here, "..", "gnuradio-wifi-imagetransfer_amd")]
    out = argv[argv.index("--out") + 1] if "--out" in argv else None
    points = [host_point(s) for s in GRID]
    for p in points:
        print("sigma %4.1f: ratio to the genie %.4f +- %.4f, random %.4f, %d of %d codes differ"
              % (p["sigma"], p["ratio"], p["ratio_se"], p["random_ratio"], p["codes_differing"], N_SETS * N_ELEMS))
    chosen = min((p for p in points if p["sigma"] > 0), key=lambda p: abs(p["ratio"] - TARGET))
    rec = {"what": "tests/irs_estimate_point.py: the restatement's channel power under codes decided from a noisy estimate, as a "
                   "fraction of the genie's; N = %d, B = %d, k_factor = 0, direct path blocked, %d sets, DFT pilots, kappa = 1 / T"
                   % (N_ELEMS, BITS, N_SETS),
           "target": TARGET, "chosen_sigma": chosen["sigma"], "chosen": chosen, "points": points}
    assert chosen["sigma"] == SIGMA, "SIGMA in this file is not the grid value nearest the target: %r" % chosen
    if out:
        with open(out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
