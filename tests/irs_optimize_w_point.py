"""What the weights of the joint decision (NUMERICS.md rule 31, tests/irs_optimize_w_ref.py) do to the channel, measured on the host
with the project's own float32 arithmetic, after tests/irs_optimize_point.py.

Scenes: an 8 x 8 surface (N = 64, every element its own group), 2-bit phases, pure scattering (k_factor = 0), the direct path
blocked, SETS tap sets each: M1_L8 (one antenna, 8 taps of an exponential power delay profile), M4_L8 and M4_L1.  The
coefficients come from tests/irs_estimate_ref.py (rule 29: the 65-point DFT pilots, kappa = 1 / T) at sigma = 0 and at
tests/irs_estimate_point.py's operating sigma.  Arms: rule 29's decision on row 0 ("ref"), w = 1 (rule 30), and per antenna
w = (1, 0, ..), (1, -0.5, ..), (1, -1, ..); for M4_L1 also the antenna weights (1, 1, 0.25, 0.25).  Every ascent starts from rule
29's codes and runs at most SWEEPS sweeps.  Per arm, under the TRUE coefficients (irs_estimate_ref.truth) in float64: the collected
power sum_rho |s_rho|^2 and the power of tap 0 over the antennas, both as means over the sets, and the flatness figure of DESIGN.md
9n -- per set the weakest over the mean of the MRC-combined spectrum sum_m |H_m[k]|^2 on the 52 occupied subcarriers of the 64-point
transform of the taps, the median over the sets.  profiles/irs_optimize_w_operating_point.json holds the values; they are
recorded, not gated.

    python tests/irs_optimize_w_point.py [--out profiles/irs_optimize_w_operating_point.json]"""
import json
import os
import sys

import numpy as np

SETS, SCALE, BITS, SWEEPS = 32, 8, 2, 4
N_ELEMS = SCALE * SCALE
IRS_SEED = 61
SCENES = {"M1_L8": (1, 8), "M4_L8": (4, 8), "M4_L1": (4, 1)}                  # (M, L)
TAP_ARMS = {"w_1": None, "w_1_0": 0.0, "w_1_-0.5": 0.5, "w_1_-1": 1.0}         # the penalty of irs.tap_weights; None: every weight 1
ANT_ARM = ("ant_1_1_0.25_0.25", (1, 1, 0.25, 0.25))


def sigmas():
    import irs_estimate_point as ep
    return (0.0, ep.SIGMA)


def arms(name):
    """{arm: float32 [M L]} of a scene, in the order they are reported"""
    from wifirx import irs
    M, L = SCENES[name]
    out = {k: irs.row_weights(M, L, tap=None if p is None else irs.tap_weights(L, penalty=p)) for k, p in TAP_ARMS.items()}
    if name == "M4_L1":
        out[ANT_ARM[0]] = irs.row_weights(M, L, ant=ANT_ARM[1])
    return out


def channel(truth, codes, M, L):
    """the taps of the TRUE coefficients under the codes, float64: truth [sets, M L, J], codes [sets, G] -> [M, sets, L]"""
    from wifirx import irs
    ph = irs.PHASES.astype(np.complex128)[codes.astype(np.intp) << (3 - BITS)]
    s = (np.asarray(truth, np.complex128)[:, :, 1:] * ph[:, None, :]).sum(axis=-1)          # the direct path is blocked
    return s.reshape(-1, M, L).transpose(1, 0, 2)


def figures(taps):
    """collected power, tap-0 power (means over the sets) and the flatness figure of taps [M, sets, L]"""
    p = np.abs(taps) ** 2
    spec = (np.abs(np.fft.fft(taps, 64, axis=2)) ** 2).sum(axis=0)
    used = spec[:, np.r_[1:27, 38:64]]
    return {"collected_power": float(p.sum(axis=(0, 2)).mean()), "tap0_power": float(p[:, :, 0].sum(axis=0).mean()),
            "median_weakest_subcarrier_over_mean": float(np.median(used.min(axis=1) / used.mean(axis=1)))}


def point(name, sigma):
    """one scene at one sigma: the estimate, the truth, rule 29's codes, and per arm the weights and the restatement's result"""
    import irs_estimate_ref as er
    import irs_optimize_w_ref as wrf
    from wifirx import irs
    M, L = SCENES[name]
    pdp = np.exp(-np.arange(L) / 2.0)
    pdp = (pdp / pdp.sum()).astype(np.float32)
    a, b = np.ones((M, N_ELEMS), np.complex64), np.ones(N_ELEMS, np.complex64)       # not looked at with k_factor = 0
    pl = irs.dft_pilots(N_ELEMS)
    out = er.irs_estimate(SETS, pdp, a, b, None, pilots=pl, sigma=sigma, est_scale=irs.est_scale(pl.shape[0]), align_bits=BITS,
                          k_factor=0.0, direct_gain=0.0, seed=IRS_SEED)
    truth = er.truth(out, pdp, 1.0, np.arange(N_ELEMS), N_ELEMS, M)[0]
    w = arms(name)
    res = {k: wrf.optimize(out["est"], BITS, SWEEPS, blocked=True, weights=None if k == "w_1" else v) for k, v in w.items()}
    return {"scene": name, "sigma": sigma, "est": out["est"], "truth": truth, "ref_codes": out["codes"], "weights": w, "res": res}


def record(pt):
    M, L = SCENES[pt["scene"]]
    ref = figures(channel(pt["truth"], pt["ref_codes"], M, L))
    rec = {"scene": pt["scene"], "sigma": pt["sigma"], "sets": SETS, "arms": {"ref": ref}}
    for k, res in pt["res"].items():
        f = figures(channel(pt["truth"], res["codes"], M, L))
        f |= {"row_weights": pt["weights"][k].tolist(), "collected_power_over_ref": f["collected_power"] / ref["collected_power"],
              "tap0_power_over_ref": f["tap0_power"] / ref["tap0_power"],
              "codes_changed_fraction": float((res["codes"] != pt["ref_codes"]).mean()), "sweeps_mean": float(res["sweeps"].mean())}
        rec["arms"][k] = f
    return rec


def records():
    return [record(point(name, s)) for name in SCENES for s in sigmas()]


def document(recs):
    return {"what": "tests/irs_optimize_w_point.py: the channel of the TRUE coefficients under the codes of rule 29 (ref), of rule "
                    "30 (w_1) and of rule 31 with weights over the taps and the antennas, %d sweeps from rule 29's codes; N = %d, "
                    "B = %d, k_factor = 0, direct path blocked, %d sets, DFT pilots, kappa = 1 / T; host float32 restatement, "
                    "no device; recorded, not gated" % (SWEEPS, N_ELEMS, BITS, SETS),
            "points": recs}


def main(argv):
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [here, os.path.join(here, ".."), os.path.join(here, "..", "gnuradio-wifi-imagetransfer_amd")]
    out = argv[argv.index("--out") + 1] if "--out" in argv else None
    recs = records()
    for r in recs:
        for k, f in r["arms"].items():
            print("%s sigma %.1f %-18s power %8.4f  tap 0 %8.4f  weakest / mean %.3f" % (
                r["scene"], r["sigma"], k, f["collected_power"], f["tap0_power"], f["median_weakest_subcarrier_over_mean"]))
    if out:
        with open(out, "w") as f:
            json.dump(document(recs), f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
