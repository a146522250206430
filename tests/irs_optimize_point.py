"""What the joint decision (NUMERICS.md rule 30, tests/irs_optimize_ref.py) is worth on the host, measured with the project's own
float32 arithmetic: the power an MRC receiver collects under the joint codes relative to the power under rule 29's decision
(antenna 0, tap 0).

Scenes: an 8 x 8 surface (N = 64, every element its own group), 2-bit phases, pure scattering (k_factor = 0), the direct path
blocked, M = 4 antennas with L = 1 tap and with L = 8 taps of an exponential power delay profile, SETS tap sets each.  The
coefficients come from tests/irs_estimate_ref.py (rule 29: the 65-point DFT pilots, kappa = 1 / T) at sigma = 0 -- the joint genie
bound -- and at tests/irs_estimate_point.py's operating point sigma = 3.5.  The ascent starts from rule 29's codes and runs at
most SWEEPS sweeps.  The collected power is the float64 power of the TRUE coefficients (irs_estimate_ref.truth) under the codes;
the objective is the same for the estimate the optimiser was given.  profiles/irs_optimize_operating_point.json holds the values.

    python tests/irs_optimize_point.py [--out profiles/irs_optimize_operating_point.json]"""
import json
import os
import sys

import numpy as np

SETS, SCALE, BITS, SWEEPS, M = 64, 8, 2, 4, 4
N_ELEMS = SCALE * SCALE
IRS_SEED = 61
SCENES = {"M4_L1": 1, "M4_L8": 8}
PREDICTED = {"M4_L1": 1.28, "M4_L8": 1.38}          # the float64 sketch that motivated the rule: to compare with, not a gate


def pdp_of(L):
    p = np.exp(-np.arange(L) / 2.0)
    return (p / p.sum()).astype(np.float32)


def sigmas():
    import irs_estimate_point as ep
    return (0.0, ep.SIGMA)


def point(name, sigma):
    """one scene at one sigma: a dict of the measured values and the arrays the test asserts on"""
    import irs_estimate_ref as er
    import irs_optimize_ref as orf
    from wifirx import irs
    L = SCENES[name]
    pdp = pdp_of(L)
    a, b = np.ones((M, N_ELEMS), np.complex64), np.ones(N_ELEMS, np.complex64)       # not looked at with k_factor = 0
    pl = irs.dft_pilots(N_ELEMS)
    out = er.irs_estimate(SETS, pdp, a, b, None, pilots=pl, sigma=sigma, est_scale=irs.est_scale(pl.shape[0]), align_bits=BITS,
                          k_factor=0.0, direct_gain=0.0, seed=IRS_SEED)
    truth = er.truth(out, pdp, 1.0, np.arange(N_ELEMS), N_ELEMS, M)[0]
    res = orf.optimize(out["est"], BITS, SWEEPS, blocked=True)
    assert res["codes"].shape == out["codes"].shape
    p_joint, p_ref = orf.true_power(truth, res["codes"], BITS, True), orf.true_power(truth, out["codes"], BITS, True)
    o_joint, o_ref = orf.true_power(out["est"], res["codes"], BITS, True), orf.true_power(out["est"], out["codes"], BITS, True)
    return {"scene": name, "sigma": sigma, "est": out["est"], "p_joint": p_joint, "p_ref": p_ref, "o_joint": o_joint, "o_ref": o_ref,
            "res": res, "ref_codes": out["codes"]}


def record(pt):
    r = pt["p_joint"] / pt["p_ref"]
    return {"scene": pt["scene"], "sigma": pt["sigma"], "sets": SETS,
            "power_ratio_of_means": float(pt["p_joint"].sum() / pt["p_ref"].sum()),
            "power_ratio_per_set_min": float(r.min()), "power_ratio_per_set_median": float(np.median(r)),
            "objective_ratio_of_means": float(pt["o_joint"].sum() / pt["o_ref"].sum()),
            "objective_ratio_per_set_min": float((pt["o_joint"] / pt["o_ref"]).min()),
            "codes_changed_fraction": float((pt["res"]["codes"] != pt["ref_codes"]).mean()),
            "sweeps_mean": float(pt["res"]["sweeps"].mean()), "predicted_by_the_float64_sketch": PREDICTED[pt["scene"]]}


def main(argv):
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [here, os.path.join(here, ".."), os.path.join(here, "..", "gnuradio-wifi-imagetransfer_amd")]
    out = argv[argv.index("--out") + 1] if "--out" in argv else None
    recs = [record(point(name, s)) for name in SCENES for s in sigmas()]
    for r in recs:
        print("%s sigma %.1f: joint / ref collected power %.4f (per set: min %.4f, median %.4f), objective %.4f, %.1f %% of the "
              "codes changed, %.2f sweeps" % (r["scene"], r["sigma"], r["power_ratio_of_means"], r["power_ratio_per_set_min"],
                                              r["power_ratio_per_set_median"], r["objective_ratio_of_means"],
                                              100 * r["codes_changed_fraction"], r["sweeps_mean"]))
    rec = {"what": "tests/irs_optimize_point.py: the restatement's collected power under the joint codes (rule 30, %d sweeps from rule "
                   "29's codes) over the power under rule 29's codes; N = %d, B = %d, M = %d, k_factor = 0, direct path blocked, %d "
                   "sets, DFT pilots, kappa = 1 / T; host float32 restatement, no device" % (SWEEPS, N_ELEMS, BITS, M, SETS),
           "points": recs}
    if out:
        with open(out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
