"""The operating point of the end-to-end stream-diversity test (tests/test_gpu_stream_diversity.py::test_stream_diversity_gain)
and the host chain that confirms its inequalities for the chosen seeds before the device is asked:
txgen -> fading_ref.channel -> oracle demod -> diversity_ref -> the oracle's decode_mac (tests/diversity_point.py's chain).

512 config-2 frames (294 bytes, QPSK 1/2) through a flat Rayleigh channel with doppler = 0 -- one static complex gain per frame and
antenna (NUMERICS.md rule 19) --, two antennas that differ in fade_seed and noise seed, 12 dB mean SNR: the operating point of
tests/diversity_point.py, where the single-antenna FER is 0.21.  The rows, laid end to end, are the antennas' streams.

    python tests/stream_diversity_point.py [--out profiles/stream_diversity_operating_point.json]"""
import math
import os
import sys

import numpy as np

N, ENC, PLEN, LEAD, TAIL = 512, 2, 294, 160, 79
SNR_DB = 12.0
PSDU_SEED = 29
SEEDS = ((9300, 21), (9400, 22))       # (noise seed, fade_seed) of antenna 0, 1


def geometry():
    from wifirx import txgen
    n_sym = txgen.n_sym_for(PLEN, ENC)
    slot = LEAD + txgen.frame_samples(PLEN, ENC) + TAIL
    return n_sym, slot + (slot & 1)


def host_chain(n=N, snr_db=SNR_DB):
    """lost frames (of n) of each antenna alone, of SELECT and of MRC: hard decisions, batch form (every row its own slot)"""
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
    for seed, fade_seed in SEEDS:
        y = fading_ref.channel(rows, taps=(1.0,), gain=math.sqrt(10 ** (snr_db / 10)), noise_voltage=1.0, seed=seed, doppler=0.0,
                               fade_seed=fade_seed)
        ant.append(orc.demod_batch(y, slot, prm, want_eq=True, want_csi=True, n_threads=8))

    def lost(frames, idx):
        fr = frames.copy()
        got = orc.decode_batch(fr, idx, prm, psdu_stride=320, n_threads=8)
        ok = ((fr["flags"] & 0x40) != 0) & (fr["psdu_len"] == PLEN) & (got[:, :PLEN] == psdus).all(axis=1)
        return int(n - ok.sum())

    res = {"frames": n, "snr_db": snr_db, "single": [lost(o["frames"], o["idx"]) for o in ant]}
    for name, mode in (("select", dr.SELECT), ("mrc", dr.MRC)):
        out = dr.new_outputs(n, n_sym, 2, fill=0)
        dr.combine([o["frames"] for o in ant], [o["eq"] for o in ant], [o["csi"] for o in ant], n_sym, 2, out, mode=mode)
        res[name] = lost(out["frames"], out["idx"])
    res["holds"] = bool(res["mrc"] <= res["select"] and 2 * res["mrc"] <= min(res["single"]))
    return res


if __name__ == "__main__":
    import argparse
    import json
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [ROOT, os.path.join(ROOT, "gnuradio-wifi-imagetransfer_amd")]
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rec = {"what": "lost frames of %d QPSK-1/2 frames of %d bytes, flat Rayleigh independent per antenna and frame, %g dB, two antennas: "
                   "each antenna alone, selection, maximal-ratio combining" % (N, PLEN, SNR_DB),
           "host_chain": host_chain()}
    if a.out and os.path.exists(a.out):             # the device's counts, written by hand from the GPU test's output, stay
        old = json.load(open(a.out))
        rec.update({k: v for k, v in old.items() if k not in rec})
    print(json.dumps(rec))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")
