#!/usr/bin/env python3
"""Record the reference's reflecting-surface channel for an AP of M antennas as a fixture: tests/golden/irs_multi_reference.npz.

Runs only where the reference tree exists (its path is the one argument); utils/SV_channel.py and utils/channel.py are
imported from it at run time, and only what they computed is written.  For S = 2 and 4 (N = S^2 elements) and M = 2 and 4 AP
antennas (antennaNum = M), the AP and surface positions of tools/make_golden_irs.py and its first user position, the file
holds, all as complex128:

  los_S{S}_M{M}_{b2r,r2u,b2u}     Saleh_Valenzuela_Channel.genLoS: [M, N], [N], [M]
  nlos_S{S}_M{M}                  [8, (M + 1) N + M]: per recorded NumPy seed the genNonLoS draws, as rows b2r[0][N] .. b2r[M-1][N],
                                  r2u[N], b2u[M] -- the layout of wifirx_irs_taps_multi's scatter
  mix_S{S}_M{M}                   [8, (M + 1) N + M]: RicianRefresh(K = 10) after the same seed (it makes the same draws), same layout
  psi_S{S}                        [2, N]: every phase e^{j pi}, and seeded random phases
  H_S{S}_M{M}                     [8, 2, M]: Channel.getChnl of the mixes, per seed and psi
  seeds, k_factor                 the seeds and K; irs_pos_S{S}, ap_pos_S{S}, user_pos_S{S} the positions [3]
"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "..", "tests", "golden", "irs_multi_reference.npz")
SEEDS = np.arange(201, 209)
K = 10
SCALES = (2, 4)
ANTENNAS = (2, 4)


def row(b2r, r2u, b2u):
    return np.concatenate([np.asarray(b2r).reshape(-1), np.asarray(r2u).reshape(-1), np.asarray(b2u).reshape(-1)])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("reference", help="root of the reference tree")
    args = ap.parse_args()
    sys.path.insert(0, args.reference)
    from utils.SV_channel import Saleh_Valenzuela_Channel      # (both modules seed NumPy with 0 at import)
    from utils.channel import Channel

    out = {"seeds": SEEDS, "k_factor": np.float64(K)}
    for S in SCALES:
        N, interval = S * S, 0.03
        irs_pos = np.array([interval / 2, interval / 2, 0])
        ap_pos = np.array([S * interval / 2, S * interval / 2, 4.5])
        user = np.array([[S * interval / 2 + 0.3, S * interval / 2 - 0.2, 1.0]])
        out["user_pos_S%d" % S], out["irs_pos_S%d" % S], out["ap_pos_S%d" % S] = user[0], irs_pos, ap_pos
        psi = np.stack([np.exp(1j * np.pi * np.ones(N)),
                        np.exp(1j * 2 * np.pi * np.random.default_rng(2000 + S).random(N))])
        out["psi_S%d" % S] = psi
        for M in ANTENNAS:
            ch = Saleh_Valenzuela_Channel(S, irs_pos, ap_pos, 1, M)
            b2r, r2u, b2u = ch.genLoS(user)
            tag = "S%d_M%d" % (S, M)
            out["los_%s_b2r" % tag] = np.array(b2r).reshape(M, N)
            out["los_%s_r2u" % tag] = np.array(r2u).reshape(-1)
            out["los_%s_b2u" % tag] = np.array(b2u).reshape(-1)
            nlos, mixes, H = [], [], np.zeros((len(SEEDS), 2, M), np.complex128)
            for i, s in enumerate(SEEDS):
                np.random.seed(int(s))
                nlos.append(row(*ch.genNonLoS()))
                np.random.seed(int(s))
                m_b2r, m_r2u, m_b2u = ch.RicianRefresh(K=K)
                mixes.append(row(m_b2r, m_r2u, m_b2u))
                for j in range(2):
                    H[i, j] = np.asarray(Channel(1, M, N).getChnl(m_b2u, m_b2r, m_r2u, psi[j])).reshape(-1)
            out["nlos_" + tag], out["mix_" + tag], out["H_" + tag] = np.array(nlos), np.array(mixes), H
    out = {k: (np.asarray(v, dtype=np.complex128) if np.iscomplexobj(v) else np.asarray(v)) for k, v in out.items()}
    np.savez_compressed(OUT, **out)
    print("wrote %s: %d arrays, %d bytes" % (OUT, len(out), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
