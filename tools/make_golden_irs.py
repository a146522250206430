#!/usr/bin/env python3
"""Record the reference's own reflecting-surface channel as a fixture: tests/golden/irs_reference.npz.

Runs only where the reference tree exists (its path is the one argument); utils/SV_channel.py and utils/channel.py are
imported from it at run time, and only what they computed is written.  For S = 2, 4 and 16 (N = S^2 elements), the AP and
surface positions of make_golden_from_reference.sv_taps and two user positions (its own and one more), the file holds, all as
complex128:

  los_S{S}_u{u}_{b2r,r2u,b2u}     Saleh_Valenzuela_Channel.genLoS: [N], [N], scalar
  nlos_S{S}_u{u}                  [8, 2 N + 1]: per recorded NumPy seed the genNonLoS draws, as rows b2r[N], r2u[N], b2u --
                                  the layout of wifirx_irs_taps' scatter
  mix_S{S}_u{u}                   [8, 2 N + 1]: RicianRefresh(K = 10) after the same seed (it makes the same draws), same layout
  psi_S{S}                        [2, N]: every phase e^{j pi}, and seeded random phases
  H_S{S}_u{u}                     [8, 2]: Channel.getChnl of the mixes, per seed and psi
  seeds, k_factor, user_pos       the seeds, K, and the user positions [2, 3]
"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "..", "tests", "golden", "irs_reference.npz")
SEEDS = np.arange(101, 109)
K = 10
SCALES = (2, 4, 16)


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
        users = np.array([[S * interval / 2 + 0.3, S * interval / 2 - 0.2, 1.0],
                          [S * interval / 2 - 1.1, S * interval / 2 + 0.7, 1.5]])
        out["user_pos_S%d" % S] = users
        out["irs_pos_S%d" % S], out["ap_pos_S%d" % S] = irs_pos, ap_pos
        psi = np.stack([np.exp(1j * np.pi * np.ones(N)),
                        np.exp(1j * 2 * np.pi * np.random.default_rng(1000 + S).random(N))])
        out["psi_S%d" % S] = psi
        for u in range(len(users)):
            ch = Saleh_Valenzuela_Channel(S, irs_pos, ap_pos, 1, 1)
            b2r, r2u, b2u = ch.genLoS(users[u:u + 1])
            tag = "S%d_u%d" % (S, u)
            out["los_%s_b2r" % tag] = np.array(b2r).reshape(-1)
            out["los_%s_r2u" % tag] = np.array(r2u).reshape(-1)
            out["los_%s_b2u" % tag] = np.array(b2u).reshape(-1)[0]
            nlos, mixes, H = [], [], np.zeros((len(SEEDS), 2), np.complex128)
            for i, s in enumerate(SEEDS):
                np.random.seed(int(s))
                nlos.append(row(*ch.genNonLoS()))
                np.random.seed(int(s))
                m_b2r, m_r2u, m_b2u = ch.RicianRefresh(K=K)
                mixes.append(row(m_b2r, m_r2u, m_b2u))
                for j in range(2):
                    H[i, j] = np.asarray(Channel(1, 1, N).getChnl(m_b2u, m_b2r, m_r2u, psi[j])).reshape(-1)[0]
            out["nlos_" + tag], out["mix_" + tag], out["H_" + tag] = np.array(nlos), np.array(mixes), H
    out = {k: (np.asarray(v, dtype=np.complex128) if np.iscomplexobj(v) else np.asarray(v)) for k, v in out.items()}
    np.savez_compressed(OUT, **out)
    print("wrote %s: %d arrays, %d bytes" % (OUT, len(out), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
