"""The three scenes that tests/test_frontend_ref.py and tests/test_gpu_stream_frontend.py share: a stream of 24 frames in
slots, impaired by a receiver's DC offset and IQ imbalance, and the count of late frames that decode."""
import numpy as np

import frontend_ref as fr

N_FRAMES, PSDU_LEN = 24, 100
LATE_FROM = 8192                 # late frames: those whose slot starts at sample >= 8192 (behind the first two blocks)

# name: (encoding, snr_db, iq_gain_db, iq_phase_deg, DC power over the noise power)
SCENES = {"a": (2, 20.0, 0.0, 0.0, 100.0), "b": (7, 26.0, 1.0, 5.0, 9.0), "c": (7, 30.0, 0.0, 0.0, 0.0)}


def build(name):
    """(impaired stream complex64, PSDUs [24, 100], slot length)"""
    from wifirx import txgen
    enc, snr, gain_db, phase_deg, p = SCENES[name]
    psdus = txgen.make_psdus(N_FRAMES, PSDU_LEN)
    tx = txgen.encode_psdus(psdus, enc)
    n = tx.samples.shape[1]
    x = txgen.impair(tx.samples, snr, cfo=0.002, lead=300, total=n + 1200, seed=7).reshape(-1).astype(np.complex64)
    mu, nu = fr.imbalance(gain_db, phase_deg)
    return fr.rx_impair(x, mu, nu, np.sqrt(p) * np.exp(0.7j)), psdus, n + 1200


def late_slots(slot_len):
    return [k for k in range(N_FRAMES) if k * slot_len >= LATE_FROM]


def good_slots(frames, psdu, psdus, slot_len):
    """the slots whose frame came out with a good CRC and the transmitted bytes; frames: records with the absolute trigger"""
    good = set()
    for f, row in zip(frames, psdu):
        k = int(f["trigger"]) // slot_len
        if (int(f["flags"]) & 64) and int(f["psdu_len"]) == PSDU_LEN and k < N_FRAMES and np.array_equal(row[:PSDU_LEN], psdus[k]):
            good.add(k)
    return good


def oracle_good(orc, x, psdus, slot_len, max_sym=64):
    """(good slots, oracle stream result, PSDU rows) of the oracle's stream receiver on x"""
    prm = orc.make_params(max_sym=max_sym)
    o = orc.demod_stream(np.ascontiguousarray(x, dtype=np.complex64), prm, want_eq=False, cap=4096)
    rows = orc.decode_batch(o["frames"], o["idx"], prm, psdu_stride=2048)
    return good_slots(o["frames"], rows, psdus, slot_len), o, rows
