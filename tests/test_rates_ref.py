"""The host statements of tests/rates_ref.py against each other and against txgen (no GPU)."""
import numpy as np

import link_ref
import rates_ref
import tx_ref
from wifirx import txgen


def test_encode_rates_is_one_encode_per_frame_and_close_to_txgen():
    rng = np.random.default_rng(1)
    lens = [1, 30, 100, 294, 61, 7, 500, 23]
    psdus = [rng.integers(0, 256, L, dtype=np.uint8).tobytes() for L in lens]
    encs = np.array([7, 0, 3, 6, 1, 5, 2, 4])
    seeds = rng.integers(1, 128, len(psdus))
    got = rates_ref.encode_rates(psdus, encs, seeds)
    for p, e, s, g in zip(psdus, encs, seeds, got):
        row = np.frombuffer(p, np.uint8)[None]
        assert g.size == txgen.frame_samples(len(p), int(e))
        assert np.array_equal(g, tx_ref.encode(row, int(e), [int(s)])[0])
        assert np.abs(g - txgen.encode_psdus(row, int(e), [int(s)]).samples[0]).max() <= 1e-6
    # the default seeds are those of wifirx_tx_batch: (i % 127) + 1
    again = rates_ref.encode_rates(psdus, encs)
    assert np.array_equal(again[3], tx_ref.encode(np.frombuffer(psdus[3], np.uint8)[None], 6, [4])[0])


def hand_made(seed, max_sym=12):
    """every class of link_ref.CLASSES at every encoding, twice, in a shuffled order"""
    rng = np.random.default_rng(seed)
    n_cls = len(link_ref.CLASSES)
    classes = np.tile(np.repeat(np.arange(n_cls), 8), 2)
    enc = np.tile(np.tile(np.arange(8), n_cls), 2)
    order = rng.permutation(classes.size)
    classes, enc = classes[order], enc[order]
    n_sym = rng.integers(1, max_sym + 1, classes.size)
    return link_ref.hand_made_batch(rng, classes, enc, n_sym, max_sym) + (classes, enc)


def test_link_stats_by_rate_on_a_hand_made_batch():
    max_sym = 12
    rx, ref, classes, enc = hand_made(5, max_sym)
    assert set(enc.tolist()) == set(range(8)) and set(classes.tolist()) == set(range(len(link_ref.CLASSES)))
    incomplete = link_ref.CLASSES.index("ref_incomplete")
    for use_hbits in (True, False):
        total, by_rate = rates_ref.link_stats_by_rate(rx, ref, max_sym, use_hbits)
        assert total == link_ref.link_stats(rx, ref, max_sym, use_hbits)[0]
        rates_ref.check_sums(total, by_rate)
        _, err, cls = link_ref.link_stats(rx, ref, max_sym, use_hbits)
        for e in range(8):
            # a reference record that is not complete lands in no rate
            sel = (enc == e) & (classes != incomplete)
            b = by_rate[e]
            assert b["frames"] == b["frames_ref"] == int(sel.sum()) == 2 * (len(link_ref.CLASSES) - 1)
            assert b["frames_good"] == int((cls[sel] & 1).sum())
            assert b["frames_crc_ok"] == int(((cls[sel] >> 1) & 1).sum())
            assert b["frames_psdu_ok"] == int(((cls[sel] >> 2) & 1).sum())
            good = sel & ((cls & 1) != 0)
            assert b["coded_bit_errors"] == int(err[good].astype(np.int64).sum())
            assert b["coded_bit_errors_sq"] == int((err[good].astype(object) ** 2).sum())
            assert b["coded_bits"] > 0 and b["coded_bit_errors"] > 0
        assert total["frames"] - total["frames_ref"] == int((classes == incomplete).sum())
    # both forms of the decisions count the same
    assert rates_ref.link_stats_by_rate(rx, ref, max_sym, True) == rates_ref.link_stats_by_rate(rx, ref, max_sym, False)
