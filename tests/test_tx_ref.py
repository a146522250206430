"""NUMERICS.md rule 16 (tests/tx_ref.py, the float32 transmitter wifirx_tx_batch must match bit for bit) against the float64
transmitter txgen.encode_psdus it restates: within 1e-6 per sample at every encoding and length, with mixed seeds."""
import numpy as np
import pytest

import tx_ref
from test_annex_data_kat import ANNEX_PSDU
from wifirx import txgen

LENGTHS = (1, 24, 100, 294, 1500, 4095)


def psdus(n, length, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(n, length), dtype=np.uint8)


@pytest.mark.parametrize("enc", range(8))
def test_rule16_within_1e6_of_txgen(enc):
    for length in LENGTHS:
        n = 3 if length > 1000 else 8
        p = psdus(n, length, 100 * enc + length)
        seeds = np.random.default_rng(length).integers(1, 128, size=n)
        got = tx_ref.encode(p, enc, seeds)
        want = txgen.encode_psdus(p, enc, seeds).samples
        assert got.shape == want.shape == (n, txgen.frame_samples(length, enc))
        assert got.dtype == np.complex64
        assert np.abs(got - want).max() <= 1e-6, (enc, length)


def test_annex_example_data_idx():
    """the Annex message (16-QAM 3/4, scrambler state 1011101): the restatement takes txgen's bits, which are the standard's"""
    p = np.frombuffer(ANNEX_PSDU, dtype=np.uint8)[None]
    tx = txgen.encode_psdus(p, txgen.QAM16_3_4, seeds=[0b1011101])
    X = tx_ref.freq_symbols(tx)
    pts = txgen.constellation_points(4).astype(np.complex64)
    got_idx = np.abs(X[0, 5:, txgen.DATA_BINS].T[:, :, None] - pts[None, None, :]).argmin(axis=2)
    assert np.array_equal(got_idx, tx.data_idx[0])
    assert tx.n_sym == 6 and tx_ref.encode(p, txgen.QAM16_3_4, [0b1011101]).shape == (1, 11 * 80 + 1)


def test_roll_off_and_window():
    """frame = sync, SIGNAL, data; the first CP sample is half its own plus half the previous symbol's first sample"""
    p = psdus(2, 50, 7)
    x = tx_ref.ifft_spec(tx_ref.freq_symbols(txgen.encode_psdus(p, 3)))
    f = tx_ref.encode(p, 3)
    h = np.float32(0.5)
    assert f[0, 0] == np.complex64(h * x[0, 0, 48].real + 1j * (h * x[0, 0, 48].imag))
    s = 7
    want = (h * x[1, s, 48].real + h * x[1, s - 1, 0].real) + 1j * (h * x[1, s, 48].imag + h * x[1, s - 1, 0].imag)
    assert f[1, 80 * s] == np.complex64(want)
    assert np.array_equal(f[1, 80 * s + 16:80 * s + 80], x[1, s])
    assert f[1, -1] == np.complex64(h * x[1, -1, 0].real + 1j * (h * x[1, -1, 0].imag))
