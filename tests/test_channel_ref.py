"""NUMERICS.md rule 17 on the host (tests/channel_ref.py) and the bookkeeping of wifirx.block.channel_model, without a GPU:
  * the restatement against txgen.impair's float64 multipath + CFO channel (tests/golden/sv_taps.npy sets);
  * its Philox4x32-10 against known answers of rocRAND's philox4x32_10 engine (the Random123 vectors);
  * a row cut into chunks that carry phase0 / sample0 gives the one-shot samples bit for bit;
  * the block, with the restatement in place of the device call, is independent of how work() is called."""
import math
import os

import numpy as np
import pytest

import channel_ref
from wifirx import block, capi, txgen

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_philox_known_answers():
    # rocrand_philox4x32_10.h, philox4x32_10_engine::ten_rounds(counter, key)
    cases = [
        ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
        ((0xFFFFFFFF,) * 4, (0xFFFFFFFF, 0xFFFFFFFF), (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
        ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
         (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
        ((12345, 7, 1, 0), (0x9ABCDEF0, 0x12345678), (0x05A9433C, 0x3B7D05B3, 0x41457989, 0x625C4CB2)),
    ]
    for c, k, want in cases:
        got = channel_ref.philox4x32_10(*[np.array([v], np.uint32) for v in c], *k)
        assert tuple(int(g[0]) for g in got) == want, (c, k)


def test_phase_inc_matches_the_library_rule():
    vals = [0.0, 1e-12, -1e-12, 3e-9, 0.001, -0.037, 0.05, 1.0, -2.5, math.pi, -math.pi, 3.2, -7.0, 100.0]
    vals += list(np.random.default_rng(3).uniform(-4, 4, 200))
    for v in vals:
        assert capi.phase_inc(v) == channel_ref.phase_inc(v), v
    assert channel_ref.phase_inc(0.0) == 0
    q = channel_ref.phase_inc(math.pi / 2)                          # float32(pi / 2): a quarter turn to float32 precision
    assert abs(q - (1 << 62)) < 1 << 40
    assert channel_ref.phase_inc(-math.pi / 2) == (1 << 64) - q


@pytest.mark.parametrize("L", [1, 2, 8])
def test_noiseless_restatement_against_txgen_impair(L):
    taps = np.load(os.path.join(GOLD, "sv_taps.npy"))
    assert taps.shape == (1024, 8)
    sets = taps[:, :L].astype(np.complex64)
    tx = txgen.encode_psdus(txgen.make_psdus(6, 100, seed=L), 4)
    rows = tx.samples.astype(np.complex64)
    n_rows, n = rows.shape
    rng = np.random.default_rng(40 + L)
    cfo = rng.uniform(-0.05, 0.05, n_rows).astype(np.float32)
    cfo[0], cfo[1] = 0.05, -0.05
    pick = rng.choice(1024, n_rows, replace=False)
    got = channel_ref.channel(rows, taps=sets[pick], cfo=cfo)
    # txgen.impair computes in float64 and rounds its result to complex64 once
    want = txgen.impair(rows, None, cfo=cfo.astype(np.float64), lead=0, total=n, taps=sets[pick].astype(np.complex128))
    tol = 1e-6 * (1.0 + np.abs(sets[pick]).sum(axis=1))
    err = np.abs(got.astype(np.complex128) - want.astype(np.complex128)).max(axis=1)
    assert (err <= tol).all(), (err, tol)


def _chunked(x, taps, inc, gain, nv, seed, cuts):
    """one row computed in pieces: each piece's row = the L - 1 inputs before it + the piece, phase0 / sample0 carried"""
    L = len(taps)
    out = []
    lo = 0
    for hi in list(cuts) + [x.size]:
        h = min(L - 1, lo)
        y = channel_ref.channel_row(x[lo - h:hi], taps, inc, (inc * (lo - h)) & channel_ref.M64, gain, nv, seed, lo - h)
        out.append(y[h:])
        lo = hi
    return np.concatenate(out)


@pytest.mark.parametrize("L", [1, 5])
def test_phase_and_noise_chain_across_chunks(L):
    rng = np.random.default_rng(L)
    n = 3001
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    taps = (rng.standard_normal(L) + 1j * rng.standard_normal(L)).astype(np.complex64)
    inc = channel_ref.phase_inc(0.0371)
    one = channel_ref.channel_row(x, taps, inc, 0, 3.5, 0.3, 77, 0)
    for cuts in ([1500], [1, 2, 3, 400, 401, 1777, 2999]):
        assert np.array_equal(_chunked(x, taps, inc, 3.5, 0.3, 77, cuts).view(np.uint32), one.view(np.uint32)), cuts


class _FakeRx:
    """capi.WifiRx with the restatement in place of the device call"""
    calls = []

    def __init__(self, *a, **kw):
        pass

    def channel(self, x, **kw):
        _FakeRx.calls.append((x.size, kw["sample0"], kw["phase0"]))
        return channel_ref.channel(x, **kw)

    def close(self):
        pass


def _run_block(x, sizes, **kw):
    blk = block.channel_model(**kw)
    out = np.zeros_like(x)
    pos = k = 0
    while pos < x.size:
        n = min(sizes[k % len(sizes)], x.size - pos)
        k += 1
        assert blk.work([x[pos:pos + n]], [out[pos:pos + n]]) == n
        pos += n
    blk.close()
    return out


def test_block_output_does_not_depend_on_chunking(monkeypatch):
    monkeypatch.setattr(capi, "WifiRx", _FakeRx)
    rng = np.random.default_rng(11)
    n = 4000
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    taps = (rng.standard_normal(8) + 1j * rng.standard_normal(8)).astype(np.complex64) * np.float32(0.3)
    kw = dict(noise_voltage=0.25, frequency_offset=0.0123, taps=taps, noise_seed=5)
    cfo = np.float32(2 * math.pi * 0.0123)
    want = channel_ref.channel(x, taps=taps, cfo=cfo, noise_voltage=0.25, seed=5)
    for sizes in ([n], [1], [3, 1, 6, 2], list(rng.integers(1, 700, 40))):
        _FakeRx.calls = []
        got = _run_block(x, sizes, **kw)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), sizes
        assert _FakeRx.calls[0][1] == 0 and _FakeRx.calls[0][2] == 0


def test_block_frequency_change_keeps_the_phase(monkeypatch):
    monkeypatch.setattr(capi, "WifiRx", _FakeRx)
    n, cut = 2000, 777
    x = np.ones(n, np.complex64)
    blk = block.channel_model(noise_voltage=0.0, frequency_offset=0.01)
    out = np.zeros_like(x)
    blk.work([x[:cut]], [out[:cut]])
    blk.set_frequency_offset(-0.02)
    assert blk.frequency_offset() == -0.02
    blk.work([x[cut:]], [out[cut:]])
    i1 = channel_ref.phase_inc(np.float32(2 * math.pi * 0.01))
    i2 = channel_ref.phase_inc(np.float32(2 * math.pi * -0.02))
    assert np.array_equal(out[:cut], channel_ref.channel_row(x[:cut], [1.0], i1))
    assert np.array_equal(out[cut:], channel_ref.channel_row(x[cut:], [1.0], i2, (i1 * cut) & channel_ref.M64))


def test_block_arguments(monkeypatch):
    monkeypatch.setattr(capi, "WifiRx", _FakeRx)
    with pytest.raises(ValueError, match="sample-rate offset is not supported"):
        block.channel_model(epsilon=1.0001)
    blk = block.channel_model(noise_voltage=0.5, frequency_offset=0.1, taps=[1, 0.5j], noise_seed=3)
    assert blk.noise_voltage() == 0.5 and blk.frequency_offset() == 0.1 and blk.timing_offset() == 1.0
    assert np.array_equal(blk.taps(), np.array([1, 0.5j], np.complex64))
    blk.set_noise_voltage(2.0)
    blk.set_taps([0.25])
    assert blk.noise_voltage() == 2.0 and blk.taps().size == 1
    with pytest.raises(ValueError):
        blk.set_taps(np.ones(65))
    with pytest.raises(ValueError):
        blk.set_timing_offset(0.9)
    assert blk.in_sig == [np.complex64] and blk.out_sig == [np.complex64]
