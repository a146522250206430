"""tests/spectrum_ref.py, the NumPy float32 restatement of NUMERICS.md rule 36, held against the float64 definition within the
rule's derived bound; a tone's bin; the tables against float64, their subset property and T[1024]; every mutant caught; the
counting against a brute-force enumeration; cuts at `consumed`; the fold, the band sums and the band edges."""
import numpy as np
import pytest

import convert_ref as cr
import spectrum_ref as sr

FORMATS = [cr.FC32, cr.SC16, cr.SC8]
FMT_ID = {cr.FC32: "fc32", cr.SC16: "sc16", cr.SC8: "sc8"}
SC8_ODD_SCALE = 1.0 / 93.0


def noise(rng, n, fmt):
    """(samples of the format [n, 2], scale, the widened float32 pairs): unit Gaussian noise; the integer formats hold it
    at 1 / scale per unit, sc8 at an odd scale"""
    x = rng.standard_normal((n, 2))
    if fmt == cr.FC32:
        x = x.astype(np.float32)
        return x, float("nan"), x
    scale = cr.SCALE[fmt] * np.float32(4) if fmt == cr.SC16 else np.float32(SC8_ODD_SCALE)
    info = np.iinfo(cr.DTYPE[fmt])
    q = np.clip(np.rint(x / float(scale)), info.min, info.max).astype(cr.DTYPE[fmt])
    return q, float(scale), cr.widen(q, scale)


@pytest.mark.parametrize("fmt", FORMATS, ids=[FMT_ID[f] for f in FORMATS])
@pytest.mark.parametrize("n_fft", sr.N_FFT)
def test_restatement_within_the_derived_bound_of_the_definition(n_fft, fmt):
    rng = np.random.default_rng(36 + n_fft + fmt)
    worst = 0.0
    for hop in (n_fft, n_fft // 2, n_fft // 4 + 1):
        for avg in (1, 3):
            q, scale, x = noise(rng, (2 * avg) * hop + n_fft + 5, fmt)
            for window in (sr.RECT, sr.HANN, sr.BLACKMAN_HARRIS):
                for mode in (sr.SUM, sr.MAX):
                    got = sr.spectrum_format(q, fmt, scale, n_fft, hop, avg, window, mode)
                    want = sr.definition(x, n_fft, hop, avg, window, mode)
                    assert got.shape == want.shape and got.shape[0] >= 2
                    err = float((np.abs(got - want) / want.mean(axis=1, keepdims=True)).max())
                    worst = max(worst, err)
                    assert err <= sr.error_bound(n_fft, avg), (hop, avg, window, mode, err)
    print("n_fft %d %s: measured %.2e, bound %.2e" % (n_fft, FMT_ID[fmt], worst, sr.error_bound(n_fft, 3)))


@pytest.mark.parametrize("n_fft", sr.N_FFT)
def test_a_tone_at_bin_k_lands_in_bin_k_plus_half(n_fft):
    """k on both sides of the first stage's boundaries (multiples of N / 4), of a later stage's, and at the band's ends"""
    n = np.arange(n_fft)
    for k in (0, 1, 3, 4, 5, 15, 16, 17, n_fft // 4 - 1, n_fft // 4, n_fft // 4 + 1, n_fft // 2 - 1, -1, -n_fft // 4, -n_fft // 2):
        z = np.exp(2j * np.pi * k * n / n_fft)
        x = np.stack([z.real, z.imag], axis=1).astype(np.float32)
        row = sr.spectrum(x, n_fft, n_fft, 1, sr.RECT)[0]
        assert int(np.argmax(row)) == k + n_fft // 2, k
        assert abs(row[k + n_fft // 2] / float(n_fft) ** 2 - 1) < 1e-4
        assert np.delete(row, k + n_fft // 2).max() < 1e-6 * n_fft ** 2, k


def test_tables_against_float64():
    hann, bh, tw = sr.tables()
    assert hann.shape == bh.shape == (sr.ENTRIES,) and tw.shape == (sr.ENTRIES, 2) and tw.dtype == hann.dtype == np.float32
    k = np.arange(sr.ENTRIES)
    half_ulp = 2.0 ** -24
    exact = np.exp(-2j * np.pi * k / sr.ENTRIES)
    assert np.abs(tw[:, 0] - exact.real).max() <= half_ulp and np.abs(tw[:, 1] - exact.imag).max() <= half_ulp
    assert np.abs(hann - sr.window64(sr.HANN, sr.ENTRIES)).max() <= half_ulp
    assert np.abs(bh - sr.window64(sr.BLACKMAN_HARRIS, sr.ENTRIES)).max() <= half_ulp
    # exactly: the axes, and a quarter turn is a swap of parts (the octant symmetry)
    assert tw[0].tolist() == [1.0, 0.0] and tw[1024].tolist() == [0.0, -1.0] and tw[2048].tolist() == [-1.0, 0.0] and tw[3072].tolist() == [0.0, 1.0]
    assert not np.signbit(tw[1024, 0]) and not np.signbit(tw[0, 1])
    assert np.array_equal(tw[1024:, 0], tw[:3072, 1]) and np.array_equal(tw[1025:, 1], -tw[1:3072, 0])
    assert hann[0] == 0.0 and hann[2048] == 1.0


def test_the_built_tables_are_the_generators_pinned_bytes():
    """csrc/wr_spectrum_table.h is written when the library is built: the tables in the library hash to the generator's
    TABLE_SHA256, and so does what the generator computes here"""
    import hashlib
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "gen_spectrum_table.py")
    spec = importlib.util.spec_from_file_location("gen_spectrum_table", path)
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    hann, bh, tw = sr.tables()
    built = hashlib.sha256(b"".join(np.ascontiguousarray(t, dtype="<f4").tobytes() for t in (tw, hann, bh))).hexdigest()
    assert built == gen.TABLE_SHA256 == gen.table_sha256()


@pytest.mark.parametrize("n_fft", sr.N_FFT)
def test_a_window_of_n_points_is_the_strided_subset(n_fft):
    """the subset of the 4096-entry tables is the float32 rounding of the N-point formula"""
    hann, bh, tw = sr.tables()
    s = sr.ENTRIES // n_fft
    assert np.abs(hann[::s] - sr.window64(sr.HANN, n_fft)).max() <= 2.0 ** -24
    assert np.abs(bh[::s] - sr.window64(sr.BLACKMAN_HARRIS, n_fft)).max() <= 2.0 ** -24
    e = np.exp(-2j * np.pi * np.arange(n_fft) / n_fft)
    assert np.abs(tw[::s, 0] - e.real).max() <= 2.0 ** -24 and np.abs(tw[::s, 1] - e.imag).max() <= 2.0 ** -24


@pytest.mark.parametrize("mutant", sr.MUTANTS)
def test_every_mutant_is_caught(mutant):
    """each mutant leaves the definition by more than the bound in at least one of the two modes (norm = -1 so that a norm applied
    in front of the MAX fold picks other segments); the restatement itself stays inside"""
    rng = np.random.default_rng(7)
    n_fft, hop, avg = 256, 128, 3
    x = rng.standard_normal((n_fft * 8, 2)).astype(np.float32)
    caught = False
    for mode in (sr.SUM, sr.MAX):
        want = sr.definition(x, n_fft, hop, avg, sr.HANN, mode, -1.0)
        scale = np.abs(want).mean(axis=1, keepdims=True)
        good = sr.spectrum(x, n_fft, hop, avg, sr.HANN, mode, -1.0)
        assert float((np.abs(good - want) / scale).max()) <= sr.error_bound(n_fft, avg)
        bad = sr.spectrum(x, n_fft, hop, avg, sr.HANN, mode, -1.0, mutant=mutant)
        caught |= float((np.abs(bad - want) / scale).max()) > sr.error_bound(n_fft, avg)
    assert caught, mutant


def test_count_against_a_brute_force_enumeration():
    rng = np.random.default_rng(8)
    for _ in range(300):
        n_fft = int(rng.choice(sr.N_FFT))
        hop, avg, n_in = int(rng.integers(1, 3 * n_fft)), int(rng.integers(1, 5)), int(rng.integers(0, 12 * n_fft))
        S, s = 0, 0
        while s + n_fft <= n_in:
            S, s = S + 1, s + hop
        rows = 0
        while (rows + 1) * avg <= S:
            rows += 1
        assert sr.count(n_fft, hop, avg, n_in) == (rows, rows * avg * hop)


@pytest.mark.parametrize("fmt", FORMATS, ids=[FMT_ID[f] for f in FORMATS])
def test_a_stream_cut_at_consumed_is_the_uncut_stream(fmt):
    rng = np.random.default_rng(9 + fmt)
    n_fft, hop, avg = 64, 17, 3
    q, scale, _ = noise(rng, 2000, fmt)
    whole = sr.spectrum_format(q, fmt, scale, n_fft, hop, avg, sr.HANN, sr.SUM, 0.5)
    parts, pos = [], 0
    for end in (300, 301, 1200, 2000):
        r = sr.spectrum_format(q[pos:end], fmt, scale, n_fft, hop, avg, sr.HANN, sr.SUM, 0.5)
        parts.append(r)
        pos += sr.count(n_fft, hop, avg, end - pos)[1]
    got = np.concatenate(parts)
    assert got.shape == whole.shape and np.array_equal(got.view(np.uint32), whole.view(np.uint32))


def test_exponent_zero_is_not_multiplied():
    """an infinity in sample 0 of a rectangular segment: bins are inf or NaN by the butterflies alone; a multiply by
    T[0] = (1, 0) would turn the partner part into NaN (inf * 0) in every bin"""
    x = np.zeros((64, 2), np.float32)
    x[0, 0] = np.inf
    row = sr.spectrum(x, 64, 64, 1, sr.RECT)[0]
    assert np.isinf(row).all()


def test_fold_and_nan_sticks():
    rng = np.random.default_rng(10)
    rows = rng.random((6, 64)).astype(np.float32)
    rows[1, 5], rows[4, 7] = np.nan, np.inf
    for mode in (sr.SUM, sr.MAX):
        assert np.array_equal(sr.fold(rows, 1, mode).view(np.uint32), rows.view(np.uint32))
        two = sr.fold(rows, 2, mode)
        assert two.shape == (3, 64) and np.isnan(two[0, 5]) and np.isinf(two[2, 7])
        allr = sr.fold(rows, 6, mode)
        assert allr.shape == (1, 64) and np.isnan(allr[0, 5]) and np.isinf(allr[0, 7])
        ref = rows.astype(np.float64)
        want = ref.max(axis=0) if mode == sr.MAX else ref.sum(axis=0)
        ok = np.isfinite(want)
        assert np.allclose(allr[0][ok], want[ok], rtol=1e-6)
    assert sr.fold(rows, 4, sr.SUM).shape == (1, 64)


def test_band_sums_and_edges():
    rng = np.random.default_rng(11)
    rows = rng.random((3, 256)).astype(np.float32)
    edges = [(0, 1), (10, 73), (64, 128), (100, 165), (0, 256), (255, 256)]
    got = sr.bands(rows, edges)
    for b, (lo, hi) in enumerate(edges):
        want = rows[:, lo:hi].astype(np.float64).sum(axis=1)
        assert np.allclose(got[:, b], want, rtol=(hi - lo) * 2.0 ** -24 + 1e-7)
    assert np.array_equal(got[:, 0], rows[:, 0]) and np.array_equal(got[:, 5], rows[:, 255])
    # the scan's bands: 20 MHz at -25, 0 and +25 MHz of 80 MS/s in 256 bins; the lower edge belongs to the band, the upper does not
    assert sr.band(-25e6, 20e6, 80e6, 256) == (16, 80) and sr.band(0.0, 20e6, 80e6, 256) == (96, 160) and sr.band(25e6, 20e6, 80e6, 256) == (176, 240)
    assert sr.band(0.0, 80e6, 80e6, 64) == (0, 64)
    assert sr.band(35e6, 20e6, 80e6, 256) is None and sr.band(0.0, 1.0, 80e6, 64) == (32, 33) and sr.band(1e5, 1.0, 80e6, 64) is None
