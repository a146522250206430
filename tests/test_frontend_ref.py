"""The host restatement of NUMERICS.md rule 32 (tests/frontend_ref.py): its own properties, and the three scenes in which the
front end decides whether the oracle's stream receiver decodes anything."""
import numpy as np
import pytest

import frontend_ref as fr
import frontend_scene as sc

f32 = np.float32


def noise(n, seed, power=1.0):
    rng = np.random.default_rng(seed)
    return ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) * np.sqrt(power / 2)).astype(np.complex64)


def same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


@pytest.mark.parametrize("flags", [0, fr.FE_DC, fr.FE_IQ, fr.FE_DC | fr.FE_IQ])
def test_chunking_gives_the_bits_and_state_of_one_call(flags):
    x = fr.rx_impair(noise(40000, 1), *fr.imbalance(1.5, -7.0), 0.4 - 0.2j)
    z, st = fr.frontend(x, flags=flags)
    rng = np.random.default_rng(2)
    fe, parts, pos = fr.Frontend(flags=flags), [], 0
    while pos < x.size:
        k = int(rng.integers(1, 9001))
        parts.append(fe.process(x[pos:pos + k]))
        pos += k
    assert same_bits(np.concatenate(parts), z)
    assert fe.state().tobytes() == st.tobytes()
    assert int(st["n"]) == x.size and st["part"].any() and st["ring"][:9].any() and not st["ring"][9:].any()


def test_a_constant_representable_input_is_removed_exactly_from_block_1_on():
    c = np.complex64(0.75 - 3.5j)                       # multiples of 2^-12
    x = np.full(3 * fr.BLOCK + 100, c)
    z, st = fr.frontend(x, flags=fr.FE_DC | fr.FE_IQ)
    assert same_bits(z[:fr.BLOCK], x[:fr.BLOCK])        # the first block of a fresh state is uncorrected
    assert not z[fr.BLOCK:].view(np.float32).any()
    assert list(st["ring"][0]) == [3072, -14336, 3072 ** 2 + 14336 ** 2, 3072 ** 2 - 14336 ** 2, 2 * 3072 * -14336]


def test_w_estimates_the_image_of_a_known_imbalance():
    """circular Gaussian noise through (mu, nu): w lands within 5 / sqrt(N) of nu / conj(mu), N the samples of the window --
    16 blocks with the defaults, so 0.02"""
    mu, nu = fr.imbalance(2.0, 10.0)
    n_blocks = 16
    x = fr.rx_impair(noise(n_blocks * fr.BLOCK, 3), mu, nu, 0.3 + 0.1j)
    fe = fr.Frontend(flags=fr.FE_DC | fr.FE_IQ)
    fe.process(x)
    d, w = fe.estimate()
    bound = 5 / np.sqrt(n_blocks * fr.BLOCK)
    assert abs(bound - 0.02) < 5e-4
    assert abs(complex(w) - nu / np.conj(mu)) < bound
    # the offset: the mean of 4 blocks of samples of power |mu|^2 + |nu|^2; 5 sigma of that mean, plus two steps of the fixed point
    assert abs(complex(d) - (0.3 + 0.1j)) < 5 * np.sqrt((abs(mu) ** 2 + abs(nu) ** 2) / (4 * fr.BLOCK)) + 2.0 ** -11
    # corrected, the image of the NEXT samples is gone: z is proper again to within the same bound
    y = fr.rx_impair(noise(fr.BLOCK, 4), mu, nu, 0.3 + 0.1j)
    z = fe.process(y).astype(np.complex128)
    assert abs(np.mean(z * z) / np.mean(np.abs(z) ** 2)) < 2 * bound + 5 / np.sqrt(fr.BLOCK)


def test_clamp_nan_and_infinity():
    assert list(fr.fix(np.array([0.5, -0.5, 1.5, 2.5, np.nan, np.inf, -np.inf, 1e30, -1e30, 4095.99988], f32), 12)) == \
        [2048, -2048, 6144, 10240, 0, fr.CLAMP, -fr.CLAMP, fr.CLAMP, -fr.CLAMP, fr.CLAMP]
    assert list(fr.fix(np.array([0.5, 1.5, 2.5, -0.5], f32), 0)) == [0, 2, 2, 0]           # ties to even
    assert list(fr.fix(np.array([3.0e38, 7.0], f32), 30)) == [fr.CLAMP, fr.CLAMP]          # the product overflows / exceeds the clamp
    x = np.zeros(2 * fr.BLOCK, np.complex64)
    x[5] = np.nan + 1j * np.inf
    x[6] = -np.inf
    z, st = fr.frontend(x, flags=fr.FE_DC)
    assert list(st["ring"][0][:2]) == [-fr.CLAMP >> 12, fr.CLAMP >> 12]                    # NaN counted as 0, the infinities clamped
    # an infinite sample leaves as NaN (inf x 0 in the image term, which is always computed); its neighbours are untouched
    assert np.isnan(z[5].real) and np.isnan(z[5].imag) and np.isnan(z[6].real)
    assert not z[:5].view(np.float32).any() and not z[7:fr.BLOCK].view(np.float32).any()
    # block 1 is corrected with block 0's means: (-(2^24 - 1) >> 12, (2^24 - 1) >> 12) = (-4096, 4095) in Q12
    assert same_bits(z[fr.BLOCK:], np.full(fr.BLOCK, np.complex64(1.0 - 4095 / 4096 * 1j)))
    # full-scale statistics stay inside int64 and give no image coefficient out of range
    big, _ = fr.frontend(np.full(2 * fr.BLOCK, 1e30 + 1e30j, np.complex64), flags=fr.FE_DC | fr.FE_IQ)
    assert np.isfinite(big[fr.BLOCK:]).all()


def test_ring_wraps_beyond_64_blocks():
    x = fr.rx_impair(noise(70 * fr.BLOCK + 5, 5), 1.0, 0.05j, 0.0)
    x += (np.arange(x.size) // fr.BLOCK).astype(np.float32) * f32(0.125)                   # a drifting offset: every block differs
    z, st = fr.frontend(x, flags=fr.FE_DC, dc_shift=6, iq_shift=6)
    for b in (6, 63, 64, 69):                            # blocks 64 .. 69 overwrote slots 0 .. 5
        u = fr.fix(x[b * fr.BLOCK:(b + 1) * fr.BLOCK].real, 12)
        assert int(st["ring"][b % 64][0]) == int(u.sum()) >> 12
    # block 70 is corrected with the mean over blocks 6 .. 69
    v = fr.widen(x)
    m = [sum(int(fr.fix(v[b * fr.BLOCK:(b + 1) * fr.BLOCK, i], 12).sum()) >> 12 for b in range(6, 70)) >> 6 for i in (0, 1)]
    d = np.array([f32(m[0] * 2.0 ** -12), f32(m[1] * 2.0 ** -12)])
    assert same_bits(z[70 * fr.BLOCK:], (v[70 * fr.BLOCK:] - d).copy().view(np.complex64).reshape(-1))


def test_windows_grow_with_the_stream():
    assert [fr.window_shift(2, b) for b in (1, 2, 3, 4, 5, 100)] == [0, 1, 1, 2, 2, 2]
    assert [fr.window_shift(6, b) for b in (1, 63, 64, 1 << 40)] == [0, 5, 6, 6]
    assert fr.window_shift(0, 9) == 0


def test_initial_values_in_block_0():
    st0 = np.zeros((), fr.STATE_DTYPE)
    st0["d0"], st0["w0"] = [2048, -4096], [0.05, -0.02]
    x = noise(fr.BLOCK + 10, 6)
    v = fr.widen(x)
    for flags in (0, fr.FE_DC, fr.FE_IQ, fr.FE_DC | fr.FE_IQ):
        z = fr.Frontend(flags=flags, state=st0).process(x)
        d = [f32(0.5), f32(-1.0)] if flags & fr.FE_DC else [f32(0), f32(0)]
        w = [f32(0.05), f32(-0.02)] if flags & fr.FE_IQ else [f32(0), f32(0)]
        assert same_bits(z[:fr.BLOCK], fr.apply(v[:fr.BLOCK], d, w).view(np.complex64).reshape(-1))
    fe = fr.Frontend(flags=3, state=st0)
    assert fe.estimate() == (np.complex64(0.5 - 1j), np.complex64(complex(f32(0.05), f32(-0.02))))
    fe.process(x)
    assert list(fe.state()["d0"]) == [2048, -4096] and same_bits(fe.state()["w0"], st0["w0"])      # carried, not consumed


def test_rx_impair_restatement():
    x = noise(1000, 7)
    assert same_bits(fr.rx_impair(x), x + np.complex64(0))                     # mu = 1, nu = 0, dc = 0
    mu, nu = fr.imbalance(1.0, 5.0)
    got = fr.rx_impair(x, mu, nu, 0.25 - 0.5j).astype(np.complex128)
    want = mu * x.astype(np.complex128) + nu * np.conj(x.astype(np.complex128)) + (0.25 - 0.5j)
    assert np.abs(got - want).max() < 8 * 2.0 ** -24 * np.abs(want).max()
    assert fr.imbalance() == (1 + 0j, 0j)


# ---- the scenes (conditions of the issue that introduced rule 32; checked on this restatement) ----

@pytest.fixture(scope="module")
def scene_counts(orc):
    """per scene and arm (off / dc / dc+iq): the late slots that decode, of the scene's late slots"""
    out = {}
    for name in sc.SCENES:
        x, psdus, slot_len = sc.build(name)
        late = set(sc.late_slots(slot_len))
        arms = {"off": x, "dc": fr.frontend(x, flags=fr.FE_DC)[0], "dc+iq": fr.frontend(x, flags=fr.FE_DC | fr.FE_IQ)[0]}
        out[name] = ({arm: sc.oracle_good(orc, z, psdus, slot_len)[0] & late for arm, z in arms.items()}, late)
    return out


def test_scene_a_a_dc_offset_ends_reception_and_the_dc_stage_brings_it_back(scene_counts):
    good, late = scene_counts["a"]
    assert len(late) == 21
    assert len(good["off"]) <= 2
    assert good["dc"] == late


def test_scene_b_64qam_needs_the_iq_stage(scene_counts):
    good, late = scene_counts["b"]
    assert len(late) == 19
    assert len(late) - len(good["dc"]) >= 4
    assert good["dc+iq"] == late


def test_scene_c_the_front_end_loses_no_frame_of_a_clean_stream(scene_counts):
    good, late = scene_counts["c"]
    assert good["off"] <= good["dc"] and good["off"] <= good["dc+iq"]
    assert good["off"] == late
