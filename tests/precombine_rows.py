"""Host-built sample rows that meet every clause of NUMERICS.md rule 33 (tests/precombine_ref.py), for the reference's own tests
and for the kernel's bit-for-bit comparison (tests/test_gpu_precombine.py).

    build(case, n_ant, slot_len, n_slots, seed=0) -> list of n_ant complex64 arrays [n_slots, slot_len]

Every case is defined for every n_ant from 1 to 8; where a case names "antenna 1" or "a later antenna" and there is only
one, it falls on antenna 0."""
import numpy as np

CASES = ("scene", "identical", "zero_antenna", "zero_slot", "tie", "nan_first", "nan_later", "inf", "known_gain")

# exact in float32 arithmetic: a product with one of these changes the exponent, swaps the parts or flips signs, nothing else.
# The strongest of the first n_ant is unique: antenna 3 (|g| = 2) from four antennas on, antenna 1 below that
KNOWN_GAINS = np.array([0.5, 1j, -0.25, -2j, 1.0, 0.5j, -1.0, 0.125], np.complex128)


def noise(rng, shape, scale=1.0):
    return ((rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) * (scale / np.sqrt(2))).astype(np.complex64)


def scene(rng, n_ant, slot_len, n_slots, noise_scale=0.3):
    """one common unit-power signal through one random complex gain per slot and antenna, plus independent noise"""
    s = noise(rng, (n_slots, slot_len))
    g = noise(rng, (n_slots, n_ant, 1))
    return [(g[:, a] * s + noise(rng, (n_slots, slot_len), noise_scale)).astype(np.complex64) for a in range(n_ant)], g[:, :, 0]


def build(case, n_ant, slot_len, n_slots, seed=0):
    rng = np.random.default_rng([seed, CASES.index(case), n_ant, slot_len])
    xs, _ = scene(rng, n_ant, slot_len, n_slots)
    last = n_ant - 1
    if case == "identical":
        xs = [xs[0].copy() for _ in range(n_ant)]
    elif case == "zero_antenna":
        xs[min(1, last)][:] = 0
    elif case == "zero_slot":                   # degenerate: the trace is 0
        for x in xs:
            x[0] = 0
    elif case == "tie":                         # conj() keeps every |x|^2 bit for bit: the two strongest antennas tie
        hi = max(last - 1, 0)
        power = lambda x: (np.abs(x.astype(np.complex128)) ** 2).sum(axis=1, keepdims=True)
        for a in range(hi):                     # every other antenna at a quarter of their power, slot by slot
            xs[a] = (xs[a] * (0.5 * np.sqrt(power(xs[hi]) / power(xs[a])))).astype(np.complex64)
        xs[last] = np.conj(xs[hi])
    elif case == "nan_first":
        xs[0][0, slot_len // 3] = complex(np.nan, 1.0)
    elif case == "nan_later":
        xs[last][0, slot_len - 1] = complex(0.5, np.nan)
    elif case == "inf":
        xs[min(1, last)][0, 5] = complex(np.inf, 0.0)
        xs[0][n_slots - 1, 63] = complex(1.0, -np.inf)
    elif case == "known_gain":
        s = noise(rng, (n_slots, slot_len))
        xs = [(s * np.complex64(KNOWN_GAINS[a])).astype(np.complex64) for a in range(n_ant)]
    return xs


def known_gain_weights(n_ant):
    """what rule 33 must find for "known_gain": g / |g|, rotated so that the strongest antenna's weight is real and >= 0"""
    g = KNOWN_GAINS[:n_ant]
    r = int(np.argmax(np.abs(g)))
    return g * np.exp(-1j * np.angle(g[r])) / np.linalg.norm(g), r


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b))


def same_values(a, b):
    """bit for bit, except that any NaN equals any NaN (which NaN an invalid operation gives is not part of the rule)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype.names:
        return all(same_values(a[k], b[k]) for k in a.dtype.names)
    if a.dtype.kind == "c":
        return same_values(a.real, b.real) and same_values(a.imag, b.imag)
    if a.dtype.kind != "f":
        return np.array_equal(a, b)
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(bits(a[~nan]), bits(b[~nan]))
