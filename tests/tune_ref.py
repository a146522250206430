"""NUMERICS.md rule 35 in NumPy float32: the tuner of wifirx_tune.  Channel k of a capture is the capture multiplied by rule 17's
fixed-point phase ramp at the STREAM index of every sample, then resampled by rule 34 -- so this module is channel_ref's
angle(), the oracle's sincos (rule 1) and arb_ref.resample, and nothing else.

Samples are float32 pairs [n, 2] as in arb_ref; a call returns float32 pairs [K, n_out, 2].  Increments and phases are Python
integers mod 2^64 (2^-64 turns).

`mutant` names ONE deliberate mistake (MUTANTS); tests/test_tune_ref.py asserts which test catches each."""
import math

import numpy as np

import arb_ref as ar
import channel_ref as chr_
import convert_ref as cr
from oracle import oracle as orc

F32 = np.float32
M64 = (1 << 64) - 1
MAX_CHANNELS = 8
MUTANTS = ("conjugate", "call_index", "no_phase0", "rotate_output", "raw_zeros")


def tune_inc(offset_hz, sample_rate) -> int:
    """wifirx_tune_inc: t = offset_hz / sample_rate reduced to [-1/2, 1/2] by its nearest integer, (uint64)(-llround(t 2^64)),
    +-1/2 turn = 2^63"""
    t = float(offset_hz) / float(sample_rate)
    t -= float(np.rint(t))
    v = t * 2.0 ** 64
    if v >= 2.0 ** 63 or v <= -2.0 ** 63:
        return 1 << 63
    a = abs(v)
    k = int(a) if a >= 2.0 ** 52 else math.floor(a + 0.5)      # llround: half away from zero (a + 0.5 is exact below 2^52)
    return (k if v < 0 else -k) & M64


def phases(inc, phase0, j_first, n):
    """P(j) = phase0 + inc j mod 2^64 for the stream indices j_first .. j_first + n - 1 (j_first may be negative: it wraps)"""
    idx = np.arange(n, dtype=np.uint64)
    with np.errstate(over="ignore"):
        return np.uint64((int(phase0) + int(inc) * int(j_first)) & M64) + np.uint64(int(inc) & M64) * idx


def rotate(x, inc, phase0, j_first, mutant=None):
    """x: float32 pairs [n, 2], x[0] at stream index j_first -> x * exp(j 2 pi P / 2^64) in rule 17's float32: the angle from
    the top 32 bits of P, sine and cosine by rule 1, four products, one subtract and one add"""
    x = np.asarray(x, dtype=F32).reshape(-1, 2)
    sn, cs = orc.sincos(chr_.angle(phases(inc, 0 if mutant == "no_phase0" else phase0, j_first, len(x))))
    if mutant == "conjugate":
        sn = -sn
    with np.errstate(invalid="ignore", over="ignore"):
        yr = x[:, 0] * cs - x[:, 1] * sn
        yi = x[:, 0] * sn + x[:, 1] * cs
    assert yr.dtype == F32 and yi.dtype == F32
    return np.stack([yr, yi], axis=1)


def is_centre(inc, phase0):
    """the channel that is not rotated at all"""
    return (int(inc) & M64) == 0 and (int(phase0) & M64) == 0


def tune(x, num, den, incs, phase0s=None, hist=None, j0=0, m0=0, mutant=None):
    """one call: x float32 pairs [n_in, 2] with in[0] at stream index j0, hist the HL RAW samples in front (None: zeros) ->
    float32 pairs [K, n_out, 2], the outputs m0 .. m_end(j0 + n_in) - 1 of every channel.

    Channel k is arb_ref.resample of the rotated (hist || x); the rotated zeros of a NULL history are passed as its hist.
    Samples in front of the stream are zeros whatever hist holds there, and they are rotated too: arb_ref.resample writes
    plain zeros at stream indices below 0, so it is called k num inputs and k den outputs further into the stream -- the
    same phase of the ratio, hence the same coefficients -- where no index is negative."""
    num, den = ar.reduce(num, den)
    HL = ar.hist_len(num, den)
    incs = [int(v) & M64 for v in incs]
    assert 1 <= len(incs) <= MAX_CHANNELS
    phase0s = [0] * len(incs) if phase0s is None else [int(v) & M64 for v in phase0s]
    assert len(phase0s) == len(incs)
    j0, m0 = int(j0), int(m0)
    xx = ar.history(x, hist, HL).copy()                       # xx[i] is stream sample j0 - HL + i
    first = j0 - HL
    if first < 0:
        xx[:min(-first, len(xx))] = 0
    shift = max(0, -(first // num))
    rows = []
    for inc, ph in zip(incs, phase0s):
        if is_centre(inc, ph):
            rows.append(ar.resample(x, num, den, hist, j0, m0))
            continue
        if mutant == "rotate_output":
            y = ar.resample(x, num, den, hist, j0, m0)
            ms = m0 + np.arange(len(y))
            sn, cs = orc.sincos(chr_.angle(np.array([(ph + inc * ((int(m) * num) // den)) & M64 for m in ms], dtype=np.uint64)))
            rows.append(np.stack([y[:, 0] * cs - y[:, 1] * sn, y[:, 0] * sn + y[:, 1] * cs], axis=1).astype(F32))
            continue
        r = rotate(xx, inc, ph, 0 if mutant == "call_index" else first, mutant)
        if mutant == "raw_zeros" and hist is None:
            r[:HL] = 0
        rows.append(ar.resample(r[HL:], num, den, r[:HL], j0 + shift * num, m0 + shift * den))
    return np.stack(rows)


def tune_format(q, fmt, scale, num, den, incs, phase0s=None, hist=None, j0=0, m0=0):
    """the same on samples of a format: integers [n, 2] are widened by rule 20 first (and so is hist), fc32 passes through"""
    if fmt == cr.FC32:
        return tune(q, num, den, incs, phase0s, hist, j0, m0)
    return tune(cr.widen(q, scale), num, den, incs, phase0s, None if hist is None else cr.widen(hist, scale), j0, m0)


def stream(x, num, den, incs, phase0s=None, n_out=None, mutant=None):
    """a whole stream from j0 = m0 = 0 on complex samples: complex64 [K, n_out]; with n_out given, zeros are pushed behind x
    until that many outputs exist (the end-of-stream flush)"""
    x = np.asarray(x, dtype=np.complex64).reshape(-1)
    if n_out is not None:
        x = np.concatenate([x, np.zeros(ar.flush_inputs(num, den, len(x), n_out), np.complex64)])
    y = tune(cr.pairs(x), num, den, incs, phase0s, mutant=mutant)
    y = np.stack([cr.to_complex(row) for row in y])
    return y if n_out is None else y[:, :n_out]


def direct(x, num, den, inc, phase0=0, outputs=None):
    """the definition in float64: the exact exp(j 2 pi P(j) / 2^64), P in exact integers, times x, through arb_ref.direct();
    x complex from the start of a stream -> complex128"""
    x = np.asarray(x, dtype=np.complex128).reshape(-1)
    turns = np.array([((int(phase0) + int(inc) * j) & M64) / 2.0 ** 64 for j in range(len(x))])
    return ar.direct(x * np.exp(2j * np.pi * turns), num, den, outputs)


SCENE_RATE, SCENE_OFFSETS = 80e6, (-25e6, 0.0, 25e6)


def three_channel_scene(enc, plen, snr_db, n_frames=8, db_up=0.0):
    """channels 1 / 6 / 11 in one 80 MS/s capture: per channel k its own n_frames frames (lead 160, tail 240), rolled by 100 k
    samples, `snr_db` above unit noise per channel bandwidth (the outer two `db_up` dB more), taken up 1/4 by rule 34 and
    mixed to -25 / 0 / +25 MHz in float64; complex noise of variance 4 per sample on the sum.
    -> (complex64 capture, [psdus of channel k], n_sym)"""
    from wifirx import txgen
    wide, psdus, n_sym = 0.0, [], 0
    for k, off in enumerate(SCENE_OFFSETS):
        p = txgen.make_psdus(n_frames, plen, seed=80 + k)
        tx = txgen.encode_psdus(p, enc)
        row = np.zeros((n_frames, 160 + tx.samples.shape[1] + 240), np.complex128)
        row[:, 160:160 + tx.samples.shape[1]] = tx.samples
        v = np.roll(row.reshape(-1), 100 * k) * math.sqrt(10 ** ((snr_db + (0.0 if k == 1 else db_up)) / 10))
        up = ar.stream(v, 1, 4, n_out=4 * len(v)).astype(np.complex128)
        j = np.arange(len(up))
        wide = wide + up * np.exp(2j * np.pi * ((j * round(off / SCENE_RATE * 16)) % 16) / 16.0)      # +-5/16 turn per sample
        psdus.append(p)
        n_sym = tx.n_sym
    rng = np.random.default_rng(81)
    wide = wide + (rng.standard_normal(len(wide)) + 1j * rng.standard_normal(len(wide))) * math.sqrt(2.0)
    return wide.astype(np.complex64), psdus, n_sym


def scene_incs():
    return [tune_inc(off, SCENE_RATE) for off in SCENE_OFFSETS]


SINCOS_ERR = 3e-7                                           # rule 1's stated bound on sp_sincos


def error_bound(num, den, max_component):
    """the rule's bound on |restatement - direct()| per component.  A = max|component| of x.  The angle: the top 32 bits of P
    drop at most 2^-32 turn (2 pi 2^-32), the conversion to float32 rounds an |angle| <= pi (pi 2^-24), the constant
    2 pi / 2^32 is a rounded float32 and so is the product (pi 2^-24 each): e_a = pi (3 * 2^-24 + 2^-31).  Sine and cosine
    are then off by e_a + 3e-7 (rule 1).  A rotated component x.re cs - x.im sn is off by (|x.re| + |x.im|) (e_a + 3e-7) <=
    2 A (e_a + 3e-7) plus the roundings of two products below A and of a sum below 2 A: 4 A 2^-24.  That error passes
    through g sum|c|, and rule 34's own bound holds on top for rotated components, which are below sqrt(2) A."""
    num, den = ar.reduce(num, den)
    S = max(num, den)
    g = den / float(S) if num > den else 1.0
    e_a = math.pi * (3 * 2.0 ** -24 + 2.0 ** -31)
    e_rot = max_component * (2 * (e_a + SINCOS_ERR) + 4 * 2.0 ** -24)
    return g * ar.coefficient_sum(num, den) * e_rot + ar.error_bound(num, den, math.sqrt(2.0) * max_component)
