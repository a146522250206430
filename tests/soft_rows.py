"""Frame records and LLR rows made on the host, for the soft-decision decode_mac (NUMERICS.md rule 14).

Test infrastructure only, and nothing of the oracle: `wifirx_decode_batch_soft` reads caller-owned buffers, so a test can
write the records a demodulation would leave and any LLR rows it likes, and compare the device with
`soft_viterbi_ref.decode_batch` bit for bit.  This module makes

* `records`: FRAME_DTYPE records of complete frames (per-frame rate, length and flags);
* coherent rows: the signs of real coded frames (`txgen.encode_psdus` -> `soft_viterbi_ref.pm1_llrs`);
* the value classes (`CLASSES`): what the +-1 rows are multiplied with / replaced by;
* `SPECS`: the one table of batches that tests/test_soft_rows.py (CPU, reference alone) and tests/test_gpu_soft_rows.py
  (device against reference) both run, and `check_conditions`, the properties that keep each batch from passing
  vacuously.
"""
from __future__ import annotations

import functools
import zlib
from dataclasses import dataclass, field

import numpy as np

import soft_viterbi_ref as ref
from llr_bf16_ref import bf16_rne, bf16_to_f32
from wifirx import txgen

FRAME_DTYPE = np.dtype([
    ("flags", "<u4"), ("trigger", "<i4"), ("frame_start", "<i4"),
    ("cfo_coarse", "<f4"), ("cfo_fine", "<f4"), ("snr_db", "<f4"),
    ("psdu_len", "<u2"), ("encoding", "u1"), ("n_bpsc", "u1"),
    ("n_sym", "<u2"), ("n_sym_out", "<u2"),
])          # wifirx.capi.FRAME_DTYPE (tests/test_soft_rows.py checks that the two are the same)
F_DETECTED, F_SYNC, F_SIGNAL = 1, 2, 4
F_FULL = F_DETECTED | F_SYNC | F_SIGNAL | ref.F_COMPLETE | ref.F_LLR          # a complete frame with LLRs
FORMATS = ("f32", "bf16")
F32_MAX = float(np.finfo(np.float32).max)
BF16_MAX = float(bf16_to_f32(np.uint16(0x7F7F)))
FILL = 0xA5                                  # what the GPU tests fill the PSDU buffer and its fences with


def records(enc, psdu_len, flags=F_FULL) -> np.ndarray:
    """Records as a demodulation leaves them for complete frames: DETECTED | SYNC | SIGNAL | COMPLETE | LLR, the rate's
    n_bpsc, n_sym = n_sym_out = the symbols of a PSDU of psdu_len bytes.  enc, psdu_len, flags: scalars or [n]."""
    enc, psdu_len, flags = np.broadcast_arrays(np.atleast_1d(enc), np.atleast_1d(psdu_len), np.atleast_1d(flags))
    n = enc.shape[0]
    r = np.zeros(n, dtype=FRAME_DTYPE)
    r["flags"] = flags
    r["trigger"] = 160 + 7 * np.arange(n)
    r["frame_start"] = r["trigger"] + 161
    r["snr_db"] = 20.0
    r["psdu_len"] = psdu_len
    r["encoding"] = enc
    r["n_bpsc"] = np.array(ref.N_BPSC)[enc]
    nd = np.array(ref.N_DBPS)[enc]
    r["n_sym"] = r["n_sym_out"] = (16 + 8 * psdu_len.astype(np.int64) + 6 + nd - 1) // nd
    return r


def make_psdu(n: int, ln: int, rng) -> np.ndarray:
    """[n][ln] random bytes, the last four the CRC-32 of the others when there is room for one (ln >= 4)"""
    p = rng.integers(0, 256, size=(n, ln), dtype=np.uint8)
    if ln >= 4:
        for k in range(n):
            p[k, ln - 4:] = np.frombuffer(zlib.crc32(p[k, :ln - 4].tobytes()).to_bytes(4, "little"), np.uint8)
    return p


def coherent(recs: np.ndarray, max_sym: int, llr_bits: int, seed: int):
    """+-1 rows in the demod's layout that carry the coded bits of real frames, one per record whose symbols fit
    max_sym and whose rate fits llr_bits (the other rows stay 0), and the transmitted PSDUs (list, None for those)."""
    rng = np.random.default_rng(seed)
    n = recs.shape[0]
    idx = np.zeros((n, max_sym, 48), np.uint8)
    psdus = [None] * n
    enc, ln = recs["encoding"].astype(np.int64), recs["psdu_len"].astype(np.int64)
    for e, l in sorted(set(zip(enc.tolist(), ln.tolist()))):
        n_sym = ref.n_sym_of(e, l)
        if n_sym > max_sym or ref.N_BPSC[e] > llr_bits or l > 4095:
            continue
        g = np.nonzero((enc == e) & (ln == l))[0]
        p = make_psdu(g.size, l, rng)
        tx = txgen.encode_psdus(p, e, seeds=rng.integers(1, 128, g.size))
        idx[g, :n_sym] = tx.data_idx
        for j, k in enumerate(g):
            psdus[k] = p[j]
    with_llr = recs.copy()
    with_llr["flags"] |= ref.F_LLR
    signs = ref.pm1_llrs(with_llr, idx, max_sym, llr_bits)
    for k in range(n):
        if psdus[k] is None:
            signs[k] = 0
    return signs, psdus


def extent(recs: np.ndarray) -> np.ndarray:
    """values of a frame's row that the decoder reads: n_sym * 48 * n_bpsc"""
    return recs["n_sym"].astype(np.int64) * 48 * recs["n_bpsc"]


# ---- value classes: (signs [n][W], records, rng, fmt) -> float32 rows, or uint16 bf16 patterns where a class makes them ----

NOISE_SIGMA = (0.84, 0.62, 0.84, 0.62, 0.84, 0.62, 0.68, 0.62)      # per rate, on unit LLRs: CRC_OK neither always nor never
WIDE_FLIP = 0.0015                                                    # sign flips of `wide` (tuned on the reference)
HUGE_FLIP = 0.10


def _sigma_rows(recs):
    return np.array(NOISE_SIGMA, np.float32)[recs["encoding"].astype(np.int64) & 7][:, None]


def v_noisy(signs, recs, rng, fmt, scale=1.0):
    return (signs + np.float32(scale) * _sigma_rows(recs) * rng.standard_normal(signs.shape, dtype=np.float32)).astype(np.float32)


def v_mild(signs, recs, rng, fmt):
    """coherent with noise that leaves every frame decodable (the geometry batches: what matters there is where bytes land)"""
    return v_noisy(signs, recs, rng, fmt, scale=0.45)


def _planted(recs, rng, n_kinds):
    """per frame and kind one position inside the frame's extent (distinct positions)"""
    ext = np.maximum(extent(recs), n_kinds)
    return np.stack([rng.permutation(int(e))[:n_kinds] for e in ext])


def v_nonfinite(signs, recs, rng, fmt):
    x = v_noisy(signs, recs, rng, fmt)
    hit = rng.random(x.shape) < 0.02
    rows = np.arange(x.shape[0])[:, None]
    if fmt == "bf16":
        kinds = np.array([0x7FC0, 0x7F80, 0xFF80, 0xFFC1], np.uint16)
        b = np.where(hit, rng.choice(kinds, size=x.shape), bf16_rne(x)).astype(np.uint16)
        b[rows, _planted(recs, rng, 4)] = kinds[None, :]
        return b
    kinds = np.array([np.nan, np.inf, -np.inf], np.float32)
    x = np.where(hit, rng.choice(kinds, size=x.shape), x).astype(np.float32)
    x[rows, _planted(recs, rng, 3)] = kinds[None, :]
    return x


def v_zeros(signs, recs, rng, fmt):
    return np.zeros_like(signs)


def v_negzero(signs, recs, rng, fmt):
    return np.where(rng.random(signs.shape) < 0.5, np.float32(-0.0), np.float32(0.0)).astype(np.float32)


def v_const_coherent(signs, recs, rng, fmt):
    return (signs * np.float32(0.375)).astype(np.float32)


def v_const_random(signs, recs, rng, fmt):
    return np.where(rng.random(signs.shape) < 0.5, np.float32(-0.375), np.float32(0.375)).astype(np.float32)


def v_subnormal(signs, recs, rng, fmt):
    """coherent signs, magnitudes log-uniform over the format's subnormal range (float32: 2^-149 .. 2^-126, 23 mantissa
    bits; bf16: 2^-133 .. 2^-126, 7 bits), made as bit patterns so that nothing rounds"""
    bits = 7 if fmt == "bf16" else 23
    m = np.floor(np.exp2(rng.uniform(0, bits, signs.shape))).astype(np.uint32)
    m = np.clip(m, 1, (1 << bits) - 1) << (16 if fmt == "bf16" else 0)
    x = m.view(np.float32)
    assert (x > 0).all() and (x < np.finfo(np.float32).tiny).all()
    return (np.sign(signs) * x).astype(np.float32)


def v_wide(signs, recs, rng, fmt):
    flip = np.where(rng.random(signs.shape) < WIDE_FLIP, np.float32(-1), np.float32(1))
    mag = np.power(10.0, rng.uniform(-30, 30, signs.shape)).astype(np.float32)
    return (signs * flip * mag).astype(np.float32)


def v_huge(signs, recs, rng, fmt):
    """coherent signs with a tenth flipped; one scale per frame, log-uniform from 1e36 to the largest finite value, every
    value within a factor two below it: frames at the top overflow all 64 metrics between two normalisations, frames
    at the bottom never do"""
    top = BF16_MAX if fmt == "bf16" else F32_MAX
    flip = np.where(rng.random(signs.shape) < HUGE_FLIP, np.float32(-1), np.float32(1))
    scale = np.power(10.0, rng.uniform(36.0, np.log10(top), (signs.shape[0], 1)))
    mag = np.minimum(scale * rng.uniform(0.5, 1.0, signs.shape), top * (1 - 2.0 ** -8)).astype(np.float32)
    return (signs * flip * mag).astype(np.float32)


CLASSES = {"noisy": v_noisy, "mild": v_mild, "nonfinite": v_nonfinite, "zeros": v_zeros, "negzero": v_negzero,
           "const_coherent": v_const_coherent, "const_random": v_const_random, "subnormal": v_subnormal, "wide": v_wide,
           "huge": v_huge}
VALUE_CLASSES = ("noisy", "nonfinite", "zeros", "negzero", "const_coherent", "const_random", "subnormal", "wide", "huge")


# ---- batch layouts: () -> (enc [n], psdu_len [n], flags [n]) ----

def pad2_lengths(enc: int, lo: int, count: int):
    """the first `count` PSDU lengths >= lo whose frame at rate enc ends two bits short of its last symbol (the smallest
    pad there is: 22 + 8 L is 2 mod 4 and every N_DBPS is a multiple of 4)"""
    nd = ref.N_DBPS[enc]
    out = [l for l in range(lo, lo + 4 * nd) if (22 + 8 * l) % nd == nd - 2]
    return out[:count]


def lay_values(n=320, lens=(30, 45, 64)):
    k = np.arange(n)
    return k % 8, np.array(lens)[(k // 8) % len(lens)], np.full(n, F_FULL)


def lay_pad2(n=320):
    k = np.arange(n)
    enc = k % 8
    lens = np.array([pad2_lengths(e, 24, 3) for e in range(8)])
    return enc, lens[enc, (k // 8) % 3], np.full(n, F_FULL)


def lay_short():
    """psdu_len 0 .. 8 at a rate of every bits-per-carrier class (and both puncturings), four frames each"""
    enc, ln = np.meshgrid(np.array([1, 2, 5, 6]), np.array([0, 1, 2, 3, 4, 5, 7, 8]), indexing="ij")
    enc, ln = np.repeat(enc.reshape(-1), 4), np.repeat(ln.reshape(-1), 4)
    return enc, ln, np.full(enc.size, F_FULL)


def lay_long(enc):
    """64 frames of the longest PSDU at one rate and, in the middle, one that is a byte longer (left alone)"""
    ln = np.full(65, ref.MAX_PSDU)
    ln[31] = ref.MAX_PSDU + 1
    return np.full(65, enc), ln, np.full(65, F_FULL)


MAXSYM_EDGE = 12          # max_sym of the `maxsym` batch


def lay_maxsym():
    """per rate the longest PSDU of MAXSYM_EDGE symbols, and one byte more (MAXSYM_EDGE + 1 symbols: left alone)"""
    k = np.arange(96)
    enc = k % 8
    fit = np.array([(MAXSYM_EDGE * ref.N_DBPS[e] - 22) // 8 for e in range(8)])
    return enc, fit[enc] + (k // 8) % 2, np.full(k.size, F_FULL)


STRIDE_EDGE = 45          # psdu_stride of the `stride` batch: odd


def lay_stride():
    """psdu_len == psdu_stride, psdu_stride + 1 (left alone) and something shorter, all rates"""
    k = np.arange(120)
    return k % 8, np.array([STRIDE_EDGE, STRIDE_EDGE + 1, 17])[(k // 8) % 3], np.full(k.size, F_FULL)


def lay_n(n):
    k = np.arange(n)
    return (k * 5 + 3) % 8, np.array([10, 14, 21])[(k // 8) % 3], np.full(n, F_FULL)


def lay_blocked_head():
    """200 records; the first 64 -- so the first of every rate, and every lane of the first task's slots -- are not
    decodable: COMPLETE cleared, LLR cleared (these still take lanes: the pre-pass counts them), PSDU longer than the row"""
    k = np.arange(200)
    enc, ln, fl = k % 8, np.array([12, 19, 26])[(k // 8) % 3].copy(), np.full(k.size, F_FULL)
    head = k < 64
    kind = (k // 8) % 3
    fl[head & (kind == 0)] &= ~ref.F_COMPLETE
    fl[head & (kind == 1)] &= ~ref.F_LLR
    ln[head & (kind == 2)] = 200          # > psdu_stride of the spec (64)
    return enc, ln, fl


def lay_one_rate(enc, n=100):
    k = np.arange(n)
    return np.full(n, enc), np.array([11, 23, 16])[k % 3], np.full(n, F_FULL)


def lay_second_rates(n=140):
    """only the second rate of every bits-per-carrier class"""
    k = np.arange(n)
    return 2 * (k % 4) + 1, np.array([11, 23, 16])[(k // 4) % 3], np.full(n, F_FULL)


def lay_tasks(n=800, lens=(9, 13, 18)):
    """100 frames per rate: two tasks of each rate, sixteen in all, four per bits-per-carrier class"""
    return lay_values(n, lens)


@dataclass(frozen=True)
class Spec:
    name: str
    cls: str
    layout: tuple                 # (function, args)
    max_sym: int
    llr_bits: int = 6
    psdu_stride: int = 64
    seed: int = 1
    checks: tuple = ()            # names of the extra conditions of check_conditions


def _specs():
    s = []
    for i, c in enumerate(VALUE_CLASSES):
        lay = (lay_pad2, ()) if c == "const_random" else (lay_values, ())
        s.append(Spec("values_" + c, c, lay, max_sym=ref.n_sym_of(0, 68), seed=100 + i, psdu_stride=96, checks=(c,)))
    s.append(Spec("short", "mild", (lay_short, ()), max_sym=4, seed=201, psdu_stride=16, checks=("all_crc_from_4",)))
    for e in range(8):
        s.append(Spec("long_%d" % e, "mild", (lay_long, (e,)), max_sym=511, llr_bits=ref.N_BPSC[e], psdu_stride=1536,
                      seed=210 + e, checks=("at_max_sym",) if e == 0 else ()))
    s.append(Spec("maxsym", "mild", (lay_maxsym, ()), max_sym=MAXSYM_EDGE, seed=221, psdu_stride=330, checks=("all_crc_from_4",)))
    s.append(Spec("stride", "mild", (lay_stride, ()), max_sym=ref.n_sym_of(0, STRIDE_EDGE), seed=222, psdu_stride=STRIDE_EDGE))
    for n in (1, 63, 64, 65, 129, 1040):
        s.append(Spec("n_%d" % n, "noisy", (lay_n, (n,)), max_sym=ref.n_sym_of(0, 21), seed=230 + n % 17, psdu_stride=24))
    s.append(Spec("blocked_head", "noisy", (lay_blocked_head, ()), max_sym=ref.n_sym_of(0, 26), seed=241))
    s.append(Spec("one_rate_3", "noisy", (lay_one_rate, (3,)), max_sym=ref.n_sym_of(3, 23), llr_bits=2, seed=242, psdu_stride=24))
    s.append(Spec("one_rate_6", "noisy", (lay_one_rate, (6,)), max_sym=ref.n_sym_of(6, 23), seed=243, psdu_stride=24))
    s.append(Spec("second_rates", "noisy", (lay_second_rates, ()), max_sym=ref.n_sym_of(1, 23), seed=244, psdu_stride=24))
    for lb in (1, 2, 4, 6):
        s.append(Spec("llr_bits_%d" % lb, "noisy", (lay_values, (160, (12, 20, 31))), max_sym=ref.n_sym_of(0, 31), llr_bits=lb,
                      seed=250 + lb, psdu_stride=32, checks=("narrow_rows",) if lb < 6 else ()))
    for c in ("noisy", "nonfinite", "huge"):
        s.append(Spec("tasks_" + c, c, (lay_tasks, ()), max_sym=ref.n_sym_of(0, 18), seed=260 + len(c), psdu_stride=20,
                      checks=(c,) if c != "noisy" else ()))
    return {x.name: x for x in s}


SPECS = _specs()
VALUE_SPECS = tuple("values_" + c for c in VALUE_CLASSES)
LONG_SPECS = tuple("long_%d" % e for e in range(8))
SHAPE_SPECS = tuple("n_%d" % n for n in (1, 63, 64, 65, 129, 1040)) + ("blocked_head", "one_rate_3", "one_rate_6", "second_rates")
LLR_BITS_SPECS = tuple("llr_bits_%d" % lb for lb in (1, 2, 4, 6))
TASK_SPECS = ("tasks_noisy", "tasks_nonfinite", "tasks_huge")
GEOMETRY_SPECS = ("short", "maxsym", "stride")


@dataclass
class Batch:
    spec: Spec
    fmt: str
    recs: np.ndarray              # what is uploaded
    rows: np.ndarray              # what is uploaded: float32, or bf16 patterns (uint16)
    rows_f32: np.ndarray          # what the reference reads
    psdus: list                   # transmitted PSDUs (None where the frame got no coherent row)
    meant: np.ndarray             # bool: frames meant to be decoded
    extra: dict = field(default_factory=dict)


def build(name: str, fmt: str) -> Batch:
    sp = SPECS[name]
    fn, args = sp.layout
    enc, ln, fl = fn(*args)
    recs = records(enc, ln, fl)
    signs, psdus = coherent(recs, sp.max_sym, sp.llr_bits, sp.seed)
    rng = np.random.default_rng(sp.seed * 7919 + (fmt == "bf16"))
    x = CLASSES[sp.cls](signs, recs, rng, fmt)
    if fmt == "bf16":
        rows = x if x.dtype == np.uint16 else bf16_rne(x)
        rows_f32 = bf16_to_f32(rows)
    else:
        rows, rows_f32 = x, x
    assert rows_f32.dtype == np.float32 and rows.shape == (recs.size, sp.max_sym * 48 * sp.llr_bits)
    meant = (((recs["flags"] & (ref.F_COMPLETE | ref.F_LLR)) == (ref.F_COMPLETE | ref.F_LLR)) & (ln <= sp.psdu_stride) &
             (ln <= ref.MAX_PSDU) & (recs["n_sym"] <= sp.max_sym) & (recs["n_bpsc"] <= sp.llr_bits))
    return Batch(sp, fmt, recs, np.ascontiguousarray(rows), rows_f32, psdus, meant)


@functools.lru_cache(maxsize=None)
def reference(name: str, fmt: str):
    """(batch, records after the reference's decode, PSDU rows [n][psdu_stride], frames that ended all-NaN)"""
    b = build(name, fmt)
    nan = np.zeros(b.recs.size, bool)
    fr, psdu = ref.decode_batch(b.recs, b.rows_f32, b.spec.max_sym, psdu_stride=b.spec.psdu_stride,
                                llr_bits=b.spec.llr_bits, nan_out=nan)
    return b, fr, psdu, nan


def expected_psdu_buffer(b: Batch, fr: np.ndarray, psdu: np.ndarray) -> np.ndarray:
    """the PSDU rows [n][psdu_stride] as the device must leave a buffer that was filled with FILL: bytes 0 .. psdu_len - 1
    of the frames the reference decoded, everything else untouched"""
    out = np.full((b.recs.size, b.spec.psdu_stride), FILL, np.uint8)
    for k in np.nonzero((fr["flags"] & ref.F_DECODED) != 0)[0]:
        ln = int(fr["psdu_len"][k])
        out[k, :ln] = psdu[k, :ln]
    return out


def check_conditions(name: str, fmt: str) -> dict:
    """What keeps a batch honest, on the reference alone; returns the figures it looked at."""
    b, fr, psdu, nan = reference(name, fmt)
    sp = b.spec
    dec = (fr["flags"] & ref.F_DECODED) != 0
    ok = (fr["flags"] & ref.F_CRC_OK) != 0
    enc = b.recs["encoding"].astype(np.int64)
    out = {"n": int(b.recs.size), "meant": int(b.meant.sum()), "decoded": int(dec.sum()), "crc_ok": int(ok.sum()),
           "all_nan": int(nan.sum())}
    assert np.array_equal(dec, b.meant), "the reference decodes exactly the frames meant to be decoded"
    assert b.meant.sum() >= 1 and 4 * dec[b.meant].sum() >= 3 * b.meant.sum()
    assert np.array_equal(fr[~b.meant], b.recs[~b.meant]) and not psdu[~b.meant].any()
    sent_ok = all(np.array_equal(psdu[k, :len(b.psdus[k])], b.psdus[k]) for k in np.nonzero(ok)[0])
    for c in sp.checks:
        if c == "noisy":
            for e in range(8):
                m = b.meant & (enc == e)
                assert 4 * ok[m].sum() >= m.sum() and 4 * (~ok[m]).sum() >= m.sum(), (e, int(ok[m].sum()), int(m.sum()))
            assert sent_ok
        elif c == "wide":
            assert 4 * ok.sum() >= b.meant.sum() and 4 * (b.meant & ~ok).sum() >= b.meant.sum(), out
            assert sent_ok
        elif c in ("subnormal", "const_coherent", "all_crc_from_4"):
            want = b.meant & (b.recs["psdu_len"] >= 4)
            assert np.array_equal(ok, want) and sent_ok, out
            if c == "subnormal":
                v = np.abs(b.rows_f32[b.rows_f32 != 0])
                assert v.size and v.max() < np.finfo(np.float32).tiny
        elif c == "nonfinite":
            x = b.rows_f32
            big = np.float32(1e30)
            for k in np.nonzero(b.meant)[0]:
                v = x[k, :int(extent(b.recs)[k])]
                assert np.isnan(v).any() and (v == np.inf).any() and (v == -np.inf).any(), k
            kept = np.nan_to_num(x, nan=big, posinf=big, neginf=-big).astype(np.float32)
            fr2, psdu2 = ref.decode_batch(b.recs, kept, sp.max_sym, psdu_stride=sp.psdu_stride, llr_bits=sp.llr_bits)
            differ = int((np.any(psdu != psdu2, axis=1) | (fr["flags"] != fr2["flags"])).sum())
            out["differ_from_unguarded"] = differ
            assert differ >= 1
        elif c == "huge":
            out["finite_to_the_end"] = int((b.meant & ~nan).sum())
            assert nan[b.meant].sum() >= 1 and (b.meant & ~nan).sum() >= 1, out
            assert np.isfinite(b.rows_f32).all() and np.abs(b.rows_f32[b.rows_f32 != 0]).min() >= 4e35
        elif c in ("zeros", "negzero"):
            assert dec[b.meant].all() and not ok.any() and not psdu.any()
            if c == "negzero":
                assert np.signbit(b.rows_f32).any() and not np.signbit(b.rows_f32).all() and not b.rows_f32.any()
        elif c == "const_random":
            pad = b.recs["n_sym"].astype(np.int64) * np.array(ref.N_DBPS)[enc] - (22 + 8 * b.recs["psdu_len"].astype(np.int64))
            assert (pad == 2).all()
        elif c == "at_max_sym":
            assert (b.recs["n_sym"][b.meant] == sp.max_sym).any()
        elif c == "narrow_rows":
            wide = b.recs["n_bpsc"] > sp.llr_bits
            assert wide.any() and not b.meant[wide].any()
        else:
            raise KeyError(c)
    return out


def n_tasks_and_longest(b: Batch):
    """tasks of 64 frames the host path makes of the batch (runs per rate start on task boundaries when it holds several
    rates), and its longest trellis, both over the frames the hard decoder's rule accepts"""
    r = b.recs
    acc = (((r["flags"] & ref.F_COMPLETE) != 0) & (r["psdu_len"] <= b.spec.psdu_stride) & (r["psdu_len"] <= ref.MAX_PSDU) &
           (r["n_sym"] <= b.spec.max_sym))
    enc = r["encoding"].astype(np.int64)
    per_rate = np.bincount(enc[acc], minlength=8)
    longest = int((r["n_sym"].astype(np.int64) * np.array(ref.N_DBPS)[enc])[acc].max())
    if (per_rate > 0).sum() > 1:
        return int(((per_rate + 63) // 64).sum()), longest
    return (r.size + 63) // 64, longest


def soft_slice(n_steps: int) -> int:
    """dec_soft_slice of csrc/wr_kernels.h: the scratch bytes of one wave"""
    return n_steps * 64 * 8 + (n_steps // 32 + 2) * 64 * 4
