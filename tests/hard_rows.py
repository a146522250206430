"""Frame records and hard decisions made on the host, for the hard-decision decode_mac (`wifirx_decode_batch`, NUMERICS.md
rule 14a).

Test infrastructure only.  `wifirx_decode_batch` reads caller-owned buffers, so a test can write the records a
demodulation would leave and ANY decisions it likes -- above all decisions far from every codeword, which no
transmission through a channel produces and which are what the decoders' tie rules, byte metrics and speculative
trace-back have to survive.  This module makes

* the decision classes (`CLASSES`): real coded frames, the same with bit flips, uniformly random bytes, all 0, all 0xFF,
  real frames with garbage above the rate's bits;
* `SPECS`: the one table of batches that tests/test_hard_rows.py (CPU: tests/hard_viterbi_ref.py against the oracle) and
  tests/test_gpu_hard_rows.py (device against the oracle) both run, and `check_conditions`, the properties that keep
  each batch from passing vacuously.

Margins of the byte metrics of decode_q_kernel, measured by the reference over every batch of the table (the kernel's
comment derives spread <= 12, candidate difference <= 14; the minimum cannot grow by more than 2 a step):
largest spread of a frame's 64 metrics from step 6 on 11 (MEASURED_SPREAD), largest |c1 - c0| 10 (MEASURED_CAND_DIFF),
largest growth of the minimum over 48 steps 16 (MEASURED_GROWTH).  tests/test_hard_rows.py::test_margins_of_the_byte_metrics
asserts both the bounds and that these figures are still what the table gives.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

import hard_viterbi_ref as ref
from helpers import planes_of
from soft_rows import (FILL, FRAME_DTYPE, F_DETECTED, F_SIGNAL, F_SYNC, MAXSYM_EDGE, STRIDE_EDGE, lay_blocked_head, lay_long,
                       lay_maxsym, lay_n, lay_short, lay_stride, lay_values, make_psdu, records)
from soft_viterbi_ref import F_COMPLETE, F_CRC_OK, F_DECODED, F_LLR, MAX_PSDU, N_BPSC, N_DBPS, n_sym_of
from wifirx import txgen

F_HARD = F_DETECTED | F_SYNC | F_SIGNAL | F_COMPLETE          # a complete frame of a handle without LLRs
MEASURED_SPREAD, MEASURED_CAND_DIFF, MEASURED_GROWTH = 11, 10, 16
BOUND_SPREAD, BOUND_CAND_DIFF, BOUND_GROWTH = 12, 14, 96       # what decode_q_kernel relies on

# bit flips per coded bit of `flips`, per rate: tuned on the reference so that CRC_OK is neither the rule nor the exception
FLIP_RATE = (0.068, 0.0256, 0.068, 0.0256, 0.068, 0.0245, 0.0385, 0.025)


# ---- decision classes: (coherent idx [n][max_sym][48], records, rng) -> idx ----

def coherent_idx(recs: np.ndarray, max_sym: int, seed: int):
    """`txgen.encode_psdus(...).data_idx` of real PSDUs, one per record whose symbols fit max_sym (the other rows stay 0),
    and the transmitted PSDUs (list, None for those)."""
    rng = np.random.default_rng(seed)
    n = recs.shape[0]
    idx = np.zeros((n, max_sym, 48), np.uint8)
    psdus = [None] * n
    enc, ln = recs["encoding"].astype(np.int64), recs["psdu_len"].astype(np.int64)
    for e, l in sorted(set(zip(enc.tolist(), ln.tolist()))):
        n_sym = n_sym_of(e, l)
        if n_sym > max_sym:
            continue
        g = np.nonzero((enc == e) & (ln == l))[0]
        p = make_psdu(g.size, l, rng)
        idx[g, :n_sym] = txgen.encode_psdus(p, e, seeds=rng.integers(1, 128, g.size)).data_idx
        for j, k in enumerate(g):
            psdus[k] = p[j]
    return idx, psdus


def _nb_mask(recs):
    """[n][1][1] uint8: the bits of a decision byte that carry coded bits at the record's rate"""
    return ((1 << np.array(N_BPSC)[recs["encoding"].astype(np.int64) & 7]) - 1).astype(np.uint8)[:, None, None]


def d_coherent(idx, recs, rng, scale):
    return idx


def d_flips(idx, recs, rng, scale):
    p = scale * np.array(FLIP_RATE)[recs["encoding"].astype(np.int64) & 7][:, None, None, None]
    flip = np.packbits(rng.random(idx.shape + (8,), dtype=np.float32) < p.astype(np.float32), axis=3, bitorder="little")[..., 0]
    return idx ^ (flip & _nb_mask(recs))


def d_random(idx, recs, rng, scale):
    return rng.integers(0, 256, idx.shape, dtype=np.uint8)


def d_zeros(idx, recs, rng, scale):
    return np.zeros_like(idx)


def d_ones(idx, recs, rng, scale):
    return np.full_like(idx, 0xFF)


def d_highbits(idx, recs, rng, scale):
    m = _nb_mask(recs)
    return (idx & m) | (rng.integers(0, 256, idx.shape, dtype=np.uint8) & ~m)


CLASSES = {"coherent": d_coherent, "flips": d_flips, "random": d_random, "zeros": d_zeros, "ones": d_ones, "highbits": d_highbits}
VALUE_CLASSES = tuple(CLASSES)


# ---- batch layouts of this table: () -> (enc [n], psdu_len [n], flags [n]); the others are soft_rows' ----

def longest_psdu(enc: int, n_sym: int) -> int:
    return (n_sym * N_DBPS[enc] - 22) // 8


LADDER_SYMS = 10


def lay_ladder():
    """per rate the longest PSDU of 1 .. 10 symbols, three frames each, rates and lengths interleaved (neighbouring lanes
    hold trellises of different lengths), and psdu_len 0 .. 3 at every rate"""
    k = np.arange(8 * LADDER_SYMS * 3)
    enc, n_sym = k % 8, (k // 8) % LADDER_SYMS + 1
    ln = np.array([[longest_psdu(e, q) for q in range(LADDER_SYMS + 1)] for e in range(8)])[enc, n_sym]
    j = np.arange(32)
    return np.concatenate([enc, j % 8]), np.concatenate([ln, j // 8]), np.full(k.size + 32, F_HARD)


# n_sym of the three lengths of `uniform_<enc>_<k>`: trellises of a multiple of 96 steps (the block of the speculative
# trace-back), of the smallest remainder the rate's n_dbps allows, and of the largest.  12 and 84 exist only where n_dbps is
# an odd multiple of 12 (36, rate 1): at 24, 72 and 216 the remainders are multiples of 24, at 144 of 48, at 192 there is
# none but 0 (three different multiples then).
UNIFORM_SYMS = {0: (12, 13, 15), 1: (8, 3, 5), 3: (4, 3, 5), 5: (2, 3, 4), 6: (1, 2, 3)}
UNIFORM_REMAINDERS = {0: (0, 24, 72), 1: (0, 12, 84), 3: (0, 24, 72), 5: (0, 48, 0), 6: (0, 0, 0)}


def lay_uniform(enc, n_sym, n=300):
    return np.full(n, enc), np.full(n, longest_psdu(enc, n_sym)), np.full(n, F_HARD)


def hard_flags(layout):
    """a soft_rows layout for the hard decoder: no record carries WIFIRX_F_LLR, and a record soft_rows blocked by clearing
    that flag alone is blocked by a missing WIFIRX_F_COMPLETE instead"""
    def lay(*args):
        enc, ln, fl = layout(*args)
        fl = np.where((fl & F_LLR) == 0, fl & ~F_COMPLETE, fl) & ~F_LLR
        return enc, ln, fl
    return lay


@dataclass(frozen=True)
class Spec:
    name: str
    cls: str
    layout: tuple                 # (function, args)
    max_sym: int
    psdu_stride: int = 64
    seed: int = 1
    flip_scale: float = 1.0
    checks: tuple = ()            # names of the extra conditions of check_conditions


N_SHAPES = (1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 513)


def _specs():
    s = []
    for i, c in enumerate(VALUE_CLASSES):
        s.append(Spec("values_" + c, c, (hard_flags(lay_values), (2112,)), max_sym=n_sym_of(0, 64), seed=300 + i, psdu_stride=96,
                      checks=(c, "values_shape")))
    s.append(Spec("ladder", "random", (lay_ladder, ()), max_sym=LADDER_SYMS, seed=320, psdu_stride=longest_psdu(7, LADDER_SYMS) + 1,
                  checks=("random", "ladder")))
    for e, syms in UNIFORM_SYMS.items():
        for k, q in enumerate(syms):
            s.append(Spec("uniform_%d_%d" % (e, k), "random", (lay_uniform, (e, q)), max_sym=q, seed=330 + 3 * e + k,
                          psdu_stride=longest_psdu(e, q) + 3, checks=("random", "uniform")))
    for e in range(8):
        for c in ("flips", "random"):
            s.append(Spec("long_%d_%s" % (e, c), c, (hard_flags(lay_long), (e,)), max_sym=511, psdu_stride=1536, seed=360 + 2 * e + (c == "random"),
                          flip_scale=0.3, checks=("long",) + (("random",) if c == "random" else ())))
    s.append(Spec("maxsym", "flips", (hard_flags(lay_maxsym), ()), max_sym=MAXSYM_EDGE, seed=381, psdu_stride=330, checks=("maxsym",)))
    s.append(Spec("stride", "flips", (hard_flags(lay_stride), ()), max_sym=n_sym_of(0, STRIDE_EDGE), seed=382, psdu_stride=STRIDE_EDGE,
                  checks=("stride",)))
    s.append(Spec("short", "flips", (hard_flags(lay_short), ()), max_sym=4, seed=383, psdu_stride=16, flip_scale=0.5, checks=("short",)))
    s.append(Spec("blocked_head", "random", (hard_flags(lay_blocked_head), ()), max_sym=n_sym_of(0, 26), seed=384,
                  checks=("random", "blocked_head")))
    for n in N_SHAPES:
        s.append(Spec("n_%d" % n, "random", (hard_flags(lay_n), (n,)), max_sym=n_sym_of(0, 21), seed=390 + n % 23, psdu_stride=24,
                      checks=("random",)))
    return {x.name: x for x in s}


SPECS = _specs()
VALUE_SPECS = tuple("values_" + c for c in VALUE_CLASSES)
UNIFORM_SPECS = tuple("uniform_%d_%d" % (e, k) for e in UNIFORM_SYMS for k in range(3))
LONG_SPECS = tuple("long_%d_%s" % (e, c) for e in range(8) for c in ("flips", "random"))
EDGE_SPECS = ("maxsym", "stride", "short", "blocked_head")
N_SPECS = tuple("n_%d" % n for n in N_SHAPES)


@dataclass
class Batch:
    spec: Spec
    recs: np.ndarray              # what is uploaded
    idx: np.ndarray               # what is uploaded: [n][max_sym][48] uint8
    psdus: list                   # transmitted PSDUs (None where the frame got no coherent row)
    meant: np.ndarray             # bool: frames meant to be decoded

    def planes(self) -> np.ndarray:
        """the bit planes of the same decisions (wifirx_out.hbits), [n][max_sym * 12] uint32"""
        return planes_of(self.recs, self.idx, self.spec.max_sym)


@functools.lru_cache(maxsize=None)
def build(name: str) -> Batch:
    sp = SPECS[name]
    fn, args = sp.layout
    enc, ln, fl = fn(*args)
    recs = records(enc, ln, fl)
    assert recs.dtype == FRAME_DTYPE and not (recs["flags"] & (F_LLR | F_DECODED | F_CRC_OK)).any()
    # "coherent" and "highbits" of one layout carry the same frames: the seed of the frames is the layout's
    idx, psdus = coherent_idx(recs, sp.max_sym, seed=300 if name.startswith("values_") else sp.seed)
    rng = np.random.default_rng(sp.seed * 7919)
    idx = np.ascontiguousarray(CLASSES[sp.cls](idx, recs, rng, sp.flip_scale), np.uint8)
    idx.setflags(write=False)
    recs.setflags(write=False)
    n_sym = recs["n_sym"].astype(np.int64)
    meant = ((recs["flags"] & F_COMPLETE) != 0) & (ln <= sp.psdu_stride) & (ln <= MAX_PSDU) & (n_sym <= min(sp.max_sym, 511))
    return Batch(sp, recs, idx, psdus, meant)


@functools.lru_cache(maxsize=None)
def reference(name: str):
    """(batch, records after tests/hard_viterbi_ref.py's decode, PSDU rows [n][psdu_stride], its margins and tie counts)"""
    b = build(name)
    fr, psdu, info = ref.decode_batch(b.recs, b.idx, b.spec.max_sym, psdu_stride=b.spec.psdu_stride)
    return b, fr, psdu, info


@functools.lru_cache(maxsize=None)
def oracle_reference(name: str):
    """(batch, records after the oracle's decode_mac, its PSDU rows [n][psdu_stride], zero-filled) -- what the GPU tests
    compare with: tests/test_hard_rows.py shows that it equals `reference` on every batch, and it takes a fraction of the time"""
    from oracle import oracle as orc
    b = build(name)
    fr = b.recs.copy()
    psdu = orc.decode_batch(fr, b.idx, orc.make_params(max_sym=b.spec.max_sym), psdu_stride=b.spec.psdu_stride, n_threads=8)
    for a in (fr, psdu):
        a.setflags(write=False)
    return b, fr, psdu


def expected_psdu_buffer(b: Batch, fr: np.ndarray, psdu: np.ndarray, stride=None) -> np.ndarray:
    """the PSDU rows [n][psdu_stride] as the device must leave a buffer that was filled with FILL: bytes 0 .. psdu_len - 1
    of the frames the reference decoded, everything else untouched.  stride: rows of another stride than the batch's own
    (for batches in which the stride holds no frame back)"""
    out = np.full((b.recs.size, stride or b.spec.psdu_stride), FILL, np.uint8)
    for k in np.nonzero((fr["flags"] & F_DECODED) != 0)[0]:
        ln = int(fr["psdu_len"][k])
        out[k, :ln] = psdu[k, :ln]
    return out


def check_conditions(name: str) -> dict:
    """What keeps a batch honest, on the reference alone; returns the figures it looked at."""
    b, fr, psdu, info = reference(name)
    sp, recs = b.spec, b.recs
    dec = (fr["flags"] & F_DECODED) != 0
    ok = (fr["flags"] & F_CRC_OK) != 0
    enc = recs["encoding"].astype(np.int64)
    ln = recs["psdu_len"].astype(np.int64)
    steps = recs["n_sym"].astype(np.int64) * np.array(N_DBPS)[enc]
    long_enough = b.meant & (steps >= 192)
    mg = info["margins"]
    out = {"n": int(recs.size), "meant": int(b.meant.sum()), "decoded": int(dec.sum()), "crc_ok": int(ok.sum()),
           "final_tied": int(info["final_tied"].sum()), "tie_on_path_192": int((info["ties"][long_enough] > 0).sum()),
           "of_192": int(long_enough.sum()), "median_ties_192": float(np.median(info["ties"][long_enough])) if long_enough.any() else 0.0,
           "spread": mg.spread, "cand_diff": mg.cand_diff, "growth": mg.growth}
    # common to all: the reference decodes exactly the frames the rule accepts and leaves the other records untouched
    assert np.array_equal(dec, b.meant) and b.meant.any(), out
    assert np.array_equal(info["steps"][b.meant], steps[b.meant])
    assert np.array_equal(fr[~b.meant], recs[~b.meant]) and not psdu[~b.meant].any()
    assert not ok[ln < 4].any()
    assert ((recs["flags"] & F_LLR) == 0).all() and (recs["encoding"] < 8).all()
    sent_ok = all(np.array_equal(psdu[k, :ln[k]], b.psdus[k]) for k in np.nonzero(ok)[0])
    for c in sp.checks:
        if c in ("coherent", "highbits"):
            assert np.array_equal(ok, b.meant & (ln >= 4)) and sent_ok, out
            assert all(np.array_equal(psdu[k, :ln[k]], b.psdus[k]) for k in np.nonzero(dec)[0])
            if c == "highbits":
                b0, fr0, psdu0, _ = reference(name.replace("highbits", "coherent"))
                assert np.array_equal(fr, fr0) and np.array_equal(psdu, psdu0)
                high = b.idx & ~_nb_mask(recs)
                assert np.array_equal(b.idx & _nb_mask(recs), b0.idx) and high[enc < 6].any() and high[enc >= 6].any()
        elif c == "flips":
            for e in range(8):
                m = b.meant & (enc == e)
                out["crc_ok_%d" % e] = int(ok[m].sum())
                assert 4 * ok[m].sum() >= m.sum() and 4 * (~ok[m]).sum() >= m.sum(), (e, int(ok[m].sum()), int(m.sum()))
            assert sent_ok
        elif c == "random":
            assert not ok.any(), out
            assert 4 * info["final_tied"][b.meant].sum() >= b.meant.sum(), out
            assert 4 * (info["ties"][long_enough] > 0).sum() >= long_enough.sum(), out
            if name == "values_random":
                assert (b.idx >> 6).any() and long_enough.any()
        elif c == "zeros":
            assert not b.idx.any() and not psdu.any() and not ok.any()
        elif c == "ones":
            assert (b.idx == 0xFF).all()
        elif c == "values_shape":
            assert all((enc == e).sum() == 264 and set(ln[enc == e].tolist()) == {30, 45, 64} for e in range(8)) and b.meant.all()
        elif c == "ladder":
            assert set(steps[enc == 0].tolist()) >= {24, 48, 96, 120, 192, 216}
            assert all(set(recs["n_sym"][enc == e].tolist()) == set(range(1, LADDER_SYMS + 1)) for e in range(8))
            assert all(set(ln[enc == e].tolist()) >= {0, 1, 2, 3} for e in range(8)) and b.meant.all()
            assert (np.diff(steps[:240]) != 0).all()          # neighbours differ in length
        elif c == "uniform":
            e, k = int(name.split("_")[1]), int(name.split("_")[2])
            assert recs.size == 300 and b.meant.all() and (enc == e).all() and len(set(steps.tolist())) == 1
            out["steps"], out["remainder"] = int(steps[0]), int(steps[0]) % 96
            assert out["remainder"] == UNIFORM_REMAINDERS[e][k] and steps[0] >= 96
            assert len({n_sym_of(e, longest_psdu(e, q)) for q in UNIFORM_SYMS[e]}) == 3
        elif c == "long":
            assert recs.size == 65 and b.meant.sum() == 64 and (ln[~b.meant] == MAX_PSDU + 1).all() and not b.meant[31]
            assert 12264 <= steps[b.meant].min() and steps[b.meant].max() <= 12384 and steps[0] // 120 > 100
            if enc[0] == 0:
                assert (recs["n_sym"][b.meant] == sp.max_sym).all()
        elif c == "maxsym":
            assert (recs["n_sym"][b.meant] == sp.max_sym).all() and (recs["n_sym"][~b.meant] == sp.max_sym + 1).all() and (~b.meant).any()
        elif c == "stride":
            assert sp.psdu_stride % 2 == 1
            assert b.meant[ln == sp.psdu_stride].all() and (ln == sp.psdu_stride).any()
            assert not b.meant[ln == sp.psdu_stride + 1].any() and (ln == sp.psdu_stride + 1).any()
        elif c == "short":
            assert set(ln.tolist()) == {0, 1, 2, 3, 4, 5, 7, 8} and b.meant.all() and ok.any()
        elif c == "blocked_head":
            head = np.arange(recs.size) < 64
            assert not b.meant[head].any() and b.meant[~head].all()
            assert ((recs["flags"][head] & F_COMPLETE) == 0).any() and (ln[head] > sp.psdu_stride).any()
            assert (((recs["flags"][head] & F_COMPLETE) == 0) | (ln[head] > sp.psdu_stride)).all()
        else:
            raise KeyError(c)
    return out
