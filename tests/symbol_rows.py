"""Host-built slots for the symbol path (SIGNAL symbol, SIGNAL decision, data-symbol bookkeeping, slicer: NUMERICS.md
rules 7, 7a, 12, 15): one table for tests/test_symbol_rows.py (CPU: the restatement of tests/symbol_ref.py against the
oracle, the table's conditions, the restatement's mutants) and tests/test_gpu_symbol_rows.py (the device against both, in
batches and in streams).

A row is a clean preamble (the four sync words of wifirx.txgen), a SIGNAL symbol that carries 48 CHOSEN bits on its data
bins -- a codeword of the SIGNAL field or anything else: the receiver hands the 48 hard decisions to its Viterbi as they
are -- and data symbols with chosen points on the data bins, all synthesised by txgen._freq_symbol_to_time with the cyclic
prefix and the roll-off sample of the transmitter.  The preamble starts at sample LEAD of a slot on its own; in a batch of
uniform slots the zeros in front grow instead (the copied length L stays).  The SIGNAL symbol's 64 samples start at slot
sample LEAD + 336, data symbol q's at LEAD + 416 + 80 q, whatever the trigger: a slot of LEAD + 480 + 80 q samples ends
exactly where data symbol q ends.

Classes (`cls`) and groups (`grp`: rows of a group share a handle, i.e. max_sym):
  grp "sig" (max_sym 3, four QPSK data symbols on the air behind every SIGNAL symbol)
    field     true codewords: the sixteen RATE nibbles, the parity bit right and wrong, the reserved bit, non-zero tail bits,
              LENGTH 0, 1, 3, 4, 1528, 1529, 4095, per rate both sides of two n_sym steps -- one of them 3 | 4, i.e. n_sym =
              max_sym and max_sym + 1
    far       48 bits far from every codeword: all-zero, all-one, alternating, period 4, RANDOM_WORDS seeded words, and
              the words SEARCHED below found on the restatement
  grp "thr" (max_sym 17) data rows: every component of every data point ON a slicer threshold in float64 (16-QAM +-2a,
              64-QAM +-2a / 4a / 6a, BPSK and QPSK 0): the receiver's rounding scatters them a few ulps around the float32
              thresholds and lands on them; `claim`: SIGNAL words that parse to another rate than the points were made for
  grp "long" (max_sym 37) one BPSK and one QPSK frame of 37 symbols of zero points: where LMS and STA end up (|Y| about 10, -0)
  grp "end" (max_sym 4) the slot's end: L where the last data symbol ends and one sample fewer, for n_sym below and at max_sym
  grp "zero" (max_sym 6) a QPSK frame cut to exact zeros at a symbol boundary and in mid-symbol: rule 10's n2 = 0 branch,
              rule 9's sp_atan2(0, 0), COMB's zero pilots

Not reachable through the API:
  a SIGNAL symbol without a synchronised preamble  the 48 decisions exist only behind SYNC; tests/lts_rows.py owns what
              happens before
  48 decisions with an erasure  the SIGNAL Viterbi takes hard bits only (the value 2 of the oracle's decode_mac Viterbi
              never occurs here); orc.viterbi is compared on hard bits alone
  metric bytes of 128 and more  the largest reachable metric after 24 steps is 48, the start value 64 + 48 stays below 128:
              the searched word reaches SEARCHED["top"][1] (reachable states) and the packed model's largest byte is
              asserted in tests/test_symbol_rows.py"""
import functools

import numpy as np

import symbol_ref as ref
from detect_rows import PUSHES, STREAM_BATCHES          # noqa: F401  (the push sizes of the stream tests)
from wifirx import txgen

LEAD = 100
GROUPS = {"sig": dict(max_sym=3, slot=960), "thr": dict(max_sym=17, slot=2000), "end": dict(max_sym=4, slot=1040),
          "zero": dict(max_sym=6, slot=1200), "long": dict(max_sym=37, slot=3600)}
LLR_BITS = 6
RANDOM_WORDS, RANDOM_SEED = 208, 7
GAP = 700                   # exact zeros between the rows of a stream

# Found by search_words(seed=5, n=120000) on the restatement (run by hand, a few minutes): 48-bit words, bit j = the
# decision of data carrier j.  "tie0": the final metrics tie between state 0 and higher states (value: word, the tied
# states); "path": the surviving path passes the most tied add-compare-selects the search saw among words whose record
# shows them (word, their number: 6 of 24); "top": the largest reachable path metric of the 24 steps (word, that metric:
# 13 -- a random word lies at distance 7 to 10 of its nearest codeword, and no state of the trellis is further than a few
# more).  "tie0" and "path" parse, and decided by the other rule they would not, or to another record.
# tests/test_symbol_rows.py recomputes the figures.
SEARCHED = {
    "tie0": (0xe2d5d260242b, (0, 1, 6, 31, 33)),
    "path": (0xcff6f020717a, 6),
    "top": (0x9214d4a251aa, 13),
}


def word_bits(w):
    return np.array([(int(w) >> j) & 1 for j in range(48)], np.uint8)


def bits_word(b):
    return sum(int(v) << j for j, v in enumerate(b))


def codeword(rate, length, parity_ok=True, reserved=0, tail=0):
    """the 48 carrier-order bits of a true SIGNAL codeword with this RATE nibble (R1 in bit 0), LENGTH, reserved bit and
    six tail bits"""
    b = [(rate >> i) & 1 for i in range(4)] + [reserved] + [(length >> i) & 1 for i in range(12)]
    b.append((sum(b) & 1) ^ (0 if parity_ok else 1))
    b += [(tail >> i) & 1 for i in range(6)]
    return np.array(ref.interleave(ref.conv_encode(b)), np.uint8)


RATE_OF = {e: r for r, e in ref.RATE.items()}


def step_lengths(enc, n):
    """the two lengths on either side of the step n_sym = n | n + 1"""
    lo = (n * ref.N_DBPS[enc] - 22) // 8
    return lo, lo + 1


def search_words(seed=5, n=30000):
    """the CPU search behind SEARCHED (run by hand)"""
    rng = np.random.default_rng(seed)
    best = {"tie0": None, "path": (0, -1), "top": (0, -1)}
    for _ in range(n):
        w = int(rng.integers(0, 1 << 48))
        b = word_bits(w)
        info = ref.viterbi24(ref.deinterleave(b))[1]
        if info["top"] > best["top"][1]:
            best["top"] = (w, info["top"])
        # "tie0" and "path" are kept only where the RECORD shows the rule: the word parses, and with the other rule it
        # would not, or to another rate or length
        if (best["tie0"] is None and info["ends"][0] == 0 and len(info["ends"]) > 1) or info["path_ties"] > max(best["path"][1], 5):
            good = ref.decode_signal(b)
            if not good[0]:
                continue
            if best["tie0"] is None and info["ends"][0] == 0 and len(info["ends"]) > 1 and ref.decode_signal(b, ("final_highest",)) != good:
                best["tie0"] = (w, tuple(info["ends"]))
            if info["path_ties"] > max(best["path"][1], 5) and ref.decode_signal(b, ("m1_le_m0",)) != good:
                best["path"] = (w, info["path_ties"])
    return best


# ---- frames -------------------------------------------------------------------------------------------------------------

def frame(sig48, points):
    """complex64 samples of preamble + SIGNAL symbol with the 48 bits + len(points) data symbols with these points"""
    points = np.asarray(points, dtype=np.complex128).reshape(-1, 48)
    n = points.shape[0]
    X = np.zeros((5 + n, 64), np.complex128)
    X[0:4] = txgen.sync_words()
    X[4, txgen.DATA_BINS] = 2.0 * np.asarray(sig48, dtype=np.float64) - 1.0
    if n:
        X[5:, txgen.DATA_BINS] = points
    p = txgen.polarity_sequence()[np.arange(n + 1) % 127]
    X[4:, 11] = p
    X[4:, 25] = p
    X[4:, 39] = p
    X[4:, 53] = -p
    x = txgen._freq_symbol_to_time(X)
    sym = np.concatenate([x[:, 48:], x], axis=1)
    sym[:, 0] *= 0.5
    sym[1:, 0] += 0.5 * x[:-1, 0]
    out = np.concatenate([sym.reshape(-1), [0.5 * x[-1, 0]]])
    return out.astype(np.complex64)


def qpsk_points(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.choice([-1.0, 1.0], (n, 48)) + 1j * rng.choice([-1.0, 1.0], (n, 48))) * np.sqrt(0.5)


def threshold_points(n_bpsc, n, seed):
    """n symbols whose 96 components each lie on a threshold of the constellation, signs and thresholds drawn"""
    rng = np.random.default_rng(seed)
    if n_bpsc <= 2:
        return np.zeros((n, 48), np.complex128)
    a, mults = (np.sqrt(0.1), (2,)) if n_bpsc == 4 else (np.sqrt(1.0 / 42.0), (2, 4, 6))
    re = rng.choice([-1, 1], (n, 48)) * rng.choice(mults, (n, 48)) * a
    im = rng.choice([-1, 1], (n, 48)) * rng.choice(mults, (n, 48)) * a
    return re + 1j * im


def _row(name, cls, grp, sig48, points, cut=None, zero_from=None, want=None, stream=True):
    """cut: the row's samples end `cut` samples behind the preamble's first (None: the whole frame and 59 zeros);
    zero_from: exact zeros from that frame sample on"""
    f = frame(sig48, points)
    if zero_from is not None:
        f = f.copy()
        f[zero_from:] = 0
    x = np.concatenate([f, np.zeros(59, np.complex64)]) if cut is None else np.concatenate([f, np.zeros(max(cut - f.size, 0), np.complex64)])[:cut]
    assert LEAD + x.size <= GROUPS[grp]["slot"], (name, x.size)
    return dict(name=name, cls=cls, grp=grp, sig48=np.asarray(sig48, np.uint8), samples=x, want=want or {}, stream=stream,
                n_air=np.asarray(points).reshape(-1, 48).shape[0])


def slot_of(row, total=None):
    s = LEAD if total is None else total - row["samples"].size
    assert s >= LEAD
    return np.concatenate([np.zeros(s, np.complex64), row["samples"]])


def never_slot(n):
    """a burst too short to trigger"""
    from detect_rows import ints_burst
    return np.concatenate([np.zeros(n - 60, np.complex64), ints_burst(60, 0, 9)])


@functools.lru_cache(maxsize=None)
def table():
    rows = []
    add = rows.append
    ms = GROUPS["sig"]["max_sym"]

    def sig(name, cls, bits, **want):
        add(_row(name, cls, "sig", bits, qpsk_points(ms + 1, len(rows)), want=want))

    # ---- SIGNAL: every field class, each a true codeword ------------------------------------------------------------------
    for r in range(16):
        sig("field/rate%d" % r, "field", codeword(r, 40), ok=r in ref.RATE)
    for r in (11, 9, 12):
        sig("field/parity_wrong/%d" % r, "field", codeword(r, 40, parity_ok=False), ok=False)
        sig("field/reserved/%d" % r, "field", codeword(r, 40, reserved=1), ok=True, reserved=True)
    # (the parity covers the reserved bit: LENGTH 41 has the other parity, so both values of bit 17 occur with bit 4 set)
    sig("field/reserved/len41", "field", codeword(10, 41, reserved=1), ok=True, reserved=True)
    for k, tail in enumerate((1, 32, 63, 0b101010)):
        sig("field/tail/%d" % tail, "field", codeword((11, 10, 9, 8)[k], 40, tail=tail), ok=True, tail=True)
    # LENGTH bit 11 is bit 16 of the word, the last one under the parity: 2048 and 4095 have it set
    for ln in (0, 1, 3, 4, 1528, 1529, 2048, 4095):
        for e in (0, 7):
            sig("field/len%d/enc%d" % (ln, e), "field", codeword(RATE_OF[e], ln), ok=True, length=ln)
    for e in range(8):
        for n in (ms, 40 + e):
            lo, hi = step_lengths(e, n)
            sig("field/step%d/enc%d/lo" % (n, e), "field", codeword(RATE_OF[e], lo), ok=True, n_sym=n, step=(e, n, 0))
            sig("field/step%d/enc%d/hi" % (n, e), "field", codeword(RATE_OF[e], hi), ok=True, n_sym=n + 1, step=(e, n, 1))

    # ---- SIGNAL: far from every codeword ----------------------------------------------------------------------------------
    j = np.arange(48)
    for name, bits in (("zeros", 0 * j), ("ones", 0 * j + 1), ("alt01", j & 1), ("alt10", 1 - (j & 1)), ("period4", (j >> 1) & 1),
                       ("period4b", ((j + 1) >> 1) & 1)):
        sig("far/" + name, "far", bits)
    rng = np.random.default_rng(RANDOM_SEED)
    for k in range(RANDOM_WORDS):
        sig("far/random/%d" % k, "far", rng.integers(0, 2, 48), random=True)
    for k in ("tie0", "path", "top"):
        sig("far/searched/" + k, "far", word_bits(SEARCHED[k][0]), searched=k)

    # ---- data points on the thresholds ------------------------------------------------------------------------------------
    for nb, e, ln, nfr in ((4, 4, 200, 12), (6, 6, 200, 16), (1, 0, 40, 6), (2, 2, 90, 6)):
        n = ref.n_sym_of(e, ln)
        for k in range(nfr):
            add(_row("thr/nb%d/%d" % (nb, k), "thr", "thr", codeword(RATE_OF[e], ln), threshold_points(nb, n, 1100 + 16 * nb + k),
                     want=dict(nb=nb, n_sym=n)))
    # 37 symbols of zero points: under LMS and STA the decision-directed update on near-zero points halves H symbol by symbol
    # and |Y| grows to about 10 -- from symbol 30 on the points are no longer near zero, and STA's first -0 components
    # appear behind symbol 32
    for e in (0, 2):
        n = GROUPS["long"]["max_sym"]
        add(_row("long/enc%d" % e, "long", "long", codeword(RATE_OF[e], step_lengths(e, n)[0]), threshold_points(ref.N_BPSC[e], n, 0),
                 want=dict(nb=ref.N_BPSC[e], n_sym=n)))
    # the rate a SIGNAL word claims: 64-QAM threshold points behind SIGNAL words of all eight rates, n_sym 5 .. 9
    for e in range(8):
        ln = step_lengths(e, 5 + e % 5)[0]
        add(_row("claim/enc%d" % e, "claim", "thr", codeword(RATE_OF[e], ln), threshold_points(6, 9, 1300 + e), want=dict(claim=e)))

    # ---- the slot's end ---------------------------------------------------------------------------------------------------
    me = GROUPS["end"]["max_sym"]
    for e, nsym in ((2, me - 1), (2, me), (5, me), (6, me - 2)):
        ln = step_lengths(e, nsym)[0]
        for d in (0, -1):
            add(_row("end/enc%d/n%d/%s" % (e, nsym, "exact" if d == 0 else "short1"), "end", "end", codeword(RATE_OF[e], ln),
                     threshold_points(ref.N_BPSC[e], me + 1, 1400 + e), cut=480 + 80 * (nsym - 1) + d,
                     want=dict(truncated=d < 0, n_sym=nsym), stream=False))
    # n_sym = max_sym + 1 with all its samples there: TRUNCATED by the output rows alone
    add(_row("end/enc2/n%d/rows" % (me + 1), "end", "end", codeword(RATE_OF[2], step_lengths(2, me + 1)[0]),
             threshold_points(2, me + 1, 1410), want=dict(truncated=True, n_sym=me + 1), stream=False))

    # ---- exact zeros ------------------------------------------------------------------------------------------------------
    mz = GROUPS["zero"]["max_sym"]
    ln = step_lengths(2, mz)[0]
    for name, z in (("boundary", 400 + 80 * 2), ("mid", 400 + 80 * 2 + 16 + 23), ("signal_mid", 320 + 16 + 40), ("first", 400)):
        add(_row("zero/" + name, "zero", "zero", codeword(RATE_OF[2], ln), qpsk_points(mz, 1500), zero_from=z, want=dict(zero_from=z)))
    return rows


def group(grp):
    return [r for r in table() if r["grp"] == grp]


def by_name():
    return {r["name"]: r for r in table()}


def sig_arrangements():
    """(name, entries) over the SIGNAL rows: an entry is a row, "never" (a slot that never triggers) or "empty" (a slot of
    length 0; the variable-length form only).  A wave of the demod kernels holds four consecutive slots: a row's byte of
    the packed Viterbi's registers is its place modulo 4."""
    rows = group("sig")
    by = by_name()
    out = [("order", list(rows)), ("reversed", list(rows[::-1]))]
    for k in (1, 2, 3):
        out.append(("rotated%d" % k, ["never"] * k + list(rows)))
    # four classes in one register, every rotation: parses / parity fails / rate invalid / parses with n_sym > max_sym
    four = [by["field/rate11"], by["field/parity_wrong/9"], by["field/rate5"], by["field/len4095/enc0"]]
    ent = []
    for k in range(4):
        ent += four[k:] + four[:k]
    out.append(("four_classes", ent))
    # the worst-metric word beside the all-zero word in every byte position, then beside nothing, then beside a slot that
    # never triggers and a slot of length 0
    top, zero = by["far/searched/top"], by["far/zeros"]
    ent = []
    for k in range(4):
        w = [zero] * 4
        w[k] = top
        ent += w
    for k in range(4):
        w = [top] * 4
        w[k] = zero
        ent += w
    out.append(("worst_beside_zero", ent))
    for n in (1, 2, 3):
        out.append(("last_wave%d" % n, four + [top, by["far/searched/tie0"], by["far/searched/path"]][:n]))
    ent = []
    for k in range(4):
        w = [by["field/rate11"], "never", "empty", by["far/searched/path"]]
        ent += w[k:] + w[:k]
    out.append(("beside_never_and_empty", ent))
    return out


V_NEVER = 200               # length of the never-triggering slot in the variable-length form
KEEP = ref.F_SIGNAL | ref.F_COMPLETE | ref.F_LLR | ref.F_TRUNCATED       # the flags the restatement decides


def entry_name(entry):
    return entry if isinstance(entry, str) else entry["name"]


def entry_samples(entry, form, grp):
    """the entry as a slot: form "u" = the group's uniform slot, "v" = on its own"""
    if isinstance(entry, str):
        if entry == "empty":
            assert form == "v"
            return np.zeros(0, np.complex64)
        return never_slot(GROUPS[grp]["slot"] if form == "u" else V_NEVER)
    return slot_of(entry, GROUPS[grp]["slot"] if form == "u" else None)


_exp = {}


def expected(orc, entry, form, chan_est=0, llr_csi=0, grp=None):
    """the oracle's outputs of one entry as a slot of its own -- the same wherever it stands in a batch: dict(frame, idx
    [max_sym, 48], llr [max_sym 48 6] float32, eq [max_sym, 48], csi [52]); computed once"""
    grp = grp or entry["grp"]
    key = (entry_name(entry), form, chan_est, llr_csi, grp)
    if key not in _exp:
        ms = GROUPS[grp]["max_sym"]
        x = entry_samples(entry, form, grp)
        if x.size == 0:
            fr = np.zeros(1, orc.FRAME_DTYPE)
            fr["trigger"] = -1
            _exp[key] = dict(frame=fr[0], idx=np.zeros((ms, 48), np.uint8), llr=np.zeros(ms * 48 * LLR_BITS, np.float32),
                             eq=np.zeros((ms, 48), np.complex64), csi=np.zeros(52, np.complex64))
        else:
            prm = orc.make_params(max_sym=ms, llr_bits=LLR_BITS, chan_est=chan_est, llr_csi=llr_csi)
            o = orc.demod_batch(x, x.size, prm, want_eq=True, want_csi=True)
            _exp[key] = dict(frame=o["frames"][0], idx=o["idx"][0], llr=o["llr"][0], eq=o["eq"][0], csi=o["csi"][0])
    return _exp[key]


def restated_record(row, frame, n_samples, max_sym, mut=(), llr_bits=LLR_BITS):
    """tests/symbol_ref.py's record of a row from its constructed bits; the trigger and the frame start are the given
    record's (frame synchronisation is the subject of tests/lts_rows.py)"""
    L = min(n_samples - (int(frame["trigger"]) - 16), 540 * 80)
    return ref.record(row["sig48"], L, int(frame["frame_start"]), max_sym, llr_bits, mut)


def record_tuple(fr):
    """the fields the restatement decides, of a record (numpy) or of symbol_ref.record's dict"""
    return (int(fr["flags"]) & KEEP, int(fr["encoding"]), int(fr["psdu_len"]), int(fr["n_bpsc"]), int(fr["n_sym"]), int(fr["n_sym_out"]))


def stream_of(rows):
    """(x, starts): the rows GAP exact zeros apart, GAP zeros behind the last"""
    parts, starts, pos = [], [], 0
    for r in rows:
        parts.append(np.zeros(GAP, np.complex64))
        pos += GAP
        starts.append(pos)
        parts.append(r["samples"])
        pos += r["samples"].size
    parts.append(np.zeros(GAP, np.complex64))
    return np.concatenate(parts), starts
