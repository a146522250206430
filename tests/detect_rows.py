"""Host-built inputs of the detect phase (NUMERICS.md rule 3 + sync_short), one table for tests/test_detect_rows.py (CPU:
the restatement of tests/detect_ref.py against the oracle, the honesty conditions) and tests/test_gpu_detect_rows.py
(the device against both).

The construction: u[0..15] drawn from {1, j, -1, -j}; a burst is x[s + i] = u[i mod 16] j^(rot (i div 16)), i < Lb, in
exact zeros.  Every product and window sum is a small integer, so A, P, |A|^2 and (thr P)^2 are exact in float32 in any
order of summation: |A| / P = (k + 1) / (17 + k) at sample s + 16 + k (k < 48), exactly 48 / 64 from s + 63 to s + Lb - 1.
thr = 0.75 is never exceeded, nextafter(0.75f, 0) on exactly those Lb - 63 samples, 0.5 from s + 32 on (16 / 32 at s + 31
is the equality case).  `rot` puts A[trigger] on the four half-axes (coarse CFO 0, pi/32, +-pi/16, -pi/32).

Value classes: `unit` (above); `ints` (components integers in +-8: the level varies, the sums stay exact); `floats` (a
periodic-16 burst of random float32 plus weak noise on the burst: the order of summation matters); `preamble` (the
start of a txgen frame in noise at 6 .. 30 dB).  In every test the reference decides, never these formulas.

+-pi: with rot = 2 the imaginary part of A is a sum of exact zeros.  Such a sum is -0 only if every term is -0, and no
choice of signed zeros makes the terms of three consecutive blocks all -0 (fma(xn.im, xd.re, -(xn.re xd.im)) = -0 needs
sign(xn.im) = sign(xn.re) for a sample as x[n] and the opposite for the same sample as x[n - 16]), so an exact zero
gives +pi only.  The `tilt` bursts (u = 1, rot = 2, every sample +- j 2^-100) have Im A = -+2^-99 times the sum of the
burst's block signs over the window: exact, tiny, of the sign the tilt chooses, and the angle is +-pi to the last bit."""
import functools

import numpy as np

PLATEAUS = (0, 1, 2, 3, 15, 16, 17, 31, 32)
NEXT75 = float(np.nextafter(np.float32(0.75), np.float32(0)))
THRS = (0.0, 1e-30, 0.35, 0.5, 0.56, NEXT75, 0.75, 1.0, 1.5, 1e19)
CLASSES = ("unit", "ints", "floats", "preamble")
EXACT = ("unit", "ints")            # classes whose window sums are exact: the float64 definition gives the same bits
SLOT = 1216                         # the edge batches' slot: room for a run across sample 1024
PUSHES = (7, 16, 63, 64, 65, 100, 777, 4096, 0)         # 0: the whole stream in one push
STREAM_BATCHES = (0, 20000)
TILT = 2.0 ** -100

_AXIS = np.array([complex(1, 0), complex(0, 1), complex(-1, 0), complex(0, -1)], dtype=np.complex64)     # every zero component +0


def unit_burst(Lb, rot, seed, tilt=0):
    i = np.arange(Lb)
    if tilt:
        return (_AXIS[(2 * (i // 16)) % 4] + np.complex64(1j * TILT * tilt)).astype(np.complex64)
    ku = np.random.default_rng(seed).integers(0, 4, 16)
    return _AXIS[(ku[i % 16] + rot * (i // 16)) % 4]


def ints_burst(Lb, rot, seed):
    """integer components in +-8.  E = sum |u|^2 is redrawn until 3 E lies in the upper half of its binade: there
    nextafter(0.75f, 0) 4 E = 3 E - E 2^-23 rounds to a float32 strictly below 3 E (E 2^-23 is more than half an ulp of
    3 E exactly when 2 E > 2^floor(log2(3 E))), which is what the float64 definition of the same comparison says; in the
    lower half the float32 product rounds up to 3 E and the comparison is the equality case (a float32 effect the
    `floats` class is there for, not this one)."""
    rng = np.random.default_rng(seed)
    while True:
        re, im = rng.integers(-8, 9, 16), rng.integers(-8, 9, 16)
        E = int((re * re + im * im).sum())
        if (re * re + im * im).min() > 0 and 2 * E > 2 ** int(np.floor(np.log2(3 * E))):
            break
    i = np.arange(Lb)
    k = (rot * (i // 16)) % 4
    r, m = re[i % 16], im[i % 16]
    xr = np.choose(k, [r, -m, -r, m])
    xi = np.choose(k, [m, r, -m, -r])
    out = np.zeros(Lb, np.complex64)
    out.real, out.imag = xr, xi
    return out


def floats_burst(Lb, rot, seed):
    rng = np.random.default_rng(seed)
    u = (rng.standard_normal(16) + 1j * rng.standard_normal(16)) * rng.uniform(0.05, 20)
    i = np.arange(Lb)
    x = u[i % 16] * (1j ** (rot * (i // 16)))
    x = x * (1 + 1e-3 * (rng.standard_normal(Lb) + 1j * rng.standard_normal(Lb)))
    return x.astype(np.complex64)


@functools.lru_cache(maxsize=None)
def _frame():
    from wifirx import txgen
    return txgen.encode_psdus(txgen.make_psdus(1, 40, seed=11), 0).samples[0]


def preamble_burst(Lb, rot, seed):
    """the first Lb samples of a frame (160 of them are the short training sequence), rotated by rot pi / 32 per sample"""
    f = _frame()
    x = np.zeros(Lb, np.complex128)
    m = min(Lb, f.size)
    x[:m] = f[:m]
    return (x * np.exp(1j * rot * np.pi / 32 * np.arange(Lb))).astype(np.complex64)


BURST = {"unit": unit_burst, "ints": ints_burst, "floats": floats_burst, "preamble": preamble_burst}


def place(total, items, cls, noise_seed=None, snr_db=None):
    """zeros [total] with bursts (s, Lb, rot, seed[, tilt]) written in; `preamble`: unit-variance noise everywhere and the
    bursts scaled to snr_db[k mod len]"""
    x = np.zeros(total, np.complex64)
    if cls == "preamble":
        rng = np.random.default_rng(noise_seed)
        x = ((rng.standard_normal(total) + 1j * rng.standard_normal(total)) * np.sqrt(0.5)).astype(np.complex64)
    for k, it in enumerate(items):
        s, Lb, rot, seed = it[:4]
        b = unit_burst(Lb, rot, seed, it[4]) if len(it) > 4 else BURST[cls](Lb, rot, seed)
        b = b[:max(0, total - s)]
        if cls == "preamble":
            x[s:s + b.size] += (b * np.float32(np.sqrt(10 ** (snr_db[k % len(snr_db)] / 10)))).astype(np.complex64)
        else:
            x[s:s + b.size] = b
    return x


SNRS = (6.0, 12.0, 18.0, 24.0, 30.0)


def _edge_items(mp, lim):
    """(s, Lb, rot, seed): runs of exactly mp (no trigger), mp + 1 and mp + 2 samples under nextafter(0.75f, 0), at the starts
    and trigger positions that meet a block, tile and wave-span edge; every burst fits in [0, lim)"""
    out, k = [], 0
    t_targets = [1024, 1024 + max(mp - 1, 0), 64 * 3, 64 * 3 + max(mp - 1, 0), 16 * 20, 16 * 20 + 15, 64 * 5 + mp // 2]
    starts = [0, 1, 15, 16, 17, 100] + [t - 63 - mp for t in t_targets]
    for s in starts:
        for d in (0, 1, 2):
            out.append((s, 63 + mp + d, k % 4, 100 + k))
            k += 1
    out.append((lim - (64 + mp), 64 + mp, 1, 98))          # the run ends on the last sample: a trigger there
    out.append((lim - (63 + mp), 63 + mp, 3, 99))          # one sample short of it
    return out


def _tilt_items(mp):
    """rot = 2 with the tilt of either sign: triggers at t mod 16 = 0, 3, 7, 12, 15, 2, 13, in blocks of either parity"""
    return [(16 * (8 + j) + r - 63 - mp + 64, 64 + mp, 2, 0, 1 - 2 * (j % 2)) for j, r in enumerate((0, 3, 7, 12, 15, 2, 13))]


@functools.lru_cache(maxsize=None)
def batch_rows(mp, cls):
    """list of dict(name, cls, thr, x, and slot_len | off): uniform slots (wifirx_demod_batch) or slots of unequal length
    (wifirx_demod_batch_v: off = n_slots + 1 offsets into x)"""
    rows = []

    def uniform(name, thr, slot_len, slots, **kw):
        x = np.concatenate([place(slot_len, [it] if it else [], cls, noise_seed=7 * mp + k, snr_db=SNRS[k % 5:] + SNRS[:k % 5])
                            for k, it in enumerate(slots)])
        rows.append(dict(name="%s/%s/mp%d/thr%.9g" % (name, cls, mp, thr), cls=cls, thr=thr, x=x, slot_len=slot_len,
                         rots=[it[2] if it else None for it in slots], **kw))

    if cls != "preamble":
        items = _edge_items(mp, SLOT) + (_tilt_items(mp) if cls == "unit" else [])
        # `prefixes`: the batch is also run cut to its first n slots (n_slots 1, 3, 4, 5, 9: full and partly filled waves)
        uniform("edges", NEXT75, SLOT, items, prefixes=(1, 3, 4, 5, 9))
    # every threshold of the list over bursts that end where |A| / P passes 1/17 (thr 0, 1e-30), 16/32 and 48/64
    for thr in THRS:
        lens = [17 + mp, 18 + mp, 32 + mp, 33 + mp, 34 + mp, 63 + mp, 64 + mp, 65 + mp, 200]
        slots = [((5, 40, 100)[k % 3], Lb, k % 4, 300 + k) for k, Lb in enumerate(lens)] + [None]
        if cls == "preamble":
            slots = [(60 + 7 * k, 400, k % 4, 0) for k in range(5)] + [None]
        uniform("thr", thr, 512, slots)
    # one wave: triggers in block 4 and in block 120, a slot that never triggers, a slot of length 0 (thr 0.5: first
    # trigger at s + 32 + mp, so block 4 is reachable for every min_plateau)
    s4, s120 = 64 + 5 - 32 - mp + min(mp // 2, 8), 1920 + 9 - 32 - mp
    parts = [place(2048, [(s4, 300, 1, 5)], cls, 1, SNRS[4:]), place(2048, [(s120, 128, 3, 6)], cls, 2, SNRS[3:]),
             place(2048, [(700, 20, 2, 7)], "unit", 3, SNRS), np.zeros(0, np.complex64)]
    off = np.concatenate([[0], np.cumsum([p.size for p in parts])]).astype(np.uint64)
    rows.append(dict(name="wave4/%s/mp%d" % (cls, mp), cls=cls, thr=0.5, x=np.concatenate(parts), off=off))
    rows.append(dict(name="wave4u/%s/mp%d" % (cls, mp), cls=cls, thr=0.5, x=np.concatenate(parts[:3] + [np.zeros(2048, np.complex64)]),
                     slot_len=2048))
    # one continuous burst cut into slots: the samples behind a slot's end and in front of its start are live
    cuts = [0, 1, 15, 16, 17, 63, 64, 65, 100, 33 + mp, 64 + mp, 63 + mp, 1500]
    off = np.concatenate([[0], np.cumsum(cuts)]).astype(np.uint64)
    for thr in (0.5, NEXT75):
        rows.append(dict(name="cut/%s/mp%d/thr%.9g" % (cls, mp, thr), cls=cls, thr=thr,
                         x=place(int(off[-1]), [(0, int(off[-1]), 1, 9)], cls, 4, SNRS[2:]), off=off))
    return rows


def _aperiodic(n, seed):
    """unit-modulus samples without the period: a burst in power whose |A| / P stays far below every threshold above 0.5"""
    return _AXIS[np.random.default_rng(seed).integers(0, 4, n)]


@functools.lru_cache(maxsize=None)
def stream_rows(mp, cls):
    """list of dict(name, cls, thr, x): streams of at most 60 000 samples"""
    rows = []
    if cls == "unit":
        # main: edge runs, the 480 / 481 pairs, a burst of 1890 samples (a trigger every 481), then one burst in power
        # longer than MAX_SAMPLES + MIN_GAP (its own stream, `expire`) -- a periodic head that triggers, an aperiodic body, a periodic tail whose
        # trigger meets the SEARCH state again (COPY has run out once)
        items, pos = [], 0
        for (s, Lb, rot, seed) in _edge_items(mp, SLOT)[:-2]:
            if s in (15, 16, 100):
                continue                    # (the batch form has them)
            pos = -(-pos // 1024) * 1024 if s > 900 else pos        # trigger positions keep their residues mod 16, 64, 1024
            items.append((pos + s, Lb, rot, seed))
            pos += 1280 if s > 900 else 640
        for it in _tilt_items(mp):
            items.append((pos + it[0],) + it[1:])
            pos += 704
        for gap in (480, 481, 479, 482):
            t1 = pos + 37 + 63 + mp
            items += [(pos + 37, 64 + mp, 1, 40 + gap), (t1 + gap - 63 - mp, 64 + mp, 3, 41 + gap)]
            pos += 1472
        items.append((pos + 11, 1890, 1, 77))
        pos += 1890 + 700
        x = place(pos, items, cls)
        assert 40000 < x.size <= 60000
        rows.append(dict(name="main/unit/mp%d" % mp, cls=cls, thr=NEXT75, x=x, sweep=True))
        head = unit_burst(80 + mp, 1, 78)
        body = _aperiodic(43200 + 480 - head.size + 100, 79)
        tail = unit_burst(200, 3, 80)
        x = np.concatenate([np.zeros(70, np.complex64), head, body, tail, np.zeros(300, np.complex64)])
        assert x.size <= 60000
        rows.append(dict(name="expire/unit/mp%d" % mp, cls=cls, thr=NEXT75, x=x))
    # exact-zero gaps of every length 0 .. 80 between bursts of 64 + mp + (k mod 3) samples
    for thr in (NEXT75, 0.5) if cls in EXACT else (0.56, 0.35):
        items, pos = [], 3
        for g in range(81):
            Lb = (64 + mp + g % 3) if cls != "preamble" else 330
            items.append((pos, Lb, g % 4, 500 + g))
            pos += Lb + g
        rows.append(dict(name="gaps/%s/mp%d/thr%.9g" % (cls, mp, thr), cls=cls, thr=thr,
                         x=place(pos + 100, items, cls, 5, SNRS)))
    # every threshold of the list in stream form: bursts 700 apart that end where |A| / P passes 1/17, 16/32, 48/64
    lens = [17 + mp, 18 + mp, 33 + mp, 34 + mp, 64 + mp, 65 + mp, 600, 63 + mp, 32 + mp]
    items = [(64 * 11 * k + (1, 15, 40)[k % 3], Lb if cls != "preamble" else 400, k % 4, 700 + k) for k, Lb in enumerate(lens)]
    x = place(64 * 11 * len(lens) + 300, items, cls, 6, SNRS)
    for thr in THRS:
        rows.append(dict(name="thr/%s/mp%d/thr%.9g" % (cls, mp, thr), cls=cls, thr=thr, x=x))
    return rows


@functools.lru_cache(maxsize=None)
def switch_stream(mp):
    """the sensitivity switched between pushes: bursts that trigger under 0.5 but not under nextafter(0.75f, 0) (34 + mp
    samples) and bursts that trigger under both, in three parts separated by exact zeros: [0, 9600) bursts, zeros up to
    10 400, bursts up to 12 000, zeros up to 12 800, bursts up to 16 000.  Returns (x, frontier of batch size 5000 = 10 000,
    number of samples pushed before the switch = 16 * 777 = 12 432): both lie more than 256 zeros behind the last burst
    sample and more than 64 in front of the next."""
    items = []
    for k, s in enumerate(list(range(50, 8900, 650)) + list(range(10400, 11600, 650)) + list(range(12800, 15500, 650))):
        items.append((s + k % 17, (34 + mp, 80 + mp, 600)[k % 3], k % 4, 900 + k))
    x = place(16000, items, "unit")
    assert not x[9650:10400].any() and not x[12050:12800].any()
    return x, 10000, 16 * 777


def slots_of(row):
    """the slots of a batch row as a list of sample arrays"""
    x = row["x"]
    if "off" in row:
        return [x[int(a):int(b)] for a, b in zip(row["off"][:-1], row["off"][1:])]
    return list(x.reshape(-1, row["slot_len"]))
