"""Host-built slots for frame synchronisation (NUMERICS.md rules 6 and 8): one table for
tests/test_lts_rows.py (CPU: the restatement of tests/lts_ref.py against the oracle, the table's conditions, the mutants
of the reference) and tests/test_gpu_lts_rows.py (the device against both, in batches and in streams).

A row is `s` exact zeros, a period-16 burst of 66 samples with integer components (detect_rows.ints_burst, rot 0: A[t] is
a positive integer, cfo_c = +0 and the derotation is the identity) and a crafted content.  Under thr = nextafter(0.75f, 0)
and min_plateau 2 sync_short triggers on the burst's last sample, t = s + 65, so window index m = 0..16 is burst and
m = 17..383 is content[m - 17]: detection is causal, so the content is free.  The content goes on for `tail` samples
behind the window: L = 384 + tail.  In every test the reference decides where the trigger is and what follows, never
these formulas.

Classes and what each row is there for (`want`: conditions asserted on the restatement by tests/test_lts_rows.py):
  ties      windows periodic in 16, 32, 64 and 128 samples: lags 8 k apart read identical floats at identical chain
            positions, so integer magnitudes AND float values tie exactly; the maximum sits in several lanes of the
            kernel's layout (lane = 16 q + col holds lags 8 col + 2 q + 128 (s >> 1) + (s & 1)) and twice in one lane
            `p32rise`: the same with float values that grow with the lag; `lane8`: ties that sit in ONE lane, the one at
            the eighth candidate cut in two and its lag lifted into the top four
  shortcut  an LTS pair 64 apart and a third copy whose integer magnitude is just below / at or above 0.875f times the
            second (the closest ratios a search over integer gains 3..24 found, SHORTCUT_GAINS); leaders 63 / 65 apart;
            near-equal copies where the float ranking ends at another pair than the two leading integer lags
  pair      scaled LTS copies at chosen lags: found 63, 64, 65, 0, a 64 behind a 63, a 65 overridden by a later 63, peaks
            at lag 17 and 319; `few`: one to three valid peaks on the wide path, a valid lag 63 / 64 / 65 away from -1
  cfo       two impulses (A at m0, -A at m0 + 32) meet the LTS's two real taps l[0] = -l[32]: the peak value is real with
            an exact +0 imaginary part; the same figure times g (+-1, +-j) 63 / 64 / 65 further on: arg = +0, +-pi, +-pi/2
            exactly.  The real preamble with the LTS part rotated by nearly +-pi/64 per sample more than the STS part.
  q8        the 8-bit image: a component that rounds to 128, components on k + 0.5, 2^126 next to a burst that quantises
            to 0, Inf / -Inf / NaN in the content and in sample 383 alone, a float magnitude that overflows to +Inf
  edges     slot ends L = 382 / 383 / 384 / 385 (384: the slot ends exactly at t + 368), t = 16 (min_plateau 0, thr 0)

Not reachable through the API.  The first two are checked by tests/test_lts_rows.py::test_what_the_api_cannot_reach; the
last two are argued here, and tests/test_lts_rows.py::test_table_conditions asserts only that no row of the table gets there
(no peak value has a -0 component, no row has Im = -0 beside a positive real part, nothing of a denormal's size decides):
  t = 15     A[n] = sum x[n] conj(x[n - 16]) is 0 for n < 16: the first possible trigger is t = 16 (min_plateau 0)
  the clamp of the scale field at 254 (E < 6, components below 2^-120): |A|^2 of such a burst underflows to 0 and
             `0 > 0` never triggers; the smallest burst that triggers has E about 90
  cfo_fine = -0 from a ZERO imaginary part: both chains of a value start from +0, so a zero component of a peak value is
             +0, and then Im(first conj(second)) = fma(a.im, b.re, -(a.re b.im)) is -0 only together with a negative real
             part, which gives -pi / diff (the rows cfo/fig64/-1/+ and cfo/fig65/-1/+; their partners with the other sign
             give +pi / diff).  -0 is reached all the same, by q8/inf_key: a small negative Im under a real part that
             overflowed to +Inf
  denormal components deciding anything: with E >= 90 the factor is at most 2^43 and a denormal scales to less than 2^-83"""
import functools

import numpy as np

import detect_rows as dr
import lts_ref as ref

THR = dr.NEXT75
MP = 2
S0 = 5                      # leading zeros of a row on its own
LB = 66                     # burst samples: the trigger falls on the last one
SLOT = 640                  # uniform slot of the batch arrangements (rows are padded with zeros in FRONT: L stays)
PUSHES = dr.PUSHES
STREAM_BATCHES = dr.STREAM_BATCHES
GAP = 700                   # exact zeros between the rows of a stream (> 480 + 64: sync_short is back in its first state)

# (g, h): LTS copies of gain g at lags 100 and 164 and one of gain h at lag 250.  Found by `search_shortcut_gains()`:
# the ratio mag1[third] / (0.875f mag1[second]) closest to 1 from below (shortcut) and from above (wide path)
SHORTCUT_GAINS = {"below": (15, 14), "above": (16, 15)}      # ratios 0.99813 and 1.00426


def lts_c64():
    t = ref.taps()[0]
    out = np.zeros(64, np.complex64)
    out.real, out.imag = t[:, 0], t[:, 1]
    return out


def blank(tail):
    return np.zeros(ref.WIN - 17 + tail, np.complex64)


def put(content, lag, samples):
    """add `samples` at window index `lag` (>= 17)"""
    assert lag >= 17
    n = min(len(samples), len(content) - (lag - 17))
    content[lag - 17:lag - 17 + n] += np.asarray(samples, dtype=np.complex64)[:n]
    return content


def copies(spec, tail=80, extra=None):
    """content with g lts at lag p for (p, g) in spec"""
    c = blank(tail)
    for p, g in spec:
        put(c, p, (np.complex64(g) * lts_c64()).astype(np.complex64))
    if extra is not None:
        extra(c)
    return c


def figure(c, m0, amp):
    """the two impulses amp at m0, -amp at m0 + 32 (window indices)"""
    c[m0 - 17] += np.complex64(amp)
    c[m0 + 32 - 17] -= np.complex64(amp)
    return c


def _row(name, cls, content, seed=3, bscale=1.0, thr=THR, mp=MP, f64=True, stream=True, want=None, burst=None, **kw):
    """content None: `burst` is the whole row (the preamble rows)"""
    b = dr.ints_burst(LB, 0, seed) if burst is None else burst
    b = (b * np.float32(bscale)).astype(np.complex64)
    x = b if content is None else np.concatenate([b, np.ascontiguousarray(content, dtype=np.complex64)])
    # ints: the row starts with the 66-sample integer burst, so its trigger is the burst's last sample
    return dict(name=name, cls=cls, samples=x, thr=thr, mp=mp, f64=f64, stream=stream, want=want or {},
                ints=burst is None and (thr, mp) == (THR, MP), **kw)


def slot_of(row, total=None):
    """the row as a slot: zeros in front (S0, or as many as make `total`), burst, content"""
    s = row.get("s", S0) if total is None else total - row["samples"].size
    assert s >= 0
    return np.concatenate([np.zeros(s, np.complex64), row["samples"]])


def search_shortcut_gains(lo=3, hi=24):
    """the CPU search behind SHORTCUT_GAINS (run by hand; tests/test_lts_rows.py checks that the recorded pairs are the
    closest of the range)"""
    best = {"below": (None, 0.0), "above": (None, np.inf)}
    for g in range(lo, hi + 1):
        for h in range(lo, g + 1):
            r = _shortcut_ratio(g, h)
            if r is None:
                continue
            if r < 1 and r > best["below"][1]:
                best["below"] = ((g, h), r)
            if r >= 1 and r < best["above"][1]:
                best["above"] = ((g, h), r)
    return best


def _shortcut_content(g, h):
    return copies([(100, g), (164, g), (250, h)])


def _shortcut_ratio(g, h):
    """float64 quotient of the third integer magnitude and the float32 product 0.875f second, when the leaders are the
    copies at 100 and 164"""
    b = dr.ints_burst(LB, 0, 3)
    c = _shortcut_content(g, h)
    w = np.concatenate([b[LB - 17:], c[:ref.WIN - 17]])
    q = ref.quantise(w.real.copy(), w.imag.copy())[2]
    mag1 = ref.int_magnitudes(q)[0]
    o = sorted(range(ref.SYNC), key=lambda i: (-mag1[i], i))[:3]
    if sorted(o[:2]) != [100, 164]:
        return None
    return float(mag1[o[2]]) / float(np.float32(0.875) * mag1[o[1]])


def _near_equal(seed, amp):
    """four LTS copies, 64 apart in two pairs, gains 8 (1 + amp n): the integer and the float ranking part"""
    rng = np.random.default_rng(seed)
    g = (8 * (1 + amp * rng.standard_normal(4))).astype(np.float32)
    return copies([(30, g[0]), (94, g[1]), (180, g[2]), (244, g[3])])


def _lane8(seed):
    """four LTS copies in one period of 128 samples, at offsets a, a + 64, c, c + 64 with gains 8 (1 + 5e-4 .. 2e-3 n), the
    period repeated over the content: lags 128 apart share a lane of the kernel's layout and tie exactly in the integer
    stage, every tie sits in ONE lane, and the near-equal gains let the float ranking lift the eighth candidate into the
    top four"""
    rng = np.random.default_rng(seed)
    a, c = (int(v) for v in rng.integers(0, 64, 2))
    g = (8 * (1 + rng.uniform(5e-4, 2e-3) * rng.standard_normal(4))).astype(np.float32)
    per = np.zeros(128, np.complex64)
    for off, gg in zip((a, a + 64, c, c + 64), g):
        per += np.roll(np.concatenate([gg * lts_c64(), np.zeros(64, np.complex64)]), off)
    return np.tile(per, 4)[:447]


# seeds (found by trying 0 .. 1499) on which a one-lane tie straddles the eighth candidate AND that lag reaches the top
# four: the first slot of the lane and the last give different records
LANE8_SEEDS = (47, 314, 877)

# (seed, amp).  On the first four (found by trying seeds 0..299) the two leading integer lags are 30 and 94 while the float
# ranking leads with 180 / 244 and the search ends there: the mechanism of the four pinned frames of test_lts_rule6.py
NEAR_EQUAL = ((22, 5e-4), (209, 2e-3), (233, 5e-4), (274, 5e-4), (0, 2e-3), (1, 2e-3))


def _preamble(omega_sts, omega_lts, n):
    """the first n samples of a txgen frame; the phase advances omega_sts per sample up to sample 176 (STS and half of
    the guard interval), omega_lts from there on"""
    f = dr._frame()[:n].astype(np.complex128)
    k = np.arange(f.size)
    ph = np.where(k < 176, omega_sts * k, omega_sts * 176 + omega_lts * (k - 176))
    return (f * np.exp(1j * ph)).astype(np.complex64)


@functools.lru_cache(maxsize=None)
def table():
    rows = []
    lts = lts_c64()
    add = rows.append

    # ---- ties -------------------------------------------------------------------------------------------------------
    for seed in (3, 4):
        whole = dr.ints_burst(LB + 367 + 80, 0, seed)
        add(_row("ties/burst16/%d" % seed, "ties", whole[LB:], seed=seed, f64=False, want=dict(tie_lanes=True, tie_lane=True)))
    for seed in (10, 11, 14, 15, 19):         # (seeds whose largest magnitude is not at a lag that reads the burst)
        rng = np.random.default_rng(seed)
        u = (rng.integers(-8, 9, 32) + 1j * rng.integers(-8, 9, 32)).astype(np.complex64)
        add(_row("ties/p32/%d" % seed, "ties", np.tile(u, 14)[:447], f64=False, want=dict(tie_lanes=True, tie_lane=True)))
    # the same with a rise of 1e-4 over the window: far below half a unit of the 8-bit image, so the integer magnitudes
    # still tie, but the float values grow with the lag: the top four are the HIGHEST four of the eight candidates, and
    # which eight of the ten tied lags stage 1 took shows in the record
    for seed in (10, 11, 14):
        rng = np.random.default_rng(seed)
        u = (rng.integers(-8, 9, 32) + 1j * rng.integers(-8, 9, 32)).astype(np.complex64)
        ramp = (1 + 1e-4 * np.arange(447) / 384).astype(np.float32)
        add(_row("ties/p32rise/%d" % seed, "ties", np.tile(u, 14)[:447] * ramp, f64=False, want=dict(tie_lanes=True, tie_lane=True, rise=True)))
    for seed in LANE8_SEEDS:
        add(_row("ties/lane8/%d" % seed, "ties", _lane8(seed), f64=False, want=dict(tie_lane=True, one_lane_at_8=True, sync=True)))
    for p in (17, 20, 23):
        c = blank(80)
        put(c, p, np.tile(8 * lts, 7))
        add(_row("ties/lts64/%d" % p, "ties", c, f64=False, want=dict(tie_lanes=True, tie_lane=True, sync=True)))
    for p, g1, g2 in ((18, 8, 6), (21, 6, 8), (40, 8, 8)):
        c = blank(80)
        put(c, p, np.tile(np.concatenate([g1 * lts, g2 * lts]), 4))
        add(_row("ties/lts128/%d" % p, "ties", c, f64=False, want=dict(tie_lane=True, sync=True)))

    # ---- shortcut ---------------------------------------------------------------------------------------------------
    for k, (g, h) in SHORTCUT_GAINS.items():
        add(_row("shortcut/%s" % k, "shortcut", _shortcut_content(g, h), want=dict(shortcut=k == "below", sync=True, fs=100)))
    add(_row("shortcut/clear", "shortcut", copies([(100, 8), (164, 8)]), want=dict(shortcut=True, sync=True, fs=100)))
    for d in (63, 65):
        add(_row("shortcut/leaders%d" % d, "shortcut", copies([(100, 8), (100 + d, 8)]), want=dict(shortcut=False, found=d)))
    for seed, amp in NEAR_EQUAL:
        add(_row("shortcut/near/%d" % seed, "shortcut", _near_equal(seed, amp), f64=False, want=dict(shortcut=False, sync=True)))

    # ---- pair search ------------------------------------------------------------------------------------------------
    P = [("pair/64", [(100, 8), (164, 7)], dict(found=64, fs=100)),
         ("pair/63", [(100, 8), (163, 7)], dict(found=63, fs=100)),
         ("pair/65", [(100, 8), (165, 7)], dict(found=65, fs=100)),
         ("pair/none", [(100, 8), (230, 7)], dict(found=0)),
         ("pair/none130", [(60, 8), (190, 7)], dict(found=0)),
         ("pair/64after63", [(100, 8), (163, 7), (164, 6)], dict(found=64, fs=100)),
         ("pair/64after65", [(100, 8), (165, 7), (164, 6)], dict(found=64, fs=100)),
         ("pair/63after65", [(100, 8), (165, 7), (228, 6)], dict(found=63, fs=165)),
         ("pair/65after63", [(100, 8), (163, 7), (228, 6)], dict(found=65, fs=163)),
         ("pair/64first", [(100, 8), (164, 7.9), (227, 7.8)], dict(found=64, fs=100, shortcut=False)),
         ("pair/64low", [(200, 8), (40, 7), (104, 6), (300, 5)], dict(found=64, fs=40)),
         ("pair/lag17", [(17, 8), (81, 8)], dict(found=64, fs=17)),
         ("pair/lag319", [(255, 8), (319, 8)], dict(found=64, fs=255)),
         ("pair/lag319x", [(256, 8), (319, 8)], dict(found=63, fs=256)),
         ("pair/lag17x", [(17, 8), (82, 8)], dict(found=65, fs=17))]
    for name, spec, want in P:
        add(_row(name, "pair", copies(spec), want=want))
    # fewer than four valid peaks ON THE WIDE PATH: one figure of 2^126 at m0 (its eight candidates lie in m0 - 29 .. m0)
    # and a NaN that makes every lag below a block boundary NaN.  E = 255, the valid candidates' magnitudes are +Inf.  The
    # top four are 1 .. 3 valid lags and -1 for the rest, a valid lag sits at 62, 63 or 64 -- 63, 64, 65 away from -1, so a
    # pair search without its `>= 0` test would invent a pair -- and no pair exists
    for m0, nan_at, n_valid in ((62, 50, 2), (63, 50, 2), (64, 50, 3), (64, 60, 1)):
        c = figure(blank(80), m0, 2.0 ** 126)
        c[nan_at - 17] = np.complex64(complex(np.nan, 0))
        add(_row("pair/few/%d/%d" % (m0, nan_at), "pair", c, f64=False, want=dict(found=0, shortcut=False, n_valid=n_valid, valid_at=m0)))

    # ---- fine CFO ---------------------------------------------------------------------------------------------------
    # arg(first conj(second)) in units of pi for second = g first; with g = -1 the sign of the zero imaginary part decides:
    # first > 0 > second gives fma(+0, second.re, -(first.re +0)) = -0 and -pi, first < 0 < second gives +0 and +pi.
    # d = 63: the 64 samples of lag m0 hold the second figure's first impulse (tap 63), so nothing is exact there
    for d in (63, 64, 65):
        for gname, g, arg in (("+1", 0.9375, (0.0, 0.0)), ("-1", -0.9375, (-1.0, 1.0)), ("+j", 0.9375j, (-0.5, -0.5)), ("-j", -0.9375j, (0.5, 0.5))):
            for k, sgn in enumerate((1, -1)):
                c = figure(figure(blank(80), 120, sgn * 64.0), 120 + d, sgn * 64.0 * g)
                want = dict(found=d, fs=120, arg=arg[k]) if d != 63 else {}
                add(_row("cfo/fig%d/%s/%s" % (d, gname, "+-"[k]), "cfo", c, f64=d != 63, want=want))
    c = blank(80)
    put(c, 40, np.concatenate([8 * lts, -8 * lts, 8 * lts, -8 * lts]))
    add(_row("cfo/negated64", "cfo", c, f64=False, want=dict(found=64, pi_abs=True)))
    for k, dw in enumerate((np.pi / 64 * (1 - 1e-4), -np.pi / 64 * (1 - 1e-4), np.pi / 64 * (1 - 1e-2), -np.pi / 64 * (1 - 1e-2),
                            np.pi / 64 * (1 + 1e-2), 0.01)):
        for w0 in (0.0, 0.05):
            add(_row("cfo/preamble/%d/%g" % (k, w0), "cfo", None, burst=_preamble(w0, w0 + dw, 560), want=dict(sync=True, cfo_near=-dw)))

    # ---- the 8-bit image --------------------------------------------------------------------------------------------
    add(_row("q8/round128", "q8", figure(figure(blank(80), 120, 127.75), 184, 127.75 * 0.9375), f64=False,
             want=dict(found=64, fs=120, rint128=True)))
    add(_row("q8/round128neg", "q8", figure(figure(blank(80), 120, -127.75), 184, -127.75 * 0.9375), f64=False,
             want=dict(found=64, fs=120)))
    for k, lag in enumerate((200, 235)):
        # burst components are integers, E = 130 (largest 8): the factor is 8, odd multiples of 1/16 land on k + 0.5
        rng = np.random.default_rng(20 + k)
        n = (2 * rng.integers(-60, 60, 128) + 1 + 1j * (2 * rng.integers(-60, 60, 128) + 1)) / 16.0
        c = copies([(60, 4), (124, 4)])
        put(c, lag, n.astype(np.complex64))
        add(_row("q8/halves/%d" % k, "q8", c, f64=False, want=dict(halves=True)))
    add(_row("q8/huge", "q8", figure(figure(blank(80), 120, 2.0 ** 126), 184, 2.0 ** 126 * 0.9375), f64=False,
             want=dict(burst_q0=True)))
    add(_row("q8/inf_key", "q8", copies([(100, 2.0 ** 59), (164, 2.0 ** 59)]), f64=False, want=dict(inf_key=True, sync=True, fs=100, minus_zero=True)))
    for k, v in enumerate((complex(np.inf, 0), complex(-np.inf, 0), complex(0, np.inf), complex(np.nan, 0), complex(1, np.nan))):
        def bad(c, v=v):
            c[300 - 17] = np.complex64(v)
        add(_row("q8/nonfinite/%d" % k, "q8", copies([(100, 8), (164, 8)], extra=bad), f64=False, want=dict(E255=True)))
    def two(c):
        c[236 - 17] = c[300 - 17] = np.complex64(complex(np.inf, 0))
    add(_row("q8/nonfinite/two", "q8", copies([(100, 8), (164, 8)], extra=two), f64=False, want=dict(E255=True, found=0)))
    # Three equal figures of 2^126 at 120, 184, 248 and a NaN in sample 115.  E = 255: the factor 2^-122 leaves the figures 16.
    # Every lag with a nonzero integer magnitude has a float magnitude of +Inf (a valid key; all tie, the lower lag first)
    # or NaN: the NaN makes lags 48..119 NaN, the first figure's side lobes 91 and 117 among them, and not lag 120 (its
    # chain starts at sample 120).  Candidates: 120, 152, 184, 216, 248 (the figures and the lags between them), 91, 117,
    # 123; without the NaNs the four lowest are 120, 123, 152, 184 and the pair 120 / 184 is found.  With a NaN as a peak
    # 91 and 117 come first and no pair is found; with NaN -> 127 the NaN's own lags fill the candidate list.  The peak
    # values are (x, +0): cfo_fine = atan2(+0, +Inf) = +0; the two LTS windows are equal: no NaN in the record.
    c = figure(figure(figure(blank(80), 120, 2.0 ** 126), 184, 2.0 ** 126), 248, 2.0 ** 126)
    c[115 - 17] = np.complex64(complex(np.nan, 0))
    add(_row("q8/nan_displaces", "q8", c, f64=False, want=dict(E255=True, found=64, fs=120)))
    for k, v in enumerate((complex(np.inf, 0), complex(0, -np.inf), complex(np.nan, 0), complex(0, np.nan))):
        def bad(c, v=v):
            c[383 - 17] = np.complex64(v)
        add(_row("q8/sample383/%d" % k, "q8", copies([(100, 8), (164, 8)], extra=bad), f64=False, want=dict(E255=True, found=0)))
    # 2^120 copies beside an Inf in sample 383: the factor 2^-122 leaves them 2 bits, the pair is still found
    def bad383(c):
        c[383 - 17] = np.complex64(complex(np.inf, 0))
    add(_row("q8/sample383/coarse", "q8", copies([(100, 2.0 ** 58), (164, 2.0 ** 58)], extra=bad383), f64=False, want=dict(E255=True)))
    add(_row("q8/tiny", "q8", copies([(100, 2.0 ** -34), (164, 2.0 ** -34)]), bscale=2.0 ** -37, f64=True, want=dict(sync=True, fs=100)))
    def den(c):
        c[200 - 17:260 - 17] = np.complex64(complex(2.0 ** -140, -2.0 ** -149))
    add(_row("q8/denormal", "q8", copies([(100, 2.0 ** -34), (164, 2.0 ** -34)], extra=den), bscale=2.0 ** -37, f64=True,
             want=dict(sync=True, fs=100)))

    # ---- window edges -----------------------------------------------------------------------------------------------
    for tail in (-2, -1, 0, 1):
        c = copies([(100, 8), (164, 8)], tail=80)[:367 + tail]
        add(_row("edges/L%d" % (384 + tail), "edges", c, want=dict(L=384 + tail)))
        c = copies([(255, 8), (319, 8)], tail=80)[:367 + tail]
        add(_row("edges/L%d/lag319" % (384 + tail), "edges", c, want=dict(L=384 + tail)))
    # t = 16: the burst starts at sample 0, min_plateau 0, thr 0 (c > 0 from sample 16 on); batch only
    for s, mp in ((0, 0), (0, 1), (1, 0)):
        add(_row("edges/t%d/mp%d" % (s + 16 + mp, mp), "edges", copies([(100, 8), (164, 8)], tail=80), thr=0.0, mp=mp, stream=False,
                 burst=dr.ints_burst(17 + mp, 0, 3), s=s, want=dict(t=s + 16 + mp)))
    return rows


def main_rows():
    """the rows of the common handle (thr, min_plateau) = (THR, MP)"""
    return [r for r in table() if (r["thr"], r["mp"]) == (THR, MP)]


_cache = {}


def restate(row, sincos, atan2, mut=(), total=None):
    """the restated record of a row as a slot: detection (tests/detect_ref.py), then tests/lts_ref.py.  Returns the dict
    of lts_ref.frame plus t (-1: no trigger), cfo_c, triggers (all of them, first_only off)"""
    key = (row["name"], tuple(mut), total)
    if key not in _cache:
        import detect_ref
        x = slot_of(row, total)
        with np.errstate(all="ignore"):
            Ar, Ai, P = detect_ref.window_sums(x)
            trig = detect_ref.sync_short(detect_ref.above(Ar, Ai, P, row["thr"])[0], row["mp"])
        if not trig:
            _cache[key] = dict(t=-1, triggers=[], flags=0, frame_start=0, cfo_fine=np.float32(0), cfo_c=np.float32(0))
        else:
            t = trig[0]
            cfo_c = (atan2(Ai[t:t + 1], Ar[t:t + 1]) / np.float32(16)).astype(np.float32)[0]
            f = ref.frame(x, t, cfo_c, sincos, atan2, mut)
            f.update(t=t, cfo_c=cfo_c, triggers=trig)
            _cache[key] = f
    return _cache[key]


def never_slot(n):
    """a burst too short to trigger (60 samples: |A| / P stays below 0.75)"""
    return np.concatenate([np.zeros(n - 60, np.complex64), dr.ints_burst(60, 0, 9)])


def arrangements():
    """(name, list of entries) for the batch tests; an entry is a row, "never" (a slot that never triggers) or "empty" (a
    slot of length 0; the variable-length form only).  Every row stands alone, in table order (the last wave
    is not full), reversed, rotated by 1, 2 and 3 (every row in every row of a wave), and in waves [row, N, N, row] beside
    each kind of neighbour N: both places of a pair, both pairs of a wave."""
    rows = main_rows()
    by = {r["name"]: r for r in rows}
    out = [("alone/" + r["name"], [r]) for r in rows]
    out.append(("order", list(rows)))
    out.append(("reversed", list(rows[::-1])))
    for k in (1, 2, 3):
        out.append(("rotated%d" % k, ["never"] * k + list(rows)))
    for nname, nb in (("shortcut", by["shortcut/clear"]), ("wide", by["shortcut/above"]), ("short", by["edges/L382"]),
                      ("never", "never"), ("empty", "empty")):
        ent = []
        for r in rows:
            ent += [r, nb, nb, r]
        out.append(("beside_" + nname, ent))
    return out


def stream_sets():
    """(name, rows): the rows of the common handle that may stand in a stream, in four streams of 20 000 to 45 000 samples"""
    rows = [r for r in main_rows() if r["stream"] and r["want"].get("L", 384) >= 384]
    sets = [("ties_shortcut", ("ties", "shortcut")), ("pair", ("pair",)), ("cfo", ("cfo",)), ("q8_edges", ("q8", "edges"))]
    return [(n, [r for r in rows if r["cls"] in cl]) for n, cl in sets]


def stream_of(rows, last_L=None):
    """(x, starts): the rows GAP exact zeros apart; last_L: the stream ends where the last row has L = last_L"""
    parts, starts, pos = [], [], 0
    for r in rows:
        parts.append(np.zeros(GAP, np.complex64))
        pos += GAP
        starts.append(pos)
        parts.append(r["samples"])
        pos += r["samples"].size
    x = np.concatenate(parts)
    if last_L is not None:
        x = x[:starts[-1] + LB - 1 - 16 + last_L]        # the last row's trigger is its burst's last sample
    else:
        x = np.concatenate([x, np.zeros(GAP, np.complex64)])
    return x, starts


def restate_stream(x, thr, mp, sincos, atan2):
    """the restated records of a stream: every trigger of sync_short, L = the samples up to the next trigger or the end"""
    import detect_ref
    with np.errstate(all="ignore"):
        Ar, Ai, P = detect_ref.window_sums(x)
        trig = detect_ref.sync_short(detect_ref.above(Ar, Ai, P, thr)[0], mp)
    out = []
    for k, t in enumerate(trig):
        L = x.size - (t - 16)
        if k + 1 < len(trig):
            L = min(L, trig[k + 1] - t)
        cfo_c = (atan2(Ai[t:t + 1], Ar[t:t + 1]) / np.float32(16)).astype(np.float32)[0]
        f = ref.frame(x, t, cfo_c, sincos, atan2, L=min(L, ref.MAX_SAMPLES))
        f.update(t=t, cfo_c=cfo_c)
        out.append(f)
    return out
