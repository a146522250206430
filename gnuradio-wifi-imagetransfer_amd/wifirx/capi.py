"""ctypes binding of libwifirx.so (include/wifirx.h) -- the product's only compute path.

There is no CPU fallback: importing works everywhere (so that the ABI can be inspected on a
CPU-only box), but creating a :class:`WifiRx` raises :class:`WifiRxError` unless a gfx950 GPU
is usable, and a missing ``libwifirx.so`` raises at import of this module.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("WIFIRX_LIB") or os.path.join(_HERE, "libwifirx.so")     # WIFIRX_LIB: A/B builds

ABI_VERSION = 4
DECODE_INPUT = "planes"      # what demod_batch(decode=True) hands decode_mac: "planes" (wifirx_out.hbits) or "idx"
EQ_LS, EQ_LMS, EQ_COMB, EQ_STA = 0, 1, 2, 3
OK, EINVAL, ENODEV, ENOMEM, EHIP, ERANGE, EDEAD = 0, -1, -2, -3, -4, -5, -6      # WIFIRX_E*; EDEAD: the stream is dead, do not retry
STREAM_BATCH_MAX = 1 << 27          # WIFIRX_STREAM_BATCH_MAX
P_BANDWIDTH, P_FREQUENCY, P_SENSITIVITY, P_CHAN_EST, P_STREAM_BATCH, P_DECODE_SMALL_MAX, P_LLR_CSI, P_STREAM_IDX = 1, 2, 3, 4, 5, 6, 7, 8
P_STREAM_SOFT = 9                   # stream mode: decode_mac on LLRs (wifirx_decode_batch_soft, NUMERICS.md rule 14)
P_LLR_FORMAT = 10                   # LLR format of the batch calls (NUMERICS.md rule 15); stream mode keeps float32
LLR_F32, LLR_BF16 = 0, 1            # WIFIRX_LLR_*
_LLR_FORMATS = {"f32": LLR_F32, "bf16": LLR_BF16}
IQ_FC32, IQ_SC16, IQ_SC8 = 0, 1, 2  # WIFIRX_IQ_*: sample formats (NUMERICS.md rule 20)
IQ_FORMATS = {"fc32": IQ_FC32, "sc16": IQ_SC16, "sc8": IQ_SC8}
IQ_DTYPE = {IQ_FC32: np.dtype(np.complex64), IQ_SC16: np.dtype(np.int16), IQ_SC8: np.dtype(np.int8)}     # sc16 / sc8: two items per sample
IQ_SCALE = {IQ_FC32: 1.0, IQ_SC16: 2.0 ** -15, IQ_SC8: 2.0 ** -7}      # the conventional widening scales
IQ_MAX_BITS = {IQ_SC16: 16, IQ_SC8: 8}
F_DETECTED, F_SYNC, F_SIGNAL, F_COMPLETE, F_LLR, F_DECODED, F_CRC_OK = 1, 2, 4, 8, 16, 32, 64

FRAME_DTYPE = np.dtype([
    ("flags", "<u4"), ("trigger", "<i4"), ("frame_start", "<i4"),
    ("cfo_coarse", "<f4"), ("cfo_fine", "<f4"), ("snr_db", "<f4"),
    ("psdu_len", "<u2"), ("encoding", "u1"), ("n_bpsc", "u1"),
    ("n_sym", "<u2"), ("n_sym_out", "<u2"),
])
assert FRAME_DTYPE.itemsize == 32

EXPORTS = [
    "wifirx_create", "wifirx_destroy", "wifirx_last_error", "wifirx_abi_version", "wifirx_set_param",
    "wifirx_get_stats", "wifirx_demod_batch", "wifirx_decode_batch", "wifirx_push", "wifirx_poll", "wifirx_poll_csi",
    "wifirx_sync", "wifirx_stream", "wifirx_synth_slots", "wifirx_dev_alloc", "wifirx_dev_free",
    "wifirx_memcpy_h2d", "wifirx_memcpy_d2h", "wifirx_time_demod", "wifirx_poll_ex", "wifirx_demod_batch_v",
    "wifirx_push_consumed", "wifirx_queued", "wifirx_decode_batch_soft", "wifirx_tx_batch", "wifirx_channel",
    "wifirx_mac_batch", "wifirx_link_stats", "wifirx_tx_batch_rates", "wifirx_link_stats_by_rate",
    "wifirx_channel_sro", "wifirx_resampler_table", "wifirx_channel_fading",
    "wifirx_iq_to_f32", "wifirx_iq_from_f32", "wifirx_push_iq",
    "wifirx_channelize", "wifirx_channelizer_table", "wifirx_combine", "wifirx_diversity_combine",
    "wifirx_push_diversity", "wifirx_poll_diversity", "wifirx_detect_multi", "wifirx_irs_taps", "wifirx_irs_sweep",
    "wifirx_irs_taps_multi", "wifirx_irs_sweep_multi", "wifirx_irs_estimate", "wifirx_irs_optimize",
    "wifirx_irs_optimize_weighted",
    "wifirx_frontend", "wifirx_frontend_estimate", "wifirx_rx_impair", "wifirx_stream_frontend", "wifirx_stream_frontend_state",
    "wifirx_precombine",
    "wifirx_arb_resample", "wifirx_arb_hist", "wifirx_arb_count", "wifirx_arb_table",
    "wifirx_tune", "wifirx_tune_inc",
    "wifirx_spectrum", "wifirx_spectrum_count", "wifirx_spectrum_fold", "wifirx_spectrum_bands", "wifirx_spectrum_band",
    "wifirx_spectrum_table",
]
FE_DC, FE_IQ = 1, 2                 # WIFIRX_FE_*: stages of the receive front end (NUMERICS.md rule 32)
FE_BLOCK, FE_RING = 4096, 64        # WIFIRX_FE_BLOCK, WIFIRX_FE_RING
# wifirx_frontend_state as a NumPy record (2632 bytes; np.zeros((), FE_STATE_DTYPE) is a fresh stream)
FE_STATE_DTYPE = np.dtype([("n", "<u8"), ("part", "<i8", (5,)), ("ring", "<i8", (FE_RING, 5)), ("d0", "<i8", (2,)), ("w0", "<f4", (2,))])
assert FE_STATE_DTYPE.itemsize == 2632
DIV_MRC, DIV_SELECT = 0, 1          # WIFIRX_DIV_*: modes of wifirx_diversity_combine (NUMERICS.md rule 23)
DIV_MODES = {"mrc": DIV_MRC, "select": DIV_SELECT}
DIV_MAX_ANT = 8
PRE_MAX_ANT, PRE_MAX_ITERS = 8, 4   # wifirx_precombine: antennas, power iterations (NUMERICS.md rule 33)
PRE_DEGENERATE = 1                  # WIFIRX_PRE_DEGENERATE: the slot's y is antenna 0's samples
# one stats row of wifirx_precombine
PRE_STATS_DTYPE = np.dtype([("lambda", "<f4"), ("trace", "<f4"), ("ref", "<u4"), ("flags", "<u4")])
assert PRE_STATS_DTYPE.itemsize == 16
CHANNELIZER_CHANNELS = (2, 4, 8)    # wifirx_channelize: n_channels (NUMERICS.md rule 21)
CHANNELIZER_HIST = 23               # input blocks of n_channels samples that a call takes from before its input
ARB_HIST_MAX = 128                  # WIFIRX_ARB_HIST_MAX: the most samples wifirx_arb_resample takes from before its input
ARB_MAX_DEN, ARB_MAX_NUM, ARB_MAX_RATIO = 512, 2048, 4      # the limits of a reduced ratio (NUMERICS.md rule 34)
TUNE_MAX_CHANNELS = 8               # WIFIRX_TUNE_MAX_CHANNELS: the most channels of one wifirx_tune call (NUMERICS.md rule 35)
# wifirx_spectrum (NUMERICS.md rule 36): WIFIRX_SPEC_*
SPEC_RECT, SPEC_HANN, SPEC_BLACKMAN_HARRIS = 0, 1, 2
SPEC_WINDOWS = {"rect": SPEC_RECT, "hann": SPEC_HANN, "blackman_harris": SPEC_BLACKMAN_HARRIS}
SPEC_SUM, SPEC_MAX = 0, 1
SPEC_MODES = {"sum": SPEC_SUM, "max": SPEC_MAX}
SPEC_MAX_BANDS, SPEC_MAX_HOP, SPEC_N_FFT = 16, 1 << 20, (64, 256, 1024, 4096)
MAX_PAYLOAD = 1500                  # WIFIRX_MAX_PSDU - 28: the longest payload wifirx_mac_batch frames


def bf16_to_f32(bits) -> np.ndarray:
    """bf16 bit patterns (np.uint16, as the batch calls return them with llr_format="bf16") -> the float32 values they
    stand for: exact, the 16 bits become the upper half of the float32 word"""
    b = np.asarray(bits, dtype=np.uint16)
    return (b.astype(np.uint32) << 16).view(np.float32)


def phase_inc(cfo) -> int:
    """The uint64 phase increment wifirx_channel derives from `cfo` rad/sample (taken as float32): llround(cfo / (2 pi) * 2^64)
    with the turns reduced to [-1/2, 1/2] first (+-1/2 turn = 2^63).  A caller that cuts a stream into calls advances its
    phase0 by phase_inc(cfo) * samples, mod 2^64."""
    f = float(np.float32(cfo)) / 6.283185307179586
    f -= float(np.rint(f))
    v = f * 2.0 ** 64
    if v >= 2.0 ** 63 or v <= -2.0 ** 63:
        return 1 << 63
    a = abs(v)
    k = int(a) if a >= 2.0 ** 52 else int(np.floor(a + 0.5))      # llround: half away from zero (a + 0.5 is exact below 2^52)
    return (-k if v < 0 else k) & 0xFFFFFFFFFFFFFFFF


SRO_MAX = 2.0 ** -8                 # the largest |sro| wifirx_channel_sro takes


def drift_inc(sro) -> int:
    """The int64 drift increment wifirx_channel_sro derives from `sro` = epsilon - 1 (taken as float32): llround(sro * 2^40),
    in 2^-40 samples per sample (NUMERICS.md rule 18).  A caller that cuts a stream into calls advances its drift0 by
    drift_inc(sro) * samples."""
    v = float(np.float32(sro)) * 2.0 ** 40      # exact: a float32 times a power of two
    a = abs(v)
    k = int(a) if a >= 2.0 ** 52 else int(np.floor(a + 0.5))      # llround: half away from zero
    return -k if v < 0 else k


def locked_sro(cfo, bandwidth=20e6, frequency=5.89e9):
    """sro of a sample clock locked to the carrier, for `cfo` rad/sample as wifirx_channel applies it (exp(+j cfo n)):
    epsilon - 1 = -cfo * bw / (2 pi fc), the offset the receiver's frame_equalizer compensates (float32 array or scalar)"""
    return (-np.asarray(cfo, dtype=np.float64) * bandwidth / (2 * np.pi * frequency)).astype(np.float32)


DOPPLER_MAX = 2.0 ** -10            # the largest doppler (cycles per sample) wifirx_channel_fading takes
FADE_MAX_TAPS = 16                  # the most taps with fading
IRS_MAX_ELEMS, IRS_MAX_TAPS = 4096, 16      # wifirx_irs_taps: the most surface elements and taps (NUMERICS.md rule 25)
IRS_MAX_CODES = 1024                        # wifirx_irs_sweep: the most codebook entries (NUMERICS.md rule 26)
IRS_MAX_ANT = 8                             # wifirx_irs_taps_multi / _sweep_multi: the most AP antennas (NUMERICS.md rule 27)
IRS_MAX_PILOTS, IRS_MAX_GROUPS = 1024, 1023 # wifirx_irs_estimate: the most pilot slots and element groups (NUMERICS.md rule 29)
IRS_MAX_ROWS, IRS_MAX_SWEEPS = 128, 16      # wifirx_irs_optimize: the most rows of a set and sweeps (NUMERICS.md rule 30)
IRS_START_REF, IRS_START_GIVEN, IRS_START_ZERO = 0, 1, 2    # WIFIRX_IRS_START_*
IRS_STARTS = {"ref": IRS_START_REF, "given": IRS_START_GIVEN, "zero": IRS_START_ZERO}


def resampler_table() -> np.ndarray:
    """wifirx_resampler_table: the rule-18 table as float32 [n_phases + 1, n_taps] (a copy; no handle, no device)"""
    p, n_ph, n_t = C.POINTER(C.c_float)(), C.c_uint32(), C.c_uint32()
    rc = _lib.wifirx_resampler_table(C.byref(p), C.byref(n_ph), C.byref(n_t))
    if rc != OK:
        raise WifiRxError(rc, "wifirx_resampler_table")
    return np.ctypeslib.as_array(p, shape=(n_ph.value + 1, n_t.value)).copy()


def channelizer_table(n_channels) -> np.ndarray:
    """wifirx_channelizer_table: the rule-21 prototype as float32 [24 * n_channels] (a copy; no handle, no device)"""
    p, n = C.POINTER(C.c_float)(), C.c_uint32()
    rc = _lib.wifirx_channelizer_table(int(n_channels), C.byref(p), C.byref(n))
    if rc != OK:
        raise WifiRxError(rc, "wifirx_channelizer_table: n_channels must be 2, 4 or 8")
    return np.ctypeslib.as_array(p, shape=(n.value,)).copy()


def arb_table() -> np.ndarray:
    """wifirx_arb_table: the rule-34 prototype as float32 [4097], 128 entries per unit (a copy; no handle, no device)"""
    p, n, per = C.POINTER(C.c_float)(), C.c_uint32(), C.c_uint32()
    rc = _lib.wifirx_arb_table(C.byref(p), C.byref(n), C.byref(per))
    if rc != OK:
        raise WifiRxError(rc, "wifirx_arb_table")
    return np.ctypeslib.as_array(p, shape=(n.value,)).copy()


def arb_ratio(rate_in, rate_out):
    """(num, den) of wifirx_arb_resample for a stream at rate_in Hz brought to rate_out Hz: the rounded Hz values in lowest
    terms.  ValueError outside 1 <= den <= 512, 1 <= num <= 2048, 1/4 <= num / den <= 4."""
    from fractions import Fraction
    a, b = int(round(float(rate_in))), int(round(float(rate_out)))
    if a <= 0 or b <= 0:
        raise ValueError("sample rates must be positive")
    f = Fraction(a, b)
    num, den = f.numerator, f.denominator
    if den > ARB_MAX_DEN or num > ARB_MAX_NUM or num > ARB_MAX_RATIO * den or den > ARB_MAX_RATIO * num:
        raise ValueError("%g Hz -> %g Hz is the ratio %d/%d: outside den <= %d, num <= %d, 1/%d <= num/den <= %d"
                         % (rate_in, rate_out, num, den, ARB_MAX_DEN, ARB_MAX_NUM, ARB_MAX_RATIO, ARB_MAX_RATIO))
    return num, den


def arb_hist(num, den) -> int:
    """wifirx_arb_hist: HL = ceil(32 max(num, den) / den) of the reduced ratio (no handle, no device)"""
    n = C.c_uint32()
    rc = _lib.wifirx_arb_hist(int(num), int(den), C.byref(n))
    if rc != OK:
        raise WifiRxError(rc, "wifirx_arb_hist: ratio outside the limits")
    return int(n.value)


def arb_count(num, den, j0, n_in, m0) -> int:
    """wifirx_arb_count: the outputs a wifirx_arb_resample call makes (host integers only; no handle, no device)"""
    n = C.c_uint64()
    rc = _lib.wifirx_arb_count(int(num), int(den), int(j0), int(n_in), int(m0), C.byref(n))
    if rc != OK:
        raise WifiRxError(rc, "wifirx_arb_count: ratio outside the limits" if rc == EINVAL else "wifirx_arb_count: index out of range")
    return int(n.value)


def arb_flush_inputs(num, den, n_in, n_out) -> int:
    """the fewest zeros behind the n_in inputs of a stream with which it yields n_out outputs (the end-of-stream flush)"""
    from math import gcd
    g = gcd(int(num), int(den))
    num, den = int(num) // g, int(den) // g
    S = max(num, den)
    return max(0, ((int(n_out) - 1) * num + 16 * S) // den + 1 - int(n_in)) if n_out > 0 else 0       # m_end(E) >= n_out


def tune_inc(offset_hz, sample_rate) -> int:
    """wifirx_tune_inc: the uint64 phase increment per input sample (2^-64 turns) that brings a channel whose centre lies
    offset_hz above the capture's centre down to 0 (no handle, no device).  A caller advances nothing: wifirx_tune forms the
    phase from the stream index."""
    v = C.c_uint64()
    rc = _lib.wifirx_tune_inc(float(offset_hz), float(sample_rate), C.byref(v))
    if rc != OK:
        raise WifiRxError(rc, "wifirx_tune_inc: offset_hz must be finite, sample_rate finite and > 0")
    return int(v.value)


def spectrum_count(n_fft, hop, avg, n_in):
    """wifirx_spectrum_count: (n_rows, consumed) of a wifirx_spectrum call on n_in samples (host integers only)"""
    r, c = C.c_uint64(), C.c_uint64()
    rc = _lib.wifirx_spectrum_count(int(n_fft), int(hop), int(avg), int(n_in), C.byref(r), C.byref(c))
    if rc != OK:
        raise WifiRxError(rc, "wifirx_spectrum_count: n_fft must be 64, 256, 1024 or 4096, hop and avg 1 .. 2^20, n_in < 2^62")
    return int(r.value), int(c.value)


def spectrum_band(offset_hz, width_hz, sample_rate, n_fft):
    """wifirx_spectrum_band: (lo, hi), the bins of a row whose centres lie in [offset - width / 2, offset + width / 2)"""
    lo, hi = C.c_uint32(), C.c_uint32()
    rc = _lib.wifirx_spectrum_band(float(offset_hz), float(width_hz), float(sample_rate), int(n_fft), C.byref(lo), C.byref(hi))
    if rc != OK:
        raise WifiRxError(rc, "wifirx_spectrum_band: the band holds no bin or leaves the capture" if rc == ERANGE
                          else "wifirx_spectrum_band: values must be finite, sample_rate and width_hz > 0, n_fft 64, 256, 1024 or 4096")
    return int(lo.value), int(hi.value)


def spectrum_table():
    """wifirx_spectrum_table: (hann float32 [4096], blackman_harris float32 [4096], twiddle float32 [4096, 2]) of rule 36
    (copies; no handle, no device)"""
    hn, bh, tw, n = C.POINTER(C.c_float)(), C.POINTER(C.c_float)(), C.POINTER(C.c_float)(), C.c_uint32()
    rc = _lib.wifirx_spectrum_table(C.byref(hn), C.byref(bh), C.byref(tw), C.byref(n))
    if rc != OK:
        raise WifiRxError(rc, "wifirx_spectrum_table")
    k = n.value
    return (np.ctypeslib.as_array(hn, shape=(k,)).copy(), np.ctypeslib.as_array(bh, shape=(k,)).copy(),
            np.ctypeslib.as_array(tw, shape=(k, 2)).copy())


def channel_centre(k, n_channels, stacking) -> float:
    """f_k of wifirx_channelize in cycles per input sample; times n_channels * bandwidth it is the channel's offset in Hz"""
    return (k + stacking / 2.0 - n_channels / 2.0) / n_channels


def link_rates(c) -> dict:
    """fer, coded_ber and coded_ber_se (float64) from the counters of wifirx_link_counts.  coded_ber_se is the standard error
    of the mean of the per-frame BER e_f / b over the good frames, b = coded_bits / frames_good bits per frame (frames of
    one length): sqrt(E[e^2] - E[e]^2) / b / sqrt(frames_good)."""
    nan = float("nan")
    g, bits = c["frames_good"], c["coded_bits"]
    out = {"fer": 1.0 - c["frames_psdu_ok"] / c["frames_ref"] if c["frames_ref"] else nan,
           "coded_ber": c["coded_bit_errors"] / bits if bits else nan, "coded_ber_se": nan}
    if g and bits:
        m1, m2 = c["coded_bit_errors"] / g, c["coded_bit_errors_sq"] / g
        out["coded_ber_se"] = float(np.sqrt(max(m2 - m1 * m1, 0.0)) / (bits / g) / np.sqrt(g))
    return out


class WifiRxError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("wifirx error %d: %s" % (code, msg))
        self.code = code


class Config(C.Structure):
    _fields_ = [("abi_version", C.c_uint32), ("device", C.c_int32), ("bandwidth", C.c_double),
                ("frequency", C.c_double), ("sensitivity", C.c_float), ("min_plateau", C.c_int32),
                ("chan_est", C.c_int32), ("max_sym", C.c_uint32), ("llr_bits", C.c_uint32),
                ("want_carrier", C.c_uint32), ("max_batch", C.c_uint32), ("max_slot_len", C.c_uint32)]


class Out(C.Structure):
    _fields_ = [("frames", C.c_void_p), ("idx", C.c_void_p), ("llr", C.c_void_p), ("carrier", C.c_void_p),
                ("psdu", C.c_void_p), ("psdu_stride", C.c_uint32), ("on_device", C.c_uint32), ("csi", C.c_void_p),
                ("sym_stats", C.c_void_p), ("hbits", C.c_void_p)]


class PollOut(C.Structure):
    _fields_ = [("frames", C.c_void_p), ("psdu", C.c_void_p), ("psdu_stride", C.c_uint32), ("reserved", C.c_uint32),
                ("idx", C.c_void_p), ("carrier", C.c_void_p), ("csi", C.c_void_p), ("sym_stats", C.c_void_p)]


class DivStream(C.Structure):
    """wifirx_div_stream: what a wifirx_push_diversity call says about its antennas"""
    _fields_ = [("n_ant", C.c_uint32), ("mode", C.c_int), ("ant_gain", C.POINTER(C.c_float)), ("fmt", C.c_int),
                ("scale", C.c_float), ("iq_on_device", C.c_int)]


class FrontendCfg(C.Structure):
    """wifirx_frontend_cfg"""
    _fields_ = [("flags", C.c_uint32), ("frac_bits", C.c_uint32), ("dc_shift", C.c_uint32), ("iq_shift", C.c_uint32)]


def frontend_cfg(dc=True, iq=False, frac_bits=12, dc_shift=2, iq_shift=4) -> FrontendCfg:
    """a wifirx_frontend_cfg with rule 32's defaults: the DC stage on, the blind IQ stage off"""
    return FrontendCfg((FE_DC if dc else 0) | (FE_IQ if iq else 0), int(frac_bits), int(dc_shift), int(iq_shift))


def frontend_state(d0=0j, w0=0j, frac_bits=12) -> np.ndarray:
    """a fresh wifirx_frontend_state (a FE_STATE_DTYPE record) whose block 0 is corrected with offset d0 and coefficient w0"""
    st = np.zeros((), FE_STATE_DTYPE)
    st["d0"] = [int(np.rint(np.real(d0) * 2.0 ** frac_bits)), int(np.rint(np.imag(d0) * 2.0 ** frac_bits))]
    st["w0"] = [np.real(w0), np.imag(w0)]
    return st


def iq_imbalance(gain_db=0.0, phase_deg=0.0):
    """(mu, nu) of a receiver whose Q branch has gain g = 10^(gain_db / 20) and phase error phi against I:
    mu = (1 + g e^{-j phi}) / 2, nu = (1 - g e^{j phi}) / 2; the receiver delivers mu x + nu conj(x)"""
    g, phi = 10.0 ** (gain_db / 20.0), np.deg2rad(phase_deg)
    return complex((1 + g * np.exp(-1j * phi)) / 2), complex((1 - g * np.exp(1j * phi)) / 2)


class Stats(C.Structure):
    _fields_ = [("samples_in", C.c_uint64), ("frames_detected", C.c_uint64), ("frames_signal_ok", C.c_uint64),
                ("frames_complete", C.c_uint64), ("frames_crc_ok", C.c_uint64), ("frames_dropped", C.c_uint64)]


class LinkCounts(C.Structure):
    """wifirx_link_counts: what wifirx_link_stats counts"""
    _fields_ = [(k, C.c_uint64) for k in ("frames", "frames_ref", "frames_good", "frames_crc_ok", "frames_psdu_ok",
                                          "frames_crc_ok_wrong", "coded_bits", "coded_bit_errors", "coded_bit_errors_sq")]


if not os.path.exists(LIB_PATH):
    raise ImportError("libwifirx.so is missing (%s): build it with `python __graft_entry__.py` or "
                      "`make -C gnuradio-wifi-imagetransfer_amd/csrc`; there is no CPU fallback" % LIB_PATH)

_lib = C.CDLL(LIB_PATH)
_lib.wifirx_last_error.restype = C.c_char_p
_lib.wifirx_last_error.argtypes = [C.c_void_p]
_lib.wifirx_stream.restype = C.c_void_p
_lib.wifirx_stream.argtypes = [C.c_void_p]
_lib.wifirx_create.argtypes = [C.POINTER(Config), C.POINTER(C.c_void_p)]
_lib.wifirx_destroy.argtypes = [C.c_void_p]
_lib.wifirx_set_param.argtypes = [C.c_void_p, C.c_int, C.c_double]
_lib.wifirx_get_stats.argtypes = [C.c_void_p, C.POINTER(Stats)]
_lib.wifirx_demod_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_uint32, C.c_uint32, C.POINTER(Out)]
_lib.wifirx_decode_batch.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(Out)]
_lib.wifirx_decode_batch_soft.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(Out)]
_lib.wifirx_demod_batch_v.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.POINTER(Out)]
_lib.wifirx_push.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
_lib.wifirx_push_consumed.restype = C.c_size_t
_lib.wifirx_queued.restype = C.c_uint32
_lib.wifirx_queued.argtypes = [C.c_void_p]
_lib.wifirx_push_consumed.argtypes = [C.c_void_p]
_lib.wifirx_poll.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p,
                             C.c_uint32, C.POINTER(C.c_uint32)]
_lib.wifirx_poll_csi.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_uint32, C.POINTER(C.c_uint32)]
_lib.wifirx_poll_ex.argtypes = [C.c_void_p, C.POINTER(PollOut), C.c_uint32, C.POINTER(C.c_uint32)]
_lib.wifirx_sync.argtypes = [C.c_void_p]
_lib.wifirx_synth_slots.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_uint32, C.c_uint32, C.c_void_p,
                                    C.c_uint32, C.c_uint32, C.c_uint32, C.c_float, C.c_float, C.c_uint64,
                                    C.c_void_p]
_lib.wifirx_tx_batch.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p,
                                 C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32]
_lib.wifirx_tx_batch_rates.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p,
                                       C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32]
_lib.wifirx_channel.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32,
                                C.c_void_p, C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64, C.c_float, C.c_float,
                                C.c_uint64, C.c_uint64]
_lib.wifirx_channel_sro.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32,
                                    C.c_void_p, C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_int64,
                                    C.c_float, C.c_float, C.c_uint64, C.c_uint64]
_lib.wifirx_channel_fading.argtypes = _lib.wifirx_channel_sro.argtypes + [C.c_void_p, C.c_float, C.c_uint64, C.c_uint64]
_lib.wifirx_irs_taps.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_float, C.c_uint32, C.c_void_p,
                                 C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_void_p, C.c_int, C.c_uint32, C.c_uint32,
                                 C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p]
_lib.wifirx_irs_sweep.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_float, C.c_uint32, C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_void_p, C.c_int, C.c_uint32,
                                  C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p]
_lib.wifirx_irs_taps_multi.argtypes = _lib.wifirx_irs_taps.argtypes[:2] + [C.c_uint32] + _lib.wifirx_irs_taps.argtypes[2:]
_lib.wifirx_irs_sweep_multi.argtypes = _lib.wifirx_irs_sweep.argtypes[:2] + [C.c_uint32] + _lib.wifirx_irs_sweep.argtypes[2:]
_lib.wifirx_irs_estimate.argtypes = _lib.wifirx_irs_taps_multi.argtypes[:13] + [
    C.c_void_p, C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_float, C.c_float, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p,
    C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
_lib.wifirx_irs_optimize.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int,
                                     C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
_lib.wifirx_irs_optimize_weighted.argtypes = _lib.wifirx_irs_optimize.argtypes[:5] + [C.c_void_p, C.c_int, C.c_uint32] + \
    _lib.wifirx_irs_optimize.argtypes[5:]
_lib.wifirx_resampler_table.argtypes = [C.POINTER(C.POINTER(C.c_float)), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
_lib.wifirx_mac_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32,
                                  C.c_uint64, C.c_void_p, C.c_uint32]
_lib.wifirx_link_stats.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(Out), C.POINTER(Out), C.c_void_p, C.c_void_p,
                                   C.POINTER(LinkCounts)]
_lib.wifirx_link_stats_by_rate.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(Out), C.POINTER(Out), C.c_void_p, C.c_void_p,
                                           C.POINTER(LinkCounts), C.POINTER(LinkCounts)]
_lib.wifirx_iq_to_f32.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_uint64, C.c_float, C.c_void_p]
_lib.wifirx_iq_from_f32.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_float, C.c_int, C.c_uint32, C.c_void_p,
                                    C.POINTER(C.c_uint64)]
_lib.wifirx_push_iq.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_float, C.c_int]
_lib.wifirx_frontend.argtypes = [C.c_void_p, C.POINTER(FrontendCfg), C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_uint64, C.c_void_p]
_lib.wifirx_frontend_estimate.argtypes = [C.POINTER(FrontendCfg), C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]
_lib.wifirx_rx_impair.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_float), C.POINTER(C.c_float),
                                  C.POINTER(C.c_float)]
_lib.wifirx_stream_frontend.argtypes = [C.c_void_p, C.POINTER(FrontendCfg), C.c_void_p]
_lib.wifirx_stream_frontend_state.argtypes = [C.c_void_p, C.c_void_p]
_lib.wifirx_channelize.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int,
                                   C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64]
_lib.wifirx_channelizer_table.argtypes = [C.c_uint32, C.POINTER(C.POINTER(C.c_float)), C.POINTER(C.c_uint32)]
_lib.wifirx_combine.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_float), C.c_void_p, C.c_void_p, C.c_uint32,
                                C.c_int, C.c_uint64, C.c_uint64, C.c_void_p]
_lib.wifirx_arb_resample.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32,
                                     C.c_uint32, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
_lib.wifirx_arb_hist.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]
_lib.wifirx_arb_count.argtypes = [C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64)]
_lib.wifirx_arb_table.argtypes = [C.POINTER(C.POINTER(C.c_float)), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
_lib.wifirx_tune.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32,
                             C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_uint64, C.c_uint64, C.c_void_p,
                             C.c_uint64, C.POINTER(C.c_uint64)]
_lib.wifirx_tune_inc.argtypes = [C.c_double, C.c_double, C.POINTER(C.c_uint64)]
_lib.wifirx_spectrum.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int,
                                 C.c_int, C.c_float, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
_lib.wifirx_spectrum_count.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
_lib.wifirx_spectrum_fold.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint64, C.c_int, C.c_void_p, C.c_uint64,
                                      C.POINTER(C.c_uint64)]
_lib.wifirx_spectrum_bands.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32),
                                       C.POINTER(C.c_uint32), C.c_void_p]
_lib.wifirx_spectrum_band.argtypes = [C.c_double, C.c_double, C.c_double, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
_lib.wifirx_spectrum_table.argtypes = [C.POINTER(C.POINTER(C.c_float)), C.POINTER(C.POINTER(C.c_float)),
                                       C.POINTER(C.POINTER(C.c_float)), C.POINTER(C.c_uint32)]
_lib.wifirx_diversity_combine.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(Out), C.c_uint32, C.c_int, C.POINTER(C.c_float),
                                          C.POINTER(Out), C.c_void_p]
_lib.wifirx_precombine.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p), C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p,
                                   C.c_void_p, C.c_void_p]
_lib.wifirx_push_diversity.argtypes = [C.c_void_p, C.POINTER(DivStream), C.POINTER(C.c_void_p), C.c_size_t]
_lib.wifirx_poll_diversity.argtypes = [C.c_void_p, C.POINTER(PollOut), C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
_lib.wifirx_detect_multi.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p), C.c_uint64, C.c_float, C.c_void_p, C.c_void_p,
                                     C.c_void_p]
_lib.wifirx_dev_alloc.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]
_lib.wifirx_dev_free.argtypes = [C.c_void_p, C.c_void_p]
_lib.wifirx_memcpy_h2d.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
_lib.wifirx_memcpy_d2h.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
_lib.wifirx_time_demod.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(Out), C.c_int,
                                   C.POINTER(C.c_float)]


def lib():
    return _lib


def iq_format(fmt) -> int:
    """"fc32" / "sc16" / "sc8" or IQ_FC32 / IQ_SC16 / IQ_SC8 -> the WIFIRX_IQ_* value"""
    if isinstance(fmt, str):
        if fmt not in IQ_FORMATS:
            raise ValueError("sample format must be 'fc32', 'sc16' or 'sc8'")
        return IQ_FORMATS[fmt]
    return int(fmt)


def _fmt_scale(fmt, scale):
    """(the WIFIRX_IQ_* value of fmt, scale as a float: None is the format's conventional widening scale, 1 for "fc32")"""
    fmt = iq_format(fmt)
    return fmt, float(IQ_SCALE.get(fmt, 1.0) if scale is None else scale)


def _np_ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _fe_state_array(state) -> np.ndarray:
    """a writable, contiguous FE_STATE_DTYPE record (a copy); None: a fresh stream"""
    if state is None:
        return np.zeros((), FE_STATE_DTYPE)
    st = np.array(state, dtype=FE_STATE_DTYPE, copy=True)
    if st.shape != ():
        raise ValueError("one wifirx_frontend_state record is required")
    return st


def frontend_estimate(cfg, state):
    """wifirx_frontend_estimate: (dc, w) as complex64 -- what the block of the stream's next sample is corrected with, from
    a host copy of the state (no handle, no device)"""
    st = _fe_state_array(state)
    d, w = (C.c_float * 2)(), (C.c_float * 2)()
    rc = _lib.wifirx_frontend_estimate(C.byref(cfg) if cfg is not None else None, _np_ptr(st), d, w)
    if rc != OK:
        raise WifiRxError(rc, _lib.wifirx_last_error(None).decode())
    return np.complex64(complex(d[0], d[1])), np.complex64(complex(w[0], w[1]))


class DevBuf:
    """A device allocation owned through the C ABI (no torch needed)."""

    def __init__(self, rx: "WifiRx", nbytes: int):
        self.rx, self.nbytes = rx, int(nbytes)
        p = C.c_void_p()
        rx._check(_lib.wifirx_dev_alloc(rx._h, max(self.nbytes, 16), C.byref(p)))
        self.ptr = p.value

    def upload(self, arr: np.ndarray):
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes <= self.nbytes
        self.rx._check(_lib.wifirx_memcpy_h2d(self.rx._h, self.ptr, _np_ptr(arr), arr.nbytes))
        return self

    def download(self, dtype, count) -> np.ndarray:
        out = np.empty(count, dtype=dtype)
        assert out.nbytes <= self.nbytes
        self.rx._check(_lib.wifirx_memcpy_d2h(self.rx._h, _np_ptr(out), self.ptr, out.nbytes))
        return out

    def free(self):
        if self.ptr:
            _lib.wifirx_dev_free(self.rx._h, self.ptr)
            self.ptr = None


class WifiRx:
    """One receive chain = one handle = one HIP stream."""

    def __init__(self, bandwidth=20e6, frequency=5.89e9, sensitivity=0.56, min_plateau=2, chan_est=EQ_LS,
                 max_sym=64, llr_bits=0, want_carrier=False, device=0, max_batch=0, max_slot_len=0, llr_format="f32"):
        """llr_format: "f32" (default) or "bf16" -- the LLR rows of the batch calls (WIFIRX_P_LLR_FORMAT); in bf16 mode the
        LLRs come back as np.uint16 bit patterns (bf16_to_f32 widens them)."""
        if llr_format not in _LLR_FORMATS:
            raise ValueError("llr_format must be 'f32' or 'bf16'")
        self.cfg = Config(ABI_VERSION, device, bandwidth, frequency, sensitivity, min_plateau, chan_est,
                          max_sym, llr_bits, int(bool(want_carrier)), max_batch, max_slot_len)
        h = C.c_void_p()
        rc = _lib.wifirx_create(C.byref(self.cfg), C.byref(h))
        if rc != 0:
            raise WifiRxError(rc, _lib.wifirx_last_error(None).decode())
        self._h = h
        self.llr_format = LLR_F32
        if _LLR_FORMATS[llr_format] != LLR_F32:
            self.set_llr_format(llr_format)

    # -- plumbing --
    def _check(self, rc):
        if rc != 0:
            raise WifiRxError(rc, _lib.wifirx_last_error(self._h).decode())

    def close(self):
        if getattr(self, "_h", None):
            _lib.wifirx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def max_sym(self):
        return self.cfg.max_sym

    @property
    def llr_bits(self):
        return self.cfg.llr_bits

    def set_param(self, pid, value):
        self._check(_lib.wifirx_set_param(self._h, pid, float(value)))
        if pid == P_LLR_FORMAT:
            self.llr_format = int(value)

    def set_llr_format(self, fmt):
        """"f32" / "bf16" (or LLR_F32 / LLR_BF16): the format of the LLR rows of later batch calls"""
        self.set_param(P_LLR_FORMAT, _LLR_FORMATS[fmt] if isinstance(fmt, str) else fmt)

    def _llr_dtype(self):
        return np.uint16 if self.llr_format == LLR_BF16 else np.float32

    def stats(self) -> dict:
        st = Stats()
        self._check(_lib.wifirx_get_stats(self._h, C.byref(st)))
        return {k: getattr(st, k) for k, _ in Stats._fields_}

    def sync(self):
        self._check(_lib.wifirx_sync(self._h))

    def stream_ptr(self):
        return _lib.wifirx_stream(self._h)

    def alloc(self, nbytes) -> DevBuf:
        return DevBuf(self, nbytes)

    # -- batch mode, host buffers (PCIe-bound convenience path) --
    def demod_batch(self, iq: np.ndarray, slot_len: int, decode=False, psdu_stride=2048, want_csi=False,
                    want_stats=False, want_hbits=False, soft=False) -> dict:
        """soft=True (with decode): decode_mac on the LLRs (wifirx_decode_batch_soft; the handle needs llr_bits > 0)."""
        iq = np.ascontiguousarray(iq, dtype=np.complex64).reshape(-1)
        n_slots = iq.size // slot_len
        assert n_slots * slot_len == iq.size
        ms = self.cfg.max_sym
        frames = np.zeros(n_slots, dtype=FRAME_DTYPE)
        idx = np.zeros((n_slots, ms, 48), dtype=np.uint8)
        llr = np.zeros((n_slots, ms * 48 * self.cfg.llr_bits), dtype=self._llr_dtype()) if self.cfg.llr_bits else None
        car = np.zeros((n_slots, ms, 48), dtype=np.complex64) if self.cfg.want_carrier else None
        psdu = np.zeros((n_slots, psdu_stride), dtype=np.uint8) if decode else None
        if not decode:
            csi = np.zeros((n_slots, 52), dtype=np.complex64) if want_csi else None
            stats = np.zeros((n_slots, 4), dtype=np.float32) if want_stats else None
            hbits = np.zeros((n_slots, ms * 12), dtype=np.uint32) if want_hbits else None
            out = Out(_np_ptr(frames), _np_ptr(idx), _np_ptr(llr), _np_ptr(car), None, 0, 0, _np_ptr(csi), _np_ptr(stats),
                      _np_ptr(hbits))
            self._check(_lib.wifirx_demod_batch(self._h, _np_ptr(iq), 0, slot_len, n_slots, C.byref(out)))
            return dict(frames=frames, idx=idx, llr=llr, carrier=car, psdu=None, csi=csi, sym_stats=stats, hbits=hbits)
        # decode needs the decisions on the device: run on device buffers, then download
        d_iq = self.alloc(iq.nbytes).upload(iq)
        # decode_mac reads the decisions as bit planes written by the demod kernel (DECODE_INPUT = "planes"), or -- for
        # callers that only hold `idx` -- packs them itself ("idx")
        dev = self.alloc_out(n_slots, psdu_stride=psdu_stride, want_csi=want_csi, want_stats=want_stats,
                             want_hbits=want_hbits or DECODE_INPUT == "planes")
        try:
            self.demod_batch_dev(d_iq.ptr, slot_len, n_slots, dev)
            if soft:
                self.decode_batch_soft_dev(n_slots, dev)
            else:
                self.decode_batch_dev(n_slots, dev)
            self.sync()
            return self.download_out(dev, n_slots)
        finally:
            d_iq.free()
            self.free_out(dev)

    def demod_batch_var(self, iq: np.ndarray, slot_off) -> dict:
        """batch mode over slots of unequal length: slot k = iq[slot_off[k] : slot_off[k+1]] (host buffers)"""
        iq = np.ascontiguousarray(iq, dtype=np.complex64).reshape(-1)
        off = np.ascontiguousarray(slot_off, dtype=np.uint64)
        n_slots = off.size - 1
        assert n_slots >= 0 and int(off[-1]) <= iq.size
        ms = self.cfg.max_sym
        frames = np.zeros(n_slots, dtype=FRAME_DTYPE)
        idx = np.zeros((n_slots, ms, 48), dtype=np.uint8)
        llr = np.zeros((n_slots, ms * 48 * self.cfg.llr_bits), dtype=self._llr_dtype()) if self.cfg.llr_bits else None
        car = np.zeros((n_slots, ms, 48), dtype=np.complex64) if self.cfg.want_carrier else None
        out = Out(_np_ptr(frames), _np_ptr(idx), _np_ptr(llr), _np_ptr(car), None, 0, 0, None, None)
        self._check(_lib.wifirx_demod_batch_v(self._h, _np_ptr(iq), 0, _np_ptr(off), n_slots, C.byref(out)))
        return dict(frames=frames, idx=idx, llr=llr, carrier=car)

    def demod_batch_var_dev(self, iq_ptr, slot_off, dev):
        """wifirx_demod_batch_v over device samples at iq_ptr: slot k = samples [slot_off[k], slot_off[k+1]) (host offsets,
        [n_slots + 1]), into the device buffers of `dev` (alloc_out)"""
        off = np.ascontiguousarray(slot_off, dtype=np.uint64)
        if off.size < 1:
            raise ValueError("slot_off needs n_slots + 1 entries")
        out = self._out_struct(dev)
        self._slot_off = off        # the library queues the copy of the offsets: they stay alive until the next call
        self._check(_lib.wifirx_demod_batch_v(self._h, iq_ptr, 1, _np_ptr(off), off.size - 1, C.byref(out)))

    # -- batch mode, device buffers (the measured path) --
    def alloc_out(self, n_slots, psdu_stride=0, want_csi=False, want_stats=False, want_hbits=False, want_idx=True) -> dict:
        ms = self.cfg.max_sym
        d = dict(n_slots=n_slots, psdu_stride=psdu_stride)
        d["csi"] = self.alloc(n_slots * 52 * 8) if want_csi else None
        d["sym_stats"] = self.alloc(n_slots * 16) if want_stats else None
        d["frames"] = self.alloc(n_slots * 32)
        d["idx"] = self.alloc(n_slots * ms * 48) if want_idx else None
        d["hbits"] = self.alloc(n_slots * ms * 48) if want_hbits else None
        d["llr"] = self.alloc(n_slots * ms * 48 * self.cfg.llr_bits * np.dtype(self._llr_dtype()).itemsize) if self.cfg.llr_bits else None
        d["carrier"] = self.alloc(n_slots * ms * 48 * 8) if self.cfg.want_carrier else None
        d["psdu"] = self.alloc(n_slots * psdu_stride) if psdu_stride else None
        for k in ("frames", "idx", "llr", "carrier", "psdu", "csi", "sym_stats", "hbits"):      # the kernels only write what a frame fills
            if d[k] is not None and d[k].nbytes:
                d[k].upload(np.zeros(d[k].nbytes, dtype=np.uint8))
        return d

    def free_out(self, dev):
        for k in ("frames", "idx", "llr", "carrier", "psdu", "csi", "sym_stats", "hbits"):
            if dev.get(k) is not None:
                dev[k].free()

    def _out_struct(self, dev) -> Out:
        g = lambda k: dev[k].ptr if dev.get(k) is not None else None
        return Out(g("frames"), g("idx"), g("llr"), g("carrier"), g("psdu"), dev.get("psdu_stride", 0), 1, g("csi"), g("sym_stats"),
                   g("hbits"))

    def demod_batch_dev(self, iq_ptr, slot_len, n_slots, dev):
        out = self._out_struct(dev)
        self._check(_lib.wifirx_demod_batch(self._h, iq_ptr, 1, slot_len, n_slots, C.byref(out)))

    def decode_batch_dev(self, n_slots, dev):
        out = self._out_struct(dev)
        self._check(_lib.wifirx_decode_batch(self._h, n_slots, C.byref(out)))

    def decode_batch_soft_dev(self, n_slots, dev):
        """soft-decision decode_mac over the LLR rows of dev (alloc_out allocates them when the handle has llr_bits > 0)"""
        out = self._out_struct(dev)
        self._check(_lib.wifirx_decode_batch_soft(self._h, n_slots, C.byref(out)))

    def time_demod(self, iq_ptr, slot_len, n_slots, dev, iters=1) -> float:
        out = self._out_struct(dev)
        ms = C.c_float(0)
        self._check(_lib.wifirx_time_demod(self._h, iq_ptr, slot_len, n_slots, C.byref(out), iters, C.byref(ms)))
        return ms.value

    def download_out(self, dev, n_slots) -> dict:
        ms = self.cfg.max_sym
        r = dict(frames=dev["frames"].download(FRAME_DTYPE, n_slots), idx=None,
                 llr=None, carrier=None, psdu=None, csi=None, sym_stats=None, hbits=None)
        if dev.get("idx") is not None:
            r["idx"] = dev["idx"].download(np.uint8, n_slots * ms * 48).reshape(n_slots, ms, 48)
        if dev.get("hbits") is not None:
            r["hbits"] = dev["hbits"].download(np.uint32, n_slots * ms * 12).reshape(n_slots, ms * 12)
        if dev.get("sym_stats") is not None:
            r["sym_stats"] = dev["sym_stats"].download(np.float32, n_slots * 4).reshape(n_slots, 4)
        if dev.get("csi") is not None:
            r["csi"] = dev["csi"].download(np.complex64, n_slots * 52).reshape(n_slots, 52)
        if dev.get("llr") is not None:
            r["llr"] = dev["llr"].download(self._llr_dtype(), n_slots * ms * 48 * self.cfg.llr_bits).reshape(n_slots, -1)
        if dev.get("carrier") is not None:
            r["carrier"] = dev["carrier"].download(np.complex64, n_slots * ms * 48).reshape(n_slots, ms, 48)
        if dev.get("psdu") is not None:
            r["psdu"] = dev["psdu"].download(np.uint8, n_slots * dev["psdu_stride"]).reshape(n_slots, -1)
        return r

    def synth_slots(self, templates: np.ndarray, slots_ptr, slot_len, n_slots, lead, snr_db, cfo_max, seed,
                    cfo_out_ptr=None):
        templates = np.ascontiguousarray(templates, dtype=np.complex64)
        n_t, flen = templates.shape
        self._check(_lib.wifirx_synth_slots(self._h, _np_ptr(templates), 0, n_t, flen, slots_ptr, slot_len,
                                            n_slots, lead, snr_db, cfo_max, seed, cfo_out_ptr))

    def synth_slots_dev(self, templates_ptr, n_templates, frame_len, slots_ptr, slot_len, n_slots, lead, snr_db, cfo_max,
                        seed, cfo_out_ptr=None):
        """synth_slots over templates already on the device (n_templates rows of frame_len samples, e.g. tx_batch_dev's)"""
        self._check(_lib.wifirx_synth_slots(self._h, templates_ptr, 1, n_templates, frame_len, slots_ptr, slot_len,
                                            n_slots, lead, snr_db, cfo_max, seed, cfo_out_ptr))

    # -- transmitter (wifirx_tx_batch) --
    @staticmethod
    def _tx_psdus(psdus, psdu_len=None):
        """list of bytes, or a 2-D uint8 array (+ optional lengths) -> (host array [n, stride] uint8, lengths uint32)"""
        if isinstance(psdus, np.ndarray):
            arr = np.ascontiguousarray(psdus, dtype=np.uint8)
            if arr.ndim != 2:
                raise ValueError("psdus must be a 2-D uint8 array or a list of bytes")
            lens = np.full(arr.shape[0], arr.shape[1], np.uint32) if psdu_len is None else np.asarray(psdu_len, np.uint32)
            return arr, np.ascontiguousarray(lens)
        lens = np.array([len(p) for p in psdus], dtype=np.uint32)
        arr = np.zeros((len(psdus), max(int(lens.max(initial=0)), 1)), dtype=np.uint8)
        for i, p in enumerate(psdus):
            arr[i, :len(p)] = np.frombuffer(bytes(p), dtype=np.uint8)
        return arr, lens

    def tx_batch_dev(self, samples_ptr, samples_cap, psdus, encoding, seeds=None, lead=0, row_len=None, row_off=None,
                     psdu_len=None, psdu_stride=None):
        """wifirx_tx_batch into device memory (samples_cap complex64 samples at samples_ptr).  psdus: host PSDUs (see
        tx_batch), or an int device pointer with psdu_len (host lengths) and psdu_stride.  encoding: an int, or an array-like
        of n_frames values (wifirx_tx_batch_rates: frame i at encoding[i]).  Asynchronous on the handle's stream.  Returns
        the lengths used."""
        if isinstance(psdus, int):
            lens = np.ascontiguousarray(psdu_len, dtype=np.uint32)
            ptr, on_dev, stride, keep = psdus, 1, int(psdu_stride), None
        else:
            keep, lens = self._tx_psdus(psdus, psdu_len)
            ptr, on_dev, stride = _np_ptr(keep), 0, keep.shape[1]
        n = lens.size
        sd = None if seeds is None else np.ascontiguousarray(np.broadcast_to(np.asarray(seeds, np.uint8), (n,)))
        ro = None if row_off is None else np.ascontiguousarray(row_off, dtype=np.uint64)
        if ro is not None and ro.size != n + 1:
            raise ValueError("row_off needs n_frames + 1 entries")
        if np.ndim(encoding) == 0:
            self._check(_lib.wifirx_tx_batch(self._h, int(encoding), ptr, on_dev, stride, _np_ptr(lens), _np_ptr(sd), n,
                                             samples_ptr, int(samples_cap), _np_ptr(ro), int(row_len or 0), int(lead)))
            return lens
        enc = self._tx_encodings(encoding, n)
        self._check(_lib.wifirx_tx_batch_rates(self._h, _np_ptr(enc), ptr, on_dev, stride, _np_ptr(lens), _np_ptr(sd), n,
                                               samples_ptr, int(samples_cap), _np_ptr(ro), int(row_len or 0), int(lead)))
        return lens

    @staticmethod
    def _tx_encodings(encoding, n):
        """array-like of n encodings -> contiguous uint8 (values outside 0..255 become 255, which the library refuses)"""
        e = np.asarray(encoding)
        if e.shape != (n,):
            raise ValueError("encoding needs n_frames entries")
        return np.ascontiguousarray(np.where((e < 0) | (e > 255), 255, e).astype(np.uint8))

    def tx_batch(self, psdus, encoding, seeds=None, lead=0, row_len=None, row_off=None, psdu_len=None):
        """Base-band frames of `psdus` (list of bytes, or a 2-D uint8 array with optional psdu_len) at one encoding (an int) or
        at one encoding per frame (an array-like of n values), built on the device.  Fixed rows (row_len; default lead + the longest frame): returns [n, row_len] complex64, frame i at
        [i, lead:lead + frame].  row_off ([n + 1] sample offsets): returns the packed 1-D stream of samples
        [row_off[0], row_off[n]), frame i `lead` samples into its row."""
        from . import txgen
        arr, lens = self._tx_psdus(psdus, psdu_len)
        n = lens.size
        if row_off is None and row_len is None:
            encs = np.broadcast_to(np.asarray(encoding), (n,))
            row_len = lead + max((txgen.frame_samples(int(l), int(e)) for l, e in zip(lens, encs)), default=0)
        total = int(row_off[-1]) if row_off is not None else n * int(row_len)
        buf = self.alloc(max(total, 1) * 8)
        try:
            self.tx_batch_dev(buf.ptr, total, arr, encoding, seeds, lead, row_len, row_off, psdu_len=lens)
            out = buf.download(np.complex64, total)      # wifirx_memcpy_d2h is ordered behind the kernel on the stream
        finally:
            buf.free()
        if row_off is not None:
            return out[int(row_off[0]):]
        return out.reshape(n, int(row_len))

    # -- channel (wifirx_channel) --
    @staticmethod
    def _channel_taps(taps):
        """1-D set or 2-D [n_tap_sets, L] array -> (complex64 [n_tap_sets, L], n_tap_sets, L)"""
        t = np.asarray(taps, dtype=np.complex64)
        if t.ndim == 1:
            t = t[None]
        if t.ndim != 2:
            raise ValueError("taps must be a 1-D set or a 2-D [n_tap_sets, L] array")
        return np.ascontiguousarray(t), t.shape[0], t.shape[1]

    def channel_dev(self, in_ptr, out_ptr, samples_cap, n_rows, *, row_len=None, row_off=None, taps=(1.0,), cfo=None,
                    phase0=0, gain=1.0, noise_voltage=0.0, seed=0, sample0=0, n_taps=None, n_tap_sets=1, sro=None, drift0=0,
                    doppler=None, k_factor=0.0, fade_seed=0, time0=0):
        """wifirx_channel over device samples: rows of row_len, or row_off ([n_rows + 1] sample offsets).  taps: a 1-D set, a
        2-D [n_tap_sets, L] array, or an int device pointer (then n_taps and n_tap_sets say its shape).  cfo: rad/sample per
        row (scalar or [n_rows]), None = 0.  phase0: uint64 phase in 2^-64 turns.  sro: epsilon - 1 per row (scalar or
        [n_rows]; wifirx_channel_sro, never in place), None = no resampler; drift0: int64 drift of the rows' first output
        sample in 2^-40 samples.  doppler: maximum Doppler shift per row in cycles per sample (scalar or [n_rows], 0 ..
        2^-10; wifirx_channel_fading, NUMERICS.md rule 19: never in place, at most 16 taps), None = static taps; 0 is a
        static random gain per row and tap.  k_factor: Rician K of tap 0 (0 = Rayleigh); fade_seed: key of the fader's draws;
        time0: uint64 stream time of the rows' first output sample.  Asynchronous on the handle's stream."""
        n, u64 = int(n_rows), lambda v: int(v) & 0xFFFFFFFFFFFFFFFF
        # scalar or [n_rows] -> contiguous float32 [n_rows]; None stays None
        per_row = lambda v: None if v is None else np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.float32), (n,)))
        if isinstance(taps, int):
            if n_taps is None:
                raise ValueError("device taps need n_taps")
            t_ptr, t_dev, L, n_sets, keep = taps, 1, int(n_taps), int(n_tap_sets), None
        else:
            keep, n_sets, L = self._channel_taps(taps)
            t_ptr, t_dev = _np_ptr(keep), 0
        c, s, fd = per_row(cfo), per_row(sro), per_row(doppler)
        ro = None if row_off is None else np.ascontiguousarray(row_off, dtype=np.uint64)
        if ro is not None and ro.size != n + 1:
            raise ValueError("row_off needs n_rows + 1 entries")
        head = (self._h, in_ptr, out_ptr, int(samples_cap), _np_ptr(ro), int(row_len or 0), n, t_ptr, t_dev, L, n_sets, _np_ptr(c), u64(phase0))
        noise = (float(gain), float(noise_voltage), u64(seed), u64(sample0))
        if fd is not None:                          # the narrowest entry point that takes the call
            rc = _lib.wifirx_channel_fading(*head, _np_ptr(s), int(drift0), *noise, _np_ptr(fd), float(k_factor), u64(fade_seed), u64(time0))
        elif s is not None:
            rc = _lib.wifirx_channel_sro(*head, _np_ptr(s), int(drift0), *noise)
        else:
            rc = _lib.wifirx_channel(*head, *noise)
        self._check(rc)

    def channel(self, x, *, row_off=None, taps=(1.0,), cfo=None, phase0=0, gain=1.0, noise_voltage=0.0, seed=0,
                sample0=0, sro=None, drift0=0, doppler=None, k_factor=0.0, fade_seed=0, time0=0):
        """channel_dev on host samples: x [n_rows, row_len] (fixed rows; 1-D = one row) or, with row_off, the 1-D buffer the
        offsets index.  Returns the output in x's shape; samples outside the rows are 0."""
        x = np.ascontiguousarray(x, dtype=np.complex64)
        if row_off is not None:
            if x.ndim != 1:
                raise ValueError("with row_off, x is the 1-D sample buffer")
            n_rows, row_len = len(row_off) - 1, None
        else:
            xr = x.reshape(1, -1) if x.ndim == 1 else x
            n_rows, row_len = xr.shape
        n = x.size
        d_in = self.alloc(max(n, 1) * 8)
        d_out = self.alloc(max(n, 1) * 8)
        try:
            d_in.upload(x)
            d_out.upload(np.zeros(n, np.complex64))
            self.channel_dev(d_in.ptr, d_out.ptr, n, n_rows, row_len=row_len, row_off=row_off, taps=taps, cfo=cfo,
                             phase0=phase0, gain=gain, noise_voltage=noise_voltage, seed=seed, sample0=sample0, sro=sro,
                             drift0=drift0, doppler=doppler, k_factor=k_factor, fade_seed=fade_seed, time0=time0)
            y = d_out.download(np.complex64, n)      # ordered behind the kernel on the handle's stream
        finally:
            d_in.free()
            d_out.free()
        return y.reshape(x.shape)

    # -- reflecting surface behind an AP of M antennas (wifirx_irs_taps, wifirx_irs_sweep and their _multi forms; NUMERICS.md
    #    rules 25 to 28).  One implementation serves each pair of wrappers; `multi` says whether the antenna axis is there: with
    #    it the call is the _multi symbol and the taps are [M, n_sets, L], without it M = 1 and they are [n_sets, L] --
    @staticmethod
    def _irs_multi_scene(pdp, los_b2r, los_r2u, los_b2u, multi=True):
        """(pdp [L], A [M, N], B [N], D [M] or None) as contiguous float32 / complex64; a 1-D los_b2r is one antenna.  Without
        `multi` los_b2r is flattened into the one antenna's N coefficients and los_b2u is one value"""
        p = np.ascontiguousarray(np.asarray(pdp, dtype=np.float32).reshape(-1))
        a = np.asarray(los_b2r, dtype=np.complex64)
        a = np.ascontiguousarray(a.reshape(1, -1) if a.ndim == 1 or not multi else a)
        b = np.ascontiguousarray(np.asarray(los_r2u, dtype=np.complex64).reshape(-1))
        if a.ndim != 2 or a.shape[1] != b.size:
            raise ValueError("los_b2r must be [M, N] and los_r2u [N]" if multi else
                             "los_b2r and los_r2u must have one length, the number of elements")
        d = None if los_b2u is None else np.ascontiguousarray(np.asarray(los_b2u, dtype=np.complex64).reshape(-1))
        if d is not None and d.size != a.shape[0]:
            raise ValueError("los_b2u is one complex value per antenna" if multi else "los_b2u is one complex value")
        return p, a, b, d

    @staticmethod
    def _irs_shape(pdp, los_b2r, multi):
        """(L, M, N) of a scene as the host-array wrappers are given it"""
        a = np.asarray(los_b2r)
        return np.asarray(pdp).size, (a.shape[0] if multi and a.ndim > 1 else 1), (a.shape[-1] if multi else a.size)

    def _irs_scatter(self, bufs, kw, scatter, M, N, multi=True):
        """upload a host `scatter` [n_scatter, (M + 1) N + M] into bufs["scatter"] and name it in the keywords of the _dev call"""
        if scatter is None:
            return
        s = np.ascontiguousarray(scatter, dtype=np.complex64)
        if s.ndim != 2 or s.shape[1] != (M + 1) * N + M:
            raise ValueError("scatter must be [n_scatter, (M + 1) N + M]" if multi else "scatter must be [n_scatter, 2 N + 1]")
        bufs["scatter"] = self.alloc(max(s.nbytes, 1)).upload(s)
        kw.update(scatter=bufs["scatter"], n_scatter=s.shape[0])

    def _irs_call(self, fn, multi, taps_ptr, n_sets, scene, gain, k_factor, direct_gain, middle, scatter, n_scatter, seed, outs):
        """one wifirx_irs_taps* / wifirx_irs_sweep* call: `scene` = (p, a, b, d) of _irs_multi_scene, `middle` the three
        arguments between direct_gain and scatter (psi or the codebook), `outs` the two output pointers behind the seed.  The C
        order: h, taps_out, [n_ant,] n_sets, n_taps, pdp, gain, n_elems, los_b2r, los_r2u, los_b2u, k_factor, direct_gain,
        then (psi, psi_on_device, n_psi_sets, align_bits) or (codebook, codebook_on_device, n_codes), then scatter, n_scatter,
        irs_seed, then (elems_out, codes_out) or (best_out, power_out)"""
        ptr = lambda p: p.ptr if isinstance(p, DevBuf) else p
        p, a, b, d = scene
        if scatter is not None and n_scatter is None:
            raise ValueError("device scatter needs n_scatter")
        ant = (a.shape[0],) if multi else ()
        self._check(fn(self._h, ptr(taps_ptr), *ant, int(n_sets), p.size, _np_ptr(p), float(gain), b.size, _np_ptr(a), _np_ptr(b),
                       _np_ptr(d), float(k_factor), float(direct_gain), *middle, ptr(scatter), int(n_scatter or 0),
                       int(seed) & 0xFFFFFFFFFFFFFFFF, *(ptr(o) for o in outs)))

    def _irs_taps_dev(self, multi, taps_ptr, n_sets, pdp, los_b2r, los_r2u, los_b2u, gain, k_factor, direct_gain, psi,
                      n_psi_sets, align_bits, scatter, n_scatter, seed, elems_ptr, codes_ptr):
        scene = self._irs_multi_scene(pdp, los_b2r, los_r2u, los_b2u, multi)
        keep, psi_ptr, psi_dev, n_psi = None, None, 0, 0
        if isinstance(psi, (int, DevBuf)):
            psi_ptr, psi_dev, n_psi = (psi.ptr if isinstance(psi, DevBuf) else psi), 1, int(n_psi_sets or 1)
        elif psi is not None:
            keep = np.asarray(psi, dtype=np.complex64)
            keep = np.ascontiguousarray(keep[None] if keep.ndim == 1 else keep)
            if keep.ndim != 2 or keep.shape[1] != scene[2].size:
                raise ValueError("psi must be [N] or [n_psi_sets, N]")
            psi_ptr, n_psi = _np_ptr(keep), keep.shape[0]
        self._irs_call(_lib.wifirx_irs_taps_multi if multi else _lib.wifirx_irs_taps, multi, taps_ptr, n_sets, scene, gain,
                       k_factor, direct_gain, (psi_ptr, psi_dev, n_psi, int(align_bits)), scatter, n_scatter, seed,
                       (elems_ptr, codes_ptr))

    def _irs_sweep_dev(self, multi, taps_ptr, n_sets, pdp, los_b2r, los_r2u, los_b2u, codebook, n_codes, gain, k_factor,
                       direct_gain, scatter, n_scatter, seed, best_ptr, power_ptr):
        scene = self._irs_multi_scene(pdp, los_b2r, los_r2u, los_b2u, multi)
        if isinstance(codebook, (int, DevBuf)):
            keep, cb_ptr, cb_dev, n_cb = None, (codebook.ptr if isinstance(codebook, DevBuf) else codebook), 1, int(n_codes or 0)
        else:
            keep = np.ascontiguousarray(np.asarray(codebook, dtype=np.complex64))
            if keep.ndim != 2 or keep.shape[1] != scene[2].size:
                raise ValueError("codebook must be [K, N]")
            cb_ptr, cb_dev, n_cb = _np_ptr(keep), 0, keep.shape[0]
        self._irs_call(_lib.wifirx_irs_sweep_multi if multi else _lib.wifirx_irs_sweep, multi, taps_ptr, n_sets, scene, gain,
                       k_factor, direct_gain, (cb_ptr, cb_dev, n_cb), scatter, n_scatter, seed, (best_ptr, power_ptr))

    def _irs_taps(self, multi, n_sets, pdp, los_b2r, los_r2u, los_b2u, scatter, want_elems, want_codes, kw):
        n_sets, (L, M, N) = int(n_sets), self._irs_shape(pdp, los_b2r, multi)
        shapes = {"taps": (np.complex64, (M, n_sets, L) if multi else (n_sets, L))}
        if want_elems:
            shapes["elems"] = (np.complex64, (n_sets, L, M + 1, N))
        if want_codes:
            shapes["codes"] = (np.uint8, (n_sets, N))
        bufs = {}
        try:
            for w, (dt, sh) in shapes.items():
                bufs[w] = self.alloc(max(int(np.prod(sh)), 1) * np.dtype(dt).itemsize)
            self._irs_scatter(bufs, kw, scatter, M, N, multi)
            (self.irs_taps_multi_dev if multi else self.irs_taps_dev)(
                bufs["taps"], n_sets, pdp, los_b2r, los_r2u, los_b2u, elems_ptr=bufs.get("elems"), codes_ptr=bufs.get("codes"), **kw)
            out = {w: bufs[w].download(dt, int(np.prod(sh))).reshape(sh) for w, (dt, sh) in shapes.items()}
        finally:
            for b in bufs.values():
                b.free()
        return out if (want_elems or want_codes) else out["taps"]

    def _irs_sweep(self, multi, n_sets, pdp, los_b2r, los_r2u, los_b2u, codebook, scatter, kw):
        n_sets, (L, M, N) = int(n_sets), self._irs_shape(pdp, los_b2r, multi)
        K = int(kw.get("n_codes") or 0) if isinstance(codebook, (int, DevBuf)) else np.asarray(codebook).shape[0]
        shapes = {"taps": (np.complex64, (M, n_sets, L) if multi else (n_sets, L)), "best": (np.uint16, (n_sets,)),
                  "power": (np.float32, (n_sets, K))}
        bufs = {}
        try:
            for w, (dt, sh) in shapes.items():
                bufs[w] = self.alloc(max(int(np.prod(sh)), 1) * np.dtype(dt).itemsize)
            self._irs_scatter(bufs, kw, scatter, M, N, multi)
            (self.irs_sweep_multi_dev if multi else self.irs_sweep_dev)(
                bufs["taps"], n_sets, pdp, los_b2r, los_r2u, los_b2u, codebook=codebook, best_ptr=bufs["best"],
                power_ptr=bufs["power"], **kw)
            return {w: bufs[w].download(dt, int(np.prod(sh))).reshape(sh) for w, (dt, sh) in shapes.items()}
        finally:
            for b in bufs.values():
                b.free()

    def irs_taps_dev(self, taps_ptr, n_sets, pdp, los_b2r, los_r2u, los_b2u=None, *, gain=1.0, k_factor=0.0, direct_gain=1.0,
                     psi=None, n_psi_sets=None, align_bits=0, scatter=None, n_scatter=None, seed=0, elems_ptr=None,
                     codes_ptr=None):
        """wifirx_irs_taps into device memory: n_sets sets of len(pdp) complex64 taps at taps_ptr (an int device pointer or a
        DevBuf, as every *_ptr here), what channel_dev takes as taps=ptr, n_taps=len(pdp), n_tap_sets=n_sets.  los_b2r, los_r2u:
        the N line-of-sight coefficients of the two legs, los_b2u the direct path's (irs.los gives all three).  psi: a host
        array [N] or [n_psi_sets, N], or a device pointer (then n_psi_sets says its rows); align_bits = 1..3 aligns the phases
        per draw instead and psi is not read.  scatter: None = Philox draws keyed by `seed`, or a device pointer to n_scatter
        rows of 2 N + 1 complex64.  elems_ptr / codes_ptr: optional device outputs [n_sets, L, 2, N] complex64 / [n_sets, N]
        uint8.  Asynchronous on the handle's stream."""
        self._irs_taps_dev(False, taps_ptr, n_sets, pdp, los_b2r, los_r2u, los_b2u, gain, k_factor, direct_gain, psi, n_psi_sets,
                           align_bits, scatter, n_scatter, seed, elems_ptr, codes_ptr)

    def irs_taps(self, n_sets, pdp, los_b2r, los_r2u, los_b2u=None, *, scatter=None, want_elems=False, want_codes=False, **kw):
        """irs_taps_dev with host arrays: returns the taps as complex64 [n_sets, L], or a dict with them under "taps" and the
        elements [n_sets, L, 2, N] under "elems" / the codes [n_sets, N] under "codes" when asked for.  scatter: None or a host
        array [n_scatter, 2 N + 1].  psi and the other keywords as irs_taps_dev."""
        return self._irs_taps(False, n_sets, pdp, los_b2r, los_r2u, los_b2u, scatter, want_elems, want_codes, kw)

    def irs_sweep_dev(self, taps_ptr, n_sets, pdp, los_b2r, los_r2u, los_b2u=None, *, codebook, n_codes=None, gain=1.0,
                      k_factor=0.0, direct_gain=1.0, scatter=None, n_scatter=None, seed=0, best_ptr=None, power_ptr=None):
        """wifirx_irs_sweep into device memory: for each of n_sets tap sets the elements of irs_taps_dev (the same seed gives
        the same elements) run against every entry of `codebook`; the winner's len(pdp) taps go to taps_ptr (what channel_dev
        takes as taps=ptr), the winning entry to best_ptr (uint16 [n_sets]) and every entry's power to power_ptr (float32
        [n_sets, K]).  Each of the three is an int device pointer, a DevBuf or None; one at least is required.  codebook: a host
        array [K, N] complex, or a device pointer (then n_codes says its rows); K <= 1024.  The other arguments as
        irs_taps_dev.  Asynchronous on the handle's stream."""
        self._irs_sweep_dev(False, taps_ptr, n_sets, pdp, los_b2r, los_r2u, los_b2u, codebook, n_codes, gain, k_factor,
                            direct_gain, scatter, n_scatter, seed, best_ptr, power_ptr)

    def irs_sweep(self, n_sets, pdp, los_b2r, los_r2u, los_b2u=None, *, codebook, scatter=None, **kw):
        """irs_sweep_dev with host arrays: returns {"taps": complex64 [n_sets, L], "best": uint16 [n_sets], "power": float32
        [n_sets, K]}.  codebook: a host array [K, N] or a device pointer with n_codes=K; scatter: None or a host array
        [n_scatter, 2 N + 1].  The other keywords as irs_sweep_dev."""
        return self._irs_sweep(False, n_sets, pdp, los_b2r, los_r2u, los_b2u, codebook, scatter, kw)

    def irs_taps_multi_dev(self, taps_ptr, n_sets, pdp, los_b2r, los_r2u, los_b2u=None, *, gain=1.0, k_factor=0.0,
                           direct_gain=1.0, psi=None, n_psi_sets=None, align_bits=0, scatter=None, n_scatter=None, seed=0,
                           elems_ptr=None, codes_ptr=None):
        """wifirx_irs_taps_multi into device memory: M = len(los_b2r) planes of n_sets sets of len(pdp) complex64 taps at
        taps_ptr, antenna-major [M, n_sets, L]; plane m (taps_ptr + m * n_sets * L * 8) is what channel_dev takes as taps=ptr,
        n_taps=L, n_tap_sets=n_sets.  los_b2r [M, N], los_r2u [N], los_b2u [M] (irs.los(antennas=M) gives all three).  The
        antennas share the surface-to-user leg and the phases; align_bits = 1..3 aligns on antenna 0, tap 0.  scatter: None =
        Philox draws keyed by `seed`, or a device pointer to n_scatter rows of (M + 1) N + M complex64.  elems_ptr / codes_ptr:
        optional device outputs [n_sets, L, M + 1, N] complex64 (a_0 .. a_{M-1}, b) / [n_sets, N] uint8.  The other arguments as
        irs_taps_dev.  Asynchronous on the handle's stream."""
        self._irs_taps_dev(True, taps_ptr, n_sets, pdp, los_b2r, los_r2u, los_b2u, gain, k_factor, direct_gain, psi, n_psi_sets,
                           align_bits, scatter, n_scatter, seed, elems_ptr, codes_ptr)

    def irs_taps_multi(self, n_sets, pdp, los_b2r, los_r2u, los_b2u=None, *, scatter=None, want_elems=False, want_codes=False,
                       **kw):
        """irs_taps_multi_dev with host arrays: returns the taps as complex64 [M, n_sets, L], or a dict with them under "taps"
        and the elements [n_sets, L, M + 1, N] under "elems" / the codes [n_sets, N] under "codes" when asked for.  scatter:
        None or a host array [n_scatter, (M + 1) N + M]."""
        return self._irs_taps(True, n_sets, pdp, los_b2r, los_r2u, los_b2u, scatter, want_elems, want_codes, kw)

    def irs_sweep_multi_dev(self, taps_ptr, n_sets, pdp, los_b2r, los_r2u, los_b2u=None, *, codebook, n_codes=None, gain=1.0,
                            k_factor=0.0, direct_gain=1.0, scatter=None, n_scatter=None, seed=0, best_ptr=None, power_ptr=None):
        """wifirx_irs_sweep_multi into device memory: irs_sweep_dev for the M = len(los_b2r) antennas of irs_taps_multi_dev, the
        entries ranked by the sum of the antennas' channel powers (what an MRC receiver collects).  The winner's taps go to
        taps_ptr as [M, n_sets, L], the winning entry to best_ptr (uint16 [n_sets]), every entry's summed power to power_ptr
        (float32 [n_sets, K]); one of the three at least.  The other arguments as irs_sweep_dev and irs_taps_multi_dev.
        Asynchronous on the handle's stream."""
        self._irs_sweep_dev(True, taps_ptr, n_sets, pdp, los_b2r, los_r2u, los_b2u, codebook, n_codes, gain, k_factor,
                            direct_gain, scatter, n_scatter, seed, best_ptr, power_ptr)

    def irs_sweep_multi(self, n_sets, pdp, los_b2r, los_r2u, los_b2u=None, *, codebook, scatter=None, **kw):
        """irs_sweep_multi_dev with host arrays: returns {"taps": complex64 [M, n_sets, L], "best": uint16 [n_sets], "power":
        float32 [n_sets, K]}.  scatter: None or a host array [n_scatter, (M + 1) N + M]."""
        return self._irs_sweep(True, n_sets, pdp, los_b2r, los_r2u, los_b2u, codebook, scatter, kw)

    # -- the surface configured from noisy pilot observations (wifirx_irs_estimate; NUMERICS.md rule 29) --
    def irs_estimate_dev(self, taps_ptr, n_sets, pdp, los_b2r, los_r2u, los_b2u=None, *, pilots, n_pilots=None, n_groups=None,
                         group=None, sigma=0.0, est_scale=None, align_bits=0, gain=1.0, k_factor=0.0, direct_gain=1.0,
                         scatter=None, n_scatter=None, noise=None, n_noise=None, seed=0, est_ptr=None, codes_ptr=None,
                         obs_ptr=None):
        """wifirx_irs_estimate into device memory: the surface of irs_taps_multi_dev (M = len(los_b2r) antennas; a 1-D los_b2r
        is one) stepped through the T pilot configurations `pilots`, observed in noise of standard deviation `sigma`, de-spread
        into an estimate of the direct path and of every group's cascade coefficient, and configured with the B = align_bits
        codes decided from that estimate.  The taps of the true channel under those codes go to taps_ptr as [M, n_sets, L]
        (plane m is what channel_dev takes as taps=ptr), the estimate to est_ptr (complex64 [n_sets, M L, G + 1], column 0 the
        direct path), the codes to codes_ptr (uint8 [n_sets, G]), the observations to obs_ptr (complex64 [n_sets, M L, T]).
        Each is an int device pointer, a DevBuf or None; one at least, and taps / codes need align_bits 1..3.  pilots: a host
        array [T, G] complex (irs.dft_pilots, irs.hadamard_pilots), or a device pointer with n_pilots=T and n_groups=G.
        group: None (G = N) or uint16 [N] (irs.groups).  est_scale: kappa, default irs.est_scale(T) = 1 / T.  noise: None
        (Philox draws keyed by `seed`) or a device pointer to n_noise rows of T complex64.  The other arguments as
        irs_taps_multi_dev.  Asynchronous on the handle's stream."""
        ptr = lambda p: p.ptr if isinstance(p, DevBuf) else p
        p, a, b, d = self._irs_multi_scene(pdp, los_b2r, los_r2u, los_b2u)
        if isinstance(pilots, (int, DevBuf)):
            keep, pl_ptr, pl_dev, T, G = None, ptr(pilots), 1, int(n_pilots or 0), int(n_groups or 0)
        else:
            keep = np.ascontiguousarray(np.asarray(pilots, dtype=np.complex64))
            if keep.ndim != 2:
                raise ValueError("pilots must be [T, G]")
            pl_ptr, pl_dev, (T, G) = _np_ptr(keep), 0, keep.shape
        grp = None
        if group is not None:
            grp = np.ascontiguousarray(np.asarray(group, dtype=np.uint16).reshape(-1))
            if grp.size != b.size:
                raise ValueError("group must hold one value per element")
        if scatter is not None and n_scatter is None:
            raise ValueError("device scatter needs n_scatter")
        if noise is not None and n_noise is None:
            raise ValueError("device noise needs n_noise")
        kappa = 1.0 / max(T, 1) if est_scale is None else float(est_scale)
        self._check(_lib.wifirx_irs_estimate(self._h, ptr(taps_ptr), a.shape[0], int(n_sets), p.size, _np_ptr(p), float(gain),
                                             b.size, _np_ptr(a), _np_ptr(b), _np_ptr(d), float(k_factor), float(direct_gain),
                                             pl_ptr, pl_dev, T, G, _np_ptr(grp), float(sigma), kappa, int(align_bits),
                                             ptr(scatter), int(n_scatter or 0), ptr(noise), int(n_noise or 0),
                                             int(seed) & 0xFFFFFFFFFFFFFFFF, ptr(est_ptr), ptr(codes_ptr), ptr(obs_ptr)))

    def irs_estimate(self, n_sets, pdp, los_b2r, los_r2u, los_b2u=None, *, pilots, scatter=None, noise=None,
                     want=("taps", "est", "codes", "obs"), **kw):
        """irs_estimate_dev with host arrays: returns a dict with the outputs named in `want`: "taps" complex64 [M, n_sets, L],
        "est" complex64 [n_sets, M L, G + 1], "codes" uint8 [n_sets, G], "obs" complex64 [n_sets, M L, T].  With align_bits = 0
        "taps" and "codes" are left out.  pilots: a host array [T, G]; scatter: None or a host array [n_scatter, (M + 1) N + M];
        noise: None or a host array [n_noise, T]."""
        n_sets, (L, M, N) = int(n_sets), self._irs_shape(pdp, los_b2r, True)
        pl = np.asarray(pilots)
        if pl.ndim != 2:
            raise ValueError("pilots must be [T, G]")
        T, G = pl.shape
        R = M * L
        want = [w for w in want if kw.get("align_bits", 0) or w in ("est", "obs")]
        shapes = {"taps": (np.complex64, (M, n_sets, L)), "est": (np.complex64, (n_sets, R, G + 1)),
                  "codes": (np.uint8, (n_sets, G)), "obs": (np.complex64, (n_sets, R, T))}
        if not want or any(w not in shapes for w in want):
            raise ValueError("want names taps, est, codes or obs; taps and codes need align_bits")
        bufs = {}
        try:
            for w in want:
                dt, sh = shapes[w]
                bufs[w] = self.alloc(max(int(np.prod(sh)) * np.dtype(dt).itemsize, 8))
            self._irs_scatter(bufs, kw, scatter, M, N)
            if noise is not None:
                w = np.ascontiguousarray(noise, dtype=np.complex64)
                if w.ndim != 2 or w.shape[1] != T:
                    raise ValueError("noise must be [n_noise, T]")
                bufs["noise"] = self.alloc(max(w.nbytes, 1)).upload(w)
                kw.update(noise=bufs["noise"], n_noise=w.shape[0])
            self.irs_estimate_dev(bufs.get("taps"), n_sets, pdp, los_b2r, los_r2u, los_b2u, pilots=pl, est_ptr=bufs.get("est"),
                                  codes_ptr=bufs.get("codes"), obs_ptr=bufs.get("obs"), **kw)
            return {w: bufs[w].download(shapes[w][0], int(np.prod(shapes[w][1]))).reshape(shapes[w][1]) for w in want}
        finally:
            for b in bufs.values():
                b.free()

    # -- the joint phase decision over antennas and taps (wifirx_irs_optimize; NUMERICS.md rule 30) --
    def irs_optimize_dev(self, coef_ptr, n_sets, n_rows, n_cols, *, bits=2, max_sweeps=4, start="ref", direct_blocked=False,
                         codes_in=None, n_elems=None, group=None, codes_ptr=None, psi_ptr=None, power_ptr=None, sweeps_ptr=None,
                         weights=None, weights_ptr=None, n_weight_sets=1):
        """wifirx_irs_optimize on device memory: cyclic coordinate ascent on the power an MRC receiver collects, over the
        B = bits codes of the G = n_cols - 1 groups, on the coefficient matrix at coef_ptr (complex64 [n_sets, n_rows, n_cols]
        in the layout of irs_estimate_dev's est_ptr: column 0 the direct term, column g + 1 group g).  start: "ref" (the
        decision of irs_estimate_dev, row 0 alone), "given" (codes_in, a device pointer to uint8 [n_sets, G]) or "zero".
        direct_blocked: the direct path is blocked (direct_gain = 0), column 0 is not read.  The final codes go to codes_ptr
        (uint8 [n_sets, G]), their phases to psi_ptr (complex64 [n_sets, N], N = n_elems, through `group`: None = the identity,
        N = G; irs_taps_multi_dev reads them as psi=ptr, n_psi_sets=n_sets), the collected power behind the start and behind
        every sweep to power_ptr (float32 [n_sets, max_sweeps + 1]), the number of sweeps that changed a code to sweeps_ptr
        (uint8 [n_sets]).  Each is an int device pointer, a DevBuf or None; codes_ptr or psi_ptr at least.  Asynchronous on the
        handle's stream.

        With weights the call is wifirx_irs_optimize_weighted (NUMERICS.md rule 31): the ascent is on sum_rho w_rho |s_rho|^2, a
        real weight of either sign on every row, a row of weight 0 absent.  ``weights`` is a host float32 array [n_rows]
        (irs.row_weights); ``weights_ptr`` a device pointer or DevBuf to float32 [n_weight_sets, n_rows], n_weight_sets 1 or
        n_sets (set r reads block r % n_weight_sets).  One of the two at most; with neither the call is wifirx_irs_optimize."""
        ptr = lambda p: p.ptr if isinstance(p, DevBuf) else p
        if start not in IRS_STARTS:
            raise ValueError("start must be ref, given or zero")
        grp = None
        if group is not None:
            grp = np.ascontiguousarray(np.asarray(group, dtype=np.uint16).reshape(-1))
            if n_elems is not None and grp.size != int(n_elems):
                raise ValueError("group must hold one value per element")
        N = int(n_elems) if n_elems is not None else (grp.size if grp is not None else int(n_cols) - 1)
        if weights is not None or weights_ptr is not None:
            if weights is not None and weights_ptr is not None:
                raise ValueError("give weights (host) or weights_ptr (device), not both")
            w = None
            if weights is not None:
                w = np.ascontiguousarray(np.asarray(weights, dtype=np.float32).reshape(-1))
                if w.size != int(n_rows) or int(n_weight_sets) != 1:
                    raise ValueError("host weights hold one value per row; per-set weights go through weights_ptr")
            self._check(_lib.wifirx_irs_optimize_weighted(
                self._h, ptr(coef_ptr), int(n_sets), int(n_rows), int(n_cols), _np_ptr(w) if w is not None else ptr(weights_ptr),
                0 if w is not None else 1, int(n_weight_sets), int(bits), int(max_sweeps), IRS_STARTS[start],
                int(bool(direct_blocked)), ptr(codes_in), N, _np_ptr(grp), ptr(codes_ptr), ptr(psi_ptr), ptr(power_ptr),
                ptr(sweeps_ptr)))
            return
        self._check(_lib.wifirx_irs_optimize(self._h, ptr(coef_ptr), int(n_sets), int(n_rows), int(n_cols), int(bits),
                                             int(max_sweeps), IRS_STARTS[start], int(bool(direct_blocked)), ptr(codes_in), N,
                                             _np_ptr(grp), ptr(codes_ptr), ptr(psi_ptr), ptr(power_ptr), ptr(sweeps_ptr)))

    def irs_optimize(self, coef, *, bits=2, max_sweeps=4, start="ref", direct_blocked=False, codes_in=None, group=None,
                     n_elems=None, want=("codes", "psi", "power", "sweeps"), weights=None):
        """irs_optimize_dev with host arrays: coef complex64 [n_sets, R, J] (or [R, J]: one set), codes_in uint8 [n_sets, G]
        with start="given".  Returns a dict with the outputs named in `want`: "codes" uint8 [n_sets, G], "psi" complex64
        [n_sets, N], "power" float32 [n_sets, max_sweeps + 1], "sweeps" uint8 [n_sets]; codes or psi at least.  weights: None
        (wifirx_irs_optimize), float32 [R] (host weights of wifirx_irs_optimize_weighted) or [n_sets, R] (uploaded for the call
        and read as device weights, one row block per set)."""
        q = np.asarray(coef, dtype=np.complex64)
        q = np.ascontiguousarray(q[None] if q.ndim == 2 else q)
        if q.ndim != 3:
            raise ValueError("coef must be [n_sets, R, J]")
        n_sets, R, J = q.shape
        G = J - 1
        N = int(n_elems) if n_elems is not None else (np.asarray(group).size if group is not None else G)
        shapes = {"codes": (np.uint8, (n_sets, G)), "psi": (np.complex64, (n_sets, N)),
                  "power": (np.float32, (n_sets, int(max_sweeps) + 1)), "sweeps": (np.uint8, (n_sets,))}
        want = list(want)
        if any(w not in shapes for w in want) or not ("codes" in want or "psi" in want):
            raise ValueError("want names codes, psi, power or sweeps; codes or psi at least")
        bufs = {}
        try:
            bufs["coef"] = self.alloc(max(q.nbytes, 8)).upload(q)
            for w in want:
                dt, sh = shapes[w]
                bufs[w] = self.alloc(max(int(np.prod(sh)) * np.dtype(dt).itemsize, 8))
            if codes_in is not None:
                ci = np.ascontiguousarray(np.asarray(codes_in, dtype=np.uint8))
                if ci.shape != (n_sets, G):
                    raise ValueError("codes_in must be [n_sets, G]")
                bufs["codes_in"] = self.alloc(max(ci.nbytes, 8)).upload(ci)
            wkw = {}
            if weights is not None:
                w = np.ascontiguousarray(np.asarray(weights, dtype=np.float32))
                if w.shape == (R,):
                    wkw = dict(weights=w)
                elif w.shape == (n_sets, R):
                    bufs["weights"] = self.alloc(max(w.nbytes, 8)).upload(w)
                    wkw = dict(weights_ptr=bufs["weights"], n_weight_sets=n_sets)
                else:
                    raise ValueError("weights must be [R] or [n_sets, R]")
            self.irs_optimize_dev(bufs["coef"], n_sets, R, J, bits=bits, max_sweeps=max_sweeps, start=start,
                                  direct_blocked=direct_blocked, codes_in=bufs.get("codes_in"), n_elems=N, group=group,
                                  codes_ptr=bufs.get("codes"), psi_ptr=bufs.get("psi"), power_ptr=bufs.get("power"),
                                  sweeps_ptr=bufs.get("sweeps"), **wkw)
            return {w: bufs[w].download(shapes[w][0], int(np.prod(shapes[w][1]))).reshape(shapes[w][1]) for w in want}
        finally:
            for b in bufs.values():
                b.free()

    # -- the ends of the loop-back (wifirx_mac_batch, wifirx_link_stats) --
    def mac_batch_dev(self, psdu_ptr, psdu_stride, n_frames, payload=None, payload_len=None, seq0=0, addr=None,
                      payload_seed=0, payload_stride=None):
        """wifirx_mac_batch into device memory (n_frames rows of psdu_stride bytes at psdu_ptr): ieee802_11.mac's PSDUs.
        payload: None (Philox bytes keyed by payload_seed, made on the device), a 2-D uint8 array [n_frames, stride] or a list of
        bytes (host payloads), or an int device pointer (with payload_stride).  payload_len: one length for all, or
        [n_frames]; default the row width of `payload` (required for Philox payloads).  addr: (dst, src, bss), 6 bytes each.
        Asynchronous on the handle's stream.  Returns the payload lengths used (uint32 [n_frames])."""
        n = int(n_frames)
        keep, ptr, on_dev = None, None, 0
        if isinstance(payload, int):
            if payload_stride is None:
                raise ValueError("a device payload needs payload_stride")
            ptr, on_dev, stride = payload, 1, int(payload_stride)
        elif payload is not None:
            if isinstance(payload, np.ndarray):
                keep = np.ascontiguousarray(payload, dtype=np.uint8)
                if keep.ndim != 2:
                    raise ValueError("payload must be a 2-D uint8 array, a list of bytes, a device pointer or None")
            else:
                keep, lens = self._tx_psdus(payload)
                if payload_len is None:
                    payload_len = lens
            if keep.shape[0] != n:
                raise ValueError("payload needs n_frames rows")
            ptr, stride = _np_ptr(keep), keep.shape[1]
        else:
            if payload_len is None:
                raise ValueError("Philox payloads need payload_len")
            stride = int(np.max(payload_len, initial=0)) if np.ndim(payload_len) else int(payload_len)
        if payload_len is None:
            lens = np.full(n, stride, np.uint32)
        else:
            lens = np.ascontiguousarray(np.broadcast_to(np.asarray(payload_len, np.uint32), (n,)))
        # one length for all that is also the stride: no array to upload (payload_len = NULL)
        uniform = payload_len is None or (np.ndim(payload_len) == 0 and int(payload_len) == stride)
        a = None
        if addr is not None:
            a = np.ascontiguousarray(np.concatenate([np.frombuffer(bytes(x), np.uint8) for x in addr]))
            if a.size != 18:
                raise ValueError("addr = (dst, src, bss), 6 bytes each")
        self._check(_lib.wifirx_mac_batch(self._h, ptr, on_dev, stride, None if uniform else _np_ptr(lens), n, _np_ptr(a), int(seq0) & 0xFFFFFFFF,
                                          int(payload_seed) & 0xFFFFFFFFFFFFFFFF, psdu_ptr, int(psdu_stride)))
        return lens

    def mac_batch(self, n_frames, payload=None, payload_len=None, seq0=0, addr=None, payload_seed=0):
        """Host convenience of mac_batch_dev: returns [n_frames, 28 + longest payload] uint8, PSDU i in row i (zeros behind
        a shorter one)."""
        n = int(n_frames)
        if payload is None and payload_len is None:
            raise ValueError("Philox payloads need payload_len")
        if payload_len is not None:
            width = int(np.max(payload_len, initial=0))
        elif isinstance(payload, np.ndarray):
            width = payload.shape[1]
        else:
            width = max((len(p) for p in payload), default=0)
        stride = width + 28
        buf = self.alloc(max(n, 1) * stride).upload(np.zeros(max(n, 1) * stride, np.uint8))
        try:
            self.mac_batch_dev(buf.ptr, stride, n, payload, payload_len, seq0, addr, payload_seed)
            return buf.download(np.uint8, n * stride).reshape(n, stride)
        finally:
            buf.free()

    def link_stats(self, n_slots, dev, ref, per_frame=False, by_rate=False) -> dict:
        """wifirx_link_stats: scores the decoded batch `dev` (an alloc_out dict after demod + decode) against `ref`, a dict with
        the DevBufs of what was sent: "frames" (required), "psdu" + "psdu_stride", "hbits" / "idx".  Returns the counters of
        wifirx_link_counts and, derived from them in float64, fer, coded_ber and coded_ber_se (the standard error of the mean
        of the per-frame BER, for frames of one length); per_frame=True adds "frame_err" (uint32) and "frame_class" (uint8)
        as DevBufs the caller frees.  by_rate=True (wifirx_link_stats_by_rate) adds "by_rate": a list of eight dicts, the same
        counters and derived values over the slots whose reference record has encoding e.  Waits for the result."""
        n = int(n_slots)
        o_rx, o_ref = self._out_struct(dev), self._out_struct(ref)
        d_err = self.alloc(4 * max(n, 1)) if per_frame else None
        d_cls = self.alloc(max(n, 1)) if per_frame else None
        cnt = LinkCounts()
        rates = (LinkCounts * 8)()
        try:
            if by_rate:
                self._check(_lib.wifirx_link_stats_by_rate(self._h, n, C.byref(o_rx), C.byref(o_ref),
                                                           d_err.ptr if per_frame else None, d_cls.ptr if per_frame else None,
                                                           C.byref(cnt), rates))
            else:
                self._check(_lib.wifirx_link_stats(self._h, n, C.byref(o_rx), C.byref(o_ref), d_err.ptr if per_frame else None,
                                                   d_cls.ptr if per_frame else None, C.byref(cnt)))
        except Exception:
            if per_frame:
                d_err.free()
                d_cls.free()
            raise
        r = {k: int(getattr(cnt, k)) for k, _ in LinkCounts._fields_}
        r.update(link_rates(r))
        if by_rate:
            r["by_rate"] = []
            for e in range(8):
                d = {k: int(getattr(rates[e], k)) for k, _ in LinkCounts._fields_}
                d.update(link_rates(d))
                r["by_rate"].append(d)
        if per_frame:
            r["frame_err"], r["frame_class"] = d_err, d_cls
        return r

    # -- sample formats (wifirx_iq_to_f32, wifirx_iq_from_f32; NUMERICS.md rule 20) --
    def iq_to_f32_dev(self, src_ptr, fmt, n, dst_ptr, scale=None):
        """wifirx_iq_to_f32 on device pointers: n samples of `fmt` at src_ptr -> complex64 at dst_ptr.  Asynchronous on the
        handle's stream."""
        fmt, scale = _fmt_scale(fmt, scale)
        self._check(_lib.wifirx_iq_to_f32(self._h, src_ptr, fmt, int(n), scale, dst_ptr))

    def iq_from_f32_dev(self, src_ptr, n, fmt, dst_ptr, scale=None, bits=None, count=False):
        """wifirx_iq_from_f32 on device pointers: n complex64 samples at src_ptr -> samples of `fmt` at dst_ptr, quantised to
        `bits` bits (default: the container's).  scale defaults to the inverse of the conventional widening scale.
        count=True waits and returns the number of clipped components; otherwise asynchronous, returns None."""
        fmt = iq_format(fmt)
        scale = 1.0 / IQ_SCALE.get(fmt, 1.0) if scale is None else scale
        bits = IQ_MAX_BITS.get(fmt, 0) if bits is None else bits
        c = C.c_uint64(0)
        self._check(_lib.wifirx_iq_from_f32(self._h, src_ptr, int(n), float(scale), fmt, int(bits), dst_ptr,
                                            C.byref(c) if count else None))
        return int(c.value) if count else None

    @staticmethod
    def _iq_array(x, fmt=None):
        """int16 / int8 samples as [n, 2] or flat [2 n] -> (contiguous flat array, format, n)"""
        x = np.asarray(x)
        if fmt is None:
            fmt = {np.dtype(np.int16): IQ_SC16, np.dtype(np.int8): IQ_SC8}.get(x.dtype)
            if fmt is None:
                raise ValueError("the sample format is taken from int16 or int8 arrays only")
        fmt = iq_format(fmt)
        if fmt in IQ_MAX_BITS:
            if x.dtype != IQ_DTYPE[fmt]:
                raise ValueError("%s samples must be %s" % ({IQ_SC16: "sc16", IQ_SC8: "sc8"}[fmt], IQ_DTYPE[fmt]))
            if not (x.ndim == 1 or (x.ndim == 2 and x.shape[1] == 2)) or x.size % 2:
                raise ValueError("integer samples come as [n, 2] or flat [2 n]")
        x = np.ascontiguousarray(x).reshape(-1)
        return x, fmt, x.size // 2 if fmt in IQ_MAX_BITS else x.size

    @classmethod
    def _host_samples(cls, x, fmt=None):
        """complex samples (fmt None or "fc32") or int16 / int8 samples (_iq_array) -> (contiguous flat array, format, n)"""
        x = np.asarray(x)
        if fmt is None and x.dtype not in (np.dtype(np.int16), np.dtype(np.int8)):
            fmt = IQ_FC32
        if fmt is not None and iq_format(fmt) == IQ_FC32:
            x = np.ascontiguousarray(x, dtype=np.complex64).reshape(-1)
            return x, IQ_FC32, x.size
        return cls._iq_array(x, fmt)

    def iq_to_f32(self, q, fmt=None, scale=None) -> np.ndarray:
        """iq_to_f32_dev on a NumPy array of int16 / int8 samples ([n, 2] or flat [2 n]): returns complex64 [n]"""
        q, fmt, n = self._iq_array(q, fmt)
        d_in, d_out = self.alloc(max(q.nbytes, 1)), self.alloc(max(n, 1) * 8)
        try:
            d_in.upload(q)
            self.iq_to_f32_dev(d_in.ptr, fmt, n, d_out.ptr, scale)
            return d_out.download(np.complex64, n)       # ordered behind the kernel on the handle's stream
        finally:
            d_in.free()
            d_out.free()

    def iq_from_f32(self, x, fmt, scale=None, bits=None):
        """iq_from_f32_dev on complex64 samples: returns (int16 / int8 array [n, 2], clipped components)"""
        x = np.ascontiguousarray(x, dtype=np.complex64).reshape(-1)
        fmt = iq_format(fmt)
        dt = IQ_DTYPE[fmt]
        d_in, d_out = self.alloc(max(x.nbytes, 1)), self.alloc(max(x.size, 1) * 2 * dt.itemsize)
        try:
            d_in.upload(x)
            clipped = self.iq_from_f32_dev(d_in.ptr, x.size, fmt, d_out.ptr, scale, bits, count=True)
            return d_out.download(dt, 2 * x.size).reshape(-1, 2), clipped
        finally:
            d_in.free()
            d_out.free()

    # -- receive front end (wifirx_frontend, wifirx_rx_impair; NUMERICS.md rule 32) --
    def frontend_dev(self, cfg, state_ptr, in_ptr, fmt, n, out_ptr, scale=None):
        """wifirx_frontend on device pointers: n samples of `fmt` at in_ptr -> corrected complex64 at out_ptr, the
        wifirx_frontend_state at state_ptr advanced.  in_ptr == out_ptr is allowed for "fc32".  Asynchronous on the handle's
        stream."""
        fmt, scale = _fmt_scale(fmt, scale)
        self._check(_lib.wifirx_frontend(self._h, C.byref(cfg), state_ptr, in_ptr, fmt, scale, int(n), out_ptr))

    def frontend(self, x, cfg=None, state=None, fmt=None, scale=None):
        """frontend_dev on host arrays: complex64 samples (fmt None or "fc32") or int16 / int8 samples ([n, 2] or flat [2 n]);
        cfg None: frontend_cfg(); state None: a fresh stream.  Returns (complex64 [n], the state behind the call as a
        FE_STATE_DTYPE record), which continues the stream when it is handed in again."""
        cfg = frontend_cfg() if cfg is None else cfg
        x, fmt, n = self._host_samples(x, fmt)
        st = _fe_state_array(state)
        d_in, d_out, d_st = self.alloc(max(x.nbytes, 1)), self.alloc(max(n, 1) * 8), self.alloc(FE_STATE_DTYPE.itemsize)
        try:
            d_in.upload(x)
            d_st.upload(st.reshape(1))
            self.frontend_dev(cfg, d_st.ptr, d_in.ptr, fmt, n, d_out.ptr, scale)
            return d_out.download(np.complex64, n), d_st.download(FE_STATE_DTYPE, 1)[0]
        finally:
            d_in.free()
            d_out.free()
            d_st.free()

    def rx_impair_dev(self, in_ptr, out_ptr, n, mu=1.0, nu=0.0, dc=0.0):
        """wifirx_rx_impair on device pointers: out = mu x + nu conj(x) + dc over n complex64 samples (mu, nu, dc complex;
        in_ptr == out_ptr is allowed).  Asynchronous on the handle's stream."""
        v = [(C.c_float * 2)(np.float32(np.real(c)), np.float32(np.imag(c))) for c in (mu, nu, dc)]
        self._check(_lib.wifirx_rx_impair(self._h, in_ptr, out_ptr, int(n), v[0], v[1], v[2]))

    def rx_impair(self, x, mu=1.0, nu=0.0, dc=0.0) -> np.ndarray:
        """rx_impair_dev on complex64 host samples (iq_imbalance() gives mu and nu of a gain / phase imbalance)"""
        x = np.ascontiguousarray(x, dtype=np.complex64).reshape(-1)
        d = self.alloc(max(x.nbytes, 1))
        try:
            d.upload(x)
            self.rx_impair_dev(d.ptr, d.ptr, x.size, mu, nu, dc)
            return d.download(np.complex64, x.size)
        finally:
            d.free()

    def stream_frontend(self, cfg=None, init=None, **kw):
        """wifirx_stream_frontend: the front end on every later push / push_iq.  cfg: a FrontendCfg, True (the keywords of
        frontend_cfg() in kw) or None / False (off).  init: a FE_STATE_DTYPE record to start from (None: fresh)."""
        if cfg is None or cfg is False:
            self._check(_lib.wifirx_stream_frontend(self._h, None, None))
            return
        cfg = frontend_cfg(**kw) if cfg is True else cfg
        st = None if init is None else _fe_state_array(init)
        self._check(_lib.wifirx_stream_frontend(self._h, C.byref(cfg), _np_ptr(st)))

    def stream_frontend_state(self) -> np.ndarray:
        """wifirx_stream_frontend_state: the stream's front-end state as a FE_STATE_DTYPE record (waits for the stream)"""
        st = np.zeros((), FE_STATE_DTYPE)
        self._check(_lib.wifirx_stream_frontend_state(self._h, _np_ptr(st)))
        return st

    # -- wideband ingest (wifirx_channelize; NUMERICS.md rule 21) --
    def channelize_dev(self, in_ptr, fmt, n_out, n_channels, stacking, out_ptr, out_stride=None, hist_ptr=None,
                       hist_out_ptr=None, m0=0, scale=None):
        """wifirx_channelize on device pointers: n_out * n_channels samples of `fmt` at in_ptr -> n_channels rows of n_out
        complex64 at out_ptr, row k at out_ptr + 8 * k * out_stride bytes (out_stride None: n_out).  hist_ptr: the
        23 * n_channels samples in front (None: zeros); hist_out_ptr: where the next call's hist goes (None: nowhere).
        Asynchronous on the handle's stream: sync() before another handle reads the rows."""
        fmt, scale = _fmt_scale(fmt, scale)
        self._check(_lib.wifirx_channelize(self._h, in_ptr, fmt, scale, hist_ptr, hist_out_ptr, int(n_channels),
                                           int(stacking), int(n_out), int(m0) & 0xFFFFFFFFFFFFFFFF, out_ptr,
                                           int(n_out if out_stride is None else out_stride)))

    # -- wideband transmit (wifirx_combine; NUMERICS.md rule 22) --
    def combine_dev(self, in_ptr, in_stride, n_in, n_channels, stacking, out_ptr, gains=None, hist_ptr=None, hist_out_ptr=None,
                    m0=0):
        """wifirx_combine on device pointers: n_channels rows of n_in complex64 at in_ptr, row k at in_ptr + 8 * k * in_stride
        bytes -> n_in * n_channels complex64 at out_ptr.  gains: n_channels finite floats (host; None: no multiply).
        hist_ptr: n_channels rows of 23 samples in front (None: zeros); hist_out_ptr: where the next call's hist goes
        (None: nowhere).  Asynchronous on the handle's stream: sync() before another handle reads the output."""
        g = None
        if gains is not None:
            g = np.ascontiguousarray(gains, dtype=np.float32).reshape(-1)
            if g.size != int(n_channels):
                raise ValueError("one gain per channel is required")
            g = g.ctypes.data_as(C.POINTER(C.c_float))
        self._check(_lib.wifirx_combine(self._h, in_ptr, int(in_stride), g, hist_ptr, hist_out_ptr, int(n_channels),
                                        int(stacking), int(n_in), int(m0) & 0xFFFFFFFFFFFFFFFF, out_ptr))

    def combine(self, streams, stacking, gains=None) -> np.ndarray:
        """combine_dev on host arrays: n_channels complex streams of one length n from the start of a stream -> complex64
        [n * n_channels] (PCIe-bound convenience)"""
        u = np.ascontiguousarray(np.asarray(streams, dtype=np.complex64))
        if u.ndim != 2:
            raise ValueError("streams of one length are required")
        M, n = u.shape
        d_in, d_out = self.alloc(max(u.nbytes, 1)), self.alloc(max(n * M, 1) * 8)
        try:
            d_in.upload(u)
            self.combine_dev(d_in.ptr, n, n, M, stacking, d_out.ptr, gains)
            return d_out.download(np.complex64, n * M)       # ordered behind the kernel on the handle's stream
        finally:
            d_in.free()
            d_out.free()

    # -- receive resampler (wifirx_arb_resample; NUMERICS.md rule 34) --
    def arb_resample_dev(self, in_ptr, fmt, n_in, num, den, out_ptr, out_cap, hist_ptr=None, hist_out_ptr=None, j0=0, m0=0,
                         scale=None) -> int:
        """wifirx_arb_resample on device pointers: n_in samples of `fmt` at in_ptr, in[0] being stream sample j0 -> the
        outputs m0 .. as complex64 at out_ptr (room for out_cap).  hist_ptr: the arb_hist(num, den) samples in front (None:
        zeros); hist_out_ptr: where the next call's hist goes (None: nowhere).  Returns n_out.  Asynchronous on the handle's
        stream: sync() before another handle reads the output."""
        fmt, scale = _fmt_scale(fmt, scale)
        n = C.c_uint64(0)
        self._check(_lib.wifirx_arb_resample(self._h, in_ptr, fmt, scale, int(n_in), hist_ptr, hist_out_ptr, int(num),
                                             int(den), int(j0), int(m0), out_ptr, int(out_cap), C.byref(n)))
        return int(n.value)

    def arb_resample(self, x, num, den, fmt=None, scale=None, n_out=None) -> np.ndarray:
        """arb_resample_dev on host arrays, a whole stream from j0 = m0 = 0: complex64 samples (fmt None or "fc32") or int16 /
        int8 samples ([n, 2] or flat [2 n]) -> complex64.  n_out: append the zeros of the end-of-stream flush and return
        exactly that many outputs (None: what the samples alone give)."""
        return self._arb_host(x, num, den, fmt, n_out, 1, lambda src, fmt, n, dst, made: self.arb_resample_dev(
            src, fmt, n, num, den, dst, made, scale=scale))[0]

    def _arb_host(self, x, num, den, fmt, n_out, K, call_dev) -> np.ndarray:
        """what arb_resample and tune do around their call: the samples (_host_samples) and the zeros of the flush up,
        call_dev(in_ptr, fmt, n_in, out_ptr, row length) -> n_out per row, the K rows down, cut to n_out"""
        x, fmt, n = self._host_samples(x, fmt)
        if n_out is not None:
            pad = arb_flush_inputs(num, den, n, n_out)
            x = np.concatenate([x, np.zeros(pad * (1 if fmt == IQ_FC32 else 2), x.dtype)])
            n += pad
        made = arb_count(num, den, 0, n, 0)
        d_in, d_out = self.alloc(max(x.nbytes, 1)), self.alloc(max(made * K, 1) * 8)
        try:
            d_in.upload(x)
            got = call_dev(d_in.ptr, fmt, n, d_out.ptr, made)
            y = d_out.download(np.complex64, got * K).reshape(K, got)       # ordered behind the kernel on the handle's stream
            return y if n_out is None else y[:, :n_out]
        finally:
            d_in.free()
            d_out.free()

    # -- tuner (wifirx_tune; NUMERICS.md rule 35) --
    def tune_dev(self, in_ptr, fmt, n_in, num, den, incs, out_ptr, out_stride, phase0s=None, hist_ptr=None, hist_out_ptr=None,
                 j0=0, m0=0, scale=None) -> int:
        """wifirx_tune on device pointers: n_in samples of `fmt` at in_ptr, in[0] being stream sample j0 -> per channel k the
        outputs m0 .. as complex64 at out_ptr + 8 * k * out_stride.  incs: one uint64 increment per channel (tune_inc);
        phase0s: the phases of stream sample 0 (None: zeros).  hist_ptr / hist_out_ptr as arb_resample_dev: raw input
        samples.  Returns n_out per channel.  Asynchronous on the handle's stream: sync() before another handle reads a row."""
        fmt, scale = _fmt_scale(fmt, scale)
        K = len(incs)
        inc = (C.c_uint64 * max(K, 1))(*[int(v) & 0xFFFFFFFFFFFFFFFF for v in incs])
        ph = None
        if phase0s is not None:
            if len(phase0s) != K:
                raise ValueError("one phase0 per channel is required")
            ph = (C.c_uint64 * max(K, 1))(*[int(v) & 0xFFFFFFFFFFFFFFFF for v in phase0s])
        n = C.c_uint64(0)
        self._check(_lib.wifirx_tune(self._h, in_ptr, fmt, scale, int(n_in), hist_ptr, hist_out_ptr, int(num), int(den), K,
                                     inc, ph, int(j0), int(m0), out_ptr, int(out_stride), C.byref(n)))
        return int(n.value)

    def tune(self, x, num, den, incs, phase0s=None, fmt=None, scale=None, n_out=None) -> np.ndarray:
        """tune_dev on host arrays, a whole stream from j0 = m0 = 0: complex64 samples (fmt None or "fc32") or int16 / int8
        samples ([n, 2] or flat [2 n]) -> complex64 [K, n_out].  n_out: append the zeros of the end-of-stream flush and return
        exactly that many outputs per channel (None: what the samples alone give)."""
        return self._arb_host(x, num, den, fmt, n_out, len(incs), lambda src, fmt, n, dst, made: self.tune_dev(
            src, fmt, n, num, den, incs, dst, made, phase0s=phase0s, scale=scale))

    # -- band survey (wifirx_spectrum, _fold, _bands; NUMERICS.md rule 36) --
    def spectrum_dev(self, in_ptr, fmt, n_in, n_fft, hop, avg, rows_ptr, rows_cap, window="blackman_harris", mode="sum", norm=1.0,
                     scale=None) -> int:
        """wifirx_spectrum on device pointers: n_in samples of `fmt` at in_ptr -> power rows of n_fft float32 at rows_ptr (room
        for rows_cap rows).  window: "rect" / "hann" / "blackman_harris" or SPEC_*; mode: "sum" / "max" or SPEC_*.  Returns
        n_rows.  Asynchronous on the handle's stream: sync() before another handle reads the rows."""
        fmt, scale = _fmt_scale(fmt, scale)
        window = SPEC_WINDOWS[window] if isinstance(window, str) else int(window)
        mode = SPEC_MODES[mode] if isinstance(mode, str) else int(mode)
        n = C.c_uint64(0)
        self._check(_lib.wifirx_spectrum(self._h, in_ptr, fmt, scale, int(n_in), int(n_fft), int(hop), int(avg), window, mode,
                                         float(norm), rows_ptr, int(rows_cap), C.byref(n)))
        return int(n.value)

    def spectrum(self, x, n_fft=1024, hop=None, avg=1, window="blackman_harris", mode="sum", norm=1.0, fmt=None, scale=None) -> np.ndarray:
        """spectrum_dev on a host array: complex64 samples (fmt None or "fc32") or int16 / int8 samples ([n, 2] or flat [2 n])
        -> float32 [n_rows, n_fft].  hop None: n_fft."""
        x, fmt, n = self._host_samples(x, fmt)
        hop = int(n_fft) if hop is None else int(hop)
        rows, _ = spectrum_count(n_fft, hop, avg, n)
        d_in, d_out = self.alloc(max(x.nbytes, 1)), self.alloc(max(rows * int(n_fft), 1) * 4)
        try:
            d_in.upload(x)
            got = self.spectrum_dev(d_in.ptr, fmt, n, n_fft, hop, avg, d_out.ptr, rows, window, mode, norm, scale)
            return d_out.download(np.float32, got * int(n_fft)).reshape(got, int(n_fft))
        finally:
            d_in.free()
            d_out.free()

    def spectrum_fold_dev(self, rows_ptr, n_rows, n_fft, group, out_ptr, out_cap, mode="sum") -> int:
        """wifirx_spectrum_fold on device pointers: out row q = the fold of rows q * group .. q * group + group - 1.  Returns
        n_out = n_rows // group."""
        mode = SPEC_MODES[mode] if isinstance(mode, str) else int(mode)
        n = C.c_uint64(0)
        self._check(_lib.wifirx_spectrum_fold(self._h, rows_ptr, int(n_rows), int(n_fft), int(group), mode, out_ptr, int(out_cap),
                                              C.byref(n)))
        return int(n.value)

    def spectrum_fold(self, rows, group=None, mode="sum") -> np.ndarray:
        """spectrum_fold_dev on a host array float32 [n_rows, n_fft] -> [n_rows // group, n_fft].  group None: all rows"""
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        n_rows, n_fft = rows.shape
        group = max(n_rows, 1) if group is None else int(group)
        made = n_rows // group if group else 0
        d_in, d_out = self.alloc(max(rows.nbytes, 4)), self.alloc(max(made * n_fft, 1) * 4)
        try:
            d_in.upload(rows)
            got = self.spectrum_fold_dev(d_in.ptr, n_rows, n_fft, group, d_out.ptr, made, mode)
            return d_out.download(np.float32, got * n_fft).reshape(got, n_fft)
        finally:
            d_in.free()
            d_out.free()

    def spectrum_bands_dev(self, rows_ptr, n_rows, n_fft, bands, out_ptr):
        """wifirx_spectrum_bands on device pointers: bands = [(lo, hi), ..] bins; out [n_rows, len(bands)] float32 at out_ptr"""
        K = len(bands)
        lo = (C.c_uint32 * max(K, 1))(*[int(b[0]) for b in bands])
        hi = (C.c_uint32 * max(K, 1))(*[int(b[1]) for b in bands])
        self._check(_lib.wifirx_spectrum_bands(self._h, rows_ptr, int(n_rows), int(n_fft), K, lo, hi, out_ptr))

    def spectrum_bands(self, rows, bands) -> np.ndarray:
        """spectrum_bands_dev on a host array float32 [n_rows, n_fft] -> float32 [n_rows, len(bands)]"""
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        n_rows, n_fft = rows.shape
        d_in, d_out = self.alloc(max(rows.nbytes, 4)), self.alloc(max(n_rows * len(bands), 1) * 4)
        try:
            d_in.upload(rows)
            self.spectrum_bands_dev(d_in.ptr, n_rows, n_fft, bands, d_out.ptr)
            return d_out.download(np.float32, n_rows * len(bands)).reshape(n_rows, len(bands))
        finally:
            d_in.free()
            d_out.free()

    # -- receive diversity (wifirx_diversity_combine; NUMERICS.md rule 23) --
    def diversity_combine_dev(self, ins, n_slots, out, mode=DIV_MRC, ant_gain=None, used_mask_ptr=None):
        """wifirx_diversity_combine on device buffers: ins = one alloc_out dict per antenna after its demod (frames, carrier and
        csi are read; they may belong to other handles with the same max_sym, synchronised first), out = an alloc_out dict
        without hbits that receives frames and, where allocated, idx, llr and carrier.  mode: DIV_MRC / DIV_SELECT (or "mrc" /
        "select").  ant_gain: one finite float >= 0 per antenna, the inverse noise power (None: equal noise).  used_mask_ptr:
        n_slots device bytes (None: not wanted).  Asynchronous on the handle's stream, behind its earlier calls."""
        mode = DIV_MODES[mode] if isinstance(mode, str) else int(mode)
        arr = (Out * max(len(ins), 1))(*[self._out_struct(d) for d in ins])
        g = None
        if ant_gain is not None:
            g = np.ascontiguousarray(ant_gain, dtype=np.float32).reshape(-1)
            if g.size != len(ins):
                raise ValueError("one gain per antenna is required")
            g = g.ctypes.data_as(C.POINTER(C.c_float))
        o = self._out_struct(out)
        self._check(_lib.wifirx_diversity_combine(self._h, len(ins), arr, int(n_slots), mode, g, C.byref(o), used_mask_ptr))

    def demod_diversity(self, iqs, slot_len, mode=DIV_MRC, ant_gain=None, soft=False, psdu_stride=2048) -> dict:
        """Host convenience (PCIe-bound): iqs = one complex64 array per antenna, slot i of each the same transmission.  Every
        array is demodulated, the batches are combined (diversity_combine_dev) and the result is decoded (soft=True: on the
        LLRs).  The handle needs want_carrier (and llr_bits > 0 for soft).  Returns the combined batch -- frames, psdu, idx,
        llr, carrier -- and used_mask (uint8 [n_slots], bit a = antenna a contributed)."""
        if not self.cfg.want_carrier:
            raise ValueError("demod_diversity needs a handle created with want_carrier=True")
        iqs = [np.ascontiguousarray(x, dtype=np.complex64).reshape(-1) for x in iqs]
        if not iqs or any(x.size != iqs[0].size for x in iqs) or iqs[0].size % slot_len:
            raise ValueError("one array of n_slots * slot_len samples per antenna is required")
        n = iqs[0].size // slot_len
        d_iq, ins, out, d_mask = self.alloc(max(iqs[0].nbytes, 1)), [], None, None
        try:
            for x in iqs:
                ins.append(self.alloc_out(n, want_csi=True))
                d_iq.upload(x)                                  # ordered behind the previous antenna's demod on the stream
                self.demod_batch_dev(d_iq.ptr, slot_len, n, ins[-1])
            out = self.alloc_out(n, psdu_stride=psdu_stride)
            d_mask = self.alloc(max(n, 1)).upload(np.zeros(max(n, 1), np.uint8))
            self.diversity_combine_dev(ins, n, out, mode, ant_gain, d_mask.ptr)
            if soft:
                self.decode_batch_soft_dev(n, out)
            else:
                self.decode_batch_dev(n, out)
            self.sync()
            r = self.download_out(out, n)
            r["used_mask"] = d_mask.download(np.uint8, n)
            return r
        finally:
            d_iq.free()
            for d in ins:
                self.free_out(d)
            if out is not None:
                self.free_out(out)
            if d_mask is not None:
                d_mask.free()

    # -- pre-detection combining (wifirx_precombine; NUMERICS.md rule 33) --
    def precombine_dev(self, iq_ptrs, slot_len, n_slots, out_ptr, iters=2, weights_ptr=None, stats_ptr=None):
        """wifirx_precombine on device buffers: iq_ptrs = one device pointer per antenna to [n_slots][slot_len] float pairs,
        slot i of every antenna the same transmission; out_ptr receives the one row set that demod_batch_dev reads as it is.
        iters: 0 .. 4 power iterations.  weights_ptr: [n_slots][n_ant] pairs, stats_ptr: [n_slots] PRE_STATS_DTYPE rows (None:
        not wanted).  Asynchronous on the handle's stream, behind its earlier calls."""
        arr = (C.c_void_p * max(len(iq_ptrs), 1))(*[None if p is None else int(p) for p in iq_ptrs])
        self._check(_lib.wifirx_precombine(self._h, len(iq_ptrs), arr, int(slot_len), int(n_slots), int(iters), out_ptr,
                                           weights_ptr, stats_ptr))

    def _precombine_host(self, iqs, slot_len, iters, bufs):
        """uploads the antennas, allocates y, weights and stats into `bufs` (the caller frees them) and queues the call:
        (n_slots, n_ant, d_y, d_w, d_s)"""
        iqs = [np.ascontiguousarray(x, dtype=np.complex64).reshape(-1) for x in iqs]
        if not iqs or any(x.size != iqs[0].size for x in iqs) or iqs[0].size % slot_len:
            raise ValueError("one array of n_slots * slot_len samples per antenna is required")
        n, A = iqs[0].size // slot_len, len(iqs)
        for x in iqs:
            bufs.append(self.alloc(max(x.nbytes, 1)).upload(x))
        for nbytes in (iqs[0].nbytes, n * A * 8, n * 16):
            bufs.append(self.alloc(max(nbytes, 1)))
        d_y, d_w, d_s = bufs[A:]
        self.precombine_dev([b.ptr for b in bufs[:A]], slot_len, n, d_y.ptr, iters, d_w.ptr, d_s.ptr)
        return n, A, d_y, d_w, d_s

    def precombine(self, iqs, slot_len, iters=2):
        """Host convenience (PCIe-bound: every antenna's samples cross the bus for one row set back): iqs = one complex64 array
        per antenna.  Returns (y complex64 [n_slots, slot_len], weights complex64 [n_slots, n_ant], stats PRE_STATS_DTYPE
        [n_slots])."""
        bufs = []
        try:
            n, A, d_y, d_w, d_s = self._precombine_host(iqs, slot_len, iters, bufs)
            self.sync()
            return (d_y.download(np.complex64, n * slot_len).reshape(n, slot_len),
                    d_w.download(np.complex64, n * A).reshape(n, A), d_s.download(PRE_STATS_DTYPE, n))
        finally:
            for b in bufs:
                b.free()

    def demod_precombined(self, iqs, slot_len, iters=2, soft=False, psdu_stride=2048) -> dict:
        """Host convenience (PCIe-bound, as demod_diversity): iqs = one complex64 array per antenna, slot i of each the same
        transmission.  The antennas are combined in front of the detector (precombine_dev), the one row set is demodulated
        ONCE and decoded (soft=True: on the LLRs, which needs llr_bits > 0).  Returns the batch -- frames, psdu, idx, llr,
        carrier where the handle produces them -- plus weights (complex64 [n_slots, n_ant]) and pre_stats (PRE_STATS_DTYPE)."""
        bufs, out = [], None
        try:
            n, A, d_y, d_w, d_s = self._precombine_host(iqs, slot_len, iters, bufs)
            out = self.alloc_out(n, psdu_stride=psdu_stride)
            self.demod_batch_dev(d_y.ptr, slot_len, n, out)
            if soft:
                self.decode_batch_soft_dev(n, out)
            else:
                self.decode_batch_dev(n, out)
            self.sync()
            r = self.download_out(out, n)
            r["weights"] = d_w.download(np.complex64, n * A).reshape(n, A)
            r["pre_stats"] = d_s.download(PRE_STATS_DTYPE, n)
            return r
        finally:
            for b in bufs:
                b.free()
            if out is not None:
                self.free_out(out)

    # -- stream mode --
    def push(self, iq: np.ndarray):
        iq = np.ascontiguousarray(iq, dtype=np.complex64).reshape(-1)
        self._check(_lib.wifirx_push(self._h, _np_ptr(iq), iq.size, 0))

    def push_iq(self, x, fmt=None, scale=None):
        """wifirx_push_iq: samples in their native format.  fmt None: taken from an int16 (sc16) / int8 (sc8) array of shape
        [n, 2] or flat [2 n]; "fc32" (complex64) is push().  scale None: 2^-15 for sc16, 2^-7 for sc8."""
        if fmt is not None and iq_format(fmt) == IQ_FC32:
            x = np.ascontiguousarray(x, dtype=np.complex64).reshape(-1)
            self._check(_lib.wifirx_push_iq(self._h, _np_ptr(x), x.size, IQ_FC32, float(1.0 if scale is None else scale), 0))
            return
        x, fmt, n = self._iq_array(x, fmt)
        self._check(_lib.wifirx_push_iq(self._h, _np_ptr(x), n, *_fmt_scale(fmt, scale), 0))

    def push_iq_dev(self, ptr, n, fmt, scale=None):
        """wifirx_push_iq on n samples of `fmt` in device memory at ptr"""
        self._check(_lib.wifirx_push_iq(self._h, ptr, int(n), *_fmt_scale(fmt, scale), 1))

    def flush(self):
        self._check(_lib.wifirx_push(self._h, None, 0, 0))

    # -- stream-mode receive diversity (wifirx_push_diversity; NUMERICS.md rules 24 and 23) --
    def _push_diversity(self, ptrs, n, mode, ant_gain, fmt, scale, on_device):
        mode = DIV_MODES[mode] if isinstance(mode, str) else int(mode)
        n_ant = len(ptrs)
        g = None
        if ant_gain is not None:
            g = np.ascontiguousarray(ant_gain, dtype=np.float32).reshape(-1)
            if g.size != n_ant:
                raise ValueError("one gain per antenna is required")
        cfg = DivStream(n_ant, mode, None if g is None else g.ctypes.data_as(C.POINTER(C.c_float)), *_fmt_scale(fmt, scale),
                        int(on_device))
        arr = (C.c_void_p * max(n_ant, 1))(*ptrs)
        self._check(_lib.wifirx_push_diversity(self._h, C.byref(cfg), arr, int(n)))
        self._div_n_ant = n_ant

    def push_diversity(self, iqs, mode=DIV_MRC, ant_gain=None, fmt=None, scale=None):
        """wifirx_push_diversity on host arrays: iqs = one array per antenna of ONE radio (sample-synchronous, one length), the
        next samples of each.  fmt None: complex64, or taken from int16 (sc16) / int8 (sc8) arrays of shape [n, 2] or flat
        [2 n]; scale None: the format's conventional one.  mode: DIV_MRC / DIV_SELECT (or "mrc" / "select"); ant_gain: one
        finite float >= 0 per antenna, the inverse noise power (None: equal noise).  The number of antennas is fixed by the
        handle's first call, and a handle that has taken samples through push() takes none here."""
        if fmt is None and np.asarray(iqs[0]).dtype.kind != "i":
            fmt = IQ_FC32
        if fmt is not None and iq_format(fmt) == IQ_FC32:
            keep, fmt = [np.ascontiguousarray(x, dtype=np.complex64).reshape(-1) for x in iqs], IQ_FC32
            ns = [x.size for x in keep]
        else:
            conv = [self._iq_array(x, fmt) for x in iqs]
            keep, fmt, ns = [c[0] for c in conv], conv[0][1], [c[2] for c in conv]
            if any(c[1] != fmt for c in conv):
                raise ValueError("one sample format for all antennas")
        if len(set(ns)) != 1:
            raise ValueError("the antennas of one radio deliver the same number of samples")
        self._push_diversity([x.ctypes.data for x in keep], ns[0], mode, ant_gain, fmt, scale, 0)

    def push_diversity_dev(self, ptrs, n, mode=DIV_MRC, ant_gain=None, fmt="fc32", scale=None):
        """wifirx_push_diversity on device memory: ptrs = one pointer per antenna to its next n samples of `fmt`"""
        self._push_diversity([int(p) for p in ptrs], n, mode, ant_gain, iq_format(fmt), scale, 1)

    def flush_diversity(self, mode=DIV_MRC, ant_gain=None, n_ant=None):
        """end of the diversity stream: settles the frames still waiting for samples (n_ant: that of the pushes before)"""
        n_ant = getattr(self, "_div_n_ant", 1) if n_ant is None else int(n_ant)
        self._push_diversity([None] * n_ant, 0, mode, ant_gain, IQ_FC32, None, 0)

    def poll_diversity(self, cap=256, psdu_stride=2048, want_idx=False, want_csi=False, want_stats=False, trim_psdu=False,
                       n_ant=None):
        """poll() for a diversity stream: the same dict plus used_mask (uint8 [n], bit a = antenna a contributed to the
        frame) and ant_frames (records [n, n_ant]: every antenna's own record of the frame, with the joint trigger)."""
        ms = self.cfg.max_sym
        n_ant = getattr(self, "_div_n_ant", 1) if n_ant is None else int(n_ant)
        frames, psdu = np.zeros(cap, dtype=FRAME_DTYPE), np.zeros((cap, psdu_stride), dtype=np.uint8)
        idx = np.zeros((cap, ms, 48), dtype=np.uint8) if want_idx else None
        car = np.zeros((cap, ms, 48), dtype=np.complex64) if self.cfg.want_carrier else None
        csi = np.zeros((cap, 52), dtype=np.complex64) if want_csi else None
        stats = np.zeros((cap, 4), dtype=np.float32) if want_stats else None
        used, ant = np.zeros(cap, dtype=np.uint8), np.zeros((cap, n_ant), dtype=FRAME_DTYPE)
        out = PollOut(_np_ptr(frames), _np_ptr(psdu), psdu_stride, 0, _np_ptr(idx), _np_ptr(car), _np_ptr(csi), _np_ptr(stats))
        n = C.c_uint32(0)
        self._check(_lib.wifirx_poll_diversity(self._h, C.byref(out), _np_ptr(used), _np_ptr(ant), cap, C.byref(n)))
        n = n.value
        w = psdu_stride
        if trim_psdu and n:
            w = min(max(int(frames["psdu_len"][:n].max()), 1), psdu_stride)
        return dict(frames=frames[:n].copy(), psdu=psdu[:n, :w].copy(), idx=None if idx is None else idx[:n].copy(),
                    carrier=None if car is None else car[:n].copy(), csi=None if csi is None else csi[:n].copy(),
                    sym_stats=None if stats is None else stats[:n].copy(), used_mask=used[:n].copy(), ant_frames=ant[:n].copy())

    def detect_multi_dev(self, iq_ptrs, n, threshold, masks_ptr, A_ptr, P_ptr=None):
        """wifirx_detect_multi: NUMERICS.md rule 24 over n samples of every antenna at the device pointers iq_ptrs, from the
        capture's origin: masks (uint64 [ceil(n / 64)]) at masks_ptr, A (complex64 [n]) at A_ptr, P (float32 [n]) at P_ptr
        or None.  One antenna is the stream detector's metric.  Asynchronous on the handle's stream."""
        ptrs = [int(p) if p is not None else None for p in iq_ptrs]
        arr = (C.c_void_p * max(len(ptrs), 1))(*ptrs)
        self._check(_lib.wifirx_detect_multi(self._h, len(ptrs), arr, int(n), float(threshold), masks_ptr, A_ptr, P_ptr))

    def queued(self) -> int:
        """finished frames waiting for poll()"""
        return int(_lib.wifirx_queued(self._h))

    def push_consumed(self) -> int:
        """Leading samples of the last push() the stream has taken over (after an error: where to repeat it from)."""
        return int(_lib.wifirx_push_consumed(self._h))

    def poll(self, cap=256, psdu_stride=2048, want_idx=False, want_csi=False, want_stats=False, trim_psdu=False):
        """Finished frames of the stream, oldest first (at most `cap`).  The landing buffers are kept between calls
        (a scheduler polls after every work()); what is returned are copies of the filled part."""
        ms = self.cfg.max_sym
        key = (cap, psdu_stride, bool(want_idx), bool(want_csi), bool(want_stats))
        if getattr(self, "_poll_key", None) != key:
            self._poll_key = key
            self._poll_buf = (np.zeros(cap, dtype=FRAME_DTYPE), np.zeros((cap, psdu_stride), dtype=np.uint8),
                              np.zeros((cap, ms, 48), dtype=np.uint8) if want_idx else None,
                              np.zeros((cap, ms, 48), dtype=np.complex64) if self.cfg.want_carrier else None,
                              np.zeros((cap, 52), dtype=np.complex64) if want_csi else None,
                              np.zeros((cap, 4), dtype=np.float32) if want_stats else None)
            frames, psdu, idx, car, csi, stats = self._poll_buf
            self._poll_out = PollOut(_np_ptr(frames), _np_ptr(psdu), psdu_stride, 0, _np_ptr(idx), _np_ptr(car),
                                     _np_ptr(csi), _np_ptr(stats))
        frames, psdu, idx, car, csi, stats = self._poll_buf
        n = C.c_uint32(0)
        self._check(_lib.wifirx_poll_ex(self._h, C.byref(self._poll_out), cap, C.byref(n)))
        n = n.value
        # trim_psdu: the rows are cut to the longest PSDU of the call before they are copied (a frame usually fills a fraction
        # of its 2048-byte row; the block polls this way)
        w = psdu_stride
        if trim_psdu and n:
            w = min(max(int(frames["psdu_len"][:n].max()), 1), psdu_stride)
        return dict(frames=frames[:n].copy(), psdu=psdu[:n, :w].copy(), idx=None if idx is None else idx[:n].copy(),
                    carrier=None if car is None else car[:n].copy(), csi=None if csi is None else csi[:n].copy(),
                    sym_stats=None if stats is None else stats[:n].copy())
