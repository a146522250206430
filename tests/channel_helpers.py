"""What the device channel's GPU tests share (test_gpu_channel.py, test_gpu_resample.py, test_gpu_fading.py): the handle, the
inputs, one call into a NaN-filled buffer, and the loop-back chain with its comparison against the oracle."""
import ctypes as C
import os

import numpy as np
import pytest

from wifirx import capi, txgen

NAN_WORD = np.uint32(0x7FC0DEAD)
ONE = 1 << 40                       # one sample of drift (NUMERICS.md rule 18)
M64 = 0xFFFFFFFFFFFFFFFF


@pytest.fixture(scope="module")
def rx():
    r = capi.WifiRx(max_sym=1, device=0)
    yield r
    r.close()


def P(a):
    """the pointer argument of a direct ABI call for a NumPy array, or None"""
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def cnoise(rng, n):
    return ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) * 0.5).astype(np.complex64)


def tap_sets(rng, n_sets, L):
    return ((rng.standard_normal((n_sets, L)) + 1j * rng.standard_normal((n_sets, L))) / np.sqrt(2 * L)).astype(np.complex64)


def same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def run(rx, x, cap, n_rows, out_shift=0, taps=(1.0,), taps_dev=False, **kw):
    """channel_dev from a device copy of x into a NaN-filled buffer (out_shift = 1: 8 bytes past a 16-byte boundary), with
    host taps or a device copy of them; returns the cap samples at the output pointer"""
    d_in = rx.alloc(max(cap, 1) * 8).upload(x)
    d_out = rx.alloc((cap + 1) * 8).upload(np.full(2 * (cap + 1), NAN_WORD, np.uint32))
    t = np.asarray(taps, np.complex64)
    t = t[None] if t.ndim == 1 else t
    d_t = None
    try:
        if taps_dev:
            d_t = rx.alloc(t.nbytes).upload(t)
            rx.channel_dev(d_in.ptr, d_out.ptr + 8 * out_shift, cap, n_rows, taps=d_t.ptr, n_taps=t.shape[1],
                           n_tap_sets=t.shape[0], **kw)
        else:
            rx.channel_dev(d_in.ptr, d_out.ptr + 8 * out_shift, cap, n_rows, taps=t, **kw)
        return d_out.download(np.complex64, cap + 1)[out_shift:out_shift + cap]
    finally:
        d_in.free()
        d_out.free()
        if d_t is not None:
            d_t.free()


def loopback(psdus, enc, lead, slot, chan_est, channels, psdu_stride, pick=None):
    """TX -> channel -> demod -> decode_mac on the device: the frames of `psdus` ([n, plen]) in rows of `slot` samples, once
    through each channel of `channels` (keywords of channel_dev).  An FCS-good frame carries its own PSDU.  Returns per
    channel (the downloaded decode result, the channel's output rows as one 1-D array: all, or those of the frames `pick`)"""
    n, plen = psdus.shape
    rx = capi.WifiRx(max_sym=txgen.n_sym_for(plen, enc), llr_bits=0, chan_est=chan_est, device=0)
    out = []
    try:
        rows = rx.alloc(n * slot * 8)
        rx.tx_batch_dev(rows.ptr, n * slot, psdus, enc, lead=lead, row_len=slot)
        iq = rx.alloc(n * slot * 8)
        for kw in channels:
            rx.channel_dev(rows.ptr, iq.ptr, n * slot, n, row_len=slot, **kw)
            dev = rx.alloc_out(n, psdu_stride=psdu_stride, want_hbits=True)
            rx.demod_batch_dev(iq.ptr, slot, n, dev)
            rx.decode_batch_dev(n, dev)
            rx.sync()
            r = rx.download_out(dev, n)
            rx.free_out(dev)
            crc = (r["frames"]["flags"] & capi.F_CRC_OK) != 0
            assert (r["psdu"][crc][:, :plen] == psdus[crc]).all(), "an FCS-good frame carries another PSDU"
            if pick is None:
                x = iq.download(np.complex64, n * slot)
            else:
                x = np.empty((len(pick), slot), np.complex64)
                for i, f in enumerate(pick):
                    rx._check(capi.lib().wifirx_memcpy_d2h(rx._h, P(x[i]), iq.ptr + int(f) * slot * 8, slot * 8))
            out.append((r, x.reshape(-1)))
        rows.free()
        iq.free()
    finally:
        rx.close()
    return out


def assert_oracle_records(orc, r, x, slot, pick=slice(None), msg=None, **params):
    """the records and the decisions of the device result r (of the frames `pick`) equal the oracle's on the rows x"""
    o = orc.demod_batch(x, slot, orc.make_params(**params), n_threads=min(os.cpu_count() or 1, 16))
    rec = r["frames"][pick].copy()
    rec["flags"] &= ~np.uint32(capi.F_DECODED | capi.F_CRC_OK)
    assert np.array_equal(rec, o["frames"]), msg
    assert np.array_equal(r["idx"][pick], o["idx"]), msg
