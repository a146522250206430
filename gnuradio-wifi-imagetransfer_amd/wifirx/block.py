"""``wifi_phy_rx`` -- drop-in for the RX half of the reference's ``wifi_phy_hier`` hier block (``wifi_phy_tx``, at the
end of this file, is the TX half).

Port names, parameters and setters are those of gnu_radio/wifi_phy_hier.grc (pad ``samp_in``
:587-604, message pads ``mac_out`` / ``carrier`` :605-640, parameters ``bandwidth``, ``chan_est``,
``encoding``, ``frequency``, ``sensitivity`` :83-92,299-308,442-451,501-510,681-690); inside
IRS_AP it replaces the inlined blocks gnu_radio/IRS_AP.py:268-269,271-273,276-285 and feeds the
consumers wired at :291-293.  ``work()`` hands the complex64 chunk through the ctypes C ABI to
the HIP chain (wifirx_push) and publishes what wifirx_poll returns:

* ``mac_out``: ``(meta, u8vector)`` with the MAC frame *without* FCS, starting at the 24-byte MAC
  header (what ``decode_mac`` publishes; the consumer strips ``[24:][4:]``,
  gnu_radio/IRS_AP_epy_block_2.py:31-36); ``meta`` carries ``frame_bytes, encoding, snr, freq,
  freq_offset, dlt``.
* ``carrier``: ``({}, c32vector[48])`` per data symbol (``frame_equalizer.symbols``,
  gnu_radio/IRS_AP.py:293).

Frames with a bad SIGNAL parity or FCS are dropped silently, as in the reference; ``work()``
never raises for channel conditions.
"""
from __future__ import annotations

import ctypes
import math

import numpy as np

from . import capi, grshim, probe, txgen
from . import irs as irs_mod

LS, LMS, COMB, STA = 0, 1, 2, 3
_C64 = np.dtype(np.complex64)
_ANCHOR = ctypes.c_char * 1
LINKTYPE_IEEE802_11 = 105


class wifi_phy_rx(grshim.sync_block):
    def __init__(self, bandwidth=10e6, chan_est=LS, encoding=0, frequency=5.89e9, sensitivity=0.56,
                 max_sym=511, publish_carrier=True, device=0, batch_samples=None, publish_csi=False, snr_probe=None,
                 soft_decision=False, sample_format="fc32", sample_scale=None, antennas=1, diversity="mrc", ant_gain=None,
                 dc_block=False, iq_correct=False, fe_frac_bits=12, fe_dc_shift=2, fe_iq_shift=4):
        # sample_format: "fc32" (complex64 items, the default), or "sc16" / "sc8": items of two int16 / int8 (I, Q), the form
        # a UHD source with an sc16 CPU format delivers; they cross the bus as they are and are widened on the device
        # (value = integer * sample_scale, default 2^-15 / 2^-7; wifirx_push_iq, NUMERICS.md rule 20)
        sf = _sample_format(sample_format, sample_scale)
        self.sample_format, self.sample_scale, self._item, in_sig = sf.fmt, sf.scale, sf.item, sf.in_sig
        # antennas = A > 1: A `samp_in` ports of the item type, the sample-synchronous channels of ONE radio (a two-channel
        # uhd.usrp_source).  Detection runs once, on all of them (NUMERICS.md rule 24), the antennas' equalised points are
        # combined (`diversity`: "mrc" or "select"; ant_gain: the inverse noise power per antenna, None = equal; rule 23) and
        # decoded once; `mac_out` and `carrier` are as with one antenna, with `antennas_used` (bit a = antenna a contributed)
        # added to the PDU's dictionary.  antennas = 1 is the single-stream path, untouched.
        self.antennas = int(antennas)
        if not 1 <= self.antennas <= capi.DIV_MAX_ANT:
            raise ValueError("antennas must be 1 .. %d" % capi.DIV_MAX_ANT)
        if diversity not in capi.DIV_MODES:
            raise ValueError("diversity must be 'mrc' or 'select'")
        self.diversity = diversity
        self.ant_gain = None
        if ant_gain is not None:
            self.ant_gain = np.array(ant_gain, dtype=np.float32).reshape(-1)
            if self.ant_gain.size != self.antennas or not (np.isfinite(self.ant_gain).all() and (self.ant_gain >= 0).all()):
                raise ValueError("ant_gain: one finite value >= 0 per antenna")
        # dc_block / iq_correct: the receive front end of NUMERICS.md rule 32 on the samples as they come in, in front of the
        # detection (wifirx_stream_frontend): the mean of the last 2^fe_dc_shift blocks of 4096 samples is removed, and the
        # image of a gain / phase imbalance between I and Q is estimated blindly over 2^fe_iq_shift blocks and removed.  Both
        # off by default; iq_correct assumes traffic whose frames are not all very short (rule 32).  One antenna only.
        self.dc_block, self.iq_correct = bool(dc_block), bool(iq_correct)
        self.fe_frac_bits, self.fe_dc_shift, self.fe_iq_shift = int(fe_frac_bits), int(fe_dc_shift), int(fe_iq_shift)
        if not (0 <= self.fe_frac_bits <= 30 and 0 <= self.fe_dc_shift <= 6 and 0 <= self.fe_iq_shift <= 6):
            raise ValueError("fe_frac_bits must be 0 .. 30, fe_dc_shift and fe_iq_shift 0 .. 6")
        if (self.dc_block or self.iq_correct) and self.antennas > 1:
            raise ValueError("dc_block / iq_correct are not available with antennas > 1")
        grshim.sync_block.__init__(self, name="wifi_phy_rx", in_sig=in_sig * self.antennas, out_sig=None)
        self.bandwidth = float(bandwidth)
        self.chan_est = int(chan_est)
        self.encoding = encoding            # TX-side parameter of the hier block: accepted, unused on RX
        self.frequency = float(frequency)
        self.sensitivity = float(sensitivity)
        self.publish_carrier = bool(publish_carrier)
        self.publish_csi = bool(publish_csi)      # "csi" entry of the mac_out dictionary, as upstream's frame_equalizer tags it
        # snr_probe = (type, msg_nsamples, alpha) or True for the reference's (0, 1000, 0.05): the
        # digital.probe_mpsk_snr_est_c of gnu_radio/IRS_AP.py:275,312, fed with per-frame moments from the device
        # (no equalised points cross the bus); its `snr` / `signal` / `noise` ports are self.snr_probe's
        self.snr_probe = None
        if snr_probe:
            args = (0, 1000, 0.05) if snr_probe is True else tuple(snr_probe)
            self.snr_probe = probe.probe_mpsk_snr_est(*args)
        self.message_port_register_out(grshim.intern("mac_out"))
        self.message_port_register_out(grshim.intern("carrier"))
        self._rx = capi.WifiRx(bandwidth=self.bandwidth, frequency=self.frequency, sensitivity=self.sensitivity,
                               chan_est=self.chan_est, max_sym=max_sym, llr_bits=0,
                               want_carrier=self.publish_carrier, device=device)
        # The scheduler calls work() with a few thousand items.  The library copies them into a pinned staging buffer
        # and returns; once `batch_samples` have come in its worker thread runs the device pipeline for that batch while
        # work() keeps filling the next one -- one device round trip per work() call could not keep up.  Default: 50 ms
        # of signal at the block's bandwidth (2^16 samples at least), so that a PDU leaves `mac_out` about 50-100 ms
        # after its last sample arrived (the reference's decode_mac publishes per frame; INTEGRATION.md, "Latency"); a
        # file-driven run that only cares for throughput passes a larger value (bench.py: 2^22).  Finished frames are
        # published by the first work() call after their batch is through (wifirx_queued: one atomic load per call), and
        # at stop().
        if batch_samples is None:
            batch_samples = max(1 << 16, int(0.05 * self.bandwidth))
        self.batch_samples = min(int(batch_samples), capi.STREAM_BATCH_MAX)
        self._rx.set_param(capi.P_STREAM_BATCH, self.batch_samples)
        self._rx.set_param(capi.P_STREAM_IDX, 0)            # PDUs only: the hard decisions stay on the device
        self.soft_decision = False
        if soft_decision:
            self.set_soft_decision(True)
        self._fe_on = False
        if self.dc_block or self.iq_correct:
            self._set_frontend()
        self._push = capi.lib().wifirx_push
        if self.sample_format != capi.IQ_FC32:
            push_iq, fmt, scale = capi.lib().wifirx_push_iq, self.sample_format, self.sample_scale
            self._push = lambda h, buf, n, on_device: push_iq(h, buf, n, fmt, scale, on_device)
        self._queued = capi.lib().wifirx_queued
        self._h = self._rx._h
        self._p_mac = grshim.intern("mac_out")
        self._p_car = grshim.intern("carrier")
        self.frames_ok = 0
        self.frames_dropped = 0
        self.raise_on_error = True
        self.push_errors = 0
        self.last_error = ""
        self.stream_dead = False        # the library has declared the stream dead (WIFIRX_EDEAD): work() ends the block

    # ---- setters generated for the hier block's parameters (gnu_radio/IRS_user.py:229,265,273;
    #      equaliser setters at gnu_radio/IRS_AP.py:348,373,382) ----
    def get_bandwidth(self):
        return self.bandwidth

    def set_bandwidth(self, bandwidth):
        self.bandwidth = float(bandwidth)
        self._rx.set_param(capi.P_BANDWIDTH, self.bandwidth)

    def get_frequency(self):
        return self.frequency

    def set_frequency(self, frequency):
        self.frequency = float(frequency)
        self._rx.set_param(capi.P_FREQUENCY, self.frequency)

    def get_chan_est(self):
        return self.chan_est

    def set_chan_est(self, chan_est):
        self._rx.set_param(capi.P_CHAN_EST, int(chan_est))     # LS, LMS, COMB, STA
        self.chan_est = int(chan_est)

    set_algorithm = set_chan_est                                # frame_equalizer.set_algorithm

    def get_sensitivity(self):
        return self.sensitivity

    def set_sensitivity(self, sensitivity):
        self._rx.set_param(capi.P_SENSITIVITY, float(sensitivity))      # refuses a negative value or a NaN: the old one stays
        self.sensitivity = float(sensitivity)

    def _set_frontend(self):
        """the handle's front end as dc_block / iq_correct say; a front end that stays on keeps its state"""
        on = self.dc_block or self.iq_correct
        if on and self.antennas > 1:
            raise ValueError("dc_block / iq_correct are not available with antennas > 1")
        init = None
        if on and self._fe_on:
            self._rx.flush()                                    # what is staged runs under the old setting
            init = self._rx.stream_frontend_state()
        cfg = capi.frontend_cfg(self.dc_block, self.iq_correct, self.fe_frac_bits, self.fe_dc_shift, self.fe_iq_shift) if on else None
        self._rx.stream_frontend(cfg, init)
        self._fe_on = on

    def get_dc_block(self):
        return self.dc_block

    def set_dc_block(self, dc_block):
        """DC removal (NUMERICS.md rule 32) for the samples that come in after the call"""
        old, self.dc_block = self.dc_block, bool(dc_block)
        try:
            self._set_frontend()
        except Exception:
            self.dc_block = old
            raise

    def get_iq_correct(self):
        return self.iq_correct

    def set_iq_correct(self, iq_correct):
        """blind IQ-imbalance correction (NUMERICS.md rule 32) for the samples that come in after the call"""
        old, self.iq_correct = self.iq_correct, bool(iq_correct)
        try:
            self._set_frontend()
        except Exception:
            self.iq_correct = old
            raise

    def get_soft_decision(self):
        return self.soft_decision

    def set_soft_decision(self, soft_decision):
        """True: decode_mac runs the soft-decision Viterbi on channel-state-weighted LLRs (WIFIRX_P_STREAM_SOFT and
        WIFIRX_P_LLR_CSI, NUMERICS.md rules 12 and 14) for the batches that run after the call; False: upstream's hard
        decoder (the default).  `mac_out` PDUs keep their format either way."""
        on = 1 if soft_decision else 0
        self._rx.set_param(capi.P_STREAM_SOFT, on)
        self._rx.set_param(capi.P_LLR_CSI, on)
        self.soft_decision = bool(on)

    def get_encoding(self):
        return self.encoding

    def set_encoding(self, encoding):
        self.encoding = encoding

    # ---- stream interface ----
    def _work_diversity(self, input_items):
        """work() with antennas > 1: the common length of the ports is pushed and consumed on every port.  A failed push has
        taken nothing (it is all or nothing): with raise_on_error it raises, otherwise 0 items are consumed and the scheduler
        hands them in again; a dead stream ends the block."""
        n = min(len(x) for x in input_items[:self.antennas])
        if n:
            xs = [x[:n] for x in input_items[:self.antennas]]
            try:
                self._rx.push_diversity(xs, self.diversity, self.ant_gain, self.sample_format, self.sample_scale)
            except capi.WifiRxError as e:
                self.push_errors += 1
                self.last_error = str(e)
                if e.code == capi.EDEAD:
                    self.stream_dead = True
                    self._publish()
                    if self.raise_on_error:
                        raise
                    return -1
                if self.raise_on_error:
                    raise
                n = 0
            if self._queued(self._h):
                self._publish()
        return n

    def work(self, input_items, output_items):
        if self.antennas > 1:
            return self._work_diversity(input_items)
        x = input_items[0]
        n = len(x)
        if n:
            if x.dtype != self._item or not x.flags.c_contiguous:
                x = np.ascontiguousarray(x, dtype=self._item)
            try:
                buf = _ANCHOR.from_buffer(x)                 # the address of x's data, without building a dict
            except (TypeError, ValueError):                  # read-only input: the slower route
                buf = x.ctypes.data
            rc = self._push(self._h, buf, n, 0)              # copies; x is the scheduler's again
            if rc:
                # Nothing is lost or doubled: what the library took over (usually nothing) counts as consumed, the
                # scheduler hands the rest in again with the next call (include/wifirx.h, WIFIRX_P_STREAM_BATCH: ERRORS).
                # raise_on_error (default): the error surfaces as an exception of the block, as any failing GNU Radio
                # block's would; otherwise it is counted and work() reports the consumed items.
                self.push_errors += 1
                self.last_error = capi.lib().wifirx_last_error(self._h).decode()
                if rc == capi.EDEAD:
                    # the stream is gone for good (include/wifirx.h: ERRORS): returning "0 items consumed" would have the
                    # scheduler hand the same items in for ever.  Publish what is finished, then end the block -- by the
                    # exception with raise_on_error, by WORK_DONE (-1) without.
                    self.stream_dead = True
                    self._publish()
                    if self.raise_on_error:
                        self._rx._check(rc)
                    return -1
                if self.raise_on_error:
                    self._rx._check(rc)
                n = self._rx.push_consumed()
            if self._queued(self._h):
                self._publish()
        return n

    def stop(self):
        """End of stream: settle the frames still waiting for samples.  A batch that failed on the library's worker thread is
        reported by the first flush (once, before it does anything) and run again by the second: flush until it goes through
        (at most three times), publish whatever is finished in any case, and only then -- with raise_on_error -- raise."""
        if self.antennas > 1:
            try:
                if not self.stream_dead:
                    self._rx.flush_diversity(self.diversity, self.ant_gain, self.antennas)
            except capi.WifiRxError as e:
                self.push_errors += 1
                self.last_error = str(e)
                self.stream_dead = self.stream_dead or e.code == capi.EDEAD
                if self.raise_on_error:
                    raise
            finally:
                self._publish()
            return True
        rc = 0
        try:
            for _ in range(3):
                if self.stream_dead:                 # no flush can succeed any more (work() has reported it)
                    break
                rc = self._push(self._h, None, 0, 0)
                if rc == 0:
                    break
                self.push_errors += 1
                self.last_error = capi.lib().wifirx_last_error(self._h).decode()
                if rc == capi.EDEAD:
                    self.stream_dead = True
        finally:
            self._publish()
        if rc and self.raise_on_error:
            self._rx._check(rc)
        return True

    def _publish(self):
        """Everything the library has finished so far, as PDUs.  Per-frame fields are taken out of the record array
        column by column (one tolist() per field, not a NumPy scalar conversion per frame and field)."""
        pub, make = self.message_port_pub, grshim.make_pdu
        want_car = self.publish_carrier
        while True:
            poll = self._rx.poll if self.antennas == 1 else self._rx.poll_diversity
            r = poll(cap=1024, psdu_stride=2048, want_csi=self.publish_csi, want_stats=self.snr_probe is not None, trim_psdu=True)
            used = r.get("used_mask")           # diversity: which antennas contributed to every frame
            fr = r["frames"]
            nf = len(fr)
            if nf == 0:
                return
            flags = fr["flags"].tolist()
            n_out = fr["n_sym_out"].tolist()
            if self.snr_probe is not None:
                st = r["sym_stats"].tolist()
                for i in range(nf):
                    if n_out[i] > 0:
                        self.snr_probe.update_frame(st[i][0], st[i][1], st[i][2], 48 * n_out[i])
            if want_car and r["carrier"] is not None:
                car, p_car = r["carrier"], self._p_car
                if not grshim.HAVE_GNURADIO:
                    # on the shim a PDU is (dict, row view): rows by iteration over the frame's block (no index arithmetic per symbol)
                    for i in range(nf):
                        for row in car[i, :n_out[i]]:
                            pub(p_car, ({}, row))
                else:
                    for i in range(nf):
                        for sy in range(n_out[i]):
                            pub(p_car, make({}, car[i, sy]))
            ok = [i for i in range(nf) if flags[i] & capi.F_CRC_OK]
            self.frames_ok += len(ok)
            self.frames_dropped += nf - len(ok)
            if not ok:
                continue
            plen = fr["psdu_len"].tolist()
            enc = fr["encoding"].tolist()
            snr = fr["snr_db"].tolist()
            # sync_long's wifi_start tag as upstream forms it: (double)cfo_coarse - (double)cfo_fine
            foff = ((fr["cfo_coarse"].astype(np.float64) - fr["cfo_fine"].astype(np.float64))
                    * (self.bandwidth / (2 * math.pi))).tolist()
            psdu = r["psdu"]
            freq = self.frequency
            csi = r["csi"] if self.publish_csi else None
            p_mac = self._p_mac
            if csi is None and used is None and not grshim.HAVE_GNURADIO:
                # the common case on the shim, kept tight: a PDU is (dict, row view) -- poll() handed out its own copy of the rows
                for i in ok:
                    pub(p_mac, ({"frame_bytes": plen[i], "encoding": enc[i], "snr": snr[i], "freq": freq,
                                 "freq_offset": foff[i], "dlt": LINKTYPE_IEEE802_11}, psdu[i, :plen[i] - 4]))
                continue
            for i in ok:
                meta = {"frame_bytes": plen[i], "encoding": enc[i], "snr": snr[i], "freq": freq,
                        "freq_offset": foff[i], "dlt": LINKTYPE_IEEE802_11}
                if csi is not None:
                    meta["csi"] = csi[i]
                if used is not None:
                    meta["antennas_used"] = int(used[i])
                pub(p_mac, make(meta, psdu[i, :plen[i] - 4]))

    def get_probe_snr(self):
        """latest estimate of the SNR probe in dB (None without a probe)"""
        return None if self.snr_probe is None else self.snr_probe.snr()

    def stats(self):
        return self._rx.stats()

    def close(self):
        """Release the library handle (device buffers, stream)."""
        self._rx.close()


class _sample_format:
    """A block's input format: ``fmt`` (the WIFIRX_IQ_* value), ``scale`` (value = integer * scale; None: the format's
    conventional one), the dtype ``item`` of one component, the block's ``in_sig`` and ``bps``, the bytes per sample."""

    def __init__(self, sample_format, sample_scale):
        self.fmt = capi.iq_format(sample_format)
        if self.fmt not in capi.IQ_DTYPE:
            raise ValueError("sample_format must be 'fc32', 'sc16' or 'sc8'")
        self.scale = float(capi.IQ_SCALE[self.fmt] if sample_scale is None else sample_scale)
        self.item = capi.IQ_DTYPE[self.fmt]
        self.in_sig = [np.complex64] if self.fmt == capi.IQ_FC32 else [(self.item.type, 2)]
        self.bps = 8 if self.fmt == capi.IQ_FC32 else 2 * self.item.itemsize

    def items(self, x):
        """the scheduler's items as (contiguous bytes, number of samples)"""
        if x.dtype != self.item or not x.flags.c_contiguous:
            x = np.ascontiguousarray(x, dtype=self.item)
        return x.reshape(-1).view(np.uint8), len(x)

    def zeros(self, n):
        return np.zeros(n * self.bps, np.uint8)


class _hist_pair:
    """The history of a stream of calls, in two device buffers of ``nbytes`` used in turn: a call reads ``cur`` (None in
    front of a stream) and writes ``nxt``; ``advance()`` behind it."""

    def __init__(self, rx, nbytes):
        self._bufs = [rx.alloc(nbytes) for _ in range(2)]
        self._cur = None                                            # index of the buffer that holds the history

    @property
    def cur(self):
        return None if self._cur is None else self._bufs[self._cur].ptr

    @property
    def nxt(self):
        return self._bufs[1 if self._cur == 0 else 0].ptr

    def advance(self):
        self._cur = 1 if self._cur == 0 else 0

    def free(self):
        for b in self._bufs:
            b.free()
        self._bufs = []


class _channel_rx(wifi_phy_rx):
    """A receive chain of ``_fed_rx``: a ``wifi_phy_rx`` whose PDUs leave on the owner's ports, with ``channel`` (and on
    ``mac_out`` the ``freq`` it already carries: the channel's own centre) in their dictionaries; ``channel`` None: unchanged."""

    def __init__(self, owner, channel=None, **kw):
        self._owner, self._channel = owner, channel if channel is None else int(channel)
        wifi_phy_rx.__init__(self, **kw)

    def message_port_pub(self, port, msg):
        if self._channel is not None:
            meta, vec = grshim.to_python(msg)
            meta = dict(meta or {})
            meta["channel"] = self._channel
            msg = grshim.make_pdu(meta, vec) if grshim.HAVE_GNURADIO else (meta, vec)
        self._owner.message_port_pub(port, msg)


class _fed_rx(grshim.sync_block):
    """What ``wifi_phy_rx_wideband``, ``wifi_phy_rx_resampled`` and ``wifi_phy_rx_tuned`` share: a front stage on a handle
    of its own, then K ``wifi_phy_rx`` chains, chain k fed row k of the front stage's output as device input.  A subclass
    gives ``_front(raw, n)`` -> (device pointer of the rows, their stride in samples, samples per row), asynchronous on the
    front stage's handle, ``_close_front()`` and, where its stream ends with a flush, ``_flush_zeros()``."""

    def _build(self, name, sf, open_front, chains, **rx_kwargs):
        """The block's signature and ports, then -- the first touch of the library -- ``open_front()`` -> the front stage's
        handle, then one chain per dictionary of ``chains``; a failure closes what was built."""
        grshim.sync_block.__init__(self, name=name, in_sig=sf.in_sig, out_sig=None)
        self.message_port_register_out(grshim.intern("mac_out"))
        self.message_port_register_out(grshim.intern("carrier"))
        self._sf, self._rx = sf, []
        self._push = capi.lib().wifirx_push
        self.raise_on_error = True
        try:
            self._fh = open_front()
            for kw in chains:
                self._rx.append(_channel_rx(self, bandwidth=self.bandwidth, **kw, **rx_kwargs))
        except Exception:
            self.close()
            raise

    def _push_rows(self, ptr, stride, n):
        for k, rx in enumerate(self._rx):
            rc = self._push(rx._h, ptr + 8 * k * stride, n, 1)
            if rc:
                rx.push_errors += 1
                rx.last_error = capi.lib().wifirx_last_error(rx._h).decode()
                if self.raise_on_error:
                    rx._rx._check(rc)
            if rx._queued(rx._h):
                rx._publish()

    def _feed(self, raw, n):
        ptr, stride, got = self._front(raw, n)
        if got:
            self._fh.sync()                                         # the rows are read on the chains' own streams
            self._push_rows(ptr, stride, got)

    def work(self, input_items, output_items):
        raw, n = self._sf.items(input_items[0])
        if n:
            self._feed(raw, n)
        return n

    def _flush_zeros(self):
        """the zero samples that end the front stage's stream"""
        return 0

    def stop(self):
        """End of stream: the front stage's flush zeros, then every chain's pending frames."""
        n = self._flush_zeros()
        if n:
            self._feed(self._sf.zeros(n), n)
        for rx in self._rx:
            rx.stop()
        return True

    @property
    def frames_ok(self):
        return sum(rx.frames_ok for rx in self._rx)

    @property
    def frames_dropped(self):
        return sum(rx.frames_dropped for rx in self._rx)

    def stats(self):
        """the channels' wifirx_stats, channel 0 first"""
        return [rx.stats() for rx in self._rx]

    def close(self):
        """Release the device buffers and every handle."""
        self._close_front()
        for rx in getattr(self, "_rx", []):
            rx.close()
        self._rx = []


class wifi_phy_rx_wideband(_fed_rx):
    """``wifi_phy_rx`` for a front end that covers ``n_channels`` = 2, 4 or 8 adjacent channels in one stream: ``samp_in`` at
    ``n_channels * bandwidth``, split on the device by wifirx_channelize (NUMERICS.md rule 21) into ``n_channels`` streams
    that never leave it, each received by a ``wifi_phy_rx`` chain of its own.  ``stacking`` = 1: the channels' centres lie at
    ``center_frequency`` -+ bandwidth/2, -+ 3 bandwidth/2, ... (5180 / 5200 / 5220 / 5240 MHz around 5210 MHz); 0: at
    ``center_frequency + (k - n_channels/2) * bandwidth``.  ``sample_format`` / ``sample_scale`` as ``wifi_phy_rx``; every
    other keyword goes to the channels' ``wifi_phy_rx``.

    ``mac_out`` and ``carrier`` carry what ``wifi_phy_rx`` publishes, with ``channel`` (k) added to the dictionaries;
    ``freq`` is the channel's own centre.  Per channel the PDUs, in order, are those of a ``wifi_phy_rx`` fed that channel's
    samples; between channels they come in the order the chains finish them.

    ``work()`` uploads its items behind the up to ``n_channels - 1`` items the call before left over, runs one
    wifirx_channelize on the block's own handle (the 23 * n_channels samples of history stay on the device, in two buffers
    used in turn), WAITS for that handle (the channels' handles read the rows on their own streams, which nothing else orders
    behind it: include/wifirx.h, wifirx_push, DEVICE INPUT) and pushes row k to channel k as device input.  All handles live
    on the one device, in this process."""

    def __init__(self, n_channels=4, stacking=1, center_frequency=5.21e9, bandwidth=20e6, sample_format="fc32",
                 sample_scale=None, device=0, **rx_kwargs):
        self.n_channels, self.stacking = int(n_channels), int(stacking)
        if self.n_channels not in capi.CHANNELIZER_CHANNELS:
            raise ValueError("n_channels must be 2, 4 or 8")
        if self.stacking not in (0, 1):
            raise ValueError("stacking must be 0 or 1")
        sf = _sample_format(sample_format, sample_scale)
        self.sample_format, self.sample_scale = sf.fmt, sf.scale
        self.bandwidth, self.center_frequency = float(bandwidth), float(center_frequency)
        M = self.n_channels
        self.frequencies = [self.center_frequency + capi.channel_centre(k, M, self.stacking) * M * self.bandwidth for k in range(M)]
        self._rem = np.zeros(0, dtype=np.uint8)                     # bytes of the fewer than M samples not yet channelised
        self._m0 = 0                                                # stream index of the next output
        self._cz = self._hist = self._d_in = self._d_out = None
        self._cap = 0                                               # outputs per channel the two buffers hold
        self._build("wifi_phy_rx_wideband", sf, lambda: self._open(device),
                    [dict(channel=k, frequency=f) for k, f in enumerate(self.frequencies)], device=device, **rx_kwargs)

    def _open(self, device):
        self._cz = capi.WifiRx(max_sym=1, device=device)           # the channelising handle: its receive side stays unused
        self._hist = _hist_pair(self._cz, capi.CHANNELIZER_HIST * self.n_channels * self._sf.bps)
        return self._cz

    def _reserve(self, n_out):
        if n_out <= self._cap:
            return
        for b in (self._d_in, self._d_out):
            if b is not None:
                b.free()
        M = self.n_channels
        self._cap = (n_out + n_out // 2 + 1) & ~1                   # even: every row starts on 16 bytes
        self._d_in = self._cz.alloc((self._cap + 1) * M * self._sf.bps)
        self._d_out = self._cz.alloc(self._cap * M * 8)

    def _front(self, raw, n):
        M, bps = self.n_channels, self._sf.bps
        n_rem = self._rem.size // bps
        n_out = (n_rem + n) // M
        if n_out == 0:
            self._rem = np.concatenate([self._rem, raw])
            return None, 0, 0
        self._reserve(n_out)
        cz, d_in = self._cz, self._d_in
        if n_rem:
            d_in.upload(self._rem)
        used = (n_out * M - n_rem) * bps                            # bytes of the items this call channelises
        cz._check(capi.lib().wifirx_memcpy_h2d(cz._h, d_in.ptr + n_rem * bps, raw.ctypes.data, used))
        cz.channelize_dev(d_in.ptr, self._sf.fmt, n_out, M, self.stacking, self._d_out.ptr, self._cap, hist_ptr=self._hist.cur,
                          hist_out_ptr=self._hist.nxt, m0=self._m0, scale=self._sf.scale)
        self._hist.advance()
        self._m0 += n_out
        self._rem = raw[used:].copy()                               # (the fewer than n_channels samples left over make no output)
        return self._d_out.ptr, self._cap, n_out

    def _close_front(self):
        for b in (getattr(self, "_hist", None), getattr(self, "_d_in", None), getattr(self, "_d_out", None)):
            if b is not None:
                b.free()
        self._hist, self._d_in, self._d_out, self._cap = None, None, None, 0
        if getattr(self, "_cz", None) is not None:
            self._cz.close()
            self._cz = None


class _arb_stream:
    """What ``arb_resampler``, ``wifi_phy_rx_resampled`` and ``wifi_phy_rx_tuned`` share: one handle, the stream indices j0 and
    m0 of wifirx_arb_resample (NUMERICS.md rule 34), the two history buffers used in turn, and the device buffers of a call.
    With ``incs`` the call is wifirx_tune (rule 35) and the output holds one row of ``cap_out`` samples per increment."""

    def __init__(self, rate_in, rate_out, sf, device, incs=None):
        self.incs = None if incs is None else [int(v) for v in incs]   # wifirx_tune's increments: one output row per channel
        self.sf = sf
        self.num, self.den = capi.arb_ratio(rate_in, rate_out)
        self.S = max(self.num, self.den)
        self.rx = capi.WifiRx(max_sym=1, device=device)            # the resampling handle: its receive side stays unused
        self.j0 = self.m0 = 0                                       # stream indices of the next input and the next output
        self.hist = _hist_pair(self.rx, capi.arb_hist(self.num, self.den) * sf.bps)
        self.d_in = self.d_out = None
        self.cap_in = self.cap_out = 0

    def room(self, n_out):
        """the most inputs with which the next call makes at most n_out outputs"""
        return max(0, ((self.m0 + n_out) * self.num + 16 * self.S) // self.den - self.j0)

    def flush_inputs(self):
        """the zeros behind the stream with which every input instant so far has come out: ceil(16 S / den)"""
        return -((-16 * self.S) // self.den)

    def run(self, raw, n):
        """n samples (raw: their bytes) -> (device pointer of the outputs, their number); asynchronous on the handle's stream"""
        n_out = capi.arb_count(self.num, self.den, self.j0, n, self.m0)
        if n > self.cap_in:
            if self.d_in is not None:
                self.d_in.free()
            self.cap_in = n + n // 2
            self.d_in = self.rx.alloc(self.cap_in * self.sf.bps)
        if n_out > self.cap_out:
            if self.d_out is not None:
                self.d_out.free()
            self.cap_out = (n_out + n_out // 2 + 1) & ~1            # even: every row starts on 16 bytes
            self.d_out = self.rx.alloc(self.cap_out * 8 * (1 if self.incs is None else len(self.incs)))
        rx = self.rx
        rx._check(capi.lib().wifirx_memcpy_h2d(rx._h, self.d_in.ptr, raw.ctypes.data, n * self.sf.bps))
        hist = dict(hist_ptr=self.hist.cur, hist_out_ptr=self.hist.nxt, j0=self.j0, m0=self.m0, scale=self.sf.scale)
        out = None if n_out == 0 else self.d_out.ptr
        if self.incs is None:
            got = rx.arb_resample_dev(self.d_in.ptr, self.sf.fmt, n, self.num, self.den, out, self.cap_out, **hist)
        else:
            got = rx.tune_dev(self.d_in.ptr, self.sf.fmt, n, self.num, self.den, self.incs, out, self.cap_out, **hist)
        self.hist.advance()
        self.j0, self.m0 = self.j0 + n, self.m0 + got
        return (self.d_out.ptr if got else None), got

    def close(self):
        for b in (self.hist, self.d_in, self.d_out):
            if b is not None:
                b.free()
        self.hist, self.d_in, self.d_out, self.cap_in, self.cap_out = None, None, None, 0, 0
        if self.rx is not None:
            self.rx.close()
            self.rx = None


class arb_resampler(grshim.basic_block):
    """GNU Radio's ``rational_resampler`` / ``pfb_arb_resampler_ccf`` on the device: one stream of ``sample_format`` items at
    ``rate_in`` Hz in, one ``complex64`` stream at ``rate_out`` Hz out, by wifirx_arb_resample (NUMERICS.md rule 34).  The
    rates' ratio in lowest terms must lie within ``capi.arb_ratio``'s limits (25, 30.72, 40, 50, 61.44, 80 MS/s to or from
    20 MS/s all do).

    ``general_work()`` (``work()`` on the shim) consumes as many input items as the output buffer has room for, writes the
    outputs they complete and returns their number; ``consumed`` holds the number of items the call took.  The stream
    indices and the history stay with the block (two device buffers used in turn), so the output does not depend on how
    the scheduler cuts the stream, and there is no delay: output m is the input at time m * rate_in / rate_out.  The last
    ceil(16 S / den) input instants come out only after that many more samples: ``stop()`` pushes them as zeros and
    leaves the outputs in ``tail``."""

    def __init__(self, rate_in, rate_out, sample_format="fc32", sample_scale=None, device=0):
        sf = _sample_format(sample_format, sample_scale)
        self._s = _arb_stream(rate_in, rate_out, sf, device)
        grshim.basic_block.__init__(self, name="arb_resampler", in_sig=sf.in_sig, out_sig=[np.complex64])
        self.num, self.den = self._s.num, self._s.den
        self.consumed = 0
        self.tail = np.zeros(0, np.complex64)

    def forecast(self, noutput_items, ninputs):
        return [self._s.room(noutput_items) or 1]

    def general_work(self, input_items, output_items):
        s, out = self._s, output_items[0]
        raw, n = s.sf.items(input_items[0])
        n = min(n, s.room(len(out)))
        self.consumed = n
        if hasattr(self, "consume"):                 # gr.basic_block's; the shim's caller reads `consumed`
            self.consume(0, n)
        if n == 0:
            return 0
        ptr, got = s.run(raw[:n * s.sf.bps], n)
        if got:
            y = np.empty(got, np.complex64)
            s.rx._check(capi.lib().wifirx_memcpy_d2h(s.rx._h, y.ctypes.data, ptr, 8 * got))     # ordered behind the kernel
            out[:got] = y
        return got

    work = general_work

    def stop(self):
        """End of stream: push the flush zeros; the outputs they complete are in ``tail``"""
        s = self._s
        if s.rx is None or s.j0 == 0:
            return True
        n = s.flush_inputs()
        ptr, got = s.run(s.sf.zeros(n), n)
        self.tail = np.zeros(0, np.complex64)
        if got:
            self.tail = np.empty(got, np.complex64)
            s.rx._check(capi.lib().wifirx_memcpy_d2h(s.rx._h, self.tail.ctypes.data, ptr, 8 * got))
        return True

    def close(self):
        """Release the device buffers and the handle."""
        self._s.close()


class _arb_fed_rx(_fed_rx):
    """``_fed_rx`` behind an ``_arb_stream``: the front stage of ``wifi_phy_rx_resampled`` and ``wifi_phy_rx_tuned``"""

    def _open(self, sample_rate, device, incs=None):
        self._s = _arb_stream(sample_rate, self.bandwidth, self._sf, device, incs=incs)
        self.num, self.den = self._s.num, self._s.den
        return self._s.rx

    def _front(self, raw, n):
        ptr, got = self._s.run(raw, n)
        return ptr, self._s.cap_out, got

    def _flush_zeros(self):
        return self._s.flush_inputs() if self._s.j0 else 0

    def _close_front(self):
        if getattr(self, "_s", None) is not None:
            self._s.close()


class wifi_phy_rx_resampled(_arb_fed_rx):
    """``wifi_phy_rx`` for a capture that does not run at the channel rate: ``samp_in`` at ``sample_rate`` Hz (25, 30.72, 40,
    50, 61.44, 80 MS/s ...; ``sample_format`` / ``sample_scale`` as ``wifi_phy_rx``), brought to ``bandwidth`` on the device
    by wifirx_arb_resample (NUMERICS.md rule 34) and received there by one ``wifi_phy_rx`` chain, which takes every other
    keyword.  ``mac_out`` and ``carrier`` carry what ``wifi_phy_rx`` publishes, unchanged: the PDUs of a ``wifi_phy_rx`` fed
    the resampled stream.

    ``work()`` uploads its items, runs one wifirx_arb_resample on the block's own handle (the history stays on the device,
    in two buffers used in turn), WAITS for that handle (the chain's handle reads the output on its own stream:
    include/wifirx.h, wifirx_push, DEVICE INPUT) and pushes the output to the chain as device input.  ``stop()`` pushes the
    ceil(16 S / den) zeros that bring out the stream's last instants, then settles the chain."""

    def __init__(self, sample_rate, bandwidth=20e6, sample_format="fc32", sample_scale=None, device=0, **rx_kwargs):
        self.sample_rate, self.bandwidth = float(sample_rate), float(bandwidth)
        self._build("wifi_phy_rx_resampled", _sample_format(sample_format, sample_scale), lambda: self._open(sample_rate, device),
                    [{}], device=device, **rx_kwargs)

    def stats(self):
        return self._rx[0].stats()


class wifi_phy_rx_tuned(_arb_fed_rx):
    """``wifi_phy_rx`` for K <= 8 channels that lie anywhere in one capture: ``samp_in`` at ``sample_rate`` Hz around
    ``center_frequency`` (``sample_format`` / ``sample_scale`` as ``wifi_phy_rx``), channel k centred ``offsets[k]`` Hz above
    it -- channels 1 / 6 / 11 of the 2.4 GHz band at -25, 0 and +25 MHz of an 80 MS/s capture around 2437 MHz, which no
    M x 20 MHz bank splits.  One wifirx_tune (NUMERICS.md rule 35) per ``work()`` mixes every channel down and brings it to
    ``bandwidth`` on the device (GNU Radio's ``freq_xlating_fir_filter`` per channel); each row is received there by a
    ``wifi_phy_rx`` chain of its own, which takes every other keyword.

    ``mac_out`` and ``carrier`` carry what ``wifi_phy_rx`` publishes, with ``channel`` (k) added to the dictionaries;
    ``freq`` is ``center_frequency + offsets[k]``.  Per channel the PDUs, in order, are those of a ``wifi_phy_rx`` fed that
    channel's samples; between channels they come in the order the chains finish them.

    The filter is rule 34's prototype: an offset must keep ``|offset| + bandwidth / 2`` inside ``sample_rate / 2`` (refused
    otherwise), and channels closer than 11.7 MHz (at 20 MHz) to a tuned centre are not rejected.  ``work()`` uploads its
    items, runs one wifirx_tune on the block's own handle (the history of raw samples stays on the device, in two buffers
    used in turn), WAITS for that handle (the chains' handles read the rows on their own streams: include/wifirx.h,
    wifirx_push, DEVICE INPUT) and pushes row k to chain k as device input.  ``stop()`` pushes the ceil(16 S / den) zeros
    that bring out the stream's last instants, then settles the chains."""

    def __init__(self, sample_rate, offsets=(-25e6, 0.0, 25e6), center_frequency=2.437e9, bandwidth=20e6, sample_format="fc32",
                 sample_scale=None, device=0, **rx_kwargs):
        self.sample_rate, self.bandwidth, self.center_frequency = float(sample_rate), float(bandwidth), float(center_frequency)
        self.offsets = [float(v) for v in offsets]
        if not 1 <= len(self.offsets) <= capi.TUNE_MAX_CHANNELS:
            raise ValueError("1 .. %d offsets are required" % capi.TUNE_MAX_CHANNELS)
        for off in self.offsets:
            if not abs(off) + self.bandwidth / 2 <= self.sample_rate / 2:
                raise ValueError("offset %g Hz: |offset| + bandwidth / 2 = %g Hz lies outside sample_rate / 2 = %g Hz, the channel "
                                 "would alias" % (off, abs(off) + self.bandwidth / 2, self.sample_rate / 2))
        self.frequencies = [self.center_frequency + off for off in self.offsets]
        self.incs = [capi.tune_inc(off, self.sample_rate) for off in self.offsets]
        self._build("wifi_phy_rx_tuned", _sample_format(sample_format, sample_scale),
                    lambda: self._open(self.sample_rate, device, incs=self.incs),
                    [dict(channel=k, frequency=f) for k, f in enumerate(self.frequencies)], device=device, **rx_kwargs)


class spectrum_probe(grshim.sync_block):
    """The numbers behind the reference's ``qtgui.sink_c(1024, window.WIN_BLACKMAN_hARRIS, fc, samp_rate, ...)`` spectrum and
    waterfall, on the device (wifirx_spectrum, NUMERICS.md rule 36): a sink with ``samp_in`` at ``sample_rate`` Hz around
    ``center_frequency`` (``sample_format`` / ``sample_scale`` as ``wifi_phy_rx``) that publishes one PDU per complete row on
    ``spectrum``: the row as an f32 vector of ``n_fft`` powers, bin i at ``center_frequency + (i - n_fft / 2) sample_rate /
    n_fft``, and the entries ``sample_rate``, ``center_frequency``, ``row_index``, ``n_fft``.  A row folds ``avg`` segments of
    ``n_fft`` samples, ``hop`` apart (None: ``n_fft``), by ``mode`` ("sum" / "max"), times ``norm`` (None: power per bin,
    ``spectrum.norm``).  With ``offsets`` (up to 16 candidate centres in Hz above ``center_frequency``, each ``width`` wide)
    a PDU also carries ``band_power_db``, one value per offset, from wifirx_spectrum_bands; ``band_rows`` collects the band
    powers of every row for ``spectrum.busy_channels``.

    ``work()`` keeps the samples that complete no row yet (the overlap of rule 36 stays with the caller), so the rows do not
    depend on how the scheduler cuts the stream: they are those of one call on the whole stream."""

    def __init__(self, sample_rate, n_fft=1024, window="blackman_harris", hop=None, avg=16, mode="sum", offsets=None, width=20e6,
                 center_frequency=0.0, sample_format="fc32", sample_scale=None, norm=None, device=0):
        from . import spectrum as _spectrum
        self.sample_rate, self.center_frequency, self.width = float(sample_rate), float(center_frequency), float(width)
        self.n_fft, self.avg = int(n_fft), int(avg)
        self.hop = self.n_fft if hop is None else int(hop)
        self.window, self.mode = window, mode
        capi.spectrum_count(self.n_fft, self.hop, self.avg, 0)       # refuses an n_fft, hop or avg outside the rule
        if window not in capi.SPEC_WINDOWS or mode not in capi.SPEC_MODES:
            raise ValueError("window must be one of %s, mode one of %s" % (sorted(capi.SPEC_WINDOWS), sorted(capi.SPEC_MODES)))
        self.norm = float(_spectrum.norm(self.n_fft, window, self.avg if mode == "sum" else 1) if norm is None else norm)
        self.offsets = None if offsets is None else [float(v) for v in offsets]
        self.bands = []
        if self.offsets is not None:
            if not 1 <= len(self.offsets) <= capi.SPEC_MAX_BANDS:
                raise ValueError("1 .. %d offsets are required" % capi.SPEC_MAX_BANDS)
            self.bands = [capi.spectrum_band(off, self.width, self.sample_rate, self.n_fft) for off in self.offsets]
        self._sf = _sample_format(sample_format, sample_scale)
        grshim.sync_block.__init__(self, name="spectrum_probe", in_sig=self._sf.in_sig, out_sig=None)
        self.message_port_register_out(grshim.intern("spectrum"))
        self._to_db = _spectrum.to_db
        self._rx = capi.WifiRx(max_sym=1, device=device)             # the survey's handle: its receive side stays unused
        self._pending = np.zeros(0, np.uint8)                        # samples that complete no row yet
        self._d_in = self._d_rows = self._d_bands = None
        self._cap_in = self._cap_rows = 0
        self.rows_made = 0
        self.band_rows = []

    def _room(self, n, rows):
        if n > self._cap_in:
            if self._d_in is not None:
                self._d_in.free()
            self._cap_in = n + n // 2
            self._d_in = self._rx.alloc(self._cap_in * self._sf.bps)
        if rows > self._cap_rows:
            for b in (self._d_rows, self._d_bands):
                if b is not None:
                    b.free()
            self._cap_rows = rows + rows // 2
            self._d_rows = self._rx.alloc(self._cap_rows * self.n_fft * 4)
            self._d_bands = self._rx.alloc(self._cap_rows * max(len(self.bands), 1) * 4)

    def work(self, input_items, output_items):
        raw, n = self._sf.items(input_items[0])
        if n == 0:
            return 0
        sf, rx = self._sf, self._rx
        data = np.concatenate([self._pending, raw]) if len(self._pending) else raw
        have = len(data) // sf.bps
        rows, consumed = capi.spectrum_count(self.n_fft, self.hop, self.avg, have)
        if rows:
            self._room(have, rows)
            data = np.ascontiguousarray(data)
            rx._check(capi.lib().wifirx_memcpy_h2d(rx._h, self._d_in.ptr, data.ctypes.data, have * sf.bps))
            got = rx.spectrum_dev(self._d_in.ptr, sf.fmt, have, self.n_fft, self.hop, self.avg, self._d_rows.ptr, self._cap_rows,
                                  self.window, self.mode, self.norm, scale=sf.scale)
            band = None
            if self.bands:
                rx.spectrum_bands_dev(self._d_rows.ptr, got, self.n_fft, self.bands, self._d_bands.ptr)
                band = self._d_bands.download(np.float32, got * len(self.bands)).reshape(got, len(self.bands))
            out = self._d_rows.download(np.float32, got * self.n_fft).reshape(got, self.n_fft)
            for r in range(got):
                meta = {"sample_rate": self.sample_rate, "center_frequency": self.center_frequency, "row_index": self.rows_made,
                        "n_fft": self.n_fft}
                if band is not None:
                    self.band_rows.append(band[r].copy())
                    meta["band_power_db"] = [float(v) for v in self._to_db(band[r])]
                self.message_port_pub(grshim.intern("spectrum"), grshim.make_pdu(meta, out[r].copy()))
                self.rows_made += 1
        self._pending = data[consumed * sf.bps:].copy()
        return n

    def busy_offsets(self, margin_db=10.0):
        """the offsets whose band was busy in the rows so far (``spectrum.busy_channels``)"""
        from . import spectrum as _spectrum
        if not self.band_rows:
            return []
        return [self.offsets[k] for k in _spectrum.busy_channels(np.stack(self.band_rows), margin_db)]

    def close(self):
        """Release the device buffers and the handle."""
        for b in (getattr(self, "_d_in", None), getattr(self, "_d_rows", None), getattr(self, "_d_bands", None)):
            if b is not None:
                b.free()
        self._d_in = self._d_rows = self._d_bands = None
        self._cap_in = self._cap_rows = 0
        if getattr(self, "_rx", None) is not None:
            self._rx.close()
            self._rx = None


class wifi_phy_tx(grshim.sync_block):
    """Drop-in for the TX half of ``wifi_phy_hier`` (mapper, SIGNAL, chunks->symbols, carrier allocator, IFFT, cyclic
    prefixer; gnu_radio/wifi_phy_hier.grc:279-479,570-586), optionally with ``foo.packet_pad2``'s zeros folded in
    (``pad_front=100, pad_tail=1000`` = gnu_radio/IRS_user.py:193).

    * ``mac_in``: the ``(meta, u8vector)`` PDU that ``ieee802_11.mac`` sends from ``phy out`` -- the PSDU, FCS included.
    * ``samp_out``: the frames back to back in arrival order, each ``pad_front`` zeros + frame + ``pad_tail`` zeros.

    The scrambler seed runs 1..127 from frame to frame across ``work()`` calls, as the mapper's does.  Every ``work()``
    builds all PDUs queued since the last one in one device call (wifirx_tx_batch, or wifirx_tx_batch_rates when
    ``set_encoding`` came between them: a PDU is built at the encoding in force when it arrived, as the mapper does -- the
    block notes at which position of its queue each setting took effect); what does not fit ``output_items[0]`` is handed
    out by the following calls.  The block emits base-band at the hier block's level: IRS_user's x0.5 gain stays in the
    flowgraph."""

    def __init__(self, encoding=0, pad_front=0, pad_tail=0, device=0):
        grshim.sync_block.__init__(self, name="wifi_phy_tx", in_sig=None, out_sig=[np.complex64])
        self._queue = []                                            # PSDUs (bytes) waiting for work()
        self._enc_from = []                                         # (position in the queue, encoding in force from there on)
        self.set_encoding(encoding)
        self.pad_front, self.pad_tail = int(pad_front), int(pad_tail)
        if self.pad_front < 0 or self.pad_tail < 0:
            raise ValueError("pad_front and pad_tail must be >= 0")
        self._rx = capi.WifiRx(max_sym=1, device=device)          # the handle's receive side stays unused
        self._carry = np.zeros(0, dtype=np.complex64)               # built samples not yet handed out
        self._n_frames = 0                                          # frames built so far: the next seed
        self.message_port_register_in(grshim.intern("mac_in"))
        self.set_msg_handler(grshim.intern("mac_in"), self._on_pdu)

    def get_encoding(self):
        return self.encoding

    def set_encoding(self, encoding):
        encoding = int(encoding)
        if not 0 <= encoding <= 7:
            raise ValueError("encoding must be 0..7")
        self.encoding = encoding
        if self._enc_from and self._enc_from[-1][0] == len(self._queue):
            self._enc_from.pop()                                    # no PDU arrived under the previous setting
        self._enc_from.append((len(self._queue), encoding))

    def _on_pdu(self, msg):
        vec = grshim.to_python(msg)[1]
        self._queue.append(np.asarray(vec, dtype=np.uint8).tobytes())

    def _build(self):
        psdus, self._queue = self._queue, []
        n = len(psdus)
        marks, self._enc_from = self._enc_from + [(n, None)], [(0, self.encoding)]
        encs = [e for (lo, e), (hi, _) in zip(marks[:-1], marks[1:]) for _ in range(hi - lo)]     # one per PDU
        seeds = (np.arange(self._n_frames, self._n_frames + n) % 127) + 1
        rows = [self.pad_front + txgen.frame_samples(len(p), e) + self.pad_tail for p, e in zip(psdus, encs)]
        row_off = np.zeros(n + 1, dtype=np.uint64)
        row_off[1:] = np.cumsum(rows)
        encoding = encs[0] if len(set(encs)) == 1 else np.array(encs, np.uint8)
        x = self._rx.tx_batch(psdus, encoding, seeds=seeds, lead=self.pad_front, row_off=row_off)
        self._n_frames += n
        self._carry = np.concatenate([self._carry, x]) if self._carry.size else x

    def work(self, input_items, output_items):
        if self._queue:
            self._build()
        out = output_items[0]
        n = min(len(out), self._carry.size)
        out[:n] = self._carry[:n]
        self._carry = self._carry[n:]
        return n

    def pending(self):
        """samples built and not yet handed out"""
        return int(self._carry.size)

    def close(self):
        """Release the library handle."""
        self._rx.close()


class mac(grshim.basic_block):
    """Drop-in for ``ieee802_11.mac(src_mac, dst_mac, bss_mac)`` (gnu_radio/IRS_user.py:192, IRS_tranceiver.py:271): the
    message block in front of the PHY.  ``app in`` takes a PDU ``(meta, u8vector)`` with the payload, ``phy out`` sends
    ``(meta, u8vector)`` with the PSDU -- 24-byte data header, payload, FCS -- which ``wifi_phy_tx``'s ``mac_in`` takes as it
    is (port names: IRS_user.py:204-205).  The sequence number counts up from 0, one per frame.

    The block frames on the host (txgen.mac_frame): one message is one frame, there is nothing to batch.  A sweep that
    frames many payloads at once calls wifirx_mac_batch (capi.WifiRx.mac_batch_dev) instead."""

    MAX_PAYLOAD = capi.MAX_PAYLOAD

    def __init__(self, src_mac=(0x23,) * 6, dst_mac=(0x42,) * 6, bss_mac=(0xFF,) * 6):
        grshim.basic_block.__init__(self, name="mac", in_sig=None, out_sig=None)
        self.src_mac, self.dst_mac, self.bss_mac = (self._addr(a) for a in (src_mac, dst_mac, bss_mac))
        self._seq = 0
        self._p_out = grshim.intern("phy out")
        self.message_port_register_out(self._p_out)
        self.message_port_register_in(grshim.intern("app in"))
        self.set_msg_handler(grshim.intern("app in"), self._on_app)

    @staticmethod
    def _addr(a):
        a = bytes(bytearray(a))
        if len(a) != 6:
            raise ValueError("a MAC address has 6 bytes")
        return a

    def _on_app(self, msg):
        meta, vec = grshim.to_python(msg)
        payload = np.asarray(vec, dtype=np.uint8).tobytes()
        if len(payload) > self.MAX_PAYLOAD:
            raise ValueError("payload longer than %d bytes" % self.MAX_PAYLOAD)
        psdu = txgen.mac_frame(payload, seq=self._seq, src=self.src_mac, dst=self.dst_mac, bss=self.bss_mac)
        self._seq = (self._seq + 1) & 0xFFF
        self.message_port_pub(self._p_out, grshim.make_pdu(dict(meta or {}), np.frombuffer(psdu, dtype=np.uint8)))


class channel_model(grshim.sync_block):
    """Drop-in for GNU Radio's ``channels.channel_model`` (the loop-back channel of gnu_radio/IRS_tranceiver.py:282-288) on the
    device: multipath FIR (``taps``), frequency offset (``frequency_offset`` in cycles/sample, as the flowgraph's
    ``epsilon*freq/10e6``) and complex Gaussian noise of variance ``noise_voltage**2``, in that order; ``samp_in`` ->
    ``samp_out``.  Arithmetic: NUMERICS.md rule 17 (wifirx_channel).

    Every ``work()`` is one wifirx_channel call on one row: the last ``len(taps) - 1`` input samples kept from before, then the
    new chunk.  The row's ``sample0`` is its stream index and its ``phase0`` the phase carried from the previous call (a uint64
    in 2^-64 turns), so the output does not depend on how the stream is cut into calls; the outputs of the kept samples are
    dropped.  A setter takes effect at the next ``work()``; a new frequency keeps the phase continuous.
    ``epsilon`` (the sample-rate offset) must be 1.0: the fractional resampler exists for rows (``WifiRx.channel(sro=...)``,
    wifirx_channel_sro), not for this stream block, whose output rate would differ from its input rate.

    ``doppler`` (cycles per sample, 0 .. 2^-10; None = static taps, the default) turns on the Doppler fader of NUMERICS.md
    rule 19 (wifirx_channel_fading): every tap is multiplied by a time-varying gain of mean power 1, Rician on tap 0 with
    ``k_factor`` > 0, drawn from ``fade_seed``; at most 16 taps then.  The gains are functions of the stream index (the call's
    ``time0``), carried across ``work()`` calls like the phase, so the output does not depend on the cut here either.
    ``doppler=0`` is not "off": it is one static random gain per tap.

    ``irs`` (an ``irs.IrsConfig``; None = the block as it is without it) takes the taps from a reflecting surface instead
    (wifirx_irs_taps, NUMERICS.md rule 25): output sample n of the stream runs through tap set ``n // irs.refresh`` of the
    configuration's draws, made on the device and handed to wifirx_channel there.  ``taps`` must then stay at its default and
    ``doppler`` at None; ``set_psi`` loads another phase configuration, which holds from the next ``work()`` on.  With
    ``IrsConfig(codebook=...)`` every tap set is the winner of a beam-training sweep over the codebook (wifirx_irs_sweep,
    NUMERICS.md rule 26), and ``irs_best`` holds the winning entries of the sets drawn so far.  With ``IrsConfig(pilots=...)``
    every tap set is trained from a noisy pilot-based estimate of its own (wifirx_irs_estimate, NUMERICS.md rule 29), and
    ``irs_codes`` holds the decided codes of the sets drawn so far.  ``IrsConfig(pilots=..., decision="joint")`` decides them over
    every antenna and tap (wifirx_irs_estimate -> wifirx_irs_optimize -> wifirx_irs_taps_multi on one stream, NUMERICS.md rule 30);
    with ``tap_weights`` or ``ant_weights`` the middle call is wifirx_irs_optimize_weighted (NUMERICS.md rule 31).

    ``IrsConfig(antennas=M)``, M = 2..8, puts an AP of M antennas behind the surface (wifirx_irs_taps_multi /
    wifirx_irs_sweep_multi, NUMERICS.md rules 27 and 28): the block then has M output ports, port m the input through plane m of
    the tap set in force.  The ports are the sample-synchronous antennas of one radio (rule 24): they share
    ``frequency_offset`` and ``epsilon``, and port m draws its noise from ``noise_seed + m``.  ``irs_best`` and ``set_psi`` work
    as with one antenna; a codebook is trained on the sum of the antennas' channel powers."""

    MAX_TAPS = 64

    def __init__(self, noise_voltage=1.0, frequency_offset=0.0, epsilon=1.0, taps=(1.0,), noise_seed=0, block_tags=False,
                 device=0, doppler=None, k_factor=0.0, fade_seed=0, irs=None, dc_offset=0j, iq_gain_db=0.0, iq_phase_deg=0.0):
        if irs is not None and not isinstance(irs, irs_mod.IrsConfig):
            raise TypeError("irs must be an irs.IrsConfig")
        self._ports = 1 if irs is None else irs.antennas         # output ports: the AP antennas behind the surface
        grshim.sync_block.__init__(self, name="channel_model", in_sig=[np.complex64], out_sig=[np.complex64] * self._ports)
        self._doppler = None
        self._irs = None
        if irs is not None:
            if doppler is not None or np.asarray(taps).size != 1 or complex(np.asarray(taps).reshape(-1)[0]) != 1.0:
                raise ValueError("with irs the taps are the surface's: leave taps and doppler at their defaults")
        self._irs_sets = None                                    # device buffer of the surface's tap sets 0 .. _irs_n - 1
        self._irs_n = 0
        self._irs_best = None                                    # device buffer of the winning entries (codebook mode)
        self._irs_codes = None                                   # device buffer of the decided codes (pilot mode)
        self.set_k_factor(k_factor)
        self.fade_seed = int(fade_seed) & 0xFFFFFFFFFFFFFFFF
        self.set_timing_offset(epsilon)
        self.set_noise_voltage(noise_voltage)
        self.set_frequency_offset(frequency_offset)
        self.set_taps(taps)
        self.set_doppler(doppler)
        self.set_rx_impairments(dc_offset, iq_gain_db, iq_phase_deg)
        self.noise_seed = int(noise_seed) & 0xFFFFFFFFFFFFFFFF
        self.block_tags = bool(block_tags)          # tags are not propagated by the shim; accepted for the signature
        self._rx = capi.WifiRx(max_sym=1, device=device)         # the handle's receive side stays unused
        self._hist = np.zeros(0, dtype=np.complex64)             # the last (up to MAX_TAPS - 1) input samples
        self._pos = 0                                            # stream index of the next input sample
        self._phase = 0                                          # phase of the next input sample, 2^-64 turns
        self._irs = irs

    # ---- the reflecting surface ----
    def set_psi(self, psi):
        """another phase configuration of the surface ([N] complex), from the next work() on"""
        if self._irs is None or self._irs.align_bits or self._irs.codebook is not None or self._irs.pilots is not None:
            raise ValueError("set_psi needs irs with given phases (align_bits = 0, no codebook, no pilots)")
        self._irs.set_psi(psi)
        self._irs_n = 0                                          # the sets are made again when they are next needed

    def _irs_set(self, s, m=0):
        """device pointer of the surface's tap set s for antenna m: the sets 0 .. s are made in one wifirx_irs_taps call (set r
        depends on r alone), twice as many each time the stream outgrows them.  With M > 1 antennas the one call is
        wifirx_irs_taps_multi / wifirx_irs_sweep_multi and the buffer holds its M planes of _irs_n sets."""
        c = self._irs
        multi = c.antennas > 1
        if s >= self._irs_n:
            n = max(16, 2 * (s + 1))
            if self._irs_sets is not None:
                self._irs_sets.free()
            self._irs_sets = self._rx.alloc(c.antennas * n * c.pdp.size * 8)
            if c.pilots is not None:                             # one call for one antenna and for several (rule 29)
                if self._irs_codes is not None:
                    self._irs_codes.free()
                self._irs_codes = self._rx.alloc(n * c.pilots.shape[1])
                scene = dict(gain=c.gain, k_factor=c.k_factor, direct_gain=c.direct_gain, seed=c.seed)
                est = dict(pilots=c.pilots, group=c.group, sigma=c.pilot_sigma, est_scale=c.est_scale, **scene)
                if c.decision == "joint":
                    # estimate -> joint decision -> taps of the true elements, on one stream (NUMERICS.md rule 30); the two
                    # scratch buffers are freed behind the handle's sync
                    R, J = c.antennas * c.pdp.size, c.pilots.shape[1] + 1
                    coef, psi = self._rx.alloc(n * R * J * 8), self._rx.alloc(n * c.n_elems * 8)
                    try:
                        self._rx.irs_estimate_dev(None, n, c.pdp, c.los_b2r, c.los_r2u, c.los_b2u, est_ptr=coef, **est)
                        self._rx.irs_optimize_dev(coef, n, R, J, bits=c.pilot_bits, max_sweeps=c.sweeps, start="ref",
                                                  direct_blocked=c.direct_gain == 0.0, n_elems=c.n_elems, group=c.group,
                                                  codes_ptr=self._irs_codes, psi_ptr=psi, weights=c.row_weights)
                        self._rx.irs_taps_multi_dev(self._irs_sets, n, c.pdp, c.los_b2r, c.los_r2u, c.los_b2u, psi=psi,
                                                    n_psi_sets=n, **scene)
                        self._rx.sync()
                    finally:
                        coef.free()
                        psi.free()
                else:
                    self._rx.irs_estimate_dev(self._irs_sets, n, c.pdp, c.los_b2r, c.los_r2u, c.los_b2u, align_bits=c.pilot_bits,
                                              codes_ptr=self._irs_codes, **est)
            elif c.codebook is not None:
                if self._irs_best is not None:
                    self._irs_best.free()
                self._irs_best = self._rx.alloc(n * 2)
                sweep = self._rx.irs_sweep_multi_dev if multi else self._rx.irs_sweep_dev
                sweep(self._irs_sets, n, c.pdp, c.los_b2r, c.los_r2u, c.los_b2u, codebook=c.codebook, gain=c.gain,
                      k_factor=c.k_factor, direct_gain=c.direct_gain, seed=c.seed, best_ptr=self._irs_best)
            else:
                taps = self._rx.irs_taps_multi_dev if multi else self._rx.irs_taps_dev
                taps(self._irs_sets, n, c.pdp, c.los_b2r, c.los_r2u, c.los_b2u, gain=c.gain, k_factor=c.k_factor,
                     direct_gain=c.direct_gain, psi=c.psi if c.align_bits == 0 else None, align_bits=c.align_bits, seed=c.seed)
            self._irs_n = n
        return self._irs_sets.ptr + 8 * c.pdp.size * (m * self._irs_n + s)

    @property
    def irs_best(self):
        """codebook mode: the winning entries of the tap sets drawn so far (uint16; set s is entry s)"""
        if self._irs is None or self._irs.codebook is None:
            raise ValueError("irs_best needs irs with a codebook")
        if self._irs_n == 0:
            return np.zeros(0, np.uint16)
        return self._irs_best.download(np.uint16, self._irs_n)

    @property
    def irs_codes(self):
        """pilot mode: the codes decided for the tap sets drawn so far (uint8 [sets, G]; row s is set s)"""
        if self._irs is None or self._irs.pilots is None:
            raise ValueError("irs_codes needs irs with pilots")
        G = self._irs.pilots.shape[1]
        if self._irs_n == 0:
            return np.zeros((0, G), np.uint8)
        return self._irs_codes.download(np.uint8, self._irs_n * G).reshape(self._irs_n, G)

    def _irs_work(self, x, outs, n):
        """work() with the surface's taps: the chunk is cut where the set index changes, every piece one wifirx_channel call
        per output port on device taps with the L - 1 samples before it in front"""
        c, L, rx = self._irs, self._irs.pdp.size, self._rx
        cfo = np.float32(2.0 * math.pi * self._frequency_offset)
        inc, m64 = capi.phase_inc(cfo), 0xFFFFFFFFFFFFFFFF
        at = 0
        while at < n:
            s = self._pos // c.refresh
            m = min(n - at, (s + 1) * c.refresh - self._pos)
            h = min(L - 1, self._hist.size)
            row = np.ascontiguousarray(np.concatenate([self._hist[self._hist.size - h:], x[at:at + m]]) if h else x[at:at + m])
            d_in, d_out = rx.alloc(row.size * 8).upload(row), rx.alloc(row.size * 8)
            try:
                for port, out in enumerate(outs):
                    rx.channel_dev(d_in.ptr, d_out.ptr, row.size, 1, row_len=row.size, taps=self._irs_set(s, port), n_taps=L,
                                   n_tap_sets=1, cfo=cfo, phase0=(self._phase - inc * h) & m64, gain=1.0,
                                   noise_voltage=self._noise_voltage, seed=(self.noise_seed + port) & m64, sample0=self._pos - h)
                    if self._impair is not None:
                        rx.rx_impair_dev(d_out.ptr, d_out.ptr, row.size, *self._impair)
                    out[at:at + m] = d_out.download(np.complex64, row.size)[h:]
            finally:
                d_in.free()
                d_out.free()
            keep = self.MAX_TAPS - 1
            self._hist = np.concatenate([self._hist, x[at:at + m]])[-keep:]
            self._pos += m
            self._phase = (self._phase + inc * m) & m64
            at += m
        return n

    # ---- GNU Radio's setters and getters ----
    def set_noise_voltage(self, noise_voltage):
        v = float(noise_voltage)
        if not math.isfinite(v):
            raise ValueError("noise_voltage must be finite")
        self._noise_voltage = v

    def noise_voltage(self):
        return self._noise_voltage

    def set_frequency_offset(self, frequency_offset):
        f = float(frequency_offset)
        if not math.isfinite(f):
            raise ValueError("frequency_offset must be finite")
        self._frequency_offset = f

    def frequency_offset(self):
        return self._frequency_offset

    def set_rx_impairments(self, dc_offset=0j, iq_gain_db=0.0, iq_phase_deg=0.0):
        """the receiver's own defects, applied behind the noise (wifirx_rx_impair): y = mu x + nu conj(x) + dc_offset with
        g = 10^(iq_gain_db / 20), mu = (1 + g e^{-j phi}) / 2, nu = (1 - g e^{j phi}) / 2.  All zero (the default): the
        block is what it is without them, and no kernel runs."""
        d, g, ph = complex(dc_offset), float(iq_gain_db), float(iq_phase_deg)
        if not (math.isfinite(d.real) and math.isfinite(d.imag) and math.isfinite(g) and math.isfinite(ph)):
            raise ValueError("dc_offset, iq_gain_db and iq_phase_deg must be finite")
        self.dc_offset, self.iq_gain_db, self.iq_phase_deg = d, g, ph
        self._impair = None if (d == 0 and g == 0.0 and ph == 0.0) else capi.iq_imbalance(g, ph) + (d,)

    def set_taps(self, taps):
        t = np.ascontiguousarray(np.asarray(taps, dtype=np.complex64).reshape(-1))
        if not 1 <= t.size <= self.MAX_TAPS:
            raise ValueError("taps must hold 1..%d values" % self.MAX_TAPS)
        if self._doppler is not None and t.size > capi.FADE_MAX_TAPS:
            raise ValueError("taps must hold 1..%d values with fading" % capi.FADE_MAX_TAPS)
        self._taps = t

    def taps(self):
        return self._taps.copy()

    def set_doppler(self, doppler):
        """maximum Doppler shift in cycles per sample, or None for static taps"""
        if doppler is not None:
            d = float(np.float32(doppler))
            if not 0.0 <= d <= capi.DOPPLER_MAX:
                raise ValueError("doppler must be 0 .. 2^-10 cycles per sample")
            if self._taps.size > capi.FADE_MAX_TAPS:
                raise ValueError("fading takes at most %d taps" % capi.FADE_MAX_TAPS)
            doppler = d
        self._doppler = doppler

    def doppler(self):
        return self._doppler

    def set_k_factor(self, k_factor):
        k = float(k_factor)
        if not (math.isfinite(k) and k >= 0.0):
            raise ValueError("k_factor must be finite and not negative")
        self._k_factor = k

    def k_factor(self):
        return self._k_factor

    def set_timing_offset(self, epsilon):
        if float(epsilon) != 1.0:
            raise ValueError("sample-rate offset is not supported")
        self._epsilon = 1.0

    def timing_offset(self):
        return self._epsilon

    # ---- stream interface ----
    def work(self, input_items, output_items):
        x = input_items[0]
        out = output_items[0]
        n = min([len(x)] + [len(o) for o in output_items[:self._ports]])
        if n == 0:
            return 0
        x = np.asarray(x[:n], dtype=np.complex64)
        if self._irs is not None:
            return self._irs_work(x, output_items[:self._ports], n)
        L = self._taps.size
        h = min(L - 1, self._hist.size)
        row = np.concatenate([self._hist[self._hist.size - h:], x]) if h else x
        cfo = np.float32(2.0 * math.pi * self._frequency_offset)
        inc = capi.phase_inc(cfo)
        m64 = 0xFFFFFFFFFFFFFFFF
        fade = {}                                                # without Doppler the call is the one it was
        if self._doppler is not None:
            fade = dict(doppler=self._doppler, k_factor=self._k_factor, fade_seed=self.fade_seed, time0=self._pos - h)
        y = self._rx.channel(row, taps=self._taps, cfo=cfo, phase0=(self._phase - inc * h) & m64, gain=1.0,
                             noise_voltage=self._noise_voltage, seed=self.noise_seed, sample0=self._pos - h, **fade)
        out[:n] = y[h:] if self._impair is None else self._rx.rx_impair(y[h:], *self._impair)
        keep = self.MAX_TAPS - 1
        self._hist = np.concatenate([self._hist, x])[-keep:] if n < keep else x[n - keep:].copy()
        self._pos += n
        self._phase = (self._phase + inc * n) & m64
        return n

    def close(self):
        """Release the library handle."""
        if self._irs_sets is not None:
            self._irs_sets.free()
            self._irs_sets = None
        if self._irs_best is not None:
            self._irs_best.free()
            self._irs_best = None
        if self._irs_codes is not None:
            self._irs_codes.free()
            self._irs_codes = None
        self._rx.close()


class wideband_combiner(grshim.sync_interpolator):
    """The transmit counterpart of ``wifi_phy_rx_wideband`` (GNU Radio's ``pfb_synthesizer_ccf``): ``n_channels`` = 2, 4 or
    8 ``complex64`` inputs at ``bandwidth``, one per adjacent channel, joined on the device by wifirx_combine (NUMERICS.md
    rule 22) into one ``complex64`` output at ``n_channels`` times the rate; input k lands at the centre that
    ``wifi_phy_rx_wideband`` gives channel k for the same ``stacking``.  ``gains``: one real factor per input, or None.

    ``work()`` consumes n = min(len of every input, len(output_items[0]) // n_channels) items of each input, writes
    n * n_channels items and returns that number.  The 23 samples of history per channel stay on the device, in two buffers
    used in turn, and so does the stream index: the output does not depend on how the scheduler cuts the stream."""

    def __init__(self, n_channels=4, stacking=1, gains=None, device=0):
        self.n_channels, self.stacking = int(n_channels), int(stacking)
        if self.n_channels not in capi.CHANNELIZER_CHANNELS:
            raise ValueError("n_channels must be 2, 4 or 8")
        if self.stacking not in (0, 1):
            raise ValueError("stacking must be 0 or 1")
        M = self.n_channels
        grshim.sync_interpolator.__init__(self, "wideband_combiner", [np.complex64] * M, [np.complex64], M)
        self.gains = None
        self.set_gains(gains)
        self._rx = capi.WifiRx(max_sym=1, device=device)           # the handle's receive side stays unused
        self._m0 = 0                                                # stream index of the next input sample
        self._hist = _hist_pair(self._rx, capi.CHANNELIZER_HIST * M * 8)
        self._d_in = self._d_out = None
        self._cap = 0                                               # samples per channel the two buffers hold

    def set_gains(self, gains):
        """one finite real factor per input from the next ``work()`` on; None: no multiply"""
        if gains is not None:
            gains = np.array(gains, dtype=np.float32).reshape(-1)
            if gains.size != self.n_channels or not np.isfinite(gains).all():
                raise ValueError("gains: one finite value per channel")
        self.gains = gains

    def _reserve(self, n):
        if n <= self._cap:
            return
        for b in (self._d_in, self._d_out):
            if b is not None:
                b.free()
        self._cap = (n + n // 2 + 1) & ~1                           # even: every row starts on 16 bytes
        self._d_in = self._rx.alloc(self._cap * self.n_channels * 8)
        self._d_out = self._rx.alloc(self._cap * self.n_channels * 8)

    def work(self, input_items, output_items):
        M, out = self.n_channels, output_items[0]
        n = min(min(len(x) for x in input_items[:M]), len(out) // M)
        if n <= 0:
            return 0
        self._reserve(n)
        rx = self._rx
        for k in range(M):
            x = np.ascontiguousarray(input_items[k][:n], dtype=np.complex64)
            rx._check(capi.lib().wifirx_memcpy_h2d(rx._h, self._d_in.ptr + 8 * k * self._cap, x.ctypes.data, 8 * n))
        rx.combine_dev(self._d_in.ptr, self._cap, n, M, self.stacking, self._d_out.ptr, gains=self.gains,
                       hist_ptr=self._hist.cur, hist_out_ptr=self._hist.nxt, m0=self._m0)
        out[:n * M] = self._d_out.download(np.complex64, n * M)    # ordered behind the kernel on the handle's stream
        self._hist.advance()
        self._m0 += n
        return n * M

    def close(self):
        """Release the device buffers and the handle."""
        for b in (getattr(self, "_hist", None), getattr(self, "_d_in", None), getattr(self, "_d_out", None)):
            if b is not None:
                b.free()
        self._hist, self._d_in, self._d_out, self._cap = None, None, None, 0
        if getattr(self, "_rx", None) is not None:
            self._rx.close()
            self._rx = None
