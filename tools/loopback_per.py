"""The reference's loop-back (gnu_radio/IRS_tranceiver.py: mac -> TX -> x gain -> channel_model -> RX -> decode_mac) on the device at
config 3's geometry, without a per-frame array crossing PCIe: wifirx_mac_batch (Philox payloads made on the device, 294-byte
PSDUs) -> wifirx_tx_batch (fixed rows of 1472 samples, lead 160) -> wifirx_channel (the 8-tap sets of tests/golden/sv_taps.npy
cycling, CFO uniform in +-20 ppm of 5.89 GHz at 20 MHz, gain sqrt(10^(snr/10)), noise_voltage 1) -> demod (LS) -> decode_mac,
hard and soft -> wifirx_link_stats against the PSDUs sent and the decisions on the clean TX rows.  Per SNR point: FER of both
decoders and the coded BER of the hard decisions, the quantities of tests/golden/config3_ber_table.json (host channel, CPU
oracle), and the raw counters.  --host-stats also downloads the buffers, keeps the books in NumPy and asserts that both agree.
Prints one JSON line, writes it to --out when given.

    python tools/loopback_per.py [--frames 1000000] [--snr 5 10 15 20 25 30] [--host-stats] [--out profiles/loopback_per_config3_device_stats.json]

--rates answers the rate question in one pass per SNR point: the same loop-back over a batch with the eight encodings cycling
(frame i at encoding i % 8; wifirx_tx_batch_rates), in row_off rows of lead 160 + frame + 32 rounded up to even (wifirx_channel
and wifirx_demod_batch_v take them), scored by wifirx_link_stats_by_rate.  Per point and rate: the counters, FER hard and soft,
coded BER, and the goodput = delivered payload bits per sample of air time.  max_sym is 99 for this mix and the soft decoder
needs 6 LLRs per carrier, so the LLR rows are bf16 (WIFIRX_LLR_BF16, 57 kB per frame); the default is 131 072 frames.

    python tools/loopback_per.py --rates [--frames 131072] [--host-stats] [--out profiles/loopback_rates.json]

--locked-clock (both modes) locks the channel's sample clock to its carrier, as a real radio's is and as the receiver's
frame_equalizer assumes: wifirx_channel_sro with sro = -cfo bw / (2 pi fc) per row (NUMERICS.md rule 18) in place of
wifirx_channel.  Everything else, the seeds included, stays, so a sweep with the switch stands beside one without.

    python tools/loopback_per.py --locked-clock [--out profiles/loopback_per_config3_locked.json]

--doppler asks which equaliser follows a channel that changes within the frame: the loop-back through wifirx_channel_fading
(NUMERICS.md rule 19) at every Doppler given (cycles per sample; 1e-4 = 1 kHz at 10 MS/s), Rician on tap 0 with --k-factor, and
per channel realisation the demodulator with each equaliser of --eq (all four by default) and the hard decode_mac.  The frames
are --psdu-len bytes at --encoding (default 1528 bytes of 64-QAM 2/3: 64 symbols) in fixed rows of lead 160 + frame + 79, the
channel is flat (--multipath: the 8-tap sets of sv_taps.npy cycling, every tap fading) and has no carrier offset.  Per SNR,
Doppler and equaliser: the FER and the counters of wifirx_link_stats.

    python tools/loopback_per.py --doppler 0 3e-5 1e-4 2e-4 --k-factor 10 --snr 25 30 [--frames 1000000] [--out profiles/loopback_fading.json]

--adc-bits asks what the converter in front of the receiver costs: config 3's loop-back with, between wifirx_channel and the
demod, wifirx_iq_from_f32 to B bits in --adc-format (default: sc8 up to 8 bits, sc16 above) and wifirx_iq_to_f32 back (NUMERICS.md
rule 20), on the device.  Full scale, 2^(B-1), is set --backoff-db above the RMS of a component of the channel output (measured on
its first 256 rows, which are downloaded for it).  Per SNR point: the float32 loop-back without a converter, then per B the FER
hard and soft and the share of clipped components, every B on the same channel output.

    python tools/loopback_per.py --adc-bits 8 6 4 12 16 --backoff-db 12 --snr 20 25 30 [--frames 262144] [--out profiles/loopback_adc.json]

--wideband M asks what a channel loses when its neighbours are loud: M = 2, 4 or 8 adjacent channels, the victim (--victim K)
carrying config 3's frames in their rows (flat channel, or --multipath; CFO uniform in +-20 ppm) and every other channel frames
of the same kind back to back, A dB above the victim for every A of --neighbour-db (and, first, silent).  Per point: the M rows
-> wifirx_combine with the gains (NUMERICS.md rule 22) -> wideband AWGN (wifirx_channel, one tap, in place, noise_voltage
sqrt(M): unit variance per channel bandwidth) -> with --adc-bits B, wifirx_iq_from_f32 to B bits at --backoff-db over the wide
stream's RMS -> wifirx_channelize (rule 21; the victim comes back 23 samples later in its rows) -> demod with each equaliser of
--eq (default ls) and both decoders -> wifirx_link_stats on the victim.  Beside it, per SNR, the same victim rows through the
single-channel path without either bank.

    python tools/loopback_per.py --wideband 4 --victim 1 --neighbour-db 0 10 20 25 30 35 40 50 --snr 25 30 [--frames 262144] [--out profiles/loopback_wideband.json]

--antennas asks what receive diversity buys in fading: the same TX rows (--psdu-len bytes at --encoding, fixed rows of lead 160 +
frame + 79) go through one wifirx_channel_fading call per antenna -- flat Rayleigh (Rician with --k-factor), Doppler the first
value of --doppler (default 0: one static gain per row and antenna), a fade_seed and a noise seed of its own per antenna, no
carrier offset --, then one demod per antenna, wifirx_diversity_combine (NUMERICS.md rule 23) in every mode of --diversity,
decode_mac hard and soft, and wifirx_link_stats.  Per SNR: the FER of every antenna count given (1 = antenna 0 alone, without
the combiner) and mode.  The counts nest: A antennas are the first A of the largest count, so the columns share their channels.

    python tools/loopback_per.py --antennas 1 2 4 --diversity mrc select --psdu-len 294 --encoding 2 --snr 5 10 15 20 25 [--frames 65536] [--out profiles/loopback_diversity.json]

--antennas with --precombine asks what combining in FRONT of the detector buys (wifirx_precombine, NUMERICS.md rule 33): the scene
of --antennas on rows of a multiple of 64 samples, every antenna's samples kept; per SNR and count A antenna 0 alone ('1'), A
demods and rule 23's MRC ('A_mrc'), and the pre-combined row set through ONE demod ('A_pre').  --multipath replaces the one tap
by the 8-tap sets of sv_taps.npy, every tap fading on its own: one weight per antenna cannot follow that channel, which is the
known limit of the rule.  Both runs land in one file, under "flat" and "multipath".

    python tools/loopback_per.py --antennas 2 4 --precombine [--precombine-iters 2] [--multipath] --psdu-len 100 --encoding 2 --snr 4 8 12 [--frames 65536] [--out profiles/loopback_precombine.json]

--irs: the link over a reflecting surface of N elements with B-bit phases (wifirx_irs_taps, NUMERICS.md rule 25): one tap set of 8
taps per frame, made on the device and read there by wifirx_channel; FER against the surface size at SNRs of one unit-power path.
--irs-mode: random phases, the one configuration aligned to the geometry, the genie aligned per draw, `estimate`: a surface
trained per draw from a noisy pilot-based channel estimate (wifirx_irs_estimate; --irs-pilots, --pilot-snr-db, --irs-group; with
--irs-decision joint the codes are decided over every antenna and tap by wifirx_irs_optimize, --pilot-snr-db inf is its genie bound;
--irs-tap-weights W0 [W1 ...] and --irs-ant-weights add arms decided by wifirx_irs_optimize_weighted, rule 31, reported as mode
estimate_joint_w with the rows' weights in the record; --irs-taps sets the tap count; every point carries the tap-0 power and the
median over the sets of the weakest subcarrier's power over the mean of the MRC-combined spectrum), or `sweep`: a surface
trained per draw by a codebook sweep (wifirx_irs_sweep, rule 26; --irs-codebook dft / dft2 / traverse, quantised to --irs-bits).
--irs 0 is the direct path alone.

    python tools/loopback_per.py --irs 0 16 64 256 --irs-bits 2 --irs-mode random los genie --k-factor 3 --direct-db -inf --psdu-len 294 --encoding 2 --snr -20 -10 0 [--frames 65536] [--out profiles/loopback_irs.json]
    python tools/loopback_per.py --irs 64 256 --irs-bits 2 --irs-mode random los genie sweep --irs-codebook dft2 --k-factor 3 --psdu-len 294 --encoding 2 --snr -30 -20 -10 [--out profiles/loopback_irs_sweep.json]
    python tools/loopback_per.py --irs 64 --irs-bits 2 --irs-mode random sweep estimate genie --k-factor 0.1 --pilot-snr-db -6 --psdu-len 294 --encoding 2 --snr -30 -25 -20 [--out profiles/loopback_irs_estimate.json]
    python tools/loopback_per.py --irs 64 --irs-bits 2 --irs-mode estimate --irs-decision ref joint --antennas 1 2 4 --k-factor 0.1 --pilot-snr-db -6 --psdu-len 294 --encoding 2 --snr -30 -25 -20 [--out profiles/loopback_irs_optimize.json]
    python tools/loopback_per.py --irs 64 --irs-bits 2 --irs-mode estimate --irs-decision ref joint --irs-tap-weights 1 0 --irs-tap-weights 1 -1 [--irs-taps 1] --antennas 1 2 4 --k-factor 0.1 --pilot-snr-db -6 --psdu-len 294 --encoding 2 --snr -30 -25 -20 --frames 16384 (the four runs of profiles/loopback_irs_optimize_w.json)

--dc-db puts a zero-IF receiver's defects between the channel and the receiver (wifirx_rx_impair: a DC offset of these many dB
above the noise power, and with --iq-imbalance GAIN_DB PHASE_DEG a gain / phase imbalance between I and Q) and runs the arms
of --frontend: "off" demodulates the impaired slots as they are, "dc" and "dc+iq" first take the slot buffer, as ONE stream
from a fresh state, through wifirx_frontend (NUMERICS.md rule 32: DC removal, blind IQ correction):
    python tools/loopback_per.py --dc-db none 0 5 10 20 30 --iq-imbalance 1 5 --frontend off dc dc+iq --snr 20 26 30 [--frames 65536] [--out profiles/loopback_frontend.json]"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gnuradio-wifi-imagetransfer_amd")]

from wifirx import capi, txgen  # noqa: E402

SLOT, LEAD, ENC, PSDU_LEN = 1472, 160, 7, 294
CFO_20PPM = 2 * np.pi * 20e-6 * 5.89e9 / 20e6
POPCOUNT6 = np.array([bin(v).count("1") for v in range(256)], np.uint8)
COUNTERS = [k for k, _ in capi.LinkCounts._fields_]


EQUALISERS = {"ls": capi.EQ_LS, "lms": capi.EQ_LMS, "comb": capi.EQ_COMB, "sta": capi.EQ_STA}


def host_stats(rx, dev, n, n_sym, nb, p, idx_tx):
    """the bookkeeping on the host: downloads the records, the PSDU rows and the decisions of the batch"""
    fr = dev["frames"].download(capi.FRAME_DTYPE, n)
    got = dev["psdu"].download(np.uint8, n * 304).reshape(n, 304)[:, :PSDU_LEN]
    crc = (fr["flags"] & capi.F_CRC_OK) != 0
    ok = crc & (got == p).all(axis=1)
    good = ((fr["flags"] & capi.F_COMPLETE) != 0) & (fr["encoding"] == ENC) & (fr["psdu_len"] == PSDU_LEN)
    idx = dev["idx"].download(np.uint8, n * n_sym * 48).reshape(n, -1)
    e = POPCOUNT6[idx[good] ^ idx_tx[good]].sum(axis=1, dtype=np.int64)
    per_frame = e / float(n_sym * 48 * nb)
    return dict(frames=n, frames_ref=n, frames_good=int(good.sum()), frames_crc_ok=int(crc.sum()), frames_psdu_ok=int(ok.sum()),
                frames_crc_ok_wrong=int((crc & ~ok).sum()), coded_bits=int(good.sum()) * n_sym * 48 * nb,
                coded_bit_errors=int(e.sum()), coded_bit_errors_sq=int((e * e).sum()),
                coded_ber=float(per_frame.mean()), coded_ber_se=float(per_frame.std() / np.sqrt(max(per_frame.size, 1))),
                fer=float(1.0 - ok.mean()))


def check_host(r, hs, what):
    assert {k: r[k] for k in COUNTERS} == {k: hs[k] for k in COUNTERS}, (what, r, hs)
    for k in ("fer", "coded_ber", "coded_ber_se"):
        assert abs(r[k] - hs[k]) <= 1e-12 * max(abs(hs[k]), 1e-300) + 1e-15, (what, k, r[k], hs[k])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=None, help="default 1 000 000; with --rates 131 072")
    ap.add_argument("--rates", action="store_true", help="the eight encodings cycling in one batch, statistics by rate")
    ap.add_argument("--snr", type=float, nargs="+", default=[5, 10, 15, 20, 25, 30])
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--host-stats", action="store_true", help="also keep the books in NumPy and assert they agree")
    ap.add_argument("--locked-clock", action="store_true", help="sample clock locked to the carrier: sro = -cfo bw / (2 pi fc)")
    ap.add_argument("--doppler", type=float, nargs="+", default=None, help="Doppler fading at these values, cycles per sample")
    ap.add_argument("--k-factor", type=float, default=0.0, help="with --doppler: Rician K of tap 0 (0 = Rayleigh)")
    ap.add_argument("--eq", nargs="+", choices=sorted(EQUALISERS, key=EQUALISERS.get), default=None,
                    help="with --doppler: the equalisers to compare (default all four)")
    ap.add_argument("--psdu-len", type=int, default=1528, help="with --doppler: PSDU bytes, 28 .. 1528")
    ap.add_argument("--encoding", type=int, default=6, help="with --doppler: 0 .. 7")
    ap.add_argument("--multipath", action="store_true", help="with --doppler: the sv_taps.npy sets in place of the flat channel")
    ap.add_argument("--adc-bits", type=int, nargs="+", default=None, help="a converter of these many bits in front of the receiver")
    ap.add_argument("--adc-format", choices=("auto", "sc16", "sc8"), default="auto", help="with --adc-bits: the container (auto: sc8 up to 8 bits)")
    ap.add_argument("--backoff-db", type=float, default=12.0, help="with --adc-bits: full scale above the RMS of the channel output")
    ap.add_argument("--wideband", type=int, default=None, choices=(2, 4, 8), help="M adjacent channels through both banks")
    ap.add_argument("--victim", type=int, default=1, help="with --wideband: the channel that is scored, 0 .. M - 1")
    ap.add_argument("--stacking", type=int, default=1, choices=(0, 1), help="with --wideband")
    ap.add_argument("--neighbour-db", type=float, nargs="+", default=[0, 20, 30, 40], help="with --wideband: the other channels' power above the victim's")
    ap.add_argument("--antennas", type=int, nargs="+", default=None, help="receive diversity: these antenna counts, 1 .. 8")
    ap.add_argument("--diversity", nargs="+", choices=sorted(capi.DIV_MODES, key=capi.DIV_MODES.get), default=None,
                    help="with --antennas: the combiner's modes (default both)")
    ap.add_argument("--precombine", action="store_true",
                    help="with --antennas: pre-detection combining (wifirx_precombine, NUMERICS.md rule 33) and ONE demod, beside "
                         "rule 23's MRC over the A demods and antenna 0 alone; --multipath: the sv_taps.npy sets in place of the flat channel")
    ap.add_argument("--precombine-iters", type=int, default=2, help="with --precombine: power iterations, 0 .. 4")
    ap.add_argument("--irs", type=int, nargs="+", default=None, help="a reflecting surface of these many elements (squares; 0 = the direct path alone)")
    ap.add_argument("--irs-bits", type=int, default=2, choices=(1, 2, 3), help="with --irs: the phase resolution")
    ap.add_argument("--irs-mode", nargs="+", choices=("random", "los", "genie", "sweep", "estimate"), default=["genie"],
                    help="with --irs: random phases, the one configuration aligned to the geometry, aligned per draw, trained "
                         "per draw by a codebook sweep (wifirx_irs_sweep), or trained per draw from a noisy pilot-based channel "
                         "estimate (wifirx_irs_estimate)")
    ap.add_argument("--irs-pilots", choices=("dft", "hadamard"), default="dft", help="with --irs-mode estimate: irs.dft_pilots or irs.hadamard_pilots")
    ap.add_argument("--pilot-snr-db", type=float, default=0.0,
                    help="with --irs-mode estimate: the SNR of one unit-power path in one pilot observation (sigma = 10^(-dB / 20))")
    ap.add_argument("--irs-group", type=int, default=1, help="with --irs-mode estimate: c x c elements behind one phase (irs.groups)")
    ap.add_argument("--irs-decision", nargs="+", choices=("ref", "joint"), default=["ref"],
                    help="with --irs-mode estimate: the codes decided on antenna 0, tap 0 (wifirx_irs_estimate's own decision) or "
                         "jointly over antennas and taps (wifirx_irs_optimize, NUMERICS.md rule 30; reported as mode estimate_joint)")
    ap.add_argument("--irs-sweeps", type=int, default=4, help="with --irs-decision joint: the most sweeps, 0 .. 16")
    ap.add_argument("--irs-tap-weights", type=float, nargs="+", action="append", default=None, metavar="W",
                    help="with --irs-decision joint: also decide with these weights over the taps, W0 [W1 ...], the last value "
                         "repeated up to the tap count (wifirx_irs_optimize_weighted, NUMERICS.md rule 31; reported as mode "
                         "estimate_joint_w); may be given several times, one arm each")
    ap.add_argument("--irs-ant-weights", type=float, nargs="+", default=None, metavar="W",
                    help="with --irs-decision joint: weights over the antennas for the estimate_joint_w arms, the last value "
                         "repeated up to the antenna count (alone: one arm with every tap weight 1)")
    ap.add_argument("--irs-taps", type=int, default=8, help="with --irs: the taps of the power delay profile exp(-l/2), 1 .. 16")
    ap.add_argument("--irs-codebook", choices=("dft", "dft2", "traverse"), default="dft2",
                    help="with --irs-mode sweep: irs.dft_codebook at over = 1 / 2, or the reference controller's 10 x 10 grid "
                         "(irs.traverse_codebook), quantised to --irs-bits")
    ap.add_argument("--direct-db", type=float, default=float("-inf"), help="with --irs: gain of the direct path in dB (-inf: blocked)")
    ap.add_argument("--dc-db", type=lambda s: float("-inf") if s == "none" else float(s), nargs="+", default=None,
                    help="a receiver's DC offset, these many dB above the noise power ('none': no offset)")
    ap.add_argument("--iq-imbalance", type=float, nargs=2, default=[0.0, 0.0], metavar=("GAIN_DB", "PHASE_DEG"),
                    help="with --dc-db: gain and phase imbalance between I and Q")
    ap.add_argument("--frontend", nargs="+", choices=("off", "dc", "dc+iq"), default=["off", "dc", "dc+iq"],
                    help="with --dc-db: the arms -- no front end, wifirx_frontend with the DC stage, with both stages")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if (a.irs_tap_weights or a.irs_ant_weights) and "joint" not in a.irs_decision:
        raise SystemExit("--irs-tap-weights and --irs-ant-weights need --irs-decision joint")
    if not 1 <= a.irs_taps <= capi.IRS_MAX_TAPS:
        raise SystemExit("--irs-taps 1 .. %d" % capi.IRS_MAX_TAPS)
    if a.irs is not None and a.antennas is not None and not a.precombine:
        return irs_multi_main(a)
    if a.irs is not None:
        return irs_main(a)
    if a.precombine:
        if a.antennas is None or a.irs is not None:
            raise SystemExit("--precombine goes with --antennas (and not with --irs)")
        return precombine_main(a)
    if a.antennas is not None:
        return diversity_main(a)
    if a.wideband is not None:
        return wideband_main(a)
    if a.adc_bits is not None:
        return adc_main(a)
    if a.dc_db is not None:
        return frontend_main(a)
    if a.doppler is not None:
        return fading_main(a)
    if a.rates:
        return rates_main(a)
    n = a.frames or 1_000_000
    n_sym = txgen.n_sym_for(PSDU_LEN, ENC)
    nb = txgen.RATE_TABLE[ENC][0]
    taps = np.load(os.path.join(ROOT, "tests", "golden", "sv_taps.npy")).astype(np.complex64)
    rx = capi.WifiRx(max_sym=n_sym, llr_bits=nb, chan_est=capi.EQ_LS, device=0)
    t_all = time.perf_counter()
    d_psdu = rx.alloc(n * PSDU_LEN)
    rows = rx.alloc(n * SLOT * 8)
    iq = rx.alloc(n * SLOT * 8)
    rx.mac_batch_dev(d_psdu.ptr, PSDU_LEN, n, None, payload_len=PSDU_LEN - 28, payload_seed=a.seed)
    rx.tx_batch_dev(rows.ptr, n * SLOT, d_psdu.ptr, ENC, psdu_len=np.full(n, PSDU_LEN, np.uint32), psdu_stride=PSDU_LEN,
                    lead=LEAD, row_len=SLOT)
    dev = rx.alloc_out(n, psdu_stride=304, want_hbits=True)
    # what was sent: the PSDUs, and the demodulator's records and decisions on the clean rows
    ref = dict(frames=rx.alloc(n * 32).upload(np.zeros(n * 32, np.uint8)), idx=rx.alloc(n * n_sym * 48), hbits=rx.alloc(n * n_sym * 48), psdu=d_psdu,
               psdu_stride=PSDU_LEN)
    rx.demod_batch_dev(rows.ptr, SLOT, n, ref)
    assert rx.link_stats(n, ref, ref)["frames_ref"] == n, "a clean frame was not demodulated"
    if a.host_stats:
        p = d_psdu.download(np.uint8, n * PSDU_LEN).reshape(n, PSDU_LEN)
        idx_tx = ref["idx"].download(np.uint8, n * n_sym * 48).reshape(n, -1)
    points = []
    for snr in a.snr:
        t0 = time.perf_counter()
        cfo = np.random.default_rng(int(1000 * snr) + a.seed).uniform(-CFO_20PPM, CFO_20PPM, n).astype(np.float32)
        rx.channel_dev(rows.ptr, iq.ptr, n * SLOT, n, row_len=SLOT, taps=taps, cfo=cfo, gain=math.sqrt(10 ** (snr / 10)),
                       noise_voltage=1.0, seed=9000 + int(snr) + (a.seed << 32),
                       sro=capi.locked_sro(cfo) if a.locked_clock else None)
        rx.demod_batch_dev(iq.ptr, SLOT, n, dev)
        rx.decode_batch_dev(n, dev)
        hard = rx.link_stats(n, dev, ref)
        if a.host_stats:
            check_host(hard, host_stats(rx, dev, n, n_sym, nb, p, idx_tx), "hard")
        rx.decode_batch_soft_dev(n, dev)
        soft = rx.link_stats(n, dev, ref)
        if a.host_stats:
            check_host(soft, host_stats(rx, dev, n, n_sym, nb, p, idx_tx), "soft")
        points.append({"snr_db": snr, "frames": n, "detected_and_signal_ok": hard["frames_good"] / n,
                       "coded_ber": hard["coded_ber"], "coded_ber_se": hard["coded_ber_se"],
                       "fer": hard["fer"], "fer_soft": soft["fer"], "crc_ok_wrong_psdu": hard["frames_crc_ok_wrong"],
                       "seconds": time.perf_counter() - t0,
                       "counts": {k: hard[k] for k in COUNTERS}, "counts_soft": {k: soft[k] for k in COUNTERS}})
        print(json.dumps(points[-1]), file=sys.stderr)
    seconds_total = time.perf_counter() - t_all
    rx.free_out(ref)
    rx.free_out(dev)
    rows.free(); iq.free(); rx.close()
    res = {"workload": "loop-back on the device, config 3: %d distinct frames per point (wifirx_mac_batch, Philox payloads), 64-QAM 3/4, PSDU 294 B, rows of 1472, "
                       "lead 160, sv_taps.npy sets cycling, CFO uniform in +-20 ppm, LS; hard and soft decode_mac" % n
                       + ("; sample clock locked to the carrier (wifirx_channel_sro, sro = -cfo bw / (2 pi fc))" if a.locked_clock else ""),
           "stats": "wifirx_link_stats on the device" + (", checked against the NumPy bookkeeping" if a.host_stats else ""),
           "seconds_total": seconds_total, "points": points}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


def adc_main(a):
    if a.rates or a.host_stats or a.locked_clock or a.doppler is not None:
        raise SystemExit("--adc-bits stands alone: not with --rates, --host-stats, --locked-clock or --doppler")
    n = a.frames or 262144
    fmt_of = lambda b: a.adc_format if a.adc_format != "auto" else ("sc8" if b <= 8 else "sc16")
    for b in a.adc_bits:
        if not 2 <= b <= capi.IQ_MAX_BITS[capi.IQ_FORMATS[fmt_of(b)]]:
            raise SystemExit("--adc-bits %d does not fit %s" % (b, fmt_of(b)))
    n_sym, nb = txgen.n_sym_for(PSDU_LEN, ENC), txgen.RATE_TABLE[ENC][0]
    taps = np.load(os.path.join(ROOT, "tests", "golden", "sv_taps.npy")).astype(np.complex64)
    rx = capi.WifiRx(max_sym=n_sym, llr_bits=nb, chan_est=capi.EQ_LS, device=0)
    t_all = time.perf_counter()
    d_psdu, rows, iq, iq_adc, d_int = rx.alloc(n * PSDU_LEN), rx.alloc(n * SLOT * 8), rx.alloc(n * SLOT * 8), rx.alloc(n * SLOT * 8), rx.alloc(n * SLOT * 4)
    rx.mac_batch_dev(d_psdu.ptr, PSDU_LEN, n, None, payload_len=PSDU_LEN - 28, payload_seed=a.seed)
    rx.tx_batch_dev(rows.ptr, n * SLOT, d_psdu.ptr, ENC, psdu_len=np.full(n, PSDU_LEN, np.uint32), psdu_stride=PSDU_LEN, lead=LEAD, row_len=SLOT)
    dev = rx.alloc_out(n, psdu_stride=304, want_hbits=True)
    ref = dict(frames=rx.alloc(n * 32).upload(np.zeros(n * 32, np.uint8)), idx=rx.alloc(n * n_sym * 48), hbits=rx.alloc(n * n_sym * 48), psdu=d_psdu,
               psdu_stride=PSDU_LEN)
    rx.demod_batch_dev(rows.ptr, SLOT, n, ref)
    assert rx.link_stats(n, ref, ref)["frames_ref"] == n, "a clean frame was not demodulated"

    def receive(ptr):
        rx.demod_batch_dev(ptr, SLOT, n, dev)
        rx.decode_batch_dev(n, dev)
        hard = rx.link_stats(n, dev, ref)
        rx.decode_batch_soft_dev(n, dev)
        soft = rx.link_stats(n, dev, ref)
        return {"fer": hard["fer"], "fer_soft": soft["fer"], "coded_ber": hard["coded_ber"], "counts": {k: hard[k] for k in COUNTERS},
                "counts_soft": {k: soft[k] for k in COUNTERS}}

    points = []
    for snr in a.snr:
        t0 = time.perf_counter()
        cfo = np.random.default_rng(int(1000 * snr) + a.seed).uniform(-CFO_20PPM, CFO_20PPM, n).astype(np.float32)
        rx.channel_dev(rows.ptr, iq.ptr, n * SLOT, n, row_len=SLOT, taps=taps, cfo=cfo, gain=math.sqrt(10 ** (snr / 10)),
                       noise_voltage=1.0, seed=9000 + int(snr) + (a.seed << 32))
        head = iq.download(np.complex64, min(n, 256) * SLOT)
        rms = math.sqrt(float(np.mean(np.abs(head.astype(np.complex128)) ** 2)) / 2.0)          # of a component
        pt = {"snr_db": snr, "frames": n, "rms_component": rms, "float32": receive(iq.ptr), "adc": []}
        for b in a.adc_bits:
            fmt = fmt_of(b)
            scale_q = float(np.float32(2.0 ** (b - 1) / (rms * 10.0 ** (a.backoff_db / 20.0))))
            clipped = rx.iq_from_f32_dev(iq.ptr, n * SLOT, fmt, d_int.ptr, scale_q, b, count=True)
            rx.iq_to_f32_dev(d_int.ptr, fmt, n * SLOT, iq_adc.ptr, float(np.float32(1.0 / scale_q)))
            r = receive(iq_adc.ptr)
            r.update(bits=b, format=fmt, scale=scale_q, clipped_share=clipped / (2.0 * n * SLOT))
            pt["adc"].append(r)
        pt["seconds"] = time.perf_counter() - t0
        points.append(pt)
        print(json.dumps({"snr_db": snr, "float32": [pt["float32"]["fer"], pt["float32"]["fer_soft"]],
                          "adc": [[r["bits"], r["format"], r["fer"], r["fer_soft"], r["clipped_share"]] for r in pt["adc"]]}), file=sys.stderr)
    seconds_total = time.perf_counter() - t_all
    rx.free_out(ref)
    rx.free_out(dev)
    for d in (rows, iq, iq_adc, d_int):
        d.free()
    rx.close()
    res = {"workload": "loop-back on the device, config 3 (%d distinct frames per point, 64-QAM 3/4, PSDU 294 B, rows of 1472, lead 160, "
                       "sv_taps.npy sets cycling, CFO uniform in +-20 ppm, LS; hard and soft decode_mac) with a converter between channel and "
                       "receiver: wifirx_iq_from_f32 to B bits, wifirx_iq_to_f32 back; full scale %.1f dB above the RMS of a component of the "
                       "channel output (its first 256 rows)" % (n, a.backoff_db),
           "columns": "per SNR: float32 = no converter; adc = one entry per B: fer (hard), fer_soft, clipped_share of the components",
           "backoff_db": a.backoff_db, "stats": "wifirx_link_stats on the device", "seconds_total": seconds_total, "points": points}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


def frontend_main(a):
    if a.rates or a.host_stats or a.locked_clock or a.doppler is not None:
        raise SystemExit("--dc-db stands alone: not with --rates, --host-stats, --locked-clock or --doppler")
    n = a.frames or 65536
    n_sym, nb = txgen.n_sym_for(PSDU_LEN, ENC), txgen.RATE_TABLE[ENC][0]
    taps = np.load(os.path.join(ROOT, "tests", "golden", "sv_taps.npy")).astype(np.complex64)
    rx = capi.WifiRx(max_sym=n_sym, llr_bits=nb, chan_est=capi.EQ_LS, device=0)
    t_all = time.perf_counter()
    d_psdu, rows, iq, iq_rx, iq_fe = rx.alloc(n * PSDU_LEN), rx.alloc(n * SLOT * 8), rx.alloc(n * SLOT * 8), rx.alloc(n * SLOT * 8), rx.alloc(n * SLOT * 8)
    d_state = rx.alloc(capi.FE_STATE_DTYPE.itemsize)
    rx.mac_batch_dev(d_psdu.ptr, PSDU_LEN, n, None, payload_len=PSDU_LEN - 28, payload_seed=a.seed)
    rx.tx_batch_dev(rows.ptr, n * SLOT, d_psdu.ptr, ENC, psdu_len=np.full(n, PSDU_LEN, np.uint32), psdu_stride=PSDU_LEN, lead=LEAD, row_len=SLOT)
    dev = rx.alloc_out(n, psdu_stride=304, want_hbits=True)
    ref = dict(frames=rx.alloc(n * 32).upload(np.zeros(n * 32, np.uint8)), idx=rx.alloc(n * n_sym * 48), hbits=rx.alloc(n * n_sym * 48), psdu=d_psdu,
               psdu_stride=PSDU_LEN)
    rx.demod_batch_dev(rows.ptr, SLOT, n, ref)
    assert rx.link_stats(n, ref, ref)["frames_ref"] == n, "a clean frame was not demodulated"
    mu, nu = capi.iq_imbalance(*a.iq_imbalance)
    cfgs = {"dc": capi.frontend_cfg(dc=True, iq=False), "dc+iq": capi.frontend_cfg(dc=True, iq=True)}

    def receive(ptr):
        rx.demod_batch_dev(ptr, SLOT, n, dev)
        rx.decode_batch_dev(n, dev)
        hard = rx.link_stats(n, dev, ref)
        rx.decode_batch_soft_dev(n, dev)
        soft = rx.link_stats(n, dev, ref)
        return {"fer": hard["fer"], "fer_soft": soft["fer"], "coded_ber": hard["coded_ber"], "counts": {k: hard[k] for k in COUNTERS},
                "counts_soft": {k: soft[k] for k in COUNTERS}}

    points = []
    for snr in a.snr:
        cfo = np.random.default_rng(int(1000 * snr) + a.seed).uniform(-CFO_20PPM, CFO_20PPM, n).astype(np.float32)
        rx.channel_dev(rows.ptr, iq.ptr, n * SLOT, n, row_len=SLOT, taps=taps, cfo=cfo, gain=math.sqrt(10 ** (snr / 10)),
                       noise_voltage=1.0, seed=9000 + int(snr) + (a.seed << 32))
        for dc_db in a.dc_db:
            t0 = time.perf_counter()
            dc = math.sqrt(10 ** (dc_db / 10)) * np.exp(0.7j) if math.isfinite(dc_db) else 0j
            rx.rx_impair_dev(iq.ptr, iq_rx.ptr, n * SLOT, mu, nu, dc)
            pt = {"snr_db": snr, "dc_db": dc_db if math.isfinite(dc_db) else None, "frames": n, "arms": {}}
            for arm in a.frontend:
                ptr = iq_rx.ptr
                if arm != "off":
                    d_state.upload(np.zeros(1, capi.FE_STATE_DTYPE))             # every arm starts a fresh stream
                    rx.frontend_dev(cfgs[arm], d_state.ptr, iq_rx.ptr, "fc32", n * SLOT, iq_fe.ptr)
                    ptr = iq_fe.ptr
                pt["arms"][arm] = receive(ptr)
                if arm != "off":
                    st = d_state.download(capi.FE_STATE_DTYPE, 1)[0]
                    d, w = capi.frontend_estimate(cfgs[arm], st)
                    pt["arms"][arm].update(dc_estimate=[float(d.real), float(d.imag)], w_estimate=[float(w.real), float(w.imag)])
            pt["seconds"] = time.perf_counter() - t0
            points.append(pt)
            print(json.dumps({"snr_db": snr, "dc_db": pt["dc_db"], "fer": {k: v["fer"] for k, v in pt["arms"].items()},
                              "fer_soft": {k: v["fer_soft"] for k, v in pt["arms"].items()}}), file=sys.stderr)
    seconds_total = time.perf_counter() - t_all
    rx.free_out(ref)
    rx.free_out(dev)
    for d in (rows, iq, iq_rx, iq_fe, d_state):
        d.free()
    rx.close()
    res = {"workload": "loop-back on the device, config 3 (%d distinct frames per point, 64-QAM 3/4, PSDU 294 B, rows of 1472, lead 160, "
                       "sv_taps.npy sets cycling, CFO uniform in +-20 ppm, LS; hard and soft decode_mac) with a zero-IF receiver's defects "
                       "behind the channel (wifirx_rx_impair: DC offset dc_db above the unit noise power at angle 0.7 rad, IQ imbalance "
                       "%.2f dB / %.2f deg) and the receive front end (wifirx_frontend, NUMERICS.md rule 32, defaults) over the slot buffer "
                       "as one stream from a fresh state" % (n, a.iq_imbalance[0], a.iq_imbalance[1]),
           "columns": "per SNR and dc_db: arms[off | dc | dc+iq] = fer (hard), fer_soft, counters; dc_estimate / w_estimate: what the "
                      "block behind the buffer would be corrected with (true image coefficient nu / conj(mu) = %s)" % str(nu / np.conj(mu)),
           "iq_imbalance": list(a.iq_imbalance), "stats": "wifirx_link_stats on the device", "seconds_total": seconds_total, "points": points}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


def wideband_main(a):
    if a.rates or a.host_stats or a.locked_clock or a.doppler is not None:
        raise SystemExit("--wideband stands alone: not with --rates, --host-stats, --locked-clock or --doppler")
    M, s, victim = a.wideband, a.stacking, a.victim
    if not 0 <= victim < M:
        raise SystemExit("--victim 0 .. M - 1")
    if a.adc_bits is not None and (len(a.adc_bits) != 1 or not 2 <= a.adc_bits[0] <= 16):
        raise SystemExit("--wideband takes one --adc-bits value, 2 .. 16")
    n = a.frames or 262144
    eqs = a.eq or ["ls"]
    n_sym, nb = txgen.n_sym_for(PSDU_LEN, ENC), txgen.RATE_TABLE[ENC][0]
    taps = np.load(os.path.join(ROOT, "tests", "golden", "sv_taps.npy")).astype(np.complex64) if a.multipath else (1.0,)
    row = n * SLOT                                            # samples per channel
    back = txgen.frame_samples(PSDU_LEN, ENC)
    back += back & 1                                          # the neighbours' frames back to back, in rows of even length
    n_nb = row // back
    rx = capi.WifiRx(max_sym=n_sym, llr_bits=nb, chan_est=capi.EQ_LS, device=0)
    t_all = time.perf_counter()
    d_psdu, d_psdu_nb = rx.alloc(n * PSDU_LEN), rx.alloc(n_nb * PSDU_LEN)
    rows, iq = rx.alloc(row * 8), rx.alloc(row * 8)
    chans, wide, split = rx.alloc(M * row * 8), rx.alloc(M * row * 8), rx.alloc(M * row * 8)
    d_int = rx.alloc(M * row * 4) if a.adc_bits else None
    rx.mac_batch_dev(d_psdu.ptr, PSDU_LEN, n, None, payload_len=PSDU_LEN - 28, payload_seed=a.seed)
    rx.tx_batch_dev(rows.ptr, row, d_psdu.ptr, ENC, psdu_len=np.full(n, PSDU_LEN, np.uint32), psdu_stride=PSDU_LEN, lead=LEAD, row_len=SLOT)
    dev = rx.alloc_out(n, psdu_stride=304, want_hbits=True)
    ref = dict(frames=rx.alloc(n * 32).upload(np.zeros(n * 32, np.uint8)), idx=rx.alloc(n * n_sym * 48), hbits=rx.alloc(n * n_sym * 48), psdu=d_psdu,
               psdu_stride=PSDU_LEN)
    rx.demod_batch_dev(rows.ptr, SLOT, n, ref)
    assert rx.link_stats(n, ref, ref)["frames_ref"] == n, "a clean frame was not demodulated"
    # the M channel rows, unit power: the victim's frames through their channel without noise, the others back to back
    cfo = np.random.default_rng(a.seed).uniform(-CFO_20PPM, CFO_20PPM, n).astype(np.float32)
    rx.channel_dev(rows.ptr, chans.ptr + 8 * victim * row, row, n, row_len=SLOT, taps=taps, cfo=cfo, gain=1.0, noise_voltage=0.0)
    nb_off = np.arange(n_nb + 1, dtype=np.uint64) * back
    nb_off[-1] = row                                          # the last row takes the rest: zeros
    for k in range(M):
        if k != victim:
            rx.mac_batch_dev(d_psdu_nb.ptr, PSDU_LEN, n_nb, None, payload_len=PSDU_LEN - 28, payload_seed=a.seed + 100 * (k + 1))
            rx.tx_batch_dev(chans.ptr + 8 * k * row, row, d_psdu_nb.ptr, ENC, psdu_len=np.full(n_nb, PSDU_LEN, np.uint32),
                            psdu_stride=PSDU_LEN, lead=0, row_off=nb_off)

    def receive(ptr):
        by_eq = {}
        for name in eqs:
            rx.set_param(capi.P_CHAN_EST, EQUALISERS[name])
            rx.demod_batch_dev(ptr, SLOT, n, dev)
            rx.decode_batch_dev(n, dev)
            hard = rx.link_stats(n, dev, ref)
            rx.decode_batch_soft_dev(n, dev)
            soft = rx.link_stats(n, dev, ref)
            by_eq[name] = {"fer": hard["fer"], "fer_soft": soft["fer"], "coded_ber": hard["coded_ber"],
                           "counts": {k: hard[k] for k in COUNTERS}, "counts_soft": {k: soft[k] for k in COUNTERS}}
        rx.set_param(capi.P_CHAN_EST, capi.EQ_LS)
        return by_eq

    points = []
    for snr in a.snr:
        g = math.sqrt(10 ** (snr / 10))
        seed = 9000 + int(snr) + (a.seed << 32)
        t0 = time.perf_counter()
        rx.channel_dev(chans.ptr + 8 * victim * row, iq.ptr, row, n, row_len=SLOT, taps=(1.0,), gain=g, noise_voltage=1.0, seed=seed)
        pt = {"snr_db": snr, "frames": n, "single_channel": receive(iq.ptr), "seconds_single_channel": time.perf_counter() - t0, "wideband": []}
        for above in [None] + list(a.neighbour_db):
            t0 = time.perf_counter()
            gains = np.full(M, 0.0 if above is None else g * 10 ** (above / 20), np.float32)
            gains[victim] = g
            rx.combine_dev(chans.ptr, row, row, M, s, wide.ptr, gains=gains)
            rx.channel_dev(wide.ptr, wide.ptr, M * row, n, row_len=M * SLOT, taps=(1.0,), gain=1.0, noise_voltage=math.sqrt(M), seed=seed + 1)
            r = {"neighbour_db": above}
            if a.adc_bits:
                b = a.adc_bits[0]
                fmt = a.adc_format if a.adc_format != "auto" else ("sc8" if b <= 8 else "sc16")
                head = wide.download(np.complex64, min(n, 256) * M * SLOT)
                rms = math.sqrt(float(np.mean(np.abs(head.astype(np.complex128)) ** 2)) / 2.0)      # of a component
                scale_q = float(np.float32(2.0 ** (b - 1) / (rms * 10.0 ** (a.backoff_db / 20.0))))
                clipped = rx.iq_from_f32_dev(wide.ptr, M * row, fmt, d_int.ptr, scale_q, b, count=True)
                rx.channelize_dev(d_int.ptr, fmt, row, M, s, split.ptr, row, scale=float(np.float32(1.0 / scale_q)))
                r.update(bits=b, format=fmt, scale=scale_q, clipped_share=clipped / (2.0 * M * row))
            else:
                rx.channelize_dev(wide.ptr, "fc32", row, M, s, split.ptr, row)
            r["by_equaliser"] = receive(split.ptr + 8 * victim * row)
            r["fer"] = {k: v["fer"] for k, v in r["by_equaliser"].items()}
            r["fer_soft"] = {k: v["fer_soft"] for k, v in r["by_equaliser"].items()}
            r["seconds"] = time.perf_counter() - t0
            pt["wideband"].append(r)
            print(json.dumps({"snr_db": snr, "neighbour_db": above, "fer": r["fer"], "fer_soft": r["fer_soft"], "seconds": r["seconds"]}), file=sys.stderr)
        points.append(pt)
    seconds_total = time.perf_counter() - t_all
    rx.free_out(ref)
    rx.free_out(dev)
    for d in (d_psdu_nb, rows, iq, chans, wide, split, d_int):
        if d is not None:
            d.free()
    rx.close()
    res = {"workload": "wideband loop-back on the device: M = %d channels, stacking %d, victim %d with %d distinct frames per point (64-QAM 3/4, PSDU "
                       "294 B, rows of 1472, lead 160, %s, CFO uniform in +-20 ppm), every other channel the same kind of frames back to back at "
                       "neighbour_db above the victim (null: silent); wifirx_combine -> AWGN of unit variance per channel bandwidth -> %s"
                       "wifirx_channelize -> demod, hard and soft decode_mac" % (
                           M, s, victim, n, "sv_taps.npy sets cycling" if a.multipath else "flat channel",
                           "a converter of %d bits, %.1f dB back-off -> " % (a.adc_bits[0], a.backoff_db) if a.adc_bits else ""),
           "columns": "per SNR: single_channel = the victim's rows without either bank; wideband = one entry per neighbour power",
           "equalisers": eqs, "stats": "wifirx_link_stats on the device", "seconds_total": seconds_total, "points": points}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


def diversity_main(a):
    if a.rates or a.host_stats or a.locked_clock or a.adc_bits is not None or a.wideband is not None:
        raise SystemExit("--antennas stands alone: not with --rates, --host-stats, --locked-clock, --adc-bits or --wideband")
    counts = sorted(set(a.antennas))
    if counts[0] < 1 or counts[-1] > capi.DIV_MAX_ANT:
        raise SystemExit("--antennas 1 .. %d" % capi.DIV_MAX_ANT)
    modes = a.diversity or ["mrc", "select"]
    n = a.frames or 65536
    plen, enc = a.psdu_len, a.encoding
    if not (28 <= plen <= 1528 and 0 <= enc <= 7):
        raise SystemExit("--psdu-len 28 .. 1528, --encoding 0 .. 7")
    fd = a.doppler[0] if a.doppler else 0.0
    n_sym, nb = txgen.n_sym_for(plen, enc), txgen.RATE_TABLE[enc][0]
    slot = LEAD + txgen.frame_samples(plen, enc) + 79
    slot += slot & 1
    stride = (plen + 15) // 16 * 16
    rx = capi.WifiRx(max_sym=n_sym, llr_bits=nb, want_carrier=True, chan_est=capi.EQ_LS, device=0)
    t_all = time.perf_counter()
    d_psdu, rows, iq = rx.alloc(n * plen), rx.alloc(n * slot * 8), rx.alloc(n * slot * 8)
    rx.mac_batch_dev(d_psdu.ptr, plen, n, None, payload_len=plen - 28, payload_seed=a.seed)
    rx.tx_batch_dev(rows.ptr, n * slot, d_psdu.ptr, enc, psdu_len=np.full(n, plen, np.uint32), psdu_stride=plen, lead=LEAD, row_len=slot)
    ref = dict(frames=rx.alloc(n * 32).upload(np.zeros(n * 32, np.uint8)), idx=rx.alloc(n * n_sym * 48), psdu=d_psdu, psdu_stride=plen)
    rx.demod_batch_dev(rows.ptr, slot, n, ref)
    assert rx.link_stats(n, ref, ref)["frames_ref"] == n, "a clean frame was not demodulated"
    ins = [rx.alloc_out(n, psdu_stride=stride, want_csi=True) for _ in range(counts[-1])]
    out = rx.alloc_out(n, psdu_stride=stride)

    def score(dev):
        rx.decode_batch_dev(n, dev)
        hard = rx.link_stats(n, dev, ref)
        rx.decode_batch_soft_dev(n, dev)
        soft = rx.link_stats(n, dev, ref)
        return {"fer": hard["fer"], "fer_soft": soft["fer"], "counts": {k: hard[k] for k in COUNTERS}, "counts_soft": {k: soft[k] for k in COUNTERS}}

    points = []
    for snr in a.snr:
        t0 = time.perf_counter()
        for ant, dev in enumerate(ins):
            rx.channel_dev(rows.ptr, iq.ptr, n * slot, n, row_len=slot, gain=math.sqrt(10 ** (snr / 10)), noise_voltage=1.0,
                           seed=9000 + int(snr) + (a.seed << 32) + (ant << 16), doppler=fd, k_factor=a.k_factor,
                           fade_seed=100 * a.seed + ant)
            rx.demod_batch_dev(iq.ptr, slot, n, dev)
        res = {}
        for A in counts:
            if A == 1:
                res["1"] = score(ins[0])          # (decode_mac marks the records DECODED / CRC_OK: the combiner clears that)
                continue
            for m in modes:
                rx.diversity_combine_dev(ins[:A], n, out, m)
                res["%d_%s" % (A, m)] = score(out)
        points.append({"snr_db": snr, "frames": n, "seconds": time.perf_counter() - t0, "fer": {k: v["fer"] for k, v in res.items()},
                       "fer_soft": {k: v["fer_soft"] for k, v in res.items()}, "by_antennas_and_mode": res})
        print(json.dumps({k: points[-1][k] for k in ("snr_db", "seconds", "fer", "fer_soft")}), file=sys.stderr)
    seconds_total = time.perf_counter() - t_all
    for d in ins + [out]:
        rx.free_out(d)
    rx.free_out(ref)
    rows.free(); iq.free(); rx.close()
    res = {"workload": "receive diversity on the device: %d distinct frames per point (wifirx_mac_batch, Philox payloads), encoding %d, PSDU %d B "
                       "(%d symbols), rows of %d, lead 160, per antenna one wifirx_channel_fading call (flat, doppler %g cycles per sample, "
                       "k_factor %g, its own fade_seed and noise seed, no carrier offset) and one LS demod; wifirx_diversity_combine; hard and "
                       "soft decode_mac" % (n, enc, plen, n_sym, slot, fd, a.k_factor),
           "columns": "fer / fer_soft per SNR: '1' = antenna 0 alone (no combiner), 'A_mode' = the first A antennas combined in that mode",
           "antennas": counts, "modes": modes, "stats": "wifirx_link_stats on the device; reported, not asserted",
           "seconds_total": seconds_total, "points": points}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


def precombine_main(a):
    """--antennas with --precombine: what combining in FRONT of the detector buys.  Every antenna's samples are kept; per SNR and
    antenna count A the same channel outputs go through (1) antenna 0's demod alone, (2) A demods and rule 23's MRC, (3)
    wifirx_precombine and one demod.  Rule 33 needs rows of a multiple of 64 samples."""
    if a.rates or a.host_stats or a.locked_clock or a.adc_bits is not None or a.wideband is not None:
        raise SystemExit("--precombine stands alone: not with --rates, --host-stats, --locked-clock, --adc-bits or --wideband")
    counts = sorted(set(a.antennas))
    if counts[0] < 1 or counts[-1] > capi.PRE_MAX_ANT or not 0 <= a.precombine_iters <= capi.PRE_MAX_ITERS:
        raise SystemExit("--antennas 1 .. %d, --precombine-iters 0 .. %d" % (capi.PRE_MAX_ANT, capi.PRE_MAX_ITERS))
    n = a.frames or 65536
    plen, enc = a.psdu_len, a.encoding
    if not (28 <= plen <= 1528 and 0 <= enc <= 7):
        raise SystemExit("--psdu-len 28 .. 1528, --encoding 0 .. 7")
    fd = a.doppler[0] if a.doppler else 0.0
    n_sym, nb = txgen.n_sym_for(plen, enc), txgen.RATE_TABLE[enc][0]
    slot = (LEAD + txgen.frame_samples(plen, enc) + 79 + 63) // 64 * 64
    stride = (plen + 15) // 16 * 16
    taps = np.load(os.path.join(ROOT, "tests", "golden", "sv_taps.npy")).astype(np.complex64) if a.multipath else (1.0,)
    rx = capi.WifiRx(max_sym=n_sym, llr_bits=nb, want_carrier=True, chan_est=capi.EQ_LS, device=0)
    t_all = time.perf_counter()
    d_psdu, rows, y = rx.alloc(n * plen), rx.alloc(n * slot * 8), rx.alloc(n * slot * 8)
    iqs = [rx.alloc(n * slot * 8) for _ in range(counts[-1])]
    d_stats = rx.alloc(n * 16)
    rx.mac_batch_dev(d_psdu.ptr, plen, n, None, payload_len=plen - 28, payload_seed=a.seed)
    rx.tx_batch_dev(rows.ptr, n * slot, d_psdu.ptr, enc, psdu_len=np.full(n, plen, np.uint32), psdu_stride=plen, lead=LEAD, row_len=slot)
    ref = dict(frames=rx.alloc(n * 32).upload(np.zeros(n * 32, np.uint8)), idx=rx.alloc(n * n_sym * 48), psdu=d_psdu, psdu_stride=plen)
    rx.demod_batch_dev(rows.ptr, slot, n, ref)
    assert rx.link_stats(n, ref, ref)["frames_ref"] == n, "a clean frame was not demodulated"
    ins = [rx.alloc_out(n, psdu_stride=stride, want_csi=True) for _ in range(counts[-1])]
    out = rx.alloc_out(n, psdu_stride=stride)

    def score(dev):
        rx.decode_batch_dev(n, dev)
        hard = rx.link_stats(n, dev, ref)
        rx.decode_batch_soft_dev(n, dev)
        soft = rx.link_stats(n, dev, ref)
        return {"fer": hard["fer"], "fer_soft": soft["fer"], "counts": {k: hard[k] for k in COUNTERS}, "counts_soft": {k: soft[k] for k in COUNTERS}}

    points = []
    for snr in a.snr:
        t0 = time.perf_counter()
        for ant, dev in enumerate(ins):
            # with --multipath every antenna cycles through the tap sets from another start, so that no two share a channel
            rx.channel_dev(rows.ptr, iqs[ant].ptr, n * slot, n, row_len=slot, taps=np.roll(taps, -7 * ant, axis=0) if a.multipath else taps,
                           gain=math.sqrt(10 ** (snr / 10)), noise_voltage=1.0, seed=9000 + int(snr) + (a.seed << 32) + (ant << 16),
                           doppler=fd, k_factor=a.k_factor, fade_seed=100 * a.seed + ant)
            rx.demod_batch_dev(iqs[ant].ptr, slot, n, dev)
        res = {"1": score(ins[0])}
        for A in counts:
            if A == 1:
                continue
            rx.diversity_combine_dev(ins[:A], n, out, "mrc")
            res["%d_mrc" % A] = score(out)
            rx.precombine_dev([b.ptr for b in iqs[:A]], slot, n, y.ptr, a.precombine_iters, None, d_stats.ptr)
            rx.demod_batch_dev(y.ptr, slot, n, out)
            res["%d_pre" % A] = score(out)
            res["%d_pre" % A]["degenerate_slots"] = int((d_stats.download(capi.PRE_STATS_DTYPE, n)["flags"] != 0).sum())
        points.append({"snr_db": snr, "frames": n, "seconds": time.perf_counter() - t0, "fer": {k: v["fer"] for k, v in res.items()},
                       "fer_soft": {k: v["fer_soft"] for k, v in res.items()}, "by_arm": res})
        print(json.dumps({k: points[-1][k] for k in ("snr_db", "seconds", "fer", "fer_soft")}), file=sys.stderr)
    seconds_total = time.perf_counter() - t_all
    for d in ins + [out]:
        rx.free_out(d)
    rx.free_out(ref)
    for b in [rows, y, d_stats] + iqs:
        b.free()
    rx.close()
    res = {"workload": "pre-detection combining on the device: %d distinct frames per point (wifirx_mac_batch, Philox payloads), encoding %d, "
                       "PSDU %d B (%d symbols), rows of %d, lead 160, per antenna one wifirx_channel_fading call (%s, doppler %g cycles per "
                       "sample, k_factor %g, its own fade_seed and noise seed, no carrier offset); LS demod; hard and soft decode_mac"
                       % (n, enc, plen, n_sym, slot, "sv_taps.npy sets cycling, every tap fading" if a.multipath else "flat", fd, a.k_factor),
           "columns": "fer / fer_soft per SNR: '1' = antenna 0 alone, 'A_mrc' = A demods and wifirx_diversity_combine (NUMERICS.md rule 23), "
                      "'A_pre' = wifirx_precombine (rule 33, %d power iterations) and ONE demod" % a.precombine_iters,
           "antennas": counts, "multipath": bool(a.multipath), "stats": "wifirx_link_stats on the device; reported, not asserted",
           "seconds_total": seconds_total, "points": points}
    print(json.dumps(res))
    if a.out:                                       # one file for both channels: the run lands under "flat" or "multipath"
        runs = {}
        if os.path.exists(a.out):
            with open(a.out) as f:
                runs = json.load(f).get("runs", {})
        runs["multipath" if a.multipath else "flat"] = res
        with open(a.out, "w") as f:
            f.write(json.dumps({"device": rx_device_name(), "runs": runs}, indent=1) + "\n")


def rx_device_name():
    try:
        import torch
        p = torch.cuda.get_device_properties(0)
        return "%s (%s, %d CUs)" % (p.name, getattr(p, "gcnArchName", "?"), p.multi_processor_count)
    except Exception as e:
        return "unknown (%s)" % e


def fading_main(a):
    if a.rates or a.host_stats or a.locked_clock:
        raise SystemExit("--doppler stands alone: not with --rates, --host-stats or --locked-clock")
    n = a.frames or 1_000_000
    plen, enc = a.psdu_len, a.encoding
    if not (28 <= plen <= 1528 and 0 <= enc <= 7):
        raise SystemExit("--psdu-len 28 .. 1528, --encoding 0 .. 7")
    eqs = a.eq or ["ls", "lms", "comb", "sta"]
    n_sym = txgen.n_sym_for(plen, enc)
    slot = LEAD + txgen.frame_samples(plen, enc) + 79
    slot += slot & 1
    stride = (plen + 15) // 16 * 16
    taps = np.load(os.path.join(ROOT, "tests", "golden", "sv_taps.npy")).astype(np.complex64) if a.multipath else (1.0,)
    rx = capi.WifiRx(max_sym=n_sym, llr_bits=0, chan_est=capi.EQ_LS, device=0)
    t_all = time.perf_counter()
    d_psdu, rows, iq = rx.alloc(n * plen), rx.alloc(n * slot * 8), rx.alloc(n * slot * 8)
    rx.mac_batch_dev(d_psdu.ptr, plen, n, None, payload_len=plen - 28, payload_seed=a.seed)
    rx.tx_batch_dev(rows.ptr, n * slot, d_psdu.ptr, enc, psdu_len=np.full(n, plen, np.uint32), psdu_stride=plen, lead=LEAD,
                    row_len=slot)
    dev = rx.alloc_out(n, psdu_stride=stride, want_hbits=True)
    ref = dict(frames=rx.alloc(n * 32).upload(np.zeros(n * 32, np.uint8)), idx=rx.alloc(n * n_sym * 48), hbits=rx.alloc(n * n_sym * 48),
               psdu=d_psdu, psdu_stride=plen)
    rx.demod_batch_dev(rows.ptr, slot, n, ref)
    assert rx.link_stats(n, ref, ref)["frames_ref"] == n, "a clean frame was not demodulated"
    points = []
    for snr in a.snr:
        for i, fd in enumerate(a.doppler):
            t0 = time.perf_counter()
            # one channel realisation per (SNR, Doppler); every equaliser sees the same samples
            rx.channel_dev(rows.ptr, iq.ptr, n * slot, n, row_len=slot, taps=taps, gain=math.sqrt(10 ** (snr / 10)), noise_voltage=1.0,
                           seed=9000 + int(snr) + (a.seed << 32), doppler=fd, k_factor=a.k_factor, fade_seed=100 * a.seed + i)
            by_eq = {}
            for name in eqs:
                rx.set_param(capi.P_CHAN_EST, EQUALISERS[name])
                rx.demod_batch_dev(iq.ptr, slot, n, dev)
                rx.decode_batch_dev(n, dev)
                r = rx.link_stats(n, dev, ref)
                by_eq[name] = {"fer": r["fer"], "coded_ber": r["coded_ber"], "coded_ber_se": r["coded_ber_se"],
                               "counts": {k: r[k] for k in COUNTERS}}
            rx.set_param(capi.P_CHAN_EST, capi.EQ_LS)
            points.append({"snr_db": snr, "doppler": fd, "frames": n, "seconds": time.perf_counter() - t0,
                           "fer": {k: v["fer"] for k, v in by_eq.items()}, "by_equaliser": by_eq})
            print(json.dumps({k: points[-1][k] for k in ("snr_db", "doppler", "seconds", "fer")}), file=sys.stderr)
    seconds_total = time.perf_counter() - t_all
    rx.free_out(ref)
    rx.free_out(dev)
    rows.free(); iq.free(); rx.close()
    res = {"workload": "loop-back on the device through wifirx_channel_fading: %d distinct frames per point (wifirx_mac_batch, Philox "
                       "payloads), encoding %d, PSDU %d B (%d symbols), rows of %d, lead 160, %s, k_factor %g, no carrier offset; hard "
                       "decode_mac; every equaliser on the same channel output"
                       % (n, enc, plen, n_sym, slot, "sv_taps.npy sets cycling, every tap fading" if a.multipath else "flat channel",
                          a.k_factor),
           "doppler_unit": "cycles per sample (1e-4 = 1 kHz at 10 MS/s)", "equalisers": eqs,
           "stats": "wifirx_link_stats on the device", "seconds_total": seconds_total, "points": points}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


def flatness(planes):
    """DESIGN.md 9n's figure, on the host from downloaded taps [antennas, sets, L]: per set the weakest over the mean of the
    MRC-combined spectrum sum_m |H_m[k]|^2 on the 52 occupied subcarriers (k = -26 .. 26 without 0) of the 64-point transform of
    the taps; the median over the sets"""
    spec = (np.abs(np.fft.fft(planes, 64, axis=2)) ** 2).sum(axis=0)
    used = spec[:, np.r_[1:27, 38:64]]
    return float(np.median(used.min(axis=1) / used.mean(axis=1)))


def estimate_keywords(a, S):
    """--irs-mode estimate: the keywords of irs_estimate_dev for an S x S surface, and what the result file says about them"""
    from wifirx import irs
    c = a.irs_group
    if c < 1 or S % c:
        raise SystemExit("--irs-group must divide the surface's side")
    G = (S // c) ** 2
    if G > capi.IRS_MAX_GROUPS:
        raise SystemExit("--irs-mode estimate takes at most %d groups: a larger --irs-group" % capi.IRS_MAX_GROUPS)
    pl = irs.dft_pilots(G) if a.irs_pilots == "dft" else irs.hadamard_pilots(G)
    sigma = 10 ** (-a.pilot_snr_db / 20)
    kw = dict(pilots=pl, group=None if c == 1 else irs.groups(S, c), sigma=sigma, est_scale=irs.est_scale(pl.shape[0]), align_bits=a.irs_bits)
    return kw, {"pilots": a.irs_pilots, "slots": int(pl.shape[0]), "groups": G, "sigma": sigma, "est_scale": float(kw["est_scale"])}


def estimate_taps(rx, a, decision, d_taps, n, pdp, b2r, r2u, b2u, est_kw, kw):
    """--irs-mode estimate: the taps of n sets at d_taps under the codes decided from the estimate -- by wifirx_irs_estimate itself
    (ref), or by estimate -> wifirx_irs_optimize -> wifirx_irs_taps_multi queued on the handle's stream (joint)"""
    if decision == "ref":
        rx.irs_estimate_dev(d_taps, n, pdp, b2r, r2u, b2u, **est_kw, **kw)
        return
    M, N = (1 if np.ndim(b2r) == 1 else np.shape(b2r)[0]), np.shape(b2r)[-1]
    weights = None if decision == "joint" else row_weights_of(a, decision[1], M, len(pdp))     # ("joint_w", tap weights or None)
    R, J = M * len(pdp), est_kw["pilots"].shape[1] + 1
    coef, psi = rx.alloc(n * R * J * 8), rx.alloc(n * N * 8)
    try:
        rx.irs_estimate_dev(None, n, pdp, b2r, r2u, b2u, est_ptr=coef, **dict(est_kw, align_bits=0), **kw)
        rx.irs_optimize_dev(coef, n, R, J, bits=est_kw["align_bits"], max_sweeps=a.irs_sweeps, start="ref",
                            direct_blocked=kw["direct_gain"] == 0.0, n_elems=N, group=est_kw["group"], psi_ptr=psi, weights=weights)
        rx.irs_taps_multi_dev(d_taps, n, pdp, b2r, r2u, b2u, psi=psi, n_psi_sets=n, **kw)
        rx.sync()
    finally:
        coef.free()
        psi.free()


def stretch(values, n):
    """W0 [W1 ...] of the command line as n values: the last one repeats"""
    v = list(values)[:n]
    return v + [v[-1]] * (n - len(v))


def row_weights_of(a, tap, M, L):
    """the rows' weights of an estimate_joint_w arm: irs.row_weights of the stretched --irs-tap-weights and --irs-ant-weights"""
    from wifirx import irs
    return irs.row_weights(M, L, tap=None if tap is None else stretch(tap, L),
                           ant=None if a.irs_ant_weights is None else stretch(a.irs_ant_weights, M))


def expand_modes(a, modes):
    """(mode, decision, label) per run: --irs-mode estimate once per --irs-decision, the joint one reported as estimate_joint and
    once more per --irs-tap-weights (or once for --irs-ant-weights alone) as estimate_joint_w, decision ("joint_w", tap weights)"""
    out = []
    for m in modes:
        if m == "estimate":
            out += [(m, d, "estimate" if d == "ref" else "estimate_joint") for d in a.irs_decision]
            if "joint" in a.irs_decision:
                arms = a.irs_tap_weights or ([None] if a.irs_ant_weights else [])
                out += [(m, ("joint_w", t), "estimate_joint_w") for t in arms]
        else:
            out.append((m, None, m))
    return out


def irs_main(a):
    if a.rates or a.host_stats or a.locked_clock or a.doppler is not None:
        raise SystemExit("--irs stands alone: not with --rates, --host-stats, --locked-clock or --doppler")
    from wifirx import irs
    n = a.frames or 65536
    plen, enc, bits = a.psdu_len, a.encoding, a.irs_bits
    if not (28 <= plen <= 1528 and 0 <= enc <= 7):
        raise SystemExit("--psdu-len 28 .. 1528, --encoding 0 .. 7")
    for N in a.irs:
        if N < 0 or N > capi.IRS_MAX_ELEMS or int(round(N ** 0.5)) ** 2 != N:
            raise SystemExit("--irs takes square surfaces of 0 .. 4096 elements")
    direct_gain = 0.0 if a.direct_db == float("-inf") else 10 ** (a.direct_db / 20)
    n_sym = txgen.n_sym_for(plen, enc)
    slot = LEAD + txgen.frame_samples(plen, enc) + 79
    slot += slot & 1
    stride = (plen + 15) // 16 * 16
    L = a.irs_taps
    pdp = np.exp(-np.arange(L) / 2.0)
    pdp = (pdp / pdp.sum()).astype(np.float32)
    rx = capi.WifiRx(max_sym=n_sym, llr_bits=0, chan_est=capi.EQ_LS, device=0)
    t_all = time.perf_counter()
    d_psdu, rows, iq, d_taps = rx.alloc(n * plen), rx.alloc(n * slot * 8), rx.alloc(n * slot * 8), rx.alloc(n * L * 8)
    d_best = rx.alloc(n * 2)
    rx.mac_batch_dev(d_psdu.ptr, plen, n, None, payload_len=plen - 28, payload_seed=a.seed)
    rx.tx_batch_dev(rows.ptr, n * slot, d_psdu.ptr, enc, psdu_len=np.full(n, plen, np.uint32), psdu_stride=plen, lead=LEAD,
                    row_len=slot)
    dev = rx.alloc_out(n, psdu_stride=stride, want_hbits=True)
    ref = dict(frames=rx.alloc(n * 32).upload(np.zeros(n * 32, np.uint8)), idx=rx.alloc(n * n_sym * 48), hbits=rx.alloc(n * n_sym * 48),
               psdu=d_psdu, psdu_stride=plen)
    rx.demod_batch_dev(rows.ptr, slot, n, ref)
    assert rx.link_stats(n, ref, ref)["frames_ref"] == n, "a clean frame was not demodulated"
    points = []
    for N in a.irs:
        # the surface in front of the AP as in the reference's scenes; --irs 0: one element that reflects nothing
        S = max(1, int(round(N ** 0.5)))
        irs_pos, ap_pos = [0.015, 0.015, 0], [S * 0.015, S * 0.015, 4.5]
        b2r, r2u, b2u = irs.los(S, irs_pos, ap_pos, [S * 0.015 + 0.3, S * 0.015 - 0.2, 1.0])
        for mode, decision, label in expand_modes(a, a.irs_mode if N else ["none"]):
            kw = dict(k_factor=a.k_factor, direct_gain=direct_gain if N else (direct_gain or 1.0), seed=(a.seed << 32) + N)
            winners = None
            if mode == "estimate":
                est_kw, winners = estimate_keywords(a, S)
            elif mode == "sweep":
                if a.irs_codebook == "traverse":
                    kw["codebook"] = irs.traverse_codebook(S, 0.03, irs_pos, ap_pos, accuracy=10, bits=bits)
                else:
                    kw["codebook"] = irs.dft_codebook(S, b2r, over=min(2 if a.irs_codebook == "dft2" else 1, max(1, 32 // S)), bits=bits)
            elif mode == "genie":
                kw["align_bits"] = bits
            elif mode == "los":
                kw["psi"] = irs.align(b2r, r2u, b2u if direct_gain else 0.0, bits)[1]
            elif mode == "random":
                kw["psi"] = irs.random_psi(N, bits, a.seed)
            else:
                kw["psi"] = np.zeros(1, np.complex64)
            # one tap set per frame, made on the device and read there by the channel
            if mode == "estimate":
                estimate_taps(rx, a, decision, d_taps, n, pdp, b2r, r2u, b2u, est_kw, kw)
            elif mode == "sweep":
                rx.irs_sweep_dev(d_taps, n, pdp, b2r, r2u, b2u, best_ptr=d_best, **kw)
                hist = np.bincount(d_best.download(np.uint16, n), minlength=kw["codebook"].shape[0])
                winners = {"entries": int(kw["codebook"].shape[0]), "distinct": int((hist > 0).sum()),
                           "histogram": {str(k): int(hist[k]) for k in np.nonzero(hist)[0]}}
            else:
                rx.irs_taps_dev(d_taps, n, pdp, b2r, r2u, b2u, **kw)
            sets = d_taps.download(np.complex64, min(n, 65536) * L).reshape(1, -1, L).astype(np.complex128)
            mean_power, tap0, flat = float((np.abs(sets) ** 2).sum() / sets.shape[1]), float((np.abs(sets[..., 0]) ** 2).mean()), flatness(sets)
            for snr in a.snr:
                t0 = time.perf_counter()
                rx.channel_dev(rows.ptr, iq.ptr, n * slot, n, row_len=slot, taps=d_taps.ptr, n_taps=L, n_tap_sets=n,
                               gain=math.sqrt(10 ** (snr / 10)), noise_voltage=1.0, seed=9000 + int(snr) + (a.seed << 32))
                rx.demod_batch_dev(iq.ptr, slot, n, dev)
                rx.decode_batch_dev(n, dev)
                r = rx.link_stats(n, dev, ref)
                points.append({"n_elems": N, "mode": label, "snr_db": snr, "frames": n, "fer": r["fer"], "coded_ber": r["coded_ber"],
                               "mean_channel_power": mean_power, "mean_tap0_power": tap0,
                               "median_weakest_subcarrier_over_mean": flat, "seconds": time.perf_counter() - t0,
                               "counts": {k: r[k] for k in COUNTERS}})
                if label == "estimate_joint_w":
                    points[-1]["row_weights"] = row_weights_of(a, decision[1], 1, L).tolist()
                if winners is not None:
                    points[-1]["training" if mode == "estimate" else "winners"] = winners
                print(json.dumps({k: points[-1][k] for k in ("n_elems", "mode", "snr_db", "fer", "mean_channel_power")}), file=sys.stderr)
    seconds_total = time.perf_counter() - t_all
    rx.free_out(ref)
    rx.free_out(dev)
    rows.free(); iq.free(); d_taps.free(); d_best.free(); rx.close()
    res = {"workload": "loop-back on the device over a reflecting surface (wifirx_irs_taps / wifirx_irs_sweep -> wifirx_channel, tap sets never leave the "
                       "device): %d distinct frames per point, one tap set per frame, encoding %d, PSDU %d B (%d symbols), rows of %d, "
                       "lead 160, %d taps (pdp exp(-l/2), sum 1), k_factor %g, direct path %s, %d-bit phases, LS, hard decode_mac"
                       % (n, enc, plen, n_sym, slot, L, a.k_factor, "blocked" if direct_gain == 0 else "%g dB" % a.direct_db, bits),
           "snr": "of one unit-power path (an element's leg, or the unattenuated direct path); n_elems 0 is the direct path alone at 0 dB",
           "modes": {"random": "one random configuration", "los": "the one configuration aligned to the geometry (irs.align)",
                     "genie": "aligned per draw on tap 0 (align_bits)",
                     "sweep": "trained per draw: the best entry of the %s codebook, quantised to the same bits (wifirx_irs_sweep, "
                              "NUMERICS.md rule 26); 'winners' holds the histogram of the winning entries" % a.irs_codebook,
                     "estimate": "trained per draw from a noisy pilot-based estimate of the direct path and of every group's cascade "
                                 "coefficient (wifirx_irs_estimate, NUMERICS.md rule 29); 'training' holds the pilots, the groups and "
                                 "the noise of one pilot observation",
                     "estimate_joint": "the same estimate, the codes decided jointly over the taps by at most %d sweeps of "
                                       "wifirx_irs_optimize from the estimate's own decision (NUMERICS.md rule 30)" % a.irs_sweeps,
                     "estimate_joint_w": "the same, decided by wifirx_irs_optimize_weighted on sum_rho w_rho |s_rho|^2 (NUMERICS.md rule "
                                         "31); 'row_weights' holds w, rho = antenna * taps + tap"},
           "stats": "wifirx_link_stats on the device", "seconds_total": seconds_total, "points": points}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


def irs_multi_main(a):
    """--irs with --antennas: the diversity receiver behind the surface.  Per antenna count A the surface is drawn for an AP of A
    antennas (wifirx_irs_taps_multi, or wifirx_irs_sweep_multi trained on the MRC metric), every antenna gets one wifirx_channel
    call on its plane with a noise seed of its own, and the A demodulated antennas are combined (wifirx_diversity_combine)."""
    if a.rates or a.host_stats or a.locked_clock or a.doppler is not None or a.adc_bits is not None or a.wideband is not None:
        raise SystemExit("--irs with --antennas: not with --rates, --host-stats, --locked-clock, --doppler, --adc-bits or --wideband")
    from wifirx import irs
    counts = sorted(set(a.antennas))
    if counts[0] < 1 or counts[-1] > min(capi.DIV_MAX_ANT, capi.IRS_MAX_ANT):
        raise SystemExit("--antennas 1 .. %d" % min(capi.DIV_MAX_ANT, capi.IRS_MAX_ANT))
    div = (a.diversity or ["mrc"])[0]
    n = a.frames or 65536
    plen, enc, bits = a.psdu_len, a.encoding, a.irs_bits
    if not (28 <= plen <= 1528 and 0 <= enc <= 7):
        raise SystemExit("--psdu-len 28 .. 1528, --encoding 0 .. 7")
    for N in a.irs:
        if N < 1 or N > capi.IRS_MAX_ELEMS or int(round(N ** 0.5)) ** 2 != N:
            raise SystemExit("--irs with --antennas takes square surfaces of 1 .. 4096 elements")
    modes = [m for m in a.irs_mode if m in ("random", "genie", "sweep", "estimate")]
    if len(modes) != len(a.irs_mode):
        raise SystemExit("--irs with --antennas: --irs-mode random, genie (on antenna 0), sweep (on the MRC metric) or estimate "
                         "(decided on antenna 0)")
    if a.irs_codebook == "traverse":
        raise SystemExit("--irs with --antennas: --irs-codebook dft or dft2")
    direct_gain = 0.0 if a.direct_db == float("-inf") else 10 ** (a.direct_db / 20)
    n_sym, nb = txgen.n_sym_for(plen, enc), txgen.RATE_TABLE[enc][0]
    slot = LEAD + txgen.frame_samples(plen, enc) + 79
    slot += slot & 1
    stride = (plen + 15) // 16 * 16
    L = a.irs_taps
    pdp = np.exp(-np.arange(L) / 2.0)
    pdp = (pdp / pdp.sum()).astype(np.float32)
    rx = capi.WifiRx(max_sym=n_sym, llr_bits=nb, want_carrier=True, chan_est=capi.EQ_LS, device=0)
    t_all = time.perf_counter()
    d_psdu, rows, iq = rx.alloc(n * plen), rx.alloc(n * slot * 8), rx.alloc(n * slot * 8)
    d_taps, d_best = rx.alloc(counts[-1] * n * L * 8), rx.alloc(n * 2)
    rx.mac_batch_dev(d_psdu.ptr, plen, n, None, payload_len=plen - 28, payload_seed=a.seed)
    rx.tx_batch_dev(rows.ptr, n * slot, d_psdu.ptr, enc, psdu_len=np.full(n, plen, np.uint32), psdu_stride=plen, lead=LEAD, row_len=slot)
    ref = dict(frames=rx.alloc(n * 32).upload(np.zeros(n * 32, np.uint8)), idx=rx.alloc(n * n_sym * 48), psdu=d_psdu, psdu_stride=plen)
    rx.demod_batch_dev(rows.ptr, slot, n, ref)
    assert rx.link_stats(n, ref, ref)["frames_ref"] == n, "a clean frame was not demodulated"
    ins = [rx.alloc_out(n, psdu_stride=stride, want_csi=True) for _ in range(counts[-1])]
    out = rx.alloc_out(n, psdu_stride=stride)
    points = []
    for N in a.irs:
        S = int(round(N ** 0.5))
        irs_pos, ap_pos, user_pos = [0.015, 0.015, 0], [S * 0.015, S * 0.015, 4.5], [S * 0.015 + 0.3, S * 0.015 - 0.2, 1.0]
        for A in counts:
            b2r, r2u, b2u = irs.los(S, irs_pos, ap_pos, user_pos, antennas=A)
            for mode, decision, label in expand_modes(a, modes):
                kw = dict(k_factor=a.k_factor, direct_gain=direct_gain, seed=(a.seed << 32) + N)       # irs_main's seeds
                winners = None
                if mode == "estimate":
                    est_kw, winners = estimate_keywords(a, S)
                    estimate_taps(rx, a, decision, d_taps, n, pdp, b2r, r2u, b2u, est_kw, kw)
                elif mode == "sweep":
                    kw["codebook"] = irs.dft_codebook(S, b2r[0], over=min(2 if a.irs_codebook == "dft2" else 1, max(1, 32 // S)), bits=bits)
                    rx.irs_sweep_multi_dev(d_taps, n, pdp, b2r, r2u, b2u, best_ptr=d_best, **kw)
                    hist = np.bincount(d_best.download(np.uint16, n), minlength=kw["codebook"].shape[0])
                    winners = {"entries": int(kw["codebook"].shape[0]), "distinct": int((hist > 0).sum())}
                elif mode == "genie":
                    rx.irs_taps_multi_dev(d_taps, n, pdp, b2r, r2u, b2u, align_bits=bits, **kw)
                else:
                    rx.irs_taps_multi_dev(d_taps, n, pdp, b2r, r2u, b2u, psi=irs.random_psi(N, bits, a.seed), **kw)
                k = min(n, 65536)
                planes = d_taps.download(np.complex64, A * n * L).reshape(A, n, L)[:, :k].astype(np.complex128)
                power = (np.abs(planes) ** 2).sum(axis=2).mean(axis=1)          # per antenna: the mean over the sets of sum_l |t|^2
                tap0, flat = float((np.abs(planes[..., 0]) ** 2).sum(axis=0).mean()), flatness(planes)
                for snr in a.snr:
                    t0 = time.perf_counter()
                    for ant in range(A):
                        rx.channel_dev(rows.ptr, iq.ptr, n * slot, n, row_len=slot, taps=d_taps.ptr + ant * n * L * 8, n_taps=L,
                                       n_tap_sets=n, gain=math.sqrt(10 ** (snr / 10)), noise_voltage=1.0,
                                       seed=9000 + int(snr) + (a.seed << 32) + (ant << 16))
                        rx.demod_batch_dev(iq.ptr, slot, n, ins[ant])
                    dev = ins[0]
                    if A > 1:
                        rx.diversity_combine_dev(ins[:A], n, out, div)
                        dev = out
                    rx.decode_batch_dev(n, dev)
                    hard = rx.link_stats(n, dev, ref)
                    rx.decode_batch_soft_dev(n, dev)
                    soft = rx.link_stats(n, dev, ref)
                    points.append({"n_elems": N, "antennas": A, "mode": label, "snr_db": snr, "frames": n, "fer": hard["fer"],
                                   "fer_soft": soft["fer"], "mean_combined_channel_power": float(power.sum()),
                                   "mean_channel_power_per_antenna": [float(v) for v in power], "mean_combined_tap0_power": tap0,
                                   "median_weakest_subcarrier_over_mean": flat, "seconds": time.perf_counter() - t0,
                                   "counts": {c: hard[c] for c in COUNTERS}, "counts_soft": {c: soft[c] for c in COUNTERS}})
                    if label == "estimate_joint_w":
                        points[-1]["row_weights"] = row_weights_of(a, decision[1], A, L).tolist()
                    if winners is not None:
                        points[-1]["training" if mode == "estimate" else "winners"] = winners
                    print(json.dumps({c: points[-1][c] for c in ("n_elems", "antennas", "mode", "snr_db", "fer", "fer_soft",
                                                                 "mean_combined_channel_power")}), file=sys.stderr)
    seconds_total = time.perf_counter() - t_all
    for d in ins + [out]:
        rx.free_out(d)
    rx.free_out(ref)
    rows.free(); iq.free(); d_taps.free(); d_best.free(); rx.close()
    res = {"workload": "the diversity receiver behind a reflecting surface, on the device (wifirx_irs_taps_multi / wifirx_irs_sweep_multi -> one "
                       "wifirx_channel per antenna on its plane -> LS demod -> wifirx_diversity_combine (%s) -> hard and soft decode_mac; the tap "
                       "sets never leave the device): %d distinct frames per point, one tap set per frame and antenna, encoding %d, PSDU %d B "
                       "(%d symbols), rows of %d, lead 160, %d taps (pdp exp(-l/2), sum 1), k_factor %g, direct path %s, %d-bit phases; the AP a "
                       "half-wavelength array along x (irs.los(antennas=A))"
                       % (div, n, enc, plen, n_sym, slot, L, a.k_factor, "blocked" if direct_gain == 0 else "%g dB" % a.direct_db, bits),
           "snr": "of one unit-power path at one antenna; every antenna has noise of variance 1 from a seed of its own",
           "modes": {"random": "one random configuration", "genie": "aligned per draw on antenna 0, tap 0 (align_bits)",
                     "sweep": "trained per draw on the sum of the antennas' channel powers: the best entry of the %s codebook, quantised to "
                              "the same bits (wifirx_irs_sweep_multi, NUMERICS.md rule 28)" % a.irs_codebook,
                     "estimate": "trained per draw from a noisy pilot-based estimate, the codes decided on antenna 0, tap 0 "
                                 "(wifirx_irs_estimate, NUMERICS.md rule 29)",
                     "estimate_joint": "the same estimate, the codes decided jointly over antennas and taps by at most %d sweeps of "
                                       "wifirx_irs_optimize from the estimate's own decision (NUMERICS.md rule 30)" % a.irs_sweeps,
                     "estimate_joint_w": "the same, decided by wifirx_irs_optimize_weighted on sum_rho w_rho |s_rho|^2 (NUMERICS.md rule "
                                         "31); 'row_weights' holds w, rho = antenna * taps + tap"},
           "antennas": counts, "stats": "wifirx_link_stats on the device; reported, not asserted",
           "seconds_total": seconds_total, "points": points}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


def host_stats_by_rate(rx, dev, n, max_sym, enc, p, fr_tx, idx_tx):
    """the bookkeeping of wifirx_link_stats_by_rate on the host, from the downloaded records, PSDU rows and decisions"""
    fr = dev["frames"].download(capi.FRAME_DTYPE, n)
    got = dev["psdu"].download(np.uint8, n * 304).reshape(n, 304)[:, :PSDU_LEN]
    idx = dev["idx"].download(np.uint8, n * max_sym * 48).reshape(n, -1)
    out = []
    for e in range(8):
        sel = np.nonzero(enc == e)[0]
        f, ft = fr[sel], fr_tx[sel]
        n_sym, nb = txgen.n_sym_for(PSDU_LEN, e), txgen.RATE_TABLE[e][0]
        crc = (f["flags"] & capi.F_CRC_OK) != 0
        ok = crc & (f["psdu_len"] == PSDU_LEN) & (got[sel] == p[sel]).all(axis=1)
        good = (((f["flags"] & capi.F_COMPLETE) != 0) & (f["encoding"] == ft["encoding"]) & (f["psdu_len"] == ft["psdu_len"])
                & (f["n_sym"] == ft["n_sym"]))
        err = POPCOUNT6[idx[sel][good][:, :n_sym * 48] ^ idx_tx[sel][good][:, :n_sym * 48]].sum(axis=1, dtype=np.int64)
        out.append(dict(frames=sel.size, frames_ref=sel.size, frames_good=int(good.sum()), frames_crc_ok=int(crc.sum()),
                        frames_psdu_ok=int(ok.sum()), frames_crc_ok_wrong=int((crc & ~ok).sum()),
                        coded_bits=int(good.sum()) * n_sym * 48 * nb, coded_bit_errors=int(err.sum()),
                        coded_bit_errors_sq=int((err * err).sum())))
    return out


def rates_main(a):
    n = a.frames or 131072
    n -= n % 8
    enc = (np.arange(n) % 8).astype(np.uint8)
    flen = np.array([txgen.frame_samples(PSDU_LEN, e) for e in range(8)])
    max_sym = txgen.n_sym_for(PSDU_LEN, 0)
    tail = 32
    row_of = LEAD + flen + tail
    row_of += row_of & 1
    row_off = np.concatenate([[0], np.cumsum(row_of[enc])]).astype(np.uint64)
    total = int(row_off[-1])
    taps = np.load(os.path.join(ROOT, "tests", "golden", "sv_taps.npy")).astype(np.complex64)
    rx = capi.WifiRx(max_sym=max_sym, llr_bits=6, chan_est=capi.EQ_LS, device=0)
    rx.set_llr_format("bf16")
    t_all = time.perf_counter()
    d_psdu, rows, iq = rx.alloc(n * PSDU_LEN), rx.alloc(total * 8), rx.alloc(total * 8)
    rx.mac_batch_dev(d_psdu.ptr, PSDU_LEN, n, None, payload_len=PSDU_LEN - 28, payload_seed=a.seed)
    rx.tx_batch_dev(rows.ptr, total, d_psdu.ptr, enc, psdu_len=np.full(n, PSDU_LEN, np.uint32), psdu_stride=PSDU_LEN,
                    lead=LEAD, row_off=row_off)
    dev = rx.alloc_out(n, psdu_stride=304, want_hbits=True)
    ref = dict(frames=rx.alloc(n * 32).upload(np.zeros(n * 32, np.uint8)), idx=rx.alloc(n * max_sym * 48),
               hbits=rx.alloc(n * max_sym * 48), psdu=d_psdu, psdu_stride=PSDU_LEN)
    rx.demod_batch_var_dev(rows.ptr, row_off, ref)
    clean = rx.link_stats(n, ref, ref, by_rate=True)
    assert clean["frames_ref"] == n and all(b["frames_good"] == n // 8 for b in clean["by_rate"]), "a clean frame was not demodulated"
    if a.host_stats:
        p = d_psdu.download(np.uint8, n * PSDU_LEN).reshape(n, PSDU_LEN)
        fr_tx = ref["frames"].download(capi.FRAME_DTYPE, n)
        idx_tx = ref["idx"].download(np.uint8, n * max_sym * 48).reshape(n, -1)
    payload_bits = 8 * (PSDU_LEN - 28)
    points = []
    for snr in a.snr:
        t0 = time.perf_counter()
        cfo = np.random.default_rng(int(1000 * snr) + a.seed).uniform(-CFO_20PPM, CFO_20PPM, n).astype(np.float32)
        rx.channel_dev(rows.ptr, iq.ptr, total, n, row_off=row_off, taps=taps, cfo=cfo, gain=math.sqrt(10 ** (snr / 10)),
                       noise_voltage=1.0, seed=9000 + int(snr) + (a.seed << 32),
                       sro=capi.locked_sro(cfo) if a.locked_clock else None)
        rx.demod_batch_var_dev(iq.ptr, row_off, dev)
        both = []
        for soft in (False, True):
            (rx.decode_batch_soft_dev if soft else rx.decode_batch_dev)(n, dev)
            r = rx.link_stats(n, dev, ref, by_rate=True)
            assert {k: r[k] for k in COUNTERS} == {k: rx.link_stats(n, dev, ref)[k] for k in COUNTERS}
            if a.host_stats:
                hs = host_stats_by_rate(rx, dev, n, max_sym, enc, p, fr_tx, idx_tx)
                for e in range(8):
                    assert {k: r["by_rate"][e][k] for k in COUNTERS} == hs[e], ("soft" if soft else "hard", e, r["by_rate"][e], hs[e])
            both.append(r)
        hard, soft = both
        rates = []
        for e in range(8):
            h, s = hard["by_rate"][e], soft["by_rate"][e]
            rates.append({"encoding": e, "frame_samples": int(flen[e]), "fer": h["fer"], "fer_soft": s["fer"],
                          "coded_ber": h["coded_ber"], "coded_ber_se": h["coded_ber_se"],
                          "goodput_bits_per_sample": h["frames_psdu_ok"] * payload_bits / (h["frames_ref"] * float(flen[e])),
                          "goodput_bits_per_sample_soft": s["frames_psdu_ok"] * payload_bits / (s["frames_ref"] * float(flen[e])),
                          "counts": {k: h[k] for k in COUNTERS}, "counts_soft": {k: s[k] for k in COUNTERS}})
        best = max(rates, key=lambda q: q["goodput_bits_per_sample_soft"])
        points.append({"snr_db": snr, "frames": n, "seconds": time.perf_counter() - t0, "best_encoding_soft": best["encoding"],
                       "counts": {k: hard[k] for k in COUNTERS}, "counts_soft": {k: soft[k] for k in COUNTERS}, "rates": rates})
        print(json.dumps({"snr_db": snr, "seconds": points[-1]["seconds"],
                          "fer": [q["fer"] for q in rates], "fer_soft": [q["fer_soft"] for q in rates],
                          "goodput_soft": [round(q["goodput_bits_per_sample_soft"], 4) for q in rates]}), file=sys.stderr)
    seconds_total = time.perf_counter() - t_all
    rx.free_out(ref)
    rx.free_out(dev)
    rows.free(); iq.free(); rx.close()
    # the encoding-7 column is config 3's experiment with other noise: both FERs side by side, with the binomial standard
    # error of each; nothing is asserted
    side, c3 = [], os.path.join(ROOT, "profiles", "loopback_per_config3_device_stats.json")
    if os.path.exists(c3):
        with open(c3) as f:
            rec = json.load(f)
        old = {q["snr_db"]: q for q in rec.get("record", rec).get("points", [])}
        se = lambda f_, m: math.sqrt(max(f_ * (1.0 - f_), 0.0) / m)
        for q in points:
            o = old.get(q["snr_db"])
            if o is None:
                continue
            r7 = q["rates"][7]
            for key in ("fer", "fer_soft"):
                side.append({"snr_db": q["snr_db"], "what": key, "here": r7[key], "here_se": se(r7[key], n // 8),
                             "config3": o[key], "config3_se": se(o[key], o["frames"])})
                print("encoding 7, %g dB, %s: %.5f +- %.5f here, %.5f +- %.5f in config 3's sweep"
                      % (q["snr_db"], key, r7[key], side[-1]["here_se"], o[key], side[-1]["config3_se"]), file=sys.stderr)
    res = {"workload": "loop-back on the device, the eight encodings cycling: %d distinct frames per point (%d per rate; wifirx_mac_batch, "
                       "Philox payloads), PSDU 294 B, row_off rows of lead 160 + frame + %d rounded up to even, sv_taps.npy sets cycling, "
                       "CFO uniform in +-20 ppm, LS; hard and soft decode_mac" % (n, n // 8, tail)
                       + ("; sample clock locked to the carrier (wifirx_channel_sro, sro = -cfo bw / (2 pi fc))" if a.locked_clock else ""),
           "llr": "bf16 (WIFIRX_LLR_BF16), 6 per carrier, max_sym %d: %d bytes per frame" % (max_sym, max_sym * 48 * 6 * 2),
           "stats": "wifirx_link_stats_by_rate on the device" + (", checked against the NumPy bookkeeping" if a.host_stats else ""),
           "goodput": "frames_psdu_ok * %d payload bits / (frames_ref * frame_samples)" % payload_bits,
           "seconds_total": seconds_total, "points": points, "encoding_7_against_config3": side}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
