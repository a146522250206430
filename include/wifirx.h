/*
 * wifirx.h -- C ABI of libwifirx.so: the MI355X-native IEEE 802.11a/g OFDM PHY receive chain (and, wifirx_tx_batch, the
 * transmitter that feeds it).
 *
 * This is the drop-in boundary for the RX half of the reference's `wifi_phy_hier` hier block
 * (gnu_radio/wifi_phy_hier.grc:100-260,480-569,698-768), which IRS_AP inlines block for block
 * (gnu_radio/IRS_AP.py:267-285,291-311).  The reference has no FFI of its own for this path (its
 * blocks are GNU Radio C++ objects reached through SWIG/pybind); a GNU Radio block that wants the
 * GPU path binds exactly these entry points (ctypes stub in INTEGRATION.md).  Every function
 * replaces the work() of the reference blocks named beside it.
 *
 * Plain C: pointers and sizes only, no torch / HIP types.  All functions return 0 on success or a
 * negative WIFIRX_E* code; nothing throws across the boundary; no global state: every call works
 * on a handle.  One handle = one stream of samples = one HIP stream; calls on one handle must be
 * serialised by the caller, different handles are independent (GNU Radio runs each block on its
 * own thread, so this matches the reference's threading).  Stream mode with WIFIRX_P_STREAM_BATCH runs its
 * device pipeline on a worker thread owned by the handle: wifirx_push returns while a batch is still in flight.
 * That stays internal: every other entry point of the handle (batch calls, decode, set_param, sync, memcpy) first
 * waits for the batch in flight, and wifirx_last_error only ever shows text written on the caller's thread.
 *
 * There is NO CPU fallback in this library: wifirx_create() fails with WIFIRX_ENODEV when no
 * gfx950 device is usable.  The CPU restatement lives in oracle/ and is test infrastructure only.
 */
#ifndef WIFIRX_H
#define WIFIRX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WIFIRX_ABI_VERSION 4

/* error codes */
#define WIFIRX_OK        0
#define WIFIRX_EINVAL   -1   /* bad argument */
#define WIFIRX_ENODEV   -2   /* no usable HIP device / kernel image (gfx950) */
#define WIFIRX_ENOMEM   -3   /* device or host allocation failed */
#define WIFIRX_EHIP     -4   /* HIP runtime error (wifirx_last_error() has the text) */
#define WIFIRX_ERANGE   -5   /* buffer too small / index out of range */
#define WIFIRX_EDEAD    -6   /* the handle's stream is dead (its sample buffer was lost): nothing to retry, destroy the handle */

/* Equalizer enum of the reference: ieee802_11.Equalizer (gnu_radio/IRS_AP.py:139-141). */
#define WIFIRX_EQ_LS   0
#define WIFIRX_EQ_LMS  1
#define WIFIRX_EQ_COMB 2
#define WIFIRX_EQ_STA  3

/* Encoding enum of the reference: ieee802_11.Encoding (gnu_radio/IRS_user.py:130-132). */
#define WIFIRX_BPSK_1_2   0
#define WIFIRX_BPSK_3_4   1
#define WIFIRX_QPSK_1_2   2
#define WIFIRX_QPSK_3_4   3
#define WIFIRX_16QAM_1_2  4
#define WIFIRX_16QAM_3_4  5
#define WIFIRX_64QAM_2_3  6
#define WIFIRX_64QAM_3_4  7

/* constants of the upstream blocks the chain follows */
#define WIFIRX_SYNC_LENGTH   320     /* sync_long(sync_length), gnu_radio/wifi_phy_hier.grc:59-75 */
#define WIFIRX_MIN_GAP       480     /* sync_short: re-trigger only after this many copied samples */
#define WIFIRX_MAX_SAMPLES   (540 * 80)
#define WIFIRX_MAX_SYM       511     /* decode_mac: frames with more data symbols are dropped */
#define WIFIRX_MAX_PSDU      1528    /* decode_mac: MAX_PAYLOAD 1500 + 28 */

/* frame flags */
#define WIFIRX_F_DETECTED   0x01u   /* sync_short plateau found (trigger valid) */
#define WIFIRX_F_SYNC       0x02u   /* sync_long found an LTS peak pair (frame_start, cfo_fine valid) */
#define WIFIRX_F_SIGNAL     0x04u   /* SIGNAL field decoded: parity ok and known rate */
#define WIFIRX_F_COMPLETE   0x08u   /* all n_sym data symbols lie inside the available samples and the
                                       output capacity (max_sym) and were written */
#define WIFIRX_F_LLR        0x10u   /* LLRs written for this frame (n_bpsc <= llr_bits) */
#define WIFIRX_F_DECODED    0x20u   /* decode_mac ran (Viterbi + descramble) */
#define WIFIRX_F_CRC_OK     0x40u   /* FCS good: PSDU delivered */
#define WIFIRX_F_TRUNCATED  0x80u   /* demodulation stopped because the samples of this trigger (or the
                                       output capacity max_sym) ran out, not because sync/SIGNAL failed */

/* One record per slot (batch mode) or per detected frame (stream mode): the stream tags
 * `wifi_start` of sync_short / sync_long / frame_equalizer rolled into one. */
typedef struct wifirx_frame {
    uint32_t flags;
    int32_t  trigger;      /* index n (in the slot / the stream) of the sync_short trigger sample of
                              the 16-delayed input, -1 if none; first copied sample is x[trigger-16] */
    int32_t  frame_start;  /* sync_long d_frame_start: offset of LTS1 in the copied samples (0..320) */
    float    cfo_coarse;   /* sync_short:  arg(A[trigger])/16          rad/sample */
    float    cfo_fine;     /* sync_long:   arg(p1*conj(p2))/64         rad/sample (upstream sign) */
    float    snr_db;       /* LS equalizer SNR estimate from LTS1/LTS2 */
    uint16_t psdu_len;     /* SIGNAL LENGTH ("frame_bytes") */
    uint8_t  encoding;     /* WIFIRX_BPSK_1_2 .. WIFIRX_64QAM_3_4 */
    uint8_t  n_bpsc;       /* bits per sub-carrier of `encoding` */
    uint16_t n_sym;        /* data symbols the SIGNAL field announces */
    uint16_t n_sym_out;    /* data symbols actually demodulated into the output buffers */
} wifirx_frame;            /* 32 bytes */

typedef struct wifirx_config {
    uint32_t abi_version;  /* WIFIRX_ABI_VERSION */
    int32_t  device;       /* HIP device ordinal */
    double   bandwidth;    /* sample rate in Hz: wifi_phy_hier `bandwidth` (grc:83-92) */
    double   frequency;    /* carrier in Hz:    wifi_phy_hier `frequency` (grc:501-510) */
    float    sensitivity;  /* sync_short threshold: wifi_phy_hier `sensitivity` (grc:681-690), 0.56.  Must be >= 0: the
                              detect phase compares |A|^2 > (sensitivity * P)^2 (NUMERICS.md rule 3), under which a
                              negative value would act as its magnitude, whereas upstream's |A| / P > sensitivity is then
                              true wherever P > 0.  A negative value or a NaN is WIFIRX_EINVAL, here and in
                              wifirx_set_param. */
    int32_t  min_plateau;  /* sync_short min_plateau, 2 (gnu_radio/IRS_AP.py:268) */
    int32_t  chan_est;     /* WIFIRX_EQ_*: wifi_phy_hier `chan_est` (grc:299-308, IRS_AP.py:139-141) */
    uint32_t max_sym;      /* output capacity per frame in data symbols (<= WIFIRX_MAX_SYM) */
    uint32_t llr_bits;     /* LLR capacity per sub-carrier (0 = no LLR output, else 1,2,4,6) */
    uint32_t want_carrier; /* 1: also write the 48 equalised points per symbol (`carrier` port) */
    uint32_t max_batch;    /* largest n_slots of a wifirx_demod_batch call (workspace size) */
    uint32_t max_slot_len; /* largest slot length in samples */
} wifirx_config;

/* parameter ids for wifirx_set_param: the setters the reference flowgraphs call
 * (gnu_radio/IRS_user.py:229,265,273; gnu_radio/IRS_AP.py:348,373,382) */
#define WIFIRX_P_BANDWIDTH   1
#define WIFIRX_P_FREQUENCY   2
/* >= 0 (see wifirx_config.sensitivity); a refused value leaves the handle's value as it was.  In stream mode the new value
 * acts on every sample the detection has not yet run over: the samples of later pushes and, with WIFIRX_P_STREAM_BATCH,
 * the samples already pushed that are still staged for their batch.  Samples already detected keep their triggers. */
#define WIFIRX_P_SENSITIVITY 3
#define WIFIRX_P_CHAN_EST    4
/* stream mode: wifirx_push only collects samples until this many are waiting, then detects / demodulates /
 * decodes them in one go (0 = on every push).  A GNU Radio scheduler hands work() a few thousand items at a
 * time; one GPU round trip per such call would not keep up with the sample rate.  A push with n = 0 flushes.
 * At most WIFIRX_STREAM_BATCH_MAX (two pinned host buffers of one batch each are kept).  Changing the value while
 * samples are staged first runs those samples as a (short) batch.
 * ERRORS: the stream never gains a gap or a doubled sample through a failed push.  wifirx_push_consumed() tells how
 * many leading samples of the last wifirx_push call the stream has taken over: all of them after WIFIRX_OK; after an
 * error 0 -- repeat the call as it was (an allocation may succeed now) --, except for a call that spanned several
 * batches (n > batch size), which may have taken a prefix: repeat it from there.  Without a batch size a failed pass
 * is undone as a whole.  With one, the failure of a batch on the worker thread is reported by the NEXT push / flush
 * (once, before it takes anything); the failed batch stays staged in the library and the call after that runs it
 * again before going on.  A pass whose frames are queued is committed: a device failure behind that point (the carry of the
 * samples a pending frame still needs) is never reported as a failed push.  If it struck before the sample buffer was
 * touched, the stream goes on unharmed; if the buffer can no longer be trusted, every later push returns WIFIRX_EDEAD
 * with wifirx_push_consumed() = 0 and a text that says the stream is dead -- not a condition to retry: destroy the handle
 * (a GNU Radio work() answers it with WORK_DONE, wifirx/block.py). */
#define WIFIRX_P_STREAM_BATCH 5
#define WIFIRX_STREAM_BATCH_MAX (1u << 27)
/* decode_mac has two kernels with identical results: 128 frames per wave (throughput; a lone wave needs ~4 ms)
 * and one frame per wave (latency; ~0.2 ms per frame).  Batches of up to this many frames take the second one
 * (default 16384; 0 = always the first). */
#define WIFIRX_P_DECODE_SMALL_MAX 6
/* 1: every LLR is multiplied by |H|^2 of its sub-carrier (the LS channel estimate of the two long training
 * symbols; the optional channel-state weight of SURVEY.md section 8 row a7).  Default 0: plain max-log LLRs. */
#define WIFIRX_P_LLR_CSI 7
/* stream mode: 0 = the hard decisions of the frames stay on the device (wifirx_poll* then delivers zeros for `idx`);
 * default 1.  A consumer of PDUs only (the wifi_phy_rx block) saves most of the device-to-host traffic of a push. */
#define WIFIRX_P_STREAM_IDX 8
/* stream mode: 1 = decode_mac runs on LLRs (wifirx_decode_batch_soft, NUMERICS.md rule 14) instead of the hard decisions.
 * The frame kernel then writes LLRs with 6 bits per carrier reserved into rows the handle owns (max_sym * 48 * 6 floats
 * per trigger, allocated once the mode is on), whatever cfg.llr_bits is; WIFIRX_P_LLR_CSI weights them as in batch mode.
 * The frame records of such a batch are those of a handle created with llr_bits = 6: WIFIRX_F_LLR is set for every frame
 * whose symbols were demodulated, also on a handle with llr_bits = 0 (wifirx_poll* still has no LLR output).
 * Default 0 (the upstream hard-decision decoder); other values are WIFIRX_EINVAL.  Batches run after the call use it. */
#define WIFIRX_P_STREAM_SOFT 9
/* LLR format of the batch calls made after it is set (NUMERICS.md rule 15): WIFIRX_LLR_F32 (default) = float32 values;
 * WIFIRX_LLR_BF16 = bfloat16 values, each the IEEE round-to-nearest-even conversion of the float32 LLR the default format
 * would write (weight of WIFIRX_P_LLR_CSI included; NaN stays a NaN, +-inf and subnormals are kept).  In bf16 mode
 * wifirx_out.llr points to uint16_t bit patterns with the same element layout, so its strides and sizes are half the float32
 * ones in bytes.  It applies to wifirx_demod_batch / wifirx_demod_batch_v (device and host outputs), wifirx_time_demod and
 * wifirx_decode_batch_soft (which reads rows in the handle's current format).  Stream mode ignores it: wifirx_push / wifirx_poll*,
 * the WIFIRX_P_STREAM_SOFT rows and the GNU Radio block keep float32.  Other values are WIFIRX_EINVAL. */
#define WIFIRX_P_LLR_FORMAT 10
#define WIFIRX_LLR_F32  0
#define WIFIRX_LLR_BF16 1

typedef struct wifirx_handle wifirx_handle;

/* Output buffers of a batch call.  Every pointer is caller-owned DEVICE memory when
 * `on_device` != 0, HOST memory otherwise (the library then stages through its own device
 * buffers; that path is PCIe-bound and is not the measured one).  NULL = do not produce.
 *   frames  [n_slots]
 *   idx     [n_slots][max_sym][48]            hard decisions, one constellation index per byte
 *                                              (output 0 of frame_equalizer, grc:550-569)
 *   llr     [n_slots][max_sym*48*llr_bits]    per frame packed [sym][carrier][bit 0..n_bpsc-1]: element
 *                                              (q*48 + k)*n_bpsc + b of a frame = bit b of carrier k of data
 *                                              symbol q.  float32 values, or uint16_t bf16 bit patterns (half
 *                                              the bytes) when WIFIRX_P_LLR_FORMAT = WIFIRX_LLR_BF16
 *   carrier [n_slots][max_sym][48][2]         equalised points (re,im): the `symbols` message port
 *   psdu    [n_slots][psdu_stride]            decode_mac output: MAC frame incl. FCS position
 *                                              (bytes 0..psdu_len-1), valid when WIFIRX_F_CRC_OK
 *   csi     [n_slots][52][2]                  channel state (re,im) on the 52 occupied sub-carriers in ascending
 *                                              order: the LS estimate from the two long training symbols (what
 *                                              the reference's disabled extract_csi block taps,
 *                                              gnu_radio/IRS_AP.grc:640-654); written once SYNC is set
 */
typedef struct wifirx_out {
    wifirx_frame* frames;
    uint8_t*      idx;
    float*        llr;
    float*        carrier;
    uint8_t*      psdu;
    uint32_t      psdu_stride;  /* bytes per slot in `psdu` (>= largest psdu_len expected) */
    uint32_t      on_device;
    float*        csi;          /* ABI 2 */
    float*        sym_stats;    /* ABI 3: [n_slots][4] = sum |y|, sum |y|^2, sum |y|^4 over the equalised points of the
                                   frame's n_sym_out data symbols (48 each), 0 -- the statistics a
                                   digital.probe_mpsk_snr_est_c fed from frame_equalizer's `symbols` port accumulates
                                   (gnu_radio/IRS_AP.py:275,312); float32 sums in the order of DESIGN.md rule 13 */
    uint32_t*     hbits;        /* ABI 4: [n_slots][max_sym * 12] -- the hard decisions of `idx` as bit planes, the form
                                   wifirx_decode_batch reads (decode_mac's input, gnu_radio/IRS_AP.py:272).  Data symbol
                                   q of a frame with n_bpsc bits per carrier occupies the 2 * n_bpsc words from
                                   q * 2 * n_bpsc on (symbols are packed; 48 bytes per symbol are reserved, as for
                                   `idx`); word 2 b + h holds bit b of the decisions of the FFT bins 32 h .. 32 h + 31
                                   (shifted order: bin 32 = DC; data carrier c of `idx` is bin c + 6 + the pilots / DC
                                   below it), bin 32 h + k in bit k, 0 for bins that carry no data.  Optional: when
                                   given, wifirx_demod_batch fills it and wifirx_decode_batch reads it instead of
                                   `idx`; words behind a frame's last symbol are not written. */
} wifirx_out;

/* Output buffers of wifirx_poll_ex (host memory; NULL = not wanted).  Row i belongs to frame i of the call. */
typedef struct wifirx_poll_out {
    wifirx_frame* frames;       /* [cap], required */
    uint8_t*      psdu;         /* [cap][psdu_stride] */
    uint32_t      psdu_stride;
    uint32_t      reserved;
    uint8_t*      idx;          /* [cap][max_sym][48] */
    float*        carrier;      /* [cap][max_sym][48][2], handles created with want_carrier */
    float*        csi;          /* [cap][52][2] */
    float*        sym_stats;    /* [cap][4], see wifirx_out */
} wifirx_poll_out;

typedef struct wifirx_stats {
    uint64_t samples_in;     /* samples consumed */
    uint64_t frames_detected;
    uint64_t frames_signal_ok;
    uint64_t frames_complete;
    uint64_t frames_crc_ok;
    uint64_t frames_dropped; /* detected but not delivered (sync / SIGNAL / truncation / CRC) */
} wifirx_stats;

/* lifetime ------------------------------------------------------------------------------------ */
int  wifirx_create(const wifirx_config* cfg, wifirx_handle** out);
int  wifirx_destroy(wifirx_handle* h);
const char* wifirx_last_error(const wifirx_handle* h);      /* never NULL */
int  wifirx_abi_version(void);

/* replaces the generated set_bandwidth/set_frequency/set_chan_est/set_sensitivity setters */
int  wifirx_set_param(wifirx_handle* h, int id, double value);
int  wifirx_get_stats(const wifirx_handle* h, wifirx_stats* st);

/* Batch mode: n_slots independent slots of slot_len samples each, laid out back to back in `iq`
 * (interleaved float re,im = complex64 / GNU Radio gr_complex).  Every slot is treated as its own
 * sample stream that starts in sync_short's SEARCH state; the first frame of every slot is
 * demodulated:  autocorrelation graph + sync_short + sync_long + fft_vcc + frame_equalizer
 * (gnu_radio/IRS_AP.py:268-269,271,273,276-285).  Asynchronous on the handle's stream when all
 * buffers are on the device; call wifirx_sync() before reading results.
 * Slots of unequal length: wifirx_demod_batch_v. */
int  wifirx_demod_batch(wifirx_handle* h, const float* iq, int iq_on_device,
                        uint32_t slot_len, uint32_t n_slots, const wifirx_out* out);

/* The same over slots of unequal length (the slot_off[] form of SURVEY.md 8(b)): slot k is the samples
 * [slot_off[k], slot_off[k+1]) of `iq`; slot_off is a HOST array of n_slots + 1 non-decreasing sample offsets (the
 * library copies it to the device before the launch).  Output row k belongs to slot k; a slot may be empty. */
int  wifirx_demod_batch_v(wifirx_handle* h, const float* iq, int iq_on_device, const uint64_t* slot_off,
                          uint32_t n_slots, const wifirx_out* out);

/* decode_mac over the hard decisions of a previous wifirx_demod_batch on the same buffers
 * (ieee802_11.decode_mac, gnu_radio/IRS_AP.py:272,291-292): de-interleave, de-puncture, Viterbi
 * K=7 (133,171), descramble, CRC-32.  Sets WIFIRX_F_DECODED / WIFIRX_F_CRC_OK in out->frames
 * and writes out->psdu.  Input: out->hbits when given (filled by the demod call: no pass over `idx` at all), else
 * out->idx (packed into bit planes by a pre-pass).  Device buffers only (out->on_device = 1).  The call waits once for the
 * stream (a pre-pass reads back the longest trellis of the batch to size the survivor scratch);
 * the decode kernel itself is then queued asynchronously. */
int  wifirx_decode_batch(wifirx_handle* h, uint32_t n_slots, const wifirx_out* out);

/* Soft-decision decode_mac: wifirx_decode_batch with the Viterbi on the LLRs of out->llr (rows of
 * max_sym * 48 * cfg.llr_bits values in the handle's WIFIRX_P_LLR_FORMAT, as wifirx_demod_batch writes them, the buffer
 * 16-byte aligned; bf16 values are widened exactly to float32 first) instead of the hard decisions;
 * metrics, tie rule, normalisation and final state are NUMERICS.md rule 14.  It decodes the frames wifirx_decode_batch
 * would that also carry WIFIRX_F_LLR, and leaves every other record as it is; WIFIRX_F_DECODED, WIFIRX_F_CRC_OK and
 * out->psdu mean what they mean there.  WIFIRX_EINVAL when out->llr is NULL, the handle has llr_bits = 0, or the buffers
 * are not on the device.  Same waiting, scratch and allocation behaviour as wifirx_decode_batch. */
int  wifirx_decode_batch_soft(wifirx_handle* h, uint32_t n_slots, const wifirx_out* out);

/* Stream mode (what the GNU Radio block's work() calls): append `n` samples of the continuous
 * input stream (host or device memory; the library copies).  Frames that completed inside the
 * samples seen so far are demodulated + decoded and queued for wifirx_poll.
 *
 * DEVICE INPUT (iq_on_device = 1), what the call guarantees.  The samples are read by work queued on the handle's own stream,
 * wifirx_stream(h): a device-to-device copy (wifirx_push), or the widening kernel (wifirx_push_iq), into the library's sample
 * buffer.  Before the call returns WIFIRX_OK it has waited for that stream at least once behind this read -- when it only
 * collects (WIFIRX_P_STREAM_BATCH not reached) it waits for the copy, otherwise for the detection behind it -- so the caller may
 * overwrite or free the buffer as soon as the call has returned; after an error return the library reads it no more either.
 * The handle's stream is created with hipStreamNonBlocking: it is ordered against NO other stream, the legacy default stream
 * included.  Whoever produced the samples on another stream -- a kernel of the caller, a torch stream, another handle's
 * wifirx_channelize -- must therefore have finished before wifirx_push is called: wifirx_sync() on the producing handle, or
 * an event recorded on the producer's stream and waited for (by the host, or by a hipStreamWaitEvent on wifirx_stream(h)). */
int  wifirx_push(wifirx_handle* h, const float* iq, size_t n, int iq_on_device);

/* How many leading samples of the last wifirx_push call the stream has taken over: n after WIFIRX_OK; after an error
 * the count from which the caller repeats the call (0 unless the call spanned several batches).  See
 * WIFIRX_P_STREAM_BATCH, ERRORS.  GNU Radio equivalent: what work() would pass to consume_each() on an error path. */
size_t wifirx_push_consumed(const wifirx_handle* h);

/* Fetch up to `cap` queued frames (host memory).  For frame i: record frames[i], its PSDU at
 * psdu + i*psdu_stride, and -- when requested at create time and the pointers are non-NULL --
 * its hard decisions at idx + i*max_sym*48 and equalised points at carrier + i*max_sym*96 floats.
 * *n_out receives the number of frames written. */
int  wifirx_poll(wifirx_handle* h, wifirx_frame* frames, uint8_t* psdu, uint32_t psdu_stride,
                 uint8_t* idx, float* carrier, uint32_t cap, uint32_t* n_out);

/* Number of finished frames waiting for wifirx_poll*: one atomic load, no lock -- cheap enough for every work() call
 * (the block polls only when this is non-zero). */
uint32_t wifirx_queued(const wifirx_handle* h);

/* wifirx_poll that also delivers the channel state of every frame: csi + i*104 floats = the LS estimate on the 52
 * occupied sub-carriers (re, im), the `csi` entry upstream's frame_equalizer puts into the frame's tag dictionary
 * (read by ieee802_11.extract_csi, gnu_radio/IRS_AP.grc:640-654).  csi may be NULL. */
int  wifirx_poll_csi(wifirx_handle* h, wifirx_frame* frames, uint8_t* psdu, uint32_t psdu_stride,
                     uint8_t* idx, float* carrier, float* csi, uint32_t cap, uint32_t* n_out);

/* wifirx_poll with every per-frame output behind one struct (what later ABI versions extend). */
int  wifirx_poll_ex(wifirx_handle* h, const wifirx_poll_out* out, uint32_t cap, uint32_t* n_out);

/* block until everything queued on the handle's stream has finished */
int  wifirx_sync(wifirx_handle* h);

/* The HIP stream of the handle as an opaque pointer (hipStream_t), so that a caller can record
 * events / order its own work against it. */
void* wifirx_stream(wifirx_handle* h);

/* Synthetic channel on the device (test bench of gnu_radio/IRS_tranceiver.py:282-294): builds
 * n_slots slots from n_templates clean frames (host or device memory, frame_len samples each, frame
 * i uses template i % n_templates): slot = noise(unit variance, Philox counter RNG, `seed`) with
 * the frame scaled by sqrt(10^(snr_db/10)) and rotated by a per-slot CFO drawn uniformly from
 * +-cfo_max rad/sample, placed `lead` samples into the slot.  Writes `cfo_out[n_slots]` when
 * non-NULL.  Output `slots` is device memory of n_slots*slot_len complex64.  snr_db = NaN selects the
 * noiseless channel (gain 1, no AWGN; the slot outside the frame is zero). */
int  wifirx_synth_slots(wifirx_handle* h, const float* templates, int templates_on_device,
                        uint32_t n_templates, uint32_t frame_len, float* slots, uint32_t slot_len,
                        uint32_t n_slots, uint32_t lead, float snr_db, float cfo_max,
                        uint64_t seed, float* cfo_out);

/* TX half of wifi_phy_hier (mapper, SIGNAL, chunks->symbols, allocator, IFFT, cyclic prefixer;
 * gnu_radio/wifi_phy_hier.grc:279-479,570-586) for n_frames PSDUs at one encoding: the base-band frames the hier block
 * emits at `samp_out` (before IRS_user's x0.5 gain), (5 + n_sym) * 80 + 1 samples each, n_sym = ceil((16 + 8 L + 6) / N_DBPS).
 * Frame i = SERVICE (16 zero bits) + PSDU i (LSB first) + 6 tail bits + pad, scrambled (x^7 + x^4 + 1, initial state seeds[i]),
 * tail re-zeroed, (133,171)-encoded, punctured, interleaved, mapped; behind the 4 sync words and the SIGNAL symbol, with
 * pilots of polarity p_n; arithmetic = NUMERICS.md rule 16.  One kernel launch per call.
 *   psdu      frame i at psdu + i * psdu_stride (psdu_stride >= every psdu_len); device memory when psdu_on_device
 *   psdu_len  HOST [n_frames], 1..4095 bytes
 *   seeds     HOST [n_frames], 1..127; NULL = (i % 127) + 1 (the mapper's per-frame increment)
 *   samples   DEVICE complex64 (8-byte aligned), samples_cap samples long
 *   rows      row i = samples [row_off[i], row_off[i+1]) when row_off (HOST [n_frames + 1], non-decreasing) is given,
 *             [i row_len, (i+1) row_len) otherwise.  Frame i starts `lead` samples into row i; every other sample of the row
 *             is written 0.  Samples outside the rows are not touched.  Fixed rows = the slots wifirx_demod_batch reads;
 *             row_off with lead = 100 and rows of 100 + frame + 1000 = foo.packet_pad2's stream (IRS_user.py:193).
 * Checked on the host before anything is queued: WIFIRX_EINVAL for an unknown encoding, psdu_len 0 or > 4095 or above
 * psdu_stride, a seed outside 1..127, a decreasing row_off, NULL psdu / psdu_len / samples; WIFIRX_ERANGE when a frame plus
 * lead does not fit its row or the rows end behind samples_cap.  n_frames = 0 does nothing and returns WIFIRX_OK.
 * ORDER: the call waits for the handle's stream until its host inputs (psdu_len, seeds, row_off, host PSDUs) are copied, so
 * they may be reused when it returns; the kernel then runs asynchronously on the handle's stream (hipStreamNonBlocking:
 * it is not ordered against the legacy default stream).  Device PSDUs and `samples` must stay valid until it has run --
 * wifirx_sync(), or an event recorded on wifirx_stream(); later calls on the same handle are ordered behind it. */
int  wifirx_tx_batch(wifirx_handle* h, int encoding, const uint8_t* psdu, int psdu_on_device, uint32_t psdu_stride,
                     const uint32_t* psdu_len, const uint8_t* seeds, uint32_t n_frames, float* samples, uint64_t samples_cap,
                     const uint64_t* row_off, uint64_t row_len, uint32_t lead);

/* wifirx_tx_batch with one encoding per frame: frame i is built at encoding[i] -- its SIGNAL RATE field, its N_DBPS / N_CBPS,
 * its n_sym = ceil((16 + 8 L_i + 6) / N_DBPS_i) and so its length (5 + n_sym) * 80 + 1 -- as upstream's mapper applies the rate in
 * force when it handles each PDU.  Row i is, value for value, what wifirx_tx_batch writes for frame i alone at encoding[i] with
 * the same seed (NUMERICS.md rule 16 holds per frame).  One kernel launch per call.
 *   encoding  HOST [n_frames], WIFIRX_BPSK_1_2 .. WIFIRX_64QAM_3_4; it travels in the same upload as psdu_len, seeds, row_off.
 *             When all entries are equal the call is wifirx_tx_batch at that encoding (the same kernel instance).
 * Everything else -- psdu, psdu_len, seeds, samples, rows, lead, ORDER -- as wifirx_tx_batch, and so are the checks on the host
 * before anything is queued: WIFIRX_EINVAL also for NULL encoding or an entry above 7; WIFIRX_ERANGE when a frame plus lead, at
 * the frame's own encoding, does not fit its row.  n_frames = 0 does nothing and returns WIFIRX_OK. */
int  wifirx_tx_batch_rates(wifirx_handle* h, const uint8_t* encoding, const uint8_t* psdu, int psdu_on_device,
                           uint32_t psdu_stride, const uint32_t* psdu_len, const uint8_t* seeds, uint32_t n_frames,
                           float* samples, uint64_t samples_cap, const uint64_t* row_off, uint64_t row_len, uint32_t lead);

/* GNU Radio's channels.channel_model(noise_voltage, frequency_offset, epsilon = 1, taps, noise_seed), the block between TX
 * and RX of the reference's loop-back (gnu_radio/IRS_tranceiver.py:282-288), over n_rows rows of device samples; arithmetic =
 * NUMERICS.md rule 17.  Sample n of row r (x: the input row, y: the output row):
 *     s      = sum_{k=0}^{L-1} t_{r,k} x[n-k]              x[m] = 0 for m < 0: every row is its own burst
 *     y[n]   = gain * (s * exp(j phi_r(n))) + noise_voltage * w(sample0 + n, r)
 *   taps      n_tap_sets sets of n_taps (L, 1..64) complex64 taps; row r uses set r % n_tap_sets.  Device memory when
 *             taps_on_device.  One set {1} is the flat channel.
 *   cfo       HOST [n_rows] rad/sample (the unit of wifirx_synth_slots and wifirx_frame.cfo_*); NULL = 0.  The phase is fixed
 *             point: inc_r = llround(cfo_r / (2 pi) * 2^64) as a uint64, P = phase0 + inc_r n mod 2^64 (phase0 in 2^-64
 *             turns), phi = (float)(int32_t)(P >> 32) * (float)(2 pi / 2^32): a stream cut into calls keeps its phase
 *             exactly when each call passes on phase0 + inc * (samples it advanced).
 *   noise     complex Gaussian of variance noise_voltage^2 (each component noise_voltage / sqrt(2)): Philox4x32-10 keyed by
 *             `seed` on the counter ((sample0 + n) >> 1, r), Box-Muller as wifirx_synth_slots -- zero input through one flat
 *             set with gain 1, noise_voltage 1, sample0 = 0 and fixed rows of even length reproduces its noise bit for bit.
 *             noise_voltage = 0 adds nothing.
 *   in, out   DEVICE complex64 (8-byte aligned), samples_cap samples long, rows at the same places in both.  In place
 *             (in == out) only with n_taps = 1; any other overlap of the rows' samples is refused.
 *   rows      row r = samples [row_off[r], row_off[r+1]) when row_off (HOST [n_rows + 1], non-decreasing) is given,
 *             [r row_len, (r+1) row_len) otherwise: wifirx_tx_batch's convention.  Every sample of every row is written;
 *             samples outside the rows are not touched.
 * Checked on the host before anything is queued: WIFIRX_EINVAL for NULL in / out / taps, misaligned buffers, n_taps outside
 * 1..64, n_tap_sets = 0, a non-finite gain / noise_voltage / cfo, a decreasing row_off and the overlap above; WIFIRX_ERANGE
 * when the rows end behind samples_cap.  n_rows = 0 does nothing and returns WIFIRX_OK.  One kernel launch per call, after
 * one upload of the host arrays (taps, cfo, row_off).
 * ORDER: as wifirx_tx_batch -- the call waits until its host inputs are copied, so they may be reused when it returns; the
 * kernel then runs asynchronously on the handle's stream, behind the handle's earlier calls.  `in`, `out` and device taps must
 * stay valid until it has run. */
int  wifirx_channel(wifirx_handle* h, const float* in, float* out, uint64_t samples_cap,
                    const uint64_t* row_off, uint64_t row_len, uint32_t n_rows,
                    const float* taps, int taps_on_device, uint32_t n_taps, uint32_t n_tap_sets,
                    const float* cfo, uint64_t phase0, float gain, float noise_voltage,
                    uint64_t seed, uint64_t sample0);

/* wifirx_channel with channel_model's fourth argument, the sample-rate offset epsilon: a fractional resampler in front of the
 * FIR (GNU Radio's order: resampler -> taps -> mixer -> noise), in the same single launch; arithmetic = NUMERICS.md rule 18.
 * Output n of row r reads its input at the position n + D_r(n) / 2^40:
 *     u[n]   = sum_{k=0}^{31} c_k(n) x[i + k - 15]         i = n + floor(D / 2^40), c = the table's taps for frac(D / 2^40)
 *     D_r(n) = drift0 + dinc_r n                           dinc_r = llround((double)sro_r * 2^40), exact int64
 * (x[m] = 0 outside the row), and wifirx_channel's chain then runs on u; the mixer and the noise count output samples.
 *   sro       HOST [n_rows] epsilon - 1 per row (y[n] = x(n epsilon)), e.g. -20e-6f; |sro| <= 2^-8.  NULL = no resampler: the
 *             call then IS wifirx_channel (the same kernel instances, drift0 is not looked at).  A sample clock locked to
 *             the carrier, which the receiver's frame_equalizer assumes, is sro_r = -cfo_r * bw / (2 pi fc) for the cfo_r
 *             rad/sample of this call (20 ppm at 5.89 GHz and 20 MS/s: cfo = +0.037, sro = -20e-6).
 *   drift0    the drift of every row's first output sample, in 2^-40 samples: what phase0 is to the mixer.  A stream cut
 *             into calls stays exact when each call passes on drift0 + dinc * (samples it advanced) -- apart from the
 *             samples within the resampler's and the FIR's reach of the cut, which see zeros across it.
 *   in, out   as wifirx_channel, but never in place, whatever n_taps: every overlap of the rows' samples is refused.
 * All-zero sro with drift0 = 0 gives wifirx_channel's bytes on finite input (table rows 0 and 128 are unit impulses).
 * Checked on the host before anything is queued, beside wifirx_channel's checks: WIFIRX_EINVAL for an sro that is not finite
 * or above 2^-8 in magnitude, and for in == out; WIFIRX_ERANGE when |drift0| + |dinc| * (longest row) >= 2^62, |dinc| the
 * largest of the call (so every D(n), and every input position, is an exact int64).  One kernel launch per call, after one
 * upload of the host arrays (taps, cfo, row_off, the drift increments).  ORDER: as wifirx_channel. */
int  wifirx_channel_sro(wifirx_handle* h, const float* in, float* out, uint64_t samples_cap,
                        const uint64_t* row_off, uint64_t row_len, uint32_t n_rows,
                        const float* taps, int taps_on_device, uint32_t n_taps, uint32_t n_tap_sets,
                        const float* cfo, uint64_t phase0, const float* sro, int64_t drift0,
                        float gain, float noise_voltage, uint64_t seed, uint64_t sample0);

/* wifirx_channel_sro with taps that vary in time: a Doppler fader (Rayleigh, or Rician on tap 0) between the resampler and the
 * rest of wifirx_channel's chain, in the same single launch; arithmetic = NUMERICS.md rule 19.  Every tap l of row r is
 * multiplied by a gain of mean power 1, a sum of 8 sinusoids whose arrival angles and start phases are Philox draws:
 *     s[n]     = sum_{l=0}^{L-1} (g_{r,l}(n) t_{r,l}) u[n-l]      the gain at the output time n for every tap
 *     g_l      = the linear interpolation, on the 32-sample grid of t = time0 + n, of
 *     G_l(t)   = sqrt(1/8) sum_{k=0}^{7} exp(j 2 pi (phi_{l,k} + inc_{l,k} t) / 2^64),    inc = llround(fd_r cos(a_{l,k}) 2^64)
 * and with k_factor = K > 0 tap 0 is sqrt(K / (K+1)) e_los(t) + sqrt(1 / (K+1)) G_0(t), e_los one more such oscillator.
 *   doppler    HOST [n_rows] maximum Doppler shift fd_r in cycles per sample (1e-4 = 1 kHz at 10 MS/s), 0 <= fd_r <= 2^-10: the
 *              interpolation is then within sqrt(8) (2 pi fd 32)^2 / 8 = 1.4e-2 of the sinusoids (1.4e-4 at 1e-4).  fd_r = 0
 *              is not "no fading": it is one static random gain per row and tap.  NULL = no fading: the call then IS
 *              wifirx_channel_sro (the same kernel instances; k_factor, fade_seed and time0 are not looked at).
 *   k_factor   Rician K of tap 0 (power of the line of sight over the scattered power); 0 = Rayleigh on every tap.
 *   fade_seed  key of the fader's draws, on the counter (8 l + k, r, 0, 1) (the line of sight: 128): word 3 keeps them apart
 *              from the noise's, which has 0 there, so one value may serve as seed and fade_seed.
 *   time0      the stream time of every row's first output sample.  The grid lies on time0 + n, so a stream cut into calls
 *              stays exact when each call passes on time0 + (samples it advanced), apart from the FIR's n_taps - 1 samples
 *              behind the cut; any uint64 is taken, the time wraps.
 *   sro        as wifirx_channel_sro; may be NULL (no resampler) with or without fading.
 *   n_taps     1..16 with fading (the gains of a tile live in LDS beside the resampler's arrays).
 *   in, out    never in place with fading, not even with one tap: every overlap of the rows' samples is refused.
 * Checked on the host before anything is queued, beside wifirx_channel_sro's checks: WIFIRX_EINVAL for a doppler that is not
 * finite, negative or above 2^-10, for a k_factor that is not finite or negative, for n_taps > 16 with fading, and for
 * in == out with fading.  One kernel launch per call, after one upload of the host arrays (taps, cfo, row_off, the drift
 * increments, doppler).  ORDER: as wifirx_channel. */
int  wifirx_channel_fading(wifirx_handle* h, const float* in, float* out, uint64_t samples_cap,
                           const uint64_t* row_off, uint64_t row_len, uint32_t n_rows,
                           const float* taps, int taps_on_device, uint32_t n_taps, uint32_t n_tap_sets,
                           const float* cfo, uint64_t phase0, const float* sro, int64_t drift0,
                           float gain, float noise_voltage, uint64_t seed, uint64_t sample0,
                           const float* doppler, float k_factor, uint64_t fade_seed, uint64_t time0);

/* The resampler's table (NUMERICS.md rule 18; tools/gen_resample_table.py): *taps = (n_phases + 1) rows of n_taps float32,
 * row p = the fractional delay p / n_phases, tap k weighing x[i + k - 15]; n_phases = 128, n_taps = 32.  Host memory owned by
 * the library.  Needs no handle and no device; any argument may be NULL.  Returns WIFIRX_OK. */
int  wifirx_resampler_table(const float** taps, uint32_t* n_phases, uint32_t* n_taps);

/* The tap sets of a link that runs over an intelligent reflecting surface, made on the device: the cascade model of the
 * reference's utils/SV_channel.py and utils/channel.py (Channel.getChnl: H = H_B2R diag(psi) H_R2U + H_B2U) for one AP antenna,
 * one user and N = n_elems surface elements; arithmetic = NUMERICS.md rule 25.  Tap l (0 <= l < L = n_taps) of set r:
 *     a_n      = a_los A_n + a_nlos w_a(n,r,l)        b_n = a_los B_n + a_nlos w_b(n,r,l)          0 <= n < N
 *     h_d      = direct_gain (a_los D + a_nlos w_d(r,l))
 *     t_{r,l}  = s_l (h_d + sum_n a_n psi_n b_n)      s_l = (float)(sqrt(pdp_l) gain)
 * with a_los = sqrt(K / (K+1)), a_nlos = sqrt(1 / (K+1)), K = k_factor (0 = Rayleigh: a_n = w_a, b_n = w_b, h_d = direct_gain
 * w_d), and w complex Gaussians of variance 1.  The sum runs in the order of a 64-wide wave: lane i adds its elements n = i,
 * i + 64, ... in ascending n, and the 64 partial sums are folded by a butterfly over lane xor 32, 16, 8, 4, 2, 1.
 *   taps_out     DEVICE complex64 [n_sets][n_taps] (8-byte aligned): the layout wifirx_channel* reads with taps_on_device = 1,
 *                n_tap_sets = n_sets.
 *   pdp, gain    HOST float32 [n_taps], each >= 0: the power delay profile; gain scales every tap.
 *   los_b2r, los_r2u, los_b2u   HOST complex64 [N], [N], [1]: the line-of-sight vectors A, B and the scalar D (Python:
 *                wifirx.irs.los, the steering vectors of genLoS).  Not looked at when k_factor = 0; los_b2u may be NULL when
 *                direct_gain = 0.
 *   direct_gain  scales the direct path; 0 is a blocked direct path (h_d = +0, nothing of it is drawn or read).
 *   psi          align_bits = 0: complex64 [n_psi_sets][N], HOST or (psi_on_device) DEVICE; set r uses row r % n_psi_sets.  Any
 *                complex value is taken, an amplitude below 1 is a lossy element.  Not looked at when align_bits > 0.
 *   align_bits   B in {1, 2, 3}: the genie bound of a B-bit surface.  The codes are decided on tap 0 of every set and applied
 *                to all its taps: with e_n = a_{0,n} b_{0,n}, code c_n = the c in 0 .. 2^B - 1 that maximises
 *                Re(conj(h_{d,0}) e_n C_c), C_c = exp(j 2 pi c / 2^B) from a float32 table, the lowest c at a tie; with
 *                h_{d,0} = 0 the surface aligns to the positive real axis (conj(h_d) -> 1).  psi_n = C_{c_n}.
 *   scatter      NULL: the w are Philox4x32-10 draws keyed by irs_seed on the counter (n, r, l, 2) -- (x, y) -> w_a, (z, w) ->
 *                w_b by wifirx_channel's Box-Muller with h = sqrt(1/2); w_d from (x, y) of the counter (0xFFFFFFFF, r, l, 2).
 *                Word 3 keeps them apart from the noise (0) and the fader (1), so one value may serve as every seed.
 *                Else DEVICE complex64 [n_scatter][2 N + 1], each row w_a[N], w_b[N], w_d; the pair (r, l) reads row
 *                (r L + l) % n_scatter and nothing is drawn.
 *   elems_out    DEVICE complex64 [n_sets][n_taps][2][N] or NULL: the realised a_n, b_n (the surface's CSI).
 *   codes_out    DEVICE uint8 [n_sets][N] or NULL: the codes of the aligned mode.
 * Checked on the host before anything is queued: WIFIRX_EINVAL for a NULL taps_out / pdp / los_b2r / los_r2u, a NULL los_b2u
 * with direct_gain != 0, a NULL psi or n_psi_sets = 0 with align_bits = 0, n_scatter = 0 with scatter, n_elems outside 1..4096,
 * n_taps outside 1..16, align_bits > 3, codes_out with align_bits = 0, a k_factor that is not finite or negative, a pdp entry
 * that is not finite or negative, a non-finite gain / direct_gain, and misaligned pointers (device complex64: 8 bytes, host
 * float32: 4); WIFIRX_ERANGE for more than 2^31 - 1 sets.  n_sets = 0 does nothing and returns WIFIRX_OK.  One kernel launch
 * per call, after one upload of the host arrays (the line-of-sight vectors, the scales, host psi).  ORDER: as wifirx_channel. */
int  wifirx_irs_taps(wifirx_handle* h, float* taps_out, uint32_t n_sets, uint32_t n_taps, const float* pdp, float gain,
                     uint32_t n_elems, const float* los_b2r, const float* los_r2u, const float* los_b2u,
                     float k_factor, float direct_gain,
                     const float* psi, int psi_on_device, uint32_t n_psi_sets, uint32_t align_bits,
                     const float* scatter, uint32_t n_scatter, uint64_t irs_seed,
                     float* elems_out, uint8_t* codes_out);

/* Beam training of the same surface: the purpose of the reference's "IRS Traverse" block (gnu_radio/IRS_tranceiver.grc), which
 * steps the surface through a codebook of configurations and keeps the one with the best link.  For every tap set the elements
 * are drawn once and run against all K = n_codes entries; arithmetic = NUMERICS.md rule 26.  With a_n, b_n, h_d and s_l exactly
 * wifirx_irs_taps' (the same irs_seed gives the same element bits: counters (n, r, l, 2) and (0xFFFFFFFF, r, l, 2), scatter row
 * (r L + l) % n_scatter) and e_n = a_n b_n:
 *     y_{l,k}  = sum_n e_n psi_{k,n}      one fma chain per part over the 2 N floats e_0.re, e_0.im, e_1.re, ... in ascending
 *                                         order from +0, filled with zero terms up to a multiple of 4: the order in which
 *                                         consecutive v_mfma_f32_16x16x4_f32 instructions accumulate
 *     t_{l,k}  = s_l (h_d + y_{l,k})
 *     P_{r,k}  = sum_l |t_{l,k}|^2        ascending l; |t|^2 = re re + im im without fma
 *     best_r   = the k with the greatest P_{r,k}: scan k ascending from top = -1, replace on a strict >, so the lowest k wins a
 *                tie, a NaN power never wins, and all powers NaN give 0
 * The reference's block never updates its running maximum and so settles on the last entry; this call implements the stated
 * purpose.  Selection is by channel power (the measured SNR up to noise); selection from noisy estimates is not modelled.
 *   taps_out     DEVICE complex64 [n_sets][n_taps] (8-byte aligned) or NULL: the winner's taps t_{l,best}, the layout
 *                wifirx_channel* reads with taps_on_device = 1, n_tap_sets = n_sets.  Within rule 26's bound of wifirx_irs_taps
 *                with psi = codebook[best] (the same value rounded in another order).
 *   best_out     DEVICE uint16 [n_sets] (2-byte aligned) or NULL: the winning entry.
 *   power_out    DEVICE float32 [n_sets][n_codes] (4-byte aligned) or NULL: P_{r,k}.
 *   codebook     complex64 [n_codes][N], HOST or (codebook_on_device) DEVICE; 1 <= n_codes <= 1024.  Any complex value is taken
 *                (Python: wifirx.irs.dft_codebook, traverse_codebook, quantize).
 *   the other arguments   as wifirx_irs_taps, refused on the same grounds.
 * Checked on the host before anything is queued: wifirx_irs_taps' WIFIRX_EINVAL cases for the shared arguments, and WIFIRX_EINVAL
 * for a NULL codebook, n_codes outside 1..1024, all three outputs NULL, and misaligned pointers (complex64: 8 bytes, power_out
 * and the host arrays: 4, best_out: 2); WIFIRX_ERANGE for more than 2^31 - 1 sets.  n_sets = 0 does nothing and returns
 * WIFIRX_OK.  One kernel launch per call, after one upload of the host arrays.  ORDER: as wifirx_channel. */
int  wifirx_irs_sweep(wifirx_handle* h, float* taps_out, uint32_t n_sets, uint32_t n_taps, const float* pdp, float gain,
                      uint32_t n_elems, const float* los_b2r, const float* los_r2u, const float* los_b2u,
                      float k_factor, float direct_gain,
                      const float* codebook, int codebook_on_device, uint32_t n_codes,
                      const float* scatter, uint32_t n_scatter, uint64_t irs_seed,
                      uint16_t* best_out, float* power_out);

/* The same surface behind an AP of M = n_ant antennas, 1 <= M <= 8: the reference's Saleh_Valenzuela_Channel(..., antennaNum = M),
 * whose H_B2R is [M, N] and H_B2U [M] while every antenna sees ONE surface-to-user leg H_R2U; arithmetic = NUMERICS.md rule 27.
 * For antenna m < M, set r, tap l and element n, in float32 with wifirx_irs_taps' operations throughout:
 *     b_n       = mix(B_n, w_b(n,r,l))                      shared by all antennas
 *     a_{m,n}   = mix(A_{m,n}, w_a(m,n,r,l))
 *     h_{d,m}   = direct_gain * mix(D_m, w_d(m,r,l))
 *     t_{m,r,l} = s_l (h_{d,m} + sum_n (a_{m,n} psi_n) b_n)
 * mix(X, w) = a_los X + a_nlos w (k_factor = 0: w itself), s_l, the order of the sum (per antenna) and the special cases
 * k_factor = 0 and direct_gain = 0 are wifirx_irs_taps'.  Antenna 0 is wifirx_irs_taps bit for bit, and n_ant = 1 is that call.
 *   taps_out     DEVICE complex64 [n_ant][n_sets][n_taps] (8-byte aligned): antenna-major, so plane m (at taps_out +
 *                2 m n_sets n_taps floats) is what wifirx_channel* reads with taps_on_device = 1, n_tap_sets = n_sets.
 *   los_b2r, los_r2u, los_b2u   HOST complex64 [n_ant][N], [N], [n_ant]: A, B and D (Python: wifirx.irs.los(antennas=M), a
 *                half-wavelength uniform linear array along x as in genLoS).  los_b2u may be NULL when direct_gain = 0.
 *   psi          as wifirx_irs_taps: one configuration per set serves every antenna.
 *   align_bits   B in {1, 2, 3}: the genie of the reference antenna.  The codes are wifirx_irs_taps' argmax on ANTENNA 0, TAP 0
 *                (e_n = a_{0,n} b_n of tap 0, h_{d,0} of tap 0) and serve every antenna and tap of the set.  A genie for the
 *                sum of the antennas' powers has no closed form; wifirx_irs_sweep_multi trains on that sum over a codebook, and
 *                wifirx_irs_optimize ascends it from an estimate (or, at sigma = 0, from the exact coefficients).
 *   scatter      NULL: Philox4x32-10 draws keyed by irs_seed, counter word 3 = 2.  w_a(0) = words (x, y) and w_b = words (z, w)
 *                of the counter (n, r, l, 2); w_d(0) = words (x, y) of (0xFFFFFFFF, r, l, 2): wifirx_irs_taps' draws.  For
 *                m >= 1, w_a(m) comes from the counter (n, r, l + 16 ((m + 1) >> 1), 2) and w_d(m) from (0xFFFFFFFF, r,
 *                l + 16 ((m + 1) >> 1), 2): words (x, y) when m is odd, (z, w) when m is even, so one draw serves two antennas
 *                and, as l < 16, no counter meets wifirx_irs_taps'.
 *                Else DEVICE complex64 [n_scatter][(M + 1) N + M], each row w_a[0][N] .. w_a[M-1][N], w_b[N], w_d[M]; the pair
 *                (r, l) reads row (r L + l) % n_scatter.  At M = 1 this is wifirx_irs_taps' row of 2 N + 1.
 *   elems_out    DEVICE complex64 [n_sets][n_taps][n_ant + 1][N] or NULL: the realised a_0 .. a_{M-1}, then b.
 *   codes_out    DEVICE uint8 [n_sets][N] or NULL: the codes of the aligned mode.
 *   the other arguments   as wifirx_irs_taps.
 * Checked on the host before anything is queued: WIFIRX_EINVAL for n_ant outside 1..8 and for every case of wifirx_irs_taps;
 * WIFIRX_ERANGE as there.  n_sets = 0 does nothing and returns WIFIRX_OK.  One kernel launch per call, after one upload of the
 * host arrays.  ORDER: as wifirx_channel. */
int  wifirx_irs_taps_multi(wifirx_handle* h, float* taps_out, uint32_t n_ant, uint32_t n_sets, uint32_t n_taps,
                           const float* pdp, float gain, uint32_t n_elems,
                           const float* los_b2r /*[n_ant][N]*/, const float* los_r2u /*[N]*/, const float* los_b2u /*[n_ant]*/,
                           float k_factor, float direct_gain,
                           const float* psi, int psi_on_device, uint32_t n_psi_sets, uint32_t align_bits,
                           const float* scatter, uint32_t n_scatter, uint64_t irs_seed,
                           float* elems_out /*[n_sets][L][n_ant+1][N]: a_0..a_{M-1}, b*/, uint8_t* codes_out);

/* Beam training of that surface for a receiver that combines the M antennas (maximum-ratio combining, wifirx_diversity_combine):
 * arithmetic = NUMERICS.md rule 28.  The elements are wifirx_irs_taps_multi's, drawn once per (set, tap); with
 * e_{m,n} = ch_mul(a_{m,n}, b_n), row rho = m L + l and entry k:
 *     y           = wifirx_irs_sweep's chain over e_{m,0}.re, e_{m,0}.im, e_{m,1}.re, ... (zero fill to a multiple of 4, on
 *                   v_mfma_f32_16x16x4_f32, the same bits as a VALU fmaf chain)
 *     t_{m,l,k}   = s_l (h_{d,m} + y)          q = re re + im im, without fma
 *     P_{r,k}     = q_0 + q_1 + ... + q_{ML-1}  in ascending rho, starting from q_0: the channel power behind an MRC receiver
 *                   with equal noise per antenna
 *     best_r      = wifirx_irs_sweep's scan: strict >, the lowest k wins a tie, a NaN never wins
 * Per-antenna noise weights and selection-combining metrics are not offered.  At n_ant = 1 this is wifirx_irs_sweep exactly.
 *   taps_out     DEVICE complex64 [n_ant][n_sets][n_taps] (8-byte aligned) or NULL: the winner's taps t_{m,l,best}, antenna-major
 *                as wifirx_irs_taps_multi's.  Within rule 26's bound, per antenna, of wifirx_irs_taps_multi with
 *                psi = codebook[best].
 *   best_out, power_out, codebook   as wifirx_irs_sweep.
 *   the other arguments   as wifirx_irs_taps_multi.
 * Checked on the host before anything is queued: WIFIRX_EINVAL for n_ant outside 1..8 and for every case of wifirx_irs_sweep;
 * WIFIRX_ERANGE as there.  n_sets = 0 does nothing and returns WIFIRX_OK.  One kernel launch per call, after one upload of the
 * host arrays.  ORDER: as wifirx_channel. */
int  wifirx_irs_sweep_multi(wifirx_handle* h, float* taps_out, uint32_t n_ant, uint32_t n_sets, uint32_t n_taps,
                            const float* pdp, float gain, uint32_t n_elems,
                            const float* los_b2r, const float* los_r2u, const float* los_b2u,
                            float k_factor, float direct_gain,
                            const float* codebook, int codebook_on_device, uint32_t n_codes,
                            const float* scatter, uint32_t n_scatter, uint64_t irs_seed,
                            uint16_t* best_out, float* power_out);

/* The surface configured as a real controller can: from noisy channel estimates, one observation per pilot configuration.  The
 * reference's Channel.CH_est over Channel.DFT_matrix / genDFT pilots (utils/channel.py: H_est = y_rx Pilot^H / (1 + sigma2)), with
 * clustered_SV_channel's grouping of elements behind one phase; arithmetic = NUMERICS.md rule 29.  The elements a_{m,n}, b_n, the
 * direct path h_{d,m}, s_l and the cases k_factor = 0 and direct_gain = 0 are wifirx_irs_taps_multi's (the same irs_seed gives the
 * same element bits, scatter rows of (M + 1) N + M); n_ant = 1 is the surface of wifirx_irs_taps.  Rows rho = m L + l, R = M L,
 * T = n_pilots, G = n_groups, J = G + 1, e_{rho,n} = a_{m,n} b_n:
 *     x_{rho,t}    = s_l (h_{d,rho} + y)        y = wifirx_irs_sweep's chain over e.re, e.im in ascending n against
 *                                               pilot[t][group[n]]: the tap wifirx_irs_sweep_multi forms for entry t
 *     obs_{rho,t}  = x + sigma w                w of variance 1 from words (x, y) of the Philox counter (t, r, rho, 3) keyed by
 *                                               irs_seed (wifirx_channel's Box-Muller, h = sqrt(1/2)); sigma = 0: obs = x
 *     ghat_{rho,j} = kappa sum_t obs_{rho,t} conj(p_{t,j})     p_{t,0} = 1 (the direct path), p_{t,g+1} = pilot[t][g]; per part
 *                                               one fma chain from +0 over obs.re, obs.im in ascending t, filled with zero terms
 *                                               up to a multiple of 4 (v_mfma_f32_16x16x4_f32), then one multiply by kappa
 *     c_g          = wifirx_irs_taps' argmax on row 0 with the estimate: the c that maximises Re(conj(ghat_{0,0}) ghat_{0,g+1} C_c),
 *                    the lowest c wins a tie, conj(ghat_{0,0}) -> 1 when both of its parts are zero and when direct_gain = 0
 *                    (a blocked direct path has nothing to align to: the real axis, as there);  psi_n = C_{c_{group[n]}}
 *     taps         = wifirx_irs_taps_multi of the TRUE elements with that psi given, bit for bit
 * A decision that is joint over antennas and taps is wifirx_irs_optimize on est_out (below).  An estimate of noise_sigma,
 * per-antenna noise weights, pilots carried through the TX -> channel -> demod chain and more than 1023 groups are not offered.
 *   taps_out     DEVICE complex64 [n_ant][n_sets][n_taps] (8-byte aligned) or NULL: antenna-major as wifirx_irs_taps_multi's.
 *   pilot        complex64 [n_pilots][n_groups], HOST or (pilot_on_device) DEVICE; 1 <= n_pilots <= 1024, 1 <= n_groups <=
 *                min(N, 1023).  Any complex value is taken (Python: wifirx.irs.dft_pilots, hadamard_pilots).
 *   group        HOST uint16 [N], every value < n_groups: the group of element n (Python: wifirx.irs.groups); NULL is the
 *                identity and needs n_groups = N.
 *   noise_sigma  sigma >= 0.  est_scale: kappa, any finite value; 1 / T is least squares, 1 / (T + sigma^2) the reference's MMSE
 *                for coefficients of variance 1 (Python: wifirx.irs.est_scale).
 *   align_bits   B in {1, 2, 3}, or 0 when neither taps_out nor codes_out is given (nothing is decided).
 *   noise        NULL, or DEVICE complex64 [n_noise][n_pilots]: the pair (r, rho) reads row (r R + rho) % n_noise as w and
 *                nothing is drawn; sigma still scales it.
 *   est_out      DEVICE complex64 [n_sets][R][n_groups + 1] or NULL: ghat.   codes_out  DEVICE uint8 [n_sets][n_groups] or NULL.
 *   obs_out      DEVICE complex64 [n_sets][R][n_pilots] or NULL: obs.  Without it the observations live in a scratch of the handle.
 *   the other arguments   as wifirx_irs_taps_multi.
 * Checked on the host before anything is queued: WIFIRX_EINVAL for every case of wifirx_irs_taps_multi for the shared arguments, a
 * NULL pilot, n_pilots outside 1..1024, n_groups outside 1..min(N, 1023), a NULL group with n_groups != N, a group value >=
 * n_groups, a negative or non-finite noise_sigma, a non-finite est_scale, n_noise = 0 with noise, align_bits > 3, taps_out or
 * codes_out with align_bits = 0, all four outputs NULL, and misaligned pointers (complex64: 8 bytes, float32: 4, uint16: 2);
 * WIFIRX_ERANGE for more than 2^31 - 1 sets or tiles of 16 rows.  n_sets = 0 does nothing and returns WIFIRX_OK.  At most three
 * kernel launches per call, after one upload of the host arrays.  ORDER: as wifirx_channel. */
int  wifirx_irs_estimate(wifirx_handle* h, float* taps_out, uint32_t n_ant, uint32_t n_sets, uint32_t n_taps,
                         const float* pdp, float gain, uint32_t n_elems,
                         const float* los_b2r, const float* los_r2u, const float* los_b2u, float k_factor, float direct_gain,
                         const float* pilot, int pilot_on_device, uint32_t n_pilots, uint32_t n_groups, const uint16_t* group,
                         float noise_sigma, float est_scale, uint32_t align_bits,
                         const float* scatter, uint32_t n_scatter, const float* noise, uint32_t n_noise, uint64_t irs_seed,
                         float* est_out   /* [n_sets][R][n_groups+1] complex64 */, uint8_t* codes_out /* [n_sets][n_groups] */,
                         float* obs_out   /* [n_sets][R][n_pilots] complex64 */);

/* The joint phase decision over antennas and taps: cyclic coordinate ascent on the power an MRC receiver collects,
 *     P = sum_rho |d_rho + sum_g e_{rho,g} C_{c_g}|^2,
 * over the B-bit codes c_g; arithmetic = NUMERICS.md rule 30, float32 with wifirx_irs_taps' ch_mul / ch_add, no fma.  The
 * coefficients are a matrix Q [n_sets][R][J] in the layout of wifirx_irs_estimate's est_out: column 0 the direct term d_rho,
 * column g + 1 the coefficient e_{rho,g} of group g, G = J - 1, rows rho = m L + l.  Per set:
 *     start      WIFIRX_IRS_START_REF: wifirx_irs_estimate's decision, the argmax of Re(conj(Q[0][0]) Q[0][g+1] C_c) on row 0,
 *                conj(..) -> 1 when both parts are zero or direct_blocked; WIFIRX_IRS_START_GIVEN: codes_in (the low B bits of
 *                every byte); WIFIRX_IRS_START_ZERO: all codes 0
 *     state      s_rho = d_rho, then for g ascending s = ch_add(s, ch_mul(e_g, C_{c_g})); formed once, never recomputed
 *     one sweep  for g ascending: p = ch_mul(e_g, C_{c_g}), r = s - p per part, t_rho = ch_mul(conj(r_rho), e_rho); lane i of a
 *                64-wide wave forms t_i + t_{i+64} (absent rows are +0) and the 64 values are folded by wifirx_irs_taps'
 *                butterfly (lane xor 32, 16, 8, 4, 2, 1) into z; c_new = wifirx_irs_taps' argmax on Re(ch_mul(z, C_c)):
 *                ascending c, strict >, the lowest c wins a tie, a NaN never replaces the running maximum.  If c_new != c_g:
 *                s = r + ch_mul(e_g, C_{c_new}) and c_g = c_new; otherwise s stays as it was (not (s - p) + p)
 *     power      q_rho = s.re s.re + s.im s.im, the same lane pairing and butterfly; power[0] behind the state, power[i] behind
 *                sweep i
 *     stopping   a sweep that changes no code ends the call (every later sweep would repeat it bit for bit); the remaining power
 *                entries repeat the last value; sweeps_out is the number of sweeps that changed a code
 * With direct_blocked d_rho = +0 and column 0 is not read (wifirx_irs_estimate's direct_gain = 0).  max_sweeps = 0 with
 * WIFIRX_IRS_START_REF gives wifirx_irs_estimate's codes.  Per-antenna noise weights and weights over the taps are
 * wifirx_irs_optimize_weighted (below); other objectives, R > 128, random restarts and other element orders are not offered.
 *   coef         DEVICE complex64 [n_sets][n_rows][n_cols] (8-byte aligned): Q.  1 <= n_rows <= 128, 2 <= n_cols <= 1024.
 *   bits         B in {1, 2, 3}.   max_sweeps  0..16.
 *   codes_in     DEVICE uint8 [n_sets][G], required with WIFIRX_IRS_START_GIVEN and not read otherwise.
 *   n_elems, group   for psi_out: HOST uint16 [n_elems], every value < G: the group of element n; NULL is the identity and needs
 *                n_elems = G.  Without psi_out neither is looked at.
 *   codes_out    DEVICE uint8 [n_sets][G] or NULL: the final codes.
 *   psi_out      DEVICE complex64 [n_sets][n_elems] (8-byte aligned) or NULL: psi_n = C_{c_{group[n]}}, what wifirx_irs_taps_multi
 *                reads with psi_on_device = 1, n_psi_sets = n_sets.  One of codes_out and psi_out at least.
 *   power_out    DEVICE float32 [n_sets][max_sweeps + 1] (4-byte aligned) or NULL.   sweeps_out  DEVICE uint8 [n_sets] or NULL.
 * Checked on the host before anything is queued: WIFIRX_EINVAL for a NULL coef, n_rows outside 1..128, n_cols outside 2..1024,
 * bits outside 1..3, max_sweeps above 16, an unknown start, WIFIRX_IRS_START_GIVEN without codes_in, codes_out and psi_out both
 * NULL, psi_out with n_elems outside 1..4096, with a NULL group and n_elems != G, or with a group value >= G, and misaligned
 * pointers (complex64: 8 bytes, float32: 4, uint16: 2); WIFIRX_ERANGE for more than 2^31 - 1 sets.  n_sets = 0 does nothing and
 * returns WIFIRX_OK.  One kernel launch per call, after one upload of the group map (none without it).  ORDER: as wifirx_channel. */
#define WIFIRX_IRS_START_REF   0
#define WIFIRX_IRS_START_GIVEN 1
#define WIFIRX_IRS_START_ZERO  2
int  wifirx_irs_optimize(wifirx_handle* h, const float* coef /* DEVICE [n_sets][R][J] complex64 */, uint32_t n_sets,
                         uint32_t n_rows, uint32_t n_cols, uint32_t bits, uint32_t max_sweeps, int start, int direct_blocked,
                         const uint8_t* codes_in /* DEVICE [n_sets][G] or NULL */,
                         uint32_t n_elems, const uint16_t* group /* HOST [N] or NULL = identity, needs N == G */,
                         uint8_t* codes_out, float* psi_out, float* power_out /* [n_sets][max_sweeps+1] */, uint8_t* sweeps_out);

/* The joint phase decision with a real weight of either sign on every row: cyclic coordinate ascent on
 *     P_w = sum_rho w_rho |d_rho + sum_g e_{rho,g} C_{c_g}|^2;
 * arithmetic = NUMERICS.md rule 31, which is rule 30 (wifirx_irs_optimize, above) with three additions and nothing else changed.
 * Because |C_c| = 1, for one group P_w(c) = const + 2 Re(z C_c) with z = sum_rho w_rho conj(r_rho) e_rho, so every step is still
 * wifirx_irs_taps' argmax and still maximises P_w over that code exactly, for negative weights too: the ascent stays monotone
 * and the early exit stays valid.
 *     weights    w_rho float32, one per row rho = m L + l.  A row with w_rho == 0 (either sign of zero) is absent from both sums
 *                below: its term is +0, selected and not multiplied, so a non-finite coefficient in an unweighted row cannot
 *                reach a decision.  The state s_rho of such a row is still carried.
 *     z          t_rho = ch_mul(conj(r_rho), e_rho) as in rule 30, then tw_rho = (w_rho t.re, w_rho t.im): one float32 multiply
 *                per part behind the product, no fma; lane i forms tw_i + tw_{i+64} (absent rows are +0), then the butterfly
 *                (lane xor 32, 16, 8, 4, 2, 1) and the argmax, unchanged
 *     power      q_rho = s.re s.re + s.im s.im as in rule 30, then w_rho q_rho, the same lane pairing and butterfly: power_out
 *                carries P_w, which may be negative
 *     the rest   WIFIRX_IRS_START_REF stays wifirx_irs_estimate's decision on row 0, whatever w_0 is; the state update, "s stays
 *                as it was", the stopping rule and sweeps_out are rule 30's
 * Uses: w = (1, 0, .., 0) per antenna aligns tap 0 jointly over the antennas and leaves the other taps incoherent;
 * w = (1, -lambda, ..) also penalises the energy that makes the notches; w_m = 1 / sigma_m^2 are per-antenna noise weights
 * (Python: wifirx.irs.row_weights, wifirx.irs.tap_weights).  Exactly: with every weight 1.0f the outputs are
 * wifirx_irs_optimize's bit for bit (a NaN stays a NaN); with every weight the same 2^k (no overflow or underflow) the codes and
 * sweeps are wifirx_irs_optimize's and the power is 2^k times its power; rows of weight zero give the same bits whatever they
 * hold (row 0 is still read by WIFIRX_IRS_START_REF), the same bits as the call with those rows zeroed and, when they are the last
 * rows, as the call with fewer rows.  Weights estimated by the library, objectives that are not a weighted sum of row powers,
 * R > 128, random restarts and other element orders are not offered.
 *   weight       weight_on_device = 0: HOST float32 [n_rows], every value finite, n_weight_sets = 1; it is uploaded with the group
 *                map in the one upload.  Otherwise DEVICE float32 [n_weight_sets][n_rows] (4-byte aligned), n_weight_sets 1 or
 *                n_sets: set r reads row block r % n_weight_sets.  Device weights are not inspected: the arithmetic above says
 *                what a NaN weight does (w != 0 holds, the term is NaN).
 *   the other arguments   as wifirx_irs_optimize.
 * Checked on the host before anything is queued: WIFIRX_EINVAL for every case of wifirx_irs_optimize, a NULL weight,
 * n_weight_sets outside {1, n_sets} or != 1 with host weights, a non-finite host weight, a misaligned weight; WIFIRX_ERANGE for
 * more than 2^31 - 1 sets.  n_sets = 0 does nothing and returns WIFIRX_OK.  One kernel launch per call, after one upload of the
 * group map and the host weights (none without either).  ORDER: as wifirx_channel. */
int  wifirx_irs_optimize_weighted(wifirx_handle* h, const float* coef /* DEVICE [n_sets][R][J] complex64 */, uint32_t n_sets,
                                  uint32_t n_rows, uint32_t n_cols,
                                  const float* weight /* HOST [R], or DEVICE [n_weight_sets][R] */, int weight_on_device,
                                  uint32_t n_weight_sets, uint32_t bits, uint32_t max_sweeps, int start, int direct_blocked,
                                  const uint8_t* codes_in /* DEVICE [n_sets][G] or NULL */,
                                  uint32_t n_elems, const uint16_t* group /* HOST [N] or NULL = identity, needs N == G */,
                                  uint8_t* codes_out, float* psi_out, float* power_out /* [n_sets][max_sweeps+1] */,
                                  uint8_t* sweeps_out);

/* ieee802_11.mac (gnu_radio/IRS_user.py:192,204-205; IRS_tranceiver.py:271,313-314) for a batch: PSDU i, at
 * psdu + i * psdu_stride, is the 24 + payload_len[i] + 4 bytes
 *     08 00 | 00 00 | addr1 = dst | addr2 = src | addr3 = bss | ((seq0 + i) & 0xFFF) << 4, little endian | payload i | FCS
 * with FCS = CRC-32 (reflected 0xEDB88320, little endian) over everything before it.  Bytes of a row behind the PSDU are not
 * touched.  One kernel launch per call.
 *   payload      frame i at payload + i * payload_stride; device memory when payload_on_device.  NULL: the payload is made on
 *                the device -- bytes 16 j .. 16 j + 15 of frame i are the four output words (x, y, z, w, each little endian)
 *                of Philox4x32-10 on the counter (j, i, 0, 0) with the key (payload_seed & 0xffffffff, payload_seed >> 32);
 *                payload_stride then only gives the default length
 *   payload_len  HOST [n_frames], 0..1500 (WIFIRX_MAX_PSDU - 28, upstream's MAX_PAYLOAD); NULL = payload_stride for all
 *   addr         HOST [18]: dst, src, bss (addr1..3); NULL = 42.. (dst), 23.. (src), ff.. (bss), the reference's flowgraphs
 *   psdu         DEVICE
 * Checked on the host before anything is queued: WIFIRX_EINVAL for NULL psdu, a payload_len above 1500 or (with a payload
 * buffer) above payload_stride; WIFIRX_ERANGE when psdu_stride is smaller than a PSDU.  n_frames = 0 does nothing and returns
 * WIFIRX_OK.
 * ORDER: as wifirx_tx_batch -- the call waits until its host inputs (payload_len, host payloads) are copied, so they may be
 * reused when it returns; the kernel then runs asynchronously on the handle's stream, so wifirx_tx_batch(psdu_on_device = 1)
 * can follow directly.  Device payloads and `psdu` must stay valid until it has run. */
int  wifirx_mac_batch(wifirx_handle* h, const uint8_t* payload, int payload_on_device, uint32_t payload_stride,
                      const uint32_t* payload_len, uint32_t n_frames, const uint8_t* addr, uint32_t seq0,
                      uint64_t payload_seed, uint8_t* psdu, uint32_t psdu_stride);

/* What wifirx_link_stats counts.  Every counter from frames_good down counts only frames whose reference record is complete;
 * fer = 1 - frames_psdu_ok / frames_ref, coded_ber = coded_bit_errors / coded_bits. */
typedef struct wifirx_link_counts {
    uint64_t frames;               /* n_slots */
    uint64_t frames_ref;           /* reference records with WIFIRX_F_COMPLETE; only these are scored below */
    uint64_t frames_good;          /* rx COMPLETE and encoding, psdu_len, n_sym equal to the reference record's */
    uint64_t frames_crc_ok;        /* rx WIFIRX_F_CRC_OK */
    uint64_t frames_psdu_ok;       /* CRC_OK, psdu_len equal, and bytes 0 .. psdu_len - 1 equal to the reference PSDU */
    uint64_t frames_crc_ok_wrong;  /* CRC_OK and not psdu_ok */
    uint64_t coded_bits;           /* sum over good frames of n_sym * 48 * n_bpsc */
    uint64_t coded_bit_errors;     /* sum over good frames of e_f */
    uint64_t coded_bit_errors_sq;  /* sum over good frames of e_f^2 (for the standard error of the mean BER) */
} wifirx_link_counts;              /* 72 bytes */

/* Scores a decoded batch against what was sent, on the device: the back end of the loop-back (what a host would do with the
 * records, PSDUs and decisions of gnu_radio/IRS_tranceiver.py's RX side).  `rx` is what wifirx_demod_batch +
 * wifirx_decode_batch[_soft] left; `ref` describes what was sent, in the same struct: ref->frames (required: e.g. the records
 * of a demod of the clean TX rows), ref->psdu / ref->psdu_stride (the transmitted PSDUs, e.g. wifirx_mac_batch's output) and
 * ref->hbits or ref->idx (the transmitted decisions).  Both are device buffers with the row layout of this handle (max_sym
 * of its config; the psdu strides may differ); idx / hbits 16-byte aligned.  Of `rx` and `ref` only frames, psdu,
 * psdu_stride, idx, hbits and on_device are read.
 *   PSDUs      when rx->psdu or ref->psdu is NULL, frames_crc_ok, frames_psdu_ok and frames_crc_ok_wrong stay 0 (and bits 1, 2
 *              of frame_class).  A frame whose psdu_len exceeds one of the strides is not psdu_ok.
 *   decisions  e_f = the differing coded bits of frame f over its n_sym data symbols: from hbits (popcount of the XOR of the
 *              first 2 * n_bpsc * n_sym words) when both sides give hbits, else from idx (popcount of the XOR of the 48 * n_sym
 *              bytes) when both give idx; the two forms give the same number.  With neither, coded_bits, coded_bit_errors and
 *              coded_bit_errors_sq stay 0 and frame_err is 0xFFFFFFFF throughout.  n_bpsc is that of the record's encoding; a
 *              record with an encoding above 7 or n_sym above max_sym is not good.
 *   frame_err  DEVICE [n_slots], optional: e_f for good frames, 0xFFFFFFFF otherwise
 *   frame_class DEVICE [n_slots], optional: bit 0 good, bit 1 crc_ok, bit 2 psdu_ok, bit 3 reference complete
 *   counts     HOST
 * All sums are integers: the result does not depend on the order of reduction.  WIFIRX_EINVAL for NULL rx / ref / counts /
 * rx->frames / ref->frames, host buffers (on_device = 0) or misaligned idx / hbits / frame_err.
 * ORDER: the call zeroes a small device buffer of the handle, runs one kernel behind the handle's earlier calls, copies the
 * 72 bytes back and WAITS for them: when it returns, everything queued on the handle's stream before it has finished. */
int  wifirx_link_stats(wifirx_handle* h, uint32_t n_slots, const wifirx_out* rx, const wifirx_out* ref,
                       uint32_t* frame_err, uint8_t* frame_class, wifirx_link_counts* counts);

/* wifirx_link_stats with the counters split by rate: for a batch that mixes encodings (wifirx_tx_batch_rates).  Same inputs,
 * same per-frame rules, same checks and ORDER (one kernel, one zeroing, one copy back of 9 * 72 bytes).
 *   total     HOST, may be NULL: exactly what wifirx_link_stats returns in `counts`
 *   by_rate   HOST [8]: by_rate[e] counts the slots whose REFERENCE record is WIFIRX_F_COMPLETE with encoding == e, so in it
 *             frames == frames_ref.  A slot whose reference record is not complete lands in no rate.
 * For every counter X except frames: sum over e of by_rate[e].X == total.X; sum over e of by_rate[e].frames == total.frames_ref.
 * WIFIRX_EINVAL also for NULL by_rate. */
int  wifirx_link_stats_by_rate(wifirx_handle* h, uint32_t n_slots, const wifirx_out* rx, const wifirx_out* ref,
                               uint32_t* frame_err, uint8_t* frame_class, wifirx_link_counts* total,
                               wifirx_link_counts* by_rate);

/* Sample formats of the radios (NUMERICS.md rule 20).  The library computes in WIFIRX_IQ_FC32, interleaved float32 (re, im);
 * the integer formats are what a USRP (sc16: int16 I, int16 Q, native endian -- UHD's wire and file format) and a HackRF
 * (sc8: int8 I, int8 Q -- what hackrf_transfer writes) deliver.
 *   widen     each component is (float)q * scale, one float32 multiply of the exactly converted integer; `scale` is a finite
 *             float32 > 0, by convention 2^-15 (sc16) and 2^-7 (sc8); exact whenever scale is a power of two
 *   quantise  to `bits` bits inside the container (2..16 for sc16, 2..8 for sc8), per component: t = x * scale (one float32
 *             multiply), r = rintf(t) (ties to even), lo = -2^(bits-1), hi = 2^(bits-1) - 1, q = r < lo ? lo : r > hi ? hi :
 *             (int)r; NaN gives 0, +-inf saturate.  A component is CLIPPED when it was NaN or r lay outside [lo, hi]. */
#define WIFIRX_IQ_FC32 0
#define WIFIRX_IQ_SC16 1
#define WIFIRX_IQ_SC8  2

/* Widen n samples of `fmt` (WIFIRX_IQ_SC16 / WIFIRX_IQ_SC8) at src into float pairs at dst.  DEVICE buffers: src at its natural
 * alignment (4 bytes sc16, 2 bytes sc8), dst 8-byte aligned; n * 4 or n * 2 bytes are read, n * 8 written.  What the batch
 * calls take a recording through: wifirx_iq_to_f32 into the float buffer wifirx_demod_batch reads.
 * Checked on the host before anything is queued: WIFIRX_EINVAL for NULL src / dst, an unknown format or WIFIRX_IQ_FC32 (there
 * is nothing to convert), a scale that is not finite or <= 0, misaligned buffers, and any overlap of the source and
 * destination bytes.  n = 0 does nothing and returns WIFIRX_OK.  One kernel launch per call.
 * ORDER: as wifirx_channel -- the kernel runs asynchronously on the handle's stream, behind the handle's earlier calls; src and
 * dst must stay valid until it has run (wifirx_sync(), or an event recorded on wifirx_stream()). */
int  wifirx_iq_to_f32(wifirx_handle* h, const void* src, int fmt, uint64_t n, float scale, float* dst);

/* Quantise n float pairs at src to `bits` bits in samples of `fmt` at dst: the converter in front of a receiver (the loop-back
 * runs it between wifirx_channel and the demod, then widens again).  DEVICE buffers, aligned as above.
 *   clipped   HOST, may be NULL: the number of clipped components of the call, I and Q each counted on their own (0 .. 2 n).
 * Checked on the host before anything is queued: wifirx_iq_to_f32's checks, and WIFIRX_EINVAL for bits outside 2..16 (sc16) /
 * 2..8 (sc8).  n = 0 does nothing and returns WIFIRX_OK (*clipped = 0).  One kernel launch per call.
 * ORDER: with clipped == NULL as wifirx_iq_to_f32: nothing is counted and nothing waits.  With clipped != NULL as
 * wifirx_link_stats: the call zeroes a small device counter of the handle, runs the kernel behind the handle's earlier calls,
 * copies the 8 bytes back and WAITS for them. */
int  wifirx_iq_from_f32(wifirx_handle* h, const float* src, uint64_t n, float scale, int fmt, uint32_t bits,
                        void* dst, uint64_t* clipped);

/* wifirx_push for a stream whose samples arrive in `fmt`: n samples (not bytes) at iq, host or device memory, at the format's
 * natural alignment.  The stream it produces is, byte for byte in every record and output, the stream wifirx_push produces
 * from the rule-20 widened samples.  WIFIRX_IQ_FC32 IS wifirx_push (the same code path; scale is not looked at).
 * Host input with WIFIRX_P_STREAM_BATCH is staged and crosses the bus in its native format (a half or a quarter of the float32
 * bytes) and is widened on the device, into the stream's sample buffer; device input is widened straight from the caller's buffer.
 * Formats and scales may alternate freely between pushes: a push whose format or scale differs from that of samples still
 * staged first runs those samples as a (short) batch, the rule a change of WIFIRX_P_STREAM_BATCH follows.  n = 0 flushes.
 * wifirx_push_consumed, the ERRORS contract of WIFIRX_P_STREAM_BATCH, WIFIRX_EDEAD and wifirx_stats.samples_in keep their
 * meaning, in samples.  WIFIRX_EINVAL, with wifirx_push_consumed() = 0 and the stream untouched, for an unknown format, a scale
 * that is not finite or <= 0 (integer formats), NULL iq with n > 0, or a misaligned iq. */
int  wifirx_push_iq(wifirx_handle* h, const void* iq, size_t n, int fmt, float scale, int iq_on_device);

/* Wideband ingest (NUMERICS.md rule 21): split one stream sampled at M * fs, M = n_channels in {2, 4, 8} adjacent channels of
 * width fs, into M streams at fs -- a critically sampled polyphase analysis bank, 24 taps per branch, on the device.  Channel k
 * (0 .. M-1) is centred at f_k = (k + stacking/2 - M/2) / M cycles per input sample: stacking = 1 puts the centres at -+fs/2,
 * -+3fs/2, ... around the tuned frequency (four 5 GHz channels around their common centre), stacking = 0 at k * fs - M/2 * fs
 * (channel 0 then straddles the band edge; it is still produced).  With z_k[n] = x[n] exp(-j 2 pi f_k n), n the stream's input
 * index, and h the prototype of wifirx_channelizer_table:  y_k[m] = sum_{i < 24 M} h[i] z_k[m M + M - 1 - i].
 * n_out outputs per channel consume exactly n_out * M input samples.
 *   in          DEVICE, n_out * M samples of `fmt` (WIFIRX_IQ_FC32 / SC16 / SC8) at the format's natural alignment (8 / 4 / 2
 *               bytes).  Integer samples are widened by rule 20 with `scale` inside the kernel; for FC32 scale is not looked at.
 *   hist        DEVICE, the 23 * M samples in front of in[0], same format; NULL = zeros (the start of a stream).
 *   hist_out    DEVICE, may be NULL: receives the last 23 * M samples of (hist || in), in the input format, by copies queued
 *               behind the kernel.  Passed on as the next call's hist, with m0 + n_out, it makes a stream cut into calls
 *               byte-identical to the uncut one from the first output on.  It must not overlap hist, in or out: a caller
 *               alternates between two buffers.
 *   m0          the stream index of the call's first output (its parity enters for stacking = 1).
 *   out         DEVICE, 8-byte aligned float pairs: channel k occupies out + 2 * k * out_stride floats, n_out samples; nothing
 *               else is written.  Each row is what wifirx_push(iq_on_device = 1) of channel k's handle takes.
 * Checked on the host before anything is queued: WIFIRX_EINVAL for NULL in / out with n_out > 0, an unknown fmt, a scale that
 * is not finite or <= 0 (integer formats), n_channels outside {2, 4, 8}, stacking outside {0, 1}, misaligned buffers, and any
 * overlap among in, hist, hist_out and the M rows of out (taken as one range, first row to last); WIFIRX_ERANGE for
 * out_stride < n_out, out_stride > 2^44 or n_out > 2^40.  n_out = 0 returns WIFIRX_OK and still produces hist_out (= hist, or
 * zeros) when asked.  One kernel launch per call, and at most two copies for hist_out.
 * ORDER: as wifirx_iq_to_f32 -- asynchronous on the handle's stream, behind the handle's earlier calls; every buffer must stay
 * valid until the work has run.  The rows are usually consumed by OTHER handles, each on its own stream: see wifirx_push,
 * DEVICE INPUT -- wifirx_sync() on this handle (or an event on wifirx_stream()) comes between this call and their pushes. */
int  wifirx_channelize(wifirx_handle* h, const void* in, int fmt, float scale, const void* hist, void* hist_out,
                       uint32_t n_channels, int stacking, uint64_t n_out, uint64_t m0, float* out, uint64_t out_stride);

/* The bank's prototype (NUMERICS.md rule 21; tools/gen_channelizer_table.py): *taps = the 24 * n_channels float32 taps h for
 * n_channels in {2, 4, 8}, symmetric, sum 1; *n_taps = their number.  Host memory owned by the library.  Needs no handle and
 * no device.  WIFIRX_EINVAL for another n_channels or a NULL argument. */
int  wifirx_channelizer_table(uint32_t n_channels, const float** taps, uint32_t* n_taps);

/* Wideband transmit (NUMERICS.md rule 22): join M = n_channels in {2, 4, 8} streams at fs, one per adjacent channel of width
 * fs, into one stream sampled at M * fs -- the critically sampled polyphase synthesis bank that mirrors wifirx_channelize, 24
 * taps per branch, on the device (GNU Radio's pfb_synthesizer_ccf).  Stream k lands at wifirx_channelize's centre
 * f_k = (k + stacking/2 - M/2) / M cycles per output sample.  With h the prototype of wifirx_channelizer_table and n the
 * stream's output index:  x[n] = sum_k g_k exp(j 2 pi f_k n) sum_m u_k[m] M h[n - m M].  Amplitudes are kept (a unit-power
 * stream gives unit power in its channel); the filter delays by (24 M - 1) / 2 output samples, and through
 * wifirx_channelize every stream comes back delayed by exactly 23 channel samples.  n_in samples per channel give exactly
 * n_in * M output samples.
 *   in          DEVICE, 8-byte aligned float pairs: channel k's n_in samples start at in + 2 * k * in_stride floats -- the layout
 *               of wifirx_channelize's out, and of M wifirx_tx_batch sample buffers laid side by side.
 *   gains       HOST, M finite floats g_k (one real multiply per component), or NULL for no multiply.  They travel as kernel
 *               arguments: nothing is uploaded, and the array may be reused as soon as the call returns.
 *   hist        DEVICE, M rows of 23 float pairs, row k at hist + 2 * 23 * k floats: the 23 samples of every channel in front
 *               of in; NULL = zeros (the start of a stream).
 *   hist_out    DEVICE, may be NULL: receives the last 23 samples of (hist || in) of every channel, same layout, by a copy
 *               queued behind the kernel.  Passed on as the next call's hist, with m0 + n_in, it makes a stream cut into calls
 *               byte-identical to the uncut one.  It must not overlap hist, in or out: a caller alternates between two buffers.
 *   m0          the stream index of the call's first input sample (its parity enters for stacking = 1).
 *   out         DEVICE, 8-byte aligned, n_in * M float pairs; nothing else is written.
 * Checked on the host before anything is queued: WIFIRX_EINVAL for NULL in / out with n_in > 0, n_channels outside {2, 4, 8},
 * stacking outside {0, 1}, a gain that is not finite, misaligned buffers, and any overlap among the M rows of in (taken as
 * one range, first row to last), hist, hist_out and out; WIFIRX_ERANGE for in_stride < n_in, in_stride > 2^44 or
 * n_in > 2^40.  n_in = 0 returns WIFIRX_OK and still produces hist_out (= hist, or zeros) when asked.  One kernel launch per
 * call, and one small copy kernel for hist_out.
 * ORDER: as wifirx_iq_to_f32 -- asynchronous on the handle's stream, behind the handle's earlier calls; every buffer must stay
 * valid until the work has run.  The rows are usually produced by OTHER handles (wifirx_tx_batch, wifirx_channel), each on its
 * own stream, and out may be consumed by another: wifirx_sync() on the producing handle (or an event on wifirx_stream())
 * comes between their calls and this one, and between this one and the consumer's. */
int  wifirx_combine(wifirx_handle* h, const float* in, uint64_t in_stride, const float* gains, const float* hist,
                    float* hist_out, uint32_t n_channels, int stacking, uint64_t n_in, uint64_t m0, float* out);

/* Receive resampler (NUMERICS.md rule 34): one stream sampled at fs_in into one sampled at fs_out = fs_in * den / num, on the
 * device -- a capture at 25, 30.72, 40, 61.44 or 100 MS/s into the 20 MS/s that wifirx_push takes, a 61.44 MS/s capture into
 * the 80 MS/s of wifirx_channelize, or a transmit stream into a converter's rate (GNU Radio's rational_resampler /
 * pfb_arb_resampler_ccf in front of wifi_phy_hier).  num / den = fs_in / fs_out is the step in input samples per output
 * sample; the call divides both by their gcd first (10/8 and 5/4 give the same bytes), and the reduced ratio must satisfy
 * 1 <= den <= 512, 1 <= num <= 2048, num <= 4 den and den <= 4 num.  With S = max(num, den), h the prototype of
 * wifirx_arb_table (a Kaiser-windowed sinc of cutoff 1/2 in units of the slower rate, 32 units long), m the stream's output
 * index and j its input index:  y[m] = g sum_j h((m num - j den) / S) x[j],  g = den / S for num > den and 1 otherwise.
 * There is no delay: output m is the input at time m num / den, and it reads the inputs jlo(m) = floor((m num - 16 S) / den) + 1
 * .. jhi(m) = floor((m num + 16 S) / den); x[j] = 0 for j < 0.  With the inputs [0, E) present the outputs m < m_end(E) =
 * max(0, ceil((E den - 16 S) / num)) can be made, so the last ceil(16 S / den) input instants of a stream appear only after
 * that many more samples: a caller ends a stream by pushing zeros.
 *   in          DEVICE, n_in samples of `fmt` (WIFIRX_IQ_FC32 / SC16 / SC8) at the format's natural alignment (8 / 4 / 2
 *               bytes); in[0] is stream sample j0.  Integer samples are widened by rule 20 with `scale` inside the kernel;
 *               for FC32 scale is not looked at.
 *   hist        DEVICE, the HL = wifirx_arb_hist(num, den) samples in front of in[0], same format; NULL = zeros (the start of
 *               a stream).
 *   hist_out    DEVICE, may be NULL: receives the last HL samples of (hist || in), in the input format, by copies queued
 *               behind the kernel.  A caller that passes on j0 + n_in, m0 + *n_out and hist_out gets a stream that is
 *               byte-identical to the uncut one, wherever it is cut.  It must not overlap hist, in or out: a caller
 *               alternates between two buffers.
 *   j0, m0      the stream indices of in[0] and of the call's first output.
 *   out         DEVICE, 8-byte aligned, room for out_cap float pairs; the outputs m0 .. m_end(j0 + n_in) - 1 are written and
 *               nothing else.  It is what wifirx_push(iq_on_device = 1) takes.
 *   n_out       HOST, required: the number of outputs, the value wifirx_arb_count gives; filled before anything is queued.
 * Checked on the host before anything is queued: WIFIRX_EINVAL for NULL in with n_in > 0, NULL out with outputs to make, NULL
 * n_out, an unknown fmt, a scale that is not finite or <= 0 (integer formats), num or den of 0 or a reduced ratio outside
 * the limits, misaligned buffers, any overlap among in, hist, hist_out and out, and a history that does not reach
 * (jlo(m0) < j0 - HL with outputs to make); WIFIRX_ERANGE for n_out > out_cap, (j0 + n_in) * den >= 2^62 or
 * (m0 + n_out) * num >= 2^62.  A refused call writes nothing, *n_out included.  n_in = 0 returns WIFIRX_OK, makes no output
 * and still produces hist_out (= hist, or zeros) when asked.  One kernel launch per call, and at most two copies for hist_out.
 * ORDER: as wifirx_iq_to_f32 -- asynchronous on the handle's stream, behind the handle's earlier calls; every buffer must stay
 * valid until the work has run.  The output is usually consumed by ANOTHER handle on its own stream: see wifirx_push,
 * DEVICE INPUT -- wifirx_sync() on this handle (or an event on wifirx_stream()) comes between this call and its push. */
#define WIFIRX_ARB_HIST_MAX 128
int  wifirx_arb_resample(wifirx_handle* h, const void* in, int fmt, float scale, uint64_t n_in, const void* hist,
                         void* hist_out, uint32_t num, uint32_t den, uint64_t j0, uint64_t m0, float* out, uint64_t out_cap,
                         uint64_t* n_out);

/* HL = ceil(32 S / den) <= WIFIRX_ARB_HIST_MAX of the reduced ratio: the samples wifirx_arb_resample takes as hist and hands
 * on as hist_out.  Needs no handle and no device.  WIFIRX_EINVAL for a ratio outside the limits or a NULL hist_len. */
int  wifirx_arb_hist(uint32_t num, uint32_t den, uint32_t* hist_len);

/* The outputs of a wifirx_arb_resample call with the same arguments: *n_out = max(0, m_end(j0 + n_in) - m0), host integers
 * only.  WIFIRX_EINVAL for a ratio outside the limits or a NULL n_out, WIFIRX_ERANGE as wifirx_arb_resample. */
int  wifirx_arb_count(uint32_t num, uint32_t den, uint64_t j0, uint64_t n_in, uint64_t m0, uint64_t* n_out);

/* The resampler's prototype (NUMERICS.md rule 34; tools/gen_arb_table.py): *table = the *n_entries = 4097 float32 values
 * h(-16 + q / 128), *per_unit = 128 entries per unit of the slower rate.  Host memory owned by the library.  Needs no handle
 * and no device.  WIFIRX_EINVAL for a NULL argument. */
int  wifirx_arb_table(const float** table, uint32_t* n_entries, uint32_t* per_unit);

/* Tuner (NUMERICS.md rule 35): n_channels = 1 .. 8 channels at any centre out of ONE capture, on the device -- channels 1 / 6 /
 * 11 of the 2.4 GHz band (25 MHz apart) out of an 80 MS/s capture around 2437 MHz, which no M x 20 MHz bank can split (GNU
 * Radio's freq_xlating_fir_filter, or rotator + rational_resampler, per channel in front of wifi_phy_hier).  Channel k is the
 * capture multiplied by exp(j 2 pi P_k(j) / 2^64), P_k(j) = phase0[k] + inc[k] * j mod 2^64 at STREAM index j (rule 17's
 * fixed-point mixer: the angle is the float32 of the top 32 bits of P, sine and cosine by rule 1, the product in plain
 * float32), and then resampled exactly as wifirx_arb_resample does: the same ratio, prototype, sum, gain and counting
 * (wifirx_arb_count, wifirx_arb_hist).  Every sample the sum reads is rotated first, the zeros in front of the stream and
 * of a NULL hist included, so a NULL hist and a hist of zeros give the same bytes.  The phase depends on the stream index
 * alone: a stream cut anywhere is byte-identical to the uncut one with nothing more than j0, m0 and hist_out passed on, and
 * hist / hist_out hold RAW input samples as in wifirx_arb_resample.  A channel with inc[k] == 0 and phase0[k] == 0 is not
 * rotated at all: its row holds the bytes of wifirx_arb_resample.
 * THE FILTER is wifirx_arb_resample's prototype and nothing sharper: a tuned centre must keep |offset| + 8.3 MHz inside
 * fs_in / 2, or the channel itself aliases, and what lies more than (1 - 26.5/64) * 20 MHz = 11.7 MHz from the tuned centre
 * is down by 69 dB (for fs_out = 20 MS/s).  25 MHz in a 61.44 MS/s capture aliases (25 + 8.3 > 30.72: the radio's filters
 * have removed the channel's upper edge, or folded something else onto it, before the samples exist); in 80 MS/s it does not.
 *   in, fmt, scale, n_in, hist, hist_out, num, den, j0, m0      as wifirx_arb_resample
 *   n_channels  1 .. WIFIRX_TUNE_MAX_CHANNELS
 *   inc         HOST [n_channels], required: the phase increments per input sample in 2^-64 turns (wifirx_tune_inc); read
 *               before the call returns
 *   phase0      HOST [n_channels], the phases of stream sample 0; NULL = zeros; read before the call returns
 *   out         DEVICE, 8-byte aligned: row k starts at out + 2 * k * out_stride floats; of each row the outputs
 *               m0 .. m_end(j0 + n_in) - 1 are written and nothing else.  A row is what wifirx_push(iq_on_device = 1) takes.
 *   out_stride  float pairs from one row to the next, >= n_out
 *   n_out       HOST, required: the outputs PER CHANNEL, the value wifirx_arb_count gives
 * Checked on the host before anything is queued: everything wifirx_arb_resample checks, with out_stride in out_cap's place and
 * the n_channels * out_stride * 8 bytes of out as the output buffer; WIFIRX_EINVAL also for n_channels of 0 or above 8 and a
 * NULL inc; WIFIRX_ERANGE also for out_stride < n_out (whatever n_channels is), for out_stride >= 2^56 (8 rows of it stay
 * below 2^62 bytes), and for more than 2^31 - 1 tiles of 256 outputs.  A refused call writes nothing, *n_out included.  One kernel launch per call, and at most two copies
 * for hist_out.
 * ORDER: as wifirx_arb_resample. */
#define WIFIRX_TUNE_MAX_CHANNELS 8
int  wifirx_tune(wifirx_handle* h, const void* in, int fmt, float scale, uint64_t n_in, const void* hist, void* hist_out,
                 uint32_t num, uint32_t den, uint32_t n_channels, const uint64_t* inc, const uint64_t* phase0, uint64_t j0,
                 uint64_t m0, float* out, uint64_t out_stride, uint64_t* n_out);

/* The increment that brings a channel whose centre lies offset_hz ABOVE the capture's centre down to 0: t = offset_hz /
 * sample_rate in double, reduced to [-1/2, 1/2] by subtracting its nearest integer, *inc = (uint64_t)(-llround(t * 2^64));
 * +-1/2 turn gives 2^63 (rule 17's phase increment without the 2 pi).  +25 MHz in 80 MS/s gives 0xB000000000000000.  Needs no
 * handle and no device.  WIFIRX_EINVAL for a NULL inc, a sample_rate that is not finite or <= 0, an offset_hz that is not
 * finite. */
int  wifirx_tune_inc(double offset_hz, double sample_rate, uint64_t* inc);

/* Band survey (NUMERICS.md rule 36): what is in a capture, before anything is tuned to.  Windowed-FFT power rows of a stream in
 * its native format (the numbers behind a spectrum display and a waterfall), the fold of rows into fewer rows, and the power of
 * each candidate channel per row.  The reference's flowgraphs show the same of the receiver's stream with
 * qtgui.sink_c(1024, window.WIN_BLACKMAN_hARRIS, ...).
 *
 * wifirx_spectrum: segment s is in[s * hop .. s * hop + n_fft - 1]; S = (n_in >= n_fft) ? (n_in - n_fft) / hop + 1 : 0 segments.
 * Row r is the fold (WIFIRX_SPEC_SUM: sum, WIFIRX_SPEC_MAX: maximum, a NaN sticks) of the powers |FFT(w * segment)|^2 of segments
 * r * avg .. r * avg + avg - 1, times norm; bin i of a row is the frequency (i - n_fft / 2) / n_fft cycles per sample.  Only
 * complete rows are made: *n_rows = S / avg, and the next row's first segment starts at sample *n_rows * avg * hop
 * (wifirx_spectrum_count's consumed): a caller that cuts a stream there and keeps the overlap gets byte-identical rows.
 *   in          DEVICE, n_in samples of `fmt` (WIFIRX_IQ_FC32 / SC16 / SC8) at the format's natural alignment (8 / 4 / 2
 *               bytes); scale widens the integer formats (rule 20; not looked at for fc32)
 *   n_fft       64, 256, 1024 or 4096;  hop, avg  1 .. WIFIRX_SPEC_MAX_HOP;  window  WIFIRX_SPEC_RECT / HANN / BLACKMAN_HARRIS
 *               (periodic forms);  norm  any float32 (1: the fold itself)
 *   rows_out    DEVICE, 4-byte aligned, room for rows_cap rows of n_fft floats; exactly *n_rows rows are written
 * Checked on the host before anything is queued, and before a device is looked for: WIFIRX_EINVAL for a NULL handle or n_rows,
 * NULL in with n_in > 0, NULL rows_out with rows to make, an unknown fmt, window or mode, a scale that is not finite or <= 0,
 * an n_fft outside the set, hop or avg of 0 or above 2^20, misaligned buffers, an overlap of in and the rows written;
 * WIFIRX_ERANGE for rows_cap < *n_rows, n_in >= 2^62, more than 2^31 - 1 tiles.  A refused call writes nothing, *n_rows
 * included.  n_in < n_fft, or fewer than avg segments, returns WIFIRX_OK with *n_rows = 0 and writes nothing else.  One kernel
 * launch per call.  ORDER: as wifirx_arb_resample. */
#define WIFIRX_SPEC_RECT 0
#define WIFIRX_SPEC_HANN 1
#define WIFIRX_SPEC_BLACKMAN_HARRIS 2
#define WIFIRX_SPEC_SUM 0
#define WIFIRX_SPEC_MAX 1
#define WIFIRX_SPEC_MAX_BANDS 16
#define WIFIRX_SPEC_MAX_HOP 1048576        /* 2^20: the largest hop and the largest avg */
int  wifirx_spectrum(wifirx_handle* h, const void* in, int fmt, float scale, uint64_t n_in, uint32_t n_fft, uint32_t hop,
                     uint32_t avg, int window, int mode, float norm, float* rows_out, uint64_t rows_cap, uint64_t* n_rows);

/* The rows a wifirx_spectrum call makes and the samples they consume (*consumed = *n_rows * avg * hop), host integers only; needs
 * no handle and no device.  WIFIRX_EINVAL for a NULL output or arguments wifirx_spectrum refuses, WIFIRX_ERANGE for
 * n_in >= 2^62.  Nothing is written by a refused call. */
int  wifirx_spectrum_count(uint32_t n_fft, uint32_t hop, uint32_t avg, uint64_t n_in, uint64_t* n_rows, uint64_t* consumed);

/* Output row q = the ascending fold, by wifirx_spectrum's two modes, of rows q * group .. q * group + group - 1, per bin;
 * *n_out = n_rows / group complete groups.  A Welch spectrum of a whole capture is wifirx_spectrum(avg <= 64) followed by
 * wifirx_spectrum_fold(group = n_rows).  rows, out: DEVICE, 4-byte aligned, [..][n_fft]; they must not overlap.
 * WIFIRX_EINVAL for a NULL handle, n_out, rows or out with rows to make, an n_fft outside the set, an unknown mode, group = 0,
 * misaligned or overlapping buffers; WIFIRX_ERANGE for out_cap < *n_out or n_rows >= 2^40.  One kernel launch per call. */
int  wifirx_spectrum_fold(wifirx_handle* h, const float* rows, uint64_t n_rows, uint32_t n_fft, uint64_t group, int mode,
                          float* out, uint64_t out_cap, uint64_t* n_out);

/* out[r][b] = the sum of row r's bins lo[b] .. hi[b] - 1: one wave per (row, band), lane l adding bins lo + l, lo + l + 64, ..
 * in ascending order, then the xor-butterfly tree of rule 5 over the 64 lanes.  rows, out: DEVICE, 4-byte aligned; lo, hi: HOST
 * [n_bands], read before the call returns.  Bands may overlap one another.
 * WIFIRX_EINVAL for a NULL handle, rows, out, lo or hi, n_bands outside 1 .. WIFIRX_SPEC_MAX_BANDS, an n_fft outside the set,
 * lo[b] >= hi[b] or hi[b] > n_fft, misaligned or overlapping buffers; WIFIRX_ERANGE for n_rows > 2^31 - 1.  n_rows = 0 does
 * nothing and returns WIFIRX_OK.  One kernel launch per call. */
int  wifirx_spectrum_bands(wifirx_handle* h, const float* rows, uint64_t n_rows, uint32_t n_fft, uint32_t n_bands,
                           const uint32_t* lo, const uint32_t* hi, float* out);

/* The bins of a row whose centres lie in [offset_hz - width_hz / 2, offset_hz + width_hz / 2): in double,
 * *lo = ceil((offset_hz - width_hz / 2) * n_fft / sample_rate) + n_fft / 2 and *hi the same of the upper edge (rule 36).  Needs
 * no handle and no device.  WIFIRX_EINVAL for a NULL output, an n_fft outside the set, values that are not finite,
 * sample_rate <= 0, width_hz <= 0; WIFIRX_ERANGE when the band holds no bin or leaves [-sample_rate / 2, sample_rate / 2). */
int  wifirx_spectrum_band(double offset_hz, double width_hz, double sample_rate, uint32_t n_fft, uint32_t* lo, uint32_t* hi);

/* The tables of rule 36 (host memory, static): the periodic Hann and 4-term Blackman-Harris windows of *n_entries = 4096 points and
 * T[k] = exp(-j 2 pi k / 4096) as *n_entries (re, im) pairs; a transform of n_fft points reads every (4096 / n_fft)-th entry.
 * Needs no handle and no device.  WIFIRX_EINVAL for a NULL argument. */
int  wifirx_spectrum_table(const float** hann, const float** blackman_harris, const float** twiddle, uint32_t* n_entries);

/* Receive diversity (NUMERICS.md rule 23): combine the equalised points of n_ant antennas' demodulated batches into one batch
 * to decode.  Slot i of every in[a] is the same transmission, demodulated from antenna a's samples by wifirx_demod_batch with
 * `carrier` and `csi` outputs (by this handle one after the other, or by other handles with the same max_sym).  Per slot: the
 * antennas whose record has WIFIRX_F_SIGNAL and WIFIRX_F_COMPLETE are usable; the reference antenna r is the usable one with
 * the greatest snr_db (the lowest index on ties); those usable antennas whose encoding and psdu_len equal r's contribute.
 *   WIFIRX_DIV_MRC     maximal-ratio combining after equalisation: per data carrier Y = sum_a u_a Y_a with u_a = w_a / sum w,
 *                      w_a = |H_a|^2 of antenna a's LS estimate (the weight of WIFIRX_P_LLR_CSI) times ant_gain[a]; a carrier
 *                      whose weights sum to 0 or to nothing finite takes the reference antenna's point as it is
 *   WIFIRX_DIV_SELECT  selection: only r contributes -- every output is a copy of antenna r's
 *   in         HOST [n_ant], n_ant = 1 .. 8; of in[a] only frames, carrier, csi and on_device are read: DEVICE buffers,
 *              16-byte aligned, in the row layout of this handle's max_sym
 *   ant_gain   HOST [n_ant], finite and >= 0: the inverse noise power of each antenna's receiver; NULL = equal noise (no
 *              multiply)
 *   out        DEVICE, 16-byte aligned.  frames (required) receives r's record with WIFIRX_F_DECODED / WIFIRX_F_CRC_OK cleared
 *              and WIFIRX_F_LLR set exactly when LLRs were written.  idx, llr, carrier are each optional (a decoder afterwards
 *              needs idx or llr) and are written for the record's n_sym symbols only; llr as wifirx_demod_batch writes it: when
 *              n_bpsc <= llr_bits, times the summed weight under WIFIRX_P_LLR_CSI, in the handle's WIFIRX_P_LLR_FORMAT.  A slot
 *              without a usable antenna gets antenna 0's record with COMPLETE, LLR, DECODED and CRC_OK cleared and nothing else.
 *              hbits must be NULL: the planes are not produced here (wifirx_decode_batch then packs them from idx); psdu,
 *              csi and sym_stats are not looked at.
 *   used_mask  DEVICE [n_slots], may be NULL: bit a = antenna a contributed to the slot (0: no usable antenna)
 * Checked on the host before anything is queued: WIFIRX_EINVAL for NULL in / out / out->frames, n_ant outside 1 .. 8, an
 * unknown mode, host buffers (on_device = 0), misaligned buffers, an antenna without frames, carrier or csi, an ant_gain that
 * is not finite or is negative, out->llr on a handle with llr_bits = 0, out->hbits != NULL, and an output pointer equal to an
 * input pointer; WIFIRX_ERANGE for n_slots above the handle's max_batch.  n_slots = 0 does nothing and returns WIFIRX_OK.
 * One kernel launch per call.
 * ORDER: as wifirx_channel -- `in` and ant_gain travel as kernel arguments, so they may be reused when the call returns; the
 * kernel runs asynchronously on the handle's stream, behind the handle's earlier calls: demod, combine, decode on one handle
 * need no wifirx_sync in between.  Batches demodulated by OTHER handles must have finished first (wifirx_sync on them). */
#define WIFIRX_DIV_MRC    0
#define WIFIRX_DIV_SELECT 1
int  wifirx_diversity_combine(wifirx_handle* h, uint32_t n_ant, const wifirx_out* in, uint32_t n_slots, int mode,
                              const float* ant_gain, const wifirx_out* out, uint8_t* used_mask);

/* Pre-detection combining (NUMERICS.md rule 33): the SAMPLES of n_ant antennas into one row set that wifirx_demod_batch reads
 * as it is.  Slot i of every antenna is the same transmission, sample for sample (the antennas of one radio).  Per slot the
 * weights v are blind: the n_ant x n_ant sample covariance R of the slot, its column at the antenna of the greatest power
 * (the lowest index on ties), `iters` power iterations, unit norm, rotated so that the reference antenna's weight is real and
 * non-negative; then y[n] = sum_a conj(v_a) x_a[n].  For one complex gain per antenna (a flat channel) and equal noise this
 * is maximal-ratio combining in front of the detector: plateau, LTS search, SIGNAL, the channel estimate and the data all get
 * the array gain, and ONE demod replaces n_ant demods and wifirx_diversity_combine.  One weight per antenna cannot follow a
 * frequency-selective channel: under multipath wifirx_diversity_combine is the better combiner.
 *   iq_dev       HOST [n_ant] of DEVICE pointers, n_ant = 1 .. 8: [n_slots][slot_len] float pairs each, 8-byte aligned
 *   slot_len     a multiple of 64, 64 .. 65536: the row stride of every antenna and of out_dev
 *   iters        0 .. 4 power iterations (0: the covariance column itself; 2 is the Python default)
 *   out_dev      DEVICE [n_slots][slot_len] pairs, 8-byte aligned, none of the inputs
 *   weights_dev  DEVICE [n_slots][n_ant] pairs or NULL: v as used
 *   stats_dev    DEVICE [n_slots] rows of 16 bytes or NULL: float lambda = Re(v^H R v), float trace = sum_a R_aa, uint32_t ref
 *                (the reference antenna), uint32_t flags (WIFIRX_PRE_DEGENERATE)
 * A slot whose trace or whose weight norm is not finite or not > 0 (silence, a NaN, an infinity, an overflow) is degenerate:
 * y = x_0 bit for bit, v = (1, 0, ..), lambda = 0, ref = 0 and the flag is set.  With n_ant = 1 y is x_0 bit for bit, v = (1, 0)
 * and the stats row is zero.
 * Checked on the host before anything is queued: WIFIRX_EINVAL for NULL h, iq_dev, iq_dev[a] or out_dev, n_ant outside 1 .. 8,
 * slot_len not a multiple of 64 or outside 64 .. 65536, iters above 4, a pointer that is not 8-byte aligned, out_dev equal to
 * an input pointer; WIFIRX_ERANGE for n_slots above the handle's max_batch.  n_slots = 0 does nothing and returns WIFIRX_OK.
 * One kernel launch per call.
 * ORDER: as wifirx_diversity_combine -- iq_dev travels as kernel arguments, so it may be reused when the call returns; the
 * kernel runs asynchronously on the handle's stream, behind the handle's earlier calls: precombine, demod, decode on one
 * handle need no wifirx_sync in between. */
#define WIFIRX_PRE_DEGENERATE 1u
int  wifirx_precombine(wifirx_handle* h, uint32_t n_ant, const float* const* iq_dev, uint32_t slot_len, uint32_t n_slots,
                       uint32_t iters, float* out_dev, float* weights_dev, void* stats_dev);

/* Stream-mode receive diversity (NUMERICS.md rules 24 and 23): wifirx_push for the n_ant sample-synchronous antennas of ONE
 * radio (a multi-channel USRP).  Detection runs once, on the sum of the antennas' autocorrelations and powers (rule 24), so
 * every antenna gets the same triggers and the same coarse CFO, and slot i of every antenna is the same transmission by
 * construction; per trigger every antenna's samples go through the frame kernel, the combiner of wifirx_diversity_combine
 * joins the n_ant rows, and decode_mac runs once, on the combined rows (on LLRs under WIFIRX_P_STREAM_SOFT).  Antennas that
 * are not sample-synchronous (several radios) are not what this takes: that needs the triggers of independent streams
 * associated, which is not built.
 *   cfg->n_ant      1 .. 8, fixed by the handle's first call.  One antenna gives, byte for byte, the stream of wifirx_push.
 *   cfg->mode       WIFIRX_DIV_MRC / WIFIRX_DIV_SELECT, cfg->ant_gain HOST [n_ant] or NULL: as wifirx_diversity_combine
 *   cfg->fmt, scale the sample format of every iq[a] (WIFIRX_IQ_*; scale widens the integer ones, rule 20)
 *   iq              HOST [n_ant] pointers, iq[a] = n samples of antenna a, host or device memory (cfg->iq_on_device), at the
 *                   format's natural alignment; n = 0 flushes.  DEVICE INPUT: what wifirx_push guarantees.
 * Everything runs in the caller's thread on the handle's stream: the pinned staging ring and the worker thread of wifirx_push
 * are not built for n_ant host streams.  WIFIRX_P_STREAM_BATCH > 0 keeps its meaning for device input: the call only collects
 * until that many samples wait.  A trigger settles when it is final (next trigger, WIFIRX_MAX_SAMPLES, flush) or when every
 * antenna's record is complete or failed for a reason more samples cannot cure.  All or nothing: after an error return the
 * stream is what it was before the call, and the call can be repeated as it was (wifirx_push_consumed is not involved).
 * DELIVERY: frames go to the handle's queue; wifirx_poll, wifirx_poll_csi, wifirx_poll_ex, wifirx_queued and wifirx_get_stats
 * work unchanged, and the statistics count a combined frame once.  The delivered record is the combiner's -- the reference
 * antenna's, then decoded --, idx / carrier / psdu are those of the combined points; the csi and sym_stats rows are the
 * reference antenna's own: the lowest usable antenna whose snr_db equals the combined record's (antenna 0 where no antenna is
 * usable).  A frame without a usable antenna is delivered as antenna 0's record with WIFIRX_F_COMPLETE cleared and zero rows.
 * WIFIRX_EINVAL, checked on the host before anything is queued and with the stream untouched: a NULL handle, cfg or iq, a NULL
 * iq[a] with n > 0, n_ant outside 1 .. 8 or different from the handle's first call, an unknown mode or fmt, a scale that is not
 * finite or <= 0 (integer formats), an ant_gain that is not finite or is negative, misaligned buffers, and a handle whose stream
 * has already taken samples through wifirx_push / wifirx_push_iq -- as those two refuse a handle that wifirx_push_diversity
 * has been called on: the two kinds of stream share the queue and the absolute sample index.  WIFIRX_EDEAD as for wifirx_push. */
typedef struct {
    uint32_t n_ant;          /* 1 .. 8, fixed by the handle's first call */
    int      mode;           /* WIFIRX_DIV_MRC / WIFIRX_DIV_SELECT */
    const float* ant_gain;   /* HOST [n_ant] or NULL, as wifirx_diversity_combine */
    int      fmt;            /* WIFIRX_IQ_* */
    float    scale;
    int      iq_on_device;
} wifirx_div_stream;

/* n samples of EVERY antenna (sample-synchronous); n = 0 flushes */
int  wifirx_push_diversity(wifirx_handle* h, const wifirx_div_stream* cfg, const void* const* iq, size_t n);

/* wifirx_poll_ex plus, per frame, which antennas contributed and every antenna's own record
 * (used_mask [cap], ant_frames [cap][n_ant]; either may be NULL).  Every antenna's record carries the joint trigger. */
int  wifirx_poll_diversity(wifirx_handle* h, const wifirx_poll_out* out, uint8_t* used_mask,
                           wifirx_frame* ant_frames, uint32_t cap, uint32_t* n_out);

/* Rule 24 over a device-resident capture from its origin: masks [ceil(n/64)] (bit l of word t = c[64 t + l] > threshold),
 * A [n] float pairs, P [n] or NULL; nothing is written behind them.  n_ant = 1 is the stream detector's metric (what the
 * reference plots on its correlation sink).  iq_dev: HOST [n_ant] device pointers, 8-byte aligned.  WIFIRX_EINVAL for NULL
 * arguments, n_ant outside 1 .. 8, a negative or NaN threshold and misaligned buffers.  Asynchronous on the handle's stream. */
int  wifirx_detect_multi(wifirx_handle* h, uint32_t n_ant, const float* const* iq_dev, uint64_t n,
                         float threshold, uint64_t* masks_dev, float* A_dev, float* P_dev);

/* Receive front end (NUMERICS.md rule 32): DC removal and blind IQ-imbalance correction of a sample stream, between the
 * ingest of rule 20 and the detection.  Opt-in everywhere; a handle or a call that does not ask for it computes what it did.
 * The stream is cut into blocks of WIFIRX_FE_BLOCK samples aligned to its origin.  Of every block five integer sums of the RAW
 * samples in Q-frac_bits fixed point are kept (sum u, sum v, sum u^2 + v^2, sum u^2 - v^2, sum 2uv), shifted right by 12 when
 * the block completes, in a ring of the last WIFIRX_FE_RING blocks.  Block b >= 1 is corrected with the mean over the
 * 2^min(shift, ilog2(b)) blocks in front of it (dc_shift for the offset d, iq_shift for the second moments that give the image
 * coefficient w); block 0 uses the state's initial values d0 and w0.  Per sample y = x - d, z = y - w conj(y).  Integer
 * statistics make the output and the state independent of how the stream is cut into calls, byte for byte.
 * The IQ stage is blind: it assumes a proper signal, which the 802.11 preamble is not, so on traffic of very short frames w is
 * biased (rule 32 gives figures); it is a switch of its own and off in every default.  The first block of a fresh state is
 * not corrected. */
#define WIFIRX_FE_DC    1u          /* flags: remove the offset */
#define WIFIRX_FE_IQ    2u          /* flags: remove the image */
#define WIFIRX_FE_BLOCK 4096
#define WIFIRX_FE_RING  64
typedef struct {
    uint32_t flags;          /* WIFIRX_FE_DC | WIFIRX_FE_IQ; a stage that is off uses d = 0 / w = 0, the statistics are taken anyway */
    uint32_t frac_bits;      /* F, 0 .. 30 (default 12): the statistics are rint(x * 2^F), clamped to +-(2^24 - 1) */
    uint32_t dc_shift;       /* 0 .. 6 (default 2): the offset is the mean over up to 2^dc_shift blocks */
    uint32_t iq_shift;       /* 0 .. 6 (default 4): the second moments are means over up to 2^iq_shift blocks */
} wifirx_frontend_cfg;

/* The state of one stream, 2632 bytes; all zero = a fresh stream.  The caller owns it (DEVICE memory for wifirx_frontend) and
 * may set d0 / w0 of a fresh state: what block 0 is corrected with. */
typedef struct {
    uint64_t n;                          /* samples taken so far */
    int64_t  part[5];                    /* the five sums of the block that is still open */
    int64_t  ring[WIFIRX_FE_RING][5];    /* the means of block b at ring[b % 64] */
    int64_t  d0[2];                      /* initial offset (I, Q) in Q-frac_bits */
    float    w0[2];                      /* initial image coefficient (re, im) */
} wifirx_frontend_state;

/* n samples of `fmt` at in (integer formats widened by rule 20 with `scale`, FC32: scale is not looked at) -> n corrected float
 * pairs at out, and *state_dev advanced by n samples.  DEVICE buffers: in at the format's natural alignment (8 / 4 / 2 bytes),
 * out and state_dev 8-byte aligned.  in == out is allowed for WIFIRX_IQ_FC32.  The same cfg must accompany a state throughout.
 * Checked on the host before anything is queued: WIFIRX_EINVAL for a NULL handle, cfg, state_dev, in or out, an unknown fmt,
 * flags outside WIFIRX_FE_DC | WIFIRX_FE_IQ, frac_bits > 30, a shift > 6, a scale that is not finite or <= 0 (integer formats),
 * misaligned buffers, n > 2^40, an overlap of in and out other than in == out for FC32, and a state that overlaps either.
 * n = 0 does nothing and returns WIFIRX_OK.  Three kernel launches per call (statistics, apply, state), whatever n is; a small
 * table of the call's block sums lives in the handle.
 * ORDER: as wifirx_iq_to_f32 -- asynchronous on the handle's stream, behind the handle's earlier calls. */
int  wifirx_frontend(wifirx_handle* h, const wifirx_frontend_cfg* cfg, wifirx_frontend_state* state_dev, const void* in,
                     int fmt, float scale, uint64_t n, float* out);

/* What the block that holds the stream's NEXT sample is corrected with, from a HOST copy of the state: dc = d (re, im),
 * w = (re, im), stages that are off giving zeros.  Pure host arithmetic, no handle, no device.  WIFIRX_EINVAL for a NULL
 * argument or a cfg that wifirx_frontend would refuse. */
int  wifirx_frontend_estimate(const wifirx_frontend_cfg* cfg, const wifirx_frontend_state* state_host, float dc[2], float w[2]);

/* Receiver impairments for the loop-back: out[i] = mu x[i] + nu conj(x[i]) + dc, elementwise in float32 (mu x and conj(x) nu
 * by NUMERICS.md rule 2, then (a + b) + dc per component).  DEVICE buffers of n float pairs, 8-byte aligned; in == out is
 * allowed, any other overlap is not.  mu, nu, dc: HOST, two finite floats each (they travel as kernel arguments).
 * WIFIRX_EINVAL for NULL arguments, a value that is not finite, misaligned buffers, a partial overlap, n > 2^40.  n = 0 does
 * nothing.  ORDER: as wifirx_iq_to_f32. */
int  wifirx_rx_impair(wifirx_handle* h, const float* in, float* out, uint64_t n, const float mu[2], const float nu[2],
                      const float dc[2]);

/* Stream mode: with a cfg, every later wifirx_push / wifirx_push_iq runs the front end on the samples it appends -- fused with
 * the widening for the integer formats, in place on the stream's sample buffer for FC32 -- in front of the detection, from the
 * state *init (HOST; NULL = fresh).  cfg == NULL switches the front end off (init is not looked at).  To be called before the
 * handle's first push or after a flush: samples already taken are not revisited.  The state lives in the handle; a push that
 * fails leaves it as it was (the call stays all or nothing).
 * OUT OF SCOPE: on a handle with the front end on, wifirx_push_diversity returns WIFIRX_EINVAL; wifirx_channelize has no
 * front-end option (condition its channel streams with wifirx_frontend, or through the handles they are pushed to).
 * WIFIRX_EINVAL for a NULL handle or a cfg that wifirx_frontend would refuse, and on a handle of a diversity stream. */
int  wifirx_stream_frontend(wifirx_handle* h, const wifirx_frontend_cfg* cfg, const wifirx_frontend_state* init);

/* The stream's front-end state to *out_host (waits for the handle's stream).  WIFIRX_EINVAL for NULL arguments or a handle
 * whose front end is off. */
int  wifirx_stream_frontend_state(wifirx_handle* h, wifirx_frontend_state* out_host);

/* plain device memory helpers so that a host language without a HIP binding can own buffers */
int  wifirx_dev_alloc(wifirx_handle* h, size_t bytes, void** out);
int  wifirx_dev_free(wifirx_handle* h, void* p);
int  wifirx_memcpy_h2d(wifirx_handle* h, void* dst, const void* src, size_t bytes);
int  wifirx_memcpy_d2h(wifirx_handle* h, void* dst, const void* src, size_t bytes);

/* Time the dominant kernel of wifirx_demod_batch with HIP events on the handle's stream: runs the
 * batch `iters` times and returns the mean kernel time in milliseconds (used by bench.py for
 * roofline.achieved). */
int  wifirx_time_demod(wifirx_handle* h, const float* iq_dev, uint32_t slot_len, uint32_t n_slots,
                       const wifirx_out* out, int iters, float* ms_mean);

#ifdef __cplusplus
}
#endif
#endif /* WIFIRX_H */
