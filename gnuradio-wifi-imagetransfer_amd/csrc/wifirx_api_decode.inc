// decode_mac entry point: Viterbi + descramble + CRC on the device (wr_decode.hip)
static int decode_batch_impl(wifirx_handle* h, uint32_t n_slots, const wifirx_out* out);

extern "C" int wifirx_decode_batch(wifirx_handle* h, uint32_t n_slots, const wifirx_out* out)
{
    if (!h || !out) return WIFIRX_EINVAL;
    stream_worker_wait_idle(h);            // the worker's own decode calls go to decode_batch_impl directly
    return decode_batch_impl(h, n_slots, out);
}

// ---- what both decoders share: the pre-pass, the grouping by rate, the survivor scratch ----

// The pre-pass: longest trellis of the batch (it sizes the survivor scratch) -> pre[0], 0 when nothing is decodable;
// decodable frames per rate -> pre[1 + enc].  The one host sync of a decode call.
static int decode_prepass(wifirx_handle* h, uint32_t n_slots, const wifirx_out* out, uint32_t (&pre)[9])
{
    HIP_TRY(h, hipSetDevice(h->device));
    int rc = h->dec.max.reserve(h, 256);
    if (rc) return rc;
    // dec_max: [0] longest trellis, [1..8] decodable frames per rate, [16..23] cursors of the permutation kernel
    HIP_TRY(h, hipMemsetAsync(h->dec.max.p, 0, 256, h->stream));
    HIP_TRY(h, wr_launch_decode_maxsteps(h->stream, n_slots, h->cfg.max_sym, out->frames, out->psdu_stride,
                                         h->dec.max.as<uint32_t>()));
    HIP_TRY(h, hipMemcpyAsync(pre, h->dec.max.p, sizeof pre, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return WIFIRX_OK;
}

// Tasks of `fpw` frames, each of one rate.  Several rates in the batch: the decodable frames are grouped by rate (a
// permutation, built on the device), every run starting on a task boundary -- the run of rate e is [starts[e],
// starts[e + 1]) -- so that each wave's frames share one rate: the decoders then read where a coded bit sits through the
// scalar unit for all of them (the per-lane look-ups of mixed waves cost +25 %), and frames decode_mac leaves alone take
// no lane at all.  One rate: no permutation, frame k is slot k.
struct DecodeGroups { uint32_t starts[9]; uint32_t n_virtual; const uint32_t* perm; };      // perm = nullptr: n_virtual = n_slots

static int decode_group_by_rate(wifirx_handle* h, uint32_t n_slots, const wifirx_out* out, const uint32_t (&pre)[9],
                                uint32_t fpw, DecodeGroups& g)
{
    uint32_t n_rates = 0;
    g.starts[0] = 0;
    for (int e = 0; e < 8; e++) {
        n_rates += pre[1 + e] != 0;
        g.starts[e + 1] = g.starts[e] + (pre[1 + e] + fpw - 1) / fpw * fpw;
    }
    g.n_virtual = n_rates > 1 ? g.starts[8] : n_slots;
    g.perm = nullptr;
    if (n_rates <= 1) return WIFIRX_OK;
    int rc = h->dec.perm.reserve(h, (size_t)g.n_virtual * sizeof(uint32_t));
    if (rc) return rc;
    HIP_TRY(h, hipMemsetAsync(h->dec.perm.p, 0xff, (size_t)g.n_virtual * sizeof(uint32_t), h->stream));
    HIP_TRY(h, wr_launch_decode_perm(h->stream, n_slots, h->cfg.max_sym, out->frames, out->psdu_stride, g.starts,
                                     h->dec.max.as<uint32_t>() + 16, h->dec.perm.as<uint32_t>()));
    g.perm = h->dec.perm.as<const uint32_t>();
    return WIFIRX_OK;
}

// The scratch budget: WR_DECODE_SCRATCH_BUDGET at most, and no more than 70 % of what the device has free right now (plus
// what this handle already holds for the purpose) -- a process that shares the GPU with other buffers, or holds several
// handles, gets fewer waves instead of ENOMEM (ADVICE r03).  The slice is kept until wifirx_destroy (INTEGRATION.md:
// footprint).
static size_t decode_scratch_budget(wifirx_handle* h)
{
    size_t budget = WR_DECODE_SCRATCH_BUDGET;
    size_t mem_free = 0, mem_total = 0;
    if (hipMemGetInfo(&mem_free, &mem_total) == hipSuccess) budget = std::min<size_t>(budget, (mem_free + h->dec.scratch.bytes) / 10 * 7);
    else (void)hipGetLastError();
    if (h->env.decode_budget) budget = std::min<size_t>(budget, h->env.decode_budget);
    return budget;
}

// `stride` bytes per wave for up to `want` waves, as many as the budget holds.  If the allocation fails all the same: half
// the waves, and again, down to four -- the kernels are grid-stride over tasks, fewer waves only take longer.
static int decode_alloc_scratch(wifirx_handle* h, size_t stride, size_t want, size_t budget, size_t& n_waves)
{
    n_waves = std::max<size_t>(1, std::min<size_t>(want, budget / stride));
    for (;;) {
        int rc;
        if (h->env.fail_decode_scratch > 0 && h->env.fail_decode_scratch-- > 0) {
            // test hook: a REAL failing hipMalloc (a size no device has), so that the retry runs with whatever state HIP keeps
            // after an exhausted allocation -- the sticky last-error above all (ADVICE r04)
            DevBuf none;
            rc = none.reserve(h, SIZE_MAX / 2);
            if (rc == WIFIRX_OK) rc = fail(h, WIFIRX_ENOMEM, "hipMalloc(decode scratch): test hook");
        } else {
            rc = h->dec.scratch.reserve(h, stride * n_waves);
        }
        if (rc == WIFIRX_OK) return WIFIRX_OK;
        if (rc != WIFIRX_ENOMEM || n_waves <= 4) return rc;
        n_waves /= 2;
    }
}

// ---------------------------------------------------------------------------------------------
static int decode_batch_impl(wifirx_handle* h, uint32_t n_slots, const wifirx_out* out)
{
    if (!h || !out) return WIFIRX_EINVAL;
    if (!out->on_device) return fail(h, WIFIRX_EINVAL, "wifirx_decode_batch works on device buffers (out->on_device = 1)");
    if (!out->frames || (!out->idx && !out->hbits) || !out->psdu || out->psdu_stride == 0)
        return fail(h, WIFIRX_EINVAL, "frames, hbits or idx, and psdu (with psdu_stride) are required");
    if (reinterpret_cast<uintptr_t>(out->hbits) & 15) return fail(h, WIFIRX_EINVAL, "out->hbits must be 16-byte aligned");
    if (n_slots == 0) return WIFIRX_OK;
    uint32_t pre[9] = { 0 };
    int rc = decode_prepass(h, n_slots, out, pre);
    if (rc || pre[0] == 0) return rc;                         // (pre[0] == 0: nothing decodable)
    const uint32_t n_steps = pre[0];
    // the decoders read the decisions as bit planes: the caller's (written by the demod kernel), or packed from idx here
    const uint32_t* hbits = out->hbits;
    if (!hbits) {
        rc = h->dec.hbits.reserve(h, (size_t)n_slots * h->cfg.max_sym * 48);
        if (rc) return rc;
        HIP_TRY(h, wr_launch_decode_pack(h->stream, n_slots, h->cfg.max_sym, out->frames, out->idx, out->psdu_stride,
                                         h->dec.hbits.as<uint32_t>(), n_steps));
        hbits = h->dec.hbits.as<const uint32_t>();
    }
    if (n_slots <= h->tune.decode_small_max) {
        // few frames: one wave per frame (8 B of survivor bits per step + the decoded words of the frame)
        const size_t stride = wr::dec_small_slice(n_steps);
        const size_t n_waves = std::min<size_t>(n_slots, WR_DECODE_MAX_WAVES);
        rc = h->dec.scratch.reserve(h, stride * n_waves);
        if (rc) return rc;
        HIP_TRY(h, wr_launch_decode_small(h->stream, n_slots, h->cfg.max_sym, out->frames, hbits, out->psdu,
                                          out->psdu_stride, h->dec.scratch.as<uint8_t>(), stride, n_steps,
                                          (uint32_t)n_waves));
        return WIFIRX_OK;
    }
    // per wave: the survivor bits of every step and lane (16 B for two frames per lane, 32 B for four) and the decoded words of
    // the lane's frames (layouts in wr_kernels.h).  Four frames per lane (decode_q_kernel: byte metrics, 256 frames per
    // wave) when the batch holds enough decodable frames to fill the GPU with such waves; WIFIRX_DECODE_Q=1 / 0 forces /
    // forbids it (tests).
    uint32_t n_dec = 0;
    for (int e = 0; e < 8; e++) n_dec += pre[1 + e];
    const bool use_q = h->env.decode_q == 1 || (h->env.decode_q < 0 && n_dec >= WR_DECODE_Q_MIN_FRAMES);
    const uint32_t fpw_max = use_q ? WR_DECODE_Q_FRAMES_PER_WAVE : WR_DECODE_FRAMES_PER_WAVE;
    size_t stride = use_q ? wr::dec_q_slice(n_steps, false) : wr::dec_pair_slice(n_steps);
    // mid-size batches: fewer frames per wave, so that about a thousand waves share the work
    uint32_t fpw = (uint32_t)std::min<size_t>(fpw_max, std::max<size_t>(1, (n_slots + 1023) / 1024));
    if (use_q && h->env.decode_q < 0) fpw = fpw_max;
    if (h->env.decode_fpw) fpw = std::min<uint32_t>(fpw_max, h->env.decode_fpw);     // tests: full waves on small batches
    DecodeGroups g;
    if ((rc = decode_group_by_rate(h, n_slots, out, pre, fpw, g))) return rc;
    const size_t n_tasks = (g.n_virtual + fpw - 1) / fpw;
    // decode_q_kernel hides the trace-back under add-compare-select work when the batch fills the GPU with 256-frame tasks: mode 2
    // (round 5) walks every block of 96 steps back speculatively while the task's own next block runs -- three waves per SIMD
    // (168 registers; two for the 64-QAM instance), one scratch slice per wave + the walks' start states.  Mode 0: the trace-back
    // behind each task.  WIFIRX_DECODE_OVL = 0 / 2 forces a mode (tests, A/B).
    size_t budget = decode_scratch_budget(h);
    const size_t stride_spec = wr::dec_q_slice(n_steps, true);
    const size_t spec_waves = (size_t)h->n_simd * ((pre[7] | pre[8]) ? 2 : WR_DQ_SPEC_WAVES);      // (the 64-QAM instance: two workgroups of its LDS fit a CU)
    int mode = 0;
    if (use_q) {
        if (h->env.decode_ovl >= 0) mode = h->env.decode_ovl;
        else if (n_tasks >= WR_DECODE_MAX_WAVES / 2 && budget / stride_spec >= spec_waves) mode = 2;
    }
    // the scratch falls back to fewer waves only: the mode stays what was chosen
    if (mode == 2) stride = stride_spec;
    size_t n_waves = 0;
    if ((rc = decode_alloc_scratch(h, stride, std::min<size_t>(n_tasks, mode == 2 ? spec_waves : WR_DECODE_MAX_WAVES), budget, n_waves)))
        return rc;
    if (use_q)
        HIP_TRY(h, wr_launch_decode_q(h->stream, n_slots, h->cfg.max_sym, out->frames, hbits, out->psdu,
                                      out->psdu_stride, h->dec.scratch.as<uint8_t>(), stride, n_steps,
                                      (uint32_t)n_waves, fpw, g.perm, g.n_virtual, (pre[7] | pre[8]) != 0, mode));
    else
        HIP_TRY(h, wr_launch_decode(h->stream, n_slots, h->cfg.max_sym, out->frames, hbits, out->psdu,
                                    out->psdu_stride, h->dec.scratch.as<uint8_t>(), stride, n_steps,
                                    (uint32_t)n_waves, fpw, g.perm, g.n_virtual));
    return WIFIRX_OK;
}

// ---------------------------------------------------------------------------------------------
// Soft-decision decode_mac (NUMERICS.md rule 14, wr_decode_soft.hip): the same frames, scratch and result fields as
// wifirx_decode_batch, the LLR rows (`llr_bits` per carrier reserved per row) instead of the hard decisions.
// bf16: the rows are WIFIRX_LLR_BF16 values (the handle's batch format; stream mode passes false).
static int decode_batch_soft_impl(wifirx_handle* h, uint32_t n_slots, const wifirx_out* out, uint32_t llr_bits, bool bf16);

extern "C" int wifirx_decode_batch_soft(wifirx_handle* h, uint32_t n_slots, const wifirx_out* out)
{
    if (!h || !out) return WIFIRX_EINVAL;
    stream_worker_wait_idle(h);
    if (h->cfg.llr_bits == 0) return fail(h, WIFIRX_EINVAL, "wifirx_decode_batch_soft needs a handle created with llr_bits > 0");
    return decode_batch_soft_impl(h, n_slots, out, h->cfg.llr_bits, h->tune.llr_format == WIFIRX_LLR_BF16);
}

static int decode_batch_soft_impl(wifirx_handle* h, uint32_t n_slots, const wifirx_out* out, uint32_t llr_bits, bool bf16)
{
    if (!out->on_device) return fail(h, WIFIRX_EINVAL, "wifirx_decode_batch_soft works on device buffers (out->on_device = 1)");
    if (!out->frames || !out->llr || !out->psdu || out->psdu_stride == 0)
        return fail(h, WIFIRX_EINVAL, "frames, llr and psdu (with psdu_stride) are required");
    if (reinterpret_cast<uintptr_t>(out->llr) & 15) return fail(h, WIFIRX_EINVAL, "out->llr must be 16-byte aligned");
    if (n_slots == 0) return WIFIRX_OK;
    // the hard path's pre-pass (frames without WIFIRX_F_LLR are counted too; the kernel leaves them alone)
    uint32_t pre[9] = { 0 };
    int rc = decode_prepass(h, n_slots, out, pre);
    if (rc || pre[0] == 0) return rc;
    const uint32_t n_steps = pre[0];
    // tasks of 64 frames (one per lane), each of one rate; one launch per bits-per-carrier class over its range of tasks
    const uint32_t fpw = 64;
    DecodeGroups g;
    if ((rc = decode_group_by_rate(h, n_slots, out, pre, fpw, g))) return rc;
    const size_t n_tasks = (g.n_virtual + fpw - 1) / fpw;
    // per wave: 8 bytes of survivor bits per step and lane, the decoded words of its 64 frames (two spare words)
    const size_t stride = wr::dec_soft_slice(n_steps);
    size_t n_waves = 0;
    if ((rc = decode_alloc_scratch(h, stride, std::min<size_t>(n_tasks, WR_DECODE_MAX_WAVES), decode_scratch_budget(h), n_waves)))
        return rc;
    const int nb_of_class[4] = { 1, 2, 4, 6 };
    for (int c = 0; c < 4; c++) {
        const int e0 = 2 * c, e1 = 2 * c + 1;
        if (pre[1 + e0] == 0 && pre[1 + e1] == 0) continue;
        // task range of the class: its runs in the permutation, or every task when the batch holds one rate
        const uint32_t lo = g.perm ? g.starts[e0] / fpw : 0u, hi = g.perm ? g.starts[e1 + 1] / fpw : (uint32_t)n_tasks;
        const uint32_t waves = (uint32_t)std::min<size_t>(n_waves, hi - lo);
        if (bf16)
            HIP_TRY(h, wr_launch_decode_soft_bf16(h->stream, nb_of_class[c], n_slots, h->cfg.max_sym, llr_bits, out->frames,
                                                  reinterpret_cast<const uint16_t*>(out->llr), out->psdu, out->psdu_stride,
                                                  h->dec.scratch.as<uint8_t>(), stride, n_steps, waves, g.perm,
                                                  g.n_virtual, lo, hi));
        else
        HIP_TRY(h, wr_launch_decode_soft(h->stream, nb_of_class[c], n_slots, h->cfg.max_sym, llr_bits, out->frames, out->llr,
                                         out->psdu, out->psdu_stride, h->dec.scratch.as<uint8_t>(), stride,
                                         n_steps, waves, g.perm, g.n_virtual, lo, hi));
    }
    return WIFIRX_OK;
}
