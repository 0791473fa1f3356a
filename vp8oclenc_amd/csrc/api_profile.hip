// api_profile.hip -- per-kernel timers, the kernels' own clocks, debug taps and test hooks (nothing a host needs to code a frame).
//
#include "vp8hip_ctx.h"

using namespace vp8;

namespace vp8 {

int prof_collect(vp8hip_ctx *c) {
    if (c->ev_used == 0) return VP8HIP_OK;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int i = 0; i < c->ev_used; i += 2) {
        float ms = 0;
        HIPCHK(c, hipEventElapsedTime(&ms, c->ev[i], c->ev[i + 1]));
        c->prof_ms[c->ev_kernel[i / 2]] += ms;
        c->prof_n[c->ev_kernel[i / 2]] += 1;
    }
    c->ev_used = 0;
    return VP8HIP_OK;
}

}  // namespace vp8

extern "C" {

int vp8hip_profile_enable(vp8hip_ctx *c, uint32_t mask) {
    USE_DEVICE(c);
    JOIN_LF(c);
    if (!c) return VP8HIP_ERR_ARG;
    int rc = prof_collect(c);
    c->prof_mask = mask;
    return rc;
}

int vp8hip_profile_read(vp8hip_ctx *c, double *total_ms, int64_t *launches) {
    USE_DEVICE(c);
    if (!c) return VP8HIP_ERR_ARG;
    int rc = prof_collect(c);
    if (rc) return rc;
    for (int k = 0; k < VP8HIP_K_COUNT; ++k) {
        if (total_ms) total_ms[k] = c->prof_ms[k];
        if (launches) launches[k] = c->prof_n[k];
        c->prof_ms[k] = 0;
        c->prof_n[k] = 0;
    }
    return VP8HIP_OK;
}

int vp8hip_profile_read_clock(vp8hip_ctx *c, double *loop_filter_ms, int64_t *loop_filter_launches, double *shader_clock_ghz) {
    USE_DEVICE(c);
    if (!c || !loop_filter_ms || !loop_filter_launches) return VP8HIP_ERR_ARG;
    JOIN_LF(c);
    unsigned long long clk[6] = {0, 0, 0, 0, 0, 0};
    int32_t *base = c->d_progress + LF_ERR_WORD + 4;
    HIPCHK(c, hipMemcpyAsync(clk, base, sizeof(clk), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemsetAsync(base + 2, 0, 40, c->stream));   // sums and count restart; the start stamp is rewritten by every launch
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->lf_context_switches = (int64_t)clk[5];
    if (getenv("VP8HIP_DEBUG_CLOCK")) fprintf(stderr, "lf clock: launches %llu anomalies %llu hw_id changed %llu\n", clk[2], clk[4], clk[5]);
    *loop_filter_ms = (double)clk[1] * 1e-5;   // 100 MHz ticks
    *loop_filter_launches = (int64_t)clk[2];
    if (shader_clock_ghz) *shader_clock_ghz = clk[2] > clk[4] ? (double)clk[3] / (double)(clk[2] - clk[4]) * 1e-4 : 0.0;   // (cycles per tick x 1000) x 100 MHz
    return VP8HIP_OK;
}

int vp8hip_profile_search2_clock(vp8hip_ctx *c, int on) {
    if (!c) return VP8HIP_ERR_ARG;
    c->s2_clock_on = on != 0;
    return VP8HIP_OK;
}

// k_search2's launches by the kernel's own clock since the last call: total ms and launches (a batched launch counts once, on
// the batch's first member).  See launch_clock_end (vp8hip_dev.h).
int vp8hip_profile_read_search2_clock(vp8hip_ctx *c, double *ms, int64_t *launches) {
    USE_DEVICE(c);
    if (!c || !ms || !launches) return VP8HIP_ERR_ARG;
    JOIN_LF(c);
    unsigned long long w[5] = {0, 0, 0, 0, 0};
    HIPCHK(c, hipMemcpyAsync(w, s2_clock_words(c), sizeof(w), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemsetAsync(s2_clock_words(c) + 3, 0, 16, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *ms = (double)w[3] * 1e-5;   // 100 MHz ticks
    *launches = (int64_t)w[4];
    return VP8HIP_OK;
}

// Launches (among those of the last vp8hip_profile_read_clock) in which the wave that runs the frame's last row ended on another
// hardware slot than it started on: it was context-switched, i.e. the hardware scheduler is rotating an oversubscribed set of
// queues (more than 24 per process on this part).  0 on a healthy configuration.
int64_t vp8hip_profile_context_switches(const vp8hip_ctx *c) { return c ? c->lf_context_switches : 0; }

int vp8hip_debug_download(vp8hip_ctx *c, int what, int ref, int level, void *dst, size_t bytes) {
    USE_DEVICE(c);
    JOIN_LF(c);
    if (!c || !dst) return VP8HIP_ERR_ARG;
    hipStream_t s = c->stream;
    switch (what) {
        case VP8HIP_DBG_NET1:
        case VP8HIP_DBG_NET2: {
            if (ref < 0 || ref > 2 || bytes != (size_t)c->b8 * 4) return VP8HIP_ERR_ARG;
            HIPCHK(c, hipMemcpyAsync(dst, c->nets.net[ref][what == VP8HIP_DBG_NET1 ? 0 : 1], bytes, hipMemcpyDeviceToHost, s));
            break;
        }
        case VP8HIP_DBG_BDIFF:
            if (ref < 0 || ref > 2 || bytes != (size_t)c->b8 * 4) return VP8HIP_ERR_ARG;
            HIPCHK(c, hipMemcpyAsync(dst, c->nets.bdiff[ref], bytes, hipMemcpyDeviceToHost, s));
            break;
        case VP8HIP_DBG_PYRAMID: {
            if (ref < 0 || ref > 3 || level < 0 || level > 4) return VP8HIP_ERR_ARG;
            if (ref < 3 && c->slot[ref] < 0) return VP8HIP_ERR_STATE;
            const Frame &f = ref == 3 ? c->cur : c->frames[c->slot[ref]].f;
            const Plane &p = f.Y[level];
            if (bytes != (size_t)p.w * p.h) return VP8HIP_ERR_ARG;
            int rc = copy_out(c, dst, p);
            if (rc) return rc;
            break;
        }
        case VP8HIP_DBG_MB_MASK:
        case VP8HIP_DBG_MB_NZ:
            if (bytes != (size_t)c->mbs * 4) return VP8HIP_ERR_ARG;
            HIPCHK(c, hipMemcpyAsync(dst, what == VP8HIP_DBG_MB_MASK ? c->out.mask : c->out.nz, bytes, hipMemcpyDeviceToHost, s));
            break;
        case VP8HIP_DBG_THIRD_CONTEXT:
            if (bytes != (size_t)c->mbs * 25) return VP8HIP_ERR_ARG;
            HIPCHK(c, hipMemcpyAsync(dst, c->ent_third, bytes, hipMemcpyDeviceToHost, s));
            break;
        case VP8HIP_DBG_CURRENT_CHROMA: {
            if (ref < 0 || ref > 1 || c->cur_count == 0) return VP8HIP_ERR_ARG;
            const Plane &p = ref ? c->cur.V : c->cur.U;
            if (bytes != (size_t)p.w * p.h) return VP8HIP_ERR_ARG;
            int rc = copy_out(c, dst, p);
            if (rc) return rc;
            break;
        }
        case VP8HIP_DBG_ARF_FRAME: {
            if (ref < 0 || ref > 5) return VP8HIP_ERR_ARG;
            if (ref < 3) {      // the frame as it left k_arf_filter_b: tight, the incoming size it was made at
                if (!c->arf_w) return VP8HIP_ERR_STATE;
                const TightI420 t = tight_i420(c->arf_w, c->arf_h);
                const size_t n = ref ? (size_t)(c->arf_w / 2) * (c->arf_h / 2) : (size_t)c->arf_w * c->arf_h;
                if (bytes != n) return VP8HIP_ERR_ARG;
                HIPCHK(c, hipMemcpyAsync(dst, c->arf_stage.p + 256 + t.off[ref], n, hipMemcpyDeviceToHost, s));
                break;
            }
            if (c->slot[2] < 0) return VP8HIP_ERR_STATE;
            const Frame &f = c->frames[c->slot[2]].f;      // ALTREF: behind a hidden frame, its filtered reconstruction
            const Plane &p = ref == 3 ? f.Y[0] : (ref == 4 ? f.U : f.V);
            if (bytes != (size_t)p.w * p.h) return VP8HIP_ERR_ARG;
            int rc = copy_out(c, dst, p);
            if (rc) return rc;
            break;
        }
        case VP8HIP_DBG_REFRESH_FRAME: {
            if (ref < 0 || ref > 2) return VP8HIP_ERR_ARG;
            if (c->refreshed < 0) return VP8HIP_ERR_STATE;
            const Frame &f = c->frames[c->refreshed].f;      // GOLDEN, or the surface of a reconstruction that was dropped
            const Plane &p = ref == 0 ? f.Y[0] : (ref == 1 ? f.U : f.V);
            if (bytes != (size_t)p.w * p.h) return VP8HIP_ERR_ARG;
            int rc = copy_out(c, dst, p);
            if (rc) return rc;
            break;
        }
        case 100:  // diagnostic build only (-DLF2_STAMPS): cycle sums written by the loop filter
            if (bytes != 512) return VP8HIP_ERR_ARG;
            HIPCHK(c, hipMemcpyAsync(dst, (const char *)c->d_progress + 4096, 512, hipMemcpyDeviceToHost, s));
            break;
        default:
            return VP8HIP_ERR_ARG;
    }
    HIPCHK(c, hipStreamSynchronize(s));
    return VP8HIP_OK;
}

// test tap (not in the public header): re-run the quarter-pel search of one reference and return, for
// block `block`, 26 x {8 rows x 8 predicted pixels, cost, valid} as 26 x 18 dwords
// test tap (not in the public header): weight_opt of n caller-supplied 4x4 difference blocks
int vp8hip_debug_weight(vp8hip_ctx *c, const int32_t *d, int n, int32_t *out) {
    USE_DEVICE(c);
    JOIN_LF(c);
    if (!c || !d || !out || n <= 0) return VP8HIP_ERR_ARG;
    int32_t *dd = nullptr, *dout = nullptr;
    HIPCHK(c, hipMalloc(&dd, (size_t)n * 64));
    HIPCHK(c, hipMalloc(&dout, (size_t)n * 4));
    HIPCHK(c, hipMemcpyAsync(dd, d, (size_t)n * 64, hipMemcpyHostToDevice, c->stream));
    launch_weight_tap(c->stream, dd, n, dout);
    HIPCHK(c, hipMemcpyAsync(out, dout, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    hipFree(dd);
    hipFree(dout);
    return VP8HIP_OK;
}

// test tap (not in the public header): the same through the matrix-core form of the search kernels (weight_mfma)
int vp8hip_debug_weight_mfma(vp8hip_ctx *c, const int32_t *d, int n, int32_t *out) {
    USE_DEVICE(c);
    JOIN_LF(c);
    if (!c || !d || !out || n <= 0) return VP8HIP_ERR_ARG;
    int32_t *dd = nullptr, *dout = nullptr;
    HIPCHK(c, hipMalloc(&dd, (size_t)n * 64));
    HIPCHK(c, hipMalloc(&dout, (size_t)n * 4));
    HIPCHK(c, hipMemcpyAsync(dd, d, (size_t)n * 64, hipMemcpyHostToDevice, c->stream));
    launch_weight_tap_mfma(c->stream, dd, n, dout);
    HIPCHK(c, hipMemcpyAsync(out, dout, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    hipFree(dd);
    hipFree(dout);
    return VP8HIP_OK;
}

// test tap (not in the public header): the same through the row-order operand of the whole-pel search's loop form (metric_a_rows)
int vp8hip_debug_weight_mfma_rows(vp8hip_ctx *c, const int32_t *d, int n, int32_t *out) {
    USE_DEVICE(c);
    JOIN_LF(c);
    if (!c || !d || !out || n <= 0) return VP8HIP_ERR_ARG;
    int32_t *dd = nullptr, *dout = nullptr;
    HIPCHK(c, hipMalloc(&dd, (size_t)n * 64));
    HIPCHK(c, hipMalloc(&dout, (size_t)n * 4));
    HIPCHK(c, hipMemcpyAsync(dd, d, (size_t)n * 64, hipMemcpyHostToDevice, c->stream));
    launch_weight_tap_mfma_rows(c->stream, dd, n, dout);
    HIPCHK(c, hipMemcpyAsync(out, dout, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    hipFree(dd);
    hipFree(dout);
    return VP8HIP_OK;
}

// test tap (not in the public header): ONE level of the batched whole-pel search (launch_search1_batch, in the form the switches pick) over
// caller-written source nets.  The members' pyramids must stand (a batched inter_transform has run on them and every stream is idle).  src[3 i + r] /
// dst[3 i + r]: member i's net of reference r going in (the coarser level's vectors, b8 x short2) and coming out; null where the reference is not enabled.
int vp8hip_debug_search1_batch(vp8hip_ctx *const *ctxs, int n, const int *use_golden, const int *use_altref, int level,
                               const int16_t *const *src, int16_t *const *dst) {
    if (!ctxs || n <= 0 || n > MAX_BATCH || !use_golden || !use_altref || level < 0 || level > 4 || !src || !dst) return VP8HIP_ERR_ARG;
    vp8hip_ctx *c0 = ctxs[0];
    USE_DEVICE(c0);
    CodingItem it[MAX_BATCH];
    for (int i = 0; i < n; ++i) {
        vp8hip_ctx *c = ctxs[i];
        if (!c || c->b8 != c0->b8 || c->mbw != c0->mbw) return VP8HIP_ERR_ARG;
        JOIN_LF(c);
        it[i] = coding_item(c, use_golden[i], use_altref[i]);
        for (int r = 0; r < 3; ++r) {
            if (!it[i].refs.use[r]) continue;
            if (!src[3 * i + r] || !dst[3 * i + r]) return VP8HIP_ERR_ARG;
            HIPCHK(c0, hipMemcpyAsync(c->nets.net[r][0], src[3 * i + r], (size_t)c->b8 * 4, hipMemcpyHostToDevice, c0->stream));
            HIPCHK(c0, hipMemsetAsync(c->nets.net[r][1], 0, (size_t)c->b8 * 4, c0->stream));
        }
    }
    launch_search1_batch(c0->stream, it, n, level, 0, c0->mbw * 2);
    for (int i = 0; i < n; ++i)
        for (int r = 0; r < 3; ++r)
            if (it[i].refs.use[r]) HIPCHK(c0, hipMemcpyAsync(dst[3 * i + r], ctxs[i]->nets.net[r][1], (size_t)ctxs[i]->b8 * 4, hipMemcpyDeviceToHost, c0->stream));
    HIPCHK(c0, hipStreamSynchronize(c0->stream));
    HIPCHK(c0, hipGetLastError());
    return VP8HIP_OK;
}

// test tap (not in the public header): n quadruples of int32 through the quarter-pel search's own round_pack4 (kernels_s2.hip): out[i] = the four
// biased bytes sat_i8(v[4 i + j] >> 7), j = 0 in the lowest byte
int vp8hip_debug_round_pack4(vp8hip_ctx *c, const int32_t *v, int n, uint32_t *out) {
    USE_DEVICE(c);
    JOIN_LF(c);
    if (!c || !v || !out || n <= 0) return VP8HIP_ERR_ARG;
    int32_t *dv = nullptr;
    uint32_t *dout = nullptr;
    HIPCHK(c, hipMalloc(&dv, (size_t)n * 16));
    HIPCHK(c, hipMalloc(&dout, (size_t)n * 4));
    HIPCHK(c, hipMemcpyAsync(dv, v, (size_t)n * 16, hipMemcpyHostToDevice, c->stream));
    launch_round_pack4_tap(c->stream, dv, n, dout);
    HIPCHK(c, hipMemcpyAsync(out, dout, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    hipFree(dv);
    hipFree(dout);
    return VP8HIP_OK;
}

// test tap (not in the public header): the batched quarter-pel search (launch_search2_batch, in the form the switches pick) over caller-written
// whole-pel nets.  The members' current frames and references must stand and every stream be idle (as for vp8hip_debug_search1_batch).  src[3 i + r]:
// member i's whole-pel net of reference r (b8 x short2) going in; dst[3 i + r] / bdiff[3 i + r]: its quarter-pel net and costs coming out; null where
// the reference is not enabled.  No parameter scan rides along.
int vp8hip_debug_search2_batch(vp8hip_ctx *const *ctxs, int n, const int *use_golden, const int *use_altref, const int16_t *const *src,
                               int16_t *const *dst, int32_t *const *bdiff) {
    if (!ctxs || n <= 0 || n > MAX_BATCH || !use_golden || !use_altref || !src || !dst || !bdiff) return VP8HIP_ERR_ARG;
    vp8hip_ctx *c0 = ctxs[0];
    USE_DEVICE(c0);
    CodingItem it[MAX_BATCH];
    for (int i = 0; i < n; ++i) {
        vp8hip_ctx *c = ctxs[i];
        if (!c || c->b8 != c0->b8 || c->mbw != c0->mbw) return VP8HIP_ERR_ARG;
        JOIN_LF(c);
        it[i] = coding_item(c, use_golden[i], use_altref[i]);
        it[i].scan = nullptr;
        for (int r = 0; r < 3; ++r) {
            if (!it[i].refs.use[r]) continue;
            if (!src[3 * i + r] || !dst[3 * i + r] || !bdiff[3 * i + r]) return VP8HIP_ERR_ARG;
            HIPCHK(c0, hipMemcpyAsync(c->nets.net[r][1], src[3 * i + r], (size_t)c->b8 * 4, hipMemcpyHostToDevice, c0->stream));
            HIPCHK(c0, hipMemsetAsync(c->nets.net[r][0], 0x55, (size_t)c->b8 * 4, c0->stream));
            HIPCHK(c0, hipMemsetAsync(c->nets.bdiff[r], 0x55, (size_t)c->b8 * 4, c0->stream));
        }
    }
    launch_search2_batch(c0->stream, it, n);
    for (int i = 0; i < n; ++i)
        for (int r = 0; r < 3; ++r) {
            if (!it[i].refs.use[r]) continue;
            HIPCHK(c0, hipMemcpyAsync(dst[3 * i + r], ctxs[i]->nets.net[r][0], (size_t)ctxs[i]->b8 * 4, hipMemcpyDeviceToHost, c0->stream));
            HIPCHK(c0, hipMemcpyAsync(bdiff[3 * i + r], ctxs[i]->nets.bdiff[r], (size_t)ctxs[i]->b8 * 4, hipMemcpyDeviceToHost, c0->stream));
        }
    HIPCHK(c0, hipStreamSynchronize(c0->stream));
    HIPCHK(c0, hipGetLastError());
    return VP8HIP_OK;
}

// test tap (not in the public header, no device needed): the metric's two A operands as the kernels hold them, 64 lanes x 4 dwords each --
// column order (K_METRIC_A) and row order (K_METRIC_A_ROWS)
int vp8hip_debug_metric_tables(uint32_t *a_cols, uint32_t *a_rows) {
    if (!a_cols || !a_rows) return VP8HIP_ERR_ARG;
    static constexpr MetricTable cols = make_metric_a(), rows = make_metric_a_rows();
    memcpy(a_cols, cols.w, sizeof(cols.w));
    memcpy(a_rows, rows.w, sizeof(rows.w));
    return VP8HIP_OK;
}

// test hook (not in the public header): while on, the loop filter's inter-band counters are published from a wrong
// base, so every band but the first runs into its bounded wait -> VP8HIP_ERR_TIMEOUT at the next synchronize
int vp8hip_debug_lf_stall(vp8hip_ctx *c, int on) {
    USE_DEVICE(c);
    JOIN_LF(c);
    if (!c) return VP8HIP_ERR_ARG;
    c->lf_stall_test = on ? 1 : 0;
    return VP8HIP_OK;
}

// test hook (not in the public header): MB_SSIM as an inter frame would have left it, so vp8hip_check_ssim can be
// driven from stored inter-frame results (the golden vectors of tests/golden/intra)
int vp8hip_debug_upload_ssim(vp8hip_ctx *c, const float *ssim) {
    USE_DEVICE(c);
    JOIN_LF(c);
    if (!c || !ssim) return VP8HIP_ERR_ARG;
    HIPCHK(c, hipMemcpyAsync(c->out.ssim, ssim, (size_t)c->mbs * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return VP8HIP_OK;
}

// test hook (not in the public header): everything vp8hip_encode_header reads, set directly -- lets the tests drive the
// device coder with the stress inputs of tests/bitstream_cases.py and the golden vectors.  NULL = leave as is.
int vp8hip_debug_upload_header_inputs(vp8hip_ctx *c, const int32_t *seg, const int32_t *nz, const int32_t *ref, const int32_t *parts,
                                      const int16_t *vectors, const int32_t *is_inter, const int32_t *modes, const uint32_t *probs,
                                      const uint32_t *denom, const int32_t *sd) {
    USE_DEVICE(c);
    JOIN_LF(c);
    if (!c) return VP8HIP_ERR_ARG;
    hipStream_t s = c->stream;
    const size_t n = c->mbs;
    if (seg) HIPCHK(c, hipMemcpyAsync(c->out.seg, seg, n * 4, hipMemcpyHostToDevice, s));
    if (nz) HIPCHK(c, hipMemcpyAsync(c->out.nz, nz, n * 4, hipMemcpyHostToDevice, s));
    if (ref) HIPCHK(c, hipMemcpyAsync(c->out.ref, ref, n * 4, hipMemcpyHostToDevice, s));
    if (parts) HIPCHK(c, hipMemcpyAsync(c->out.parts, parts, n * 4, hipMemcpyHostToDevice, s));
    if (vectors) HIPCHK(c, hipMemcpyAsync(c->out.vec, vectors, n * 16, hipMemcpyHostToDevice, s));
    if (is_inter) HIPCHK(c, hipMemcpyAsync(c->intra_is_inter, is_inter, n * 4, hipMemcpyHostToDevice, s));
    if (modes) HIPCHK(c, hipMemcpyAsync(c->intra_modes, modes, n * 64, hipMemcpyHostToDevice, s));
    if (probs) HIPCHK(c, hipMemcpyAsync(c->ent_probs, probs, sizeof(uint32_t) * ENT_NCTX, hipMemcpyHostToDevice, s));
    if (denom) HIPCHK(c, hipMemcpyAsync(c->ent_denom0, denom, sizeof(uint32_t) * ENT_NCTX, hipMemcpyHostToDevice, s));
    if (sd) HIPCHK(c, hipMemcpyAsync(c->d_sd, sd, sizeof(SegData), hipMemcpyHostToDevice, s));
    HIPCHK(c, hipStreamSynchronize(s));
    if (probs || denom) c->ent_counted_partitions = 1;
    return VP8HIP_OK;
}

}  // extern "C"
