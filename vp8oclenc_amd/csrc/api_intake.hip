// api_intake.hip -- how a frame becomes a context's current frame: the source size, scaling, format and colour setters, the staging
// buffers, the stage order (take_frames: window, convert, deinterlace, orient, scale or pack, overlay, denoise, analysis, segment map -- the one place that knows it), and the
// single-context ways in (vp8hip_set_current_device, vp8hip_upload_current, vp8hip_prefetch_current).  A batch's ways in are api_batch.hip's;
// they end in take_frames too.  A context with a canvas (vp8hip_set_canvas) takes several sources per frame: vp8hip_compose_current_device / _host
// launch k_compose_b in the place of the pack or scale launch and share everything behind it (finish_frames).  Replaces the uploads of vp8enc.cpp:386-401.
#include "vp8hip_ctx.h"

using namespace vp8;

// what is still in flight may read the scaler's tables, a staging buffer or a stage's history, or write a record: it ends first
int vp8::quiesce_intake(vp8hip_ctx *c) {
    (void)hipSetDevice(c->device);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->lf_stream) HIPCHK(c, hipStreamSynchronize(c->lf_stream));
    if (c->h2d_stream) HIPCHK(c, hipStreamSynchronize(c->h2d_stream));
    if (c->batch && c->batch->prep) HIPCHK(c, hipStreamSynchronize(c->batch->prep));
    if (c->batch && c->batch->copy) HIPCHK(c, hipStreamSynchronize(c->batch->copy));
    return VP8HIP_OK;
}

int DeviceBuf::grow(vp8hip_ctx *c, size_t need) {
    if (need <= bytes) return VP8HIP_OK;
    { const int rc = quiesce_intake(c); if (rc) return rc; }
    uint8_t *d = nullptr;
    HIPCHK(c, hipMalloc(&d, need));
    (void)hipFree(p);
    p = d;
    bytes = need;
    return VP8HIP_OK;
}

namespace vp8 {

// sw, sh: size of the planes that come in (0 = the coded size): the current frames of a context with a source size
int set_frame_planes(vp8hip_ctx *c, Frame &f, const void *y, const void *u, const void *v, hipMemcpyKind kind, int sw, int sh) {
    Timed t(c, VP8HIP_K_PACK);
    if (kind == hipMemcpyDeviceToDevice) {
        const SourceItem it{&f, y, u, v, nullptr};
        launch_pack_batch(c->stream, &it, 1, sw, sh);
        return VP8HIP_OK;
    }
    if (sw > 0) {
        // the source rectangle into the surface, then copy_with_padding in place: the pack kernel with the surface as its own
        // source (samples inside the rectangle are rewritten with themselves, the rest repeats the rectangle's edge)
        HIPCHK(c, hipMemcpy2DAsync(f.Y[0].p, f.Y[0].stride, y, sw, sw, sh, kind, c->stream));
        HIPCHK(c, hipMemcpy2DAsync(f.U.p, f.U.stride, u, sw / 2, sw / 2, sh / 2, kind, c->stream));
        HIPCHK(c, hipMemcpy2DAsync(f.V.p, f.V.stride, v, sw / 2, sw / 2, sh / 2, kind, c->stream));
        const SourceItem it{&f, f.Y[0].p, f.U.p, f.V.p, nullptr};
        launch_pack_batch(c->stream, &it, 1, sw, sh, f.Y[0].stride, f.U.stride);
        return VP8HIP_OK;
    }
    int rc;
    if ((rc = copy_in(c, f.Y[0], y, kind))) return rc;
    if ((rc = copy_in(c, f.U, u, kind))) return rc;
    return copy_in(c, f.V, v, kind);
}

int copy_planes(vp8hip_ctx *c, uint8_t *d, const void *y, const void *u, const void *v, const size_t nb[3], hipMemcpyKind kind, hipStream_t s) {
    const uint8_t *py = static_cast<const uint8_t *>(y);
    if (c->in.win_on) {      // y, u, v: the plane bases of a surface; the window's rows, tight, and nothing else
        size_t off[3];
        int32_t rb[3], rows[3];
        if (window_rule(c, off, rb, rows) != 0) return VP8HIP_ERR_ARG;
        const uint8_t *src[3] = {py, static_cast<const uint8_t *>(u), static_cast<const uint8_t *>(v)};
        for (int p = 0; p < 3; ++p) {
            if (rows[p]) HIPCHK(c, hipMemcpy2DAsync(d, (size_t)rb[p], src[p] + off[p], (size_t)c->in.win_pitch[p], (size_t)rb[p], (size_t)rows[p], kind, s));
            d += nb[p];
        }
        return VP8HIP_OK;
    }
    if (!nb[1] || (u == py + nb[0] && (!nb[2] || v == py + nb[0] + nb[1]))) {      // (one plane, or planes end to end)
        HIPCHK(c, hipMemcpyAsync(d, y, nb[0] + nb[1] + nb[2], kind, s));
        return VP8HIP_OK;
    }
    HIPCHK(c, hipMemcpyAsync(d, y, nb[0], kind, s));
    HIPCHK(c, hipMemcpyAsync(d + nb[0], u, nb[1], kind, s));
    if (nb[2]) HIPCHK(c, hipMemcpyAsync(d + nb[0] + nb[1], v, nb[2], kind, s));
    return VP8HIP_OK;
}

// the item of a stage that writes a member's three planes into a staging buffer of its own, plane p at stage + at[p] (k_window_b,
// k_convert_b / k_tonemap_b, k_orient_b): afterwards y, u, v are the planes there, and what follows reads those
static void planes_item(PlanesItem &it, uint8_t *stage, const size_t at[3], const void *&y, const void *&u, const void *&v) {
    const void *src[3] = {y, u, v};
    for (int p = 0; p < 3; ++p) {
        it.src[p] = static_cast<const uint8_t *>(src[p]);
        it.dst[p] = stage + at[p];
    }
    y = it.dst[0]; u = it.dst[1]; v = it.dst[2];
}

int intake_ready(vp8hip_ctx *const *m, int n) {
    for (int i = 0; i < n; ++i) {      // (first use, or the incoming size has grown: not a per-frame event)
        vp8hip_ctx *c = m[i];
        if (!needs_device_planes(c->in)) continue;      // (no stage in front of the pack: no staging buffer)
        int w, h;
        size_t nb[3];
        incoming_size(c, &w, &h);
        incoming_bytes(c, nb);
        const size_t tight = tight_i420(w, h).bytes;
        int rc = c->in.src_fmt ? c->fmt_stage.grow(c, tight) : VP8HIP_OK;      // the converter's output
        if (!rc) rc = deinterlace_ready(c);
        if (!rc && c->in.win_on) rc = c->win_stage.grow(c, nb[0] + nb[1] + nb[2]);      // the window's tight planes, laid out as raw_stage
        if (!rc && (c->in.or_turns || c->in.or_mirror)) rc = c->or_stage.grow(c, tight);      // the upright frame (the same bytes for w x h and h x w)
        if (rc) return rc;
    }
    return VP8HIP_OK;
}

int intake_apply(vp8hip_ctx *c, const IntakeSettings &next) {
    if (next == c->in) return VP8HIP_OK;
    if (intake_valid(c->W, c->H, next) != VP8HIP_OK) return VP8HIP_ERR_ARG;
    // a launch still in flight reads the staging buffers, the tables and the histories and writes the records: it ends first
    { const int rc = quiesce_intake(c); if (rc) return rc; }
    const IntakeSettings before = c->in;
    c->in = next;
    { const int rc = intake_ready(&c, 1); if (rc) { c->in = before; return rc; } }
    if (!(static_cast<const SourceShape &>(next) == before)) {      // planes prefetched under another shape are not this shape's frame
        c->h2d_pre_valid = false;
        if (c->batch) c->batch->pre_valid = false;
    }
    return VP8HIP_OK;
}

int take_frames(vp8hip_ctx *const *m, const void *const *y, const void *const *u, const void *const *v, int n, hipStream_t s,
                const hipMemcpyKind *alone, hipEvent_t planes_read, bool tight) {
    vp8hip_ctx *c0 = m[0];
    const IntakeSettings &in = c0->in;      // (same_intake: every member's)
    { const int rc = intake_ready(m, n); if (rc) return rc; }
    SourceItem src[MAX_BATCH];
    PlanesItem wn[MAX_BATCH], cv[MAX_BATCH], orn[MAX_BATCH];
    DeinterlaceItem di[MAX_BATCH];
    const bool window = in.win_on && !tight;      // (planes that came from the host are the window already: copy_planes)
    const bool orient = in.or_turns || in.or_mirror;
    int w, h;
    size_t nb[3];
    incoming_size(c0, &w, &h);      // (the raw size: what the window, the converter and the deinterlacer work at)
    incoming_bytes(c0, nb);
    const size_t raw_at[3] = {0, nb[0], nb[0] + nb[1]};      // the raw planes end to end
    const TightI420 t = tight_i420(w, h);                    // tight I420 of the raw size (the same offsets for w x h and h x w)
    for (int i = 0; i < n; ++i) {
        next_current(m[i]);
        src[i] = SourceItem{&m[i]->cur, y[i], u[i], v[i], &m[i]->scale};
        if (window) planes_item(wn[i], m[i]->win_stage.p, raw_at, src[i].y, src[i].u, src[i].v);      // (a window: what follows reads the member's tight planes)
        if (in.src_fmt) planes_item(cv[i], m[i]->fmt_stage.p, t.off, src[i].y, src[i].u, src[i].v);      // (a source format: ... the member's converted planes)
        (void)deinterlace_item(m[i], s, di[i], src[i].y, src[i].u, src[i].v);      // (a deinterlacer: ... the member's deinterlaced planes)
        if (orient) planes_item(orn[i], m[i]->or_stage.p, t.off, src[i].y, src[i].u, src[i].v);      // (an orientation: ... the member's upright planes)
    }
    if (window) {      // one launch for all members, in front of everything else
        Timed t(c0, VP8HIP_K_PACK);
        size_t off[3];
        int32_t rb[3], rows[3];
        if (window_rule(c0, off, rb, rows) != 0) return VP8HIP_ERR_ARG;
        launch_window_batch(s, off, in.win_pitch, rb, rows, wn, n);
    }
    if (in.src_fmt) {      // one launch for all members, in front of the pack or scale launch
        Timed t(c0, VP8HIP_K_PACK);     // (the input side's stage: a profile counts this launch and the pack or scale launch behind it)
        if (in.src_transfer) {     // (same_intake: one transfer and peak, so the first member's tables are every member's)
            if (!launch_tonemap_batch(s, in.src_fmt, in.src_colour, w, h, reinterpret_cast<const uint32_t *>(c0->tm_tables.p), cv, n)) return VP8HIP_ERR_ARG;
        } else if (!launch_convert_batch(s, in.src_fmt, in.src_colour, w, h, cv, n)) return VP8HIP_ERR_ARG;
    }
    if (in.di_mode) {      // ... behind the converter and in front of the pack or scale launch
        Timed t(c0, VP8HIP_K_PACK);
        launch_deinterlace_batch(s, w, h, in.di_keep, di, n);
    }
    if (orient) {      // ... behind the deinterlacer (fields are rows of the source) and in front of the pack or scale launch
        Timed t(c0, VP8HIP_K_PACK);
        launch_orient_batch(s, in.or_turns, in.or_mirror, w, h, orn, n);
    }
    if (in.in_w) {      // a frame that is scaled is not packed as well
        Timed t(c0, VP8HIP_K_PACK);
        launch_scale_batch(s, src, n);
    } else if (alone) {        // (s is the context's stream: the launch of one, or planes from the host straight into the surface)
        const int rc = set_frame_planes(c0, c0->cur, src[0].y, src[0].u, src[0].v, *alone, in.src_w, in.src_h);
        if (rc) return rc;
    } else {
        Timed t(c0, VP8HIP_K_PACK);
        static const bool skip = experiment_skip("pack");      // timing experiment only: the batches' pack
        if (!skip) launch_pack_batch(s, src, n, in.src_w, in.src_h);
    }
    return finish_frames(m, n, s, planes_read);
}

int finish_frames(vp8hip_ctx *const *m, int n, hipStream_t s, hipEvent_t planes_read) {
    vp8hip_ctx *c0 = m[0];
    const IntakeSettings &in = c0->in;      // (same_intake: every member's)
    if (planes_read) HIPCHK(c0, hipEventRecord(planes_read, s));
    {   // vp8hip_set_overlay_*: the members that have layers, in one launch behind the pack or scale launch and IN FRONT of the denoiser,
        // whose history is the previous current surface: everything downstream sees the composed frame, the one that is coded
        OverlayItem ov[MAX_BATCH];
        int no = 0;
        for (int i = 0; i < n; ++i)
            if (overlay_item(m[i], s, ov[no])) ++no;
        if (no) {
            int pw, ph;
            picture_size(c0, &pw, &ph);      // (same_intake: one picture size)
            Timed t(c0, VP8HIP_K_PACK);
            launch_overlay_batch(s, ov, no, pw, ph);
        }
    }
    {   // vp8hip_set_denoise: the members that have a history, in one launch behind the pack (the others' frames pass through)
        DenoiseItem dn[MAX_BATCH];
        int nd = 0;
        for (int i = 0; i < n; ++i)
            if (denoise_item(m[i], s, dn[nd])) ++nd;
        launch_denoise_batch(s, dn, nd, in.dn_level);
    }
    {   // vp8hip_set_analysis: the members' source sides in one launch behind the denoiser (the frame as the searches will read it)
        AnalysisSrcItem an[MAX_BATCH];
        int na = 0;
        for (int i = 0; i < n; ++i)
            if (analysis_src_item(m[i], s, an[na])) ++na;
        launch_analyse_src_batch(s, an, na);
    }
    {   // vp8hip_set_segment_mode, mode 2: the members' variance-adaptive maps, last (same_intake: all members or none)
        AqItem aq[MAX_BATCH];
        int nq = 0;
        for (int i = 0; i < n; ++i)
            if (aq_item(m[i], aq[nq])) ++nq;
        if (nq) {      // (two launches of the input side's stage, each with its own pair of events)
            { Timed t(c0, VP8HIP_K_PACK); launch_aq_map_batch(s, aq, nq); }
            { Timed t(c0, VP8HIP_K_PACK); launch_aq_seg_batch(s, aq, nq, in.seg_strength); }
        }
    }
    return VP8HIP_OK;
}

// one context's new current frame on its own stream; planes from the host that a convert, deinterlace, orient or scale launch is to read,
// and the window of a surface in host memory, pass through raw_stage first (a frame larger than the surface cannot be copied into the
// surface).  tight: planes in device memory that are the window already (a prefetch's).
static int take_current(vp8hip_ctx *c, const void *y, const void *u, const void *v, hipMemcpyKind kind, hipEvent_t planes_read = nullptr, bool tight = false) {
    if (kind != hipMemcpyDeviceToDevice && needs_device_planes(c->in)) {
        size_t nb[3];
        incoming_bytes(c, nb);
        int rc = c->raw_stage.grow(c, nb[0] + nb[1] + nb[2]);
        if (!rc) rc = copy_planes(c, c->raw_stage.p, y, u, v, nb, kind, c->stream);
        if (rc) return rc;
        y = c->raw_stage.p;
        u = c->raw_stage.p + nb[0];
        v = c->raw_stage.p + nb[0] + nb[1];
        kind = hipMemcpyDeviceToDevice;
        tight = true;
    }
    // (&kind: a context on its own, and where its planes are by now -- the host's only without a format, deinterlacer or scaler)
    return take_frames(&c, &y, &u, &v, 1, c->stream, &kind, planes_read, tight);
}

// a tile's three planes of this frame: their widths, rows and pitches in bytes (0 = tight)
static void tile_planes(const vp8hip_tile &t, const vp8hip_tile_planes &p, const uint8_t *ptr[3], int32_t width[3], int32_t rows[3], int32_t pitch[3]) {
    ptr[0] = p.y; ptr[1] = p.u; ptr[2] = p.v;
    const int32_t given[3] = {p.pitch_y, p.pitch_u, p.pitch_v};
    for (int k = 0; k < 3; ++k) {
        width[k] = k ? t.in_w / 2 : t.in_w;
        rows[k] = k ? t.in_h / 2 : t.in_h;
        pitch[k] = given[k] ? given[k] : width[k];
    }
}

// one context's new current frame composed of its canvas' tiles (vp8hip_compose_current_*), on its own stream.  Tiles in host memory
// pass through raw_stage first, only their bytes, tight and end to end: one 2-D copy per plane.
static int take_composed(vp8hip_ctx *c, const vp8hip_tile_planes *src, hipMemcpyKind kind) {
    const IntakeSettings &in = c->in;
    if (!in.n_tiles) return VP8HIP_ERR_STATE;
    ComposeSource cs[VP8HIP_MAX_TILES] = {};
    size_t total = 0;
    for (int k = 0; k < in.n_tiles; ++k) {      // everything that can be refused, before anything of the context changes
        if (!src[k].y) continue;
        if (!src[k].u || !src[k].v) return VP8HIP_ERR_ARG;
        const uint8_t *ptr[3];
        int32_t width[3], rows[3];
        tile_planes(in.tile[k], src[k], ptr, width, rows, cs[k].pitch);
        for (int p = 0; p < 3; ++p) {
            if (cs[k].pitch[p] < width[p]) return VP8HIP_ERR_ARG;
            cs[k].p[p] = ptr[p];
            total += round256((size_t)width[p] * rows[p]);
        }
    }
    if (kind != hipMemcpyDeviceToDevice) {
        { const int rc = c->raw_stage.grow(c, total); if (rc) return rc; }
        uint8_t *d = c->raw_stage.p;
        for (int k = 0; k < in.n_tiles; ++k) {
            if (!src[k].y) continue;
            const uint8_t *ptr[3];
            int32_t width[3], rows[3], pitch[3];
            tile_planes(in.tile[k], src[k], ptr, width, rows, pitch);
            for (int p = 0; p < 3; ++p) {
                HIPCHK(c, hipMemcpy2DAsync(d, (size_t)width[p], ptr[p], (size_t)pitch[p], (size_t)width[p], (size_t)rows[p], kind, c->stream));
                cs[k].p[p] = d;
                cs[k].pitch[p] = width[p];
                d += round256((size_t)width[p] * rows[p]);
            }
        }
    }
    next_current(c);
    {
        int pw, ph;
        picture_size(c, &pw, &ph);
        Timed t(c, VP8HIP_K_PACK);
        launch_compose(c->stream, c->cur, c->canvas, pw, ph, cs);
    }
    return finish_frames(&c, 1, c->stream, nullptr);
}

}  // namespace vp8

extern "C" {

// The next frame's planes started on their way while the current frame is coded (vp8hip_ctx.h): tight planes of the source size, one
// copy when they lie end to end (an I420 frame as a file reader holds it), on a stream of their own into the staging buffer the pack
// of two frames ago has finished with.  Touches nothing of the frame under way.
int vp8hip_prefetch_current(vp8hip_ctx *c, const uint8_t *y, const uint8_t *u, const uint8_t *v) {
    USE_DEVICE_ONLY(c);
    if (!c || !y || !u || !v) return VP8HIP_ERR_ARG;
    if (c->in.n_tiles) return VP8HIP_ERR_STATE;      // (a canvas: frames come in through vp8hip_compose_current_*)
    size_t nb[3];      // (the planes of the context's source format: ny, nc, nc for I420)
    incoming_bytes(c, nb);
    const size_t total = nb[0] + nb[1] + nb[2];
    if (!c->h2d_stream) {
        HIPCHK(c, hipStreamCreateWithFlags(&c->h2d_stream, hipStreamNonBlocking));
        HIPCHK(c, hipEventCreateWithFlags(&c->ev_h2d, hipEventDisableTiming));
        HIPCHK(c, hipEventCreateWithFlags(&c->ev_stage_read[0], hipEventDisableTiming));
        HIPCHK(c, hipEventCreateWithFlags(&c->ev_stage_read[1], hipEventDisableTiming));
    }
    if (c->h2d_stage[0].bytes != total || c->h2d_stage[1].bytes != total) {     // first use, or the source size has changed: whatever still reads the old buffers ends first
        { const int rc = quiesce_intake(c); if (rc) return rc; }
        for (int k = 0; k < 2; ++k) {
            c->h2d_stage[k].release();
            const int rc = c->h2d_stage[k].grow(c, total);
            if (rc) return rc;
        }
        c->stage_read_valid[0] = c->stage_read_valid[1] = false;
    }
    const int slot = c->h2d_idx ^ 1;
    if (c->stage_read_valid[slot]) HIPCHK(c, hipStreamWaitEvent(c->h2d_stream, c->ev_stage_read[slot], 0));
    { const int rc = copy_planes(c, c->h2d_stage[slot].p, y, u, v, nb, hipMemcpyHostToDevice, c->h2d_stream); if (rc) return rc; }
    HIPCHK(c, hipEventRecord(c->ev_h2d, c->h2d_stream));
    c->h2d_pre[0] = y; c->h2d_pre[1] = u; c->h2d_pre[2] = v;
    c->h2d_pre_valid = true;
    return VP8HIP_OK;
}

int vp8hip_upload_current(vp8hip_ctx *c, const uint8_t *y, const uint8_t *u, const uint8_t *v) {
    USE_DEVICE(c);
    if (!c || !y || !u || !v) return VP8HIP_ERR_ARG;
    if (c->in.n_tiles) return VP8HIP_ERR_STATE;
    size_t nb[3];
    incoming_bytes(c, nb);
    // a prefetch counts only for the source size and format it was made for: the staging buffers hold the planes' bytes of THAT size and the pack
    // would read them with this one's offsets (vp8hip_set_source_size and vp8hip_set_source_format also drop a pending prefetch; this is the
    // second lock on the same door)
    const int next = c->h2d_idx ^ 1;
    if (c->h2d_pre_valid && c->h2d_stage[next].bytes == nb[0] + nb[1] + nb[2] && c->h2d_pre[0] == y && c->h2d_pre[1] == u && c->h2d_pre[2] == v) {
        // prefetched: the planes are in (or on their way into) the staging buffer; the pack waits for the copy, nothing is copied here
        c->h2d_pre_valid = false;
        const int slot = c->h2d_idx = next;
        HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_h2d, 0));
        const uint8_t *d = c->h2d_stage[slot].p;
        const int rc = take_current(c, d, d + nb[0], d + nb[0] + nb[1], hipMemcpyDeviceToDevice, c->ev_stage_read[slot], true);
        if (rc) return rc;
        c->stage_read_valid[slot] = true;
        HIPCHK(c, hipEventSynchronize(c->ev_h2d));      // the host's planes are the host's again when this returns (done long ago, normally)
        return VP8HIP_OK;
    }
    c->h2d_pre_valid = false;
    const int rc = take_current(c, y, u, v, hipMemcpyHostToDevice);
    if (rc) return rc;
    // pageable host memory: the call must not return while the copy still reads the host buffer
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return VP8HIP_OK;
}

int vp8hip_set_current_device(vp8hip_ctx *c, const void *y, const void *u, const void *v) {
    USE_DEVICE(c);
    if (!c || !y || !u || !v) return VP8HIP_ERR_ARG;
    if (c->in.n_tiles) return VP8HIP_ERR_STATE;
    return take_current(c, y, u, v, hipMemcpyDeviceToDevice);
}

int vp8hip_canvas_tiles(const vp8hip_ctx *c) { return c ? c->in.n_tiles : 0; }

int vp8hip_compose_current_device(vp8hip_ctx *c, const vp8hip_tile_planes *src) {
    USE_DEVICE(c);
    if (!c || !src) return VP8HIP_ERR_ARG;
    return take_composed(c, src, hipMemcpyDeviceToDevice);
}

int vp8hip_compose_current_host(vp8hip_ctx *c, const vp8hip_tile_planes *src) {
    USE_DEVICE(c);
    if (!c || !src) return VP8HIP_ERR_ARG;
    const int rc = take_composed(c, src, hipMemcpyHostToDevice);
    if (rc) return rc;
    // pageable host memory: the call must not return while a copy still reads the host's planes
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return VP8HIP_OK;
}

int vp8hip_set_canvas(vp8hip_ctx *c, const vp8hip_tile *tiles, int n, int bg_y, int bg_u, int bg_v) {
    if (!c || n < 0 || n > VP8HIP_MAX_TILES || (n && !tiles)) return VP8HIP_ERR_ARG;
    IntakeSettings next = c->in;
    next.n_tiles = n;
    next.bg[0] = bg_y; next.bg[1] = bg_u; next.bg[2] = bg_v;
    for (int k = 0; k < n; ++k) next.tile[k] = tiles[k];
    next = canonical(next, c->W, c->H);
    if (intake_valid(c->W, c->H, next) != VP8HIP_OK) return VP8HIP_ERR_ARG;      // (here too: the plan below is made of arguments that passed)
    // a batch's ways in and a by-reference split take one source per frame
    if (n && (c->batch || c->shard_comm)) return VP8HIP_ERR_STATE;
    if (next == c->in) return VP8HIP_OK;
    // everything that can be refused is tried before anything of the context changes
    ComposePlan plan;
    if (n) {
        std::vector<uint8_t> blob;
        if (!compose_plan_make(&plan, next.tile, n, next.bg, blob)) return VP8HIP_ERR_ARG;
        (void)hipSetDevice(c->device);
        HIPCHK(c, hipMalloc(&plan.d_blob, blob.size()));
        const hipError_t e = hipMemcpy(plan.d_blob, blob.data(), blob.size(), hipMemcpyHostToDevice);
        if (e != hipSuccess) { (void)hipFree(plan.d_blob); c->last_hip_error = (int)e; return VP8HIP_ERR_HIP; }
    }
    const int rc = intake_apply(c, next);
    if (rc) { (void)hipFree(plan.d_blob); return rc; }
    (void)hipFree(c->canvas.d_blob);      // (nothing in flight reads the old blob: intake_apply has waited)
    c->canvas = plan;
    return VP8HIP_OK;
}

int vp8hip_set_source_size(vp8hip_ctx *c, int src_width, int src_height) {
    if (!c) return VP8HIP_ERR_ARG;
    IntakeSettings next = c->in;      // (a source size takes the scaler out)
    next.src_w = src_width;
    next.src_h = src_height;
    next.in_w = next.in_h = 0;
    const int rc = intake_apply(c, canonical(next, c->W, c->H));
    if (!rc && c->scale.d_blob) {      // (nothing in flight reads the tables: intake_apply has waited) the plan goes with the scaler
        (void)hipFree(c->scale.d_blob);
        c->scale = ScalePlan{};
    }
    return rc;
}

int vp8hip_set_source_scaling(vp8hip_ctx *c, int in_width, int in_height, int dst_width, int dst_height, int filter) {
    if (!c) return VP8HIP_ERR_ARG;
    if (!in_width && !in_height && !dst_width && !dst_height) return vp8hip_set_source_size(c, 0, 0);
    if (in_width <= 0 || in_height <= 0 || !source_size_ok(c->W, c->H, dst_width, dst_height)) return VP8HIP_ERR_ARG;
    IntakeSettings next = c->in;
    next.src_w = dst_width;
    next.src_h = dst_height;
    next.in_w = in_width;
    next.in_h = in_height;
    next.scale_kind = filter;
    next = canonical(next, c->W, c->H);
    if (intake_valid(c->W, c->H, next) != VP8HIP_OK) return VP8HIP_ERR_ARG;      // (here too: the plan below is made of arguments that passed)
    if (in_width == dst_width && in_height == dst_height) return vp8hip_set_source_size(c, dst_width, dst_height);
    if (next == c->in) return VP8HIP_OK;
    // everything that can be refused is tried before anything of the context changes
    ScalePlan plan;
    std::vector<uint8_t> blob;
    if (!scale_plan_make(&plan, in_width, in_height, dst_width, dst_height, c->W, c->H, filter, blob)) return VP8HIP_ERR_ARG;
    (void)hipSetDevice(c->device);
    HIPCHK(c, hipMalloc(&plan.d_blob, blob.size()));
    const hipError_t e = hipMemcpy(plan.d_blob, blob.data(), blob.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)hipFree(plan.d_blob); c->last_hip_error = (int)e; return VP8HIP_ERR_HIP; }
    const int rc = intake_apply(c, next);
    if (rc) { (void)hipFree(plan.d_blob); return rc; }
    (void)hipFree(c->scale.d_blob);      // (nothing in flight reads the old tables: intake_apply has waited)
    c->scale = plan;
    return VP8HIP_OK;
}

int vp8hip_set_source_transfer(vp8hip_ctx *c, int transfer, int peak) {
    if (!c) return VP8HIP_ERR_ARG;
    IntakeSettings next = c->in;
    next.src_transfer = transfer;
    next.src_peak = peak;      // (off has no peak: canonical)
    next = canonical(next, c->W, c->H);
    if (next == c->in) return VP8HIP_OK;
    DeviceBuf tables;      // the new transfer's, in a buffer of their own: a launch in flight reads the old ones, and a refusal keeps them
    if (next.src_transfer) {
        std::vector<uint8_t> t(TONEMAP_TABLE_BYTES);
        uint32_t *lin = reinterpret_cast<uint32_t *>(t.data());
        if (vp8host_tonemap_tables(transfer, peak, lin, lin + 4096, t.data() + 32768, t.data() + 36864) != 0) return VP8HIP_ERR_ARG;
        { const int rc = tables.grow(c, t.size()); if (rc) return rc; }
        const hipError_t e = hipMemcpy(tables.p, t.data(), t.size(), hipMemcpyHostToDevice);
        if (e != hipSuccess) { tables.release(); c->last_hip_error = (int)e; return VP8HIP_ERR_HIP; }
    }
    const int rc = intake_apply(c, next);
    if (rc) { tables.release(); return rc; }
    c->tm_tables.release();      // (nothing in flight reads them: intake_apply has waited)
    c->tm_tables = tables;
    return VP8HIP_OK;
}

int vp8hip_set_source_format(vp8hip_ctx *c, int format) {
    if (!c) return VP8HIP_ERR_ARG;
    IntakeSettings next = c->in;      // (a transfer in force: P010, I010, or back to I420; a window in force: its pitches under the new format)
    next.src_fmt = format;
    return intake_apply(c, next);
}

int vp8hip_set_source_colour(vp8hip_ctx *c, int matrix) {
    if (!c) return VP8HIP_ERR_ARG;
    IntakeSettings next = c->in;
    next.src_colour = matrix;
    return intake_apply(c, next);
}

}  // extern "C"
