// api_overlay.hip -- layers burnt into the source frames (vp8hip_set_overlay_host / _device, vp8hip_set_overlay_placement,
// vp8hip_clear_overlay): the slots, their retained pixels and prepared planes, and the item of the launch behind every pack or scale
// launch (k_overlay_b, kernels_overlay.hip; take_frames launches it, in front of the denoiser).
//
// A setter copies the layer's pixels into the slot and marks its planes stale; the intake that follows launches k_overlay_prepare in
// front of k_overlay_b on ITS stream, so the copy (on the same stream), the prepare launch and the frames' launches are ordered by
// the stream alone and a subtitle can change between two frames of a live batch without a host wait -- unless a buffer has to grow
// (DeviceBuf::grow quiesces), the pixels come from pageable host memory (the caller's buffer is free when the call returns), or the
// context has a loop filter stream of its own (vp8hip_filter_overlap: its intake stream changes from frame to frame).
#include "vp8hip_ctx.h"

using namespace vp8;

namespace vp8 {

static hipStream_t overlay_stream(const vp8hip_ctx *c) {      // the stream the context's frames are taken in on
    if (c->batch) return c->batch->prep ? c->batch->prep : c->batch->stream;
    return c->stream;
}

// the planes' bytes at the placement that needs most: a move or a fade never grows the buffer
static size_t planes_room(int lw, int lh) {
    size_t most = 0;
    for (int x = 0; x < 8; ++x)
        for (int y = 0; y < 2; ++y) {
            const size_t b = overlay_planes(lw, lh, x, y).bytes;
            most = b > most ? b : most;
        }
    return most;
}

bool overlay_item(vp8hip_ctx *c, hipStream_t s, OverlayItem &it) {
    if (!c->ov_count) return false;
    int pw, ph;
    picture_size(c, &pw, &ph);
    it.y = c->cur.Y[0];
    it.u = c->cur.U;
    it.v = c->cur.V;
    it.n = 0;
    int bx0 = INT_MAX, by0 = INT_MAX, bx1 = 0, by1 = 0;
    for (int k = 0; k < VP8HIP_MAX_OVERLAYS; ++k) {
        vp8hip_ctx::OverlaySlot &o = c->ov[k];
        if (!o.set) continue;
        const int x0 = o.x > 0 ? o.x : 0, y0 = o.y > 0 ? o.y : 0, x1 = o.x + o.lw < pw ? o.x + o.lw : pw, y1 = o.y + o.lh < ph ? o.y + o.lh : ph;
        if (x0 >= x1 || y0 >= y1) continue;      // (wholly outside the picture: its planes stay as they are)
        if (o.stale) {
            if (!launch_overlay_prepare(s, o.format, o.matrix, o.pixels.p, o.lw, o.lh, o.x, o.y, o.opacity, o.planes.p)) continue;
            o.stale = false;
        }
        const OverlayPlanes p = overlay_planes(o.lw, o.lh, o.x, o.y);
        it.layer[it.n++] = OverlayLayer{o.planes.p, p.off_e, p.off_E, p.off_tu, p.off_tv, p.X0, o.y, p.lstride, o.lh, p.CX0, p.cy0, p.cstride, p.crows};
        bx0 = x0 < bx0 ? x0 : bx0; by0 = y0 < by0 ? y0 : by0;
        bx1 = x1 > bx1 ? x1 : bx1; by1 = y1 > by1 ? y1 : by1;
    }
    if (!it.n) return false;
    // the padding behind the last column and row repeats them -- in chroma the sample of the last TWO luma columns or rows
    if (bx1 >= pw - 1) bx1 = c->W;
    if (by1 >= ph - 1) by1 = c->H;
    it.ux0 = bx0 >> 3; it.ux1 = (bx1 + 7) >> 3;
    it.uy0 = by0 >> 1; it.uy1 = (by1 + 1) >> 1;
    return true;
}

void overlay_release(vp8hip_ctx *c) {
    for (vp8hip_ctx::OverlaySlot &o : c->ov) {
        o.pixels.release();
        o.planes.release();
        o.set = false;
    }
    c->ov_count = 0;
}

static bool placement_ok(int x, int y, int opacity) {
    return x >= -VP8HOST_OVERLAY_MAX_POS && x <= VP8HOST_OVERLAY_MAX_POS && y >= -VP8HOST_OVERLAY_MAX_POS && y <= VP8HOST_OVERLAY_MAX_POS && opacity >= 0 && opacity <= 255;
}

// what is in flight may read the slot's buffers on a stream that is not the next intake's: a context with a loop filter stream
static int overlay_settle(vp8hip_ctx *c) { return !c->batch && c->lf_stream ? quiesce_intake(c) : VP8HIP_OK; }

static int set_overlay(vp8hip_ctx *c, int slot, int format, int matrix, const void *pixels, int lw, int lh, int pitch, int x, int y, int opacity, hipMemcpyKind kind) {
    if (!c || slot < 0 || slot >= VP8HIP_MAX_OVERLAYS || (format != VP8HOST_FORMAT_BGRA && format != VP8HOST_FORMAT_RGBA) || matrix < 0 ||
        matrix >= VP8HOST_COLOUR_COUNT || !pixels || lw < 1 || lh < 1 || lw > VP8HOST_OVERLAY_MAX_SIZE || lh > VP8HOST_OVERLAY_MAX_SIZE || pitch < 4 * lw ||
        !placement_ok(x, y, opacity))
        return VP8HIP_ERR_ARG;
    if (c->shard_comm) return VP8HIP_ERR_STATE;      // (a frame split by reference over devices: each rank takes its frames in on its own)
    USE_DEVICE(c);
    { const int rc = overlay_settle(c); if (rc) return rc; }
    vp8hip_ctx::OverlaySlot &o = c->ov[slot];
    // the planes first: they are made again from the pixels anyway, so a pixel buffer that cannot grow leaves the old layer whole
    const bool planes_grow = planes_room(lw, lh) > o.planes.bytes;
    { const int rc = o.planes.grow(c, planes_room(lw, lh)); if (rc) return rc; }
    if (planes_grow) o.stale = true;
    { const int rc = o.pixels.grow(c, (size_t)lw * (size_t)lh * 4); if (rc) return rc; }
    hipStream_t s = overlay_stream(c);
    HIPCHK(c, hipMemcpy2DAsync(o.pixels.p, (size_t)lw * 4, pixels, (size_t)pitch, (size_t)lw * 4, (size_t)lh, kind, s));
    if (kind != hipMemcpyDeviceToDevice || (!c->batch && c->lf_stream)) HIPCHK(c, hipStreamSynchronize(s));
    if (!o.set) ++c->ov_count;
    o.set = true;
    o.stale = true;
    o.format = format; o.matrix = matrix; o.lw = lw; o.lh = lh; o.x = x; o.y = y; o.opacity = opacity;
    return VP8HIP_OK;
}

}  // namespace vp8

extern "C" {

int vp8hip_set_overlay_host(vp8hip_ctx *c, int slot, int format, int matrix, const uint8_t *pixels, int lw, int lh, int pitch, int x, int y, int opacity) {
    return set_overlay(c, slot, format, matrix, pixels, lw, lh, pitch, x, y, opacity, hipMemcpyHostToDevice);
}

int vp8hip_set_overlay_device(vp8hip_ctx *c, int slot, int format, int matrix, const void *pixels, int lw, int lh, int pitch, int x, int y, int opacity) {
    return set_overlay(c, slot, format, matrix, pixels, lw, lh, pitch, x, y, opacity, hipMemcpyDeviceToDevice);
}

int vp8hip_set_overlay_placement(vp8hip_ctx *c, int slot, int x, int y, int opacity) {
    if (!c || slot < 0 || slot >= VP8HIP_MAX_OVERLAYS || !c->ov[slot].set || !placement_ok(x, y, opacity)) return VP8HIP_ERR_ARG;
    if (c->shard_comm) return VP8HIP_ERR_STATE;
    USE_DEVICE(c);
    { const int rc = overlay_settle(c); if (rc) return rc; }
    vp8hip_ctx::OverlaySlot &o = c->ov[slot];
    if (x == o.x && y == o.y && opacity == o.opacity) return VP8HIP_OK;
    o.x = x; o.y = y; o.opacity = opacity;
    o.stale = true;      // (the planes have room for any placement: the next intake prepares them again, behind the frames that read them)
    return VP8HIP_OK;
}

int vp8hip_clear_overlay(vp8hip_ctx *c, int slot) {
    if (!c || slot < -1 || slot >= VP8HIP_MAX_OVERLAYS || (slot >= 0 && !c->ov[slot].set)) return VP8HIP_ERR_ARG;
    if (c->shard_comm) return VP8HIP_ERR_STATE;
    if (!c->ov_count) return VP8HIP_OK;      // (slot -1 on a context without a layer)
    USE_DEVICE(c);
    { const int rc = quiesce_intake(c); if (rc) return rc; }      // a launch in flight reads the buffers: it ends first
    for (int k = 0; k < VP8HIP_MAX_OVERLAYS; ++k) {
        vp8hip_ctx::OverlaySlot &o = c->ov[k];
        if (!o.set || (slot >= 0 && k != slot)) continue;
        o.pixels.release();
        o.planes.release();
        o.set = o.stale = false;
        --c->ov_count;
    }
    return VP8HIP_OK;
}

int vp8hip_overlay_count(const vp8hip_ctx *c) { return c ? c->ov_count : 0; }

}  // extern "C"
