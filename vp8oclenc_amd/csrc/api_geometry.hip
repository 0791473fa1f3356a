// api_geometry.hip -- the two geometric stages of the input side: the window of a pitched surface (vp8hip_set_source_window; k_window_b
// in front of everything, or 2-D copies for planes from the host) and quarter turns with a mirror (vp8hip_set_source_orientation;
// k_orient_b behind the deinterlacer): the switches, the staging buffers and the items of the two launches (kernels_geometry.hip;
// take_frames launches them).  Neither has a history or a record.
#include "vp8hip_ctx.h"

using namespace vp8;

namespace vp8 {

int window_rule(const vp8hip_ctx *c, size_t off[3], int32_t row_bytes[3], int32_t rows[3]) {
    int w, h;
    incoming_size(c, &w, &h);
    return vp8host_source_window(c->src_fmt, w, h, c->win_x, c->win_y, c->win_pitch, off, row_bytes, rows);
}

bool geometry_allows(const vp8hip_ctx *c, int format, int upright_w, int upright_h, int turns) {
    const int w = (turns & 1) ? upright_h : upright_w, h = (turns & 1) ? upright_w : upright_h;
    if (c->di_mode && h < 4) return false;      // (the deinterlacer needs a row of each field in every plane)
    if (!c->win_on) return true;
    size_t off[3];
    int32_t rb[3], rows[3];
    return vp8host_source_window(format, w, h, c->win_x, c->win_y, c->win_pitch, off, rb, rows) == 0;
}

int geometry_ready(vp8hip_ctx *c) {
    if (c->win_on) {
        size_t off[3], nb[3];
        int32_t rb[3], rows[3];
        if (window_rule(c, off, rb, rows) != 0) return VP8HIP_ERR_ARG;
        incoming_bytes(c, nb);
        const int rc = c->win_stage.grow(c, nb[0] + nb[1] + nb[2]);      // (first use, or the incoming size has grown: not a per-frame event)
        if (rc) return rc;
    }
    if (c->or_turns || c->or_mirror) {
        int w, h;
        incoming_size(c, &w, &h);
        const int rc = c->or_stage.grow(c, tight_i420(w, h).bytes);
        if (rc) return rc;
    }
    return VP8HIP_OK;
}

bool window_item(vp8hip_ctx *c, GeometryItem &it, const void *&y, const void *&u, const void *&v) {
    if (!c->win_on) return false;
    size_t nb[3];
    incoming_bytes(c, nb);
    const void *src[3] = {y, u, v};
    const size_t at[3] = {0, nb[0], nb[0] + nb[1]};
    for (int p = 0; p < 3; ++p) {
        it.src[p] = static_cast<const uint8_t *>(src[p]);
        it.dst[p] = c->win_stage.p + at[p];
    }
    y = it.dst[0]; u = it.dst[1]; v = it.dst[2];
    return true;
}

bool orient_item(vp8hip_ctx *c, GeometryItem &it, const void *&y, const void *&u, const void *&v) {
    if (!c->or_turns && !c->or_mirror) return false;
    int w, h;
    incoming_size(c, &w, &h);
    const TightI420 t = tight_i420(w, h);      // (the same offsets for w x h and h x w)
    const void *src[3] = {y, u, v};
    for (int p = 0; p < 3; ++p) {
        it.src[p] = static_cast<const uint8_t *>(src[p]);
        it.dst[p] = c->or_stage.p + t.off[p];
    }
    y = it.dst[0]; u = it.dst[1]; v = it.dst[2];
    return true;
}

// planes prefetched under other settings are handed over again
static void drop_prefetch(vp8hip_ctx *c) {
    c->h2d_pre_valid = false;
    if (c->batch) c->batch->pre_valid = false;
}

}  // namespace vp8

extern "C" {

int vp8hip_set_source_window(vp8hip_ctx *c, const int32_t *pitch, int x, int y) {
    if (!c) return VP8HIP_ERR_ARG;
    int32_t pt[3] = {0, 0, 0};
    if (pitch) {      // everything that can be refused is tried before anything of the context changes
        int w, h;
        incoming_size(c, &w, &h);
        size_t off[3];
        int32_t rb[3], rows[3];
        if (vp8host_source_window(c->src_fmt, w, h, x, y, pitch, off, rb, rows) != 0) return VP8HIP_ERR_ARG;
        for (int p = 0; p < 3; ++p) pt[p] = rows[p] ? pitch[p] : 0;      // (entries of planes the format lacks are ignored)
    } else {
        x = y = 0;
    }
    USE_DEVICE(c);
    if ((pitch != nullptr) == c->win_on && pt[0] == c->win_pitch[0] && pt[1] == c->win_pitch[1] && pt[2] == c->win_pitch[2] && x == c->win_x && y == c->win_y)
        return VP8HIP_OK;
    // a launch still in flight reads the staging buffer: it ends first (not a per-frame call)
    { const int rc = quiesce_intake(c); if (rc) return rc; }
    const bool on_before = c->win_on;
    const int32_t pt_before[3] = {c->win_pitch[0], c->win_pitch[1], c->win_pitch[2]};
    const int x_before = c->win_x, y_before = c->win_y;
    c->win_on = pitch != nullptr;
    for (int p = 0; p < 3; ++p) c->win_pitch[p] = pt[p];
    c->win_x = x;
    c->win_y = y;
    const int rc = geometry_ready(c);
    if (rc) {
        c->win_on = on_before;
        for (int p = 0; p < 3; ++p) c->win_pitch[p] = pt_before[p];
        c->win_x = x_before;
        c->win_y = y_before;
        return rc;
    }
    drop_prefetch(c);
    return VP8HIP_OK;
}

int vp8hip_set_source_orientation(vp8hip_ctx *c, int turns, int mirror) {
    if (!c || turns < 0 || turns > 3 || (mirror != 0 && mirror != 1)) return VP8HIP_ERR_ARG;
    int w, h;
    upright_size(c, &w, &h);
    if (!geometry_allows(c, c->src_fmt, w, h, turns)) return VP8HIP_ERR_ARG;
    USE_DEVICE(c);
    if (turns == c->or_turns && mirror == c->or_mirror) return VP8HIP_OK;
    { const int rc = quiesce_intake(c); if (rc) return rc; }
    const int turns_before = c->or_turns, mirror_before = c->or_mirror;
    c->or_turns = turns;
    c->or_mirror = mirror;
    const int rc = geometry_ready(c);
    if (rc) { c->or_turns = turns_before; c->or_mirror = mirror_before; return rc; }
    drop_prefetch(c);
    return VP8HIP_OK;
}

}  // extern "C"
