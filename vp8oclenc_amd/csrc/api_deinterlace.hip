// api_deinterlace.hip -- interlaced source frames made progressive (vp8hip_set_deinterlace): the switch, the history's restart, the
// buffers, the record of the last frame taken in, and the item of the launch in front of every pack or scale launch (k_deinterlace_b,
// kernels_deinterlace.hip).
//
// Mode 2's history is the frame as the deinterlacer RECEIVED it, so it needs buffers of its own: two, tight, of the incoming size; the
// launch reads one and writes the frame verbatim into the other, and they trade places with every frame taken in.
#include "vp8hip_ctx.h"

using namespace vp8;

namespace vp8 {

int deinterlace_ready(vp8hip_ctx *c) {
    if (!c->in.di_mode) return VP8HIP_OK;
    int w, h;
    incoming_size(c, &w, &h);
    const size_t need = tight_i420(w, h).bytes;      // (first use, or the incoming size has grown: not a per-frame event)
    { const int rc = c->di_stage.grow(c, need); if (rc) return rc; }
    if (c->in.di_mode == 2 && need > c->di_hist[0].bytes) {      // the two histories: both or neither
        DeviceBuf d[2];
        int rc = d[0].grow(c, need);
        if (!rc) rc = d[1].grow(c, need);
        if (rc) { d[0].release(); return rc; }
        for (int k = 0; k < 2; ++k) {
            c->di_hist[k].release();
            c->di_hist[k] = d[k];
        }
        c->di_have_history = false;
    }
    return VP8HIP_OK;
}

bool deinterlace_item(vp8hip_ctx *c, hipStream_t s, DeinterlaceItem &it, const void *&y, const void *&u, const void *&v) {
    if (!c->in.di_mode) return false;
    int w, h;
    incoming_size(c, &w, &h);
    const TightI420 t = tight_i420(w, h);
    const uint8_t *src[3] = {static_cast<const uint8_t *>(y), static_cast<const uint8_t *>(u), static_cast<const uint8_t *>(v)};
    const bool adaptive = c->in.di_mode == 2;
    const bool have = adaptive && c->di_have_history && c->di_hist_w == w && c->di_hist_h == h;
    for (int p = 0; p < 3; ++p) {
        it.src[p] = src[p];
        it.dst[p] = c->di_stage.p + t.off[p];
        it.hist[p] = have ? c->di_hist[c->di_idx].p + t.off[p] : nullptr;
        it.keep_hist[p] = adaptive ? c->di_hist[c->di_idx ^ 1].p + t.off[p] : nullptr;
    }
    if (adaptive) {      // the frame as received is the history from now on
        c->di_idx ^= 1;
        c->di_have_history = true;
        c->di_hist_w = w;
        c->di_hist_h = h;
    }
    it.word = reinterpret_cast<unsigned long long *>(c->di.d);
    it.host = c->di.h;
    it.seq = ++c->di.seq;
    it.frame_number = c->cur_count - 1;
    c->di.stream = s;
    c->di_taken = true;
    y = it.dst[0]; u = it.dst[1]; v = it.dst[2];
    return true;
}

}  // namespace vp8

extern "C" {

int vp8hip_set_deinterlace(vp8hip_ctx *c, int mode, int keep) {
    if (!c) return VP8HIP_ERR_ARG;
    IntakeSettings next = c->in;
    next.di_mode = mode;
    next.di_keep = keep;      // (off has no parity: canonical; the parity itself is judged as given)
    if (intake_valid(c->W, c->H, next) != VP8HIP_OK) return VP8HIP_ERR_ARG;      // (here, not only in intake_apply: before canonical drops the parity of "off")
    next = canonical(next, c->W, c->H);
    USE_DEVICE(c);
    if (next == c->in) return VP8HIP_OK;
    if (mode) { const int rc = c->di.make(c, 256, 256); if (rc) return rc; }
    { const int rc = intake_apply(c, next); if (rc) return rc; }
    c->di_have_history = false;
    c->di_taken = false;
    return VP8HIP_OK;
}

int vp8hip_deinterlace_restart(vp8hip_ctx *c) {
    if (!c) return VP8HIP_ERR_ARG;
    c->di_have_history = false;
    return VP8HIP_OK;
}

int vp8hip_deinterlace_result(vp8hip_ctx *c, vp8hip_deinterlace_stats *s) {
    USE_DEVICE_ONLY(c);
    if (!c || !s) return VP8HIP_ERR_ARG;
    if (!c->in.di_mode || !c->di_taken) return VP8HIP_ERR_STATE;
    const int rc = c->di.wait(c);
    if (rc) return rc;
    const DeinterlaceMirror m = *c->di.h;
    s->frame_number = m.frame_number;
    s->woven = m.woven;
    s->missing = m.missing;
    return VP8HIP_OK;
}

}  // extern "C"
