// api_geometry.hip -- the two geometric stages of the input side: the window of a pitched surface (vp8hip_set_source_window; k_window_b
// in front of everything, or 2-D copies for planes from the host) and quarter turns with a mirror (vp8hip_set_source_orientation;
// k_orient_b behind the deinterlacer): the setters.  The staging buffers are intake_ready's and the launches take_frames'
// (api_intake.hip; kernels_geometry.hip).  Neither has a history or a record.
#include "vp8hip_ctx.h"

using namespace vp8;

extern "C" {

int vp8hip_set_source_window(vp8hip_ctx *c, const int32_t *pitch, int x, int y) {
    if (!c) return VP8HIP_ERR_ARG;
    IntakeSettings next = c->in;
    next.win_on = pitch != nullptr;
    next.win_x = x;
    next.win_y = y;
    for (int p = 0; p < 3; ++p) next.win_pitch[p] = pitch ? pitch[p] : 0;
    if (pitch) {      // (entries of planes the format lacks are ignored)
        size_t off[3];
        int32_t rb[3], rows[3];
        if (window_rule(next, c->W, c->H, off, rb, rows) != 0) return VP8HIP_ERR_ARG;
        for (int p = 0; p < 3; ++p)
            if (!rows[p]) next.win_pitch[p] = 0;
    }
    USE_DEVICE(c);
    return intake_apply(c, canonical(next, c->W, c->H));
}

int vp8hip_set_source_orientation(vp8hip_ctx *c, int turns, int mirror) {
    if (!c) return VP8HIP_ERR_ARG;
    IntakeSettings next = c->in;
    next.or_turns = turns;
    next.or_mirror = mirror;
    USE_DEVICE(c);
    return intake_apply(c, next);
}

}  // extern "C"
