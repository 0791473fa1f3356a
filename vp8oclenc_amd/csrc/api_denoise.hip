// api_denoise.hip -- temporal noise reduction of the source frames (vp8hip_set_denoise): the switch, the history's restart, the
// record of the last frame taken in, and the item of the launch behind every pack (k_denoise_b, kernels_denoise.hip; take_frames launches it).
//
// The history needs no buffer of its own: a context's two current surfaces trade places with every frame taken in, so the surface the
// new frame is NOT packed into holds the previous frame as it left the denoiser (or as it passed through).
#include "vp8hip_ctx.h"

using namespace vp8;

namespace vp8 {

bool denoise_item(vp8hip_ctx *c, hipStream_t s, DenoiseItem &it) {
    if (!c->in.dn_level) return false;
    c->dn_taken = true;
    if (!c->dn_have_history) {      // first frame, after a restart or a level change: unchanged, and the history from now on
        c->dn_have_history = true;
        c->dn_host = true;
        c->dn_passed = DenoiseMirror{c->cur_count - 1, 0, c->mbs, 0u};
        return false;
    }
    c->dn_host = false;
    it.cur = c->cur;
    it.hist = c->cur_prev;
    it.word = reinterpret_cast<unsigned long long *>(c->dn.d);
    it.host = c->dn.h;
    it.seq = ++c->dn.seq;
    it.frame_number = c->cur_count - 1;
    c->dn.stream = s;
    return true;
}

}  // namespace vp8

extern "C" {

int vp8hip_set_denoise(vp8hip_ctx *c, int level) {
    if (!c || level < 0 || level > 3) return VP8HIP_ERR_ARG;
    USE_DEVICE(c);
    if (level == c->in.dn_level) return VP8HIP_OK;
    if (level) { const int rc = c->dn.make(c, 256, 256); if (rc) return rc; }
    IntakeSettings next = c->in;
    next.dn_level = level;
    { const int rc = intake_apply(c, next); if (rc) return rc; }
    c->dn_have_history = false;
    c->dn_taken = false;
    return VP8HIP_OK;
}

int vp8hip_denoise_restart(vp8hip_ctx *c) {
    if (!c) return VP8HIP_ERR_ARG;
    c->dn_have_history = false;
    return VP8HIP_OK;
}

int vp8hip_denoise_result(vp8hip_ctx *c, vp8hip_denoise_stats *s) {
    USE_DEVICE_ONLY(c);
    if (!c || !s) return VP8HIP_ERR_ARG;
    if (!c->in.dn_level || !c->dn_taken) return VP8HIP_ERR_STATE;
    DenoiseMirror m = c->dn_passed;
    if (!c->dn_host) {
        const int rc = c->dn.wait(c);
        if (rc) return rc;
        m = *c->dn.h;
    }
    s->frame_number = m.frame_number;
    s->mbs_filtered = m.mbs_filtered;
    s->mbs_total = m.mbs_total;
    return VP8HIP_OK;
}

}  // extern "C"
