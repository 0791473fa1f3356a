// api_denoise.hip -- temporal noise reduction of the source frames (vp8hip_set_denoise): the switch, the history's restart, the
// record of the last frame taken in, and the launch behind every pack (k_denoise_b, kernels_denoise.hip).
//
// The history needs no buffer of its own: a context's two current surfaces trade places with every frame taken in, so the surface the
// new frame is NOT packed into holds the previous frame as it left the denoiser (or as it passed through).
#include "vp8hip_ctx.h"

using namespace vp8;

namespace vp8 {

bool denoise_item(vp8hip_ctx *c, hipStream_t s, DenoiseItem &it) {
    if (!c->dn_level) return false;
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
    it.word = c->d_dn;
    it.host = c->h_dn;
    it.seq = ++c->dn_seq;
    it.frame_number = c->cur_count - 1;
    c->dn_stream = s;
    return true;
}

void denoise_current(vp8hip_ctx *c) {
    DenoiseItem it;
    if (denoise_item(c, c->stream, it)) launch_denoise_batch(c->stream, &it, 1, c->dn_level);
}

namespace {

// the last launch's record is complete (its seq is there); polled like the quality record, with the stream's liveness looked at now and then
int denoise_wait(vp8hip_ctx *c) {
    const uint32_t want = c->dn_seq;
    for (unsigned spins = 0; __atomic_load_n(&c->h_dn->seq, __ATOMIC_ACQUIRE) != want; ++spins) {
        if ((spins & 0xfff) == 0xfff) {
            const hipError_t q = hipStreamQuery(c->dn_stream);
            if (q != hipErrorNotReady && __atomic_load_n(&c->h_dn->seq, __ATOMIC_ACQUIRE) != want) {
                if (q != hipSuccess) { c->last_hip_error = (int)q; return VP8HIP_ERR_HIP; }
                return VP8HIP_ERR_TIMEOUT;   // the stream is idle and the word never came
            }
        }
        __builtin_ia32_pause();
    }
    return VP8HIP_OK;
}

}  // namespace

}  // namespace vp8

extern "C" {

int vp8hip_set_denoise(vp8hip_ctx *c, int level) {
    if (!c || level < 0 || level > 3) return VP8HIP_ERR_ARG;
    USE_DEVICE(c);
    if (level == c->dn_level) return VP8HIP_OK;
    // a launch still in flight reads the level's history and writes the record: it ends first (not a per-frame call)
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->lf_stream) HIPCHK(c, hipStreamSynchronize(c->lf_stream));
    if (c->batch && c->batch->prep) HIPCHK(c, hipStreamSynchronize(c->batch->prep));
    if (level && !c->d_dn) {
        unsigned long long *d = nullptr;
        DenoiseMirror *h = nullptr;
        HIPCHK(c, hipMalloc(&d, 256));
        hipError_t e = hipMemset(d, 0, 256);
        if (e == hipSuccess) e = hipHostMalloc(&h, sizeof(DenoiseMirror), hipHostMallocCoherent);
        if (e != hipSuccess) { (void)hipFree(d); c->last_hip_error = (int)e; return VP8HIP_ERR_HIP; }
        memset(h, 0, sizeof(*h));
        c->d_dn = d;
        c->h_dn = h;
    }
    c->dn_level = level;
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
    if (!c->dn_level || !c->dn_taken) return VP8HIP_ERR_STATE;
    DenoiseMirror m = c->dn_passed;
    if (!c->dn_host) {
        const int rc = denoise_wait(c);
        if (rc) return rc;
        m = *c->h_dn;
    }
    s->frame_number = m.frame_number;
    s->mbs_filtered = m.mbs_filtered;
    s->mbs_total = m.mbs_total;
    return VP8HIP_OK;
}

}  // extern "C"
