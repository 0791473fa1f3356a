// api_deinterlace.hip -- interlaced source frames made progressive (vp8hip_set_deinterlace): the switch, the history's restart, the
// buffers, the record of the last frame taken in, and the item of the launch in front of every pack or scale launch (k_deinterlace_b,
// kernels_deinterlace.hip).
//
// Mode 2's history is the frame as the deinterlacer RECEIVED it, so it needs buffers of its own: two, tight, of the incoming size; the
// launch reads one and writes the frame verbatim into the other, and they trade places with every frame taken in.
#include "vp8hip_ctx.h"

using namespace vp8;

namespace vp8 {

static size_t round256(size_t n) { return (n + 255) & ~(size_t)255; }

int deinterlace_ready(vp8hip_ctx *c) {
    if (!c->di_mode) return VP8HIP_OK;
    int w, h;
    incoming_size(c, &w, &h);
    if (h < 4) return VP8HIP_ERR_ARG;
    const size_t need = round256((size_t)w * h) + 2 * round256((size_t)(w / 2) * (h / 2));
    const bool hist = c->di_mode == 2;
    if (need <= c->di_stage_bytes && (!hist || need <= c->di_hist_bytes)) return VP8HIP_OK;
    { const int rc = scale_quiesce(c); if (rc) return rc; }      // (first use, or the incoming size has grown: not a per-frame event)
    if (need > c->di_stage_bytes) {
        uint8_t *d = nullptr;
        HIPCHK(c, hipMalloc(&d, need));
        (void)hipFree(c->di_stage);
        c->di_stage = d;
        c->di_stage_bytes = need;
    }
    if (hist && need > c->di_hist_bytes) {
        uint8_t *d[2] = {nullptr, nullptr};
        HIPCHK(c, hipMalloc(&d[0], need));
        const hipError_t e = hipMalloc(&d[1], need);
        if (e != hipSuccess) { (void)hipFree(d[0]); c->last_hip_error = (int)e; return VP8HIP_ERR_HIP; }
        (void)hipFree(c->di_hist[0]);
        (void)hipFree(c->di_hist[1]);
        c->di_hist[0] = d[0];
        c->di_hist[1] = d[1];
        c->di_hist_bytes = need;
        c->di_have_history = false;
    }
    return VP8HIP_OK;
}

bool deinterlace_item(vp8hip_ctx *c, hipStream_t s, DeinterlaceItem &it, const void *&y, const void *&u, const void *&v) {
    if (!c->di_mode) return false;
    int w, h;
    incoming_size(c, &w, &h);
    const size_t oy = round256((size_t)w * h), oc = round256((size_t)(w / 2) * (h / 2));
    const size_t off[3] = {0, oy, oy + oc};
    const uint8_t *src[3] = {static_cast<const uint8_t *>(y), static_cast<const uint8_t *>(u), static_cast<const uint8_t *>(v)};
    const bool adaptive = c->di_mode == 2;
    const bool have = adaptive && c->di_have_history && c->di_hist_w == w && c->di_hist_h == h;
    for (int p = 0; p < 3; ++p) {
        it.src[p] = src[p];
        it.dst[p] = c->di_stage + off[p];
        it.hist[p] = have ? c->di_hist[c->di_idx] + off[p] : nullptr;
        it.keep_hist[p] = adaptive ? c->di_hist[c->di_idx ^ 1] + off[p] : nullptr;
    }
    if (adaptive) {      // the frame as received is the history from now on
        c->di_idx ^= 1;
        c->di_have_history = true;
        c->di_hist_w = w;
        c->di_hist_h = h;
    }
    it.word = c->d_di;
    it.host = c->h_di;
    it.seq = ++c->di_seq;
    it.frame_number = c->cur_count - 1;
    c->di_stream = s;
    c->di_taken = true;
    y = it.dst[0]; u = it.dst[1]; v = it.dst[2];
    return true;
}

namespace {

// the last launch's record is complete (its seq is there); polled like the denoiser's record
int deinterlace_wait(vp8hip_ctx *c) {
    const uint32_t want = c->di_seq;
    for (unsigned spins = 0; __atomic_load_n(&c->h_di->seq, __ATOMIC_ACQUIRE) != want; ++spins) {
        if ((spins & 0xfff) == 0xfff) {
            const hipError_t q = hipStreamQuery(c->di_stream);
            if (q != hipErrorNotReady && __atomic_load_n(&c->h_di->seq, __ATOMIC_ACQUIRE) != want) {
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

int vp8hip_set_deinterlace(vp8hip_ctx *c, int mode, int keep) {
    if (!c || mode < 0 || mode > 2 || (keep != 0 && keep != 1)) return VP8HIP_ERR_ARG;
    if (mode) {
        int w, h;
        incoming_size(c, &w, &h);
        if (h < 4) return VP8HIP_ERR_ARG;      // every plane needs a row of each field
    }
    USE_DEVICE(c);
    if (mode == c->di_mode && (!mode || keep == c->di_keep)) return VP8HIP_OK;
    // a launch still in flight reads the history and writes the record: it ends first (not a per-frame call)
    { const int rc = scale_quiesce(c); if (rc) return rc; }
    if (mode && !c->d_di) {
        unsigned long long *d = nullptr;
        DeinterlaceMirror *h = nullptr;
        HIPCHK(c, hipMalloc(&d, 256));
        hipError_t e = hipMemset(d, 0, 256);
        if (e == hipSuccess) e = hipHostMalloc(&h, sizeof(DeinterlaceMirror), hipHostMallocCoherent);
        if (e != hipSuccess) { (void)hipFree(d); c->last_hip_error = (int)e; return VP8HIP_ERR_HIP; }
        memset(h, 0, sizeof(*h));
        c->d_di = d;
        c->h_di = h;
    }
    const int mode_before = c->di_mode, keep_before = c->di_keep;
    c->di_mode = mode;
    c->di_keep = keep;
    { const int rc = deinterlace_ready(c); if (rc) { c->di_mode = mode_before; c->di_keep = keep_before; return rc; } }
    c->di_have_history = false;
    c->di_taken = false;
    c->h2d_pre_valid = false;      // planes prefetched under other settings are handed over again
    if (c->batch) c->batch->pre_valid = false;
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
    if (!c->di_mode || !c->di_taken) return VP8HIP_ERR_STATE;
    const int rc = deinterlace_wait(c);
    if (rc) return rc;
    const DeinterlaceMirror m = *c->h_di;
    s->frame_number = m.frame_number;
    s->woven = m.woven;
    s->missing = m.missing;
    return VP8HIP_OK;
}

}  // extern "C"
