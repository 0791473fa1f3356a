// api_arf.hip -- the hidden alternate reference frame's source side (vp8hip_arf_filter_device / _host): the temporal filter over the
// caller's window (k_arf_filter_b, kernels_arf.hip) into a staging buffer the context owns, and the filtered frame taken in as the
// current frame through the ordinary intake (vp8hip_set_current_device: padding, scaling, orientation and the segment map see it as
// they see any source frame).  The coding side -- the reconstruction becomes ALTREF and LAST stays -- is vp8hip_loop_filter_hidden,
// api_inter.hip.
#include "vp8hip_ctx.h"

using namespace vp8;

namespace {

// what a context must not be or have for a hidden frame (include/vp8hip.h says why); the window's parameters
int arf_check(const vp8hip_ctx *c, const void *frames, int n, int centre, int strength) {
    if (!c || !frames || n < 1 || n > VP8HOST_ARF_MAX_FRAMES || centre < 0 || centre >= n || strength < 0 || strength > 6) return VP8HIP_ERR_ARG;
    if (excludes_arf(c->in)) return VP8HIP_ERR_ARG;
    if (c->batch || c->shard_comm || c->lf_overlap) return VP8HIP_ERR_STATE;
    return VP8HIP_OK;
}

}  // namespace

extern "C" {

int vp8hip_arf_filter_device(vp8hip_ctx *c, const void *const (*frames)[3], int n, int centre, int strength) {
    { const int rc = arf_check(c, frames, n, centre, strength); if (rc) return rc; }
    for (int k = 0; k < n; ++k)
        if (!frames[k][0] || !frames[k][1] || !frames[k][2]) return VP8HIP_ERR_ARG;
    USE_DEVICE(c);
    int w, h;
    incoming_size(c, &w, &h);
    const TightI420 t = tight_i420(w, h);
    { const int rc = c->arf_stage.grow(c, 256 + t.bytes); if (rc) return rc; }      // (first use, or a larger incoming size: not per frame)
    ArfItem it;
    for (int k = 0; k < VP8HOST_ARF_MAX_FRAMES; ++k)
        for (int p = 0; p < 3; ++p) it.src[k][p] = static_cast<const uint8_t *>(frames[k < n ? k : centre][p]);
    for (int p = 0; p < 3; ++p) it.dst[p] = c->arf_stage.p + 256 + t.off[p];
    it.weights = reinterpret_cast<unsigned long long *>(c->arf_stage.p);
    it.w = w;
    it.h = h;
    it.n = n;
    it.centre = centre;
    it.strength = strength;
    // (the pack of the hidden frame before read the buffer on this stream: in order behind it)
    static_assert(ARF_WEIGHT_SLOTS * sizeof(unsigned long long) <= 256, "the weight words lie in front of the staged frame");
    HIPCHK(c, hipMemsetAsync(it.weights, 0, ARF_WEIGHT_SLOTS * sizeof(unsigned long long), c->stream));
    {
        Timed tm(c, VP8HIP_K_PACK);      // (the input side's stage: a profile counts this launch with the pack or scale launch behind it)
        launch_arf_filter(c->stream, it);
    }
    HIPCHK(c, hipGetLastError());
    c->arf_w = w;
    c->arf_h = h;
    return vp8hip_set_current_device(c, it.dst[0], it.dst[1], it.dst[2]);
}

int vp8hip_arf_filter_host(vp8hip_ctx *c, const uint8_t *const (*frames)[3], int n, int centre, int strength) {
    { const int rc = arf_check(c, frames, n, centre, strength); if (rc) return rc; }
    for (int k = 0; k < n; ++k)
        if (!frames[k][0] || !frames[k][1] || !frames[k][2]) return VP8HIP_ERR_ARG;
    USE_DEVICE(c);
    int w, h;
    incoming_size(c, &w, &h);
    const TightI420 t = tight_i420(w, h);
    { const int rc = c->arf_in.grow(c, (size_t)n * t.bytes); if (rc) return rc; }
    const size_t nb[3] = {(size_t)w * h, (size_t)(w / 2) * (h / 2), (size_t)(w / 2) * (h / 2)};
    const void *dev[VP8HOST_ARF_MAX_FRAMES][3];
    for (int k = 0; k < n; ++k)
        for (int p = 0; p < 3; ++p) {
            uint8_t *d = c->arf_in.p + (size_t)k * t.bytes + t.off[p];
            HIPCHK(c, hipMemcpyAsync(d, frames[k][p], nb[p], hipMemcpyHostToDevice, c->stream));
            dev[k][p] = d;
        }
    const int rc = vp8hip_arf_filter_device(c, reinterpret_cast<const void *const (*)[3]>(dev), n, centre, strength);
    if (rc) return rc;
    // pageable host memory, and one upload buffer: the call returns when the window has been read
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return VP8HIP_OK;
}

int vp8hip_arf_result(vp8hip_ctx *c, int32_t weights[3]) {
    if (!c || !weights) return VP8HIP_ERR_ARG;
    if (!c->arf_w) return VP8HIP_ERR_STATE;
    USE_DEVICE(c);
    JOIN_LF(c);
    unsigned long long slot[ARF_WEIGHT_SLOTS], sum = 0;
    HIPCHK(c, hipMemcpyAsync(slot, c->arf_stage.p, sizeof slot, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int k = 0; k < ARF_WEIGHT_SLOTS; ++k) sum += slot[k];
    for (int b = 0; b < 3; ++b) weights[b] = (int32_t)((sum >> (21 * b)) & 0x1FFFFFull);
    return VP8HIP_OK;
}

int vp8hip_arf_release(vp8hip_ctx *c) {
    if (!c) return VP8HIP_ERR_ARG;
    if (!c->arf_stage.p && !c->arf_in.p) return VP8HIP_OK;
    USE_DEVICE(c);
    { const int rc = quiesce_intake(c); if (rc) return rc; }      // (the pack that read the staged frame has ended; the current frame is a surface of its own)
    c->arf_stage.release();
    c->arf_in.release();
    c->arf_w = c->arf_h = 0;
    return VP8HIP_OK;
}

}  // extern "C"
