// api_segment.hip -- the per-macroblock quantiser (vp8hip_set_segment_mode): the switch, the caller's map, the item of the
// variance-adaptive map's launch (k_aq_map_b + k_aq_seg_b at the end of every intake; kernels_aq.hip), what the mapped k_mb reads,
// and the map for the host.  The rule is include/vp8hip_host.h's.
#include "vp8hip_ctx.h"

using namespace vp8;

namespace vp8 {

namespace {

size_t seg_array_bytes(const vp8hip_ctx *c) { return round256((size_t)c->mbs); }
uint32_t *aq_sum(const vp8hip_ctx *c, int slot) { return reinterpret_cast<uint32_t *>(c->seg_buf.p + 128 * slot); }
uint8_t *aq_e(const vp8hip_ctx *c, int slot) { return c->seg_buf.p + 256 + (size_t)slot * seg_array_bytes(c); }
uint8_t *aq_map(const vp8hip_ctx *c, int slot) { return c->seg_buf.p + 256 + (size_t)(2 + slot) * seg_array_bytes(c); }
uint8_t *caller_map(const vp8hip_ctx *c) { return c->seg_buf.p + 256 + 4 * seg_array_bytes(c); }

// the context's one allocation for both modes (no-op once made): the sum words zero
int segment_buffers(vp8hip_ctx *c) {
    if (c->seg_buf.p) return VP8HIP_OK;
    const int rc = c->seg_buf.grow(c, 256 + 5 * seg_array_bytes(c));
    if (rc) return rc;
    HIPCHK(c, hipMemsetAsync(c->seg_buf.p, 0, 256, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));      // (the launches that add into the words may come on another stream)
    return VP8HIP_OK;
}

// who may have a mode or a map at all
int segment_refusal(const vp8hip_ctx *c) {
    if (c->ssim_target >= 0.0f) return VP8HIP_ERR_STATE;      // (the SSIM ladder and the map both own the segment id)
    if (c->shard_comm) return VP8HIP_ERR_STATE;               // (a frame split by reference over devices)
    return VP8HIP_OK;
}

int set_map(vp8hip_ctx *c, const uint8_t *map, hipMemcpyKind kind) {
    { const int rc = segment_refusal(c); if (rc) return rc; }
    { const int rc = segment_buffers(c); if (rc) return rc; }
    HIPCHK(c, hipMemcpyAsync(caller_map(c), map, (size_t)c->mbs, kind, c->stream));
    c->seg_map_set = true;
    return VP8HIP_OK;
}

}  // namespace

bool aq_item(vp8hip_ctx *c, AqItem &it) {
    if (c->in.seg_mode != 2) return false;
    const int frame = c->cur_count - 1, k = frame & 1;
    it.cur = c->cur.Y[0];
    it.e = aq_e(c, k);
    it.map = aq_map(c, k);
    it.sum = aq_sum(c, k);
    c->aq_frame[k] = frame;
    return true;
}

const uint8_t *segment_map_in_force(const vp8hip_ctx *c) {
    if (c->in.seg_mode == 1) return c->seg_map_set ? caller_map(c) : nullptr;
    if (c->in.seg_mode != 2) return nullptr;
    const int frame = c->cur_count - 1;
    return frame >= 0 && c->aq_frame[frame & 1] == frame ? aq_map(c, frame & 1) : nullptr;   // (a frame taken in before mode 2 was set has no map)
}

}  // namespace vp8

extern "C" {

int vp8hip_set_segment_mode(vp8hip_ctx *c, int mode, int strength) {
    if (!c || mode < 0 || mode > 2 || (mode == 2 && (strength < 1 || strength > 3))) return VP8HIP_ERR_ARG;
    USE_DEVICE(c);
    if (mode) { const int rc = segment_refusal(c); if (rc) return rc; }
    IntakeSettings next = c->in;
    next.seg_mode = mode;
    next.seg_strength = strength;      // (mode 2's: canonical)
    next = canonical(next, c->W, c->H);
    if (next == c->in) return VP8HIP_OK;
    // a launch still in flight writes the maps and the sum words: it ends first (not a per-frame call)
    JOIN_LF(c);
    if (mode) { const int rc = segment_buffers(c); if (rc) return rc; }
    { const int rc = intake_apply(c, next); if (rc) return rc; }
    c->aq_frame[0] = c->aq_frame[1] = -1;
    return VP8HIP_OK;
}

int vp8hip_set_segment_map_device(vp8hip_ctx *c, const uint8_t *map) {
    if (!c || !map) return VP8HIP_ERR_ARG;
    USE_DEVICE(c);
    return set_map(c, map, hipMemcpyDeviceToDevice);
}

int vp8hip_upload_segment_map(vp8hip_ctx *c, const uint8_t *host_map) {
    if (!c || !host_map) return VP8HIP_ERR_ARG;
    for (int i = 0; i < c->mbs; ++i)
        if (host_map[i] > 3) return VP8HIP_ERR_ARG;
    USE_DEVICE(c);
    const int rc = set_map(c, host_map, hipMemcpyHostToDevice);
    if (rc) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));      // pageable host memory: the map is the caller's again when this returns
    return VP8HIP_OK;
}

int vp8hip_segment_mode(const vp8hip_ctx *c, int *mode, int *strength) {
    if (!c) return VP8HIP_ERR_ARG;
    if (mode) *mode = c->in.seg_mode;
    if (strength) *strength = c->in.seg_strength;
    return VP8HIP_OK;
}

int vp8hip_download_segment_map(vp8hip_ctx *c, uint8_t *map_out, uint8_t *e_out) {
    if (!c || !map_out) return VP8HIP_ERR_ARG;
    USE_DEVICE(c);
    if (!c->in.seg_mode || (e_out && c->in.seg_mode != 2)) return VP8HIP_ERR_STATE;
    const uint8_t *map = segment_map_in_force(c);
    if (c->in.seg_mode == 2 && !map) return VP8HIP_ERR_STATE;
    // (the intake of a batch's member may be on the batch's head-of-frame stream: USE_DEVICE has joined it)
    if (map) HIPCHK(c, hipMemcpyAsync(map_out, map, (size_t)c->mbs, hipMemcpyDeviceToHost, c->stream));
    else memset(map_out, 3, (size_t)c->mbs);
    if (e_out) HIPCHK(c, hipMemcpyAsync(e_out, aq_e(c, (c->cur_count - 1) & 1), (size_t)c->mbs, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return VP8HIP_OK;
}

}  // extern "C"
