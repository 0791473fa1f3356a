// api_quality.hip -- PSNR and SSIM of the coded frames (vp8hip_set_quality_stats): k_quality behind every loop filter, the records and
// the summary for the host, the batched launch, the test tap.
#include "vp8hip_ctx.h"

using namespace vp8;

namespace vp8 {

namespace {

size_t quality_state_room() { return round256(sizeof(QualityState)); }
QualityState *quality_state(const vp8hip_ctx *c) { return reinterpret_cast<QualityState *>(c->quality.d); }
unsigned *quality_ticket(const vp8hip_ctx *c) { return reinterpret_cast<unsigned *>(c->quality.d + quality_state_room()); }
QualityPartial *quality_partial(const vp8hip_ctx *c) { return reinterpret_cast<QualityPartial *>(c->quality.d + quality_state_room() + 256); }

}  // namespace

bool quality_item(vp8hip_ctx *c, const Frame &rec, hipStream_t s, QualityArgs &a) {
    if (!c->quality_on) return false;
    // (with vp8hip_set_source_scaling the source size is what the frames are scaled TO and c->cur holds the scaled frame: the codec's
    // error is measured, not the scaler's)
    int w, h;
    picture_size(c, &w, &h);
    a = quality_args(c->cur, rec, w, h);
    a.partial = quality_partial(c);
    a.ticket = quality_ticket(c);
    a.state = quality_state(c);
    a.host = c->quality.h;
    a.seq = ++c->quality.seq;
    a.frame_number = c->cur_count - 1;
    a.is_key = c->lf_key ? 1 : 0;
    c->quality.stream = s;
    return true;
}

void quality_after_filter(vp8hip_ctx *c, const Frame &rec, hipStream_t s) {
    QualityArgs a;
    if (quality_item(c, rec, s, a)) launch_quality(s, a);
}

int batch_quality(vp8hip_batch *b, const int *active) {
    QualityArgs a[MAX_BATCH];
    int n = 0;
    for (int i = 0; i < b->n; ++i) {
        if (active && !active[i]) continue;
        vp8hip_ctx *c = b->c[i];
        if (c->slot[0] < 0) return VP8HIP_ERR_STATE;
        if (quality_item(c, c->frames[c->slot[0]].f, b->stream, a[n])) ++n;
    }
    launch_quality_batch(b->stream, a, n);
    HIPCHK(b->c[0], hipGetLastError());
    return VP8HIP_OK;
}

}  // namespace vp8

extern "C" {

int vp8hip_set_quality_stats(vp8hip_ctx *c, int on) {
    USE_DEVICE(c);
    if (!c || (on != 0 && on != 1)) return VP8HIP_ERR_ARG;
    JOIN_LF(c);
    if (!on || c->quality_on) {
        c->quality_on = on != 0;
        return VP8HIP_OK;
    }
    { const int rc = c->quality.make(c, quality_state_room() + 256 + sizeof(QualityPartial) * (size_t)quality_tiles(c->W, c->H), 0); if (rc) return rc; }      // (zeroed below, with every new summary)
    // a new summary: nothing of an earlier measurement may still be on its way into the state or its mirror
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->quality.stream) HIPCHK(c, hipStreamSynchronize(c->quality.stream));
    HIPCHK(c, hipMemsetAsync(c->quality.d, 0, quality_state_room() + 256, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    memset(c->quality.h, 0, sizeof(QualityState));
    c->quality.seq = 0;
    c->quality_on = true;
    return VP8HIP_OK;
}

int vp8hip_quality_result(vp8hip_ctx *c, vp8hip_quality *q) {
    USE_DEVICE_ONLY(c);
    if (!c || !q) return VP8HIP_ERR_ARG;
    if (!c->quality_on || c->quality.seq == 0) return VP8HIP_ERR_STATE;
    const int rc = c->quality.wait(c);
    if (rc) return rc;
    *q = c->quality.h->pending;
    return VP8HIP_OK;
}

int vp8hip_quality_summary(vp8hip_ctx *c, vp8hip_quality_totals *s) {
    USE_DEVICE_ONLY(c);
    if (!c || !s) return VP8HIP_ERR_ARG;
    if (!c->quality_on) return VP8HIP_ERR_STATE;
    if (c->quality.seq) {
        const int rc = c->quality.wait(c);
        if (rc) return rc;
    }
    quality_totals(*c->quality.h, s);
    return VP8HIP_OK;
}

int vp8hip_batch_quality(vp8hip_batch *b, const int *active) {
    if (!b) return VP8HIP_ERR_ARG;
    USE_DEVICE(b->c[0]);
    return batch_quality(b, active);
}

// test tap (vp8hip_taps.h): the kernel on caller planes, in buffers of its own
int vp8hip_debug_quality(vp8hip_ctx *c, int width, int height, const uint8_t *const src[3], const int32_t src_stride[3],
                         const uint8_t *const rec[3], const int32_t rec_stride[3], vp8hip_quality *q) {
    USE_DEVICE(c);
    JOIN_LF(c);
    if (!c || !src || !rec || !src_stride || !rec_stride || !q || width < 1 || height < 1 || width > 16384 || height > 16384)
        return VP8HIP_ERR_ARG;
    const int pw[3] = {width, (width + 1) / 2, (width + 1) / 2}, ph[3] = {height, (height + 1) / 2, (height + 1) / 2};
    size_t off[3][2], total = 0;
    int stride[3];
    for (int p = 0; p < 3; ++p) {
        if (!src[p] || !rec[p] || src_stride[p] < pw[p] || rec_stride[p] < pw[p]) return VP8HIP_ERR_ARG;
        stride[p] = (pw[p] + 63) & ~63;     // the kernel reads whole dwords of a row
        for (int k = 0; k < 2; ++k) {
            off[p][k] = total;
            total += (size_t)stride[p] * ph[p];
        }
    }
    const int tiles = quality_tiles(width, height);
    const size_t room = quality_state_room();
    uint8_t *d = nullptr;
    HIPCHK(c, hipMalloc(&d, total + room + 256 + sizeof(QualityPartial) * (size_t)tiles));
    hipStream_t s = c->stream;
    int rc = VP8HIP_OK;
    auto run = [&]() -> int {
        for (int p = 0; p < 3; ++p) {
            HIPCHK(c, hipMemcpy2DAsync(d + off[p][0], stride[p], src[p], src_stride[p], pw[p], ph[p], hipMemcpyHostToDevice, s));
            HIPCHK(c, hipMemcpy2DAsync(d + off[p][1], stride[p], rec[p], rec_stride[p], pw[p], ph[p], hipMemcpyHostToDevice, s));
        }
        HIPCHK(c, hipMemsetAsync(d + total, 0, room + 256, s));
        QualityArgs a{};
        for (int p = 0; p < 3; ++p) a.p[p] = QualityPlane{d + off[p][0], d + off[p][1], stride[p], stride[p], pw[p], ph[p]};
        a.state = reinterpret_cast<QualityState *>(d + total);
        a.ticket = reinterpret_cast<unsigned *>(d + total + room);
        a.partial = reinterpret_cast<QualityPartial *>(d + total + room + 256);
        launch_quality(s, a);
        HIPCHK(c, hipGetLastError());
        QualityState st;
        HIPCHK(c, hipMemcpyAsync(&st, a.state, sizeof(st), hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipStreamSynchronize(s));
        *q = st.pending;
        return VP8HIP_OK;
    };
    rc = run();
    (void)hipStreamSynchronize(s);
    (void)hipFree(d);
    return rc;
}

}  // extern "C"
