// api_analysis.hip -- the frame analysis record (vp8hip_set_analysis): the switch, the history's restart, the two launches' items
// (k_analyse_src_b behind every intake, k_analyse_mb_b behind every loop filter; kernels_analysis.hip) and the record for the host.
//
// One device allocation: the five sum / ticket words of the source-side launch (256 bytes), then the history plane.  The host mirror
// (one allocation too; each of its three parts has a seq and a view of its own, vp8hip_ctx.h) keeps TWO source-side records, by the
// frame number's parity: a host may hand frame n + 1 over while frame n's record is still to be read (vp8drv_stage_frame_host), and
// frame n's coding side names the frame it belongs to.
#include "vp8hip_ctx.h"

using namespace vp8;

namespace vp8 {

namespace {

unsigned long long *analysis_acc(const vp8hip_ctx *c) { return reinterpret_cast<unsigned long long *>(c->an.d); }
uint8_t *analysis_history(const vp8hip_ctx *c) { return c->an.d + 256; }

}  // namespace

bool analysis_src_item(vp8hip_ctx *c, hipStream_t s, AnalysisSrcItem &it) {
    if (!c->in.an_on) return false;
    const int frame = c->cur_count - 1, k = frame & 1;
    it.cur = c->cur.Y[0];
    it.hist = analysis_history(c);
    it.acc = analysis_acc(c);
    it.host = c->an_src[k].h;
    it.seq = c->an_src[k].seq = ++c->an_src_launches;
    it.frame_number = frame;
    it.have_prev = c->an_have_prev ? 1 : 0;
    c->an_have_prev = true;
    c->an_src_frame[k] = frame;
    c->an_src[k].stream = s;
    return true;
}

bool analysis_mb_item(vp8hip_ctx *c, hipStream_t s, AnalysisMbItem &it) {
    const bool checked = c->an_checked, forced = c->an_forced;
    c->an_checked = c->an_forced = false;
    const int frame = c->cur_count - 1;
    if (!c->in.an_on || frame < 0 || c->an_src_frame[frame & 1] != frame) return false;   // (a frame taken in before analysis was turned on has no record)
    it.parts = c->out.parts;
    it.ref = c->out.ref;
    it.seg = c->out.seg;
    it.nz = c->out.nz;
    it.vec = c->out.vec;
    it.is_inter = c->intra_is_inter;
    it.replaced = (checked && !c->lf_key) ? c->intra_stats : nullptr;
    it.host = c->an_mb.h;
    it.seq = ++c->an_mb.seq;
    it.frame_number = frame;
    it.is_key = c->lf_key ? 1 : 0;
    it.mbs = c->mbs;
    it.forced = (forced && !c->lf_key) ? 1 : 0;
    c->an_mb_frame = frame;
    c->an_mb.stream = s;
    return true;
}

void analysis_after_filter(vp8hip_ctx *c, hipStream_t s) {
    AnalysisMbItem it;
    if (analysis_mb_item(c, s, it)) launch_analyse_mb_batch(s, &it, 1);
}

void batch_analysis(vp8hip_batch *b, const int *active) {
    AnalysisMbItem it[MAX_BATCH];
    int n = 0;
    for (int i = 0; i < b->n; ++i) {
        if (active && !active[i]) continue;
        if (analysis_mb_item(b->c[i], b->stream, it[n])) ++n;
    }
    launch_analyse_mb_batch(b->stream, it, n);
}

}  // namespace vp8

extern "C" {

int vp8hip_set_analysis(vp8hip_ctx *c, int on) {
    if (!c || (on != 0 && on != 1)) return VP8HIP_ERR_ARG;
    USE_DEVICE(c);
    if ((on != 0) == c->in.an_on) return VP8HIP_OK;
    if (on && c->shard_comm) return VP8HIP_ERR_STATE;      // (a context whose frames are split over devices codes only part of a frame)
    // a launch still in flight reads and writes the history and the record: it ends first (not a per-frame call)
    JOIN_LF(c);
    if (on) {
        const int rc = c->an.make(c, 256 + (size_t)c->mbs * 256, 256);
        if (rc) return rc;
        c->an_src[0].h = &c->an.h->src[0];
        c->an_src[1].h = &c->an.h->src[1];
        c->an_mb.h = &c->an.h->mb;
    }
    IntakeSettings next = c->in;
    next.an_on = on != 0;
    { const int rc = intake_apply(c, next); if (rc) return rc; }
    c->an_have_prev = false;
    c->an_src_frame[0] = c->an_src_frame[1] = c->an_mb_frame = -1;
    return VP8HIP_OK;
}

int vp8hip_analysis_restart(vp8hip_ctx *c) {
    if (!c) return VP8HIP_ERR_ARG;
    c->an_have_prev = false;
    return VP8HIP_OK;
}

int vp8hip_analysis_result(vp8hip_ctx *c, vp8hip_analysis *a) {
    USE_DEVICE_ONLY(c);
    if (!c || !a) return VP8HIP_ERR_ARG;
    const int last = c->cur_count - 1;
    if (!c->in.an_on || last < 0 || c->an_src_frame[last & 1] != last) return VP8HIP_ERR_STATE;
    const bool coded = c->an_mb_frame >= 0 && c->an_mb_frame >= last - 1 && c->an_src_frame[c->an_mb_frame & 1] == c->an_mb_frame;
    const int frame = coded ? c->an_mb_frame : last, k = frame & 1;
    int rc = c->an_src[k].wait(c);
    if (!rc && coded) rc = c->an_mb.wait(c);
    if (rc) return rc;
    const AnalysisSrcMirror s = *c->an_src[k].h;
    memset(a, 0, sizeof(*a));
    a->frame_number = frame;
    a->have_prev = s.have_prev;
    a->static_mbs = s.static_mbs;
    a->spatial = s.spatial;
    a->temporal_sse = s.sse;
    a->temporal_sad = s.sad;
    if (!coded) return VP8HIP_OK;
    const AnalysisMbMirror m = *c->an_mb.h;
    a->coded = 1;
    a->is_key = m.is_key;
    a->mbs_total = m.mbs_total;
    a->mbs_intra = m.mbs_intra;
    a->mbs_split = m.mbs_split;
    a->mbs_zero_mv = m.mbs_zero_mv;
    a->mbs_no_coeffs = m.mbs_no_coeffs;
    for (int i = 0; i < 3; ++i) a->mbs_ref[i] = m.mbs_ref[i];
    for (int i = 0; i < 4; ++i) a->segment_mbs[i] = m.segment_mbs[i];
    for (int i = 0; i < 2; ++i) {
        a->mv_abs_sum[i] = m.mv_abs_sum[i];
        a->mv_sum[i] = m.mv_sum[i];
    }
    a->mv_sq_sum = m.mv_sq_sum;
    a->nz_coeffs = m.nz_coeffs;
    return VP8HIP_OK;
}

}  // extern "C"
