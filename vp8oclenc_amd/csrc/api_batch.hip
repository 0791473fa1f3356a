// api_batch.hip -- batched contexts: up to MAX_BATCH contexts of one geometry advance one frame together, every stage ONE launch (vp8hip_batch_*).
// The stages are those of api_inter.hip / api_entropy.hip; what a host with many GOP chunks in flight uses instead of a stream per chunk.
#include "vp8hip_ctx.h"
#include "batch_lanes.h"

#include <mutex>

using namespace vp8;

namespace vp8 {

// ---- lanes: the chain streams of a device's batches ------------------------------------------------------------------------
// Which hardware queue a stream lands on is the runtime's bookkeeping (it counts the streams on each queue and gives a new stream
// the queue with the fewest; idle streams count).  A stream per batch, made when the batch is -- between the members' own streams
// going, six at a time -- left it to that sequence which chains shared a queue, and with fewer queues than batches some queues got
// three chains and others one.  The library owns the mapping instead: L = lane_count(vp8hip_hw_queues()) streams per device, made
// TOGETHER at the device's first vp8hip_batch_create BEFORE any member's own stream is retired (the runtime's counts are then as
// even as the host's streams left them, and L streams made in a row go to L different queues), handed to the batches by pick_lane
// (batch_lanes.h), reference-counted and destroyed with the device's last batch.  Two batches on one lane are independent work in
// one in-order queue: each batch's own order is its host thread's, and what one of them waits for on the lane (an event of a side
// stream) the other waits for too -- as it did when their streams shared a hardware queue.
// VP8HIP_BATCH_LANES=0 (read once): a stream per batch as before, for A/B runs.
struct LanePool {
    hipStream_t s[MAX_LANES] = {};
    int load[MAX_LANES] = {};
    int lanes = 0;       // 0: not made
    int batches = 0;
};
static std::mutex g_lane_mu;
static LanePool g_lane_pool[64];      // by device ordinal (a device beyond them gets a stream per batch)

static bool lanes_enabled() {
    static const bool on = [] { const char *v = getenv("VP8HIP_BATCH_LANES"); return !(v && v[0] == '0'); }();
    return on;
}
// The batch's chain stream: a lane (b->lane >= 0) or a stream of its own.  The device is current.
static bool batch_take_stream(vp8hip_batch *b, int device) {
    if (!lanes_enabled() || device < 0 || device >= 64) {
        if (hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking) != hipSuccess) return false;
        ++g_live_contexts;
        return true;
    }
    std::lock_guard<std::mutex> lock(g_lane_mu);
    LanePool &p = g_lane_pool[device];
    if (!p.lanes) {
        const int want = lane_count(vp8hip_hw_queues());
        for (int l = 0; l < want; ++l)
            if (hipStreamCreateWithFlags(&p.s[l], hipStreamNonBlocking) != hipSuccess) {
                while (l-- > 0) { hipStreamDestroy(p.s[l]); p.s[l] = nullptr; }
                return false;
            }
        p.lanes = want;
    }
    const int l = pick_lane(p.load, p.lanes);
    if (p.load[l]++ == 0) ++g_live_contexts;
    ++p.batches;
    b->lane = l;
    b->stream = p.s[l];
    return true;
}
// ... given back: everything of this batch on it is over; a lane stays while any batch of the device lives.
static void batch_release_stream(vp8hip_batch *b, int device) {
    if (!b->stream) return;
    hipStreamSynchronize(b->stream);
    if (b->lane < 0) {
        hipStreamDestroy(b->stream);
        --g_live_contexts;
    } else {
        std::lock_guard<std::mutex> lock(g_lane_mu);
        LanePool &p = g_lane_pool[device];
        if (--p.load[b->lane] == 0) --g_live_contexts;
        if (--p.batches == 0) {
            for (int l = 0; l < p.lanes; ++l) { hipStreamDestroy(p.s[l]); p.s[l] = nullptr; }
            p.lanes = 0;
        }
    }
    b->stream = nullptr;
    b->lane = -1;
}

// A batch's second stream for the entropy stage, made when the first frame is asked for as bytes (a batch that only runs the
// inter path never has one: idle streams still take part in the runtime's stream -> hardware queue assignment).
bool batch_ent_stream(vp8hip_batch *b) {
    static const int mode = [] { const char *v = getenv("VP8HIP_BATCH_ENT_STREAM"); return v && v[0] ? atoi(v) : 0; }();
    if (!b->ev_ent && (hipEventCreateWithFlags(&b->ev_ent_fork, hipEventDisableTiming) != hipSuccess ||
                       hipEventCreateWithFlags(&b->ev_ent, FRAME_EVENT_FLAGS) != hipSuccess))
        return false;
    if (!mode) return false;
    if (b->ent) return true;
    int least = 0, greatest = 0;
    if (mode >= 2 && hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess) {   // A/B: 2 = in the lowest priority class, 3 = in the highest
        if (hipStreamCreateWithPriority(&b->ent, hipStreamNonBlocking, mode == 3 ? greatest : least) != hipSuccess) b->ent = nullptr;
    } else if (hipStreamCreateWithFlags(&b->ent, hipStreamNonBlocking) != hipSuccess) {
        b->ent = nullptr;
    }
    return b->ent != nullptr;
}

// The members a batched call is for: `active[i] == 0` leaves member i out of it (a chunk whose frame is a key frame goes through the
// intra path), active == NULL means all.  m[k] is member pos[k] of the batch: what the caller passes per member (prev_is_golden[i],
// refqi[i], params[i], the planes) is indexed by position.  Every entry point starts here, and every one keeps THE RULE: every
// member is checked before any member's state changes -- a call that refuses leaves the batch as it found it.
struct Members {
    int n = 0;
    vp8hip_ctx *m[MAX_BATCH];
    int pos[MAX_BATCH];
};
static Members active_members(const vp8hip_batch *b, const int *active) {
    Members a;
    for (int i = 0; i < b->n; ++i) {
        if (active && !active[i]) continue;
        a.m[a.n] = b->c[i];
        a.pos[a.n++] = i;
    }
    return a;
}

}  // namespace vp8

extern "C" {

// ---- batched contexts ---------------------------------------------------------------------------------------------------
// Up to MAX_BATCH contexts of one geometry on one device advance one frame together: every stage is ONE launch for all of
// them (vp8hip_dev.h, "batched launches").  The members share the batch's stream, so their own entry points (key frames,
// the entropy stage, downloads) stay ordered with the batched stages.

int vp8hip_batch_create(vp8hip_batch **out, vp8hip_ctx *const *ctxs, int n) {
    if (!out || !ctxs || n < 1 || n > MAX_BATCH) return VP8HIP_ERR_ARG;
    *out = nullptr;
    for (int i = 0; i < n; ++i) {
        if (!ctxs[i] || ctxs[i]->W != ctxs[0]->W || ctxs[i]->H != ctxs[0]->H || ctxs[i]->device != ctxs[0]->device ||
            ctxs[i]->ssim_target != ctxs[0]->ssim_target || ctxs[i]->lf_overlap || ctxs[i]->conformant != ctxs[0]->conformant ||
            !same_intake(ctxs[i], ctxs[0]) || excludes_batch(ctxs[i]->in))
            return VP8HIP_ERR_ARG;
        if (!ctxs[i]->own_stream) return VP8HIP_ERR_STATE;            // already a member of a batch
        for (int j = 0; j < i; ++j)
            if (ctxs[j] == ctxs[i]) return VP8HIP_ERR_ARG;            // the same context twice
    }
    vp8hip_batch *b = new (std::nothrow) vp8hip_batch();
    if (!b) return VP8HIP_ERR_ARG;
    USE_DEVICE(ctxs[0]);
    b->n = n;
    // The chain's stream is a lane of the device's pool (above): batch number i of the device on lane i mod L, so eight batches at
    // four hardware queues are two per lane, and at sixteen queues eight lanes carry one batch each -- the streams of before in
    // effect.  The lanes are made (first batch of the device) while the members' own streams are all still alive.  TRACED in
    // bench.py's order -- six contexts, then their batch, eight times: four lanes on four different queues, two chains each
    // (profiles/queue_lanes_parent_vs_this.txt).  NOT traced, an argument from the runtime's least-used rule only: a host that
    // makes all its contexts first (48: twelve per queue) gets distinct queues too, which it would not if the first batch's six
    // streams went before the lanes came (10 / 10 / 12 / 12).  Idle streams still take part in the runtime's assignment, so the
    // members' own streams go once the batch has its lane, and vp8hip_batch_destroy gives every member a stream of its own again.
    if (!batch_take_stream(b, ctxs[0]->device)) {      // (nothing of the members has changed)
        delete b;
        return VP8HIP_ERR_HIP;
    }
    for (int i = 0; i < n; ++i) {
        hipStreamSynchronize(ctxs[i]->stream);
        if (ctxs[i]->own_stream) hipStreamDestroy(ctxs[i]->own_stream);
        ctxs[i]->own_stream = nullptr;
    }
    for (int i = 0; i < n; ++i) {
        ctxs[i]->stream = b->stream;
        ctxs[i]->batch = b;
        b->c[i] = ctxs[i];
        if (ctxs[i]->counted) --g_live_contexts;   // the batch's lane is counted in their place (batch_take_stream)
        ctxs[i]->counted = false;
    }
    // the head-of-frame stream (VP8HIP_BATCH_PREP): 0 (default) = none, the head of the frame stays at the head of the chain;
    // 1 = one per batch, in the lowest priority class; 2 = one for all batches of the process.  Measured on MI355X, 48 chunks
    // in 8 batches, same box: 62.2 M MB/s without, 59.5 with one per batch (59.9 in the default priority class), 60.9 with one
    // for all -- the second set of queues costs more than the shorter chains win, so it is off unless asked for.
    const int prep_mode = vp8hip_batch_prep_mode();
    bool ok = true;
    if (prep_mode) {
        ok = hipEventCreateWithFlags(&b->ev_gate, hipEventDisableTiming) == hipSuccess &&
             hipEventCreateWithFlags(&b->ev_gate2, hipEventDisableTiming) == hipSuccess &&
             hipEventCreateWithFlags(&b->ev_prep, hipEventDisableTiming) == hipSuccess;
        int least = 0, greatest = 0;
        ok = ok && hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess;
        static const bool normal_priority = getenv("VP8HIP_BATCH_PREP_PRIO") != nullptr;   // A/B: the head-of-frame stream in the default class
        if (normal_priority) least = 0;
        if (ok && prep_mode == 2) {
            static hipStream_t shared[64] = {};
            hipStream_t &sh = shared[ctxs[0]->device & 63];
            if (!sh) ok = hipStreamCreateWithPriority(&sh, hipStreamNonBlocking, least) == hipSuccess;
            b->prep = sh;
            b->prep_shared = true;
        } else if (ok) {
            ok = hipStreamCreateWithPriority(&b->prep, hipStreamNonBlocking, least) == hipSuccess;
        }
    }
    if (!ok) {
        vp8hip_batch_destroy(b);
        return VP8HIP_ERR_HIP;
    }
    *out = b;
    return VP8HIP_OK;
}

void vp8hip_batch_destroy(vp8hip_batch *b) {   // the contexts stay (destroy the batch before its members), each back on its own stream
    if (!b) return;
    hipSetDevice(b->c[0]->device);
    if (b->prep) hipStreamSynchronize(b->prep);
    // the chain's stream is synchronised and, where it is a lane, only given back: a lane other batches still use stays (whatever
    // of theirs was enqueued by now is waited for too, nothing more)
    batch_release_stream(b, b->c[0]->device);
    if (b->prep && !b->prep_shared) hipStreamDestroy(b->prep);
    if (b->ev_gate) hipEventDestroy(b->ev_gate);
    if (b->ev_gate2) hipEventDestroy(b->ev_gate2);
    if (b->ev_prep) hipEventDestroy(b->ev_prep);
    if (b->ent) {
        hipStreamSynchronize(b->ent);
        hipStreamDestroy(b->ent);
    }
    if (b->copy) {
        hipStreamSynchronize(b->copy);
        hipStreamDestroy(b->copy);
        hipEventDestroy(b->ev_copied);
        hipEventDestroy(b->ev_packed[0]);
        hipEventDestroy(b->ev_packed[1]);
        for (int i = 0; i < b->n; ++i) { b->stage[i][0].release(); b->stage[i][1].release(); }
    }
    if (b->ev_ent_fork) hipEventDestroy(b->ev_ent_fork);
    if (b->ev_ent) hipEventDestroy(b->ev_ent);
    if (b->ev_chroma) hipEventDestroy(b->ev_chroma);      // (the stream has been synchronised: a member's pending scan has its sums)
    for (int i = 0; i < b->n; ++i) b->c[i]->frame_event = nullptr;
    for (int i = 0; i < b->n; ++i) {
        b->c[i]->batch = nullptr;
        if (!b->c[i]->own_stream) hipStreamCreateWithFlags(&b->c[i]->own_stream, hipStreamNonBlocking);
        b->c[i]->stream = b->c[i]->own_stream;
        if (!b->c[i]->counted) ++g_live_contexts;
        b->c[i]->counted = true;
    }
    delete b;
}

int vp8hip_batch_lane(const vp8hip_batch *b) { return b ? b->lane : -1; }

// the copy stream, its events and the members' staging buffers (two each), made on first use and again when the source size has changed
static int batch_stage_ready(vp8hip_batch *b) {
    vp8hip_ctx *c0 = b->c[0];
    size_t nb[3];
    incoming_bytes(c0, nb);
    const size_t bytes = nb[0] + nb[1] + nb[2];
    if (!b->copy) {
        HIPCHK(c0, hipStreamCreateWithFlags(&b->copy, hipStreamNonBlocking));
        HIPCHK(c0, hipEventCreateWithFlags(&b->ev_copied, hipEventDisableTiming));
        HIPCHK(c0, hipEventCreateWithFlags(&b->ev_packed[0], hipEventDisableTiming));
        HIPCHK(c0, hipEventCreateWithFlags(&b->ev_packed[1], hipEventDisableTiming));
    }
    if (b->stage_bytes == bytes && b->stage_fmt == c0->in.src_fmt) return VP8HIP_OK;
    // (first call, or the source size or format has changed: nothing in flight reads the old buffers after this)
    { const int rc = quiesce_intake(c0); if (rc) return rc; }
    b->stage_bytes = 0;
    for (int i = 0; i < b->n; ++i)
        for (int k = 0; k < 2; ++k) {
            b->stage[i][k].release();
            const int rc = b->stage[i][k].grow(c0, bytes);      // (quiesces once more, on idle streams: not a per-frame path)
            if (rc) return rc;
        }
    b->stage_bytes = bytes;
    b->stage_fmt = c0->in.src_fmt;
    b->packed_valid[0] = b->packed_valid[1] = false;
    b->pre_valid = false;
    return VP8HIP_OK;
}

// the members' new frames, tight planes in device memory (host == false) or in host memory (copied into the batch's staging buffers first)
static int batch_set_current(vp8hip_batch *b, const int *active, const void *const *y, const void *const *u, const void *const *v, bool host) {
    if (!b || !y || !u || !v) return VP8HIP_ERR_ARG;
    vp8hip_ctx *c0 = b->c[0];
    USE_DEVICE_ONLY(c0);
    const Members a = active_members(b, active);
    vp8hip_ctx *const *m = a.m;
    const int n = a.n;
    const void *my[MAX_BATCH], *mu[MAX_BATCH], *mv[MAX_BATCH];      // the members' planes
    int slot = -1;
    // an error return must leave the staging slots, the prefetch record and the members' current frames as they were (a retry that
    // flipped stage_idx once more would pack an older frame from the other slot)
    for (int k = 0; k < n; ++k) {
        const int i = a.pos[k];
        if (!y[i] || !u[i] || !v[i]) return VP8HIP_ERR_ARG;
        if (!same_intake(m[k], c0)) return VP8HIP_ERR_ARG;   // one launch, one source format and size (and one scaler: incoming size, dst, filter)
        my[k] = y[i]; mu[k] = u[i]; mv[k] = v[i];
    }
    { const int rc = intake_ready(m, n); if (rc) return rc; }      // (take_frames would ask too -- behind the staging flip, which is too late to refuse)
    if (host) {
        const int rc = batch_stage_ready(b);
        if (rc) return rc;
        size_t nb[3];
        incoming_bytes(c0, nb);
        slot = b->stage_idx ^= 1;
        bool waited = false;
        for (int k = 0; k < n; ++k) {
            const int i = a.pos[k];
            uint8_t *d = b->stage[i][slot].p;
            if (!(b->pre_valid && b->pre[i][0] == y[i] && b->pre[i][1] == u[i] && b->pre[i][2] == v[i])) {   // not prefetched: copied now
                if (!waited && b->packed_valid[slot]) HIPCHK(c0, hipStreamWaitEvent(b->copy, b->ev_packed[slot], 0));   // the pack of two frames ago has read this buffer
                waited = true;
                {
                    const int cr = copy_planes(c0, d, y[i], u[i], v[i], nb, hipMemcpyHostToDevice, b->copy);
                    if (cr) {       // a failed copy: nothing of this call counts -- not the flip, not the prefetch
                        b->stage_idx ^= 1;
                        b->pre_valid = false;
                        return cr;
                    }
                }
            }
            my[k] = d; mu[k] = d + nb[0]; mv[k] = d + nb[0] + nb[1];
        }
        b->pre_valid = false;
        HIPCHK(c0, hipEventRecord(b->ev_copied, b->copy));
    }
    // (a parameter scan of the frame that is being replaced, asked for and never used: on that frame, now -- on `stream`, in front of the
    // gate below, so that the next call's head-of-frame work, which overwrites that frame's surface, waits for it)
    for (int i = 0; i < n; ++i) flush_scan(m[i]);
    if (!n) return VP8HIP_OK;
    hipStream_t ps = b->prep ? b->prep : b->stream;      // the stream the members' frames are taken in on
    if (b->prep) {
        // A new frame goes into the surface (and its parameters into the blocks) of the frame before the previous one: all
        // of that frame's work -- enqueued on `stream` before the PREVIOUS frame call began, which is where ev_gate was last
        // recorded -- must be over; the previous frame's chain may still be running, and that is the point.
        HIPCHK(c0, hipStreamWaitEvent(b->prep, b->ev_gate, 0));
        HIPCHK(c0, hipEventRecord(b->ev_gate2, b->stream));
        hipEvent_t t_ = b->ev_gate;
        b->ev_gate = b->ev_gate2;
        b->ev_gate2 = t_;
        b->prep_pending = true;
    }
    if (host) HIPCHK(c0, hipStreamWaitEvent(ps, b->ev_copied, 0));
    { const int rc = take_frames(m, my, mu, mv, n, ps, nullptr, nullptr, host); if (rc) return rc; }
    HIPCHK(c0, hipGetLastError());
    if (host) {
        HIPCHK(c0, hipEventRecord(b->ev_packed[slot], ps));
        b->packed_valid[slot] = true;
    }
    return VP8HIP_OK;
}

int vp8hip_batch_set_current_device(vp8hip_batch *b, const int *active, const void *const *y, const void *const *u, const void *const *v) {
    return batch_set_current(b, active, y, u, v, false);
}

// Planes in HOST memory (vp8enc.cpp:386-388, the reference's own hand-over: clEnqueueWriteBuffer from the frame it has read).  The
// copies are asynchronous when the planes are page-locked (vp8hip_host_alloc) and then overlap the batch's previous frame still on the
// device; page-locked or not, the planes must stay as they are until the NEXT vp8hip_batch_upload_current of this batch has returned (it waits for these
// copies first) or the batch's contexts have been synchronised.
// The frame AFTER the one under way, started on its way early: the copies go into the buffers the next vp8hip_batch_upload_current
// will pack from, and that call, given the same planes, finds them there.  A host that knows its next frame (a decoder's ring, a file
// reader one frame ahead) calls this right after it has enqueued the current one: the copies then have a whole frame's time.
int vp8hip_batch_prefetch_current(vp8hip_batch *b, const uint8_t *const *y, const uint8_t *const *u, const uint8_t *const *v) {
    if (!b || !y || !u || !v) return VP8HIP_ERR_ARG;
    vp8hip_ctx *c0 = b->c[0];
    USE_DEVICE_ONLY(c0);
    const int rc = batch_stage_ready(b);
    if (rc) return rc;
    size_t nb[3];
    incoming_bytes(c0, nb);
    const int slot = b->stage_idx ^ 1;       // what the next upload will flip to
    if (b->packed_valid[slot]) HIPCHK(c0, hipStreamWaitEvent(b->copy, b->ev_packed[slot], 0));
    for (int i = 0; i < b->n; ++i) {
        b->pre[i][0] = b->pre[i][1] = b->pre[i][2] = nullptr;
        if (!y[i] || !u[i] || !v[i]) continue;
        { const int cr = copy_planes(c0, b->stage[i][slot].p, y[i], u[i], v[i], nb, hipMemcpyHostToDevice, b->copy); if (cr) return cr; }
        b->pre[i][0] = y[i]; b->pre[i][1] = u[i]; b->pre[i][2] = v[i];
    }
    HIPCHK(c0, hipEventRecord(b->ev_copied, b->copy));
    b->pre_valid = true;
    return VP8HIP_OK;
}

int vp8hip_batch_upload_current(vp8hip_batch *b, const int *active, const uint8_t *const *y, const uint8_t *const *u, const uint8_t *const *v) {
    if (!b) return VP8HIP_ERR_ARG;
    if (b->copy) {
        (void)hipSetDevice(b->c[0]->device);
        HIPCHK(b->c[0], hipEventSynchronize(b->ev_copied));     // the previous call's copies have left the host's planes
    }
    return batch_set_current(b, active, reinterpret_cast<const void *const *>(y), reinterpret_cast<const void *const *>(u),
                             reinterpret_cast<const void *const *>(v), true);
}

int vp8hip_batch_auto_segments(vp8hip_batch *b, const int *active, const int *is_key_frame, const int32_t (*refqi)[4], int qi_min) {
    if (!b || !is_key_frame || !refqi) return VP8HIP_ERR_ARG;
    vp8hip_ctx *c0 = b->c[0];
    USE_DEVICE_ONLY(c0);
    const Members a = active_members(b, active);
    for (int k = 0; k < a.n; ++k)
        if (a.m[k]->cur_count == 0) return VP8HIP_ERR_STATE;
    ScanRequest q[MAX_BATCH];
    for (int k = 0; k < a.n; ++k) {
        next_params(a.m[k]);
        q[k] = scan_request(a.m[k], is_key_frame[a.pos[k]], refqi[a.pos[k]], qi_min);
    }
    // The scan rides in k_search2's launch of the same frame (vp8hip_batch_inter_transform, next; kernels_s2.hip says why): with the part
    // full a launch of its own holds the batch's stream for half a millisecond where its work is 15 us (VP8HIP_BATCH_SCAN_LAUNCH=1: as it was)
    static const bool own_launch = [] { const char *v = getenv("VP8HIP_BATCH_SCAN_LAUNCH"); return v && v[0] == '1'; }();
    if (a.n && !b->prep && !own_launch) {
        for (int k = 0; k < a.n; ++k) {
            a.m[k]->scan_req = q[k];
            a.m[k]->scan_deferred = true;
        }
        return VP8HIP_OK;
    }
    if (a.n && b->prep) b->prep_pending = true;
    if (a.n) launch_auto_segments_batch(b->prep ? b->prep : b->stream, q, a.n);
    HIPCHK(c0, hipGetLastError());
    return VP8HIP_OK;
}

int vp8hip_batch_inter_transform(vp8hip_batch *b, const int *active, const int *prev_is_golden, const int *prev_is_altref,
                                 const int *use_golden, const int *use_altref) {
    if (!b || !prev_is_golden || !prev_is_altref || !use_golden || !use_altref) return VP8HIP_ERR_ARG;
    vp8hip_ctx *c0 = b->c[0];
    USE_DEVICE_ONLY(c0);
    const Members a = active_members(b, active);
    vp8hip_ctx *const *m = a.m;
    const int n = a.n;
    for (int k = 0; k < n; ++k) {
        const int i = a.pos[k];
        if (m[k]->conformant != c0->conformant) return VP8HIP_ERR_ARG;   // one launch, one predictor
        if (m[k]->in.seg_mode != c0->in.seg_mode || m[k]->in.seg_strength != c0->in.seg_strength) return VP8HIP_ERR_ARG;   // ... and one segment mode (the maps are the members' own)
        const int rc = inter_check(m[k], prev_is_golden[i], prev_is_altref[i], use_golden[i], use_altref[i]);
        if (rc) return rc;
    }
    CodingItem it[MAX_BATCH];      // (it[k].scan: the member's parameter scan still waiting for a launch to ride in, vp8hip_batch_auto_segments)
    const Frame *pyr[2 * MAX_BATCH], *pyr_cur[MAX_BATCH];
    int npyr = 0, npyr_cur = 0;
    uint32_t pyr_border = 0;
    for (int k = 0; k < n; ++k) {
        const int i = a.pos[k];
        vp8hip_ctx *c = m[k];
        const int rc = inter_begin(c, prev_is_golden[i], prev_is_altref[i], use_golden[i], use_altref[i]);
        if (rc) {   // (inter_check above has passed: not expected.)  The scans collected so far have not been launched: they wait again
            for (int j = 0; j < k; ++j)
                if (it[j].scan) m[j]->scan_deferred = true;
            return rc;
        }
        FrameSurf &last = c->frames[c->slot[0]];
        if (!c->cur_pyramid_valid) {
            if (b->prep) pyr_cur[npyr_cur++] = &c->cur;   // the new frame's pyramid: head-of-frame work
            else pyr[npyr++] = &c->cur;
        }
        bool border_alone = false;
        if (!last.pyramid_valid) {
            if (!last.border_valid) pyr_border |= 1u << npyr;
            pyr[npyr++] = &last.f;
        } else if (!last.border_valid) {
            border_alone = true;
        }
        if (border_alone) {
            batch_join_prep(b);
            launch_border(b->stream, last.f);
        }
        last.pyramid_valid = true;
        last.border_valid = true;
        c->cur_pyramid_valid = true;
        it[k] = coding_item(c, use_golden[i], use_altref[i]);
        c->scan_deferred = false;      // (this call launches it: in k_search2's launch, or on its own right behind it)
    }
    if (!n) return VP8HIP_OK;
    hipStream_t s = b->stream;
    if (npyr_cur) {
        b->prep_pending = true;
        launch_pyramid_batch(b->prep, pyr_cur, npyr_cur, 0);
    }
    batch_join_prep(b);   // the chain starts here: LAST's pyramid and replicated edges, the searches, the transform
    if (npyr) {
        Timed t(c0, VP8HIP_K_DOWNSAMPLE);
        launch_pyramid_batch(s, pyr, npyr, pyr_border);
    }
    const int net_width = c0->mbw * 2;
    // A launch per level of the hierarchical search: the coarse levels fused into one launch, as one video has them, measured 9 % (levels 4-1)
    // to 15 % (all five) slower with 48 chunks in flight (profiles/README.md, round 6).
    int src = 0;
    for (int l = 4; l >= 0; --l) {
        Timed t(c0, VP8HIP_K_SEARCH1_L4 + (4 - l));
        launch_search1_batch(s, it, n, l, src, net_width);
        src ^= 1;
    }
    bool carried;
    {
        Timed t(c0, VP8HIP_K_SEARCH2);
        carried = launch_search2_batch(s, it, n, s2_clock(c0));
    }
    for (int k = 0; k < n && !carried; ++k)
        if (it[k].scan) launch_auto_segments(s, *it[k].scan);
    {
        Timed t(c0, VP8HIP_K_MB);
        launch_mb_batch(s, it, n, c0->ssim_target, c0->mbw, c0->mbh, c0->conformant != 0, c0->in.seg_mode != 0);
    }
    for (int k = 0; k < n; ++k) recon_made(m[k], false);
    HIPCHK(c0, hipGetLastError());
    return VP8HIP_OK;
}

int vp8hip_batch_loop_filter(vp8hip_batch *b, const int *active) {
    if (!b) return VP8HIP_ERR_ARG;
    vp8hip_ctx *c0 = b->c[0];
    USE_DEVICE(c0);   // (joins the head-of-frame stream)
    const Members a = active_members(b, active);
    vp8hip_ctx *const *m = a.m;
    const int n = a.n;
    for (int k = 0; k < n; ++k) {
        if (!m[k]->recon_ready || m[k]->recon < 0) return VP8HIP_ERR_STATE;
        if (m[k]->lf_type != m[0]->lf_type) return VP8HIP_ERR_STATE;   // one launch, one filter: the members' types must agree
    }
    if (!n) return VP8HIP_OK;
    FilterItem it[MAX_BATCH];
    for (int k = 0; k < n; ++k) {
        it[k] = filter_item(m[k]);
        m[k]->verdict_stream = b->stream;
    }
    // the entropy stage of these frames may start here (everything it reads has been enqueued), beside the filter
    if (b->ent) HIPCHK(c0, hipEventRecord(b->ev_ent_fork, b->stream));
    {
        Timed t(c0, VP8HIP_K_LOOP_FILTER);
        // (form 3 for batches: with the part full a launch's instructions and LDS count, not its latency; VP8HIP_LF_BATCH_FORM=4 for A/B runs)
        static const bool form4 = [] { const char *v = getenv("VP8HIP_LF_BATCH_FORM"); return v && atoi(v) == 4; }();
        if (m[0]->lf_type == 1) launch_loop_filter_simple_batch(b->stream, it, n, c0->mbw, c0->mbh);
        else if (form4) launch_loop_filter4_batch(b->stream, it, n, c0->mbw, c0->mbh, c0->conformant != 0);
        else launch_loop_filter3_batch(b->stream, it, n, c0->mbw, c0->mbh, c0->conformant != 0);
    }
    b->ent_fork_fresh = b->ent != nullptr;
    for (int k = 0; k < n; ++k) recon_filtered(m[k]);
    HIPCHK(c0, hipGetLastError());
    batch_analysis(b, active);         // (vp8hip_set_analysis: the members' coding sides, one launch behind the filter)
    return batch_quality(b, active);   // (the members with stats on: one launch behind the filter)
}

// intra_transform (intra_part.h:1089-1109) for the members whose frame is a key frame, in ONE launch (the members' wavefronts side by side:
// a batch whose chunks all start a GOP used to run them one after the other), then every member's filter mask
// (prepare_filter_mask, loop_filter.h:25-55).  vp8hip_batch_loop_filter for the same members follows.
int vp8hip_batch_intra_transform(vp8hip_batch *b, const int *active) {
    if (!b) return VP8HIP_ERR_ARG;
    vp8hip_ctx *c0 = b->c[0];
    USE_DEVICE(c0);
    const Members a = active_members(b, active);
    vp8hip_ctx *const *m = a.m;
    const int n = a.n;
    for (int k = 0; k < n; ++k)
        if (m[k]->cur_count == 0) return VP8HIP_ERR_STATE;
    CheckItem it[MAX_BATCH];
    for (int j = 0; j < n; ++j) {
        vp8hip_ctx *c = m[j];
        const int rc = claim_recon(c);
        if (rc) return rc;
        c->ent_counted_partitions = 0;
        drop_overflowed_frame(c);
        ++c->out_gen;
        CheckItem &k = it[j];
        k.cur = &c->cur;
        k.recon = &c->frames[c->recon].f;
        k.o = &c->out;
        k.sd = c->d_sd;
        k.modes = c->intra_modes;
        k.is_inter = c->intra_is_inter;
        k.prog = c->intra_prog;
        k.err = c->d_progress + LF_ERR_WORD;
        k.gen = ++c->intra_gen;
    }
    if (!n) return VP8HIP_OK;
    {
        Timed t(c0, VP8HIP_K_INTRA);
        launch_intra_key_batch(b->stream, it, n, c0->mbw, c0->mbh);
    }
    {
        Timed t(c0, VP8HIP_K_FILTER_MASK);
        for (int i = 0; i < n; ++i) launch_filter_mask(b->stream, m[i]->out, m[i]->d_sd, m[i]->mbs);
    }
    for (int k = 0; k < n; ++k) recon_made(m[k], true);
    HIPCHK(c0, hipGetLastError());
    return VP8HIP_OK;
}

int vp8hip_batch_check_ssim_async(vp8hip_batch *b, const int *active, const int32_t (*refqi)[4], int qi_min) {
    if (!b || !refqi) return VP8HIP_ERR_ARG;
    vp8hip_ctx *c0 = b->c[0];
    USE_DEVICE(c0);
    const Members a = active_members(b, active);
    const int n = a.n;
    for (int k = 0; k < n; ++k) {
        const vp8hip_ctx *c = a.m[k];
        if (!c->recon_ready || c->recon < 0 || c->cur_count == 0 || c->verdict_pending || c->chk_armed) return VP8HIP_ERR_STATE;
    }
    CheckItem it[MAX_BATCH];
    for (int k = 0; k < n; ++k) check_item(a.m[k], it[k], refqi[a.pos[k]], qi_min);
    if (!n) return VP8HIP_OK;
    if (fallback_possible(c0->ssim_target)) {
        Timed t(c0, VP8HIP_K_INTRA);
        launch_check_fallback(b->stream, it, n, c0->ssim_target, c0->mbw, c0->mbh, c0->conformant);
    }
    HIPCHK(c0, hipGetLastError());
    return VP8HIP_OK;
}

// scene_change()'s two sums (vp8enc.cpp:265-284) for the active members in ONE launch with its fold, nobody waiting: the members' words are
// those of vp8hip_chroma_change_async, the event is the batch's, and vp8hip_chroma_change_result per member takes the answer.
int vp8hip_batch_chroma_change_async(vp8hip_batch *b, const int *active) {
    if (!b) return VP8HIP_ERR_ARG;
    vp8hip_ctx *c0 = b->c[0];
    USE_DEVICE(c0);   // (joins the head-of-frame stream: the members' intake is in front of what follows)
    const Members a = active_members(b, active);
    for (int k = 0; k < a.n; ++k)
        if (a.m[k]->cur_count == 0) return VP8HIP_ERR_STATE;
    if (!b->ev_chroma) HIPCHK(c0, hipEventCreateWithFlags(&b->ev_chroma, FRAME_EVENT_FLAGS));
    ChromaScan q[MAX_BATCH];
    int nq = 0;
    for (int k = 0; k < a.n; ++k) {
        vp8hip_ctx *c = a.m[k];
        flush_scan(c);      // (a parameter scan still waiting for a launch uses the same partial sums)
        c->chroma_pending = true;
        c->chroma_none = c->cur_count < 2;
        c->chroma_by_batch = true;
        if (c->chroma_none) continue;
        q[nq++] = ChromaScan{&c->cur, &c->cur_prev, c->d_stats + 8, reinterpret_cast<uint32_t *>(c->h_verdict) + 32};
    }
    if (!nq) return VP8HIP_OK;
    launch_chroma_sad_batch(b->stream, q, nq);
    HIPCHK(c0, hipGetLastError());
    HIPCHK(c0, hipEventRecord(b->ev_chroma, b->stream));
    // (the next frame's intake overwrites the older of the two surfaces the scan reads: on a head-of-frame stream it waits for the scan)
    if (b->prep) HIPCHK(c0, hipStreamWaitEvent(b->prep, b->ev_chroma, 0));
    return VP8HIP_OK;
}

// The entropy stage of the frames of a batch's members in the same nine launches (blockIdx.z = member; the coder takes the
// members' bool strings as job pairs).  Every active member is then between _begin and _end: vp8hip_encode_frame_end
// per member reads its frame back (and, should a frame have been denser than the coder's scratch, codes that one again
// on its own).
int vp8hip_batch_encode_frame_begin(vp8hip_batch *b, const int *active, int num_partitions, const vp8hip_header_params *params) {
    if (!b || !params) return VP8HIP_ERR_ARG;
    const int P = num_partitions;
    if (P != 1 && P != 2 && P != 4 && P != 8) return VP8HIP_ERR_ARG;
    vp8hip_ctx *c0 = b->c[0];
    bool early = b->ent_fork_fresh;     // (read before USE_DEVICE, which marks it stale for whatever this call enqueues)
    USE_DEVICE(c0);
    FrameEntropy e[MAX_BATCH];
    FrameOut fo[MAX_BATCH];
    const Members a = active_members(b, active);
    vp8hip_ctx *const *m = a.m;
    const int n = a.n;
    for (int k = 0; k < n; ++k)
        if (m[k]->frame_pending) return VP8HIP_ERR_STATE;
    for (int k = 0; k < n; ++k) {
        vp8hip_ctx *c = m[k];
        const int rc = frame_prepare(c, P, &params[a.pos[k]], e[k], fo[k]);
        if (rc) return rc;
        c->frame_params = params[a.pos[k]];
        c->frame_partitions = P;
    }
    if (!n) return VP8HIP_OK;
    // Beside the loop filter, on the batch's second stream: the stage reads the frame's coefficients, modes and vectors (final
    // before the filter's launch: ev_ent_fork) and the segment data check_SSIM may have updated INSIDE that launch -- so only a
    // caller that has taken every member's verdict (vp8hip_check_ssim_result: the update is then in memory) gets the early
    // start; otherwise, and whenever anything was enqueued for the batch since the filter, the stage starts behind all of it.
    // The chain waits for the stage before it goes on (the next frame's k_mb overwrites what the stage reads).
    const bool side = !c0->prof_mask && batch_ent_stream(b);
    hipStream_t s = side ? b->ent : b->stream;
    if (side) {
        for (int i = 0; i < n; ++i) early = early && !m[i]->verdict_pending;
        if (!early) HIPCHK(c0, hipEventRecord(b->ev_ent_fork, b->stream));
        HIPCHK(c0, hipStreamWaitEvent(b->ent, b->ev_ent_fork, 0));
    }
    {
        Timed t(c0, VP8HIP_K_ENT_COUNT);
        launch_fe_count_batch(s, e, n);
    }
    {
        Timed t(c0, VP8HIP_K_HDR_ENCODE);
        launch_fe_emit_batch(s, e, n);
    }
    {
        Timed t(c0, VP8HIP_K_ENT_ENCODE);
        launch_frame_code_batch(s, e, fo, n);
    }
    HIPCHK(c0, hipGetLastError());
    for (int i = 0; i < n; ++i) {
        vp8hip_ctx *c = m[i];
        c->ent_counted_partitions = P;
        if (!frame_zero_copy()) {
            const size_t first = c->h_frame_cap < FRAME_FIRST_COPY ? c->h_frame_cap : FRAME_FIRST_COPY;
            HIPCHK(c0, hipMemcpyAsync(c->h_frame, c->d_frame, first, hipMemcpyDeviceToHost, s));
        }
        c->frame_pending = true;
        c->frame_gen = c->out_gen;
        c->frame_event = b->ev_ent;      // the end of the stage, not of whatever the caller enqueues behind it before it takes the bytes
    }
    if (b->ev_ent) HIPCHK(c0, hipEventRecord(b->ev_ent, s));
    if (side) HIPCHK(c0, hipStreamWaitEvent(b->stream, b->ev_ent, 0));
    return VP8HIP_OK;
}

}  // extern "C"
