// vp8hip_ctx.h -- INTERNAL to libvp8hip.so: the context behind include/vp8hip.h, the batch, and what the api_*.hip units share.
//
// What the reference keeps as ~70 cl_mem objects and 60 pre-bound cl_kernel instances
// (init.h:430-593, 595-1271) is one context here: a pool of padded frame surfaces (a reference
// "slot" is an index into the pool, so golden := last is a pointer copy, not the five
// clEnqueueCopyBuffer + three clEnqueueCopyImage of inter_part.h:35-50,72-83), the vector nets,
// the per-macroblock outputs, and one in-order HIP stream.
//
// Units: api_context.hip (create / destroy, surfaces, parameters, stream ordering, the record wait, downloads, device memory),
// intake_settings.h (pure host code: the intake's settings in one struct, their one validity rule, their equality, the sizes that follow),
// api_intake.hip (how a frame becomes current: intake_apply, the one way a setting changes; the source size / scaling / format / colour / transfer
// setters, staging, the stage order; upload, prefetch, set_current_device),
// api_geometry.hip (the window and orientation setters), api_deinterlace.hip, api_denoise.hip, api_analysis.hip, api_segment.hip, api_quality.hip
// (a stage each: its setter -- which edits a copy of the settings and hands it to intake_apply --, its item, its results),
// api_inter.hip (inter path, check_SSIM, key frames, loop filter), api_entropy.hip (coefficient + header entropy stage, frames out),
// api_batch.hip (vp8hip_batch_*), api_shard.hip (export / import, RCCL: vp8hip_shard_*, vp8hip_group_*), api_profile.hip (timers, debug taps).
#ifndef VP8HIP_CTX_H
#define VP8HIP_CTX_H
#include <limits.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <mutex>
#include <vector>
#include <new>

#include "../../include/vp8hip.h"
#include "../../include/vp8hip_host.h"
#include "vp8hip_dev.h"
#include "intake_settings.h"

struct ncclComm;     // (rccl.h is included by api_shard.hip only; the library resolves RCCL when a host first asks for it)

namespace vp8 {

constexpr int NFRAMES = 5;  // LAST, GOLDEN, ALTREF may all differ, + the reconstruction in flight, + 1 spare
constexpr int MAX_EVENTS = 4096;

struct FrameSurf {
    Frame f;
    bool pyramid_valid = false;
    bool border_valid = true;    // false: fresh out of the loop filter, replicated edges still to be made (with its pyramid)
};

}  // namespace vp8

struct vp8hip_batch;
struct vp8hip_ctx;
inline size_t round256(size_t n) { return (n + 255) & ~(size_t)255; }
// Device buffers that are made and freed together come out of ONE allocation: a context has forty of them, and forty hipMalloc + forty
// hipFree -- each a trip through the driver, the frees synchronising -- were 11 ms to make a context and 15 ms to destroy it (48 chunks:
// 1.2 s).  Every buffer starts 256-byte aligned and has a page of slack behind it.
struct DeviceArena {
    uint8_t *base = nullptr;
    size_t bytes = 0;
    struct Want { void **p; size_t bytes; };
    std::vector<Want> wants;
    template <class T> void want(T **p, size_t n) { wants.push_back(Want{reinterpret_cast<void **>(p), n}); }
    static size_t room(size_t n) { return round256(n) + 4096; }
    hipError_t commit() {      // one hipMalloc; the pointers handed to want() are set
        size_t total = 0;
        for (const Want &w : wants) total += room(w.bytes);
        bytes = total ? total : 256;
        const hipError_t e = hipMalloc(reinterpret_cast<void **>(&base), bytes);
        if (e != hipSuccess) { base = nullptr; wants.clear(); return e; }
        size_t at = 0;
        for (const Want &w : wants) { *w.p = base + at; at += room(w.bytes); }
        wants.clear();
        return hipSuccess;
    }
    void release() { if (base) (void)hipFree(base); base = nullptr; bytes = 0; }
};

// What a launch leaves for the host: a mirror in host memory the device writes, the mirror's seq last.  seq: the launches so far (the
// last one writes this into h->seq); stream: the stream that one is on.  A view owns nothing: it is waited for, never released.
template <class Mirror> struct RecordView {
    Mirror *h = nullptr;
    uint32_t seq = 0;
    hipStream_t stream = nullptr;
    int wait(vp8hip_ctx *c) const;     // the last launch's mirror is complete
};
// ... with what it owns: the mirror's allocation and the launch's device words (counts, tickets, state: zero at rest).
template <class Mirror> struct Record : RecordView<Mirror> {
    uint8_t *d = nullptr;
    // (no-op once made; of a pair half made nothing is kept; zeroed_bytes 0: the caller zeroes the words itself)
    int make(vp8hip_ctx *c, size_t device_bytes, size_t zeroed_bytes);
    void release();
};

// A device buffer that grows when a setter or a larger incoming size asks for more (never per frame): whatever is in flight ends, the
// new one is allocated, the old one freed.  On failure the old buffer and size stay.
struct DeviceBuf {
    uint8_t *p = nullptr;
    size_t bytes = 0;
    int grow(vp8hip_ctx *c, size_t need);
    void release() { (void)hipFree(p); p = nullptr; bytes = 0; }
};

// Tight I420 of w x h in one buffer, each plane 256-byte aligned: how fmt_stage, di_stage and di_hist hold a frame.
struct TightI420 { size_t off[3], bytes; };
inline TightI420 tight_i420(int w, int h) {
    const size_t ny = round256((size_t)w * h), nc = round256((size_t)(w / 2) * (h / 2));
    return TightI420{{0, ny, ny + nc}, ny + 2 * nc};
}

struct vp8hip_ctx {
    int W = 0, H = 0, mbw = 0, mbh = 0, mbs = 0, b8 = 0;
    float ssim_target = -1.0f;
    int device = 0;
    hipStream_t stream = nullptr;       // the stream in use: the context's own, or its batch's (vp8hip_batch_create)
    hipStream_t own_stream = nullptr;   // the one vp8hip_create made
    int last_hip_error = 0;

    uint8_t *pixel_pool = nullptr;  // one allocation for every surface
    vp8::FrameSurf frames[vp8::NFRAMES];
    vp8::Frame cur;
    int slot[3] = {-1, -1, -1};     // pool index of LAST / GOLDEN / ALTREF
    int recon = -1;                 // pool index of the reconstruction being produced
    bool recon_ready = false;       // holds an unfiltered reconstruction
    int refreshed = -1;             // pool index of the surface the last vp8hip_loop_filter_refresh(GOLDEN / NONE) ended (VP8HIP_DBG_REFRESH_FRAME)
    bool cur_pyramid_valid = false;
    vp8::Frame cur_prev;                 // the previous current frame (the two surfaces swap on every upload)
    int cur_count = 0;              // current frames received so far
    uint32_t *d_stats = nullptr;    // reductions of kernels_rc.hip: the block in force (one of d_stats2), travels with d_sd
    uint32_t *d_stats2[2] = {nullptr, nullptr};
    vp8hip_batch *batch = nullptr;  // the batch this context is a member of
    // check_SSIM without the host round trip (vp8hip_check_ssim_async): the verdict lands in host memory the device writes
    int32_t *h_verdict = nullptr;   // {replaced, new_SSIM, min SSIM, time-out flag, filter updated, seq}: polled, no event
    uint32_t verdict_seq = 0;       // the seq the loop filter launch that carries the verdict will write last
    bool verdict_pending = false;   // that launch is enqueued
    hipStream_t verdict_stream = nullptr;   // ... on this stream (with vp8hip_filter_overlap not the one the context is on afterwards)
    bool chk_armed = false;         // vp8hip_check_ssim_async ran: the next loop filter launch carries the verdict
    int32_t chk_refqi[4] = {0, 0, 0, 0};
    int chk_qi_min = 0;
    unsigned intra_gen = 0;         // launches on intra_prog (its counters carry the launch number: nothing to clear)

    vp8::NetSet nets{};
    vp8::MBOut out{};
    vp8::SegData *d_sd = nullptr;        // the segment data in force (one of d_sd2)
    vp8::SegData *d_sd2[2] = {nullptr, nullptr};
    const vp8::SegData *lf_sd = nullptr; // what the loop filter in flight on lf_stream reads: the next frame's data go to the other buffer
    vp8::SegData *h_sd_ring = nullptr;   // pinned staging for vp8hip_set_segments
    unsigned sd_ring_pos = 0;
    int32_t *d_progress = nullptr;
    // a frame's reference searches on several devices (vp8hip_shard_*): this context's communicator
    ncclComm *shard_comm = nullptr;
    int shard_rank = 0, shard_world = 1;
    void *d_lf_handoff = nullptr;   // loop filter form 4: a band's bottom rows on their way to the next band (tagged granules)
    unsigned lf_launches = 0;       // window index of the loop filter's never-reset band counters
    int lf_type = 0;                // vp8hip_set_loop_filter_type: 0 normal, 1 simple
    unsigned lf_simple_launches = 0;   // ... the simple filter's own window index (its counters are its own, LF_SIMPLE_WORD)
    // THE INTAKE SETTINGS (intake_settings.h): every switch of the way a source frame becomes the current frame, changed by intake_apply
    // alone.  What follows down to seg_buf is what the stages own besides: buffers, histories, records.
    vp8::IntakeSettings in;
    // vp8hip_set_source_scaling: current frames come in at in.in_w x in.in_h (0 = no scaling) and k_scale_b makes in.src_w x in.src_h of
    // them (the coded size when those are 0); `scale` is what the launch reads, the tables live in scale.d_blob (an empty plan while in.in_w is 0)
    vp8::ScalePlan scale;
    // vp8hip_set_canvas: current frames are composed of in.n_tiles scaled sources (0 = no canvas) by k_compose_b, in the place of the
    // pack or scale launch; `canvas` is what the launch reads (the tiles' geometry and tables live in canvas.d_blob; an empty plan
    // without a canvas).  Tiles from the host pass through raw_stage, end to end.
    vp8::ComposePlan canvas;
    // vp8hip_set_source_format: what the three pointers of a current frame are (0 = I420: fmt_stage is not used).  k_convert_b makes tight
    // I420 of the incoming size of them in fmt_stage (tight_i420) and the pack or scale launch reads that.
    // vp8hip_set_source_colour: the colour matrix BGRA / RGBA frames are read with, and a tone-mapped frame is written with.
    // vp8hip_set_source_transfer: the transfer (0 = off) and peak P010 / I010 frames carry: k_tonemap_b in k_convert_b's place, with the
    // four tables of (in.src_transfer, in.src_peak) in tm_tables (made by the setter, released when the transfer goes back to 0).
    DeviceBuf fmt_stage, tm_tables;
    // vp8hip_set_overlay_host / _device: the layers burnt into every frame taken in, in slot order (ov_count of them are set; 0: no
    // launch, no buffer).  A slot keeps the layer's pixels (tight rows) and its prepared planes (overlay_planes; sized for any
    // placement); `stale`: the planes are not those of the placement in force -- the next intake launches k_overlay_prepare in front
    // of k_overlay_b, on its own stream.
    struct OverlaySlot {
        bool set = false, stale = false;
        int format = 0, matrix = 0, lw = 0, lh = 0, x = 0, y = 0, opacity = 0;
        DeviceBuf pixels, planes;
    };
    OverlaySlot ov[VP8HIP_MAX_OVERLAYS];
    int ov_count = 0;
    // planes from host memory that were not prefetched, on their way to a convert, deinterlace or scale launch, pass through here: the
    // planes in the source format end to end (incoming_bytes; the call synchronises before it returns: one buffer is enough)
    DeviceBuf raw_stage;
    // vp8hip_set_denoise: whether cur_prev holds a history (the previous frame taken in, as it left k_denoise_b, at
    // this level); the record (dn.d: the count / ticket word of the launch).  dn_host: the last frame taken in passed through and its
    // record is the host's own.
    bool dn_have_history = false, dn_taken = false, dn_host = false;
    Record<vp8::DenoiseMirror> dn;
    vp8::DenoiseMirror dn_passed{};
    // vp8hip_set_deinterlace: k_deinterlace_b writes tight I420 of the incoming size into di_stage
    // (planes laid out as in fmt_stage) and the pack or scale launch reads that.  Mode 2's history, the previous frame AS RECEIVED, is
    // di_hist[di_idx]; the launch that reads it copies the new frame into the other one and the two trade places (both of one size).
    // di_hist_w x di_hist_h: the incoming size the history was taken at (another size: no history).  The record: as the denoiser's
    // (di.d: the count / ticket word).
    bool di_have_history = false, di_taken = false;
    DeviceBuf di_stage, di_hist[2];
    int di_idx = 0, di_hist_w = 0, di_hist_h = 0;
    Record<vp8::DeinterlaceMirror> di;
    // vp8hip_set_source_window: the three pointers of a current frame are the plane bases of a surface whose rows are in.win_pitch[p] bytes
    // apart, and the frame is the window of the incoming size at (win_x, win_y).  k_window_b, in front of everything, writes the tight
    // planes end to end into win_stage (laid out as raw_stage) and the next stage reads that; planes from the HOST arrive windowed
    // (copy_planes: 2-D copies) and skip the launch.
    // vp8hip_set_source_orientation: or_turns clockwise quarter turns behind a left-right flip (or_mirror).  Every size of the context
    // describes the UPRIGHT frame; the planes handed in, the window, the converter and the deinterlacer are of the raw size
    // (incoming_size), which is the upright incoming size with width and height traded when or_turns is odd.  k_orient_b, behind the
    // deinterlacer, writes tight I420 of the upright size into or_stage (tight_i420) and the pack or scale launch reads that.
    DeviceBuf win_stage, or_stage;
    // vp8hip_set_analysis: one allocation (an.d: the five sum / ticket words of k_analyse_src_b, then at +256 the history plane -- the luma
    // of the previous frame taken in, tight, coded size) and one mirror (an.h) of three parts, each with a seq of its own: the views
    // an_src[frame & 1] and an_mb point into an.h and hold the seq their part's last launch writes and its stream (`an` itself is never waited for).
    // an_src_launches: source-side launches so far (the two an_src share the count).  an_src_frame, an_mb_frame: the frame each part was
    // last launched for.  an_checked: check_SSIM ran on the reconstruction in flight (its verdict's device copy says whether the
    // fallback's flags count).
    bool an_have_prev = false, an_checked = false;
    bool an_forced = false;         // vp8hip_intra_refresh ran on the reconstruction in flight: is_inter is defined, forced macroblocks count as intra
    Record<vp8::AnalysisMirror> an;
    RecordView<vp8::AnalysisSrcMirror> an_src[2];
    RecordView<vp8::AnalysisMbMirror> an_mb;
    uint32_t an_src_launches = 0;
    int an_src_frame[2] = {-1, -1}, an_mb_frame = -1;
    // vp8hip_set_segment_mode: 0 off, 1 the caller's map, 2 variance-adaptive at in.seg_strength.  seg_buf, made when the mode first leaves 0
    // (segment_buffers): the two sum words of k_aq_map_b (at 0 and 128: zero at rest), then five arrays of round256(mbs) bytes -- e and
    // the map of mode 2 for each of the two current-frame slots (cur_count & 1, as the analysis records: a frame may be taken in while
    // the one before it is coded), and the caller's map.  aq_frame: the frame each slot's map was made for; seg_map_set: a caller's map
    // is in force.
    bool seg_map_set = false;
    int aq_frame[2] = {-1, -1};
    DeviceBuf seg_buf;
    // vp8hip_arf_filter_device: arf_stage, made on first use and grown with the incoming size: the weight words of k_arf_filter_b
    // at 0, the filtered frame (tight_i420 of the incoming size) at 256.  arf_w x arf_h: the size the frame in it was made at (0: none).
    // arf_in: the window of vp8hip_arf_filter_host on its way to the device.
    DeviceBuf arf_stage, arf_in;
    int arf_w = 0, arf_h = 0;
    int conformant = 0;             // vp8hip_conformant_stream (NOT the reference; off by default)
    int lf_stall_test = 0;          // test hook (vp8hip_debug_lf_stall): make the next loop filters / intra wavefronts time out
    // vp8hip_set_quality_stats: the record (quality.d: the state, the ticket and the per-wave partials of k_quality)
    bool quality_on = false;
    bool recon_key = false;         // the reconstruction in flight came from the intra path ...
    bool lf_key = false;            // ... and so did the last filtered one
    Record<vp8::QualityState> quality;
    void *scratch = nullptr;        // device staging for debug pyramid downloads
    // coefficient entropy stage: per-block flags and third contexts, token counts per partition, probabilities
    uint8_t *ent_flags = nullptr, *ent_third = nullptr;
    uint32_t *ent_counts = nullptr, *ent_probs = nullptr, *ent_denom0 = nullptr;
    int ent_counted_partitions = 0; // partitions of the vp8hip_count_probs whose block contexts are current (0 = stale)
    DeviceArena arena;                   // every fixed device buffer of the context but the pixel planes (vp8hip_create)
    DeviceArena ent_arena, hdr_arena;    // the boolean coder's scratch for the coefficient partitions / the first partition
    vp8::EntBuffers ent{};               // boolean coder scratch, allocated on first vp8hip_encode_coefficients
    // vp8hip_filter_overlap: the context has a second stream and the loop filter and whatever does not depend on it run side
    // by side (the entropy stage of the same frame, the next frame's pack / parameter scan / GOLDEN + ALTREF searches).  The
    // FILTER stays on the stream the frame was coded on and the context moves over (`stream` and `lf_stream` trade places
    // in vp8hip_loop_filter and back in join_lf): a video's dependency chain -- LAST search, transform, filter, border, LAST
    // search ... -- is then launches of ONE stream, and the two cross-stream hand-offs (12 us each on this part) are on the
    // side work's path, which has 0.25 ms of slack.  Every entry point that needs the filtered frame joins first (join_lf).
    hipStream_t lf_stream = nullptr;   // the stream `stream` is not
    hipEvent_t ev_fork = nullptr, ev_lf = nullptr;
    hipEvent_t ev_src = nullptr;       // behind the current frame's pack / parameter scan / pyramid on the side stream: see side_sources_done()
    // A batch member's parameter scan (vp8hip_batch_auto_segments) waits here for the frame's longest launch, k_search2's, and rides in it
    // (launch_search2_batch); whoever needs the segment data earlier launches it on its own first (flush_scan).
    bool scan_deferred = false;
    vp8::ScanRequest scan_req{};
    bool lf_overlap = false, lf_pending = false;
    bool fork_by_verdict = false;      // the pending filter's launch has no fork event in front of it: see side_stream_ordered()
    bool fork_by_verdict_at_launch = false;   // ... as it was launched (fork_by_verdict is cleared once the ordering is established)
    int64_t lf_context_switches = 0;   // see vp8hip_profile_context_switches
    bool s2_clock_on = false;          // k_search2 stamps its launches (vp8hip_profile_search2_clock)
    bool frame_pending = false;     // between vp8hip_encode_frame_begin and _end
    bool frame_overflowed = false;  // ... and _end found the caller's buffer too small: the coded frame waits in h_frame for a retry
    hipEvent_t frame_event = nullptr;   // the end of the pending frame's entropy stage when it ran beside the chain (a batch's second stream, ent_stream)
    // vp8hip_filter_overlap: the entropy stage of a frame on a THIRD stream, beside its loop filter and beside the next frame's side
    // work -- a caller may start the next frame between vp8hip_encode_frame_begin and _end (the chain waits for the stage before
    // anything overwrites what it reads)
    // vp8hip_prefetch_current: the NEXT frame's planes (host memory) on their way into one of two staging buffers on a stream of their own,
    // while the current frame is coded; the vp8hip_upload_current that names the same planes packs from there and copies nothing
    hipStream_t h2d_stream = nullptr;
    hipEvent_t ev_h2d = nullptr, ev_stage_read[2] = {nullptr, nullptr};
    hipEvent_t ev_chroma = nullptr;    // behind the fold of vp8hip_chroma_change_async
    bool chroma_pending = false, chroma_none = false;
    bool chroma_by_batch = false;      // the pending scan is vp8hip_batch_chroma_change_async's: its event is the batch's
    bool stage_read_valid[2] = {false, false};
    DeviceBuf h2d_stage[2];            // (both of the planes' exact size: a prefetch counts only for the size it was made for)
    int h2d_idx = 0;
    const void *h2d_pre[3] = {nullptr, nullptr, nullptr};
    bool h2d_pre_valid = false;
    hipStream_t ent_stream = nullptr;
    hipEvent_t ev_ent = nullptr;
    bool ent_pending = false;           // the chain has not yet been told to wait for ev_ent
    unsigned out_gen = 0, frame_gen = 0;   // frames whose results went into `out` so far / when the pending frame's stage was enqueued
    bool counted = false;           // in g_live_contexts
    vp8hip_header_params frame_params{};
    int frame_partitions = 0;
    int ent_bools_per_block = 64;   // what that scratch is sized for; doubled (up to 304, the maximum) when a frame needs more
    // host intra path on the device: sub-block modes, replaced flags, row progress, {replaced, new_SSIM, min SSIM}
    int32_t *intra_modes = nullptr, *intra_is_inter = nullptr, *intra_prog = nullptr, *intra_stats = nullptr;
    // first partition on the device: its own coder scratch, per-workgroup statistics, probability table, {H, skip_prob, replaced}
    vp8::EntBuffers hdr{};
    uint32_t *hdr_partial = nullptr, *hdr_info = nullptr;
    uint8_t *hdr_sym = nullptr;
    uint8_t *h_frame = nullptr;     // pinned staging of vp8hip_encode_frame's read-back (pageable targets serialise inside the runtime)
    uint8_t *d_frame = nullptr;     // the frame as gathered on the device: [0] size, [1] first-partition size, bytes from +16
    size_t h_frame_cap = 0;

    uint32_t prof_mask = 0;
    hipEvent_t ev[vp8::MAX_EVENTS];
    int ev_kernel[vp8::MAX_EVENTS / 2];
    int ev_used = 0;
    int ev_made = 0;                // ev[0 .. ev_made) are taken from the process's pool so far (event_pool_get)
    double prof_ms[VP8HIP_K_COUNT] = {0};
    int64_t prof_n[VP8HIP_K_COUNT] = {0};
};

// Up to MAX_BATCH contexts of one geometry on one device advance one frame together (see "batched contexts" below).
// `prep` is the batch's second stream: what a frame needs done before its searches but what does not depend on the previous
// frame's reconstruction -- taking the new frame in (pack / copy_with_padding), the parameter scan with the segment data, the
// new frame's pyramid -- runs there, beside the previous frame's chain on `stream`, instead of at the head of the chain behind the
// loop filter.  In the kernel trace of 48 chunks in 8 batches those three launches, a few microseconds of work each, lasted
// 0.2-0.45 ms per frame waiting for their turn: a fifth of the summed kernel time.
struct vp8hip_batch {
    int n = 0;
    vp8hip_ctx *c[vp8::MAX_BATCH] = {};
    hipStream_t stream = nullptr;        // the chain's stream: a lane of the device's pool (shared with other batches), or the batch's own
    int lane = -1;                       // which lane of the pool (api_batch.hip, batch_lanes.h); -1: `stream` is this batch's alone
    hipStream_t prep = nullptr;          // nullptr: everything on `stream` (VP8HIP_BATCH_PREP=0)
    bool prep_shared = false;            // prep is the process-wide one (VP8HIP_BATCH_PREP=2), not this batch's to destroy
    hipEvent_t ev_gate = nullptr;        // on `stream`, at the start of a frame call: everything of the earlier frames
    hipEvent_t ev_gate2 = nullptr;       // (the two alternate: a wait never names an event that is recorded again right behind it)
    hipEvent_t ev_prep = nullptr;        // on `prep`: the head-of-frame work enqueued so far
    bool prep_pending = false;           // `stream` has not yet been told to wait for ev_prep
    // The entropy stage of the members' frames beside their loop filter (vp8hip_batch_encode_frame_begin): a second stream, forked
    // from `stream` right before the filter's launch (ev_ent_fork) and joined back behind the stage (ev_ent).
    hipStream_t ent = nullptr;           // nullptr: the stage stays in the chain (VP8HIP_BATCH_ENT_STREAM=0)
    hipEvent_t ev_ent_fork = nullptr, ev_ent = nullptr;
    bool ent_fork_fresh = false;         // nothing was enqueued for a member since ev_ent_fork was recorded
    hipEvent_t ev_chroma = nullptr;      // behind the launch of vp8hip_batch_chroma_change_async (made on first use)
    // vp8hip_batch_upload_current: the members' new frames from HOST memory.  The copies run on a stream of their own (the copy engines,
    // beside whatever the batch's stream still has: the previous frame's loop filter) into one of two staging buffers per member; the
    // launch that packs them waits for the copies, the copies for the pack that last read their buffer.
    hipStream_t copy = nullptr;
    hipEvent_t ev_copied = nullptr, ev_packed[2] = {nullptr, nullptr};
    bool packed_valid[2] = {false, false};
    DeviceBuf stage[vp8::MAX_BATCH][2];
    size_t stage_bytes = 0;              // the planes' exact size all of them were made for (0: not all made)
    int stage_fmt = 0;                   // the source format the staging buffers' planes were laid out for
    int stage_idx = 0;
    // vp8hip_batch_prefetch_current: the NEXT frame's planes already on their way into the buffer the next upload will pack from
    const void *pre[vp8::MAX_BATCH][3] = {};
    bool pre_valid = false;
};

#define HIPCHK(c, call)                                  \
    do {                                                 \
        hipError_t e_ = (call);                          \
        if (e_ != hipSuccess) {                          \
            (c)->last_hip_error = (int)e_;               \
            return VP8HIP_ERR_HIP;                       \
        }                                                \
    } while (0)

// The one wait for a word a launch writes last into host memory (api_context.hip): VP8HIP_OK once *word == want.
int wait_for_seq(vp8hip_ctx *c, const uint32_t *word, uint32_t want, hipStream_t s);

template <class Mirror> int Record<Mirror>::make(vp8hip_ctx *c, size_t device_bytes, size_t zeroed_bytes) {
    if (d) return VP8HIP_OK;
    uint8_t *nd = nullptr;
    Mirror *nh = nullptr;
    HIPCHK(c, hipMalloc(&nd, device_bytes));
    hipError_t e = zeroed_bytes ? hipMemset(nd, 0, zeroed_bytes) : hipSuccess;
    if (e == hipSuccess) e = hipHostMalloc(&nh, sizeof(Mirror), hipHostMallocCoherent);
    if (e != hipSuccess) { (void)hipFree(nd); c->last_hip_error = (int)e; return VP8HIP_ERR_HIP; }
    memset(nh, 0, sizeof(Mirror));
    d = nd;
    this->h = nh;
    return VP8HIP_OK;
}
template <class Mirror> int RecordView<Mirror>::wait(vp8hip_ctx *c) const { return wait_for_seq(c, &h->seq, seq, stream); }
template <class Mirror> void Record<Mirror>::release() {
    if (this->h) (void)hipHostFree(this->h);
    (void)hipFree(d);
    this->h = nullptr;
    d = nullptr;
}

namespace vp8 {

// The event behind which a host thread reads a finished frame out of pinned memory the stage's last kernel wrote: recorded with a
// SYSTEM-scope release.  An event made with hipEventDisableTiming alone releases to the device only, and the host then read, once in
// a few hundred frames, the previous frame's size word (the frame tag's first-partition size was the symptom).
static constexpr unsigned FRAME_EVENT_FLAGS = hipEventDisableTiming | hipEventReleaseToSystem;

// ---- per-kernel event timing --------------------------------------------------------------------
// Stages that are ONE kernel launch get their two events recorded by the dispatch itself (VP8_LAUNCH, vp8hip_dev.h): the
// kernel's own begin and end.  Stages made of several launches (entropy stage, intra) are bracketed with hipEventRecord.
// On a LANE that batches share (api_batch.hip) the two kinds differ: a dispatch's own events time that kernel whatever else is on
// the lane, and so does k_search2's launch clock (s2_clock: stamped by the launch's own workgroups into its context's words), but a
// bracket spans whatever the other batch's thread enqueued between the two records -- the bracketed stages' times of a batch that
// shares its lane are upper bounds.  bench.py's roofline kernels are all single-launch stages.
constexpr uint32_t SINGLE_LAUNCH_STAGES = (1u << VP8HIP_K_PACK) | (1u << VP8HIP_K_DOWNSAMPLE) | (1u << VP8HIP_K_SEARCH1_L4) | (1u << VP8HIP_K_SEARCH1_L3) |
                                          (1u << VP8HIP_K_SEARCH1_L2) | (1u << VP8HIP_K_SEARCH1_L1) | (1u << VP8HIP_K_SEARCH1_L0) | (1u << VP8HIP_K_SEARCH2) |
                                          (1u << VP8HIP_K_MB) | (1u << VP8HIP_K_LOOP_FILTER) | (1u << VP8HIP_K_BORDER);
hipEvent_t event_pool_get(int device);
void event_pool_put(int device, hipEvent_t *ev, int n);

struct Timed {
    vp8hip_ctx *c;
    int slot = -1;
    bool by_dispatch = false;
    Timed(vp8hip_ctx *ctx, int kernel) : c(ctx) {
        if (!(c->prof_mask & (1u << kernel)) || c->ev_used + 2 > MAX_EVENTS) return;
        while (c->ev_made < c->ev_used + 2) {   // taken when first needed: a context that times nothing holds none
            hipEvent_t e = event_pool_get(c->device);
            if (!e) return;
            c->ev[c->ev_made++] = e;
        }
        slot = c->ev_used;
        c->ev_kernel[slot / 2] = kernel;
        c->ev_used += 2;
        by_dispatch = (SINGLE_LAUNCH_STAGES >> kernel) & 1u;
        if (by_dispatch) {
            tl_timing.start = c->ev[slot];
            tl_timing.stop = c->ev[slot + 1];
            tl_timing.launches = 0;
        } else {
            hipEventRecord(c->ev[slot], c->stream);
        }
    }
    ~Timed() {
        if (slot < 0) return;
        if (by_dispatch) {
            if (tl_timing.launches == 0) c->ev_used -= 2;   // nothing was launched (a pyramid level without a block): give the slot back
            tl_timing = LaunchTiming{};
        } else {
            hipEventRecord(c->ev[slot + 1], c->stream);
        }
    }
};

// ---- api_context.hip: surfaces, parameters, stream ordering ----
extern std::atomic<int> g_live_contexts;   // chain streams in use: contexts on a stream of their own, lanes with a batch, batches with a stream of their own
void note_queue_oversubscription();
int pick_free_frame(const vp8hip_ctx *c);
int copy_in(vp8hip_ctx *c, const Plane &dst, const void *src, hipMemcpyKind kind);
int copy_out(vp8hip_ctx *c, void *dst, const Plane &src);
void build_pyramid(vp8hip_ctx *c, Frame *a, Frame *b, uint32_t border_mask = 0);
int make_last(vp8hip_ctx *c, const void *y, const void *u, const void *v, hipMemcpyKind kind);
SegData *sd_for_writing(vp8hip_ctx *c);
void next_params(vp8hip_ctx *c);
ScanRequest scan_request(const vp8hip_ctx *c, int is_key, const int32_t refqi[4], int qi_min);
void next_current(vp8hip_ctx *c);
int join_ent(vp8hip_ctx *c);
hipStream_t join_lf_swap(vp8hip_ctx *c);
int join_lf_wait(vp8hip_ctx *c, hipStream_t side);
bool side_sources_done(vp8hip_ctx *c);
int join_lf(vp8hip_ctx *c, bool defer_ent = false);
void flush_scan(vp8hip_ctx *c);
void batch_join_prep(vp8hip_batch *b);
void side_stream_ordered(vp8hip_ctx *c);
int check_device_timeout(vp8hip_ctx *c);
// ---- api_intake.hip: how a frame becomes current ----
int set_frame_planes(vp8hip_ctx *c, Frame &f, const void *y, const void *u, const void *v, hipMemcpyKind kind, int sw = 0, int sh = 0);
// the sizes of intake_settings.h for a context's settings in force
inline void upright_size(const vp8hip_ctx *c, int *w, int *h) { upright_size(c->in, c->W, c->H, w, h); }
inline void incoming_size(const vp8hip_ctx *c, int *w, int *h) { incoming_size(c->in, c->W, c->H, w, h); }
inline void incoming_bytes(const vp8hip_ctx *c, size_t bytes[3]) { incoming_bytes(c->in, c->W, c->H, bytes); }
inline void picture_size(const vp8hip_ctx *c, int *w, int *h) { picture_size(c->in, c->W, c->H, w, h); }
inline int window_rule(const vp8hip_ctx *c, size_t off[3], int32_t row_bytes[3], int32_t rows[3]) { return window_rule(c->in, c->W, c->H, off, row_bytes, rows); }
// what one batched convert / pack / scale launch takes as one value: the members' settings are equal
inline bool same_intake(const vp8hip_ctx *a, const vp8hip_ctx *b) { return a->in == b->in; }
static_assert(INTAKE_OK == VP8HIP_OK && INTAKE_REFUSED == VP8HIP_ERR_ARG, "intake_valid returns the library's codes");
// THE ONE WAY a setting changes: nothing to do when `next` (canonical) is what is in force; refused (intake_valid) with nothing
// changed; otherwise whatever is in flight ends, the stages' buffers are made for the new settings (on failure the old ones stay in
// force), and planes prefetched under another SourceShape are dropped, the context's and its batch's: they are handed over again.
int intake_apply(vp8hip_ctx *c, const IntakeSettings &next);
// whatever is in flight on the context's streams (and its batch's) ends: setters and growing buffers, never per frame
int quiesce_intake(vp8hip_ctx *c);
// a frame's planes (nb: their bytes in the source format; a format of two planes or one never reads the later pointers) end to end into d,
// on stream s: ONE copy when they lie end to end already (an I420 frame as a file reader or a decoder holds it).  A context with a
// window: y, u, v are the plane bases of a surface and only the window's bytes travel, one 2-D copy per plane.
int copy_planes(vp8hip_ctx *c, uint8_t *d, const void *y, const void *u, const void *v, const size_t nb[3], hipMemcpyKind kind, hipStream_t s);
// the buffers the members' next frames need, at their incoming size (as a rule: they are there); changes nothing else
int intake_ready(vp8hip_ctx *const *m, int n);
// THE ORDER, once: n contexts of one intake (same_intake) take their new current frames in on stream s -- window, convert, deinterlace,
// orient, scale or pack, overlay, denoise, analysis.  y, u, v: the members' planes in DEVICE memory in their source format: the plane bases of
// their surfaces when the contexts have a window, unless `tight` (planes that came from the host through copy_planes are the window already).
// alone: nullptr for a batch's members.  For a context on its own (n == 1, s its stream) it points at where the planes are: such a
// context keeps the pack launch of one, and without a format, deinterlacer or scaler its planes may be the host's, copied straight
// into the surface.
// planes_read (or nullptr) is recorded behind the pack or scale launch: nothing behind it reads the caller's planes.
int take_frames(vp8hip_ctx *const *m, const void *const *y, const void *const *u, const void *const *v, int n, hipStream_t s,
                const hipMemcpyKind *alone = nullptr, hipEvent_t planes_read = nullptr, bool tight = false);
// ... and what stands behind the pack, scale or compose launch, shared by every way in: planes_read is recorded, then overlay, denoise,
// analysis, segment map on the members' new current frames.
int finish_frames(vp8hip_ctx *const *m, int n, hipStream_t s, hipEvent_t planes_read);
// ---- api_inter.hip ----
void drop_overflowed_frame(vp8hip_ctx *c);
int inter_check(const vp8hip_ctx *c, int prev_is_golden, int prev_is_altref, int use_golden, int use_altref);
int inter_begin(vp8hip_ctx *c, int prev_is_golden, int prev_is_altref, int use_golden, int use_altref);
RefSet ref_set(const vp8hip_ctx *c, int use_last, int use_golden, int use_altref);
unsigned long long *s2_clock_words(const vp8hip_ctx *c);
unsigned long long *s2_clock(const vp8hip_ctx *c);
CodingItem coding_item(const vp8hip_ctx *c, int use_golden, int use_altref);
int claim_recon(vp8hip_ctx *c);
void recon_made(vp8hip_ctx *c, bool key);
void recon_filtered(vp8hip_ctx *c);
void check_item(vp8hip_ctx *c, CheckItem &it, const int32_t refqi[4], int qi_min);
FilterItem filter_item(vp8hip_ctx *c);
bool fallback_possible(float ssim_target);
// ---- api_entropy.hip ----
constexpr size_t FRAME_FIRST_COPY = 192 * 1024;
bool frame_zero_copy();
int frame_prepare(vp8hip_ctx *c, int P, const vp8hip_header_params *p, FrameEntropy &e, FrameOut &fo);
// ---- api_shard.hip ----
void shard_release(vp8hip_ctx *c);            // the context's communicator, if it has one
int receive_last_surface(const vp8hip_ctx *c);
int adopt_last(vp8hip_ctx *c, int idx);
// ---- api_profile.hip ----
int prof_collect(vp8hip_ctx *c);
// ---- api_denoise.hip ----
// The frame just packed or scaled into c->cur passes through the denoiser (take_frames: right behind the pack, on the pack's stream).  denoise_item: false = nothing to launch (off, or no history: the frame passes through and
// is the history from now on).
bool denoise_item(vp8hip_ctx *c, hipStream_t s, DenoiseItem &it);
// ---- api_overlay.hip ----
// The frame just packed or scaled into c->cur takes the context's layers (take_frames: behind the pack or scale launch and in front of
// the denoiser, on the same stream s).  overlay_item: launches k_overlay_prepare on s for the slots whose planes are stale; false = no
// layer covers the picture, nothing to launch.  overlay_release: every slot's buffers (vp8hip_destroy).
bool overlay_item(vp8hip_ctx *c, hipStream_t s, OverlayItem &it);
void overlay_release(vp8hip_ctx *c);
// ---- api_deinterlace.hip ----
// The frame about to be packed or scaled passes through the deinterlacer (take_frames: behind the convert launch and in front of the
// pack or scale launch, on the same stream).  deinterlace_ready: the staging and history buffers at the context's incoming size.
// deinterlace_item: y, u, v = tight I420 in DEVICE memory; afterwards they are the planes in di_stage.  false: off, nothing to launch.
int deinterlace_ready(vp8hip_ctx *c);
bool deinterlace_item(vp8hip_ctx *c, hipStream_t s, DeinterlaceItem &it, const void *&y, const void *&u, const void *&v);
// ---- api_analysis.hip ----
// The source side: the frame just taken into c->cur, behind its pack / scale / denoise launches on stream s (take_frames).  The coding side: the attempt whose loop filter was just launched on s (c->lf_key says which kind).
// *_item: false = analysis off, nothing to launch.
bool analysis_src_item(vp8hip_ctx *c, hipStream_t s, AnalysisSrcItem &it);
bool analysis_mb_item(vp8hip_ctx *c, hipStream_t s, AnalysisMbItem &it);
void analysis_after_filter(vp8hip_ctx *c, hipStream_t s);
void batch_analysis(vp8hip_batch *b, const int *active);
// ---- api_segment.hip ----
// The variance-adaptive map of the frame just taken into c->cur, at the end of the intake chain (take_frames).  false: not mode 2,
// nothing to launch.  segment_map_in_force: what the mapped k_mb reads for the current frame -- the caller's map in mode 1, the
// current slot's map in mode 2, nullptr (segment 3 everywhere) without one, and in mode 0.
bool aq_item(vp8hip_ctx *c, AqItem &it);
const uint8_t *segment_map_in_force(const vp8hip_ctx *c);
// ---- api_quality.hip ----
bool quality_item(vp8hip_ctx *c, const Frame &rec, hipStream_t s, QualityArgs &a);   // false: stats off
void quality_after_filter(vp8hip_ctx *c, const Frame &rec, hipStream_t s);           // the measurement behind the context's filter
int batch_quality(vp8hip_batch *b, const int *active);

}  // namespace vp8

// HIP's current device is per host thread: a context may be driven from a thread other than its creator's, or two contexts
// on two GPUs from one thread -- every entry point that may allocate or use the null stream selects the context's device.
// A member of a batch launches on the batch's stream: whatever it does there comes after the batch's head-of-frame work.
// vp8hip_filter_overlap: the side stream's work must start behind everything the frame's chain enqueued BEFORE the filter (the next
// frame's GOLDEN / ALTREF searches overwrite nets the frame's k_mb reads).  An event recorded in front of the filter's launch says
// so on the device -- and costs the chain 12 us per frame: a marker packet with a completion signal between k_mb and the filter
// (0.375 -> 0.362 ms per 1080p frame without it).  When the filter's launch carries check_SSIM's verdict, the verdict itself is
// the proof: its sequence number arrives in host memory from INSIDE that launch, and a launch starts when everything before it on
// its stream has completed.  So no event is recorded then, and the first entry point that would enqueue on the side stream makes
// sure the number is there (the native frame loop has taken the verdict by then anyway: nothing waits).
#define USE_DEVICE(c) do { if (c) { (void)hipSetDevice((c)->device); batch_join_prep((c)->batch); side_stream_ordered(c); flush_scan(c); } } while (0)
#define USE_DEVICE_ONLY(c) do { if (c) (void)hipSetDevice((c)->device); } while (0)
#define JOIN_LF(c) do { if (c) { const int jr_ = join_lf(c); if (jr_) return jr_; } } while (0)

#endif
