/*
 * vp8hip_driver.h -- the reference's frame loop (main(), src/vp8enc.cpp:351-488) as native host code over
 * include/vp8hip.h and include/vp8hip_host.h.
 *
 * The reference host is C++ and this is its C++ counterpart (vp8oclenc_amd/csrc/vp8_driver.cpp): frame-type
 * state machine, per-frame loop-filter strength and segment data, key frames (intra_transform), inter_transform,
 * check_SSIM with its intra fallback, its filter-parameter update and its "redo as key frame" decision, filter
 * mask, loop filter -- in the reference's order, every stage on the device.  scene_change()'s decision is the caller's
 * (force_key; vp8hip_chroma_change + vp8host_scene_change produce it) or, with cfg.scene_detect, made here the same way.  Not here: the header/MV entropy
 * coder and the container.
 * vp8oclenc_amd/driver.py is the same loop in Python for the parity tests (it also runs the CPU oracle).
 */
#ifndef VP8HIP_DRIVER_H
#define VP8HIP_DRIVER_H

#include <stddef.h>
#include <stdint.h>

#include "vp8hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vp8drv vp8drv;

typedef struct {
    int32_t gop_size;        /* -g, frames between key frames (init.h:1575) */
    int32_t altref_range;    /* frames between altref frames (vp8enc.cpp:340-344) */
    int32_t qi_min, qi_max;  /* -qmin / -qmax -> the two quantizer ladders (init.h:1585-1603) */
    float ssim_target;       /* -SSIM-target (init.h:1512,1576) */
    int32_t device_params;   /* 1: loop-filter strength + segment data on the device, no host round trip
                                (vp8hip_auto_segments); 0: host mirror on the caller's luma plane */
    int32_t check_ssim;      /* 1: check_SSIM after every inter_transform (vp8enc.cpp:231-263, 442-453) -- what the reference does:
                                intra fallback, filter update when even the worst macroblock is above 0.95, redo as key frame.
                                With device_params the call does not wait for it (vp8hip_check_ssim_async): fallback, statistics
                                and filter update run on the device in front of the loop filter, and the one decision that is the
                                host's -- redo as key frame -- is taken when the verdict is next needed: at the start of the next
                                vp8drv_encode_frame_* / vp8drv_batch_encode_frame_device, in vp8drv_get_frame[_begin], or in
                                vp8drv_resolve.  Until then the return value "inter frame" and the counters of vp8drv_get_stats
                                are provisional.  (A bounded device-side wait of the SAME frame's loop filter that expires is
                                reported one step later still: the verdict workgroup samples the error word when the filter's
                                launch starts, so a time-out inside that launch shows in the next verdict or in
                                vp8hip_synchronize / vp8drv_get_frame, whichever comes first.)  With device_params == 0 the
                                host sits in the middle, as in the reference.
                                0: skip it (the reference's loop minus the filter update; kept for A/B runs) */
    int32_t num_partitions;  /* -partitions: 1, 2, 4 or 8 coefficient partitions (init.h:1451-1469, default 1) */
    int32_t display_width, display_height;   /* video.dst_width/height written into key frames; 0 = the coded size */
    int32_t host_bitstream;  /* vp8drv_get_frame: 0 = the whole entropy stage on the device (vp8hip_encode_frame);
                                1 = first partition on the host (vp8bs_encode_header) after downloading what it reads,
                                the way the reference does it -- kept as the cross-check */
    int32_t overlap_filter;  /* 1: loop filter on its own stream, side by side with the frame's entropy stage
                                (vp8hip_filter_overlap); for a single video coded frame after frame.  Default 0 */
    int32_t ref_mask;        /* which of the two optional references inter frames may search besides LAST: bit 0 GOLDEN,
                                bit 1 ALTREF, ANDed onto the reference's own rule (inter_part.h:103-104).  Default 3 (= the
                                reference); 0 = LAST only (BASELINE configs[1]) */
    int32_t conformant_stream;   /* 1 = vp8hip_conformant_stream: the stream decodes to the encoder's own reconstruction (the
                                format's predictor, the kept attempt's modes); 0 = the reference's stream, byte for byte.
                                Default 0 */
    int32_t scene_detect;        /* 1: scene_change() (vp8enc.cpp:265-311, 408-416) inside the loop: the chroma differences to the
                                previous input frame on the device (vp8hip_chroma_change; blocks for two words per frame),
                                the decision with its hold-over on the host (vp8host_scene_change); a detected cut is coded
                                as a key frame.  0 (default): the caller's force_key alone decides */
    int32_t src_width, src_height;   /* size of the frames handed to vp8drv_encode_frame_* when it is below the coded size
                                (video.src_* against video.wrk_*, init.h:375-392): copy_with_padding (encIO.h:141-196) then
                                runs on the device (vp8hip_set_source_size) and key frames carry this size as the display
                                size unless display_width/height say otherwise.  0 = frames of the coded size.  Needs
                                device_params = 1 */
    int32_t loop_filter_type;    /* 0 (default): the normal loop filter, the reference's; 1: the simple loop filter (RFC 6386
                                section 15.2, vp8hip_set_loop_filter_type), written into every frame header.  Other values:
                                vp8drv_create returns VP8HIP_ERR_ARG.  Members of a batch must agree */
    int32_t in_width, in_height, scale_filter;   /* in_* non-zero: the frames handed to vp8drv_encode_frame_* (and the prefetch / stage /
                                batched forms) have THIS size and are scaled down on the device (vp8hip_set_source_scaling) to
                                src_width x src_height, or to the coded size when those are 0; scale_filter 0 = area, 1 = Lanczos-3.
                                Key frames carry the size scaled TO as the display size, as they carry src now.  Needs
                                device_params = 1; vp8drv_create returns VP8HIP_ERR_ARG for whatever the setter refuses.
                                0, 0 (default): no scaling.  Members of a batch must agree.  (They stand in front of
                                quality_stats, which stays the struct's last field.) */
    int32_t quality_stats;       /* 1: PSNR and SSIM of every coded frame, measured on the device (vp8hip_set_quality_stats):
                                vp8drv_get_frame_quality, vp8drv_get_quality_summary.  0 (default): off.  Other values:
                                vp8drv_create returns VP8HIP_ERR_ARG */
} vp8drv_config;

void vp8drv_default_config(vp8drv_config *cfg);   /* the reference's defaults: 150, 5, 0, 48, -1, 1, 1, 1, 0, 0, 0, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0 */

int vp8drv_create(vp8drv **out, int width, int height, int device_ordinal, const vp8drv_config *cfg);
void vp8drv_destroy(vp8drv *d);
vp8hip_ctx *vp8drv_context(vp8drv *d);   /* for downloads, the entropy stage, profiling */

/* One iteration of the while-loop body, vp8enc.cpp:351-488, for a frame whose planes are already in this
 * device's memory (tight stride).  Returns 1 = coded as a key frame, 0 = inter frame, < 0 = vp8hip_status.
 * force_key: the caller's scene_change() verdict (vp8enc.cpp:408-416).  Asynchronous unless check_ssim is on. */
int vp8drv_encode_frame_device(vp8drv *d, const void *d_y, const void *d_u, const void *d_v, int force_key);
/* same for host planes (blocks for the upload).  With device_params == 0 the host mirror scans y. */
int vp8drv_encode_frame_host(vp8drv *d, const uint8_t *y, const uint8_t *u, const uint8_t *v, int force_key);
/* The frame AFTER the one just handed in, started on its way to the device (vp8hip_prefetch_current): a reader that is one frame ahead
 * calls this right after vp8drv_encode_frame_host and hands the same pointers to the next vp8drv_encode_frame_host. */
int vp8drv_prefetch_frame_host(vp8drv *d, const uint8_t *y, const uint8_t *u, const uint8_t *v);
/* ... and handed over altogether -- made the context's current frame (a pack from the prefetch's staging buffer), with cfg.scene_detect its
 * chroma scan started (vp8hip_chroma_change_async) -- while the frame just coded is still in its loop filter: a reader that is a frame ahead
 * calls this after vp8drv_get_frame_begin (or vp8drv_resolve) of the frame just coded and hands the same pointers to the next
 * vp8drv_encode_frame_host, which then uploads nothing and waits for no scan: the new frame's side work is enqueued a hundred microseconds
 * earlier, early enough to run beside the previous frame's loop filter (scripts/native/y4m_to_ivf.cpp).  Takes the open verdict first. */
int vp8drv_stage_frame_host(vp8drv *d, const uint8_t *y, const uint8_t *u, const uint8_t *v);

/* With check_ssim: waits for the verdict on the frame just coded and, if it sends the frame back (vp8enc.cpp:443-453), codes it
 * again as a key frame.  Returns 1 if the last frame ended as a key frame, 0 if as an inter frame, < 0 = vp8hip_status.  Implied by
 * the next vp8drv_encode_frame_* and by vp8drv_get_frame[_begin]; a no-op when nothing is open. */
int vp8drv_resolve(vp8drv *d);
/* 1 if the next call on this driver (this batch) would not wait for a verdict: a host that advances several chunks from one
 * thread takes the ones that are ready first instead of waiting for them in a fixed order */
int vp8drv_ready(const vp8drv *d);

/* The frame just coded, as bytes: entropy_encode() + gather_frame() of the reference (vp8enc.cpp:48-94, 476-481;
 * encIO.h:1-30) -- coefficient statistics, coefficient partitions and the first partition (frame header, macroblock
 * modes, motion vectors) coded on the device and assembled into `out` (vp8hip_encode_frame; with host_bitstream the
 * first partition comes from the host coder of include/vp8hip_bitstream.h instead).  Call it after vp8drv_encode_frame_* and before the next one.
 * Blocks.  *size = bytes written; VP8HIP_ERR_OVERFLOW if `capacity` is too small.  With vp8bs_ivf_file_header /
 * vp8bs_ivf_frame_header around the frames this is the reference's .ivf output, byte for byte. */
int vp8drv_get_frame(vp8drv *d, uint8_t *out, size_t capacity, size_t *size);
/* The same in two halves (device entropy stage only: VP8HIP_ERR_STATE with host_bitstream): _begin enqueues the
 * stage and returns, _end waits and fills `out`.  One host thread can thus keep many GOP chunks in flight:
 * encode_frame + get_frame_begin on every chunk, then get_frame_end on every chunk.  With cfg.overlap_filter (one video frame
 * after frame) the NEXT frame may be started between the two -- encode(t), get_frame_begin(t), encode(t + 1), get_frame_end(t): the
 * stage of frame t runs beside its loop filter and beside frame t + 1's input side (vp8hip_encode_frame_begin, include/vp8hip.h;
 * call vp8hip_reserve_frame_path_dense(vp8drv_context(d)) once); without it no other call on this driver between the two. */
int vp8drv_get_frame_begin(vp8drv *d);
int vp8drv_get_frame_end(vp8drv *d, uint8_t *out, size_t capacity, size_t *size);

/* Several GOP chunks advanced one frame at a time, every stage ONE launch for all of them (vp8hip_batch_* in vp8hip.h): what a
 * host with many chunks in flight uses instead of one stream per chunk -- the part runs four to five kernels at once, so
 * sixteen narrow launches queue where four wide ones fill it.  Members: up to VP8HIP_MAX_BATCH drivers of one geometry
 * with device_params = 1, overlap_filter = 0, scene_detect = 0 and the same qi_min / qi_max / num_partitions / check_ssim.  One call = vp8drv_encode_frame_device on every member
 * (force_key / was_key indexed by member, either may be NULL); a member whose frame is a key frame takes its ordinary key-frame
 * path on the shared stream.  vp8drv_get_frame[_begin/_end] per member afterwards, as usual. */
typedef struct vp8drv_batch vp8drv_batch;
int vp8drv_batch_create(vp8drv_batch **out, vp8drv *const *drv, int n);
void vp8drv_batch_destroy(vp8drv_batch *b);      /* the drivers stay */
int vp8drv_batch_lane(const vp8drv_batch *b);    /* vp8hip_batch_lane of the batch underneath: the chain stream it shares, -1 = its own */
int vp8drv_batch_encode_frame_device(vp8drv_batch *b, const int *members /* NULL = all; 0 = this member sits the call out */,
                                     const void *const *y, const void *const *u, const void *const *v, const int *force_key, int *was_key);
/* ... with the members' frames in host memory (vp8hip_batch_upload_current: tight planes of the source size, page-locked for the copies
 * to be asynchronous, unchanged until the next call on this batch has returned) */
int vp8drv_batch_encode_frame_host(vp8drv_batch *b, const int *members, const void *const *y, const void *const *u, const void *const *v,
                                   const int *force_key, int *was_key);
/* the members' NEXT frames started on their way (vp8hip_batch_prefetch_current; y[i] NULL: nothing for member i): hand the same pointers
 * to the next vp8drv_batch_encode_frame_host */
int vp8drv_batch_prefetch_frame_host(vp8drv_batch *b, const uint8_t *const *y, const uint8_t *const *u, const uint8_t *const *v);
/* Scene cuts in GOP-parallel coding.  The serial loop's key-frame schedule with scene_detect on is a function of the chroma differences
 * of consecutive frames as taken in and of the GOP length (vp8host_scene_plan, include/vp8hip_host.h), so a host scans the file first
 * -- members of a batch each walking a segment of it, the frame before the segment first -- plans, and then codes the chunks between
 * the planned key frames side by side, each started with force_key.
 * vp8drv_batch_scan_frame_*: the members' frames are taken in (as vp8drv_batch_encode_frame_* takes them in, prefetch included) and the
 * differences against each member's previous frame started, ONE launch for all (vp8hip_batch_chroma_change_async).  Nothing is coded;
 * the GOP state, the scene history and the statistics do not move.  vp8drv_batch_scan_result: udiff[i], vdiff[i] of the members of the
 * last scan call (zeros for a member's first frame).  A batch that has scanned codes afterwards what a fresh batch codes, byte for byte.
 * VP8HIP_ERR_STATE, and nothing changed, when a member of the call has the denoiser on, deinterlace mode 2, analysis or quality
 * statistics: each keeps a history of the frames taken in or numbers them, and frames taken in without being coded would change it. */
int vp8drv_batch_scan_frame_device(vp8drv_batch *b, const int *members, const void *const *y, const void *const *u, const void *const *v);
int vp8drv_batch_scan_frame_host(vp8drv_batch *b, const int *members, const void *const *y, const void *const *u, const void *const *v);
int vp8drv_batch_scan_result(vp8drv_batch *b, const int *members, int32_t *udiff, int32_t *vdiff);
/* vp8drv_get_frame_begin for the members' frames in one set of launches (src/vp8enc.cpp:48-94 for up to four chunks at
 * once); then vp8drv_get_frame_end on every member */
int vp8drv_batch_get_frame_begin(vp8drv_batch *b, const int *members);
int vp8drv_batch_ready(const vp8drv_batch *b);
/* One frame on EVERY batch of `batches` -- vp8drv_batch_encode_frame_device(batches[k], NULL, y[k], u[k], v[k], NULL, was_key[k])
 * (was_key may be NULL, and so may any was_key[k]) -- in the order of the array, each batch waiting for its own members' check_SSIM
 * verdicts: the loop a host with many chunks in flight would otherwise write itself, in one call.  (The fixed order is on
 * purpose: serving whichever batch is ready first lets the batches bunch up and was 3-6 % slower.) */
int vp8drv_batches_encode_frame_device(vp8drv_batch *const *batches, int nbatches, const void *const *const *y, const void *const *const *u,
                                       const void *const *const *v, int *const *was_key);
/* `nframes` frames on every batch, ONE HOST THREAD PER BATCH (started and joined here): the batches share nothing, and with
 * check_SSIM in the loop each one's next frame waits for the verdict on its previous one -- a thread of its own keeps one
 * batch's wait from holding up the others' streams (same box, 48 chunks in 8 batches: one thread serving the batches in turn
 * 55-59 M MB/s, a thread per batch 60.3-60.4, check_SSIM off 60.7-60.9).  Frame t of member i of batch k is
 * frames[(start[k][i] + t) % nd]: `frames` = nd device-resident frames as {y, u, v} pointer triples, shared by all chunks (a
 * transcoder's ring of decoded frames; the bench's synthetic sequence).  The threads start 200 us apart: batches that start together
 * from an idle device stay in lockstep, all their loop filters running at once with nothing wide beside them (5-8 % slower).
 * keys_out[k][i] (may be NULL) counts member i's key frames.  bytes_out (may be NULL): with it every frame is also delivered as
 * bytes -- vp8drv_batch_get_frame_begin for the batch, vp8drv_get_frame_end per member into a buffer of the thread -- and
 * bytes_out[k][i] receives the sum of member i's frame sizes: the loop of a transcoder that writes the frames away.
 * check_out (may be NULL; needs bytes_out): check_out[k][i] is folded with a checksum of every frame of member i as it is
 * delivered, in order -- vp8drv_frame_check(previous value, frame, size); start it at 0 -- so that a caller can hold the bytes of
 * a whole run against a second coding of the same frames without keeping them (bench.py's self-check).
 * Every thread ends with its members' last verdicts taken (vp8drv_resolve) and their stream synchronised: a bounded device-side wait that
 * expired anywhere in the run -- the last frame's loop filter included -- is THIS call's VP8HIP_ERR_TIMEOUT.
 * Returns the first error of any batch, or VP8HIP_OK. */
int vp8drv_batches_encode_frames_device(vp8drv_batch *const *batches, int nbatches, int nframes, const void *const (*frames)[3], int nd,
                                        const int *const *start, int *const *keys_out, uint64_t *const *bytes_out, uint64_t *const *check_out);
/* The same with the nd frames in HOST memory ({y, u, v} tight planes of the source size; page-locked -- vp8hip_host_alloc -- for the copies
 * to overlap the device's work): every frame crosses the host-device link on its way in (vp8hip_batch_upload_current), and with bytes_out
 * on its way out as well -- the whole-job rate WITH the link in it, the reference's own hand-over (vp8enc.cpp:386-388, 476-481). */
int vp8drv_batches_encode_frames_host(vp8drv_batch *const *batches, int nbatches, int nframes, const void *const (*frames)[3], int nd,
                                      const int *const *start, int *const *keys_out, uint64_t *const *bytes_out, uint64_t *const *check_out);
/* ONE video, `nframes` frames, frame after frame with the frames out -- the loop of scripts/native/y4m_to_ivf.cpp for frames that are
 * already in device memory: encode(t), take frame t - 1's bytes, enqueue frame t's entropy stage, take frame t's verdict; frame t
 * is frames[(start + t) % nd].  With overlap_filter the stage of a frame runs on a stream of its own beside its loop filter and the
 * next frame's side work (vp8hip_encode_frame_begin).  Because frame t + 1 is under way before frame t's bytes are taken, a frame denser
 * than the coder's scratch could not be coded again: the call sizes the scratch for the densest frame there can be
 * (vp8hip_reserve_frame_path_dense; a no-op when the caller has done it) -- about 270 MB per context at 1080p and four times that at
 * 4K, allocated behind a stream synchronisation, so a caller that times this call reserves beforehand.  The frames
 * are laid end to end into `out` (capacity bytes), sizes[t] = frame t's size; keys (may be NULL) counts the key frames, frames sent
 * back by check_SSIM included.  out == NULL (sizes is then not used): the same video WITHOUT frames out -- encode after encode, the
 * last verdict taken at the end and the context synchronised (vp8hip_synchronize: a bounded device-side wait that expired inside the last
 * frame's loop filter is reported by THIS call, VP8HIP_ERR_TIMEOUT) -- for callers that code several videos side by side from a thread each and want no interpreter in
 * the loop (bench.py's config3_literal).  A native loop because the host's reaction times are on the path: every microsecond between a
 * frame's verdict and the enqueue of its stage moves the stage further under the next frame's LAST search (one video with frames
 * out, 1080p: 0.383 ms per frame from Python). */
int vp8drv_encode_video_device(vp8drv *d, int nframes, const void *const (*frames)[3], int nd, int start, uint8_t *out, size_t capacity,
                               uint32_t *sizes, int *keys);
/* the fold above: f = h * 0x9E3779B97F4A7C15 + size; for every little-endian 64-bit word w of the frame, in order (the tail
 * zero-padded): f = (rotl(f, 5) ^ w) * 0x100000001B3; h' = f.  Position-dependent: words that trade places change the value. */
uint64_t vp8drv_frame_check(uint64_t h, const uint8_t *frame, size_t size);

/* counters and the flags inter_transform was given for the last inter frame (tests, logs) */
typedef struct {
    int32_t frame_number, inter_frames, key_frames;
    int32_t last_use_golden, last_use_altref, last_prev_is_golden, last_prev_is_altref, last_was_altref;
    int32_t redone_as_key;            /* inter frames recoded as key frames by check_SSIM's verdict (vp8enc.cpp:443-453) */
    int32_t last_replaced;            /* frames.replaced, frames.new_SSIM and min1 of the last check_SSIM */
    float last_new_ssim, last_min_ssim;
    int32_t scene_changes;            /* encStat.scene_changes_by_color: key frames forced by scene_detect (vp8enc.cpp:411) */
    int32_t refs_searched;            /* references searched by all inter frames so far (1 + use_golden + use_altref each) */
} vp8drv_stats;
void vp8drv_get_stats(const vp8drv *d, vp8drv_stats *s);
/* cfg.quality_stats = 1: the record of the frame just made final (its check_SSIM verdict is taken first, as vp8drv_get_frame does:
 * a frame coded again as a key frame has the key frame's record, is_key 1), and the summary over every frame made final so far.
 * Neither waits for more than the last measurement.  VP8HIP_ERR_STATE when stats are off or no frame was coded yet. */
typedef vp8hip_quality vp8drv_quality;
typedef vp8hip_quality_totals vp8drv_quality_summary;
int vp8drv_get_frame_quality(vp8drv *d, vp8drv_quality *q);
int vp8drv_get_quality_summary(vp8drv *d, vp8drv_quality_summary *s);
/* Temporal noise reduction of the source frames (vp8hip_set_denoise; the rule: include/vp8hip_host.h), an entry point and not a field
 * because vp8drv_config keeps its size.  Call it after vp8drv_create; level 0-3, 0 (default) = off.  It takes the open check_SSIM
 * verdict first.  VP8HIP_ERR_ARG: a bad level, or device_params = 0 (the host parameter mirror would scan the caller's luma, which
 * is not the frame that is coded); VP8HIP_ERR_STATE: the driver is a member of a live batch (members must agree: set the level before
 * vp8drv_batch_create, which refuses members that disagree).
 * The history restarts when the GOP schedule makes the incoming frame a key frame (gop.current_is_key at the moment the frame is taken
 * in, through vp8drv_encode_frame_device / _host, vp8drv_stage_frame_host, a prefetched frame, the batched calls), so a closed GOP coded
 * as a chunk of its own sees the frames the serial program sees.  force_key, scene cuts and frames sent back by check_SSIM do not restart
 * it -- the block decision rejects a cut by itself -- and a frame coded again as a key frame is not denoised twice. */
int vp8drv_set_denoise(vp8drv *d, int level);
/* the record of the last frame taken in (vp8hip_denoise_result); VP8HIP_ERR_STATE when denoising is off or no frame was taken in */
int vp8drv_get_denoise_stats(vp8drv *d, vp8hip_denoise_stats *s);
/* Interlaced source frames made progressive (vp8hip_set_deinterlace; the rule: include/vp8hip_host.h), an entry point and not a field
 * for the reason vp8drv_set_denoise is one, and under its rules: call it after vp8drv_create; mode 0 (default, off), 1 (field) or 2
 * (adaptive), keep 0 (top field) or 1 (bottom field).  It takes the open check_SSIM verdict first.  VP8HIP_ERR_ARG: another mode or
 * keep, an incoming height below 4, or cfg.device_params = 0 (the host parameter mirror would scan the caller's luma, which is not the
 * frame that is coded); VP8HIP_ERR_STATE: the driver is a member of a live batch (members must agree on mode and parity: set them
 * before vp8drv_batch_create, which refuses members that differ).  Every way a frame is taken in passes through it:
 * vp8drv_encode_frame_device / _host, vp8drv_prefetch_frame_host, vp8drv_stage_frame_host and the batched calls.
 * The order is convert, then deinterlace, then pack or scale, then denoise, then the analysis source side; the chroma scan, the
 * analysis and the quality statistics see the deinterlaced frame, the one that was coded.
 * The history of mode 2 restarts where the denoiser's does: when the GOP schedule makes the incoming frame a key frame, so a closed GOP
 * coded as a chunk of its own sees what the serial program sees.  force_key, scene cuts and frames sent back by check_SSIM do not
 * restart it, and a frame coded again as a key frame is not deinterlaced twice.  KNOWN COST: a GOP's first frame is therefore
 * field-interpolated in mode 2.  Handing the frame BEFORE a chunk's first frame in as a primer would lift that, and it would be exact
 * because the history is unprocessed input; it is not done here. */
int vp8drv_set_deinterlace(vp8drv *d, int mode, int keep);
/* the record of the last frame taken in (vp8hip_deinterlace_result); VP8HIP_ERR_STATE when deinterlacing is off or no frame was taken in */
int vp8drv_get_deinterlace_stats(vp8drv *d, vp8hip_deinterlace_stats *s);
/* The format of the source frames (vp8hip_set_source_format; the formats and the rule: include/vp8hip_host.h), an entry point and not a
 * field of vp8drv_config for the reason vp8drv_set_denoise is one.  Call it after vp8drv_create and before the first frame, or
 * between frames.  From then on the three pointers of vp8drv_encode_frame_device / _host, vp8drv_prefetch_frame_host,
 * vp8drv_stage_frame_host and the batched calls are that format's planes (the two-plane formats do not read the third: pass the
 * second again).  0 = 8-bit I420, the default.  VP8HIP_ERR_ARG: an unknown format, or cfg.device_params = 0 (the host parameter
 * mirror reads the caller's luma plane as 8-bit samples).  VP8HIP_ERR_STATE: the driver is a member of a live batch (the members
 * must agree: set the format before vp8drv_batch_create, which refuses members that differ). */
int vp8drv_set_source_format(vp8drv *d, int format);
/* The colour matrix BGRA / RGBA source frames are read with (vp8hip_set_source_colour; enum vp8host_colour_matrix and the tables:
 * include/vp8hip_host.h), 0 = BT.601 limited range, the default.  The rules of vp8drv_set_source_format: between frames, in any order
 * relative to the format; VP8HIP_ERR_ARG: not one of the four matrices, or cfg.device_params = 0; VP8HIP_ERR_STATE: the driver is a
 * member of a live batch (vp8drv_batch_create refuses members that differ). */
int vp8drv_set_source_colour(vp8drv *d, int matrix);
/* The transfer function and peak P010 / I010 source frames carry (vp8hip_set_source_transfer; enum vp8host_transfer and the rule:
 * include/vp8hip_host.h): PQ or HLG frames are tone-mapped to SDR on the device, 0 = off, the default.  The rules of
 * vp8drv_set_source_format: an entry point, between frames, in any order relative to the format (whichever of the two completes a
 * combination the rule does not cover is refused); VP8HIP_ERR_ARG: an unknown transfer, a peak outside 400 .. 10000, a format in
 * force other than I420, P010 or I010, or cfg.device_params = 0; VP8HIP_ERR_STATE: the driver is a member of a live batch
 * (vp8drv_batch_create refuses members that differ in transfer or peak). */
int vp8drv_set_source_transfer(vp8drv *d, int transfer, int peak);
/* Layers burnt into the source frames (vp8hip_set_overlay_host / _device, vp8hip_set_overlay_placement, vp8hip_clear_overlay, which say
 * what a layer is; the rule: include/vp8hip_host.h).  Entry points, not fields of vp8drv_config, for the reason vp8drv_set_denoise is
 * one.  A layer is in force from the next frame the driver takes in, whichever call hands it over (vp8drv_stage_frame_host and the
 * batch scan included); the scene scan and the coder see the same composed frame, so scene_detect keeps working.  Unlike the other
 * intake setters they are allowed on a member of a live batch between frames, as vp8drv_set_segment_map is: a subtitle may change from
 * frame to frame.  They take the open check_SSIM verdict first.  VP8HIP_ERR_ARG: what the context's entry point refuses, or
 * cfg.device_params = 0 (the host mirror scans the caller's luma, which is not the frame coded).  While any layer is set
 * vp8drv_encode_arf_device / _host refuse with VP8HIP_ERR_ARG: the window frames bypass the intake. */
int vp8drv_set_overlay_host(vp8drv *d, int slot, int format, int matrix, const uint8_t *pixels, int lw, int lh, int pitch, int x, int y, int opacity);
int vp8drv_set_overlay_device(vp8drv *d, int slot, int format, int matrix, const void *pixels, int lw, int lh, int pitch, int x, int y, int opacity);
int vp8drv_set_overlay_placement(vp8drv *d, int slot, int x, int y, int opacity);
int vp8drv_clear_overlay(vp8drv *d, int slot);
/* Frames composed of scaled video tiles (vp8hip_set_canvas, vp8hip_compose_current_device / _host, which say what a canvas is; the
 * rule: include/vp8hip_host.h, "CANVAS").  Entry points, not fields of vp8drv_config, for the reason vp8drv_set_denoise is one; call
 * vp8drv_set_canvas after vp8drv_create and before the first frame, or between frames (it takes the open check_SSIM verdict first and
 * waits for the context's streams; n = 0 ends the canvas).  With a canvas the driver's frames come in through
 * vp8drv_encode_frame_tiles_device / _host -- src[k]: tile k's planes of this frame, y == NULL for a tile that is absent -- which
 * return what vp8drv_encode_frame_device / _host return; scene detection, check_SSIM, the GOP schedule, key frames, overlays, the
 * denoiser and the quality statistics work as for any frame, on the composed frame.  The host form returns when the host's planes are
 * the host's again.  VP8HIP_ERR_ARG: what the context's entry point refuses, or cfg.device_params = 0.  VP8HIP_ERR_STATE: a member of a
 * live batch (vp8drv_batch_create in turn refuses a driver with a canvas), the tile calls without a canvas, and with a canvas
 * vp8drv_encode_frame_device / _host, vp8drv_prefetch_frame_host, vp8drv_stage_frame_host and vp8drv_set_arf; nothing has changed then. */
int vp8drv_set_canvas(vp8drv *d, const vp8hip_tile *tiles, int n, int bg_y, int bg_u, int bg_v);
int vp8drv_encode_frame_tiles_device(vp8drv *d, const vp8hip_tile_planes *src /* [n] */, int force_key);
int vp8drv_encode_frame_tiles_host(vp8drv *d, const vp8hip_tile_planes *src /* [n] */, int force_key);
/* Source frames that are the window of a pitched surface, and source frames stored sideways or upside down
 * (vp8hip_set_source_window, vp8hip_set_source_orientation; the rules: include/vp8hip_host.h).  Entry points, not fields of
 * vp8drv_config, for the reason vp8drv_set_denoise is one; call them after vp8drv_create and before the first frame, or between
 * frames, in any order relative to each other and to the other setters.  With a window the three pointers of
 * vp8drv_encode_frame_device / _host, vp8drv_prefetch_frame_host, vp8drv_stage_frame_host and the batched calls are the plane bases
 * of a surface (pitch = bytes between the rows of each plane, NULL = off; (x, y) = the window's top-left luma sample, both even); with
 * an odd number of turns the planes handed in are cfg's incoming height wide and its incoming width high, and every size of
 * vp8drv_config keeps describing the upright frame.  VP8HIP_ERR_ARG: what the library refuses, or cfg.device_params = 0 (the host
 * parameter mirror reads the caller's luma plane as the tight upright frame).  VP8HIP_ERR_STATE: the driver is a member of a live
 * batch (the members must agree: set them before vp8drv_batch_create, which refuses members that differ). */
int vp8drv_set_source_window(vp8drv *d, const int32_t *pitch /* [3], NULL = off */, int x, int y);
int vp8drv_set_source_orientation(vp8drv *d, int turns, int mirror);
/* ---- what a rate controller needs: a record to measure with and a quantizer to set -------------------------------------------
 * Frame analysis statistics (vp8hip_set_analysis; the rules: include/vp8hip_host.h), entry points and not a field for the reason
 * vp8drv_set_denoise is one.  on = 0 (default) or 1; it takes the open check_SSIM verdict first.  VP8HIP_ERR_ARG: another value, or
 * cfg.device_params = 0; VP8HIP_ERR_STATE: the driver is a member of a live batch (set it before vp8drv_batch_create, which refuses
 * members that differ).  The history restarts where the denoiser's does: when the GOP schedule makes the incoming frame a key frame, so
 * a closed GOP coded as a chunk of its own gives the records the serial program gives (have_prev = 0 on its first frame). */
int vp8drv_set_analysis(vp8drv *d, int on);
typedef vp8hip_analysis vp8drv_analysis;
/* The record of the frame just made final: its verdict first, as vp8drv_get_frame_quality (a frame coded again as a key frame has the
 * key frame's coding side; its source side was measured once, when it was taken in).  VP8HIP_ERR_STATE: analysis off or no frame coded. */
int vp8drv_get_frame_analysis(vp8drv *d, vp8drv_analysis *a);
/* A quantiser per macroblock (vp8hip_set_segment_mode; the rule: include/vp8hip_host.h), entry points and not a field for the reason
 * vp8drv_set_denoise is one.  mode 0 (default) off, 1 the caller's map, 2 variance-adaptive at strength 1..3.  Inter frames are coded in
 * the mode from the next frame taken in on (a frame already handed over with vp8drv_stage_frame_host has no variance map: segment 3);
 * key frames, scheduled or not, stay as they are.  GOP chunks give the serial program's bytes: mode 2's map depends on the current
 * frame alone.  With vp8drv_set_analysis, segment_mbs of vp8drv_get_frame_analysis is the map's histogram on inter frames.  It takes
 * the open check_SSIM verdict first.  VP8HIP_ERR_ARG: a bad mode or strength; VP8HIP_ERR_STATE: cfg.ssim_target >= 0, or the driver is
 * a member of a live batch (members must agree on mode and strength: set them before vp8drv_batch_create, which refuses a mix). */
int vp8drv_set_segment_mode(vp8drv *d, int mode, int strength);
/* The map of mode 1: MBs bytes in host memory, raster order, each 0..3 (a larger value: VP8HIP_ERR_ARG), copied before the call returns
 * and in force until replaced; a member of a batch may get a new one between frames.  Without one mode 1 codes segment 3 everywhere. */
int vp8drv_set_segment_map(vp8drv *d, const uint8_t *host_map);
/* cfg.qi_min / qi_max from the next frame coded on: both ladders are made again with vp8host_quantizer_ladders and the driver's qi_min
 * becomes the smaller of the two, exactly as in vp8drv_create.  It takes the open check_SSIM verdict first, so a frame sent back is coded
 * again with the quantizers it was coded with.  References, GOP position and every other state stay: behind a key frame of the GOP
 * schedule the frames are those of a driver created with the new pair.  VP8HIP_ERR_ARG: a value outside 0..127, the range of a VP8
 * quantizer index (vp8drv_create does not look at its pair; the device clamps an index to this range); VP8HIP_ERR_STATE: the driver is
 * a member of a live batch (members share the pair: set it before vp8drv_batch_create). */
int vp8drv_set_quantizer(vp8drv *d, int qi_min, int qi_max);
/* the pair in force, as given (not swapped) */
int vp8drv_get_quantizer(const vp8drv *d, int32_t *qi_min, int32_t *qi_max);
/* ---- hidden alternate reference frames (vp8hip_arf_filter_device, include/vp8hip.h; the rule: include/vp8hip_host.h) -----------------
 * libvpx's --auto-alt-ref=1 --arnr-maxframes --arnr-strength with the placement left to the caller: the caller owns the lookahead and
 * hands the window in whenever it wants a hidden frame; the driver keeps no queue.  Entry points and not fields of vp8drv_config for
 * the reason vp8drv_set_denoise is one.
 * vp8drv_set_arf: 0 (default) = off, 1 .. 7 = on at strength 0 .. 6.  Takes the open check_SSIM verdict first.  Turning it off
 * frees the filter's staging buffers and nothing else: the current frame and the references stay.
 * vp8drv_encode_arf_device: frames[k][0..2] = the planes of frame k of the window, tight 8-bit I420 of the incoming size in device
 * memory, 1 <= n <= 7, centre in 0 .. n - 1.  It takes the open check_SSIM verdict first, filters the window on the device and codes
 * the filtered frame as an INTER frame that is not shown: on the altrefqi ladder, with the references the next shown frame would be
 * allowed (cfg.scene_detect keeps working: the hidden frame steps out of the intake when it is coded, so the next frame's chroma
 * comparison is with the last SHOWN frame; GOLDEN unless the last shown frame was a key frame; ALTREF unless that frame was a key frame or a scheduled alt-ref, and
 * only where it differs from GOLDEN; both subject to cfg.ref_mask), WITHOUT check_SSIM (no fallback, no filter update, no redo as key
 * frame), and with the reconstruction into ALTREF while LAST stays.  frame_number, the GOP counters, the scene history, vp8drv_stats
 * and the quality summary are left alone: they count shown frames.  Returns 0; vp8drv_get_frame / _begin / _end then deliver its bytes
 * like any frame's (show_frame = 0, refresh_alternate = 1, refresh_last = 0 in them).  A container gives it a record of its own with
 * the timestamp of the next shown frame.
 * AFTERWARDS shown inter frames search ALTREF, subject to cfg.ref_mask, until a key frame or a scheduled shown alt-ref replaces it;
 * use_golden keeps following the real history of shown frames.  A caller that wants hidden alt-refs only sets cfg.altref_range above
 * cfg.gop_size.  Hidden frames of a GOP depend on that GOP's frames only when the caller clips its windows to the GOP.
 * vp8drv_encode_arf_host: the simple form -- uploads the window, blocks, and does the same.
 * THE VERDICT IT TAKES: when the open verdict sends the last shown frame back, that frame is coded again as a key frame inside this
 * call, before the hidden frame (which then follows a key frame), and the call still returns 0: its return value speaks of the hidden
 * frame only.  A caller that has to know -- one that has not taken that frame's bytes yet, or that clips its windows to the GOP --
 * calls vp8drv_resolve or vp8drv_get_frame for the shown frame first, as the tools do; vp8drv_stats.redone_as_key counts it either way.
 * VP8HIP_ERR_STATE: hidden frames off, no frame coded yet (no reference), the driver is a member of a live batch (vp8drv_batch_create
 * in turn refuses a driver with hidden frames on: they are not batched), a frame handed over early with vp8drv_stage_frame_host is
 * waiting, or the context shares a frame's searches with other devices.  VP8HIP_ERR_ARG: a bad n, centre or strength, a null plane,
 * cfg.device_params = 0, cfg.overlap_filter (the next frame's ALTREF search would start beside the filter that writes ALTREF),
 * a source format other than 0, a source window,
 * deinterlacing, denoising or analysis switched on (the last three keep a history that a hidden frame would disturb).
 * vp8drv_get_arf_stats: hidden frames coded so far, and of the last one its window, its reference flags and the (tile, frame) pairs by
 * block weight 0, 1, 2; blocks.  VP8HIP_ERR_STATE: none coded. */
typedef struct {
    int32_t hidden_frames;
    int32_t last_frames, last_use_golden, last_use_altref;
    int32_t last_weight[3];
} vp8drv_arf_stats;
int vp8drv_set_arf(vp8drv *d, int strength_plus_one);
int vp8drv_encode_arf_device(vp8drv *d, const void *const (*frames)[3], int n, int centre);
int vp8drv_encode_arf_host(vp8drv *d, const uint8_t *const (*frames)[3], int n, int centre);
int vp8drv_get_arf_stats(vp8drv *d, vp8drv_arf_stats *s);
/* ---- temporal layers (the rule: vp8host_temporal_step, include/vp8hip_host.h; the ending: vp8hip_loop_filter_refresh, include/vp8hip.h) ----
 * A stream of two or three temporal layers, the patterns WebRTC runs VP8 with: a forwarding unit may drop every frame above a layer
 * and what is left still decodes.  Entry points and not fields of vp8drv_config for the reason vp8drv_set_denoise is one.
 * vp8drv_set_temporal_layers: layers 1 (default, off) to 3; flags: VP8DRV_TL_KEEP_RECON or 0.  It takes the open check_SSIM verdict first.
 * The layer count is IN FORCE FROM THE NEXT KEY FRAME ON, whoever asks for that key frame (the GOP schedule, force_key, a scene cut, a
 * frame sent back by check_SSIM) -- before the first frame that is the first frame; until then the frames are coded as they were, so
 * turning layers on or off in the middle of a GOP never leaves a receiver with a half pattern.  The flags are in force at once.
 * With layers in force an inter frame takes its references and its ending from the rule in the place of the GOP state's flags: p counts
 * the shown frames since the last key frame as finally coded, ALTREF is never searched, every frame is quantised on the lastqi ladder,
 * vp8drv_stats.refs_searched advances by 1 + use_golden.  The rotation a key frame owes is applied by the next frame's transform as ever.
 * A closed GOP coded as a chunk of its own (a fresh driver, force_key) gives the bytes the serial program gives.  Everything on the input
 * side -- canvas, overlays, formats, scaler, denoiser, deinterlacer, the per-macroblock quantiser, analysis, scene detection --
 * composes unchanged: it follows the frames taken in, not the references.
 * A frame that refreshes nothing is FILTERED only if something reads the filter's output or rides in its launch: cfg.check_ssim,
 * cfg.quality_stats, vp8drv_set_analysis or VP8DRV_TL_KEEP_RECON (for a caller that reads the reconstruction back).  Otherwise no
 * filter, no edge and no pyramid launch is made for it; its bytes are the same either way.
 * VP8HIP_ERR_ARG, for layers > 1: cfg.device_params = 0, cfg.overlap_filter, cfg.altref_range <= cfg.gop_size (scheduled alt-refs must
 * be off, by the convention of vp8drv_encode_arf_device); and layers or flags out of range.  VP8HIP_ERR_STATE, for layers > 1: a member
 * of a live batch (vp8drv_batch_create in turn refuses such a driver: layers are not batched), vp8drv_set_arf on (which in turn refuses
 * while layers are on or asked for), a context that shares a frame's searches with other devices -- and if the context joins such a
 * split later, the calls that take a frame in.  Nothing has changed after a refusal.
 * vp8drv_get_frame_layer: the frame just made final, valid after vp8drv_resolve or vp8drv_get_frame (it takes the open verdict itself:
 * a frame coded again as a key frame has the key frame's record); for any driver, layers or not.  VP8HIP_ERR_STATE: no frame coded yet,
 * or the frame just coded is a hidden one.  What an RTP VP8 payload descriptor carries: INTEGRATION.md, section 6.6. */
#define VP8DRV_TL_KEEP_RECON 1
typedef struct {
    int32_t temporal_id;      /* 0 = the base layer; key frames are 0 */
    int32_t tl0_pic_idx;      /* a running index of the temporal_id 0 frames, key frames included, modulo 256: the first frame's is 0, a
                                 frame of a higher layer carries the index of the base frame before it */
    int32_t layer_sync;       /* 1: the frame reads temporal layer 0 only (a receiver may start taking this layer here) */
    int32_t refresh;          /* VP8HOST_REFRESH_LAST, _GOLDEN, _NONE; _ALL for a key frame */
    int32_t use_golden;       /* GOLDEN was searched beside LAST */
    int32_t filtered;         /* the loop filter ran on its reconstruction */
} vp8drv_layer_info;
int vp8drv_set_temporal_layers(vp8drv *d, int layers, int flags);
int vp8drv_get_frame_layer(vp8drv *d, vp8drv_layer_info *info);
/* ---- cyclic intra refresh (the rule: vp8host_intra_refresh_forced, include/vp8hip_host.h; the launch: vp8hip_intra_refresh, include/vp8hip.h) ----
 * A few macroblocks of every inter frame coded as intra, in a pattern that covers the picture every `period` frames: a receiver that
 * lost a frame can heal within a period without a key frame (libvpx's error-resilient cyclic refresh; what to do with a PLI:
 * INTEGRATION.md, section 6.7).  Entry points and not fields of vp8drv_config for the reason vp8drv_set_denoise is one.
 * vp8drv_set_intra_refresh: period 0 (default, off) or 4 .. 1024, IN FORCE AT THE NEXT FRAME, no key frame needed: the phase q -- the
 * inter frames since the last key frame as finally coded that refreshed LAST -- advances whether or not refresh is on, so a closed GOP
 * coded as a chunk of its own (a fresh driver, force_key, the same period) gives the bytes the serial program gives.  It takes the
 * open check_SSIM verdict first.  With a period in force every shown inter frame that refreshes LAST and has a forced macroblock at
 * its phase gets vp8hip_intra_refresh behind its transform, and its header carries the intra information, from either first-partition
 * coder.  Frames of a temporal layer that refresh GOLDEN only or nothing, hidden frames (vp8drv_encode_arf_*) and key frames force
 * nothing and do not advance q; any key frame restarts it.  Temporal layers, segment modes 1 and 2, vp8drv_set_quantizer, quality
 * statistics, analysis (mbs_intra counts the forced macroblocks) and everything on the input side compose unchanged.  With period 0:
 * no launch, no allocation, no byte changes.
 * VP8HIP_ERR_ARG: a period outside 0 and 4 .. 1024; for a period other than 0: cfg.device_params = 0 or cfg.ssim_target > -1.
 * VP8HIP_ERR_STATE, for a period other than 0: a member of a live batch (vp8drv_batch_create in turn refuses a driver with a period:
 * refresh is not batched), a context that shares a frame's searches with other devices -- and if the context joins such a split
 * later, the calls that take a frame in.  Nothing has changed after a refusal.
 * vp8drv_get_intra_refresh: for any driver; forced counts are those of the frame just coded as first coded (a frame sent back as a
 * key frame has forced 0 once its verdict is taken: the call takes it). */
typedef struct {
    int32_t period;           /* in force (0 = off) */
    int32_t last_q;           /* the phase of the frame just coded (0 for a key frame; of a frame that does not refresh LAST: the phase it would have had) */
    int32_t last_forced;      /* forced macroblocks of the frame just coded */
    int64_t total_forced;     /* ... of all frames so far */
} vp8drv_intra_refresh_info;
int vp8drv_set_intra_refresh(vp8drv *d, int period);
int vp8drv_get_intra_refresh(vp8drv *d, vp8drv_intra_refresh_info *info);

#ifdef __cplusplus
}
#endif
#endif
