/*
 * vp8hip.h -- C ABI of the MI355X (gfx950) inter-frame path of vp8oclenc.
 *
 * Drop-in boundary: each entry point replaces a group of OpenCL calls that the reference host
 * driver makes (citations are file:line under the reference's src/).  The library owns every
 * device allocation; the host owns every host buffer; no host pointer is kept after a call
 * returns.  All calls are made from one host thread per context.  Return value: 0 on success,
 * negative vp8hip_status on failure (the reference stores cl_int errors in device.state_gpu,
 * inter_part.h:380).  There is no CPU fallback: without a usable HIP device vp8hip_create fails.
 *
 * Plane convention at the boundary: tightly packed 8-bit planes of the padded ("wrk") size,
 * width and height multiples of 16 (init.h:381-389), chroma planes (W/2)x(H/2) -- exactly
 * hostFrameBuffers.current_Y/U/V and reconstructed_Y/U/V (vp8enc.h:364-372).
 */
#ifndef VP8HIP_H
#define VP8HIP_H

#include <stddef.h>
#include <stdint.h>

#include "vp8hip_host.h"      /* vp8hip_tile, vp8hip_tile_planes, VP8HIP_MAX_TILES (vp8hip_set_canvas) */

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vp8hip_ctx vp8hip_ctx;

typedef enum {
    VP8HIP_OK = 0,
    VP8HIP_ERR_ARG = -1,       /* bad size / NULL pointer */
    VP8HIP_ERR_NO_DEVICE = -2, /* no HIP device, or device_ordinal out of range */
    VP8HIP_ERR_HIP = -3,       /* a HIP runtime call failed (vp8hip_last_hip_error) */
    VP8HIP_ERR_STATE = -4,     /* call out of order (e.g. loop filter before any transform) */
    VP8HIP_ERR_ARCH = -5,      /* device is not gfx950: the kernels are built for MI355X only */
    VP8HIP_ERR_TIMEOUT = -6,   /* a bounded device-side wait of the loop filter expired: the frame is invalid
                                  (reported by vp8hip_synchronize / vp8hip_download_*; the context stays usable) */
    VP8HIP_ERR_OVERFLOW = -7,  /* vp8hip_encode_coefficients: output or scratch too small for this frame */
    VP8HIP_ERR_FORMAT = -8     /* the frame cannot be written as VP8: its first partition has 512 KB or more and the frame tag
                                  has 19 bits for that size (RFC 6386 section 9.1) -- key frames of about 7000x4000 and up.  The
                                  reference writes the low 19 bits (entropy_host.cpp:1237-1241) and emits a frame no decoder
                                  can read; here the call fails */
} vp8hip_status;

/* segment_data[4], vp8enc.h:80-92: 11 ints per segment */
#define VP8HIP_SD_INTS 44

/* Host pointers filled by vp8hip_download_results; any member may be NULL (skipped).
 * Layouts: vp8enc.h:105-120, 378-382. */
typedef struct {
    int32_t *MB_parts;           /* [MBs] 0=16x16 1=8x8                         inter_part.h:263 */
    int32_t *MB_reference_frame; /* [MBs] 0 LAST 1 GOLDEN 2 ALTREF              inter_part.h:264 */
    int16_t *MB_vectors;         /* [MBs][4]{x,y} qpel, TL TR BL BR             inter_part.h:265 */
    int16_t *MB_coeffs;          /* [MBs][25][16] zig-zag order                 vp8enc.cpp:422   */
    int32_t *MB_segment_id;      /* [MBs]                                        vp8enc.cpp:423   */
    float *MB_SSIM;              /* [MBs]                                        vp8enc.cpp:424   */
    uint8_t *recon_Y;            /* reconstruction BEFORE the loop filter        vp8enc.cpp:431   */
    uint8_t *recon_U;            /*                                              vp8enc.cpp:432   */
    uint8_t *recon_V;            /*                                              vp8enc.cpp:433   */
} vp8hip_results;

/* init_all() GPU half (init.h:133-312, 430-582, 595-1166) / finalize() (vp8enc.cpp:501-708).
 * width,height: padded luma size.  ssim_target: video.SSIM_target (init.h:1512,1576). */
int vp8hip_create(vp8hip_ctx **out, int width, int height, float ssim_target, int device_ordinal);
void vp8hip_destroy(vp8hip_ctx *ctx);

/* clEnqueueWriteBuffer(current_frame_Y/U/V), vp8enc.cpp:386-388 */
int vp8hip_upload_current(vp8hip_ctx *ctx, const uint8_t *y, const uint8_t *u, const uint8_t *v);
/* The NEXT frame's planes started on their way early, while the current frame is coded: tight planes of the source size (one copy when
 * U follows Y and V follows U in memory), asynchronous when they are page-locked (vp8hip_host_alloc), into a staging buffer of the
 * context's.  The vp8hip_upload_current that names the same three pointers then copies nothing: it packs from the staging buffer, behind
 * the copy.  The planes stay unchanged until that vp8hip_upload_current has returned.  Touches nothing of the frame under way. */
int vp8hip_prefetch_current(vp8hip_ctx *ctx, const uint8_t *y, const uint8_t *u, const uint8_t *v);
/* same, from planes already resident in this device's memory (tight stride); async on the ctx stream */
int vp8hip_set_current_device(vp8hip_ctx *ctx, const void *d_y, const void *d_u, const void *d_v);

/* LAST := these (already loop-filtered) planes: vp8enc.cpp:395-401, intra_part.h:1112-1125.
 * Needed after a key frame and whenever the host changed the reconstruction. */
int vp8hip_upload_last(vp8hip_ctx *ctx, const uint8_t *y, const uint8_t *u, const uint8_t *v);
int vp8hip_set_last_device(vp8hip_ctx *ctx, const void *d_y, const void *d_u, const void *d_v);

/* The two per-frame host scans that produce parameters of this path, on the device copy of the
 * current frame -- at 0.2 ms per 1080p frame a single-threaded 2-Mpixel scan on the host would be the bottleneck.
 * Both block until the values are back.
 * get_loopfilter_strength(), vp8enc.cpp:96-127: reductor and sharpness of the current luma plane. */
int vp8hip_loopfilter_strength(vp8hip_ctx *ctx, int32_t *reductor, int32_t *sharpness);
/* scene_change()'s inputs, vp8enc.cpp:265-282: mean absolute difference of the U and V planes between this current
 * frame and the previous current frame (the context keeps both; 0,0 while there is only one).  The decision
 * logic with its hold-over stays on the host: vp8host_scene_change(), include/vp8hip_host.h. */
int vp8hip_chroma_change(vp8hip_ctx *ctx, int32_t *Udiff, int32_t *Vdiff);
/* ... in two halves: _async enqueues the scan behind the current frame's pack and returns; _result waits for the two sums only (they
 * arrive in page-locked memory; not for the stream) and returns what vp8hip_chroma_change returns.  A second _async before a _result
 * replaces the first; _result without a pending _async: VP8HIP_ERR_STATE.  For a host that hands the next frame over early (while the
 * previous frame's loop filter runs) and wants scene_change()'s verdict without a round trip in its critical path. */
int vp8hip_chroma_change_async(vp8hip_ctx *ctx);
int vp8hip_chroma_change_result(vp8hip_ctx *ctx, int32_t *Udiff, int32_t *Vdiff);

/* get_loopfilter_strength() + prepare_segments_data() (vp8enc.cpp:96-127, 129-221) evaluated on the device for the
 * current frame: the segment data of the following vp8hip_inter_transform / vp8hip_loop_filter are produced without
 * any host round trip (asynchronous on the context's stream) -- what a frame loop at several thousand frames per
 * second needs.  refqi = the lastqi or altrefqi ladder (vp8enc.cpp:149-151).  vp8hip_get_segments reads back the
 * segment data in force (the frame header needs them) and the strength pair; it blocks. */
int vp8hip_auto_segments(vp8hip_ctx *ctx, int is_key_frame, const int32_t refqi[4], int qi_min);
int vp8hip_get_segments(vp8hip_ctx *ctx, int32_t sd[VP8HIP_SD_INTS], int32_t *reductor, int32_t *sharpness);

/* clEnqueueWriteBuffer(segments_data_gpu), vp8enc.cpp:224 */
int vp8hip_set_segments(vp8hip_ctx *ctx, const int32_t sd[VP8HIP_SD_INTS]);

/* prepare_GPU_buffers() + inter_transform(), inter_part.h:1-94, 96-384.  Flags as computed at
 * inter_part.h:103-104 and vp8enc.cpp:364-366.  Asynchronous; results via vp8hip_download_results. */
int vp8hip_inter_transform(vp8hip_ctx *ctx, int prev_is_golden, int prev_is_altref, int use_golden,
                           int use_altref);

/* the clEnqueueReadBuffer group at inter_part.h:263-265 and vp8enc.cpp:422-433, followed by the
 * clFinish at vp8enc.cpp:439-440: returns when the copies are complete */
int vp8hip_download_results(vp8hip_ctx *ctx, const vp8hip_results *r);

/* Host-side changes made between the transform and the loop filter (per-MB intra fallback,
 * intra_part.h:1063-1084; key frames): any pointer may be NULL = keep the device copy.
 * vp8enc.cpp:460-470, loop_filter.h:7, 63-65 */
int vp8hip_upload_mb_data(vp8hip_ctx *ctx, const int16_t *MB_coeffs, const int32_t *MB_parts,
                          const int32_t *MB_segment_id);
int vp8hip_upload_recon(vp8hip_ctx *ctx, const uint8_t *y, const uint8_t *u, const uint8_t *v);

/* ---- the host intra path on the device -----------------------------------------------------------
 * The reference codes key frames and the intra fallback of inter frames on one CPU thread, which forces the
 * reconstruction and all coefficients across the bus twice per frame (vp8enc.cpp:422-433, 460-470;
 * loop_filter.h:7,63-65).  Both run here as a row wavefront on the current frame already in HBM.
 *
 * intra_transform()'s loop, intra_part.h:1089-1109 (predict_and_transform_mb, :517-741): the current frame as a key
 * frame -- B_PRED luma with the mode of every 4x4 block picked by pick_luma_predictor (:252-515), TM_PRED chroma,
 * quantizers of segment 0 of the segment data in force (vp8hip_set_segments / vp8hip_auto_segments with
 * is_key_frame).  Leaves coefficients (blocks 0..23, zigzag), MB_parts = are4x4, MB_segment_id = 0 and the
 * unfiltered reconstruction where vp8hip_inter_transform leaves them; continue with vp8hip_prepare_filter_mask and
 * vp8hip_loop_filter, after which the next vp8hip_inter_transform takes prev_is_golden = prev_is_altref = 1
 * (intra_part.h:1091-1098).  Asynchronous. */
int vp8hip_intra_transform(vp8hip_ctx *ctx);
/* check_SSIM(), vp8enc.cpp:231-263, on the results of the preceding vp8hip_inter_transform: every macroblock whose
 * SSIM is below the context's ssim_target is tried as intra in segments AQ, HQ, UQ (test_inter_on_intra,
 * intra_part.h:855-1087) and replaced -- coefficients, MB_parts, MB_segment_id, MB_SSIM, reconstruction -- when that
 * scores higher.  Returns frames.replaced, frames.new_SSIM and the minimum SSIM (`min1`; the reference updates
 * the filter parameters when it exceeds 0.95, :260).  Blocks until the three values are back. */
int vp8hip_check_ssim(vp8hip_ctx *ctx, int32_t *replaced, float *new_ssim, float *min_ssim);
/* The same without the host in the middle -- what a frame loop at thousands of frames per second needs.  The call enqueues
 * check_SSIM's fallback (a launch whose workgroups leave at once unless the transform has flagged a macroblock below the
 * target -- not made at all when the context's target is -1 or lower, which no macroblock's SSIM can lie below; it also renews
 * the filter mask and non-zero count of what it replaces: no vp8hip_prepare_filter_mask needed) and
 * arms the NEXT vp8hip_loop_filter / vp8hip_batch_loop_filter call, whose launch then carries the rest: every band of the
 * filter takes the frame's minimum SSIM and, above 0.95, filters with the segment data `prepare_segments_data(1, 7)` gives
 * (:260-261; from the strength pair vp8hip_auto_segments left on the device, so the frame's segment data must come from that
 * call; refqi / qi_min as for it), and one extra workgroup writes those segment data back for the entropy stage, sums the
 * frame's SSIM in the reference's order and hands replaced / new_SSIM / min SSIM to the host through memory the host polls.
 * vp8hip_check_ssim_result collects them when the host next needs them -- the reference's "redo as key frame" decision
 * (:443-453), which the native frame loop takes at the start of the NEXT call (include/vp8hip_driver.h) -- and returns as soon
 * as the verdict workgroup has run, a few microseconds into the filter's launch.  filter_updated: 1 when the segment data were
 * rewritten (video.loop_filter_sharpness is then 7).  VP8HIP_ERR_STATE while no armed loop filter has been launched.
 * vp8hip_check_ssim_ready: 1 if _result would not wait. */
int vp8hip_check_ssim_async(vp8hip_ctx *ctx, const int32_t refqi[4], int qi_min);
int vp8hip_check_ssim_result(vp8hip_ctx *ctx, int32_t *replaced, float *new_ssim, float *min_ssim, int32_t *filter_updated);
int vp8hip_check_ssim_ready(const vp8hip_ctx *ctx);
/* e_data[].mode[16] of the last vp8hip_intra_transform / vp8hip_check_ssim (the sub-block modes the header coder
 * writes; after check_ssim: of the LAST attempt on a macroblock, as in the reference -- see
 * vp8hip_conformant_stream -- and 0 where none was made) and
 * e_data[].is_inter_mb (check_ssim only).  Either pointer may be NULL.  After vp8hip_check_ssim_async both are defined only
 * if the verdict says that macroblocks were replaced (with none below the target the fallback does not touch them, and the
 * header coder is not to read them: use_intra_info = 0 gives the reference's bits). */
int vp8hip_download_intra(vp8hip_ctx *ctx, int32_t *modes, int32_t *is_inter_mb);
/* NOT the reference's behaviour, off by default: with on = 1 the emitted stream decodes, in any VP8 decoder, to exactly the
 * reconstruction the encoder keeps as its references.  The reference's does not, in three places (1, 2 found by decoding the frames
 * with a decoder written from RFC 6386, tests/vp8_decode.py, tests/test_decode_roundtrip.py):
 *  1. `construct` (GPU_kernels.cl:702-758) wraps the last three of the nine first-pass lines of a 4x4 predictor to 8 bits
 *     where the format saturates them (RFC 6386 section 18.3): wherever the six-tap filter overshoots on one of those lines --
 *     hard edges, text, graphics -- the encoder predicts from other samples than every decoder will;
 *  2. check_SSIM writes e_data.mode on every attempt (intra_part.h:964) but coefficients and reconstruction only when the
 *     attempt is kept (:1058-1086): a macroblock whose AQ attempt was kept and whose HQ / UQ attempts then failed goes out with
 *     sub-block modes that do not belong to its coefficients;
 *  3. the normal loop filter (CPU_kernels.cl:970-1075) hands the q registers of one edge to the next edge of the macroblock as
 *     its p registers without the saturation its stores apply (:1024, :1062), where a decoder filters the stored samples: on
 *     content the filter moves past 0 or 255 a few samples of the filtered reconstruction differ (found by tests/lf_ref.py;
 *     REFERENCE_DEFECTS.md has the measured rarity).
 * Each error lives on through inter prediction until the next key frame.  on = 1 saturates all nine lines, keeps the
 * modes of the attempt that was KEPT and saturates the loop filter's registers where they are handed on (vp8hip_loop_filter and
 * vp8hip_batch_loop_filter then launch the _conformant instantiations of their kernels); the output is then no longer the
 * reference's byte for byte wherever one of the three cases occurs (and identical where none does).  All members of a batch
 * must agree.
 * Outside this promise: a macroblock whose segment has loop_filter_level 0 ends the whole plane's filtering in either mode
 * (:990), where a decoder skips that macroblock alone.  Segment data made by vp8hip_auto_segments / prepare_segments_data never
 * hold a level 0 (the level is dc_q(qi + 15) / reductor with dc_q >= 17 and the reductor at most 16); a caller who sets one
 * with vp8hip_set_segments beside non-zero levels gets the reference's behaviour, not a decoder's. */
int vp8hip_conformant_stream(vp8hip_ctx *ctx, int on);
/* copy_with_padding(), encIO.h:141-196, on the device: after this call the planes handed to vp8hip_upload_current /
 * vp8hip_set_current_device / vp8hip_batch_set_current_device are tight planes of src_width x src_height (both even, less than
 * 16 below the coded size the context was created with -- 1920x1080 for a 1920x1088 context), and the step that brings them
 * into the context's surfaces repeats the last row downwards and every row's last sample to the right.  0, 0 = back to planes
 * of the coded size.  (Reconstruction planes -- vp8hip_upload_last, vp8hip_set_last_device, downloads -- always have the coded
 * size.)  Identical to the reference whenever the width needs no padding, which covers every BASELINE config; for other
 * widths the reference never writes V's right padding (:180-183 read and write U instead) and this is what it means.
 * All members of a batch must have the same source size (vp8hip_batch_create and the batched launch check it). */
int vp8hip_set_source_size(vp8hip_ctx *ctx, int src_width, int src_height);
/* The other half of the reference's three sizes (video.src_* against video.dst_*; init.h:414-417 allocates "a buffer to store the
 * resized input frame", init.h:1731-1732 sets dst = src "for now" and get_yuv420_frame's resize branch, encIO.h:228, has no body):
 * source frames LARGER than the coded picture, scaled down on the device.  After this call the planes handed to
 * vp8hip_upload_current / vp8hip_prefetch_current / vp8hip_set_current_device and the batched forms are tight planes of
 * in_width x in_height (even, at most 16384, not below dst), and ONE launch (k_scale_b, in place of the pack) scales them to
 * dst_width x dst_height and pads that to the coded size as vp8hip_set_source_size describes.  dst obeys vp8hip_set_source_size's
 * rules for src and takes its place everywhere the source size is used (display size, the region of the quality statistics, which
 * compare the reconstruction with the frame that was CODED, the scaled one: their PSNR is the codec's, not the scaler's).
 * filter: 0 = area (box) filter, integers only, alias-free at any ratio; 1 = Lanczos-3 stretched by the ratio.  The arithmetic --
 * separable, every plane on its own, chroma from (in / 2) to (dst / 2) -- is stated bit for bit in include/vp8hip_host.h
 * (vp8host_scale_taps returns the very tables the device applies).  A size pair that needs more than 32 taps in a dimension (area
 * beyond about 31:1, Lanczos beyond about 5:1), a bad size or filter: VP8HIP_ERR_ARG and nothing has changed.  0, 0, 0, 0 (any
 * filter) = no scaling, frames of the coded size; in == dst = vp8hip_set_source_size(dst); vp8hip_set_source_size ends scaling.
 * A pending vp8hip_prefetch_current made for another incoming size is dropped.  Waits for the context's streams (the tables change
 * under them): not a per-frame call.  Reference planes (vp8hip_upload_last, vp8hip_set_last_device, downloads) keep the coded size.
 * No upscaling: a decoder does that from the key frame header's scale bits.  All members of a batch must agree on all five values. */
int vp8hip_set_source_scaling(vp8hip_ctx *ctx, int in_width, int in_height, int dst_width, int dst_height, int filter);
/* Source frames in another format than tight 8-bit I420: NV12 (what a hardware decoder hands out), P010 (its 10-bit form), planar 4:2:2
 * and 4:4:4, and 10-bit planar.  format: one of enum vp8host_source_format, from include/vp8hip_host.h (which states the planes of each format and the
 * ONE integer rule that makes 8-bit I420 of them, bit for bit; vp8host_convert_frame is the rule in plain C++).  After this call the
 * three pointers handed to vp8hip_set_current_device, vp8hip_upload_current, vp8hip_prefetch_current and the batched forms
 * (vp8hip_batch_set_current_device, vp8hip_batch_upload_current, vp8hip_batch_prefetch_current) are that format's tight planes at the
 * size frames come in at (the scaler's incoming size, the source size, or the coded size).  The two-plane formats never read the third
 * pointer: pass the second one again.  ONE launch (k_convert_b) in front of the pack or scale launch, on the same stream, writes tight
 * I420 of the incoming size into a staging buffer of the context, and the pack or scale launch reads that as if the caller had handed
 * it in: convert, then pack or scale, then denoise.  Padding, scaling, denoising, the chroma scan and the quality statistics (which
 * compare with the CONVERTED frame, the one that was coded) see exactly what they see for the equivalent I420 frame; it composes with
 * vp8hip_set_source_size, vp8hip_set_source_scaling and vp8hip_set_denoise in any order of calls.
 * 0 (I420, the default): no launch, no allocation, no byte and no number changes.  An unknown format: VP8HIP_ERR_ARG and nothing has
 * changed.  A pending vp8hip_prefetch_current made in another format is dropped.  Waits for the context's streams: not a per-frame
 * call.  Reference planes (vp8hip_upload_last, vp8hip_set_last_device, vp8hip_upload_recon, downloads) stay 8-bit I420 of the coded
 * size.  All members of a batch must agree on the format (vp8hip_batch_create and the batched launch check it). */
int vp8hip_set_source_format(vp8hip_ctx *ctx, int format);
/* The packed family of the same enum, numbers 16 .. 19 (8 .. 15 are refused): YUY2 and UYVY, a capture card's packed 4:2:2, and BGRA
 * and RGBA, a renderer's or a screen capture's 32-bit surface.  ONE plane: the second and third pointers of every call above are never
 * read (they must still not be null: pass the first again).  The same single launch in front of the pack or scale launch
 * (k_convert_packed_b), the same staging buffer, the same composition with the source size, the scaler and the denoiser; a
 * vp8hip_prefetch_current stages the plane's 2 w h or 4 w h bytes.  YUY2 / UYVY follow the I422 rule.  BGRA / RGBA are read with the
 * colour matrix of vp8hip_set_source_colour: matrix = one of enum vp8host_colour_matrix: BT.601 or BT.709, limited or full range (the
 * integer tables and the rule are in include/vp8hip_host.h, vp8host_convert_frame_colour is the rule in plain C++), 0 = BT.601 limited,
 * the default.  The matrix is stored with the context and read by the RGB formats and by a tone-mapped source
 * (vp8hip_set_source_transfer) only, so it may be set before or after the format,
 * and with any other format it changes no byte.  Waits for the context's streams: not a per-frame call.  A pending
 * vp8hip_prefetch_current made under another matrix is dropped.  Anything but 0 .. 3: VP8HIP_ERR_ARG and nothing has changed.  All
 * members of a batch must agree on the matrix as on the format. */
int vp8hip_set_source_colour(vp8hip_ctx *ctx, int matrix);
/* HDR ten-bit sources made SDR.  P010 and I010 are what a hardware decoder or a phone delivers for HDR video -- HLG from phones, PQ
 * from HDR10 sources, both BT.2020 -- and the format rule alone keeps the PQ or HLG signal and the BT.2020 primaries, which every VP8
 * player then shows as BT.601 / BT.709 SDR: grey and flat, or dim and desaturated.  transfer: one of enum vp8host_transfer
 * (include/vp8hip_host.h, which states the rule bit for bit: inverse transfer, BT.2020 -> BT.709 primaries, a tone curve from `peak`
 * nits to SDR white, the SDR transfer, and the colour matrix of vp8hip_set_source_colour on the way back to Y'CbCr;
 * vp8host_tonemap_frame is the rule in plain C++); peak: the peak luminance the source was graded for, 400 .. 10000 nits.  With a
 * transfer in force ONE launch (k_tonemap_b) stands where k_convert_b stands and writes the same staging buffer, so every way a frame
 * becomes current takes it -- vp8hip_set_current_device, vp8hip_upload_current, vp8hip_prefetch_current and the batched forms -- and
 * the window in front of it and the deinterlacer, the orientation, the scaler, the pack and the denoiser behind it see what they see
 * for the equivalent SDR I420 frame.  The setter makes the rule's four tables (40 KiB) and uploads them into a buffer of the context.
 * VP8HOST_TRANSFER_SDR (0, the default; peak is not looked at): no launch, no allocation -- the table buffer is released -- and no
 * byte changes: P010 / I010 frames are converted by k_convert_b again.
 * The rule covers P010 and I010 only.  Like the colour matrix the transfer may be set before or after the format: with I420 in force
 * it is held and nothing reads it, and whichever of the two setters would complete another combination -- this one with NV12, 4:2:2,
 * 4:4:4 or a packed format in force, vp8hip_set_source_format to one of those with a transfer in force -- returns VP8HIP_ERR_ARG and
 * changes nothing, as does a peak out of range or an unknown transfer.  Waits for the context's streams: not a per-frame call.  A
 * pending vp8hip_prefetch_current made under another transfer or peak is dropped.  All members of a batch must agree on transfer and
 * peak as on the format.  (A context with hidden alt-refs refuses every source format but I420, so it never tone-maps.) */
int vp8hip_set_source_transfer(vp8hip_ctx *ctx, int transfer, int peak);
/* Layers burnt into the source frames: station logos, watermarks, subtitles, timecode.  A LAYER is a plane of lw x lh pixels of four
 * bytes, BGRA or RGBA (VP8HOST_FORMAT_BGRA / _RGBA, no other format) with straight alpha, rows `pitch` bytes apart, placed with its
 * top-left pixel at (x, y) of the PICTURE -- the upright frame the pack or scale launch writes: the source size or the scaler's
 * destination -- with an opacity 0 .. 255 and a colour matrix of its own (enum vp8host_colour_matrix; vp8hip_set_source_colour has no
 * say).  The rule -- effective alpha, luma and chroma, rounding, several layers, the padding -- is stated bit for bit in
 * include/vp8hip_host.h (vp8host_overlay_frame is its plain C++ form).  Slots 0 .. VP8HIP_MAX_OVERLAYS - 1 are applied in slot order.
 * The layer's pixels are copied before the call returns (only the layer's bytes: a 2-D copy), so the caller's buffer is free
 * afterwards (_device: once what the context's intake stream holds has run, as with vp8hip_set_current_device); k_overlay_prepare
 * then makes the layer's prepared planes, once per layer set or moved, never per frame.
 * A layer is in force FROM THE NEXT FRAME MADE CURRENT, by any route: vp8hip_set_current_device, vp8hip_upload_current (a prefetched
 * frame is composed when it is made current, with the layers in force then), the batched forms, the driver's calls.  ONE launch
 * (k_overlay_b) for all members of a batch stands behind the pack or scale launch and in front of the denoiser, so everything
 * downstream -- denoiser, chroma scan, analysis, AQ map, searches, quality statistics -- sees the composed frame, the one that is
 * coded.  Once per frame TAKEN IN, never per coding attempt.  Members of a batch may have different layers, or none; setting a layer
 * on a member of a live batch is allowed between frames: the copy and the prepare launch go on the stream the member's frames are
 * taken in on, and the host waits only where a buffer has to grow, where the pixels come from host memory, or where the context has a
 * loop filter stream of its own (vp8hip_filter_overlap).
 * A context that never sets a layer launches nothing, allocates nothing and gives the bytes it gave.
 * vp8hip_set_overlay_placement: move or fade a layer (the planes are prepared again from the retained copy).
 * vp8hip_clear_overlay: slot, or -1 = all; frees the slot's buffers; waits for the context's streams.
 * VP8HIP_ERR_ARG: a bad slot, format, matrix, size (1 .. 16384), pitch (< 4 lw), position (outside -16384 .. 16384) or opacity, a null
 * pointer, placement or clear of an empty slot (slot -1 on a context without a layer is VP8HIP_OK); VP8HIP_ERR_STATE: a context in a
 * by-reference split (vp8hip_shard_join, which in turn refuses a context with a layer).  Everything that can be refused is checked
 * before anything of the context changes.  Out of scope: premultiplied alpha, 24-bit RGB and YUVA layers, scaling or rotating a
 * layer, text rendering, reading PNG, hidden alt-ref frames (vp8hip_arf_filter_*: the window frames bypass the intake). */
#define VP8HIP_MAX_OVERLAYS 4
int vp8hip_set_overlay_host(vp8hip_ctx *ctx, int slot, int format, int matrix, const uint8_t *pixels, int lw, int lh, int pitch, int x, int y, int opacity);
int vp8hip_set_overlay_device(vp8hip_ctx *ctx, int slot, int format, int matrix, const void *pixels, int lw, int lh, int pitch, int x, int y, int opacity);
int vp8hip_set_overlay_placement(vp8hip_ctx *ctx, int slot, int x, int y, int opacity);
int vp8hip_clear_overlay(vp8hip_ctx *ctx, int slot);
int vp8hip_overlay_count(const vp8hip_ctx *ctx);      /* slots that hold a layer */
/* A CANVAS: frames composed of scaled video tiles -- a film with bars, a pillarboxed 4:3 source, the grid of a conference, a speaker
 * with thumbnails, a screen share with a camera in a corner.  The canvas is the picture (the size of vp8hip_set_source_size, or the
 * coded size); up to VP8HIP_MAX_TILES tiles {in_w, in_h, x, y, w, h, filter} say which rectangle of it takes frames of which size,
 * scaled down with which filter (0 area, 1 Lanczos-3; no upscaling, equal sizes are the identity); what no tile covers is the
 * background.  The rule -- what a valid tile is, the composition, overlaps (later tiles lie on top), the padding -- is stated bit for
 * bit in include/vp8hip_host.h ("CANVAS"; vp8host_compose_frame is its plain C++ form).
 * vp8hip_set_canvas is a setter like the others: it waits for the context's streams, builds the tiles' tables once, and is not a
 * per-frame call; n = 0 ends the canvas.  VP8HIP_ERR_ARG and nothing has changed: an invalid tile, n outside 0 .. VP8HIP_MAX_TILES, a
 * background value outside 0 .. 255, or a context with something a canvas excludes -- the scaler's incoming size
 * (vp8hip_set_source_scaling), a source format other than I420, a window, an orientation, the deinterlacer; each of those setters in
 * turn refuses while a canvas is in force.  VP8HIP_ERR_STATE: a member of a batch (vp8hip_batch_create in turn refuses a context with
 * a canvas) or a context that shares a frame's searches with other devices (and vp8hip_shard_init refuses a canvas).
 * With a canvas a frame becomes current through vp8hip_compose_current_device or vp8hip_compose_current_host: src[k] holds tile k's
 * three planes of this frame, 8-bit I420 of in_w x in_h, a pointer and a pitch each (0 = tight; no alignment is asked of either);
 * src[k].y == NULL: the tile is absent this frame (a participant without video) and leaves what is under it.  ONE launch
 * (k_compose_b) stands in the place of the pack or scale launch; everything behind it -- overlays, denoiser, analysis, AQ map, chroma
 * scan, quality statistics, searches -- runs unchanged on the composed frame, the one that is coded.  The host form brings only the
 * tiles' bytes over and returns when the host's planes are the host's again; the device form reads the planes on the context's
 * stream, as vp8hip_set_current_device does.  VP8HIP_ERR_ARG: a null pointer, a present tile with a null u or v or a pitch below its
 * plane's width.  VP8HIP_ERR_STATE: no canvas -- and with a canvas vp8hip_set_current_device, vp8hip_upload_current and
 * vp8hip_prefetch_current return VP8HIP_ERR_STATE, as vp8hip_arf_filter_* return VP8HIP_ERR_ARG; nothing has changed then.
 * A context that never sets a canvas launches nothing, allocates nothing and gives the bytes it gave.
 * Out of scope: upscaling, NV12 or ten-bit tiles, alpha between tiles, rotating a tile, borders and labels (the overlay layers do
 * those), batches, hidden alt-ref frames, a per-frame change of geometry without the setter's wait. */
int vp8hip_set_canvas(vp8hip_ctx *ctx, const vp8hip_tile *tiles, int n, int bg_y, int bg_u, int bg_v);
int vp8hip_canvas_tiles(const vp8hip_ctx *ctx);      /* tiles of the canvas in force, 0 = none */
int vp8hip_compose_current_device(vp8hip_ctx *ctx, const vp8hip_tile_planes *src /* [n] */);
int vp8hip_compose_current_host(vp8hip_ctx *ctx, const vp8hip_tile_planes *src /* [n] */);
/* Temporal noise reduction of the source frames, the third stage of the input side (libvpx: --noise-sensitivity); the reference never
 * did anything about noise.  level 1, 2, 3: every frame that becomes current -- vp8hip_upload_current, vp8hip_set_current_device, the
 * pack out of a vp8hip_prefetch_current staging buffer, vp8hip_batch_set_current_device, vp8hip_batch_upload_current, with or without a
 * source size or scaling -- passes through ONE more launch (k_denoise_b) right behind its pack or scale launch, on the same stream,
 * before anything else reads it: pyramid, edge replication, chroma scan, vp8hip_auto_segments, the searches, the quality statistics.
 * The launch works on whole coded macroblocks of the padded frame against the context's HISTORY, the previous frame taken in as it
 * left the denoiser; the rule -- per-sample steps towards the history, a per-macroblock decision that leaves moving blocks alone -- is
 * stated bit for bit in include/vp8hip_host.h (vp8host_denoise_frame).  Without a history (the first frame, after
 * vp8hip_denoise_restart, after the level changed) the frame passes through unchanged and becomes the history.  Once per frame TAKEN
 * IN: a frame coded a second time (check_SSIM's verdict) is the same current frame and is not denoised again.  The quality statistics
 * measure against the frame that was CODED, the denoised one, as they do with scaling: their PSNR is the codec's.
 * level 0 (default): off -- no launch, no byte and no number changes.  Any other value: VP8HIP_ERR_ARG and nothing has changed.
 * Turning it on or changing the level restarts the history.  Waits for the context's streams: not a per-frame call.  All members of a
 * batch must agree on the level (vp8hip_batch_create and the batched launch check it).  Shard and group contexts: not supported. */
int vp8hip_set_denoise(vp8hip_ctx *ctx, int level);
/* The next frame taken in passes through unchanged and becomes the history (a host calls it where its stream restarts: a key frame of
 * the GOP schedule, so that a closed GOP coded on its own sees the frames the serial program sees). */
int vp8hip_denoise_restart(vp8hip_ctx *ctx);
typedef struct {
    int32_t frame_number;    /* 0-based index of the frame taken in, as in vp8hip_quality */
    int32_t mbs_filtered;    /* macroblocks whose luma was filtered (0 for a frame that passed through) */
    int32_t mbs_total;
} vp8hip_denoise_stats;
/* The record of the last frame taken in.  Waits for that launch's last word only, as vp8hip_quality_result does.
 * VP8HIP_ERR_STATE: denoising off, or no frame taken in since it was turned on. */
int vp8hip_denoise_result(vp8hip_ctx *ctx, vp8hip_denoise_stats *s);

/* Interlaced source frames made progressive, a stage of the input side between the format converter and the pack or scale launch.  A
 * capture card, a broadcast archive or a decoder often hands over frames whose even and odd rows are two fields taken a field period
 * apart (1080i, 576i, 480i); VP8 has no interlaced coding tools, and coded as they are every moving edge is a comb that the search and
 * the transform pay for, the scaler mixes the fields and the denoiser sees motion in every second row.  mode 1 (field) or 2
 * (adaptive), keep = the field that survives and defines the frame's instant, 0 = top (rows 0, 2, ...), 1 = bottom: every frame that
 * becomes current -- vp8hip_upload_current, vp8hip_set_current_device, the pack out of a vp8hip_prefetch_current staging buffer,
 * vp8hip_batch_set_current_device, vp8hip_batch_upload_current -- passes through ONE more launch (k_deinterlace_b) on the same stream,
 * which reads tight I420 of the incoming size (the caller's planes, the converter's output or an upload's staging buffer) and writes
 * tight I420 into a staging buffer of the context; the pack or scale launch reads that as if the caller had handed it in.  The rule --
 * kept rows copied, missing rows a four-tap value of the kept rows (mode 1), clamped around the sample that came in by how much the
 * neighbourhood moved since the previous frame (mode 2: what stands still is woven at full vertical resolution) -- is stated bit for
 * bit in include/vp8hip_host.h (vp8host_deinterlace_frame).  One frame out per frame in: no rate doubling.
 * COMPOSITION: convert, then deinterlace, then pack or scale, then denoise, then the analysis source side.  The chroma scan, the
 * analysis and the quality statistics see the deinterlaced frame: the one that was coded.  It composes with vp8hip_set_source_size,
 * vp8hip_set_source_scaling, vp8hip_set_source_format and vp8hip_set_denoise in any order of calls.
 * Mode 2's history is the previous frame taken in AS RECEIVED (both fields, unprocessed), kept in buffers of the context: nothing
 * depends on the caller's planes after the call that took them has returned.  Without a history (the first frame, after
 * vp8hip_deinterlace_restart, after the mode, the parity or the incoming size changed) the frame is mode 1's.  Once per frame TAKEN
 * IN: a frame coded a second time (check_SSIM's verdict) is the same current frame and is not deinterlaced again.
 * mode 0 (default): off -- no launch, no allocation, no byte and no number changes.  Any other mode or keep, or an incoming height
 * below 4 (every plane needs a row of each field; the size setters refuse such a height while a mode is set): VP8HIP_ERR_ARG and
 * nothing has changed.  Turning it on, or changing mode or parity, restarts the history and drops a pending vp8hip_prefetch_current.
 * Waits for the context's streams: not a per-frame call.  All members of a batch must agree on mode and parity
 * (vp8hip_batch_create and the batched launch check it).  Shard and group contexts: not supported. */
int vp8hip_set_deinterlace(vp8hip_ctx *ctx, int mode, int keep);
/* The next frame taken in has no history (a host calls it where its stream restarts: a key frame of the GOP schedule, so that a closed
 * GOP coded on its own sees the frames the serial program sees). */
int vp8hip_deinterlace_restart(vp8hip_ctx *ctx);
typedef struct {
    int32_t frame_number;    /* 0-based index of the frame taken in, as in vp8hip_quality */
    int32_t woven;           /* luma samples of missing rows that left as they came (0 in mode 1 and without a history) */
    int32_t missing;         /* luma samples of missing rows */
} vp8hip_deinterlace_stats;
/* The record of the last frame taken in.  Waits for that launch's last word only, as vp8hip_quality_result does.
 * VP8HIP_ERR_STATE: deinterlacing off, or no frame taken in since it was turned on. */
int vp8hip_deinterlace_result(vp8hip_ctx *ctx, vp8hip_deinterlace_stats *s);

/* The two geometric stages of the input side, each opt-in, each ONE more launch; pure data movement whose rule is stated bit for bit
 * in include/vp8hip_host.h.  After them the order of the input side is
 *     window -> convert -> deinterlace -> orient -> scale or pack -> denoise -> analysis.
 * THE WINDOW.  A hardware decoder, a capture API or a renderer hands out SURFACES: rows a pitch apart (2048 bytes for a 1920-wide NV12
 * frame) and the picture a window inside (1920x1080 in 1920x1088, a letterboxed 1920x800 in 1920x1080).  pitch = the bytes between the
 * rows of each of the three planes (entries of planes the source format lacks are ignored), (x, y) = the window's top-left luma
 * sample: from now on the three pointers of every call that makes a frame current -- vp8hip_set_current_device,
 * vp8hip_upload_current, vp8hip_prefetch_current, the three batched forms -- are the plane bases of a surface in the context's source
 * format, and the frame is the window of the INCOMING SIZE (below) at (x, y): vp8host_source_window has the table and
 * vp8host_window_frame is the rule in plain C++.  No byte outside the window is ever read; the surface's own size is no parameter;
 * neither pitch nor base needs any alignment.  Planes in DEVICE memory: one launch (k_window_b) for all members of a batch, in front of
 * everything else, writes the window's tight planes into a staging buffer of the context, and the next stage reads that as if the
 * caller had handed it in.  Planes in HOST memory: only the window's bytes travel, as 2-D copies into the staging buffers the uploads
 * already use; no launch.
 * pitch NULL (default): off.  VP8HIP_ERR_ARG and nothing has changed: x or y negative or odd, or for a plane the format has
 * pitch[p] < ((x + width) >> hs) * bpe.  Checked against the format and incoming size in force at the call; the format, size, scaling
 * and orientation setters refuse a change that would make the window in force invalid.
 * THE ORIENTATION.  Phone and action-camera video is stored sideways or upside down; VP8 in IVF or WebM carries no rotation tag, so a
 * transcoder bakes the rotation in.  turns = 0..3 clockwise quarter turns, mirror = 0 or 1: a left-right flip of the incoming frame
 * FIRST, then the rotation (vp8host_orient_frame).  Every size the library knows describes the UPRIGHT frame: the coded size,
 * vp8hip_set_source_size, the scaler's in_width x in_height, the quality statistics' region.  With an odd `turns` the planes handed
 * in -- the INCOMING SIZE, which is also the window's -- are in_height wide and in_width high; the window, the converter and the
 * deinterlacer (fields are rows of the source) work at that raw size, the scaler or the pack sees the upright one.  One launch
 * (k_orient_b) behind the deinterlacer and in front of the pack or scale launch reads tight I420 and writes tight I420 into a staging
 * buffer of its own.  (0, 0), the default: off.  Anything else out of range, a raw height below 4 while a deinterlacer mode is set, or
 * a window in force that the raw size would make invalid: VP8HIP_ERR_ARG and nothing has changed.
 * BOTH: once per frame TAKEN IN, never per coding attempt.  Off is off: no launch, no allocation, no byte and no number changes.
 * They compose with the size, scaling, format, colour, deinterlace, denoise and analysis setters in any order of calls.  A setter
 * waits for the context's streams (not a per-frame call) and drops a pending prefetch of the context and of its batch.  All members of
 * a batch must agree on pitches, origin, turns and mirror (vp8hip_batch_create and the batched launch check it).  Reconstructions
 * (vp8hip_upload_last, vp8hip_set_last_device, vp8hip_upload_recon) stay tight, upright and of the coded size. */
int vp8hip_set_source_window(vp8hip_ctx *ctx, const int32_t *pitch /* [3], NULL = off */, int x, int y);
int vp8hip_set_source_orientation(vp8hip_ctx *ctx, int turns, int mirror);

/* prepare_filter_mask_and_non_zero_coeffs(), loop_filter.h:25-55.  nz_out: [MBs] or NULL.
 * (vp8hip_inter_transform already produced mask and counts for its own coefficients; this call
 * recomputes them from the device copy, e.g. after vp8hip_upload_mb_data.) */
int vp8hip_prepare_filter_mask(vp8hip_ctx *ctx, int32_t *nz_out);

/* do_loop_filter(), loop_filter.h:185-190: the loop filter of the context's type (vp8hip_set_loop_filter_type; the normal
 * filter by default) on the reconstruction, in place, after which that reconstruction IS the LAST reference of the next
 * vp8hip_inter_transform. */
int vp8hip_loop_filter(vp8hip_ctx *ctx);
/* The loop filter vp8hip_loop_filter / vp8hip_batch_loop_filter apply from the next call on: 0 = the normal filter (RFC 6386
 * section 15.3, the default and the reference's), 1 = the simple filter (section 15.2: luma only, p0 and q0 only, no hev; a
 * macroblock whose segment has loop_filter_level 0 is skipped and the rest of the plane is filtered).  The frame header's
 * filter_type bit (vp8hip_header_params / vp8bs_frame.loop_filter_type) must say the same, or decoders drift from the encoder's
 * reconstruction.  Any other value: VP8HIP_ERR_ARG. */
int vp8hip_set_loop_filter_type(vp8hip_ctx *ctx, int type);
/* ---- quality of the coded frames (opt-in) -------------------------------------------------------------------------------
 * With stats on, every vp8hip_loop_filter / vp8hip_batch_loop_filter measures the FILTERED reconstruction against the current frame
 * as it was handed in, on the device, on the stream the filter runs on, without a host wait: the source region only (the size of
 * vp8hip_set_source_size, or the coded size; chroma ((w + 1) / 2) x ((h + 1) / 2)), never the padding.  Per plane Y, U, V the exact
 * sum of squared errors, PSNR = 10 log10(samples 255^2 / sse) (100 when sse is 0, libvpx's cap), and SSIM in libvpx's integer form
 * (8x8 windows every 4 samples, c1 = 26634, c2 = 239708; the mean over the plane's windows, 1.0 / 0.0 for a plane without a whole
 * window and sse 0 / not 0); ssim_all = 0.8 ssim_Y + 0.1 (ssim_U + ssim_V).  Deterministic: the same bits whether a context runs alone
 * or in a batch.  These numbers describe the encoder's reconstruction: what a decoder shows whenever the stream decodes to it (with
 * vp8hip_conformant_stream 0 the reference's stream defects, REFERENCE_DEFECTS.md, can make a decoder's picture differ). */
typedef struct {
    int32_t frame_number;    /* 0-based index of the current frame measured, in the order the context received its frames */
    int32_t is_key;          /* the reconstruction came from vp8hip_intra_transform */
    uint64_t sse[3];         /* Y, U, V */
    uint64_t samples[3];
    double psnr[3];
    double psnr_all;         /* over sse_Y + sse_U + sse_V and samples_Y + samples_U + samples_V */
    double ssim[3];
    double ssim_all;
} vp8hip_quality;
/* Over every frame made final so far.  A frame's record becomes final when the context measures a frame with ANOTHER frame_number: a
 * second filter of the same current frame (a frame sent back by check_SSIM and coded again as a key frame) replaces the first's record. */
typedef struct {
    int64_t frames;
    uint64_t sse[3], samples[3];   /* summed */
    double psnr[3];                /* from the summed sse and samples per plane (vpxenc's "Y", "U", "V") */
    double psnr_all;               /* from the summed sse and samples of all planes (vpxenc's "Overall") */
    double psnr_avg;               /* mean of the frames' psnr_all (vpxenc's "Avg") */
    double ssim[3];                /* mean of the frames' ssim[p] */
    double ssim_all;               /* mean of the frames' ssim_all */
    double psnr_min;               /* lowest psnr_all (0 without frames) ... */
    int64_t psnr_min_frame;        /* ... and its frame_number (-1 without frames) */
} vp8hip_quality_totals;
/* on = 1: from the next filter on, every frame is measured; turning it on from off starts a new summary.  0 (default): nothing runs.
 * With vp8hip_set_source_scaling the frame measured against is the one that was coded, the SCALED source, over dst_width x dst_height:
 * the PSNR is the codec's, not the scaler's. */
int vp8hip_set_quality_stats(vp8hip_ctx *ctx, int on);
/* The record of the last frame measured.  Waits for that measurement alone (a word its launch writes last), not for the stream.
 * VP8HIP_ERR_STATE: stats off, or nothing measured yet. */
int vp8hip_quality_result(vp8hip_ctx *ctx, vp8hip_quality *q);
/* The summary since stats were turned on, the last frame measured included.  Waits the same way.  VP8HIP_ERR_STATE: stats off. */
int vp8hip_quality_summary(vp8hip_ctx *ctx, vp8hip_quality_totals *s);
/* ---- frame analysis statistics (opt-in): what a rate controller measures -----------------------------------------------------
 * libvpx's first-pass record cut to what this encoder knows, every field an exact integer; the two rules are stated bit for bit in
 * include/vp8hip_host.h.  SOURCE SIDE: every frame that becomes current -- vp8hip_upload_current, vp8hip_set_current_device, the pack
 * out of a vp8hip_prefetch_current staging buffer, vp8hip_batch_set_current_device, vp8hip_batch_upload_current -- passes through ONE
 * more launch (k_analyse_src_b) behind its convert / pack / scale / denoise launches on the same stream: it measures the coded luma
 * (padding included, as the searches see it) against the context's history plane, the luma of the previous frame taken in, and
 * writes the new luma into the history.  Once per frame TAKEN IN, never per coding attempt.  CODING SIDE: every vp8hip_loop_filter /
 * vp8hip_batch_loop_filter is followed, on the filter's stream and without a host wait, by k_analyse_mb_b, one reduction over the
 * per-macroblock arrays as the frame's coding attempt left them; a second filter of the same current frame (a frame sent back by
 * check_SSIM and coded again as a key frame) replaces the first's record.
 * on = 0 (default): no allocation, no launch, no byte and no number changes.  Turning it on allocates the history plane and the record
 * and starts without a history.  Waits for the context's streams: not a per-frame call.  All members of a batch must agree
 * (vp8hip_batch_create and the batched launch check it).  A context that shares a frame's searches with other devices (vp8hip_shard_init)
 * codes only part of a frame: turning analysis on for one is refused with VP8HIP_ERR_STATE, and so is vp8hip_shard_init while it is on. */
typedef struct {
    int32_t frame_number;    /* 0-based index of the frame, in the order the context received its frames, as in vp8hip_quality */
    int32_t is_key;          /* the coding attempt measured came from vp8hip_intra_transform (0 when coded is 0) */
    int32_t have_prev;       /* 0: no history (first frame, after a restart); the three temporal fields are then 0 */
    int32_t static_mbs;
    uint64_t spatial, temporal_sse, temporal_sad;
    int32_t coded;           /* 0: the frame was taken in and not coded yet; every field below is then 0 */
    int32_t mbs_total, mbs_intra, mbs_split, mbs_zero_mv, mbs_no_coeffs;
    int32_t mbs_ref[3];      /* LAST, GOLDEN, ALTREF */
    int32_t segment_mbs[4];
    int32_t reserved;        /* 0 */
    uint64_t mv_abs_sum[2];  /* x, y; quarter pixels */
    int64_t mv_sum[2];
    uint64_t mv_sq_sum;
    uint64_t nz_coeffs;
} vp8hip_analysis;
int vp8hip_set_analysis(vp8hip_ctx *ctx, int on);
/* The next frame taken in has no history: have_prev = 0 (a host calls it where its stream restarts: a key frame of the GOP schedule, so
 * that a closed GOP coded on its own gives the records the serial program gives). */
int vp8hip_analysis_restart(vp8hip_ctx *ctx);
/* The record of the last frame coded -- while it is the last or the last but one frame taken in (a host may hand the next frame over
 * early) -- or else of the last frame taken in, with coded = 0.  Waits for the two measurements alone (a word each launch writes
 * last), not for the streams.  VP8HIP_ERR_STATE: analysis off, or no frame taken in since it was turned on. */
int vp8hip_analysis_result(vp8hip_ctx *ctx, vp8hip_analysis *a);
/* ---- a quantiser per macroblock: the caller's segment map, or variance-adaptive quantisation ----------------------------
 * Every inter frame carries the four-segment map with the four quantiser indices of the ladder (vp8hip_auto_segments); by default
 * the reference's SSIM loop picks a macroblock's segment, and with ssim_target = -1 that is segment 3 for every macroblock.  Here
 * something else picks it; the rule is stated bit for bit in include/vp8hip_host.h.
 *   mode 0 (default): off -- no launch, no allocation, no byte and no number changes.
 *   mode 1: the caller's map (libvpx's VP8E_SET_ROI_MAP): MBs bytes, raster order, each 0..3, handed over with
 *           vp8hip_set_segment_map_device or vp8hip_upload_segment_map and in force until replaced.  Without a map: segment 3
 *           everywhere, which is exactly the default's frames.
 *   mode 2: variance-adaptive, strength 1..3 (mode 0 and 1 ignore strength).  Every frame that becomes current passes through two more launches at the end
 *           of its intake (k_aq_map_b, k_aq_seg_b) that make the map from the coded luma as the searches read it: flat macroblocks
 *           take the finer segments, busy ones the coarser.  Once per frame TAKEN IN, never per coding attempt.  A frame taken in
 *           before mode 2 was set has no map and is coded in segment 3.
 * In mode 1 or 2 vp8hip_inter_transform, vp8hip_inter_finish and vp8hip_batch_inter_transform launch the mapped form of the
 * macroblock kernel (k_mb_p_map): each macroblock runs ONE transform pass,
 * in segment map[mb] & 3, and MB_segment_id is that value; MB_SSIM is still computed.  Key frames stay as they are: segment 0, no
 * segmentation in the header.  Everything behind the transform (loop filters, entropy stage, analysis record) reads MB_segment_id.
 * VP8HIP_ERR_ARG and nothing has changed: mode outside 0..2, strength outside 1..3 in mode 2.  VP8HIP_ERR_STATE and nothing has
 * changed (mode 1 or 2, or a map): a context created with ssim_target >= 0 (the SSIM ladder and the map both own the segment id), or one
 * that shares a frame's searches with other devices (vp8hip_shard_init, which in turn refuses a context with a mode).  Turning a mode
 * on allocates the maps; the setter waits for the context's streams: not a per-frame call.  All members of a batch must agree on
 * mode and strength (vp8hip_batch_create and the batched launches check it); the maps are the members' own. */
int vp8hip_set_segment_mode(vp8hip_ctx *ctx, int mode, int strength);
int vp8hip_segment_mode(const vp8hip_ctx *ctx, int *mode, int *strength);      /* what is in force (either pointer may be NULL) */
/* The caller's map, MBs bytes: copied into the context on its stream (from device memory: values are taken & 3, and the map may be
 * reused when the call returns only after the stream has got there; from host memory: a value above 3 is refused with VP8HIP_ERR_ARG,
 * and the call returns when the copy is done).  A map may be set in any mode; mode 1 reads it. */
int vp8hip_set_segment_map_device(vp8hip_ctx *ctx, const uint8_t *map);
int vp8hip_upload_segment_map(vp8hip_ctx *ctx, const uint8_t *host_map);
/* The map in force for the current frame, MBs bytes (mode 1 without a map: all 3), and in mode 2 the e of the rule for every
 * macroblock (e_out may be NULL; not NULL outside mode 2: VP8HIP_ERR_STATE).  Blocks.  VP8HIP_ERR_STATE: mode 0, or mode 2 and no
 * frame taken in since it was set. */
int vp8hip_download_segment_map(vp8hip_ctx *ctx, uint8_t *map_out, uint8_t *e_out);
/* ---- hidden alternate reference frames (opt-in; NOT the reference, which never codes a frame it does not show) -------------------
 * libvpx's --auto-alt-ref with its ARNR filter, the placement left to the caller: a frame made by motion-compensated temporal
 * filtering of up to VP8HOST_ARF_MAX_FRAMES source frames around a centre frame is coded as an inter frame that is NOT shown
 * (show_frame = 0), refreshes ALTREF only (refresh_last = 0) and so gives the frames behind it a reference cleaner than their
 * neighbours.  A context that never calls these entry points launches nothing, allocates nothing and changes no byte or number.
 * vp8hip_arf_filter_device: frames[k][0..2] = the Y, U, V planes of frame k, tight 8-bit I420 of the context's INCOMING size (its
 * scaler's incoming size, else its source size, else the coded size) in this device's memory; centre in 0 .. n - 1; strength 0 .. 6.
 * ONE launch (k_arf_filter_b; the rule is stated bit for bit in include/vp8hip_host.h, vp8host_arf_filter_frame) writes the filtered
 * frame into a staging buffer the context owns (allocated on first use), and that frame becomes the CURRENT frame through the
 * ordinary intake, exactly as if vp8hip_set_current_device had been given it: padding, scaling, orientation and the segment map of
 * mode 2 see it as they see a source frame.  The planes may be reused once the context's stream has got there.
 * vp8hip_arf_filter_host: the same for planes in host memory (uploaded into a buffer of the context's; returns when they were read).
 * vp8hip_arf_result: the (tile, frame k != centre) pairs of the last filter launch by block weight 0, 1, 2; blocks.
 * vp8hip_arf_release: frees the two buffers (whatever reads them ends first: not a per-frame call); the next filter call makes them again.
 * The frame is then coded like any inter frame -- vp8hip_auto_segments or vp8hip_set_segments, vp8hip_inter_transform with the
 * rotation owed by the previous shown frame -- and ENDS with vp8hip_loop_filter_hidden in the place of vp8hip_loop_filter: the
 * filtered reconstruction becomes ALTREF, a slot assignment, with its replicated edges and its pyramid made behind the filter; LAST
 * stays the surface it is, and the intake is left as the hidden frame found it: the current frame is the last shown frame again, so
 * the next frame taken in is compared with it (vp8hip_chroma_change) and numbered behind it.  The rotation is consumed by the hidden frame's transform: the next shown frame's takes prev_is_golden =
 * prev_is_altref = 0, or LAST overwrites the new ALTREF.  Its bytes: vp8hip_header_params.is_altref = VP8HIP_ALTREF_HIDDEN.
 * VP8HIP_ERR_ARG and nothing has changed: n, centre or strength out of range, a null plane, a context with a source format other than
 * I420, a source window, a deinterlacer, a denoiser or analysis (the last three keep a history of the frames taken in that a frame
 * out of order would disturb).  VP8HIP_ERR_STATE: a member of a batch, a context that shares a frame's searches with other devices
 * (vp8hip_shard_init), a context with vp8hip_filter_overlap (the next frame's ALTREF search would start beside the filter that
 * writes ALTREF; the combination is refused rather than ordered), vp8hip_arf_result before any filter launch, and
 * vp8hip_loop_filter_hidden without an inter reconstruction, or with an armed check_SSIM (a hidden frame has no fallback). */
#define VP8HIP_ALTREF_HIDDEN 2
int vp8hip_arf_filter_device(vp8hip_ctx *ctx, const void *const (*frames)[3], int n, int centre, int strength);
int vp8hip_arf_filter_host(vp8hip_ctx *ctx, const uint8_t *const (*frames)[3], int n, int centre, int strength);
int vp8hip_arf_result(vp8hip_ctx *ctx, int32_t weights[3]);
int vp8hip_arf_release(vp8hip_ctx *ctx);
int vp8hip_loop_filter_hidden(vp8hip_ctx *ctx);
/* ---- temporal layers (opt-in): the end of a SHOWN inter frame whose reconstruction refreshes the buffer the caller names --------------
 * The rule that names it -- which references a frame of a two- or three-layer stream searches, what it refreshes and which layer it
 * belongs to -- is vp8host_temporal_step (include/vp8hip_host.h).  The frame is coded like any inter frame (vp8hip_inter_transform
 * with the rule's use_golden and use_altref = 0, check_SSIM if wanted) and ENDS with vp8hip_loop_filter_refresh in the place of
 * vp8hip_loop_filter:
 *   refresh = VP8HIP_REFRESH_LAST, filter = 1:    vp8hip_loop_filter, exactly.
 *   refresh = VP8HIP_REFRESH_GOLDEN, filter = 1:  the filter runs and the reconstruction becomes GOLDEN -- a slot assignment, as the
 *       hidden ending's -- with its replicated edges and its pyramid made behind the filter.  LAST, and what the context knows
 *       about LAST, stay.
 *   refresh = VP8HIP_REFRESH_NONE:  the reconstruction is dropped: no frame will read it.  With filter = 0 NOTHING is launched: no
 *       filter, no edges, no pyramid.  With filter = 1 the filter runs for what rides behind or in its launch.
 * The frame is shown, so unlike the hidden ending the intake is not stepped back, and the quality measurement, the analysis record and
 * an armed check_SSIM's verdict follow the filter as they follow vp8hip_loop_filter.  Its bytes: vp8hip_header_params.is_golden =
 * VP8HIP_GOLDEN_ONLY (refresh_golden_frame = 1, refresh_alternate_frame = 0 with its copy field 0, sign biases 0,
 * refresh_entropy_probs = 0, refresh_last = 0, show_frame = 1) or VP8HIP_REFRESH_NOTHING (both refresh flags 0, both copy fields 0,
 * the rest alike); is_altref is not read for either.  No entropy state passes from frame to frame (every frame sends every
 * probability and the whole segment map), so a stream without the dropped frames decodes.
 * VP8HIP_ERR_ARG: refresh or filter out of range, filter = 0 with a refresh other than NONE.  VP8HIP_ERR_STATE, for GOLDEN and NONE:
 * no inter reconstruction, a member of a batch, a context that shares a frame's searches with other devices, a context with
 * vp8hip_filter_overlap (the next frame's GOLDEN search would start beside the filter that writes GOLDEN), and filter = 0 with an
 * armed check_SSIM (the verdict rides in the filter's launch). */
#define VP8HIP_REFRESH_LAST 0
#define VP8HIP_REFRESH_GOLDEN 1
#define VP8HIP_REFRESH_NONE 2
#define VP8HIP_GOLDEN_ONLY 2
#define VP8HIP_REFRESH_NOTHING 3
int vp8hip_loop_filter_refresh(vp8hip_ctx *ctx, int refresh, int filter);
/* ---- cyclic intra refresh (opt-in): forced intra macroblocks in the inter reconstruction in flight -----------------------------------
 * The rule -- which macroblocks at phase q of period P, what a forced macroblock becomes, why they are independent of each other -- is
 * vp8host_intra_refresh_forced (include/vp8hip_host.h).  Call it between vp8hip_inter_transform (or vp8hip_inter_finish) and the loop
 * filter: ONE launch (k_intra_refresh, one workgroup per forced macroblock, no waits), asynchronous, nobody waiting.  It writes the
 * forced macroblocks' coefficients, unfiltered reconstruction, MB_parts, MB_SSIM, non-zero counts and filter masks -- no
 * vp8hip_prepare_filter_mask is needed behind it -- and EVERY macroblock's is_inter and modes, so vp8hip_download_intra and the header
 * coders with use_intra_info = 1 read defined arrays; MB_segment_id stays.  The analysis record counts the forced macroblocks as
 * intra; an armed check_SSIM (vp8hip_check_ssim_async, before or behind this call) still reports replaced = 0: a refresh is not a
 * replacement that sends a frame back as a key frame.  The SYNCHRONOUS vp8hip_check_ssim initialises is_inter and modes itself and
 * is refused (VP8HIP_ERR_STATE, nothing changed) on a reconstruction that carries forced macroblocks.
 * The caller owns q (vp8drv_set_intra_refresh keeps it for the native frame loop) and decides which frames are refreshed: by the
 * rule, shown frames that refresh LAST.
 * VP8HIP_ERR_ARG: period outside 4 .. 1024, q < 0.  VP8HIP_ERR_STATE: a context created with ssim_target > -1 (the SSIM ladder owns
 * the segment id, and its fallback the intra arrays), a context that shares a frame's searches with other devices, no inter
 * reconstruction in flight.  Nothing has changed after a refusal. */
int vp8hip_intra_refresh(vp8hip_ctx *ctx, int period, int q);
/* on = 1: the context gets a second stream, and work that does not depend on the filtered frame runs beside the loop filter:
 * the entropy stage of the same frame (vp8hip_count_probs ... vp8hip_encode_frame), the next frame's upload, parameter scan
 * and GOLDEN / ALTREF searches.  The filter stays on the stream the frame was coded on and the CONTEXT moves to the other one
 * until a call needs the filtered frame (it then moves back, behind the filter): a video's frame-to-frame dependency chain
 * is launches of one stream.  vp8hip_stream() names the stream the next call will use.  A single video coded frame after
 * frame: 0.60 -> 0.43 ms per 1080p frame.  Off by default: a host that runs many contexts side by side (GOP chunks) already
 * keeps the device busy and advances them in batches (vp8hip_batch_create), which excludes this mode. */
int vp8hip_filter_overlap(vp8hip_ctx *ctx, int on);

/* ---- coefficient entropy stage: the consumer of the coefficient buffer -------------------------
 * The reference runs it on a CPU OpenCL device, one work-item per partition (vp8enc.cpp:48-94).  Here the
 * statistics are a device histogram over all blocks.  Input = the context's current coefficients, MB_parts
 * and non-zero counts (as left by vp8hip_inter_transform, or vp8hip_upload_mb_data + vp8hip_prepare_filter_mask).
 *
 * count_probs + num_div_denom + the two read-backs of vp8enc.cpp:58-69.
 *   new_probs[4][8][3][11]       probability (1..255) of a zero branch per context, summed over the partitions;
 *   new_probs_denom[4][8][3][11] partition 0's denominators (1 + branches seen), which is what the reference's
 *                                host code inspects to fall back to the default probabilities (:70-76).
 * num_partitions: 1, 2, 4 or 8 (partition p owns macroblock rows p, p+n, ...). */
#define VP8HIP_NUM_COEFF_PROBS 1056
int vp8hip_count_probs(vp8hip_ctx *ctx, int num_partitions, uint32_t *new_probs, uint32_t *new_probs_denom);

/* The write-back of the final probabilities, encode_coefficients and the read of the partitions (vp8enc.cpp:77-81,
 * gather at entropy_host.cpp): codes the macroblock rows of every partition with the boolean coder, on the
 * device, and returns partition p at partitions + p * partition_step with its length in partition_sizes[p].
 * coeff_probs[4][8][3][11] (low byte used) = new_probs after the host's default-probability fallback.
 * Must follow vp8hip_count_probs for the same coefficients and num_partitions (it reuses the block contexts).
 * VP8HIP_ERR_OVERFLOW if a partition does not fit partition_step (nothing is written then).  The device scratch
 * starts at 64 bools per 4x4 block on average and is doubled -- the frame is then coded again -- up to the 304 a
 * block can produce at most, so no frame is refused for the device's sake. */
int vp8hip_encode_coefficients(vp8hip_ctx *ctx, const uint32_t *coeff_probs, int num_partitions, int partition_step,
                               uint8_t *partitions, int32_t *partition_sizes);

/* encode_header(), entropy_host.cpp:709-1256 -- the first partition (frame header, then segment id / skip flag /
 * reference frame / motion-vector mode and vectors or intra modes of every macroblock) -- coded on the device from
 * the results that are already there, instead of on one host thread after downloading them (2-3 ms per 1080p frame
 * there).  Uses MB_segment_id, the non-zero counts, MB_reference_frame, MB_parts, MB_vectors as the transform and
 * vp8hip_prepare_filter_mask left them, the segment data in force, the coefficient statistics of the preceding
 * vp8hip_count_probs (the header transmits the probability of every context that occurred) and, for key frames or
 * with use_intra_info, e_data.mode / is_inter_mb of vp8hip_intra_transform / vp8hip_check_ssim.  skip_prob,
 * prob_intra, prob_last/prob_gf, the segment-map and motion-vector probabilities are derived on the device as
 * encode_header derives them.  Writes the partition with its 3- or 10-byte uncompressed chunk to `out`; *size = its
 * size (frames.encoded_frame_size after encode_header).  Blocks.  The host implementation of the same function is
 * vp8bs_encode_header (include/vp8hip_bitstream.h); vp8bs_gather_frame appends the coefficient partitions. */
#define VP8HIP_SHARPNESS_ON_DEVICE INT32_MIN
typedef struct {
    int32_t is_key, is_golden, is_altref;    /* frames.current_is_{key,golden,altref}_frame; is_altref = VP8HIP_ALTREF_HIDDEN (inter frames): a
                                                hidden frame -- show_frame = 0 in the frame tag, refresh_alternate = 1, refresh_last = 0;
                                                is_golden = VP8HIP_GOLDEN_ONLY / VP8HIP_REFRESH_NOTHING (inter frames): a shown frame of a
                                                temporal layer that refreshes GOLDEN only / no buffer (vp8hip_loop_filter_refresh) */
    int32_t loop_filter_type;                /* video.loop_filter_type: 0 normal, 1 simple -- the filter the context applies (vp8hip_set_loop_filter_type) */
    int32_t loop_filter_sharpness;           /* video.loop_filter_sharpness; VP8HIP_SHARPNESS_ON_DEVICE = the value vp8hip_auto_segments
                                                computed.  (Not -1: get_loopfilter_strength's `int` accumulator overflows on large noisy
                                                frames, vp8enc.cpp:112-126, and the sharpness it then leaves is NEGATIVE -- -1 on a 1080p
                                                frame of noise; the reference writes its low three bits into the header, and so must this.) */
    int32_t partitions_log2;                 /* video.number_of_partitions_ind */
    int32_t width, height;                   /* video.dst_width/height for key frames; 0 = the coded size */
    int32_t use_intra_info;                  /* inter frames: 1 = vp8hip_check_ssim ran on this frame */
} vp8hip_header_params;
int vp8hip_encode_header(vp8hip_ctx *ctx, const vp8hip_header_params *params, uint8_t *out, size_t capacity, size_t *size);

/* entropy_encode() + gather_frame() (vp8enc.cpp:48-94, encIO.h:1-30) in one call and entirely on the device:
 * count_probs, num_div_denom, the default-probability fallback, encode_coefficients, encode_header, then the frame
 * is assembled in `out` -- first partition, the sizes of all coefficient partitions but the last, the partitions.
 * Nine kernel launches, the last of which writes the finished frame into pinned host memory itself (no copy command),
 * instead of the 21 launches and eight blocking transfers of the step-by-step calls; any frame
 * size (the step-by-step vp8hip_encode_coefficients stops at 2^20 4x4 blocks).  params->partitions_log2 is ignored (derived from num_partitions).  *size = bytes of the finished frame:
 * what the reference hands to write_output_file(). */
int vp8hip_encode_frame(vp8hip_ctx *ctx, int num_partitions, const vp8hip_header_params *params, uint8_t *out, size_t capacity,
                        size_t *size);

/* init_all() allocates everything before the first frame (init.h:430-593); the entropy stage's scratch (about 100 MB at 1080p)
 * and the pinned frame buffer are made when the first frame is asked for, or here -- a host that wants no allocation inside its
 * frame loop calls this once after vp8hip_create. */
int vp8hip_reserve_frame_path(vp8hip_ctx *ctx);
/* ... sized for the densest frame there can be (304 bools per 4x4 block instead of 64; about 270 MB at 1080p): no frame ever has to
 * be coded a second time because the scratch was too small.  For a caller that starts the next frame before it takes the bytes of
 * this one (vp8hip_encode_frame_begin below). */
int vp8hip_reserve_frame_path_dense(vp8hip_ctx *ctx);

/* The same in two halves, for a host thread that drives several contexts (GOP chunks) or wants the next frame under way before
 * it takes this one's bytes: _begin enqueues the whole entropy stage and the read-back and returns at once; _end waits for the
 * stage (not for whatever was enqueued behind it) and fills `out`.  VP8HIP_ERR_STATE from _begin while a frame is pending,
 * from _end when none is.
 * With vp8hip_filter_overlap the stage runs on a stream of its own beside the frame's loop filter, and the NEXT frame may be
 * started between _begin and _end (vp8hip_set_current_device ... vp8hip_loop_filter: its side work runs beside filter and stage,
 * its macroblock kernel waits for the stage): one video then costs a frame what it costs without frames out.  Only the recode
 * after a scratch overflow is lost that way (its input is overwritten): _end then returns VP8HIP_ERR_STATE -- call
 * vp8hip_reserve_frame_path_dense once and it cannot happen.  Without the overlap mode no other call may be made on the context
 * between the two. */
int vp8hip_encode_frame_begin(vp8hip_ctx *ctx, int num_partitions, const vp8hip_header_params *params);
int vp8hip_encode_frame_end(vp8hip_ctx *ctx, uint8_t *out, size_t capacity, size_t *size);

/* filtered planes = the current LAST (debug.h:8-36 dump; host intra fallback input) */
int vp8hip_download_last(vp8hip_ctx *ctx, uint8_t *y, uint8_t *u, uint8_t *v);

int vp8hip_synchronize(vp8hip_ctx *ctx);
/* hipStream_t the context launches on (for event timing by the caller) */
void *vp8hip_stream(vp8hip_ctx *ctx);
int vp8hip_last_hip_error(const vp8hip_ctx *ctx);
/* Hardware queues the HIP runtime of this process multiplexes its streams onto.  The runtime reads GPU_MAX_HW_QUEUES once, at the
 * process's first HIP call (default 4), and streams that share a queue serialise -- so the LIBRARY sets it when it is loaded (a
 * constructor: setenv("GPU_MAX_HW_QUEUES", "16", 0), i.e. unless the host exported a value of its own): a host that links or dlopens
 * libvp8hip.so before it touches the GPU runs on 16 queues without knowing any of this (the reference creates the queues it needs
 * itself, init.h:1162-1165).  16: measured optimum; beyond 24 queues per process the hardware scheduler rotates them and
 * context-switches running waves.  Returns the value in force as far as the library can tell: what the environment said when the
 * runtime initialised.  If the runtime was ALREADY initialised when the library was loaded (a host that made HIP calls first) the
 * constructor changes nothing, says so on stderr once (VP8HIP_QUIET=1 silences it) and this returns what the environment held then
 * (4 if nothing).  vp8hip_inter_transform prints one line when more contexts launch on streams of their own than there are queues.
 * SIDE EFFECTS of that constructor, stated: (1) setenv() in the host process -- safe when the library is loaded at program start or
 * before the host has made threads; a host that dlopen()s it while other threads may call getenv() exports GPU_MAX_HW_QUEUES itself or
 * sets VP8HIP_NO_ENV=1, with which the library touches nothing; (2) the variable is inherited by the host's child processes. */
int vp8hip_hw_queues(void);

const char *vp8hip_status_string(int status);
/* The ABI of this header as MAJOR * 1000 + MINOR: MAJOR changes when an existing entry point or struct changes its meaning or
 * layout (vp8drv_config grew in round 2: 2; vp8drv_stats grew by refs_searched and vp8drv_default_config turned check_ssim on
 * -- return values and counters provisional until vp8drv_resolve -- in round 3: 3), MINOR when entry points are added.  A host
 * built against an older header checks it once after loading the library.  3001: the shard, device-memory and frame-check entry points;
 * 3002: vp8drv_encode_video_device; 3003: vp8hip_import_last, vp8hip_group_*, the load-time hardware-queue setting;
 * vp8drv_frame_check folds position in (4: its values change); 4009: vp8hip_set_loop_filter_type and vp8drv_config.loop_filter_type;
 * 4010: quality statistics (vp8hip_set_quality_stats, vp8hip_batch_quality, vp8drv_config.quality_stats, vp8drv_get_frame_quality);
 * also under 4010: vp8hip_set_source_scaling, vp8host_scale_taps and vp8drv_config.in_width / in_height / scale_filter, in front of
 * quality_stats, which stays the last field (a host fills the struct with vp8drv_default_config, which zeroes them: no scaling);
 * also under 4010: vp8hip_set_denoise, vp8hip_denoise_restart, vp8hip_denoise_result, vp8host_denoise_frame, vp8drv_set_denoise and
 * vp8drv_get_denoise_stats (entry points only: vp8drv_config is unchanged);
 * also under 4010: the deinterlacer (vp8hip_set_deinterlace, vp8hip_deinterlace_restart, vp8hip_deinterlace_result,
 * vp8host_deinterlace_frame, vp8host_y4m_interlace, vp8drv_set_deinterlace, vp8drv_get_deinterlace_stats; entry points only:
 * vp8drv_config is unchanged);
 * also under 4010: source formats (vp8hip_set_source_format, vp8drv_set_source_format, vp8host_source_plane_bytes, vp8host_convert_frame,
 * vp8host_y4m_colourspace; entry points only: vp8drv_config is unchanged);
 * also under 4010: the packed source formats YUY2, UYVY, BGRA, RGBA and their colour matrix (vp8hip_set_source_colour,
 * vp8drv_set_source_colour, vp8host_convert_frame_colour, vp8host_colour_coefficients; entry points only);
 * also under 4010: frame analysis (vp8hip_set_analysis, vp8hip_analysis_restart, vp8hip_analysis_result, vp8host_analyse_luma,
 * vp8drv_set_analysis, vp8drv_get_frame_analysis) and vp8drv_set_quantizer / vp8drv_get_quantizer (entry points only);
 * also under 4010: source windows and orientation (vp8hip_set_source_window, vp8hip_set_source_orientation, vp8host_source_window,
 * vp8host_window_frame, vp8host_orient_frame, vp8drv_set_source_window, vp8drv_set_source_orientation; entry points only:
 * vp8drv_config is unchanged);
 * also under 4010: the per-macroblock quantiser (vp8hip_set_segment_mode, vp8hip_segment_mode, vp8hip_set_segment_map_device,
 * vp8hip_upload_segment_map, vp8hip_download_segment_map, vp8host_aq_segment_map, vp8host_aq_segment, vp8drv_set_segment_mode, vp8drv_set_segment_map;
 * entry points only: vp8drv_config is unchanged);
 * also under 4010: hidden alternate reference frames (vp8hip_arf_filter_device, vp8hip_arf_filter_host, vp8hip_arf_result,
 * vp8hip_arf_release, vp8hip_loop_filter_hidden, vp8host_arf_filter_frame, vp8host_arf_round_divide, vp8drv_set_arf,
 * vp8drv_encode_arf_device, vp8drv_encode_arf_host, vp8drv_get_arf_stats; entry points only, and the value VP8HIP_ALTREF_HIDDEN of
 * the existing is_altref fields: vp8drv_config, vp8drv_stats, vp8hip_header_params and vp8bs_frame keep their layout);
 * also under 4010: HDR tone mapping (vp8hip_set_source_transfer, vp8drv_set_source_transfer, vp8host_tonemap_tables,
 * vp8host_tonemap_frame; entry points only: vp8drv_config is unchanged);
 * also under 4010: overlays (vp8hip_set_overlay_host, vp8hip_set_overlay_device, vp8hip_set_overlay_placement, vp8hip_clear_overlay,
 * vp8hip_overlay_count, vp8host_overlay_frame, vp8drv_set_overlay_host, vp8drv_set_overlay_device, vp8drv_set_overlay_placement,
 * vp8drv_clear_overlay; entry points only: vp8drv_config is unchanged);
 * also under 4010: canvases (vp8hip_set_canvas, vp8hip_canvas_tiles, vp8hip_compose_current_device, vp8hip_compose_current_host,
 * vp8host_tile_valid, vp8host_compose_frame, vp8drv_set_canvas, vp8drv_encode_frame_tiles_device, vp8drv_encode_frame_tiles_host;
 * entry points and the types vp8hip_tile and vp8hip_tile_planes only: vp8drv_config is unchanged);
 * also under 4010: temporal layers (vp8host_temporal_step, vp8hip_loop_filter_refresh, vp8drv_set_temporal_layers,
 * vp8drv_get_frame_layer; entry points, the type vp8drv_layer_info and the values VP8HIP_GOLDEN_ONLY and VP8HIP_REFRESH_NOTHING of
 * the existing is_golden fields only: vp8drv_config, vp8drv_stats, vp8hip_header_params and vp8bs_frame keep their layout);
 * also under 4010: cyclic intra refresh (vp8host_intra_refresh_forced, vp8host_intra_refresh_count, vp8hip_intra_refresh,
 * vp8drv_set_intra_refresh, vp8drv_get_intra_refresh; entry points and the type vp8drv_intra_refresh_info only: vp8drv_config and
 * vp8drv_stats keep their layout). */
#define VP8HIP_ABI_VERSION 4010
int vp8hip_abi_version(void);
/* 1 if this build of the library honours the timing-experiment switches that leave work out of a launch or a wait
 * (VP8HIP_EXPERIMENT_SKIP, VP8HIP_EXPERIMENT_SKIP_ENT, VP8HIP_EXPERIMENT_NOWAIT, VP8DRV_EXPERIMENT_READY_FIRST; built with
 * -DVP8HIP_EXPERIMENTS, results are then garbage on purpose); 0 for the shipped build, in which they are constants and no
 * environment can take work out of a run.  bench.py refuses to print a line from a build that answers 1. */
int vp8hip_experiments_compiled_in(void);
/* the head-of-frame stream mode of batches in force in this process: 0 none (default), 1 per batch, 2 one for all (VP8HIP_BATCH_PREP) */
int vp8hip_batch_prep_mode(void);

/* ---- device memory for a caller that has none of its own ---------------------------------------------------------------
 * vp8hip_set_current_device / vp8hip_set_last_device / the batched forms take planes that are already in this device's memory.
 * A host that is not a GPU program itself (the reference's main(), bench.py, the tests) gets such memory here, so that the process
 * needs no second GPU runtime beside the one this library was built for (PyTorch ships its own copy of the HIP runtime; both in
 * one process was where a one-in-twenty teardown crash of round 3 lived).  Plain hipMalloc / hipMemcpy / hipDeviceSynchronize
 * on device_ordinal; the copies block. */
int vp8hip_device_count(void);
int vp8hip_device_alloc(int device_ordinal, size_t bytes, void **out);
int vp8hip_device_free(int device_ordinal, void *p);
int vp8hip_device_upload(int device_ordinal, void *dst, const void *src, size_t bytes);
int vp8hip_device_download(int device_ordinal, void *dst, const void *src, size_t bytes);
int vp8hip_device_synchronize(int device_ordinal);
/* page-locked host memory (hipHostMalloc): source planes handed to vp8hip_prefetch_current / vp8hip_batch_upload_current / _prefetch_current from it
 * are copied asynchronously (vp8hip_upload_current itself returns when its copy is done, whatever the memory) */
int vp8hip_host_alloc(int device_ordinal, size_t bytes, void **out);
int vp8hip_host_free(int device_ordinal, void *p);
int vp8hip_device_mem_info(int device_ordinal, size_t *free_bytes, size_t *total_bytes);
/* "dddd:bb:dd.f" of the device (for pinning the host threads to its NUMA node); len >= 16 */
int vp8hip_device_pci_bus_id(int device_ordinal, char *out, int len);
/* version of the HIP runtime this process's library calls land in (hipRuntimeGetVersion), e.g. 70226015 */
int vp8hip_runtime_version(void);


#ifdef __cplusplus
}
#endif

/* the rest of the ABI, in headers of their own (they include this one): several contexts at a time, and the measurement taps */
#include "vp8hip_multi.h"
#include "vp8hip_taps.h"

#endif
