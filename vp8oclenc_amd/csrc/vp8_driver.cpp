// vp8_driver.cpp -- the reference's frame loop (main(), src/vp8enc.cpp:351-488), native host code over the C ABI
// (include/vp8hip_driver.h).  No GPU code here: it only sequences vp8hip_* calls with the parameters the host
// mirror (vp8_host.cpp) or the device (vp8hip_auto_segments) produces.
#include <stdlib.h>

#include <new>
#include <chrono>
#include <string.h>
#include <thread>
#include <vector>

#include "../../include/vp8hip_bitstream.h"
#include "../../include/vp8hip_driver.h"
#include "../../include/vp8hip_host.h"
#include "driver_settings.h"

struct vp8drv {
    vp8hip_ctx *hip = nullptr;
    vp8drv_config cfg{};
    int W = 0, H = 0, mbs = 0;
    vp8host_gop gop{};
    vp8host_scene_state scene{};     // scene_change()'s hold-over and frames.last_key_detect
    int32_t lastqi[4]{}, altrefqi[4]{};
    int qi_min = 0;
    vp8drv_stats st{};
    // what vp8drv_get_frame needs to know about the frame just coded
    bool have_frame = false, last_key = false, last_altref = false, checked = false;
    int sharpness = VP8HIP_SHARPNESS_ON_DEVICE;   // video.loop_filter_sharpness in force, or: still on the device (vp8hip_get_segments).  May be NEGATIVE (vp8hip.h)
    int replaced = 0;
    bool verdict_pending = false;    // check_SSIM's verdict on the frame just coded is still on its way (resolve())
    const uint8_t *staged = nullptr; // vp8drv_stage_frame_host: these planes are the context's current frame already (and, with scene_detect, their scan is under way)
    bool staged_scan = false;
    vp8::DriverSettings s;           // the settings in force: what every refusal reads (driver_settings.h)
    // last_hidden: the frame just coded is a hidden one.  rotation_consumed: a hidden frame's transform has applied the reference rotation
    // the last shown frame owed; the next shown frame's must not apply it again.  hidden_altref: ALTREF holds a hidden frame's
    // reconstruction (until a key frame or a scheduled shown alt-ref rotates LAST into it).
    bool last_hidden = false, rotation_consumed = false, hidden_altref = false;
    vp8drv_arf_stats arf_st{};
    // temporal layers: the rule's p of the next frame (shown frames since the last key frame as finally coded), tid-0 frames made final,
    // the frame just coded
    int tl_p = 0, tl0_count = 0;
    vp8drv_layer_info layer{};
    // intra refresh: the rule's q of the next inter frame that refreshes LAST (it advances whether or not a period is set), the forced
    // macroblocks of the frame just coded, the record
    int ir_q = 0, ir_forced = 0;
    vp8drv_intra_refresh_info ir{};
    // read-back buffers of vp8drv_get_frame
    std::vector<int32_t> seg, nz, ref, parts, is_inter, modes;
    std::vector<int16_t> vectors;
    std::vector<uint8_t> partitions;
};

extern "C" {

void vp8drv_default_config(vp8drv_config *c) {
    if (!c) return;
    c->gop_size = 150;
    c->altref_range = 5;
    c->qi_min = 0;
    c->qi_max = 48;
    c->ssim_target = -1.0f;
    c->device_params = 1;
    c->check_ssim = 1;
    c->num_partitions = 1;
    c->display_width = 0;
    c->display_height = 0;
    c->host_bitstream = 0;
    c->overlap_filter = 0;
    c->ref_mask = 3;
    c->conformant_stream = 0;
    c->scene_detect = 0;
    c->src_width = c->src_height = 0;
    c->loop_filter_type = 0;
    c->in_width = c->in_height = c->scale_filter = 0;
    c->quality_stats = 0;
}

int vp8drv_create(vp8drv **out, int width, int height, int device_ordinal, const vp8drv_config *cfg) {
    if (!out || !cfg) return VP8HIP_ERR_ARG;
    *out = nullptr;
    if (cfg->loop_filter_type != 0 && cfg->loop_filter_type != 1) return VP8HIP_ERR_ARG;
    if (cfg->quality_stats != 0 && cfg->quality_stats != 1) return VP8HIP_ERR_ARG;
    vp8drv *d = new (std::nothrow) vp8drv();
    if (!d) return VP8HIP_ERR_ARG;
    d->cfg = *cfg;
    const int rc = vp8hip_create(&d->hip, width, height, cfg->ssim_target, device_ordinal);
    if (rc != VP8HIP_OK) {
        delete d;
        return rc;
    }
    if (cfg->loop_filter_type) {
        const int rc = vp8hip_set_loop_filter_type(d->hip, cfg->loop_filter_type);
        if (rc != VP8HIP_OK) {
            vp8hip_destroy(d->hip);
            delete d;
            return rc;
        }
    }
    if (cfg->quality_stats) {
        const int rc = vp8hip_set_quality_stats(d->hip, 1);
        if (rc != VP8HIP_OK) {
            vp8hip_destroy(d->hip);
            delete d;
            return rc;
        }
    }
    if (cfg->overlap_filter) vp8hip_filter_overlap(d->hip, 1);
    if (cfg->conformant_stream) vp8hip_conformant_stream(d->hip, 1);
    if (cfg->src_width || cfg->src_height || cfg->in_width || cfg->in_height) {
        // the size the frames are scaled to (or come in at): video.dst_width/height
        const int dw = cfg->src_width ? cfg->src_width : width, dh = cfg->src_height ? cfg->src_height : height;
        int rc = VP8HIP_ERR_ARG;
        if (cfg->device_params && (cfg->in_width || cfg->in_height) && cfg->in_width > 0 && cfg->in_height > 0)
            rc = vp8hip_set_source_scaling(d->hip, cfg->in_width, cfg->in_height, dw, dh, cfg->scale_filter);
        else if (cfg->device_params && !cfg->in_width && !cfg->in_height)
            rc = vp8hip_set_source_size(d->hip, cfg->src_width, cfg->src_height);
        if (rc != VP8HIP_OK) {
            vp8hip_destroy(d->hip);
            delete d;
            return rc;
        }
        if (!d->cfg.display_width) d->cfg.display_width = cfg->src_width;       // (0 = the coded size)
        if (!d->cfg.display_height) d->cfg.display_height = cfg->src_height;
    }
    d->W = width;
    d->H = height;
    d->mbs = (width / 16) * (height / 16);
    vp8host_gop_init(&d->gop, cfg->gop_size, cfg->altref_range);
    vp8host_quantizer_ladders(cfg->qi_min, cfg->qi_max, d->lastqi, d->altrefqi);
    d->qi_min = cfg->qi_min < cfg->qi_max ? cfg->qi_min : cfg->qi_max;
    vp8::DriverSettings &s = d->s;
    s.device_params = cfg->device_params != 0;
    s.overlap_filter = cfg->overlap_filter != 0;
    s.scene_detect = cfg->scene_detect != 0;
    s.quality_stats = cfg->quality_stats != 0;
    s.ssim_target = cfg->ssim_target > -1.0f;
    s.scheduled_altref = cfg->altref_range <= cfg->gop_size;
    s.qi_min = cfg->qi_min;
    s.qi_max = cfg->qi_max;
    s.num_partitions = cfg->num_partitions;
    s.check_ssim = cfg->check_ssim != 0;
    s.loop_filter_type = cfg->loop_filter_type;
    s.in_width = cfg->in_width;
    s.in_height = cfg->in_height;
    s.scale_filter = cfg->in_width ? cfg->scale_filter : 0;
    *out = d;
    return VP8HIP_OK;
}

void vp8drv_destroy(vp8drv *d) {
    if (!d) return;
    vp8hip_destroy(d->hip);
    delete d;
}

vp8hip_ctx *vp8drv_context(vp8drv *d) { return d ? d->hip : nullptr; }

void vp8drv_get_stats(const vp8drv *d, vp8drv_stats *s) {
    if (d && s) *s = d->st;
}

}  // extern "C"

namespace {

#define DRV_CHK(call)                     \
    do {                                  \
        const int rc_ = (call);           \
        if (rc_ != VP8HIP_OK) return rc_; \
    } while (0)

using vp8::refusal;

// the settings with what moves by itself filled in: what refusal() and operator== are asked about
vp8::DriverSettings settings(const vp8drv *d) {
    vp8::DriverSettings s = d->s;
    s.hidden_shapes_refs = d->rotation_consumed || d->hidden_altref;
    s.shard = vp8hip_shard_world(d->hip) > 0;
    s.overlays = vp8hip_overlay_count(d->hip) > 0;
    vp8hip_segment_mode(d->hip, &s.seg_mode, &s.seg_strength);
    return s;
}

// planes handed over early under other settings are not these settings' frame
void drop_staged(vp8drv *d) {
    d->staged = nullptr;
    d->staged_scan = false;
}

// segment data of the current frame: on the device, or from the host mirror on the caller's luma plane
int segments(vp8drv *d, const uint8_t *host_y, bool key, const int32_t *refqi) {
    d->sharpness = VP8HIP_SHARPNESS_ON_DEVICE;
    if (d->cfg.device_params || !host_y) return vp8hip_auto_segments(d->hip, key ? 1 : 0, refqi, d->qi_min);
    int32_t red = 0, sharp = 0, sd[VP8HIP_SD_INTS];
    vp8host_loopfilter_strength(host_y, d->W, d->H, &red, &sharp);
    vp8host_prepare_segments_data(key ? 1 : 0, refqi, d->qi_min, red, sharp, 0, 0, sd);
    d->sharpness = sharp;
    return vp8hip_set_segments(d->hip, sd);
}

// vp8drv_get_frame_layer's record once the frame is final: a tid-0 frame takes the next index, the others carry their base frame's
void layer_final(vp8drv *d) {
    if (d->layer.temporal_id == 0) ++d->tl0_count;
    d->layer.tl0_pic_idx = (d->tl0_count - 1) & 255;
}

// a key frame is p = 0 of the temporal pattern, whoever asked for it: the pattern restarts, and a layer count asked for takes force
void key_layer_record(vp8drv *d) {
    d->s.tl_layers = d->s.tl_next;
    d->tl_p = 1;
    d->layer = vp8drv_layer_info{0, 0, 0, VP8HOST_REFRESH_ALL, 0, 1};
    layer_final(d);
    d->ir_q = d->ir_forced = 0;      // ... and so does the intra refresh's phase; a key frame forces nothing
    d->ir.last_q = d->ir.last_forced = 0;
}

// the key frame just coded and filtered is final: GOP state, counters and the record of the frame just coded
void key_frame_final(vp8drv *d) {
    d->scene.last_key_detect = d->gop.frame_number;       // intra_part.h:1093, for every key frame whoever asked for it
    vp8host_gop_key_coded(&d->gop);
    vp8host_gop_frame_done(&d->gop);
    d->st.key_frames++;
    d->st.frame_number = d->gop.frame_number;
    d->have_frame = true;
    d->last_key = d->last_altref = true;
    // (LAST = GOLDEN = ALTREF = this frame, by the rotation it owes.  For a member of a batch a no-op: batch membership refuses a driver
    // whose references a hidden frame shapes, and a member codes no hidden frame)
    d->last_hidden = d->rotation_consumed = d->hidden_altref = false;
    d->checked = false;
    d->replaced = 0;
    key_layer_record(d);
}

// prepare_segments_data() + intra_transform() (vp8enc.cpp:379-383, :411-414, :446-450) and the common tail
// (:472-473): filter mask, loop filter.  The filtered key frame is LAST = GOLDEN = ALTREF (intra_part.h:1091-1098).
int key_frame(vp8drv *d, const uint8_t *host_y) {
    DRV_CHK(segments(d, host_y, true, d->altrefqi));
    DRV_CHK(vp8hip_intra_transform(d->hip));
    DRV_CHK(vp8hip_prepare_filter_mask(d->hip, nullptr));
    DRV_CHK(vp8hip_loop_filter(d->hip));
    key_frame_final(d);
    return 1;
}

// the inter frame just coded, shown or hidden: what vp8drv_get_frame needs to know about it
void inter_frame_coded(vp8drv *d, bool altref, bool hidden) {
    d->have_frame = true;
    d->last_key = false;
    d->last_altref = altref;
    d->last_hidden = hidden;
    d->checked = false;
    d->replaced = 0;
}

// ... and a shown one's references, for vp8drv_get_stats
void shown_inter_coded(vp8drv *d, int use_golden, int use_altref, int prev_is_golden, int prev_is_altref, int was_altref) {
    d->st.last_use_golden = use_golden;
    d->st.last_use_altref = use_altref;
    d->st.refs_searched += 1 + use_golden + use_altref;
    d->st.last_prev_is_golden = prev_is_golden;
    d->st.last_prev_is_altref = prev_is_altref;
    d->st.last_was_altref = was_altref;
    inter_frame_coded(d, was_altref != 0, false);
}

// the inter frame just coded is final: the counters of main()'s loop tail
void inter_frame_done(vp8drv *d) {
    vp8host_gop_frame_done(&d->gop);
    d->st.inter_frames++;
    d->st.frame_number = d->gop.frame_number;
    d->tl_p++;
    if (d->layer.refresh == VP8HOST_REFRESH_LAST) d->ir_q++;      // the intra refresh's phase counts the frames that refreshed LAST
    layer_final(d);
}

// The verdict of the asynchronous check_SSIM on the frame just coded (vp8enc.cpp:442-453): statistics, and -- when more than a
// sixth of the macroblocks were replaced or the frame's SSIM is below the target -- the frame again as a key frame, on the
// current frame the context still holds.  (The inter version's loop filter has run by then: its output is simply never used.)
// Returns 1 if the frame ended as a key frame, 0 if not, < 0 = vp8hip_status.
int resolve(vp8drv *d) {
    if (!d->verdict_pending) return 0;
    d->verdict_pending = false;
    int32_t replaced = 0, updated = 0;
    float new_ssim = 0.0f, min1 = 2.0f;
    DRV_CHK(vp8hip_check_ssim_result(d->hip, &replaced, &new_ssim, &min1, &updated));
    d->st.last_replaced = replaced;
    d->st.last_new_ssim = new_ssim;
    d->st.last_min_ssim = min1;
    // e_data.is_inter_mb / mode travel to the header coder only when something was replaced: with nothing below the target the
    // fallback's launch left at once and did not even initialise them (all macroblocks inter: the same bits without them)
    // ... or when the frame carries forced intra macroblocks (vp8drv_set_intra_refresh: replaced is then 0, the target being -1)
    d->checked = replaced > 0 || d->ir_forced > 0;
    d->replaced = replaced > 0 ? replaced : d->ir_forced;
    if (updated) d->sharpness = 7;      // prepare_segments_data(1, 7), :260-261, happened on the device
    if (replaced > d->mbs / 6 || new_ssim < d->cfg.ssim_target) {
        d->st.redone_as_key++;
        return key_frame(d, nullptr);
    }
    inter_frame_done(d);
    return 0;
}

// the loop body once the current frame is on the device; host_y: the caller's luma plane or nullptr
int frame_body(vp8drv *d, const uint8_t *host_y, bool key) {
    const bool scan_under_way = d->staged_scan;
    d->staged_scan = false;
    if (!key && d->cfg.scene_detect) {     // vp8enc.cpp:408-416: only frames that would be inter frames are looked at
        int32_t Udiff = 0, Vdiff = 0;
        if (scan_under_way) DRV_CHK(vp8hip_chroma_change_result(d->hip, &Udiff, &Vdiff));     // (started when the frame was handed over early)
        else DRV_CHK(vp8hip_chroma_change(d->hip, &Udiff, &Vdiff));
        if (vp8host_scene_change(&d->scene, Udiff, Vdiff, d->gop.frame_number)) {
            d->st.scene_changes++;
            key = true;
        }
    }
    if (key) return key_frame(d, host_y);
    // vp8enc.cpp:390, 419: loop-filter strength of the current frame -> segment data
    // vp8drv_set_temporal_layers: references, ending and quantiser ladder from the rule in the place of the GOP state's flags
    const bool layered = d->s.tl_layers > 1;
    vp8host_temporal tl{0, 0, VP8HOST_REFRESH_LAST, 0};
    if (layered && vp8host_temporal_step(d->s.tl_layers, d->tl_p, d->cfg.ref_mask, &tl)) return VP8HIP_ERR_STATE;
    const int32_t *refqi = (d->gop.current_is_altref && !layered) ? d->altrefqi : d->lastqi;   // vp8enc.cpp:149-151
    DRV_CHK(segments(d, host_y, false, refqi));
    int32_t use_golden = 0, use_altref = 0;
    vp8host_gop_inter_flags(&d->gop, &use_golden, &use_altref);                  // inter_part.h:103-104
    if (layered) {
        use_golden = tl.use_golden;
        use_altref = 0;
    }
    // vp8drv_encode_arf_*: a hidden frame's transform has applied the rotation already (again, and LAST would overwrite the new
    // ALTREF); and while ALTREF holds a hidden frame's reconstruction it differs from GOLDEN whatever the frame numbers say
    const int32_t prev_is_golden = d->rotation_consumed ? 0 : d->gop.prev_is_golden, prev_is_altref = d->rotation_consumed ? 0 : d->gop.prev_is_altref;
    if (prev_is_altref) d->hidden_altref = false;
    if (d->hidden_altref) use_altref = 1;
    d->rotation_consumed = false;
    use_golden &= d->cfg.ref_mask & 1;
    use_altref &= (d->cfg.ref_mask >> 1) & 1;
    DRV_CHK(vp8hip_inter_transform(d->hip, prev_is_golden, prev_is_altref, use_golden, use_altref));
    shown_inter_coded(d, use_golden, use_altref, prev_is_golden, prev_is_altref, layered ? 0 : d->gop.current_is_altref);
    // vp8drv_set_intra_refresh: the forced macroblocks of a frame that refreshes LAST, behind the transform; the header then takes the
    // intra information (from either first-partition coder: the host coder's prob_intra is made of d->replaced)
    d->ir_forced = 0;
    d->ir.last_q = d->ir_q;
    if (d->s.ir_period && tl.refresh == VP8HOST_REFRESH_LAST) {
        d->ir_forced = vp8host_intra_refresh_count(d->W / 16, d->H / 16, d->s.ir_period, d->ir_q);
        if (d->ir_forced > 0) {
            DRV_CHK(vp8hip_intra_refresh(d->hip, d->s.ir_period, d->ir_q));
            d->checked = true;
            d->replaced = d->ir_forced;
            d->ir.total_forced += d->ir_forced;
        }
    }
    d->ir.last_forced = d->ir_forced;
    // an unreferenced frame is filtered only if something reads the filter's output or rides in its launch
    const bool filter = tl.refresh != VP8HOST_REFRESH_NONE || d->cfg.check_ssim || d->cfg.quality_stats || d->s.analysis || (d->s.tl_flags & VP8DRV_TL_KEEP_RECON);
    d->layer = vp8drv_layer_info{tl.temporal_id, 0, tl.layer_sync, tl.refresh, use_golden, filter ? 1 : 0};
    if (d->cfg.check_ssim && (d->cfg.device_params || !host_y)) {
        // check_SSIM (vp8enc.cpp:231-263) with nobody waiting for it: fallback, statistics and the filter update on the device,
        // the loop filter right behind them.  What the host has to decide -- "redo as key frame", :443-453 -- it decides when it
        // next needs to know: at the start of the next call or in vp8drv_get_frame (resolve()).
        DRV_CHK(vp8hip_check_ssim_async(d->hip, refqi, d->qi_min));
        DRV_CHK(vp8hip_loop_filter_refresh(d->hip, tl.refresh, 1));
        d->verdict_pending = true;
        return 0;
    }
    if (d->cfg.check_ssim) {
        // the same with the host in the middle (host parameter mirror: the reference's own sequence of calls)
        int32_t replaced = 0;
        float new_ssim = 0.0f, min1 = 2.0f;
        DRV_CHK(vp8hip_check_ssim(d->hip, &replaced, &new_ssim, &min1));
        d->st.last_replaced = replaced;
        d->st.last_new_ssim = new_ssim;
        d->st.last_min_ssim = min1;
        d->checked = true;
        d->replaced = replaced;
        if (min1 > 0.95f) {
            // even the worst macroblock is good: weaken the loop filter (reductor * 2, sharpness 7; :155-159, :260-261)
            int32_t red = 0, sharp = 0, sd[VP8HIP_SD_INTS];
            if (d->cfg.device_params || !host_y) DRV_CHK(vp8hip_get_segments(d->hip, sd, &red, &sharp));
            else vp8host_loopfilter_strength(host_y, d->W, d->H, &red, &sharp);
            vp8host_prepare_segments_data(0, refqi, d->qi_min, red, sharp, 1, 7, sd);
            DRV_CHK(vp8hip_set_segments(d->hip, sd));
            d->sharpness = 7;
        }
        if (replaced > d->mbs / 6 || new_ssim < d->cfg.ssim_target) {   // vp8enc.cpp:443-453: redo as a key frame
            d->st.redone_as_key++;
            return key_frame(d, host_y);
        }
        // the fallback changed coefficients: mask and non-zero counts again (loop_filter.h:25-55)
        if (replaced > 0) DRV_CHK(vp8hip_prepare_filter_mask(d->hip, nullptr));
    }
    // otherwise prepare_filter_mask was produced by vp8hip_inter_transform for its own coefficients;
    // do_loop_filter (loop_filter.h:185-190) follows directly
    DRV_CHK(vp8hip_loop_filter_refresh(d->hip, tl.refresh, filter ? 1 : 0));
    inter_frame_done(d);
    return 0;
}

// entropy_encode() + gather_frame() (vp8enc.cpp:48-94, 476-481; encIO.h:1-30) for the frame just coded:
// coefficient statistics and partitions on the device, first partition on the host
int layer_is_golden(const vp8drv *d) {
    if (d->last_key || d->last_hidden) return d->last_key;
    return d->layer.refresh == VP8HOST_REFRESH_GOLDEN ? VP8HIP_GOLDEN_ONLY : (d->layer.refresh == VP8HOST_REFRESH_NONE ? VP8HIP_REFRESH_NOTHING : 0);
}

vp8hip_header_params header_params(const vp8drv *d) {
    vp8hip_header_params hp{};
    hp.is_key = d->last_key;
    hp.is_golden = layer_is_golden(d);          // current_is_golden_frame = current_is_key_frame (vp8enc.cpp:369), or a temporal layer's refresh
    hp.is_altref = d->last_hidden ? VP8HIP_ALTREF_HIDDEN : d->last_altref;
    hp.loop_filter_type = d->cfg.loop_filter_type;   // 0 in the reference (init.h:1583)
    hp.loop_filter_sharpness = d->sharpness;    // or VP8HIP_SHARPNESS_ON_DEVICE
    hp.width = d->cfg.display_width;
    hp.height = d->cfg.display_height;
    hp.use_intra_info = d->checked;
    return hp;
}

// vp8drv_set_denoise: the history restarts where the GOP schedule starts a GOP -- the frame about to be taken in is a scheduled key
// frame -- so that a closed GOP coded as a chunk of its own sees the frames the serial program sees.  force_key, scene cuts and
// frames sent back by check_SSIM are not the schedule's.
// vp8drv_set_analysis: its history restarts at the same frames, for the same reason.
int intake_restarts(vp8drv *d, bool scheduled_key) {
    if (d->s.analysis && scheduled_key) {
        const int rc = vp8hip_analysis_restart(d->hip);
        if (rc != VP8HIP_OK) return rc;
    }
    if (d->s.deinterlace && scheduled_key) {      // vp8drv_set_deinterlace: and so does its history
        const int rc = vp8hip_deinterlace_restart(d->hip);
        if (rc != VP8HIP_OK) return rc;
    }
    if (d->s.denoise && scheduled_key) return vp8hip_denoise_restart(d->hip);
    return VP8HIP_OK;
}

// a driver with temporal layers whose context has since joined a by-reference split (the context's refresh ending would refuse it in
// the middle of the frame): refused before the frame is taken in
// ... and so is a driver with an intra refresh period (vp8hip_intra_refresh would refuse behind the transform)
bool layers_refused(const vp8drv *d) {
    const vp8::DriverSettings s = settings(d);
    if (layered(s) && refusal(s, vp8::LAYERS)) return true;
    return s.ir_period && refusal(s, vp8::INTRA_REFRESH);
}

// a setter's way in: the table's word on the feature, then the open check_SSIM verdict (a frame sent back is coded again under the
// settings it was coded under)
int ask(vp8drv *d, vp8::Feature f, bool on = true) {
    DRV_CHK(refusal(settings(d), f, on));
    const int rc = resolve(d);
    return rc < 0 ? rc : VP8HIP_OK;
}

// The shape the intake setters share: the arguments, the table, the open verdict, the context's setter (which judges the value against
// the other intake settings); restage: planes handed over early under the other setting are not this setting's frame.  The caller
// records the value behind it.
template <class Set> int intake_setter(vp8drv *d, bool args_ok, bool restage, Set set) {
    if (!d || !args_ok) return VP8HIP_ERR_ARG;
    DRV_CHK(ask(d, vp8::INTAKE_SETTER));
    DRV_CHK(set());
    if (restage) drop_staged(d);
    return VP8HIP_OK;
}

int get_frame(vp8drv *d, uint8_t *out, size_t capacity, size_t *size) {
    const int P = d->cfg.num_partitions;
    const size_t n = (size_t)d->mbs;
    const vp8hip_header_params hp = header_params(d);
    if (!d->cfg.host_bitstream) return vp8hip_encode_frame(d->hip, P, &hp, out, capacity, size);      // the whole entropy stage on the device, one read-back
    uint32_t probs[VP8BS_NUM_COEFF_PROBS], denom[VP8BS_NUM_COEFF_PROBS];
    d->nz.resize(n);
    DRV_CHK(vp8hip_prepare_filter_mask(d->hip, d->nz.data()));                   // counts of the final coefficients (vp8enc.cpp:472)
    DRV_CHK(vp8hip_count_probs(d->hip, P, probs, denom));                        // :58-68
    vp8bs_default_probs(probs, denom);                                           // :69-76
    // four times video.partition_step (init.h:409,1190): a partition that outgrows the reference's buffer overruns it
    // there; found by the randomised parity run with noise at a low quantizer on a frame of two macroblock rows
    const size_t step = n * 3200 / (size_t)P + 4096;
    d->partitions.resize(step * (size_t)P);
    int32_t sizes[8] = {0};
    DRV_CHK(vp8hip_encode_coefficients(d->hip, probs, P, (int)step, d->partitions.data(), sizes));   // :77-81
    // what encode_header reads from the frame's results (entropy_host.cpp:221-223, 808, 986-987, 1086)
    d->seg.resize(n);
    d->ref.resize(n);
    d->parts.resize(n);
    d->vectors.resize(n * 8);
    vp8hip_results r{};
    r.MB_segment_id = d->seg.data();
    if (!d->last_key) {
        r.MB_reference_frame = d->ref.data();
        r.MB_parts = d->parts.data();
        r.MB_vectors = d->vectors.data();
    }
    DRV_CHK(vp8hip_download_results(d->hip, &r));
    const bool intra_info = d->last_key || d->checked;
    if (intra_info) {
        d->modes.resize(n * 16);
        d->is_inter.resize(n);
        DRV_CHK(vp8hip_download_intra(d->hip, d->modes.data(), d->last_key ? nullptr : d->is_inter.data()));
    }
    int32_t sd[VP8HIP_SD_INTS], red = 0, sharp = 0;
    DRV_CHK(vp8hip_get_segments(d->hip, sd, &red, &sharp));
    if (d->sharpness != VP8HIP_SHARPNESS_ON_DEVICE) sharp = d->sharpness;
    vp8bs_frame f{};
    f.width = d->cfg.display_width > 0 ? d->cfg.display_width : d->W;
    f.height = d->cfg.display_height > 0 ? d->cfg.display_height : d->H;
    f.mb_width = d->W / 16;
    f.mb_height = d->H / 16;
    f.is_key = hp.is_key;
    f.is_golden = hp.is_golden;
    f.is_altref = hp.is_altref;
    f.loop_filter_type = hp.loop_filter_type;
    f.loop_filter_sharpness = sharp;
    f.partitions_log2 = P == 8 ? 3 : (P == 4 ? 2 : (P == 2 ? 1 : 0));
    f.skip_prob = vp8host_skip_prob(d->nz.data(), d->mbs);
    f.replaced = d->last_key ? 0 : d->replaced;
    f.segments = sd;
    f.MB_segment_id = d->seg.data();
    f.MB_non_zero_coeffs = d->nz.data();
    f.MB_reference_frame = d->last_key ? nullptr : d->ref.data();
    f.MB_parts = d->last_key ? nullptr : d->parts.data();
    f.MB_vectors = d->last_key ? nullptr : d->vectors.data();
    f.is_inter_mb = (!d->last_key && d->checked) ? d->is_inter.data() : nullptr;
    f.modes = intra_info ? d->modes.data() : nullptr;
    f.new_probs = probs;
    f.new_probs_denom = denom;
    const size_t head = vp8bs_encode_header(&f, out, capacity, nullptr);          // :84
    if (head == (size_t)-1) return VP8HIP_ERR_FORMAT;   // 19-bit size field of the frame tag
    if (!head) return VP8HIP_ERR_OVERFLOW;
    const size_t total = vp8bs_gather_frame(out, head, capacity, P, d->partitions.data(), step, sizes);
    if (!total) return VP8HIP_ERR_OVERFLOW;
    *size = total;
    return VP8HIP_OK;
}

}  // namespace

extern "C" {

int vp8drv_encode_frame_device(vp8drv *d, const void *y, const void *u, const void *v, int force_key) {
    if (!d || !y || !u || !v) return VP8HIP_ERR_ARG;
    if (d->s.canvas) return VP8HIP_ERR_STATE;      // (frames come in through vp8drv_encode_frame_tiles_*)
    if (layers_refused(d)) return VP8HIP_ERR_STATE;
    { const int rc = resolve(d); if (rc < 0) return rc; }                        // the previous frame's check_SSIM verdict, if still open
    vp8host_gop_next(&d->gop);
    DRV_CHK(intake_restarts(d, d->gop.current_is_key != 0));
    DRV_CHK(vp8hip_set_current_device(d->hip, y, u, v));                          // vp8enc.cpp:386-388
    return frame_body(d, nullptr, d->gop.current_is_key || force_key);
}

int vp8drv_encode_frame_host(vp8drv *d, const uint8_t *y, const uint8_t *u, const uint8_t *v, int force_key) {
    if (!d || !y || !u || !v) return VP8HIP_ERR_ARG;
    if (d->s.canvas || layers_refused(d)) return VP8HIP_ERR_STATE;
    { const int rc = resolve(d); if (rc < 0) return rc; }
    vp8host_gop_next(&d->gop);
    const bool staged = d->staged == y;
    d->staged = nullptr;
    if (!staged) {
        d->staged_scan = false;
        DRV_CHK(intake_restarts(d, d->gop.current_is_key != 0));      // (a prefetched frame is packed, and denoised, in this upload)
        DRV_CHK(vp8hip_upload_current(d->hip, y, u, v));
    }
    return frame_body(d, y, d->gop.current_is_key || force_key);
}

// The NEXT frame handed to the device early -- while the frame just coded is in its loop filter -- so that the next
// vp8drv_encode_frame_host, given the same planes, finds the frame there and (with cfg.scene_detect) scene_change()'s two sums on their
// way or back: its side work (parameter scan, pyramid, GOLDEN / ALTREF searches) is then enqueued early enough to run beside the filter.
// Takes the open verdict first (the frame it belongs to must not lose its place as the context's current frame before a "redo as key
// frame").  Call it after vp8drv_get_frame_begin / vp8drv_resolve of the frame just coded; the planes stay unchanged until the
// vp8drv_encode_frame_host that names them has returned.
int vp8drv_stage_frame_host(vp8drv *d, const uint8_t *y, const uint8_t *u, const uint8_t *v) {
    if (!d || !y || !u || !v) return VP8HIP_ERR_ARG;
    if (d->s.canvas) return VP8HIP_ERR_STATE;
    { const int rc = resolve(d); if (rc < 0) return rc; }
    if (d->s.denoise || d->s.analysis || d->s.deinterlace) {      // the schedule's word on this frame, one call early: the verdict is in, so vp8host_gop_next will say the same
        vp8host_gop g = d->gop;
        vp8host_gop_next(&g);
        DRV_CHK(intake_restarts(d, g.current_is_key != 0));
    }
    DRV_CHK(vp8hip_upload_current(d->hip, y, u, v));
    d->staged = y;
    d->staged_scan = false;
    if (d->cfg.scene_detect) {
        DRV_CHK(vp8hip_chroma_change_async(d->hip));
        d->staged_scan = true;
    }
    return VP8HIP_OK;
}

int vp8drv_prefetch_frame_host(vp8drv *d, const uint8_t *y, const uint8_t *u, const uint8_t *v) {
    if (!d || !y || !u || !v) return VP8HIP_ERR_ARG;
    if (d->s.canvas) return VP8HIP_ERR_STATE;
    return vp8hip_prefetch_current(d->hip, y, u, v);
}

// vp8drv_set_canvas: frames composed of scaled video tiles from now on (n = 0: one source per frame again)
int vp8drv_set_canvas(vp8drv *d, const vp8hip_tile *tiles, int n, int bg_y, int bg_u, int bg_v) {
    if (!d) return VP8HIP_ERR_ARG;
    DRV_CHK(ask(d, vp8::CANVAS, n != 0));
    DRV_CHK(vp8hip_set_canvas(d->hip, tiles, n, bg_y, bg_u, bg_v));
    d->s.canvas = n;
    drop_staged(d);
    return VP8HIP_OK;
}

static int encode_frame_tiles(vp8drv *d, const vp8hip_tile_planes *src, int force_key, bool host) {
    if (!d || !src) return VP8HIP_ERR_ARG;
    if (!d->s.canvas) return VP8HIP_ERR_STATE;
    for (int k = 0; k < d->s.canvas; ++k)      // (what the context would refuse, before the schedule moves)
        if (src[k].y && (!src[k].u || !src[k].v || src[k].pitch_y < 0 || src[k].pitch_u < 0 || src[k].pitch_v < 0)) return VP8HIP_ERR_ARG;
    if (layers_refused(d)) return VP8HIP_ERR_STATE;
    { const int rc = resolve(d); if (rc < 0) return rc; }
    vp8host_gop_next(&d->gop);
    DRV_CHK(intake_restarts(d, d->gop.current_is_key != 0));
    DRV_CHK(host ? vp8hip_compose_current_host(d->hip, src) : vp8hip_compose_current_device(d->hip, src));
    return frame_body(d, nullptr, d->gop.current_is_key || force_key);
}

int vp8drv_encode_frame_tiles_device(vp8drv *d, const vp8hip_tile_planes *src, int force_key) { return encode_frame_tiles(d, src, force_key, false); }
int vp8drv_encode_frame_tiles_host(vp8drv *d, const vp8hip_tile_planes *src, int force_key) { return encode_frame_tiles(d, src, force_key, true); }

// ---- several GOP chunks one frame at a time, every stage one launch for all of them (vp8hip_batch_*) -----------------------
struct vp8drv_batch {
    int n = 0;
    vp8drv *d[VP8HIP_MAX_BATCH] = {};
    vp8hip_batch *hb = nullptr;
};

int vp8drv_batch_create(vp8drv_batch **out, vp8drv *const *drv, int n) {
    if (!out || !drv || n < 1 || n > VP8HIP_MAX_BATCH) return VP8HIP_ERR_ARG;
    *out = nullptr;
    vp8hip_ctx *ctx[VP8HIP_MAX_BATCH];
    vp8::DriverSettings first;
    for (int i = 0; i < n; ++i) {
        // Every member's settings are judged here, in front of vp8hip_batch_create: the context repeats part of this, but it judges
        // "already a member" (ERR_STATE) member by member, before a later member's ERR_ARG
        if (!drv[i]) return VP8HIP_ERR_ARG;
        const vp8::DriverSettings s = settings(drv[i]);
        if (i == 0) first = s;
        DRV_CHK(refusal(s, vp8::BATCH_MEMBER));
        const vp8::BatchShared &shared = s, &shared0 = first;
        if (!(shared == shared0)) return VP8HIP_ERR_ARG;
        ctx[i] = drv[i]->hip;
    }
    vp8drv_batch *b = new (std::nothrow) vp8drv_batch();
    if (!b) return VP8HIP_ERR_ARG;
    const int rc = vp8hip_batch_create(&b->hb, ctx, n);
    if (rc != VP8HIP_OK) {
        delete b;
        return rc;
    }
    b->n = n;
    for (int i = 0; i < n; ++i) {
        b->d[i] = drv[i];
        drv[i]->s.in_batch = true;
    }
    *out = b;
    return VP8HIP_OK;
}

void vp8drv_batch_destroy(vp8drv_batch *b) {
    if (!b) return;
    for (int i = 0; i < b->n; ++i) b->d[i]->s.in_batch = false;
    vp8hip_batch_destroy(b->hb);
    delete b;
}

int vp8drv_batch_lane(const vp8drv_batch *b) { return b ? vp8hip_batch_lane(b->hb) : -1; }

static int batch_encode_frame(vp8drv_batch *b, const int *members, const void *const *y, const void *const *u, const void *const *v,
                              const int *force_key, int *was_key, bool host) {
    if (!b || !y || !u || !v) return VP8HIP_ERR_ARG;
    int key[VP8HIP_MAX_BATCH], active[VP8HIP_MAX_BATCH], zero[VP8HIP_MAX_BATCH] = {};
    int pg[VP8HIP_MAX_BATCH], pa[VP8HIP_MAX_BATCH], ug[VP8HIP_MAX_BATCH], ua[VP8HIP_MAX_BATCH];
    int32_t refqi[VP8HIP_MAX_BATCH][4];
    for (int i = 0; i < b->n; ++i) {   // the members' open check_SSIM verdicts: a frame sent back is recoded as a key frame now
        const int rc = resolve(b->d[i]);
        if (rc < 0) return rc;
    }
    for (int i = 0; i < b->n; ++i) {
        vp8drv *d = b->d[i];
        key[i] = active[i] = 0;
        if (was_key) was_key[i] = 0;
        if (members && !members[i]) continue;      // this member sits the call out
        vp8host_gop_next(&d->gop);
        key[i] = d->gop.current_is_key || (force_key && force_key[i]);
        active[i] = !key[i];
        if (was_key) was_key[i] = key[i];
        DRV_CHK(intake_restarts(d, d->gop.current_is_key != 0));
    }
    if (host) DRV_CHK(vp8hip_batch_upload_current(b->hb, members, reinterpret_cast<const uint8_t *const *>(y), reinterpret_cast<const uint8_t *const *>(u),
                                                  reinterpret_cast<const uint8_t *const *>(v)));
    else DRV_CHK(vp8hip_batch_set_current_device(b->hb, members, y, u, v));          // vp8enc.cpp:386-388, all members in one launch
    int n_inter = 0, n_key = 0;
    for (int i = 0; i < b->n; ++i) n_key += key[i];
    static const bool batch_keys = [] { const char *e = getenv("VP8DRV_BATCH_KEYS"); return !(e && e[0] == '0'); }();   // =0: one after the other, as before (A/B runs)
    if (!batch_keys) n_key = n_key ? 1 : 0;
    if (n_key > 1) {
        // Several members start a GOP in this call (every chunk of a file coded GOPs side by side does, together): their key frames --
        // each a raster-order wavefront a millisecond and a half long -- in ONE launch instead of one after the other on the shared
        // stream, with the segment data, filter masks and loop filters of key_frame() batched the same way
        int32_t kq[VP8HIP_MAX_BATCH][4];
        int ones[VP8HIP_MAX_BATCH];
        for (int i = 0; i < b->n; ++i) {
            ones[i] = 1;
            for (int k = 0; k < 4; ++k) kq[i][k] = b->d[i]->altrefqi[k];
        }
        DRV_CHK(vp8hip_batch_auto_segments(b->hb, key, ones, kq, b->d[0]->qi_min));   // prepare_segments_data(), vp8enc.cpp:379-383
        DRV_CHK(vp8hip_batch_intra_transform(b->hb, key));                            // intra_transform() + prepare_filter_mask
        DRV_CHK(vp8hip_batch_loop_filter(b->hb, key));
        for (int i = 0; i < b->n; ++i) {
            if (!key[i]) continue;
            b->d[i]->sharpness = VP8HIP_SHARPNESS_ON_DEVICE;
            key_frame_final(b->d[i]);
        }
    }
    for (int i = 0; i < b->n; ++i) {
        vp8drv *d = b->d[i];
        if (members && !members[i]) continue;
        if (key[i]) {   // a single key frame: the member's ordinary path, on the shared stream
            if (n_key > 1) continue;
            const int rc = key_frame(d, nullptr);
            if (rc < 0) return rc;
            continue;
        }
        ++n_inter;
        const int32_t *q = d->gop.current_is_altref ? d->altrefqi : d->lastqi;   // vp8enc.cpp:149-151
        for (int k = 0; k < 4; ++k) refqi[i][k] = q[k];
        int32_t g = 0, a = 0;
        vp8host_gop_inter_flags(&d->gop, &g, &a);                               // inter_part.h:103-104
        ug[i] = g & (d->cfg.ref_mask & 1);
        ua[i] = a & ((d->cfg.ref_mask >> 1) & 1);
        pg[i] = d->gop.prev_is_golden;
        pa[i] = d->gop.prev_is_altref;
        d->sharpness = VP8HIP_SHARPNESS_ON_DEVICE;
    }
    if (!n_inter) return VP8HIP_OK;
    DRV_CHK(vp8hip_batch_auto_segments(b->hb, active, zero, refqi, b->d[0]->qi_min));   // vp8enc.cpp:390, 419
    DRV_CHK(vp8hip_batch_inter_transform(b->hb, active, pg, pa, ug, ua));
    const bool check = b->d[0]->cfg.check_ssim != 0;
    if (check) DRV_CHK(vp8hip_batch_check_ssim_async(b->hb, active, refqi, b->d[0]->qi_min));   // vp8enc.cpp:442, nobody waiting
    DRV_CHK(vp8hip_batch_loop_filter(b->hb, active));
    for (int i = 0; i < b->n; ++i) {
        if (!active[i]) continue;
        vp8drv *d = b->d[i];
        shown_inter_coded(d, ug[i], ua[i], pg[i], pa[i], d->gop.current_is_altref);
        d->ir_forced = d->ir.last_forced = 0;      // (a member has no period; what its last frame on its own forced is not this frame's)
        d->ir.last_q = d->ir_q;
        d->layer = vp8drv_layer_info{0, 0, 0, VP8HOST_REFRESH_LAST, ug[i], 1};
        if (check) d->verdict_pending = true;   // counted when the verdict is in (resolve())
        else inter_frame_done(d);
    }
    return VP8HIP_OK;
}

int vp8drv_batch_encode_frame_device(vp8drv_batch *b, const int *members, const void *const *y, const void *const *u, const void *const *v,
                                     const int *force_key, int *was_key) {
    return batch_encode_frame(b, members, y, u, v, force_key, was_key, false);
}
int vp8drv_batch_encode_frame_host(vp8drv_batch *b, const int *members, const void *const *y, const void *const *u, const void *const *v,
                                   const int *force_key, int *was_key) {
    return batch_encode_frame(b, members, y, u, v, force_key, was_key, true);
}

int vp8drv_batch_prefetch_frame_host(vp8drv_batch *b, const uint8_t *const *y, const uint8_t *const *u, const uint8_t *const *v) {
    if (!b) return VP8HIP_ERR_ARG;
    return vp8hip_batch_prefetch_current(b->hb, y, u, v);
}

// ---- the scan of a file's chroma differences, batched: what vp8host_scene_plan makes the key-frame schedule of ---------------------
// The members' frames are taken in and scene_change()'s two sums started (one launch for all of them); nothing is coded and neither the
// GOP state nor the scene history moves.  Whatever keeps a history of the frames taken in, or numbers them, would be disturbed by frames
// that are never coded -- and the schedule would then depend on itself: such members are refused, before anything changes.
//   denoiser:            the previous frame taken in is its history (and a scanned frame would be filtered against it)
//   deinterlace mode 2:  the previous frame as received is its history
//   analysis:            numbers the frames taken in and keeps the previous luma
//   quality statistics:  number their records by the frames taken in
// (deinterlace mode 1, a source format, scaling, a window, an orientation and a segment mode are functions of the one frame: allowed.)
static int batch_scan_frame(vp8drv_batch *b, const int *members, const void *const *y, const void *const *u, const void *const *v, bool host) {
    if (!b || !y || !u || !v) return VP8HIP_ERR_ARG;
    for (int i = 0; i < b->n; ++i) {
        if (members && !members[i]) continue;
        DRV_CHK(refusal(b->d[i]->s, vp8::SCAN));      // (it reads no fact that moves by itself)
    }
    for (int i = 0; i < b->n; ++i) {   // an open check_SSIM verdict needs the member's current frame: taken before the frame is replaced
        if (members && !members[i]) continue;
        const int rc = resolve(b->d[i]);
        if (rc < 0) return rc;
    }
    if (host) DRV_CHK(vp8hip_batch_upload_current(b->hb, members, reinterpret_cast<const uint8_t *const *>(y), reinterpret_cast<const uint8_t *const *>(u),
                                                  reinterpret_cast<const uint8_t *const *>(v)));
    else DRV_CHK(vp8hip_batch_set_current_device(b->hb, members, y, u, v));
    return vp8hip_batch_chroma_change_async(b->hb, members);
}

int vp8drv_batch_scan_frame_device(vp8drv_batch *b, const int *members, const void *const *y, const void *const *u, const void *const *v) {
    return batch_scan_frame(b, members, y, u, v, false);
}
int vp8drv_batch_scan_frame_host(vp8drv_batch *b, const int *members, const void *const *y, const void *const *u, const void *const *v) {
    return batch_scan_frame(b, members, y, u, v, true);
}

int vp8drv_batch_scan_result(vp8drv_batch *b, const int *members, int32_t *udiff, int32_t *vdiff) {
    if (!b || !udiff || !vdiff) return VP8HIP_ERR_ARG;
    for (int i = 0; i < b->n; ++i) {
        if (members && !members[i]) continue;
        DRV_CHK(vp8hip_chroma_change_result(b->d[i]->hip, &udiff[i], &vdiff[i]));
    }
    return VP8HIP_OK;
}

int vp8drv_resolve(vp8drv *d) {
    if (!d) return VP8HIP_ERR_ARG;
    const int rc = resolve(d);
    return rc < 0 ? rc : (d->have_frame && d->last_key ? 1 : 0);
}

// the record of the frame just made final: its verdict first (a frame coded again as a key frame has the key frame's record)
int vp8drv_get_frame_quality(vp8drv *d, vp8drv_quality *q) {
    if (!d || !q) return VP8HIP_ERR_ARG;
    if (!d->cfg.quality_stats || !d->have_frame) return VP8HIP_ERR_STATE;
    { const int rc = resolve(d); if (rc < 0) return rc; }
    return vp8hip_quality_result(d->hip, q);
}

int vp8drv_get_quality_summary(vp8drv *d, vp8drv_quality_summary *s) {
    if (!d || !s) return VP8HIP_ERR_ARG;
    if (!d->cfg.quality_stats) return VP8HIP_ERR_STATE;
    { const int rc = resolve(d); if (rc < 0) return rc; }
    return vp8hip_quality_summary(d->hip, s);
}

int vp8drv_set_denoise(vp8drv *d, int level) {
    DRV_CHK(intake_setter(d, level >= 0 && level <= 3, false, [&] { return vp8hip_set_denoise(d->hip, level); }));
    d->s.denoise = level;
    return VP8HIP_OK;
}

int vp8drv_set_deinterlace(vp8drv *d, int mode, int keep) {
    DRV_CHK(intake_setter(d, mode >= 0 && mode <= 2 && (keep == 0 || keep == 1), false, [&] { return vp8hip_set_deinterlace(d->hip, mode, keep); }));
    d->s.deinterlace = mode;
    d->s.field = mode ? keep : 0;
    return VP8HIP_OK;
}

int vp8drv_set_source_format(vp8drv *d, int format) {
    const bool known = (format >= 0 && format < VP8HOST_FORMAT_COUNT) || (format >= VP8HOST_FORMAT_PACKED_FIRST && format < VP8HOST_FORMAT_PACKED_END);
    DRV_CHK(intake_setter(d, known, true, [&] { return vp8hip_set_source_format(d->hip, format); }));
    d->s.format = format;
    return VP8HIP_OK;
}

int vp8drv_set_source_colour(vp8drv *d, int matrix) {
    DRV_CHK(intake_setter(d, matrix >= 0 && matrix < VP8HOST_COLOUR_COUNT, true, [&] { return vp8hip_set_source_colour(d->hip, matrix); }));
    d->s.colour = matrix;
    return VP8HIP_OK;
}

int vp8drv_set_source_transfer(vp8drv *d, int transfer, int peak) {
    DRV_CHK(intake_setter(d, transfer >= VP8HOST_TRANSFER_SDR && transfer <= VP8HOST_TRANSFER_HLG, true, [&] { return vp8hip_set_source_transfer(d->hip, transfer, peak); }));
    d->s.transfer = transfer;
    d->s.peak = transfer ? peak : 0;
    return VP8HIP_OK;
}

// vp8drv_set_overlay_*: layers burnt into the frames taken in from now on.  Allowed on a member of a live batch between frames, as
// vp8drv_set_segment_map is; with cfg.device_params = 0 the host mirror scans the caller's luma, which is not the frame coded.
int vp8drv_set_overlay_host(vp8drv *d, int slot, int format, int matrix, const uint8_t *pixels, int lw, int lh, int pitch, int x, int y, int opacity) {
    if (!d || !d->cfg.device_params) return VP8HIP_ERR_ARG;
    { const int rc = resolve(d); if (rc < 0) return rc; }      // the open check_SSIM verdict first
    return vp8hip_set_overlay_host(d->hip, slot, format, matrix, pixels, lw, lh, pitch, x, y, opacity);
}

int vp8drv_set_overlay_device(vp8drv *d, int slot, int format, int matrix, const void *pixels, int lw, int lh, int pitch, int x, int y, int opacity) {
    if (!d || !d->cfg.device_params) return VP8HIP_ERR_ARG;
    { const int rc = resolve(d); if (rc < 0) return rc; }
    return vp8hip_set_overlay_device(d->hip, slot, format, matrix, pixels, lw, lh, pitch, x, y, opacity);
}

int vp8drv_set_overlay_placement(vp8drv *d, int slot, int x, int y, int opacity) {
    if (!d || !d->cfg.device_params) return VP8HIP_ERR_ARG;
    { const int rc = resolve(d); if (rc < 0) return rc; }
    return vp8hip_set_overlay_placement(d->hip, slot, x, y, opacity);
}

int vp8drv_clear_overlay(vp8drv *d, int slot) {
    if (!d || !d->cfg.device_params) return VP8HIP_ERR_ARG;
    { const int rc = resolve(d); if (rc < 0) return rc; }
    return vp8hip_clear_overlay(d->hip, slot);
}

int vp8drv_set_source_window(vp8drv *d, const int32_t *pitch, int x, int y) {
    DRV_CHK(intake_setter(d, true, true, [&] { return vp8hip_set_source_window(d->hip, pitch, x, y); }));
    d->s.window = pitch != nullptr;
    return VP8HIP_OK;
}

int vp8drv_set_source_orientation(vp8drv *d, int turns, int mirror) {
    return intake_setter(d, true, true, [&] { return vp8hip_set_source_orientation(d->hip, turns, mirror); });
}

int vp8drv_set_analysis(vp8drv *d, int on) {
    DRV_CHK(intake_setter(d, on == 0 || on == 1, false, [&] { return vp8hip_set_analysis(d->hip, on); }));
    d->s.analysis = on != 0;
    return VP8HIP_OK;
}

// vp8hip_set_segment_mode for the frame loop: inter frames are coded in the mode from the next frame taken in on, key frames as ever
int vp8drv_set_segment_mode(vp8drv *d, int mode, int strength) {
    if (!d || mode < 0 || mode > 2 || (mode == 2 && (strength < 1 || strength > 3))) return VP8HIP_ERR_ARG;
    if (d->s.in_batch) return VP8HIP_ERR_STATE;
    { const int rc = resolve(d); if (rc < 0) return rc; }
    return vp8hip_set_segment_mode(d->hip, mode, strength);
}

// the caller's map of mode 1, in force until replaced (the members of a batch each have their own)
int vp8drv_set_segment_map(vp8drv *d, const uint8_t *host_map) {
    if (!d || !host_map) return VP8HIP_ERR_ARG;
    { const int rc = resolve(d); if (rc < 0) return rc; }      // (a frame sent back is coded again under the map it was coded under)
    return vp8hip_upload_segment_map(d->hip, host_map);
}

// the record of the frame just made final: its verdict first (a frame coded again as a key frame has the key frame's coding side)
int vp8drv_get_frame_analysis(vp8drv *d, vp8drv_analysis *a) {
    if (!d || !a) return VP8HIP_ERR_ARG;
    if (!d->s.analysis || !d->have_frame) return VP8HIP_ERR_STATE;
    { const int rc = resolve(d); if (rc < 0) return rc; }
    return vp8hip_analysis_result(d->hip, a);
}

// the two ladders and qi_min as vp8drv_create makes them, from the next frame coded on (every frame takes its quantizers from them)
int vp8drv_set_quantizer(vp8drv *d, int qi_min, int qi_max) {
    if (!d || qi_min < 0 || qi_min > 127 || qi_max < 0 || qi_max > 127) return VP8HIP_ERR_ARG;
    if (d->s.in_batch) return VP8HIP_ERR_STATE;
    { const int rc = resolve(d); if (rc < 0) return rc; }      // (a frame sent back is coded again with the pair it was coded with)
    d->s.qi_min = qi_min;
    d->s.qi_max = qi_max;
    vp8host_quantizer_ladders(qi_min, qi_max, d->lastqi, d->altrefqi);
    d->qi_min = qi_min < qi_max ? qi_min : qi_max;
    return VP8HIP_OK;
}

int vp8drv_get_quantizer(const vp8drv *d, int32_t *qi_min, int32_t *qi_max) {
    if (!d || !qi_min || !qi_max) return VP8HIP_ERR_ARG;
    *qi_min = d->s.qi_min;
    *qi_max = d->s.qi_max;
    return VP8HIP_OK;
}

int vp8drv_get_denoise_stats(vp8drv *d, vp8hip_denoise_stats *s) {
    if (!d || !s) return VP8HIP_ERR_ARG;
    return vp8hip_denoise_result(d->hip, s);
}

int vp8drv_get_deinterlace_stats(vp8drv *d, vp8hip_deinterlace_stats *s) {
    if (!d || !s) return VP8HIP_ERR_ARG;
    return vp8hip_deinterlace_result(d->hip, s);
}

// ---- hidden alternate reference frames ------------------------------------------------------------------------------------------------
int vp8drv_set_arf(vp8drv *d, int strength_plus_one) {
    if (!d || strength_plus_one < 0 || strength_plus_one > 7) return VP8HIP_ERR_ARG;
    DRV_CHK(ask(d, vp8::ARF, strength_plus_one != 0));
    d->s.arf = strength_plus_one;
    if (!strength_plus_one && d->arf_st.hidden_frames) (void)vp8hip_arf_result(d->hip, d->arf_st.last_weight);
    if (!strength_plus_one) return vp8hip_arf_release(d->hip);      // (the staging buffers only: the current frame and ALTREF are surfaces)
    return VP8HIP_OK;
}

// The filtered frame is the context's current frame: code it as an inter frame on the finer ladder, with the references the next
// shown frame would be allowed, no check_SSIM, and the reconstruction into ALTREF.  The GOP state, the frame counters, the scene
// history and the quality summary are not touched: they count shown frames.
static int hidden_frame(vp8drv *d) {
    DRV_CHK(segments(d, nullptr, false, d->altrefqi));
    // the rotation the last shown frame owes (vp8host_gop_next would name it prev_is_*), unless a hidden frame has applied it already
    const int32_t owed_golden = d->rotation_consumed ? 0 : d->gop.current_is_golden, owed_altref = d->rotation_consumed ? 0 : d->gop.current_is_altref;
    if (owed_altref) d->hidden_altref = false;
    int32_t use_golden = !d->gop.current_is_golden;
    int32_t use_altref = !owed_altref && (d->hidden_altref || d->gop.altref_frame_number != d->gop.golden_frame_number);
    use_golden &= d->cfg.ref_mask & 1;
    use_altref &= (d->cfg.ref_mask >> 1) & 1;
    DRV_CHK(vp8hip_inter_transform(d->hip, owed_golden, owed_altref, use_golden, use_altref));
    d->rotation_consumed = true;
    DRV_CHK(vp8hip_loop_filter_hidden(d->hip));
    d->hidden_altref = true;
    inter_frame_coded(d, true, true);
    d->arf_st.hidden_frames++;
    d->arf_st.last_use_golden = use_golden;
    d->arf_st.last_use_altref = use_altref;
    return VP8HIP_OK;
}

static int arf_check(vp8drv *d, const void *frames, int n, int centre) {
    if (!d || !frames || n < 1 || n > VP8HOST_ARF_MAX_FRAMES || centre < 0 || centre >= n) return VP8HIP_ERR_ARG;
    // what refuses hidden frames refuses this one, and so do layers burnt in (the window frames bypass the intake: a layer would miss
    // them) and the states of the moment: off; no reference yet; a frame handed over early is the current frame.  (The overlapped filter
    // is the setter's word alone: with it hidden frames are never on, and the answer here is "off".)
    vp8::DriverSettings s = settings(d);
    s.overlap_filter = false;
    const int table = refusal(s, vp8::ARF);
    if (table == VP8HIP_ERR_ARG || s.overlays) return VP8HIP_ERR_ARG;
    if (table != VP8HIP_OK || !s.arf || !d->have_frame || d->staged) return VP8HIP_ERR_STATE;
    const int rc = resolve(d);                                                                // the open check_SSIM verdict first
    return rc < 0 ? rc : VP8HIP_OK;
}

int vp8drv_encode_arf_device(vp8drv *d, const void *const (*frames)[3], int n, int centre) {
    DRV_CHK(arf_check(d, frames, n, centre));
    DRV_CHK(vp8hip_arf_filter_device(d->hip, frames, n, centre, d->s.arf - 1));
    d->arf_st.last_frames = n;
    return hidden_frame(d);
}

int vp8drv_encode_arf_host(vp8drv *d, const uint8_t *const (*frames)[3], int n, int centre) {
    DRV_CHK(arf_check(d, frames, n, centre));
    DRV_CHK(vp8hip_arf_filter_host(d->hip, frames, n, centre, d->s.arf - 1));
    d->arf_st.last_frames = n;
    return hidden_frame(d);
}

int vp8drv_get_arf_stats(vp8drv *d, vp8drv_arf_stats *s) {
    if (!d || !s) return VP8HIP_ERR_ARG;
    if (!d->arf_st.hidden_frames) return VP8HIP_ERR_STATE;
    const int rc = vp8hip_arf_result(d->hip, d->arf_st.last_weight);      // (VP8HIP_ERR_STATE: released by vp8drv_set_arf(d, 0), which kept them)
    if (rc != VP8HIP_OK && rc != VP8HIP_ERR_STATE) return rc;
    *s = d->arf_st;
    return VP8HIP_OK;
}

// ---- temporal layers --------------------------------------------------------------------------------------------------------------------
int vp8drv_set_temporal_layers(vp8drv *d, int layers, int flags) {
    if (!d || layers < 1 || layers > 3 || (flags & ~VP8DRV_TL_KEEP_RECON)) return VP8HIP_ERR_ARG;
    DRV_CHK(ask(d, vp8::LAYERS, layers > 1));
    d->s.tl_next = layers;
    d->s.tl_flags = layers > 1 ? flags : 0;
    return VP8HIP_OK;
}

int vp8drv_get_frame_layer(vp8drv *d, vp8drv_layer_info *info) {
    if (!d || !info) return VP8HIP_ERR_ARG;
    if (!d->have_frame || d->last_hidden) return VP8HIP_ERR_STATE;
    { const int rc = resolve(d); if (rc < 0) return rc; }
    *info = d->layer;
    return VP8HIP_OK;
}

// ---- cyclic intra refresh ---------------------------------------------------------------------------------------------------------------
int vp8drv_set_intra_refresh(vp8drv *d, int period) {
    if (!d || (period != 0 && (period < VP8HOST_INTRA_REFRESH_MIN || period > VP8HOST_INTRA_REFRESH_MAX))) return VP8HIP_ERR_ARG;
    DRV_CHK(ask(d, vp8::INTRA_REFRESH, period != 0));
    d->s.ir_period = d->ir.period = period;
    return VP8HIP_OK;
}

int vp8drv_get_intra_refresh(vp8drv *d, vp8drv_intra_refresh_info *info) {
    if (!d || !info) return VP8HIP_ERR_ARG;
    { const int rc = resolve(d); if (rc < 0) return rc; }
    *info = d->ir;
    return VP8HIP_OK;
}

int vp8drv_ready(const vp8drv *d) { return !d || !d->verdict_pending || vp8hip_check_ssim_ready(d->hip); }
int vp8drv_batch_ready(const vp8drv_batch *b) {
    if (!b) return 1;
    for (int i = 0; i < b->n; ++i)
        if (!vp8drv_ready(b->d[i])) return 0;
    return 1;
}

int vp8drv_batches_encode_frame_device(vp8drv_batch *const *batches, int nbatches, const void *const *const *y, const void *const *const *u,
                                       const void *const *const *v, int *const *was_key) {
    if (!batches || nbatches < 1 || nbatches > 64 || !y || !u || !v) return VP8HIP_ERR_ARG;
    // In the order of the array, each batch waiting for its own verdicts.  (Serving whichever batch is ready first was tried
    // and is slower -- 55-58.8 against 58.8-59.5 M MB/s on the same box: a fixed order keeps the batches evenly staggered, and it
    // is the staggering that lets one batch's latency-bound loop filter run beside the others' searches.)
#ifdef VP8HIP_EXPERIMENTS
    static const bool ready_first = getenv("VP8DRV_EXPERIMENT_READY_FIRST") != nullptr;
#else
    constexpr bool ready_first = false;
#endif
    if (!ready_first) {
        for (int k = 0; k < nbatches; ++k)
            DRV_CHK(vp8drv_batch_encode_frame_device(batches[k], nullptr, y[k], u[k], v[k], nullptr, was_key ? was_key[k] : nullptr));
        return VP8HIP_OK;
    }
    bool done[64] = {};
    for (int left = nbatches; left > 0;) {
        bool progress = false;
        for (int k = 0; k < nbatches; ++k) {
            if (done[k] || !vp8drv_batch_ready(batches[k])) continue;
            DRV_CHK(vp8drv_batch_encode_frame_device(batches[k], nullptr, y[k], u[k], v[k], nullptr, was_key ? was_key[k] : nullptr));
            done[k] = true;
            --left;
            progress = true;
        }
        if (!progress) __builtin_ia32_pause();
    }
    return VP8HIP_OK;
}

uint64_t vp8drv_frame_check(uint64_t h, const uint8_t *frame, size_t size) {
    // position-dependent: every word is folded into a running value that is rotated and multiplied before the next one, so words
    // that trade places (a misplaced chunk of the parallel coder's output) or changes that cancel in a sum do not go unnoticed
    uint64_t f = h * 0x9E3779B97F4A7C15ull + (uint64_t)size;
    size_t i = 0;
    for (; i + 8 <= size; i += 8) {
        uint64_t w;
        memcpy(&w, frame + i, 8);
        f = (((f << 5) | (f >> 59)) ^ w) * 0x100000001B3ull;
    }
    if (i < size) {
        uint64_t w = 0;
        memcpy(&w, frame + i, size - i);
        f = (((f << 5) | (f >> 59)) ^ w) * 0x100000001B3ull;
    }
    return f;
}

static int batches_encode_frames(vp8drv_batch *const *batches, int nbatches, int nframes, const void *const (*frames)[3], int nd,
                                 const int *const *start, int *const *keys_out, uint64_t *const *bytes_out, uint64_t *const *check_out, bool host) {
    if (!batches || nbatches < 1 || nbatches > 64 || nframes < 0 || !frames || nd < 1 || !start || (check_out && !bytes_out)) return VP8HIP_ERR_ARG;
    for (int k = 0; k < nbatches; ++k)
        if (!batches[k] || batches[k]->n < 1 || !batches[k]->d[0] || !start[k]) return VP8HIP_ERR_ARG;
    std::vector<std::thread> th;
    std::vector<int> rc((size_t)nbatches, VP8HIP_OK);
    // Thread k starts k * 200 us after thread 0.  Batches that start together from an idle device stay in lockstep -- every verdict
    // arrives at the same moment, every next frame is enqueued at the same moment -- and then all the latency-bound loop filters run
    // at once with nothing wide beside them: 55.3-59.0 M MB/s from run to run on one box; with the starts a fraction of a frame
    // apart the batches stay staggered: 60.2-60.6 (800 us apart: 60.1-60.4).  VP8DRV_STAGGER_US overrides (experiments).
    // A thread per batch also where two batches share a chain stream (a lane, vp8hip_batch_lane): the two are independent work in one
    // in-order stream, each batch's own order is its thread's, and nothing here waits on a batch's stream being empty of OTHER work
    // (finish() below synchronises the lane, which then includes what the other batch had enqueued by then -- it ends, since that
    // batch's thread never waits for this one).
    static const int stagger_us = [] { const char *v = getenv("VP8DRV_STAGGER_US"); return v ? atoi(v) : 200; }();
    for (int k = 0; k < nbatches; ++k)
        th.emplace_back([&, k] {
            if (stagger_us > 0) std::this_thread::sleep_for(std::chrono::microseconds((long)k * stagger_us));
            vp8drv_batch *b = batches[k];
            const void *y[VP8HIP_MAX_BATCH], *u[VP8HIP_MAX_BATCH], *v[VP8HIP_MAX_BATCH];
            int key[VP8HIP_MAX_BATCH] = {};
            std::vector<uint8_t> frame;
            if (bytes_out) frame.resize((size_t)b->d[0]->mbs * 1900 + (1u << 20));
            auto encode = [&](int t) {
                for (int i = 0; i < b->n; ++i) {
                    const void *const *f = frames[(start[k][i] + t) % nd];
                    y[i] = f[0]; u[i] = f[1]; v[i] = f[2];
                }
                rc[k] = batch_encode_frame(b, nullptr, y, u, v, nullptr, key, host);
                if (rc[k] == VP8HIP_OK && keys_out && keys_out[k])   // (a failed call may not have filled key[])
                    for (int i = 0; i < b->n; ++i) keys_out[k][i] += key[i];
                if (host && rc[k] == VP8HIP_OK && t + 1 < nframes) {   // the next frame's planes on their way while this one is coded
                    const uint8_t *py[VP8HIP_MAX_BATCH], *pu[VP8HIP_MAX_BATCH], *pv[VP8HIP_MAX_BATCH];
                    for (int i = 0; i < b->n; ++i) {
                        const void *const *f = frames[(start[k][i] + t + 1) % nd];
                        py[i] = static_cast<const uint8_t *>(f[0]); pu[i] = static_cast<const uint8_t *>(f[1]); pv[i] = static_cast<const uint8_t *>(f[2]);
                    }
                    rc[k] = vp8hip_batch_prefetch_current(b->hb, py, pu, pv);
                }
            };
            // A bounded device-side wait that expires inside a frame's loop filter shows in the NEXT frame's verdict at the earliest (the
            // verdict workgroup samples the error word when the filter's launch starts), and nobody comes after the last frame: the call
            // ends with every member's last verdict taken and its stream synchronised, so that a time-out anywhere in the run is THIS
            // call's return value (VP8HIP_ERR_TIMEOUT), not a later call's surprise.
            auto finish = [&] {
                for (int i = 0; i < b->n && rc[k] == VP8HIP_OK; ++i) {
                    const int r = vp8drv_resolve(b->d[i]);
                    rc[k] = r < 0 ? r : vp8hip_synchronize(b->d[i]->hip);
                }
            };
            if (!bytes_out) {
                for (int t = 0; t < nframes && rc[k] == VP8HIP_OK; ++t) encode(t);
                finish();
                return;
            }
            // The frames as bytes: one set of launches for the batch's entropy stage, then every member's read-back -- with frame t + 1
            // ENQUEUED before frame t's bytes are waited for: the stage is a link of the batch's chain (same stream), so frame t + 1's
            // kernels queue up behind it and the stream never runs dry while this thread sleeps on the stage's event, copies six
            // frames and comes back (in the old order -- encode, begin, end, encode -- it did, once per frame and batch).  A frame
            // denser than the coder's scratch could not be coded again once the next frame has overwritten its coefficients, so the
            // scratch is sized for the densest frame there can be (a no-op when the caller has done it: vp8hip_reserve_frame_path_dense).
            for (int i = 0; i < b->n && rc[k] == VP8HIP_OK; ++i) rc[k] = vp8hip_reserve_frame_path_dense(b->d[i]->hip);
            if (nframes > 0 && rc[k] == VP8HIP_OK) encode(0);
            for (int t = 0; t < nframes && rc[k] == VP8HIP_OK; ++t) {
                rc[k] = vp8drv_batch_get_frame_begin(b, nullptr);                       // frame t's type is final here (its verdict is in)
                if (rc[k] == VP8HIP_OK && t + 1 < nframes) encode(t + 1);
                for (int i = 0; i < b->n && rc[k] == VP8HIP_OK; ++i) {
                    size_t size = 0;
                    rc[k] = vp8drv_get_frame_end(b->d[i], frame.data(), frame.size(), &size);
                    if (bytes_out[k]) bytes_out[k][i] += size;
                    if (check_out && check_out[k] && rc[k] == VP8HIP_OK) check_out[k][i] = vp8drv_frame_check(check_out[k][i], frame.data(), size);
                }
            }
            finish();
        });
    for (auto &t : th) t.join();
    for (int k = 0; k < nbatches; ++k)
        if (rc[k] != VP8HIP_OK) return rc[k];
    return VP8HIP_OK;
}

int vp8drv_batches_encode_frames_device(vp8drv_batch *const *batches, int nbatches, int nframes, const void *const (*frames)[3], int nd,
                                        const int *const *start, int *const *keys_out, uint64_t *const *bytes_out, uint64_t *const *check_out) {
    return batches_encode_frames(batches, nbatches, nframes, frames, nd, start, keys_out, bytes_out, check_out, false);
}
int vp8drv_batches_encode_frames_host(vp8drv_batch *const *batches, int nbatches, int nframes, const void *const (*frames)[3], int nd,
                                      const int *const *start, int *const *keys_out, uint64_t *const *bytes_out, uint64_t *const *check_out) {
    return batches_encode_frames(batches, nbatches, nframes, frames, nd, start, keys_out, bytes_out, check_out, true);
}

int vp8drv_get_frame(vp8drv *d, uint8_t *out, size_t capacity, size_t *size) {
    if (!d || !out || !size) return VP8HIP_ERR_ARG;
    if (!d->have_frame) return VP8HIP_ERR_STATE;
    const int P = d->cfg.num_partitions;
    if (P != 1 && P != 2 && P != 4 && P != 8) return VP8HIP_ERR_ARG;
    { const int rc = resolve(d); if (rc < 0) return rc; }    // the frame's type and intra information must be final
    return get_frame(d, out, capacity, size);
}

int vp8drv_get_frame_begin(vp8drv *d) {
    if (!d) return VP8HIP_ERR_ARG;
    if (!d->have_frame || d->cfg.host_bitstream) return VP8HIP_ERR_STATE;
    const int P = d->cfg.num_partitions;
    if (P != 1 && P != 2 && P != 4 && P != 8) return VP8HIP_ERR_ARG;
    { const int rc = resolve(d); if (rc < 0) return rc; }
    const vp8hip_header_params hp = header_params(d);
    return vp8hip_encode_frame_begin(d->hip, P, &hp);
}

// vp8drv_get_frame_begin for the members of a batch in one set of launches; every member then takes its frame with
// vp8drv_get_frame_end
int vp8drv_batch_get_frame_begin(vp8drv_batch *b, const int *members) {
    if (!b) return VP8HIP_ERR_ARG;
    vp8hip_header_params hp[VP8HIP_MAX_BATCH];
    const int P = b->d[0]->cfg.num_partitions;
    if (P != 1 && P != 2 && P != 4 && P != 8) return VP8HIP_ERR_ARG;
    for (int i = 0; i < b->n; ++i) {
        if (members && !members[i]) continue;
        vp8drv *d = b->d[i];
        if (d->cfg.num_partitions != P) return VP8HIP_ERR_ARG;
        if (!d->have_frame || d->cfg.host_bitstream) return VP8HIP_ERR_STATE;
        const int rc = resolve(d);
        if (rc < 0) return rc;
        hp[i] = header_params(d);
    }
    return vp8hip_batch_encode_frame_begin(b->hb, members, P, hp);
}

int vp8drv_get_frame_end(vp8drv *d, uint8_t *out, size_t capacity, size_t *size) {
    if (!d || !out || !size) return VP8HIP_ERR_ARG;
    return vp8hip_encode_frame_end(d->hip, out, capacity, size);
}

int vp8drv_encode_video_device(vp8drv *d, int nframes, const void *const (*frames)[3], int nd, int start, uint8_t *out, size_t capacity,
                               uint32_t *sizes, int *keys) {
    if (!d || nframes < 0 || !frames || nd < 1 || start < 0 || (out && !sizes)) return VP8HIP_ERR_ARG;
    size_t used = 0;
    int nkeys = 0;
    if (!out) {      // no frames out: a frame's verdict is taken by the next call (resolve() at its head), the last one's here
        for (int t = 0; t < nframes; ++t) {
            const void *const *f = frames[(start + t) % nd];
            const int rc = vp8drv_encode_frame_device(d, f[0], f[1], f[2], 0);
            if (rc < 0) return rc;
        }
        const int rc = vp8drv_resolve(d);
        if (rc < 0) return rc;
        if (keys) *keys = -1;     // (not counted here: vp8drv_get_stats has key_frames and redone_as_key)
        // The last frame's filter is still running, and a bounded device-side wait that expires INSIDE it shows only in a later
        // verdict or here (the verdict workgroup samples the error word when the filter's launch starts): nobody comes after the last frame
        return vp8hip_synchronize(d->hip);
    }
    // Frame t + 1 is started before frame t's bytes are taken: a frame denser than the coder's scratch could not be coded again by
    // then (vp8hip_encode_frame_end: VP8HIP_ERR_STATE), so the scratch is sized for the densest frame there can be -- a no-op if the
    // caller has done it.  ~270 MB per context at 1080p, four times that at 4K; allocated behind a synchronisation, so callers that
    // time this call reserve beforehand (vp8hip_reserve_frame_path_dense).
    if (nframes > 0) DRV_CHK(vp8hip_reserve_frame_path_dense(d->hip));
    for (int t = 0; t < nframes; ++t) {
        const void *const *f = frames[(start + t) % nd];
        int rc = vp8drv_encode_frame_device(d, f[0], f[1], f[2], 0);          // frame t under way ...
        if (rc < 0) return rc;
        if (t > 0) {                                                          // ... now frame t - 1's bytes
            size_t n = 0;
            rc = vp8drv_get_frame_end(d, out + used, capacity - used, &n);
            if (rc < 0) return rc;
            sizes[t - 1] = (uint32_t)n;
            used += n;
        }
        rc = vp8drv_get_frame_begin(d);                                       // frame t's type is final (the verdict is in): its stage
        if (rc < 0) return rc;
        rc = vp8drv_resolve(d);
        if (rc < 0) return rc;
        nkeys += rc > 0;
    }
    if (nframes > 0) {
        size_t n = 0;
        const int rc = vp8drv_get_frame_end(d, out + used, capacity - used, &n);
        if (rc < 0) return rc;
        sizes[nframes - 1] = (uint32_t)n;
    }
    if (keys) *keys = nkeys;
    return VP8HIP_OK;
}

}  // extern "C"
