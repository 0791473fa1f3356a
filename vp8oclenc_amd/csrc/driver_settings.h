// driver_settings.h -- what the native frame loop (vp8_driver.cpp) knows about one driver's settings, in one struct, and the one answer
// to "may these settings stand together?": refusal(), the table below, and operator== over what the members of a batch must share.
// Pure host code over the public headers: no HIP type, no vp8drv.  Every setter and every frame entry point of the driver asks here;
// a new opt-in adds its field, its row and its column, and touches no other list.
//
//   asked for                          VP8HIP_ERR_ARG when                                        VP8HIP_ERR_STATE when
//   ARF            hidden alt-refs on  !device_params, overlap_filter, format, window,            in_batch, canvas, layers in force or asked for
//                                      deinterlace, denoise, analysis
//                  ... off             --                                                         in_batch
//   LAYERS         more than one       !device_params, overlap_filter, scheduled alt-refs         in_batch, arf, a by-reference split
//   INTRA_REFRESH  a period            !device_params, an SSIM target above -1                    in_batch, a by-reference split
//   CANVAS         tiles               !device_params                                             in_batch, arf
//                  ... none            !device_params                                             --
//   INTAKE_SETTER  denoise, deinterlace, format, colour, transfer, window, orientation, analysis
//                                      !device_params                                             in_batch
//   BATCH_MEMBER                       !device_params, overlap_filter, scene_detect, arf, canvas, --
//                                      a hidden frame still shapes the references, layers in
//                                      force or asked for, a refresh period
//   SCAN           the batched scan    --                                                         denoise, deinterlace mode 2, analysis, quality_stats
//
// One layer and period 0 are always accepted.  The ARG clauses are judged before the STATE clauses.
#ifndef VP8HIP_DRIVER_SETTINGS_H
#define VP8HIP_DRIVER_SETTINGS_H
#include "../../include/vp8hip_driver.h"

namespace vp8 {

// What the members of a batch must share: one launch serves all of them, so what travels as ONE kernel argument must agree (the segment
// maps are the members' own).  scale_filter holds 0 where no scaler is set.
struct BatchShared {
    int qi_min = 0, qi_max = 0, num_partitions = 0, loop_filter_type = 0, in_width = 0, in_height = 0, scale_filter = 0;   // vp8drv_config (vp8drv_set_quantizer)
    bool check_ssim = false;
    int denoise = 0;                      // vp8drv_set_denoise: the level in force
    int deinterlace = 0, field = 0;       // vp8drv_set_deinterlace: the mode and the field kept
    int format = 0, colour = 0;           // vp8drv_set_source_format, vp8drv_set_source_colour
    int transfer = 0, peak = 0;           // vp8drv_set_source_transfer (0, 0: off)
    bool analysis = false;                // vp8drv_set_analysis
    int seg_mode = 0, seg_strength = 0;   // vp8drv_set_segment_mode, as the context has it: filled in before the question
};
inline bool operator==(const BatchShared &a, const BatchShared &b) {
    return a.qi_min == b.qi_min && a.qi_max == b.qi_max && a.num_partitions == b.num_partitions && a.loop_filter_type == b.loop_filter_type &&
           a.in_width == b.in_width && a.in_height == b.in_height && a.scale_filter == b.scale_filter && a.check_ssim == b.check_ssim &&
           a.denoise == b.denoise && a.deinterlace == b.deinterlace && a.field == b.field && a.format == b.format && a.colour == b.colour &&
           a.transfer == b.transfer && a.peak == b.peak && a.analysis == b.analysis && a.seg_mode == b.seg_mode && a.seg_strength == b.seg_strength;
}

struct DriverSettings : BatchShared {
    // vp8drv_config, fixed at creation
    bool device_params = false, overlap_filter = false, scene_detect = false, quality_stats = false;
    bool ssim_target = false;             // an SSIM target above -1
    bool scheduled_altref = false;        // altref_range <= gop_size: the GOP schedule makes shown alt-ref frames
    // the setters
    bool window = false;                  // vp8drv_set_source_window: a window is in force
    int canvas = 0;                       // vp8drv_set_canvas: tiles of the canvas in force (0 = none)
    int arf = 0;                          // vp8drv_set_arf: strength + 1 (0 = off)
    int tl_layers = 1, tl_next = 1, tl_flags = 0;   // vp8drv_set_temporal_layers: layers in force (1 = off), asked for (in force from the next key frame on), the flags
    int ir_period = 0;                    // vp8drv_set_intra_refresh: the period in force (0 = off)
    bool in_batch = false;                // a member of a live vp8drv_batch
    // what moves by itself: filled in before the question
    bool hidden_shapes_refs = false;      // a hidden frame's rotation or reconstruction still shapes the references
    bool shard = false;                   // the context has joined a by-reference split
    bool overlays = false;                // layers are burnt into the frames taken in (vp8drv_encode_arf_*: the window frames would miss them)
};

enum Feature { ARF, LAYERS, INTRA_REFRESH, CANVAS, INTAKE_SETTER, BATCH_MEMBER, SCAN };

inline bool layered(const DriverSettings &s) { return s.tl_layers > 1 || s.tl_next > 1; }

// THE TABLE: may a driver with these settings have the feature (on), or drop it (!on)?  VP8HIP_OK, VP8HIP_ERR_ARG or VP8HIP_ERR_STATE.
inline int refusal(const DriverSettings &s, Feature f, bool on = true) {
    bool arg = false, state = false;
    switch (f) {
    case ARF:      // (what keeps a history or reads the planes another way would miss the window frames; a canvas: they bypass the compose launch; layers never search ALTREF)
        arg = on && (!s.device_params || s.overlap_filter || s.format || s.window || s.deinterlace || s.denoise || s.analysis);
        state = s.in_batch || (on && (s.canvas || layered(s)));
        break;
    case LAYERS:
        arg = on && (!s.device_params || s.overlap_filter || s.scheduled_altref);
        state = on && (s.in_batch || s.arf || s.shard);
        break;
    case INTRA_REFRESH:
        arg = on && (!s.device_params || s.ssim_target);
        state = on && (s.in_batch || s.shard);
        break;
    case CANVAS:
        arg = !s.device_params;
        state = on && (s.in_batch || s.arf);
        break;
    case INTAKE_SETTER:      // (with host parameters the mirror scans the caller's luma, which is not the frame coded)
        arg = !s.device_params;
        state = s.in_batch;
        break;
    case BATCH_MEMBER:       // (the batched loop is the device-parameter loop; hidden frames, layers and intra refresh are not batched)
        arg = !s.device_params || s.overlap_filter || s.scene_detect || s.arf || s.canvas || s.hidden_shapes_refs || layered(s) || s.ir_period;
        break;
    case SCAN:               // (whatever keeps a history of the frames taken in, or numbers them, would be disturbed by frames that are never coded)
        state = s.denoise || s.deinterlace == 2 || s.analysis || s.quality_stats;
        break;
    }
    return arg ? VP8HIP_ERR_ARG : (state ? VP8HIP_ERR_STATE : VP8HIP_OK);
}

}  // namespace vp8

#endif
