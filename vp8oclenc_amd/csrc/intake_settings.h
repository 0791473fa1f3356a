// intake_settings.h -- the settings that steer how a source frame becomes a context's current frame (take_frames, api_intake.hip), in
// one struct: what is valid (intake_valid, the one judge of a complete candidate), what is equal (operator==: two contexts may share a
// batch, a setter has nothing to do), and the sizes that follow.  Pure host code over include/vp8hip_host.h: no HIP type, no context.
// A setter copies the context's settings, edits the copy and hands it to intake_apply (api_intake.hip).
#ifndef VP8HIP_INTAKE_SETTINGS_H
#define VP8HIP_INTAKE_SETTINGS_H
#include "../../include/vp8hip_host.h"

namespace vp8 {

constexpr int INTAKE_OK = 0, INTAKE_REFUSED = -1;      // (VP8HIP_OK, VP8HIP_ERR_ARG: vp8hip_ctx.h asserts it)

// Everything in front of the pack or scale launch: what the caller's raw planes mean.  Every size describes the UPRIGHT frame.
struct SourceShape {
    int src_w = 0, src_h = 0;                 // vp8hip_set_source_size: the picture inside the coded size (0 = the coded size)
    int in_w = 0, in_h = 0, scale_kind = 0;   // vp8hip_set_source_scaling: frames come in at in_w x in_h (0 = no scaling), the filter
    int src_fmt = 0, src_colour = 0;          // vp8hip_set_source_format (0 = I420), vp8hip_set_source_colour
    int src_transfer = 0, src_peak = 0;       // vp8hip_set_source_transfer (0 = off, and no peak)
    bool win_on = false;                      // vp8hip_set_source_window: rows win_pitch[p] apart, the frame at (win_x, win_y)
    int32_t win_pitch[3] = {0, 0, 0};
    int win_x = 0, win_y = 0;
    int or_turns = 0, or_mirror = 0;          // vp8hip_set_source_orientation
    int di_mode = 0, di_keep = 0;             // vp8hip_set_deinterlace (0 = off, and no parity)
    // vp8hip_set_canvas: the frame is composed of n_tiles scaled sources (0 = no canvas) over the background bg (Y, U, V)
    int n_tiles = 0, bg[3] = {0, 0, 0};
    vp8hip_tile tile[VP8HIP_MAX_TILES] = {};
};
inline bool operator==(const vp8hip_tile &a, const vp8hip_tile &b) {
    return a.in_w == b.in_w && a.in_h == b.in_h && a.x == b.x && a.y == b.y && a.w == b.w && a.h == b.h && a.filter == b.filter;
}
inline bool same_canvas(const SourceShape &a, const SourceShape &b) {
    if (a.n_tiles != b.n_tiles || a.bg[0] != b.bg[0] || a.bg[1] != b.bg[1] || a.bg[2] != b.bg[2]) return false;
    for (int k = 0; k < VP8HIP_MAX_TILES; ++k)
        if (!(a.tile[k] == b.tile[k])) return false;
    return true;
}
inline bool operator==(const SourceShape &a, const SourceShape &b) {
    return a.src_w == b.src_w && a.src_h == b.src_h && a.in_w == b.in_w && a.in_h == b.in_h && a.scale_kind == b.scale_kind &&
           a.src_fmt == b.src_fmt && a.src_colour == b.src_colour && a.src_transfer == b.src_transfer && a.src_peak == b.src_peak &&
           a.win_on == b.win_on && a.win_pitch[0] == b.win_pitch[0] && a.win_pitch[1] == b.win_pitch[1] && a.win_pitch[2] == b.win_pitch[2] &&
           a.win_x == b.win_x && a.win_y == b.win_y && a.or_turns == b.or_turns && a.or_mirror == b.or_mirror &&
           a.di_mode == b.di_mode && a.di_keep == b.di_keep && same_canvas(a, b);
}
// ... and the switches behind it, which work on the coded surface.
struct IntakeSettings : SourceShape {
    int dn_level = 0;                         // vp8hip_set_denoise (0 = off)
    bool an_on = false;                       // vp8hip_set_analysis
    int seg_mode = 0, seg_strength = 0;       // vp8hip_set_segment_mode (the strength is mode 2's)
};
inline bool operator==(const IntakeSettings &a, const IntakeSettings &b) {
    return static_cast<const SourceShape &>(a) == static_cast<const SourceShape &>(b) && a.dn_level == b.dn_level && a.an_on == b.an_on &&
           a.seg_mode == b.seg_mode && a.seg_strength == b.seg_strength;
}

// The canonical form, which every setter hands to intake_apply: a field whose switch is off holds 0, so equal behaviour is equal bytes.
inline IntakeSettings canonical(IntakeSettings s, int W, int H) {
    if (s.src_w == W && s.src_h == H) s.src_w = s.src_h = 0;
    if (!s.in_w && !s.in_h) s.scale_kind = 0;
    if (!s.src_transfer) s.src_peak = 0;
    if (!s.win_on) s.win_pitch[0] = s.win_pitch[1] = s.win_pitch[2] = s.win_x = s.win_y = 0;
    if (!s.di_mode) s.di_keep = 0;
    if (s.n_tiles <= 0) s.n_tiles = s.bg[0] = s.bg[1] = s.bg[2] = 0;
    for (int k = s.n_tiles < VP8HIP_MAX_TILES ? s.n_tiles : VP8HIP_MAX_TILES; k < VP8HIP_MAX_TILES; ++k) s.tile[k] = vp8hip_tile{};
    if (s.seg_mode != 2) s.seg_strength = 0;
    return s;
}

// the picture inside the coded surface: the source size, or the coded size
inline void picture_size(const SourceShape &s, int W, int H, int *w, int *h) { *w = s.src_w ? s.src_w : W; *h = s.src_h ? s.src_h : H; }
// size of the UPRIGHT frame taken in: the incoming size of the scaler, or the picture
inline void upright_size(const SourceShape &s, int W, int H, int *w, int *h) {
    picture_size(s, W, H, w, h);
    if (s.in_w) { *w = s.in_w; *h = s.in_h; }
}
// size of the planes handed in (what the window, the converter and the deinterlacer work at): the upright size, width and height
// traded under an odd number of quarter turns
inline void incoming_size(const SourceShape &s, int W, int H, int *w, int *h) {
    if (s.or_turns & 1) upright_size(s, W, H, h, w);
    else upright_size(s, W, H, w, h);
}
// bytes of those planes in the source format (I420: ny, nc, nc)
inline void incoming_bytes(const SourceShape &s, int W, int H, size_t bytes[3]) {
    int w, h;
    incoming_size(s, W, H, &w, &h);
    (void)vp8host_source_plane_bytes(s.src_fmt, w, h, bytes);
}
// vp8host_source_window for the window, format and incoming size in force
inline int window_rule(const SourceShape &s, int W, int H, size_t off[3], int32_t row_bytes[3], int32_t rows[3]) {
    int w, h;
    incoming_size(s, W, H, &w, &h);
    return vp8host_source_window(s.src_fmt, w, h, s.win_x, s.win_y, s.win_pitch, off, row_bytes, rows);
}

// a stage in front of the pack or scale launch reads the planes: they must be in device memory by then
inline bool needs_device_planes(const SourceShape &s) { return s.src_fmt || s.di_mode || s.in_w || s.win_on || s.or_turns || s.or_mirror; }
// what a context must not have for a hidden alt-ref frame (vp8hip_arf_filter_*), and to split its frames over devices (vp8hip_shard_init)
inline bool excludes_arf(const IntakeSettings &s) { return s.src_fmt || s.win_on || s.di_mode || s.dn_level || s.an_on || s.n_tiles; }
inline bool excludes_shard(const IntakeSettings &s) { return s.an_on || s.seg_mode || s.n_tiles; }
// ... and to be a member of a batch (vp8hip_batch_create): a canvas takes several sources per frame, a batch's ways in take one
inline bool excludes_batch(const IntakeSettings &s) { return s.n_tiles != 0; }

// dst of a scaler, or the source size: even, not above the coded size and fewer than 16 below it
inline bool source_size_ok(int W, int H, int w, int h) {
    return w > 0 && h > 0 && !(w & 1) && !(h & 1) && w <= W && h <= H && W - w < 16 && H - h < 16;
}

// THE RULE: may a context of coded size W x H have these settings, all of them together?  INTAKE_OK or INTAKE_REFUSED.
inline int intake_valid(int W, int H, const IntakeSettings &s) {
    int pw, ph, w, h;
    picture_size(s, W, H, &pw, &ph);
    if ((s.src_w || s.src_h) && !source_size_ok(W, H, s.src_w, s.src_h)) return INTAKE_REFUSED;
    if ((s.in_w || s.in_h) && ((s.scale_kind != 0 && s.scale_kind != 1) || (s.in_w & 1) || (s.in_h & 1) || s.in_w < pw || s.in_h < ph ||
                               s.in_w > 16384 || s.in_h > 16384))
        return INTAKE_REFUSED;
    if (s.src_fmt < 0 || (s.src_fmt >= VP8HOST_FORMAT_COUNT && s.src_fmt < VP8HOST_FORMAT_PACKED_FIRST) || s.src_fmt >= VP8HOST_FORMAT_PACKED_END)
        return INTAKE_REFUSED;
    if (s.src_colour < 0 || s.src_colour >= VP8HOST_COLOUR_COUNT) return INTAKE_REFUSED;
    if (s.src_transfer != VP8HOST_TRANSFER_SDR && s.src_transfer != VP8HOST_TRANSFER_PQ && s.src_transfer != VP8HOST_TRANSFER_HLG) return INTAKE_REFUSED;
    // (the tone-mapping rule reads P010 and I010, and I420 frames pass it by)
    if (s.src_transfer && (s.src_peak < VP8HOST_PEAK_MIN || s.src_peak > VP8HOST_PEAK_MAX ||
                           (s.src_fmt != VP8HOST_FORMAT_I420 && s.src_fmt != VP8HOST_FORMAT_P010 && s.src_fmt != VP8HOST_FORMAT_I010)))
        return INTAKE_REFUSED;
    if (s.or_turns < 0 || s.or_turns > 3 || (s.or_mirror != 0 && s.or_mirror != 1)) return INTAKE_REFUSED;
    incoming_size(s, W, H, &w, &h);
    size_t off[3];
    int32_t rb[3], rows[3];
    if (s.win_on && window_rule(s, W, H, off, rb, rows) != 0) return INTAKE_REFUSED;      // (the window fits its pitches at the raw size, in this format)
    if (s.di_mode < 0 || s.di_mode > 2 || (s.di_keep != 0 && s.di_keep != 1) || (s.di_mode && h < 4)) return INTAKE_REFUSED;   // (every plane needs a row of each field)
    // a canvas: the frame is composed of its tiles, 8-bit I420 each, scaled and placed by k_compose_b in the place of the pack or scale
    // launch -- so nothing else stands in front of that launch, both ways round
    if (s.n_tiles < 0 || s.n_tiles > VP8HIP_MAX_TILES) return INTAKE_REFUSED;
    if (s.n_tiles) {
        if (s.in_w || s.in_h || s.src_fmt || s.win_on || s.or_turns || s.or_mirror || s.di_mode) return INTAKE_REFUSED;
        if (((s.bg[0] | s.bg[1] | s.bg[2]) & ~255) != 0) return INTAKE_REFUSED;
        for (int k = 0; k < s.n_tiles; ++k)
            if (!vp8host_tile_valid(pw, ph, &s.tile[k])) return INTAKE_REFUSED;
    }
    if (s.dn_level < 0 || s.dn_level > 3 || s.seg_mode < 0 || s.seg_mode > 2 || (s.seg_mode == 2 && (s.seg_strength < 1 || s.seg_strength > 3))) return INTAKE_REFUSED;
    return INTAKE_OK;
}

}  // namespace vp8

#endif
