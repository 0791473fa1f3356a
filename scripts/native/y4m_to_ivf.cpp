// y4m_to_ivf.cpp -- the reference's program with the path swapped in, as a complete C++ user of the C ABI: YUV4MPEG2 in,
// IVF out (main() of src/vp8enc.cpp reduced to: parse the header, per frame read / code / write, patch the frame count).
//   y4m_to_ivf <in.y4m> <out.ivf> [-g gop] [-partitions P] [-qmin q] [-qmax q] [-SSIM-target t] [-altref-range n] [-no-scene-detect]
//              [-no-check-ssim] [-conformant] [-simple-filter] [-psnr] [-resize WxH] [-resize-filter area|lanczos] [-denoise N] [-aq N]
//              [-input-format NAME] [-input-transfer pq|hlg[:PEAK]] [-overlay FILE:WxH:X:Y[:OPACITY]] [-analysis FILE] [-deinterlace field|adaptive[:top|bottom]] [-crop W:H:X:Y] [-rotate 0|90|180|270] [-mirror]
//              [-arf PERIOD[:FRAMES[:STRENGTH]]] [-temporal-layers N] [-intra-refresh N]
// -intra-refresh N (4..1024): cyclic intra refresh (vp8drv_set_intra_refresh; the rule: include/vp8hip_host.h,
// vp8host_intra_refresh_forced): a few macroblocks of every inter frame that refreshes LAST are coded as intra, in a pattern that covers
// the picture every N such frames, so that a receiver that lost a frame heals without a key frame.  The forced share of all macroblocks
// is printed next to -psnr's summary.  Not with an -SSIM-target above -1.
// -temporal-layers N (1..3): a stream of N temporal layers (vp8drv_set_temporal_layers; the rule: include/vp8hip_host.h,
// vp8host_temporal_step), which still decodes when every frame above a layer is dropped.  The option sets -altref-range to the GOP
// size + 1 (scheduled alt-refs off), turns the overlapped loop filter off and with it the early hand-over of the next frame: this mode
// is a plain loop too (read, code, take the bytes, write).  The frames per layer are printed next to the summary.  Not with -arf.
// -arf PERIOD[:FRAMES[:STRENGTH]] (FRAMES 1..7, default 7; STRENGTH 0..6, default 3): hidden alternate reference frames
// (vp8drv_set_arf, vp8drv_encode_arf_host; libvpx's --auto-alt-ref=1 --arnr-maxframes --arnr-strength).  In front of the first frame of
// every group of PERIOD frames of a GOP -- behind the key frame for the GOP's first group -- a hidden frame is coded, made by temporal
// filtering of FRAMES frames centred on the group's last frame, the window clipped to the GOP and the file.  It is an IVF record of its own
// with the timestamp of the next shown frame, and the file header's frame count includes it.  The option reads ahead, so this mode is a
// plain loop (no reader thread, no frame handed over early, the filter on the frame's own stream); scene detection works as without
// the option, and a key frame it or check_SSIM makes starts the GOP the windows are clipped to; it composes with
// -resize, -rotate, -mirror, -aq, -psnr and the quantiser options and refuses -denoise, -deinterlace, -analysis, -crop and any format
// but 8-bit I420.
// -crop W:H:X:Y (ffmpeg's order): the Y4M header gives the SURFACE, the crop the window of it that is the frame (vp8drv_set_source_window:
// W, H, X, Y even; the pitch is the surface's tight pitch) and so the size that comes in; the whole surface is read from the file, only
// the window travels to the device.  -rotate N: the frames are stored sideways or upside down and are turned clockwise by N degrees on
// the device; -mirror: flipped left-right first (vp8drv_set_source_orientation).  Behind 90 or 270 degrees the picture that is coded,
// and that -resize scales, is as wide as the frames that come in are high.  They compose with -resize, -deinterlace (fields are rows of
// the frames as stored), -denoise and -input-format.
// -deinterlace: interlaced frames are made progressive on the device (vp8drv_set_deinterlace; the rule: include/vp8hip_host.h), field =
// every missing row interpolated, adaptive = what stands still is woven.  :top / :bottom names the field that is kept; without it that
// is the FIRST field of the header's I tag (It: top, Ib: bottom; vp8host_y4m_interlace), and top, with a line on stderr, for a file
// that says it is progressive or says nothing.  An Im (mixed) file is refused.  Without the option nothing changes, whatever the tag
// says.  The share of missing samples that were woven is printed at the end, next to -psnr's summary.
// -analysis FILE: the frame analysis record of every frame (vp8drv_set_analysis; the rules: include/vp8hip_host.h) as one text line per
// frame, the first-pass file a caller's second pass reads.  Decimal integers separated by single spaces, in this order:
//   frame_number is_key bytes have_prev static_mbs spatial temporal_sse temporal_sad coded mbs_total mbs_intra mbs_split mbs_zero_mv
//   mbs_no_coeffs mbs_ref[0..2] segment_mbs[0..3] mv_abs_sum[0..1] mv_sum[0..1] mv_sq_sum nz_coeffs
// (bytes = the size of the coded frame in the IVF file; the .ivf is the one written without the option).
// The format of the frames is the header's C tag (vp8host_y4m_colourspace): C420* files are I420, C422, C444, C420p10, C422p10 and
// C444p10 files are converted on the device (vp8drv_set_source_format), any other colourspace is refused.  -input-format NAME (i420,
// nv12, i422, i444, p010, i010, i210, i410) says it instead of the tag: for frames the header cannot describe (NV12, P010).
// -input-transfer pq|hlg[:PEAK]: the ten-bit frames carry a PQ (HDR10) or HLG signal in BT.2020, graded for PEAK nits (400..10000,
// default 1000), and are tone-mapped to SDR on the device (vp8drv_set_source_transfer; the rule: include/vp8hip_host.h).  A Y4M header
// carries neither transfer nor primaries, so the option says it.  It goes with C420p10 files only (their frames read as i010, or as
// p010 with -input-format); any other file is refused with its tag named.
// -overlay FILE:WxH:X:Y[:OPACITY]: FILE holds W x H pixels of raw BGRA, tight, straight alpha; the layer is burnt into every frame on the
// device with its top-left pixel at (X, Y) of the coded picture (any integers, odd and negative ones included) at OPACITY 0..255
// (default 255), read with BT.601 limited range (vp8drv_set_overlay_host; the rule: include/vp8hip_host.h).  Up to four times: the
// layers are applied in the order they appear.
// -aq N: variance-adaptive quantisation of the inter frames at strength N = 1, 2, 3 (vp8drv_set_segment_mode, mode 2; 0 = off): flat
// macroblocks take the finer segments of the quantiser ladder, busy ones the coarser.
// -denoise N: temporal noise reduction of the source frames on the device, N = 1, 2, 3 (vp8drv_set_denoise; 0 = off); the share of
// macroblocks it filtered is printed at the end, next to -psnr's summary.
// -resize: the Y4M header gives the size of the frames that come in, WxH (even, not above it) the picture that is coded: the frames are
// scaled down on the device (cfg.in_width / in_height, vp8hip_set_source_scaling); IVF header and key frames carry WxH.
// As in the reference, check_SSIM runs after every inter frame and scene_change() looks at every frame that would be an inter frame.
// Everything between the two files runs behind include/vp8hip_driver.h; the frames are handed over at their source size
// and padded on the device (cfg.src_width / src_height), key frames carry that size as the display size.
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <strings.h>
#include <chrono>
#include <condition_variable>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "vp8hip_bitstream.h"
#include "vp8hip_driver.h"
#include "vp8hip_host.h"

#define CK(x) do { int rc_ = (x); if (rc_ < 0) { fprintf(stderr, "%s -> %d (%s)\n", #x, rc_, vp8hip_status_string(rc_)); return 1; } } while (0)

int main(int argc, char **argv) {
    if (argc < 3) { fprintf(stderr, "usage: see the head of y4m_to_ivf.cpp\n"); return 2; }
    vp8drv_config cfg;
    vp8drv_default_config(&cfg);
    cfg.scene_detect = 1;                       // main() calls scene_change() for every would-be inter frame (vp8enc.cpp:408)
    cfg.overlap_filter = 1;
    int rw = 0, rh = 0;      // -resize: the size of the coded picture (0 = the file's)
    int denoise = 0;         // -denoise
    int aq = 0;              // -aq
    int deint = 0, field = -1;      // -deinterlace: the mode, and the field kept (-1: the first field of the header's I tag)
    int32_t format = -1;     // -input-format (-1: the header's C tag)
    // -overlay FILE:WxH:X:Y[:OPACITY]: raw BGRA bytes, tight, burnt into every frame; slots in order of appearance, matrix 0
    struct Overlay { int w = 0, h = 0, x = 0, y = 0, opacity = 255; std::vector<uint8_t> pixels; };
    std::vector<Overlay> overlays;
    int transfer = 0, peak = 1000;  // -input-transfer: PQ or HLG ten-bit frames are tone-mapped to SDR on the device
    int crop[4] = {0, 0, 0, 0};     // -crop: W, H, X, Y (W == 0: the whole surface)
    int turns = 0, mirror = 0;      // -rotate, -mirror
    const char *analysis_path = nullptr;      // -analysis
    int arf_period = 0, arf_frames = 7, arf_strength = 3;      // -arf
    int layers = 0;          // -temporal-layers (0: the option was not given)
    int refresh = 0;         // -intra-refresh (0: off)
    static const char *const format_names[VP8HOST_FORMAT_COUNT] = {"i420", "nv12", "i422", "i444", "p010", "i010", "i210", "i410"};
    for (int i = 3; i < argc; ++i) {
        auto val = [&]() { return i + 1 < argc ? argv[++i] : "0"; };
        if (!strcmp(argv[i], "-g")) cfg.gop_size = atoi(val());
        else if (!strcmp(argv[i], "-partitions")) cfg.num_partitions = atoi(val());
        else if (!strcmp(argv[i], "-qmin")) cfg.qi_min = atoi(val());
        else if (!strcmp(argv[i], "-qmax")) cfg.qi_max = atoi(val());
        else if (!strcmp(argv[i], "-SSIM-target")) cfg.ssim_target = (float)atof(val());
        else if (!strcmp(argv[i], "-altref-range")) cfg.altref_range = atoi(val());
        else if (!strcmp(argv[i], "-scene-detect")) cfg.scene_detect = 1;
        else if (!strcmp(argv[i], "-no-scene-detect")) cfg.scene_detect = 0;
        else if (!strcmp(argv[i], "-no-check-ssim")) cfg.check_ssim = 0;
        else if (!strcmp(argv[i], "-conformant")) cfg.conformant_stream = 1;
        else if (!strcmp(argv[i], "-simple-filter")) cfg.loop_filter_type = 1;   // RFC 6386 section 15.2
        else if (!strcmp(argv[i], "-psnr")) cfg.quality_stats = 1;               // PSNR / SSIM summary on stderr
        else if (!strcmp(argv[i], "-denoise")) denoise = atoi(val());
        else if (!strcmp(argv[i], "-aq")) aq = atoi(val());
        else if (!strcmp(argv[i], "-analysis")) analysis_path = val();
        else if (!strcmp(argv[i], "-deinterlace")) {
            const char *f = val(), *colon = strchr(f, ':');
            const size_t len = colon ? (size_t)(colon - f) : strlen(f);
            if (len == 5 && !strncmp(f, "field", 5)) deint = 1;
            else if (len == 8 && !strncmp(f, "adaptive", 8)) deint = 2;
            if (colon && !strcmp(colon + 1, "top")) field = 0;
            else if (colon && !strcmp(colon + 1, "bottom")) field = 1;
            if (!deint || (colon && field < 0)) { fprintf(stderr, "-deinterlace field|adaptive[:top|bottom]\n"); return 2; }
        }
        else if (!strcmp(argv[i], "-input-format")) {
            const char *f = val();
            for (int k = 0; k < VP8HOST_FORMAT_COUNT; ++k)
                if (!strcasecmp(f, format_names[k])) format = k;
            if (format < 0) { fprintf(stderr, "-input-format %s: one of i420 nv12 i422 i444 p010 i010 i210 i410\n", f); return 2; }
        }
        else if (!strcmp(argv[i], "-input-transfer")) {
            const char *f = val(), *colon = strchr(f, ':');
            const size_t len = colon ? (size_t)(colon - f) : strlen(f);
            if (len == 2 && !strncasecmp(f, "pq", 2)) transfer = VP8HOST_TRANSFER_PQ;
            else if (len == 3 && !strncasecmp(f, "hlg", 3)) transfer = VP8HOST_TRANSFER_HLG;
            if (colon) peak = atoi(colon + 1);
            if (!transfer || peak < VP8HOST_PEAK_MIN || peak > VP8HOST_PEAK_MAX) { fprintf(stderr, "-input-transfer pq|hlg[:PEAK], PEAK 400..10000 nits\n"); return 2; }
        }
        else if (!strcmp(argv[i], "-overlay")) {
            Overlay o;
            const char *f = val(), *colon = strchr(f, ':');
            if (!colon || sscanf(colon + 1, "%dx%d:%d:%d:%d", &o.w, &o.h, &o.x, &o.y, &o.opacity) < 4 || o.w < 1 || o.h < 1 || o.w > VP8HOST_OVERLAY_MAX_SIZE ||
                o.h > VP8HOST_OVERLAY_MAX_SIZE || o.opacity < 0 || o.opacity > 255 || overlays.size() == VP8HIP_MAX_OVERLAYS) {
                fprintf(stderr, "-overlay FILE:WxH:X:Y[:OPACITY], OPACITY 0..255, at most %d times\n", VP8HIP_MAX_OVERLAYS);
                return 2;
            }
            const std::string path(f, (size_t)(colon - f));
            FILE *lf = fopen(path.c_str(), "rb");
            o.pixels.resize((size_t)o.w * o.h * 4);
            if (!lf || fread(o.pixels.data(), 1, o.pixels.size(), lf) != o.pixels.size()) { fprintf(stderr, "-overlay %s: not %d x %d x 4 bytes of BGRA\n", path.c_str(), o.w, o.h); return 2; }
            fclose(lf);
            overlays.push_back(std::move(o));
        }
        else if (!strcmp(argv[i], "-crop")) {
            if (sscanf(val(), "%d:%d:%d:%d", &crop[0], &crop[1], &crop[2], &crop[3]) != 4 || crop[0] <= 0 || crop[1] <= 0) { fprintf(stderr, "-crop W:H:X:Y\n"); return 2; }
        }
        else if (!strcmp(argv[i], "-rotate")) {
            const int deg = atoi(val());
            if (deg != 0 && deg != 90 && deg != 180 && deg != 270) { fprintf(stderr, "-rotate 0|90|180|270\n"); return 2; }
            turns = deg / 90;
        }
        else if (!strcmp(argv[i], "-mirror")) mirror = 1;
        else if (!strcmp(argv[i], "-arf")) {
            const int k = sscanf(val(), "%d:%d:%d", &arf_period, &arf_frames, &arf_strength);
            if (k < 1 || arf_period < 1 || arf_frames < 1 || arf_frames > VP8HOST_ARF_MAX_FRAMES || arf_strength < 0 || arf_strength > 6) {
                fprintf(stderr, "-arf PERIOD[:FRAMES[:STRENGTH]]: PERIOD >= 1, FRAMES 1..7, STRENGTH 0..6\n");
                return 2;
            }
        }
        else if (!strcmp(argv[i], "-temporal-layers")) {
            layers = atoi(val());
            if (layers < 1 || layers > 3) { fprintf(stderr, "-temporal-layers 1..3\n"); return 2; }
        }
        else if (!strcmp(argv[i], "-intra-refresh")) {
            refresh = atoi(val());
            if (refresh < VP8HOST_INTRA_REFRESH_MIN || refresh > VP8HOST_INTRA_REFRESH_MAX) { fprintf(stderr, "-intra-refresh 4..1024\n"); return 2; }
        }
        else if (!strcmp(argv[i], "-resize")) { if (sscanf(val(), "%dx%d", &rw, &rh) != 2) { fprintf(stderr, "-resize WxH\n"); return 2; } }
        else if (!strcmp(argv[i], "-resize-filter")) {
            const char *f = val();
            if (!strcmp(f, "area")) cfg.scale_filter = 0;
            else if (!strcmp(f, "lanczos")) cfg.scale_filter = 1;
            else { fprintf(stderr, "-resize-filter area|lanczos\n"); return 2; }
        }
        else { fprintf(stderr, "unknown option %s\n", argv[i]); return 2; }
    }
    if (arf_period) {
        if (denoise || deint || analysis_path || crop[0] || !overlays.empty()) { fprintf(stderr, "-arf does not go with -denoise, -deinterlace, -analysis, -crop or -overlay\n"); return 2; }
        cfg.overlap_filter = 0;    // (the next frame's ALTREF search would start beside the filter that writes ALTREF; the key frames stay where they are without the option)
        fprintf(stderr, "-arf: the loop filter runs on the frame's own stream in this mode (no frame is handed over early)\n");
    }
    if (layers) {
        if (arf_period) { fprintf(stderr, "-temporal-layers does not go with -arf (layers never search ALTREF)\n"); return 2; }
        cfg.altref_range = cfg.gop_size + 1;      // scheduled alt-refs off
        cfg.overlap_filter = 0;                   // (the next frame's GOLDEN search would start beside the filter that writes GOLDEN)
        fprintf(stderr, "-temporal-layers: the loop filter runs on the frame's own stream in this mode (no frame is handed over early)\n");
    }
    if (refresh && cfg.ssim_target > -1.0f) { fprintf(stderr, "-intra-refresh does not go with an -SSIM-target above -1 (the SSIM ladder owns the intra fallback)\n"); return 2; }
    FILE *in = fopen(argv[1], "rb");
    if (!in) { perror(argv[1]); return 1; }
    uint8_t head[256];
    const size_t got = fread(head, 1, sizeof head, in);
    int32_t W = 0, H = 0, fps = 0;
    size_t first = 0;
    if (vp8host_y4m_parse_header(head, got, &W, &H, &fps, &first) != 0 || (W & 1) || (H & 1)) {
        fprintf(stderr, "%s: not a YUV4MPEG2 stream the reference accepts\n", argv[1]);
        return 1;
    }
    // the header's C tag by name: what follows the first " C" of the header line
    const uint8_t *line_end = static_cast<const uint8_t *>(memchr(head, '\n', got));
    const size_t line_len = line_end ? (size_t)(line_end - head) : got;
    size_t tag_a = 0;
    while (tag_a + 1 < line_len && !(head[tag_a] == ' ' && head[tag_a + 1] == 'C')) ++tag_a;
    size_t tag_b = tag_a + 1;
    while (tag_b < line_len && head[tag_b] != ' ') ++tag_b;
    const bool has_tag = tag_a + 1 < line_len;
    const int tag_len = has_tag ? (int)(tag_b - tag_a - 1) : 7;
    const char *tag = has_tag ? reinterpret_cast<const char *>(head + tag_a + 1) : "(no C)";
    if (transfer) {      // ten-bit 4:2:0 and nothing else carries a PQ or HLG signal this encoder maps
        int32_t tagged = -1;
        if (vp8host_y4m_colourspace(head, got, &tagged) != 0 || tagged != VP8HOST_FORMAT_I010 || !has_tag ||
            (format >= 0 && format != VP8HOST_FORMAT_I010 && format != VP8HOST_FORMAT_P010)) {
            fprintf(stderr, "%s: -input-transfer goes with C420p10 files only (frames as i010 or p010), not with colourspace tag %.*s%s%s\n", argv[1], tag_len, tag,
                    format >= 0 ? " read as " : "", format >= 0 ? format_names[format] : "");
            return 2;
        }
    }
    if (format < 0 && vp8host_y4m_colourspace(head, got, &format) != 0) {
        fprintf(stderr, "%s: colourspace tag %.*s is not one this encoder takes (C420*, C422, C444, C420p10, C422p10, C444p10)\n", argv[1],
                has_tag ? tag_len : 1, has_tag ? tag : "?");
        return 1;
    }
    if (deint) {
        int32_t order = 0;
        if (vp8host_y4m_interlace(head, got, &order) != 0) {
            fprintf(stderr, "%s: interlace tag Im (mixed) or unknown: not a field order -deinterlace can follow (Ip, I?, It, Ib)\n", argv[1]);
            return 1;
        }
        if (field < 0) {
            if (order == VP8HOST_FIELDS_PROGRESSIVE) fprintf(stderr, "%s: no field order in the header: -deinterlace keeps the top field\n", argv[1]);
            field = order == VP8HOST_FIELDS_BOTTOM_FIRST ? 1 : 0;
        }
    }
    fseek(in, (long)first, SEEK_SET);
    // video.src_* is the file's size, video.dst_* the picture that is coded and displayed (-resize; the file's without it), video.wrk_* that
    // rounded up to whole macroblocks (init.h:375-392).  The frames are handed over as the file has them: scaled and padded on the device.
    // -crop: the file's frames are surfaces and the window is what comes in; -rotate: the upright picture trades its sides
    int32_t pitch[3] = {0, 0, 0};
    if (crop[0]) {
        const int32_t any[3] = {INT32_MAX, INT32_MAX, INT32_MAX};
        size_t off[3];
        int32_t rows[3];
        if (vp8host_source_window(format, W, H, 0, 0, any, off, pitch, rows) != 0 ||      // (row_bytes of the whole surface: its tight pitch)
            vp8host_source_window(format, crop[0], crop[1], crop[2], crop[3], pitch, off, rows, rows) != 0 || crop[3] + crop[1] > H) {
            fprintf(stderr, "-crop %d:%d:%d:%d: even numbers, and a window inside the file's %dx%d\n", crop[0], crop[1], crop[2], crop[3], W, H);
            return 2;
        }
    }
    const int Wraw = crop[0] ? crop[0] : W, Hraw = crop[0] ? crop[1] : H;
    const int Win = (turns & 1) ? Hraw : Wraw, Hin = (turns & 1) ? Wraw : Hraw;      // the upright frame that comes in
    const int Wd = rw ? rw : Win, Hd = rh ? rh : Hin;
    if (Wd < 2 || Hd < 2 || (Wd & 1) || (Hd & 1) || Wd > Win || Hd > Hin) { fprintf(stderr, "-resize %dx%d: even, and not above the incoming %dx%d\n", Wd, Hd, Win, Hin); return 2; }
    const int Wc = (Wd + 15) / 16 * 16, Hc = (Hd + 15) / 16 * 16;
    if (Wc != Wd || Hc != Hd) { cfg.src_width = Wd; cfg.src_height = Hd; }
    if (Wd != Win || Hd != Hin) { cfg.in_width = Win; cfg.in_height = Hin; }
    vp8drv *drv = nullptr;
    CK(vp8drv_create(&drv, Wc, Hc, 0, &cfg));
    if (denoise) CK(vp8drv_set_denoise(drv, denoise));
    if (aq) CK(vp8drv_set_segment_mode(drv, 2, aq));
    if (format) CK(vp8drv_set_source_format(drv, format));
    if (transfer) CK(vp8drv_set_source_transfer(drv, transfer, peak));
    for (size_t k = 0; k < overlays.size(); ++k)
        CK(vp8drv_set_overlay_host(drv, (int)k, VP8HOST_FORMAT_BGRA, 0, overlays[k].pixels.data(), overlays[k].w, overlays[k].h, 4 * overlays[k].w, overlays[k].x, overlays[k].y, overlays[k].opacity));
    if (turns || mirror) CK(vp8drv_set_source_orientation(drv, turns, mirror));
    if (crop[0]) CK(vp8drv_set_source_window(drv, pitch, crop[2], crop[3]));
    if (deint) CK(vp8drv_set_deinterlace(drv, deint, field));
    if (layers) CK(vp8drv_set_temporal_layers(drv, layers, 0));
    if (refresh) CK(vp8drv_set_intra_refresh(drv, refresh));
    uint32_t per_layer[3] = {0, 0, 0}, unfiltered = 0;
    long long dn_filtered = 0, dn_total = 0, di_woven = 0, di_missing = 0;
    FILE *analysis = nullptr;
    vp8drv_analysis an{};      // the record of the frame whose bytes are still to be taken
    if (analysis_path) {
        CK(vp8drv_set_analysis(drv, 1));
        analysis = fopen(analysis_path, "w");
        if (!analysis) { perror(analysis_path); return 1; }
    }
    FILE *out = fopen(argv[2], "wb");
    if (!out) { perror(argv[2]); return 1; }
    uint8_t fh[32];
    fwrite(fh, 1, vp8bs_ivf_file_header(fh, Wd, Hd, (uint32_t)(fps ? fps : 30), 1, 0), out);     // frame count patched at the end (encIO.h:100-139)
    size_t nb[3];            // the planes of a frame as the file has them (nb[2] == 0: two planes, the third pointer is the second again)
    if (vp8host_source_plane_bytes(format, W, H, nb) != 0) { fprintf(stderr, "%dx%d: not a frame size of format %s\n", W, H, format_names[format]); return 1; }
    std::vector<uint8_t> bytes((size_t)(Wc / 16) * (Hc / 16) * 1900 + (1 << 20));
    if (arf_period) {      // the plain loop with a lookahead
        if (format) { fprintf(stderr, "-arf takes 8-bit I420 frames only\n"); return 2; }
        CK(vp8drv_set_arf(drv, arf_strength + 1));
        const size_t fsz = nb[0] + nb[1] + nb[2];
        std::vector<std::vector<uint8_t>> ahead;      // frames first .. first + ahead.size() - 1 of the file
        long first_held = 0;
        bool eof = false;
        auto have = [&](long idx) -> bool {           // frame idx is in memory (reads up to it); false: the file ends before it
            while (!eof && first_held + (long)ahead.size() <= idx) {
                std::vector<uint8_t> f(fsz);
                uint8_t marker[6];
                if (fread(f.data(), 1, fsz, in) != fsz) { eof = true; break; }
                const size_t k = fread(marker, 1, 6, in);
                if (k > 0 && !vp8host_y4m_frame_marker_ok(marker)) { fprintf(stderr, "broken stream!\n"); eof = true; break; }
                ahead.push_back(std::move(f));
            }
            return idx < first_held + (long)ahead.size();
        };
        auto frame = [&](long idx) { return ahead[(size_t)(idx - first_held)].data(); };
        uint32_t records = 0, shown = 0, hidden = 0, keys = 0;
        size_t total = 32;
        auto write_record = [&](uint64_t timestamp) -> int {
            size_t size = 0;
            const int rc = vp8drv_get_frame(drv, bytes.data(), bytes.size(), &size);
            if (rc < 0) return rc;
            uint8_t ph[12];
            fwrite(ph, 1, vp8bs_ivf_frame_header(ph, (uint32_t)size, timestamp), out);
            fwrite(bytes.data(), 1, size, out);
            total += 12 + size;
            ++records;
            return 0;
        };
        long gop_start = 0;
        // the hidden frame of the group that starts at `group_first`, centred on the group's last frame; timestamp: the next shown frame's
        auto hidden_frame = [&](long group_first, uint64_t timestamp) -> int {
            const long gop_end = gop_start + cfg.gop_size;
            long last = group_first + arf_period - 1;
            if (last > gop_end - 1) last = gop_end - 1;
            while (last > group_first && !have(last)) --last;
            if (last == gop_start || !have(last)) return 0;      // (a group that is the key frame alone)
            long lo = last - arf_frames / 2, hi = last + arf_frames / 2;
            if (lo < gop_start) lo = gop_start;
            if (lo < first_held) lo = first_held;
            if (hi > gop_end - 1) hi = gop_end - 1;
            while (hi > last && !have(hi)) --hi;
            const uint8_t *win[VP8HOST_ARF_MAX_FRAMES][3];
            for (long k = lo; k <= hi; ++k) { win[k - lo][0] = frame(k); win[k - lo][1] = win[k - lo][0] + nb[0]; win[k - lo][2] = win[k - lo][1] + nb[1]; }
            const int rc = vp8drv_encode_arf_host(drv, win, (int)(hi - lo + 1), (int)(last - lo));
            if (rc < 0) return rc;
            ++hidden;
            return write_record(timestamp);
        };
        const auto t_loop = std::chrono::steady_clock::now();
        for (long t = 0; have(t); ++t) {
            if (t - gop_start >= cfg.gop_size) gop_start = t;      // (the schedule makes this frame a key frame)
            const long pos = t - gop_start;
            if (pos && pos % arf_period == 0) CK(hidden_frame(t, (uint64_t)t));
            const uint8_t *y = frame(t);
            CK(vp8drv_encode_frame_host(drv, y, y + nb[0], y + nb[0] + nb[1], 0));
            CK(write_record((uint64_t)t));
            const int key = vp8drv_resolve(drv);
            CK(key);
            keys += key;
            ++shown;
            if (key) {      // a GOP starts here, by the schedule or because check_SSIM sent the frame back
                gop_start = t;
                CK(hidden_frame(t, (uint64_t)t + 1));
            }
            while (first_held < t - arf_frames) { ahead.erase(ahead.begin()); ++first_held; }      // (no window reaches further back than FRAMES / 2)
        }
        const double loop_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_loop).count();
        fseek(out, 0, SEEK_SET);
        fwrite(fh, 1, vp8bs_ivf_file_header(fh, Wd, Hd, (uint32_t)(fps ? fps : 30), 1, records + 1), out);      // (one more than it holds, as without the option)
        fclose(out);
        fclose(in);
        if (cfg.quality_stats) {
            vp8drv_quality_summary q;
            CK(vp8drv_get_quality_summary(drv, &q));
            fprintf(stderr, "Stream 0 PSNR (Overall/Avg/Y/U/V) %.3f %.3f %.3f %.3f %.3f  SSIM %.5f (Y %.5f)  worst frame %lld: %.3f dB  (%lld frames)\n",
                    q.psnr_all, q.psnr_avg, q.psnr[0], q.psnr[1], q.psnr[2], q.ssim_all, q.ssim[0], (long long)q.psnr_min_frame, q.psnr_min,
                    (long long)q.frames);
        }
        vp8drv_arf_stats as{};
        if (hidden) CK(vp8drv_get_arf_stats(drv, &as));
        fprintf(stderr, "Hidden alt-refs: %u, period %d, %d frames, strength %d; the last one's tiles by block weight 0 / 1 / 2: %d / %d / %d\n", hidden, arf_period,
                arf_frames, arf_strength, as.last_weight[0], as.last_weight[1], as.last_weight[2]);
        vp8drv_destroy(drv);
        printf("%s: %u shown + %u hidden frames %dx%d (coded %dx%d), %u key, %zu bytes\n", argv[2], shown, hidden, W, H, Wc, Hc, keys, total);
        printf("%.6f s of reading + coding + writing (%.1f frames/s)\n", loop_s, shown / (loop_s > 0 ? loop_s : 1));
        return 0;
    }
    // A reader thread keeps a ring of page-locked frame buffers filled ahead of the coder (get_yuv420_frame's fread, encIO.h:204-254, off the
    // frame loop's thread: 3 MB per 1080p frame is 0.4 ms of the loop's 0.5), the frame after the one under way is started on its way to the
    // device (vp8drv_prefetch_frame_host) and, once the frame just coded has its verdict and its entropy stage enqueued, handed over
    // altogether (vp8drv_stage_frame_host: the pack, scene_change()'s scan) while that frame's loop filter still has most of its time to run.
    const size_t fsz = nb[0] + nb[1] + nb[2];
    enum { RING = 6 };
    uint8_t *buf[RING];
    int state[RING];                 // get_yuv420_frame's verdict on the frame in this slot: 1 = a frame, 0 = end of stream, -1 = broken
    for (int k = 0; k < RING; ++k) CK(vp8hip_host_alloc(0, fsz, reinterpret_cast<void **>(&buf[k])));
    std::mutex m;
    std::condition_variable cv;
    size_t rd_head = 0, rd_tail = 0, rd_freed = 0;      // filled by the reader / taken by the loop / given back by the loop
    bool stop = false;
    std::thread reader([&] {
        for (;;) {
            size_t slot;
            {
                std::unique_lock<std::mutex> l(m);
                cv.wait(l, [&] { return stop || rd_head - rd_freed < RING; });
                if (stop) return;
                slot = rd_head % RING;
            }
            int st = 1;
            if (fread(buf[slot], 1, fsz, in) != fsz) st = 0;
            else {
                uint8_t marker[6];
                const size_t n = fread(marker, 1, 6, in);
                if (n > 0 && !vp8host_y4m_frame_marker_ok(marker)) st = -1;
            }
            {
                std::lock_guard<std::mutex> l(m);
                state[slot] = st;
                ++rd_head;
            }
            cv.notify_all();
            if (st != 1) return;
        }
    });
    auto stop_reader = [&] {
        { std::lock_guard<std::mutex> l(m); stop = true; }
        cv.notify_all();
        if (reader.joinable()) reader.join();
    };
    auto peek = [&](bool wait) -> int {          // the state of the next frame in the ring: 1 / 0 / -1, or 2 = not read yet (wait == false)
        std::unique_lock<std::mutex> l(m);
        if (wait) cv.wait(l, [&] { return rd_tail < rd_head; });
        return rd_tail < rd_head ? state[rd_tail % RING] : 2;
    };
    auto planes = [&](size_t seq, const uint8_t *p[3]) { p[0] = buf[seq % RING]; p[1] = p[0] + nb[0]; p[2] = nb[2] ? p[1] + nb[1] : p[1]; };
    uint32_t n = 0, keys = 0;
    size_t total = 32;
    // One video: the loop filter of a frame runs beside the next frame's input side (vp8hip_filter_overlap), and its entropy stage
    // beside both on a third stream -- so frame t + 1 is read and started BEFORE frame t's bytes are taken (vp8drv_get_frame_begin /
    // _end).  The scratch is sized for the densest frame there can be: no frame is ever coded twice.
    CK(vp8hip_reserve_frame_path_dense(vp8drv_context(drv)));
    bool pending = false;
    size_t prefetched = (size_t)-1;
    auto prefetch_next = [&]() -> int {           // the frame at the ring's rd_tail started on its way, once
        if (peek(false) != 1 || prefetched == rd_tail) return 0;
        const uint8_t *p[3];
        planes(rd_tail, p);
        prefetched = rd_tail;
        return vp8drv_prefetch_frame_host(drv, p[0], p[1], p[2]);
    };
    auto write_frame = [&](size_t size) {      // a frame's bytes as an IVF record, and its analysis line
        uint8_t ph[12];
        fwrite(ph, 1, vp8bs_ivf_frame_header(ph, (uint32_t)size, n), out);
        fwrite(bytes.data(), 1, size, out);
        total += 12 + size;
        if (analysis)
            fprintf(analysis, "%d %d %zu %d %d %llu %llu %llu %d %d %d %d %d %d %d %d %d %d %d %d %d %llu %llu %lld %lld %llu %llu\n", an.frame_number,
                    an.is_key, size, an.have_prev, an.static_mbs, (unsigned long long)an.spatial, (unsigned long long)an.temporal_sse,
                    (unsigned long long)an.temporal_sad, an.coded, an.mbs_total, an.mbs_intra, an.mbs_split, an.mbs_zero_mv, an.mbs_no_coeffs,
                    an.mbs_ref[0], an.mbs_ref[1], an.mbs_ref[2], an.segment_mbs[0], an.segment_mbs[1], an.segment_mbs[2], an.segment_mbs[3],
                    (unsigned long long)an.mv_abs_sum[0], (unsigned long long)an.mv_abs_sum[1], (long long)an.mv_sum[0], (long long)an.mv_sum[1],
                    (unsigned long long)an.mv_sq_sum, (unsigned long long)an.nz_coeffs);
        ++n;
    };
    const auto t_loop = std::chrono::steady_clock::now();      // (the frame loop by the host's clock: what scripts/drop_in_bench.py quotes as fps_loop)
    for (;;) {
        const int have = peek(true);
        if (have < 0) { fprintf(stderr, "broken stream!\n"); stop_reader(); return 1; }
        const bool got = have > 0;
        if (got) {
            const uint8_t *p[3];
            planes(rd_tail, p);
            {   // the previous frame's buffer goes back to the reader; this one is taken
                std::lock_guard<std::mutex> l(m);
                if (rd_tail > rd_freed) rd_freed = rd_tail;
                ++rd_tail;
            }
            cv.notify_all();
            CK(vp8drv_encode_frame_host(drv, p[0], p[1], p[2], 0));      // (uploads nothing if the frame was handed over early)
            if (denoise) {      // the record of the frame just taken in (its launch ended long ago)
                vp8hip_denoise_stats ds;
                CK(vp8drv_get_denoise_stats(drv, &ds));
                dn_filtered += ds.mbs_filtered;
                dn_total += ds.mbs_total;
            }
            if (deint) {
                vp8hip_deinterlace_stats is;
                CK(vp8drv_get_deinterlace_stats(drv, &is));
                di_woven += is.woven;
                di_missing += is.missing;
            }
            if (!layers) CK(prefetch_next());
        }
        if (layers && got) {      // the plain loop: this frame's bytes now, its type final behind them
            size_t size = 0;
            CK(vp8drv_get_frame(drv, bytes.data(), bytes.size(), &size));
            const int key = vp8drv_resolve(drv);
            CK(key);
            keys += key;
            if (analysis) CK(vp8drv_get_frame_analysis(drv, &an));
            vp8drv_layer_info li;
            CK(vp8drv_get_frame_layer(drv, &li));
            per_layer[li.temporal_id]++;
            unfiltered += !li.filtered;
            write_frame(size);
            continue;
        }
        if (pending) {      // the previous frame's bytes
            size_t size = 0;
            CK(vp8drv_get_frame_end(drv, bytes.data(), bytes.size(), &size));
            write_frame(size);
            pending = false;
        }
        if (!got) break;
        CK(vp8drv_get_frame_begin(drv));
        const int key = vp8drv_resolve(drv);       // the frame's final type: check_SSIM may have sent it back to be a key frame
        CK(key);
        keys += key;
        pending = true;
        if (analysis) CK(vp8drv_get_frame_analysis(drv, &an));      // (the frame's type is final; before the next frame is handed over)
        if (peek(false) == 1) {     // the next frame, early: current on the device, its scene scan under way, the one after it on its way
            const uint8_t *p[3];
            planes(rd_tail, p);
            CK(vp8drv_stage_frame_host(drv, p[0], p[1], p[2]));
        }
    }
    stop_reader();
    const double loop_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_loop).count();
    fseek(out, 0, SEEK_SET);
    // the reference's file says one frame more than it holds: write_output_header counts from a frame number that main() has
    // already advanced past the last frame (encIO.h:124-134, vp8enc.cpp:487-489; REFERENCE_DEFECTS.md #8) -- reproduced, the bar
    // being the reference's bytes
    fwrite(fh, 1, vp8bs_ivf_file_header(fh, Wd, Hd, (uint32_t)(fps ? fps : 30), 1, n + 1), out);
    fclose(out);
    fclose(in);
    if (analysis) fclose(analysis);
    vp8drv_stats st;
    vp8drv_get_stats(drv, &st);
    if (cfg.quality_stats) {   // vpxenc --psnr's summary, measured on the device (vp8drv_config.quality_stats)
        vp8drv_quality_summary q;
        CK(vp8drv_get_quality_summary(drv, &q));
        fprintf(stderr, "Stream 0 PSNR (Overall/Avg/Y/U/V) %.3f %.3f %.3f %.3f %.3f  SSIM %.5f (Y %.5f)  worst frame %lld: %.3f dB  (%lld frames)\n",
                q.psnr_all, q.psnr_avg, q.psnr[0], q.psnr[1], q.psnr[2], q.ssim_all, q.ssim[0], (long long)q.psnr_min_frame, q.psnr_min,
                (long long)q.frames);
    }
    if (denoise)
        fprintf(stderr, "Denoiser level %d: %lld of %lld macroblocks filtered (%.1f %%)\n", denoise, dn_filtered, dn_total,
                dn_total ? 100.0 * (double)dn_filtered / (double)dn_total : 0.0);
    if (deint)
        fprintf(stderr, "Deinterlacer %s, %s field kept: %lld of %lld missing luma samples woven (%.1f %%)\n", deint == 1 ? "field" : "adaptive",
                field ? "bottom" : "top", di_woven, di_missing, di_missing ? 100.0 * (double)di_woven / (double)di_missing : 0.0);
    if (refresh) {
        vp8drv_intra_refresh_info ri;
        CK(vp8drv_get_intra_refresh(drv, &ri));
        const double all = (double)n * (double)((Wc / 16) * (Hc / 16));
        fprintf(stderr, "Intra refresh period %d: %lld of %.0f macroblocks forced intra (%.2f %%)\n", refresh, (long long)ri.total_forced, all,
                all > 0 ? 100.0 * (double)ri.total_forced / all : 0.0);
    }
    vp8drv_destroy(drv);
    for (int k = 0; k < RING; ++k) vp8hip_host_free(0, buf[k]);
    printf("%s: %u frames %dx%d (coded %dx%d), %u key (%d by scene change, %d recoded), %zu bytes; %d hardware queues\n", argv[2], n, W, H, Wc, Hc, keys,
           st.scene_changes, st.redone_as_key, total, vp8hip_hw_queues());
    if (layers)
        printf("Temporal layers: %d; frames in layer 0 / 1 / 2: %u / %u / %u; %u unreferenced frames not loop-filtered\n", layers, per_layer[0], per_layer[1],
               per_layer[2], unfiltered);
    printf("%.6f s of reading + coding + writing (%.1f frames/s)\n", loop_s, n / (loop_s > 0 ? loop_s : 1));
    return 0;
}
