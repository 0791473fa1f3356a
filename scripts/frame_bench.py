#!/usr/bin/env python3
"""Whole-encoder timing: native frame loop + vp8drv_get_frame (complete VP8 frames out), one thread per GOP stream.
    python scripts/frame_bench.py [--streams N] [--frames K] [--width W --height H] [--partitions P]
--tiles LAYOUT: every frame is composed on the device of device-resident tiles (vp8drv_set_canvas, vp8drv_encode_frame_tiles_device):
letterbox = one source of the picture's size scaled to 20/27 of its height between bars (1920x1080 -> 1920x800), grid4 = four sources
of 2/3 of the picture's size scaled to its quarters (1280x720 -> 960x540), pip = a 1:1 full frame and a source of 2/3 of the picture's
size scaled to a quarter of its width and height in the bottom right corner (1280x720 -> 480x270).  --tiles-precomposed: the same
pictures composed on the host beforehand (vp8host_compose_frame) and handed over as plain frames: what the composition costs."""
import argparse, os, sys, threading, time
os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from vp8oclenc_amd import api, gop_shard
from vp8oclenc_amd.synth import SynthSequence

ap = argparse.ArgumentParser()
ap.add_argument("--streams", type=int, default=16)
ap.add_argument("--frames", type=int, default=60)
ap.add_argument("--width", type=int, default=1920)
ap.add_argument("--height", type=int, default=1080)
ap.add_argument("--partitions", type=int, default=8)
ap.add_argument("--check-ssim", type=int, default=0)
ap.add_argument("--loop-filter-type", type=int, choices=(0, 1), default=0, help="0 = the normal loop filter, 1 = the simple one")
ap.add_argument("--quality-stats", type=int, choices=(0, 1), default=0, help="1 = PSNR / SSIM of every frame on the device (vp8drv_config.quality_stats): what it costs")
ap.add_argument("--scale-from", default="", metavar="WxH", help="the frames come in at this size and are scaled down to --width x --height on the device (vp8drv_config.in_width / in_height)")
ap.add_argument("--scale-filter", choices=("area", "lanczos"), default="area")
ap.add_argument("--denoise", type=int, choices=(0, 1, 2, 3), default=0, help="temporal noise reduction of every frame taken in (vp8drv_set_denoise): what k_denoise_b costs")
ap.add_argument("--deinterlace", choices=("off", "field", "adaptive"), default="off", metavar="MODE", help="every frame taken in passes through the deinterlacer (vp8drv_set_deinterlace): what k_deinterlace_b costs")
ap.add_argument("--field", choices=("top", "bottom"), default="top", help="... the field that is kept")
ap.add_argument("--source-format", default="", metavar="NAME", help="the device-resident frames are this format's planes (nv12, p010, i444, ..., or the packed yuy2, uyvy, bgra, rgba: vp8drv_set_source_format): what k_convert_b / k_convert_packed_b costs")
ap.add_argument("--source-matrix", choices=("bt601", "bt709"), default="bt601", help="the colour matrix bgra / rgba frames are read with (vp8drv_set_source_colour)")
ap.add_argument("--source-range", choices=("limited", "full"), default="limited")
ap.add_argument("--source-transfer", choices=("pq", "hlg"), default="", help="with --source-format p010 or i010: the frames are tone-mapped to SDR on the device (vp8drv_set_source_transfer): what k_tonemap_b costs in k_convert_b's place")
ap.add_argument("--source-peak", type=int, default=1000, metavar="N", help="... the peak luminance in nits, 400..10000")
ap.add_argument("--overlay", action="append", default=[], metavar="FILE:WxH:X:Y[:OPACITY]", help="a layer of raw BGRA bytes burnt into every frame taken in (vp8drv_set_overlay_host), up to four times: what k_overlay_b costs")
ap.add_argument("--window-pitch", type=int, default=0, metavar="P", help="the device-resident frames are surfaces whose luma rows are P bytes apart (the other planes' in proportion) and the frame is the window at (0, 0) (vp8drv_set_source_window): what k_window_b costs")
ap.add_argument("--rotate", type=int, choices=(0, 90, 180, 270), default=0, help="the device-resident frames are stored turned back by this many degrees and are turned clockwise on the device (vp8drv_set_source_orientation): what k_orient_b costs; the coded bytes do not change")
ap.add_argument("--mirror", action="store_true", help="... behind a left-right flip")
ap.add_argument("--analysis", type=int, choices=(0, 1), default=0, help="1 = the frame analysis record of every frame (vp8drv_set_analysis): what k_analyse_src_b and k_analyse_mb_b cost")
ap.add_argument("--aq", type=int, choices=(0, 1, 2, 3), default=0, metavar="N", help="variance-adaptive quantisation at strength N (vp8drv_set_segment_mode, mode 2): what k_aq_map_b + k_aq_seg_b cost, and with one stream the mapped macroblock kernel next to the default's in the same run")
ap.add_argument("--arf", default="", metavar="PERIOD[:FRAMES[:STRENGTH]]", help="hidden alternate reference frames (vp8drv_set_arf, vp8drv_encode_arf_device): every stream codes one in front of every PERIOD-th frame from a window of FRAMES device-resident frames (default 7) at STRENGTH (default 3); with one stream also what k_arf_filter_b costs by HIP events")
ap.add_argument("--temporal-layers", type=int, choices=(1, 2, 3), default=1, metavar="N", help="a stream of N temporal layers (vp8drv_set_temporal_layers): with N > 1 scheduled alt-refs are off (--altref-range above the GOP) and the unreferenced frames are loop-filtered only if --check-ssim, --quality-stats or --analysis reads the filter's launch")
ap.add_argument("--intra-refresh", type=int, default=0, metavar="N", help="cyclic intra refresh with period N, 4..1024 (vp8drv_set_intra_refresh): what k_intra_refresh costs; with one stream also its launch by HIP events (VP8HIP_INTRA_REFRESH_1WAVE=1: the one-wavefront form)")
ap.add_argument("--altref-range", type=int, default=5, metavar="N", help="vp8drv_config.altref_range (default 5, the driver's); above the GOP size = no scheduled alt-refs, what --temporal-layers 2 and 3 run with: the base to compare them with")
ap.add_argument("--tiles", choices=("", "letterbox", "grid4", "pip"), default="", metavar="LAYOUT", help="compose every frame of device-resident tiles (vp8drv_set_canvas): letterbox, grid4 or pip; with one stream also what k_compose_b costs by HIP events")
ap.add_argument("--tiles-precomposed", action="store_true", help="with --tiles: the same pictures composed on the host beforehand and handed over as plain frames")
ap.add_argument("--switch-interval", type=float, default=0.0, help="sys.setswitchinterval (0 = Python's default 5 ms)")
ap.add_argument("--only", choices=("both", "on", "off"), default="both", help="which of the two legs to time")
ap.add_argument("--pipeline", action="store_true", help="one host thread: encode + get_frame_begin on every stream, then get_frame_end on every stream")
a = ap.parse_args()
if a.tiles and a.pipeline:
    sys.exit("--tiles: not with --pipeline")
if a.switch_interval > 0:
    sys.setswitchinterval(a.switch_interval)
seq = SynthSequence(a.width, a.height, seed=1)
W, H = seq.W, seq.H
mbs = (W // 16) * (H // 16)
nd = 8
scale = {}
if a.scale_from:      # the same coded size, every frame through k_scale_b instead of k_pack_b
    in_w, in_h = (int(x) for x in a.scale_from.lower().split("x"))
    seq = SynthSequence(in_w, in_h, seed=1)
    scale = dict(in_width=in_w, in_height=in_h, scale_filter=int(a.scale_filter == "lanczos"))
    if (a.width, a.height) != (W, H):
        scale.update(src_width=a.width, src_height=a.height)
    host = [[np.ascontiguousarray(p[:in_h >> (i > 0), :in_w >> (i > 0)]) for i, p in enumerate(seq.frame(t))] for t in range(nd)]
else:
    host = [list(seq.frame(t)) for t in range(nd)]
def rgb_near_i420(fmt, y, u, v):
    """a BGRA or RGBA frame (one flat uint8 plane, alpha 255) that looks like this I420 frame: the floating-point inverse of BT.601
    limited range, chroma replicated, clipped.  Not exact -- no RGB frame carries an arbitrary I420 frame -- so the coded bytes change"""
    Y = np.asarray(y, np.float32) - 16.0
    U, V = (np.repeat(np.repeat(np.asarray(p, np.float32) - 128.0, 2, axis=0), 2, axis=1) for p in (u, v))
    r, g, b = 1.164 * Y + 1.596 * V, 1.164 * Y - 0.392 * U - 0.813 * V, 1.164 * Y + 2.017 * U
    chans = (b, g, r) if fmt == api.FORMAT_BGRA else (r, g, b)
    px = np.stack([np.clip(np.rint(c), 0, 255).astype(np.uint8) for c in chans] + [np.full(Y.shape, 255, np.uint8)], axis=-1)
    return [np.ascontiguousarray(px).ravel()]


turns = a.rotate // 90
if turns or a.mirror:      # the frames as a sideways camera stored them: the orientation undone (a mirrored turn undoes itself)
    host = [api.orient_frame(turns if a.mirror else (4 - turns) & 3, int(a.mirror), f) for f in host]
fmt = api.source_format(a.source_format) if a.source_format else 0
if fmt:      # the same frames carried by the format's planes (chroma replicated, samples shifted up): the coded bytes do not change
    rgb = fmt in (api.FORMAT_BGRA, api.FORMAT_RGBA)      # (RGB: a picture close to the frame, not the frame: the coded bytes do change)
    host = [rgb_near_i420(fmt, *f) if rgb else api.planes_from_i420(fmt, *f) for f in host]
    host = [f + [f[-1]] * (3 - len(f)) for f in host]      # (the two-plane formats: the second pointer again; the packed ones: the first)
pitch = None
if a.window_pitch:      # every plane's rows a pitch apart: the tight rows at the front of rows of `pitch` bytes
    rh, rw = np.asarray(host[0][0]).shape if not fmt else ((seq.W, seq.H) if turns & 1 else (seq.H, seq.W))
    _, tight, rows = api.source_window(fmt, rw, rh, 0, 0, [2 ** 31 - 1] * 3)
    if a.window_pitch < tight[0]:
        sys.exit(f"--window-pitch {a.window_pitch}: a luma row of these frames has {tight[0]} bytes")
    pitch = [t * a.window_pitch // tight[0] for t in tight]
    def pitched(f):
        out = []
        for p in range(3):
            if not rows[p]:
                out.append(out[-1])
                continue
            s = np.zeros((rows[p], pitch[p]), np.uint8)
            s[:, :tight[p]] = np.ascontiguousarray(f[p]).view(np.uint8).reshape(rows[p], tight[p])
            out.append(s)
        return out
    host = [pitched(f) for f in host]
tiles, tile_dev = [], []
if a.tiles:      # the sources: a synthetic sequence per tile, device-resident, tight
    if a.scale_from or fmt or pitch or turns or a.mirror or a.deinterlace != "off" or a.arf or a.width % 24 or a.height % 108:
        sys.exit("--tiles goes with none of --scale-from, --source-format, --window-pitch, --rotate, --mirror, --deinterlace, --arf, and a picture whose width is a multiple of 24 and whose height one of 108")
    w, h = a.width, a.height
    tiles = {"letterbox": [(w, h, 0, (h - h * 20 // 27) // 2, w, h * 20 // 27, 0)],
             "grid4": [(w * 2 // 3, h * 2 // 3, x, y, w // 2, h // 2, 0) for y in (0, h // 2) for x in (0, w // 2)],
             "pip": [(w, h, 0, 0, w, h, 0), (w * 2 // 3, h * 2 // 3, w - w // 4 - 32, h - h // 4 - 32 - (h // 4 & 1), w // 4, h // 4 + (h // 4 & 1), 0)]}[a.tiles]
    tile_host = []
    for k, t in enumerate(tiles):
        s = SynthSequence(t[0], t[1], seed=1 + k)
        tile_host.append([tuple(np.ascontiguousarray(p[:t[1] >> (i > 0), :t[0] >> (i > 0)]) for i, p in enumerate(s.frame(j))) for j in range(nd)])
    if a.tiles_precomposed:
        host = [list(api.compose_frame(w, h, tiles, [th[j] for th in tile_host])) for j in range(nd)]
        if (w, h) != (W, H):
            scale = dict(src_width=w, src_height=h)
    else:
        tile_dev = [[tuple(api.to_device(p) for p in th[j]) for th in tile_host] for j in range(nd)]
        tile_src = [[(f[0].data_ptr(), f[1].data_ptr(), f[2].data_ptr(), (0, 0, 0)) for f in frame] for frame in tile_dev]
        if (w, h) != (W, H):
            scale = dict(src_width=w, src_height=h)
    print(f"--tiles {a.tiles}{' (composed on the host beforehand)' if a.tiles_precomposed else ''}: " + ", ".join(f"{t[0]}x{t[1]} -> {t[4]}x{t[5]} at ({t[2]}, {t[3]})" for t in tiles))
dev = [tuple(api.to_device(p) for p in f) for f in host]
api.device_synchronize()
GOP = 1 << 30
if a.temporal_layers > 1 and a.arf:
    sys.exit("--temporal-layers does not go with --arf")
altref = dict(altref_range=GOP + 1) if a.temporal_layers > 1 else dict(altref_range=a.altref_range) if a.altref_range != 5 else {}
drvs = [api.NativeDriver(W, H, gop_size=GOP, num_partitions=a.partitions, check_ssim=a.check_ssim, **altref,
                         loop_filter_type=a.loop_filter_type, quality_stats=a.quality_stats, **scale) for _ in range(a.streams)]
if tile_dev:
    for d in drvs:
        d.set_canvas(tiles)
if a.denoise:
    for d in drvs:
        d.set_denoise(a.denoise)
if a.deinterlace != "off":
    for d in drvs:
        d.set_deinterlace(a.deinterlace, a.field)
if fmt:
    for d in drvs:
        d.set_source_format(fmt)
        d.set_source_colour(a.source_matrix, a.source_range)
if a.source_transfer:      # (the frames carry an SDR picture's codes: the mapped picture means nothing, the kernel's work is the same)
    if fmt not in (api.FORMAT_P010, api.FORMAT_I010):
        sys.exit("--source-transfer goes with --source-format p010 or i010")
    for d in drvs:
        d.set_source_transfer(a.source_transfer, a.source_peak)
for k, (px, ox, oy, opacity) in enumerate(api.parse_overlay(o) for o in a.overlay):
    for d in drvs:
        d.set_overlay(k, px, ox, oy, opacity)
if turns or a.mirror:
    for d in drvs:
        d.set_source_orientation(turns, int(a.mirror))
if pitch:
    for d in drvs:
        d.set_source_window(pitch, 0, 0)
if a.analysis:
    for d in drvs:
        d.set_analysis(True)
if a.aq:
    for d in drvs:
        d.set_segment_mode(2, a.aq)
arf = gop_shard.parse_arf(a.arf) if a.arf else None
if arf:
    for d in drvs:
        d.set_arf(arf[2] + 1)
if a.temporal_layers > 1:
    for d in drvs:
        d.set_temporal_layers(a.temporal_layers)
if a.intra_refresh:
    for d in drvs:
        d.set_intra_refresh(a.intra_refresh)
sizes = [0] * a.streams
hidden_coded = [0] * a.streams


def hidden_frame(d, k, t, emit):
    """in front of frame t: a hidden frame centred on the last frame of the group of PERIOD frames that starts there"""
    c = t + arf[0] - 1
    lo, hi = max(0, c - arf[1] // 2), c + arf[1] // 2
    d.encode_arf_device([tuple(p.data_ptr() for p in dev[(j + 3 * k) % nd]) for j in range(lo, hi + 1)], c - lo)
    hidden_coded[k] += 1
    if emit:
        sizes[k] += len(d.get_frame())


def work(k, n, emit):
    d = drvs[k]
    for t in range(n):
        y, u, v = dev[(t + 3 * k) % nd]
        if arf and t and t % arf[0] == 0:
            hidden_frame(d, k, t, emit)
        if tile_dev:
            d.encode_tiles(tile_src[(t + 3 * k) % nd], device=True)
        else:
            d.encode_frame_device(y.data_ptr(), u.data_ptr(), v.data_ptr())
        if emit:
            sizes[k] += len(d.get_frame())
    d.hip.synchronize()

def run_pipeline(n, emit):
    t0 = time.perf_counter()
    for t in range(n):
        for k, d in enumerate(drvs):
            y, u, v = dev[(t + 3 * k) % nd]
            if arf and t and t % arf[0] == 0:
                hidden_frame(d, k, t, emit)
            d.encode_frame_device(y.data_ptr(), u.data_ptr(), v.data_ptr())
            if emit:
                d.get_frame_begin()
        if emit:
            for k, d in enumerate(drvs):
                sizes[k] += len(d.get_frame_end())
    for d in drvs: d.hip.synchronize()
    return time.perf_counter() - t0

def run(n, emit):
    if a.pipeline:
        return run_pipeline(n, emit)
    th = [threading.Thread(target=work, args=(k, n, emit)) for k in range(a.streams)]
    t0 = time.perf_counter()
    for t in th: t.start()
    for t in th: t.join()
    return time.perf_counter() - t0

run(4, True)
for emit in {"both": (False, True), "on": (True,), "off": (False,)}[a.only]:
    for k in range(a.streams): sizes[k] = 0
    el = run(a.frames, emit)
    fps = a.streams * a.frames / el
    print(f"{W}x{H}{' scaled from ' + a.scale_from + ' (' + a.scale_filter + ')' if a.scale_from else ''} {a.streams} streams x {a.frames} frames, bitstream {'on ' if emit else 'off'}: {fps:8.1f} fps, {fps * mbs / 1e6:6.2f} M MB/s, "
          f"{el / a.frames * 1e3 / 1:7.3f} ms per frame and stream" + (f", {sum(sizes) / (a.streams * a.frames) / 1024:.1f} KiB per frame" if emit else ""))
if a.streams == 1:   # the loop filter by its own clock (the kernel of the chosen type stamps the same words)
    ms, n, ghz = drvs[0].hip.profile_read_clock()
    if n:
        print(f"loop filter type {a.loop_filter_type} by its own clock: {ms / n * 1e3:.1f} us per launch over {n} launches, shader clock {ghz:.2f} GHz")
if a.streams == 1:   # the input side by HIP events: the pack launch, with k_convert_b in front of it when a source format is set
    d = drvs[0]
    d.hip.synchronize()
    d.hip.profile_enable(["pack"])
    work(0, 32, False)
    ms, n = d.hip.profile_read().get("pack", (0.0, 0))
    d.hip.profile_enable([])
    print(f"input side ({'tiles ' + a.tiles if tile_dev else a.source_format or 'i420'}{' ' + a.source_transfer + ' ' + str(a.source_peak) if a.source_transfer else ''}), {n} timed launches over 32 frames: {ms / 32 * 1e3:.2f} us per frame")
if a.aq and a.streams == 1:   # k_mb_p_map next to k_mb_p, and the input side without the map's launches: the same process, HIP events
    d = drvs[0]

    def stage_us(name):
        d.hip.synchronize()
        d.hip.profile_enable([name])
        work(0, 32, False)
        ms, n = d.hip.profile_read().get(name, (0.0, 0))
        d.hip.profile_enable([])
        return ms / max(n, 1) * 1e3, n
    mapped, n_on = stage_us("mb")
    d.set_segment_mode(0)
    plain, n_off = stage_us("mb")
    pack_off, _ = stage_us("pack")
    d.set_segment_mode(2, a.aq)
    print(f"macroblock kernel, mapped (--aq {a.aq}) {mapped:.2f} us per launch over {n_on} launches, default {plain:.2f} us over {n_off}; "
          f"input side without the map {pack_off:.2f} us per launch")
if arf:
    st = drvs[0].arf_stats()
    print(f"hidden alt-refs (--arf {a.arf}): {sum(hidden_coded)} coded over all runs and streams; stream 0's last: {st.last_frames} frames, tiles by block weight 0 / 1 / 2: {list(st.last_weight)}")
    if a.streams == 1:      # the filter launch by HIP events: the input side's stage of a hidden frame (filter + pack) minus a shown frame's (pack)
        d = drvs[0]
        d.hip.synchronize()
        d.hip.profile_enable(["pack"])
        work(0, 1, False)
        pack_ms, _ = d.hip.profile_read().get("pack", (0.0, 0))
        for _ in range(8):
            hidden_frame(d, 0, 8, False)
        ms, n = d.hip.profile_read().get("pack", (0.0, 0))
        d.hip.profile_enable([])
        print(f"k_arf_filter_b, window of {st.last_frames}: {(ms / 8 - pack_ms) * 1e3:.1f} us per launch (the stage's {n} launches over 8 hidden frames minus the pack launch's {pack_ms * 1e3:.1f} us)")
if a.temporal_layers > 1:
    period = 2 * (a.temporal_layers - 1)
    steps = [api.temporal_step(a.temporal_layers, p) for p in range(1, period + 1)]
    info = drvs[0].frame_layer()
    print(f"temporal layers {a.temporal_layers}: of every {period} inter frames {sum(s['refresh'] == api.REFRESH_NONE for s in steps)} refresh no buffer and "
          f"{sum(s['use_golden'] for s in steps)} search GOLDEN beside LAST; stream 0's last frame: temporal_id {info.temporal_id}, tl0_pic_idx {info.tl0_pic_idx}, "
          f"{'loop-filtered' if info.filtered else 'not loop-filtered'}")
if a.intra_refresh:
    info = drvs[0].intra_refresh()
    frames_coded = drvs[0].stats().frame_number
    print(f"intra refresh, period {info.period}: {info.total_forced} forced macroblocks over {frames_coded} frames of stream 0 "
          f"({info.total_forced / max(1, frames_coded) / mbs * 100:.2f} % of the macroblocks); its last frame: phase {info.last_q}, {info.last_forced} forced")
    if a.streams == 1:      # the launch by HIP events (the intra stage of an inter frame is this launch alone)
        d = drvs[0]
        d.hip.synchronize()
        d.hip.profile_enable(["intra"])
        work(0, 32, False)
        ms, n = d.hip.profile_read().get("intra", (0.0, 0))
        d.hip.profile_enable([])
        print(f"k_intra_refresh ({'one wavefront' if os.environ.get('VP8HIP_INTRA_REFRESH_1WAVE') else 'two wavefronts'} per forced macroblock) by HIP events: "
              f"{ms / max(n, 1) * 1e3:.1f} us per launch over {n} launches")
if a.quality_stats:
    q = drvs[0].quality_summary()
    print(f"quality of stream 0 over {q.frames} frames: PSNR overall {q.psnr_all:.3f} dB, avg {q.psnr_avg:.3f} dB, SSIM {q.ssim_all:.5f}")
if a.analysis:
    r = drvs[0].frame_analysis().as_dict()
    print(f"analysis of stream 0, frame {r['frame_number']}: " + ", ".join(f"{k} {v}" for k, v in r.items() if k != "frame_number"))
for d in drvs: d.close()
