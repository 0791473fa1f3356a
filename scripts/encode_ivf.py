#!/usr/bin/env python3
"""Encode a sequence to .ivf with the native frame loop, GOP chunks sharded over the visible GPUs.

    python scripts/encode_ivf.py out.ivf [--y4m in.y4m | --yuv in.yuv --width 1920 --height 1080] [--frames 120 --gop 30 --partitions 4]
    python -m torch.distributed.run --nproc-per-node N --master-addr 127.0.0.1 scripts/encode_ivf.py out.ivf ...

--y4m: YUV4MPEG2, the reference's own input format (size, frame rate and -- from the C tag -- the format of the frames from its header,
vp8oclenc_amd/y4m.py: C422, C444, C420p10, C422p10 and C444p10 files are converted on the device, vp8drv_set_source_format; other
colourspaces are refused); --yuv: raw frames of the given size, I420 or --source-format NAME (nv12, i422, i444, p010, i010, i210,
i410, or the packed yuy2, uyvy, bgra, rgba; the RGB ones are read with --source-matrix bt601|bt709 and --source-range limited|full,
vp8drv_set_source_colour); without either the synthetic sequence of the tests is used.  A raw I420 file has the given width/height (even numbers); when
they are not multiples of 16 the frames are padded on the device (vp8hip_set_source_size = copy_with_padding, encIO.h:141-196)
and the key frames carry the source size as display size.
--surface WxH --crop X:Y (with --yuv): the file's frames are surfaces of WxH and the frame is the window of --width x --height whose
top-left luma sample is (X, Y) (vp8drv_set_source_window with the surface's tight pitch; everything even); --rotate 90|180|270 and
--mirror: the frames are stored sideways, upside down or flipped and are turned clockwise (behind the flip) on the device
(vp8drv_set_source_orientation); behind 90 or 270 degrees the picture that is coded is as wide as the frames that come in are high.
--arf PERIOD[:FRAMES[:STRENGTH]] (FRAMES 1..7, default 7; STRENGTH 0..6, default 3): hidden alternate reference frames (vp8drv_set_arf,
vp8drv_encode_arf_host), placed as scripts/native/y4m_to_ivf -arf places them (gop_shard.hidden_frame_events): the file is the one that
tool writes with -no-scene-detect (with --arf this script does not detect scenes).  One process; 8-bit I420 frames without --denoise, --deinterlace, --analysis or --surface.
--scene-detect: the file scripts/native/y4m_to_ivf writes with its default, scene detection on.  A cut is a key frame and restarts the GOP
counter, so rank 0 first scans the chroma differences of the whole sequence in batches on the device (gop_shard.scan_differences),
api.scene_plan makes the serial loop's own key-frame schedule of them, gop_shard.chunks_from_keys the chunks, and the ranks shard those as
they shard the fixed ones.  Not with --denoise, --deinterlace adaptive, --analysis or --arf: their histories follow the frames taken in.
--temporal-layers N [--keep-layers K]: a stream of N = 1..3 temporal layers (vp8drv_set_temporal_layers; the rule: vp8host_temporal_step,
include/vp8hip_host.h): the file scripts/native/y4m_to_ivf -temporal-layers N writes with the matching settings.  The script sets
altref_range to the GOP size + 1 itself (scheduled alt-refs off) and turns the overlapped filter off.  --keep-layers K writes only the
frames of temporal_id <= K -- what a forwarding unit sends a slow receiver -- each with its own timestamp; the header's frame count is then
the number of frames written (a thinned file is not one the reference's program writes: its off-by-one is not reproduced).  One
process; not with --arf.
--canvas with --tile FILE.yuv:INWxINH:X:Y:W:H[:area|lanczos] (repeatable, in tile order; up to 16): the picture of --width x --height is
composed on the device of the tiles' frames (vp8drv_set_canvas, vp8drv_encode_frame_tiles_host) -- every FILE holds tight I420 frames of
INW x INH, scaled to W x H and placed at (X, Y); a file that ends makes its tile absent from then on; --canvas-bg Y,U,V is what no tile
covers (default 16,128,128).  One process, one driver over the whole sequence with a key frame every --gop frames; goes with
--overlay, --denoise, --aq, --scene-detect (the driver's own), --partitions, --qmin / --qmax, --conformant and --simple-filter only."""
import argparse, os, sys, time
os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from vp8oclenc_amd import gop_shard
from vp8oclenc_amd.synth import SynthSequence


class YuvFile:
    def __init__(self, path, W, H, fmt=0):
        from vp8oclenc_amd import api
        self.W, self.H, self.format = W, H, fmt
        self.m = np.memmap(path, np.uint8, "r")
        self.plane_bytes = api.source_plane_bytes(fmt, W, H)
        self.fsz = sum(self.plane_bytes)
        self.n = len(self.m) // self.fsz

    def planes(self, t):
        b = self.m[t * self.fsz:(t + 1) * self.fsz]
        n0, n1, n2 = self.plane_bytes
        return [np.ascontiguousarray(p) for p in (b[:n0], b[n0:n0 + n1], b[n0 + n1:])[:3 if n2 else 2 if n1 else 1]]

    def frame(self, t):
        b = self.m[t * self.fsz:(t + 1) * self.fsz]
        W, H = self.W, self.H
        return (np.ascontiguousarray(b[:W * H].reshape(H, W)), np.ascontiguousarray(b[W * H:W * H * 5 // 4].reshape(H // 2, W // 2)),
                np.ascontiguousarray(b[W * H * 5 // 4:].reshape(H // 2, W // 2)))


class FormatPlanes:
    """frame(t) of a file in another format than I420: the three pointers vp8drv_set_source_format expects (the second plane again for
    the two-plane formats, the only plane again for the packed ones)"""

    def __init__(self, seq):
        self.seq, self.W, self.H, self.n = seq, seq.W, seq.H, seq.n

    def frame(self, t):
        p = self.seq.planes(t)
        return p + [p[-1]] * (3 - len(p))


def canvas_main(a):
    """--canvas: one driver over the whole sequence, every frame composed of the tiles' files"""
    from vp8oclenc_amd import api
    if not (a.canvas and a.tile) or a.yuv or a.y4m or a.resize or a.source_format or a.source_transfer or a.deinterlace != "off" or a.surface or a.rotate or a.mirror or \
            a.analysis or a.segment_map or a.arf or int(os.environ.get("WORLD_SIZE", 1)) > 1:
        sys.exit("--canvas goes with --tile (and --tile with --canvas), one process, and none of --yuv, --y4m, --resize, --source-format, --source-transfer, "
                 "--deinterlace, --surface, --rotate, --mirror, --analysis, --segment-map, --arf")
    try:
        tiles = [api.parse_tile(t) for t in a.tile]
        bg = tuple(int(x) for x in a.canvas_bg.split(","))
        overlays = [api.parse_overlay(o) for o in a.overlay]
        if len(bg) != 3 or len(tiles) > api.MAX_TILES or len(overlays) > api.MAX_OVERLAYS:
            raise ValueError(f"three background values, at most {api.MAX_TILES} tiles and {api.MAX_OVERLAYS} layers")
        files = [YuvFile(path, t.in_w, t.in_h) for path, t in tiles]
    except (ValueError, OSError) as e:
        sys.exit(f"--canvas: {e}")
    Wd, Hd = a.width, a.height
    Wc, Hc = (Wd + 15) // 16 * 16, (Hd + 15) // 16 * 16
    src = dict(src_width=Wd, src_height=Hd) if (Wc, Hc) != (Wd, Hd) else {}
    t0 = time.perf_counter()
    try:
        drv = api.NativeDriver(Wc, Hc, device=int(os.environ.get("LOCAL_RANK", 0)), **src, gop_size=a.gop, num_partitions=a.partitions, qi_min=a.qmin, qi_max=a.qmax,
                               ssim_target=a.ssim_target, check_ssim=1, conformant_stream=int(a.conformant), loop_filter_type=int(a.simple_filter),
                               scene_detect=int(a.scene_detect))
        drv.set_canvas([t for _, t in tiles], bg)
    except api.Vp8HipError as e:
        sys.exit(f"--canvas: {e}")
    if a.denoise:
        drv.set_denoise(a.denoise)
    if a.aq:
        drv.set_segment_mode(2, a.aq)
    if a.intra_refresh:
        drv.set_intra_refresh(a.intra_refresh)
    for k, (px, ox, oy, opacity) in enumerate(overlays):
        drv.set_overlay(k, px, ox, oy, opacity)
    out = []
    for t in range(a.frames):
        drv.encode_tiles([f.frame(t) if t < f.n else None for f in files])
        out.append(drv.get_frame())
    drv.close()
    n = gop_shard.write_ivf(a.out, out, Wd, Hd, a.framerate)
    el = time.perf_counter() - t0
    print(f"{a.out}: {a.frames} frames {Wd}x{Hd} composed of {len(tiles)} tiles, {n} bytes, {a.frames / el:.1f} frames/s including the host-side frame sources")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out"); ap.add_argument("--yuv"); ap.add_argument("--y4m")
    ap.add_argument("--width", type=int, default=1920); ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--frames", type=int, default=60); ap.add_argument("--gop", type=int, default=30)
    ap.add_argument("--partitions", type=int, default=1); ap.add_argument("--qmin", type=int, default=0); ap.add_argument("--qmax", type=int, default=48)
    ap.add_argument("--ssim-target", type=float, default=-1.0); ap.add_argument("--framerate", type=int, default=30)
    ap.add_argument("--simple-filter", action="store_true", help="the simple loop filter (RFC 6386 section 15.2, filter_type 1) instead of the normal one")
    ap.add_argument("--conformant", action="store_true", help="vp8hip_conformant_stream: NOT the reference byte for byte, but a stream that decodes to the encoder's own reconstruction")
    ap.add_argument("--resize", default="", metavar="WxH", help="code the picture at this size: the frames are scaled down on the device (vp8hip_set_source_scaling)")
    ap.add_argument("--resize-filter", choices=("area", "lanczos"), default="area")
    ap.add_argument("--source-format", default="", metavar="NAME", help="the format of the frames of --yuv (or of --y4m, instead of its C tag: nv12 and p010 have none): i420, nv12, i422, i444, p010, i010, i210, i410, and for --yuv the packed yuy2, uyvy, bgra, rgba; converted on the device (vp8drv_set_source_format)")
    ap.add_argument("--source-matrix", choices=("bt601", "bt709"), default="bt601", help="the colour matrix bgra / rgba frames are read with (vp8drv_set_source_colour)")
    ap.add_argument("--source-range", choices=("limited", "full"), default="limited", help="... and the range of the YUV it makes")
    ap.add_argument("--source-transfer", choices=("pq", "hlg"), default="", help="the ten-bit frames (--source-format p010 or i010, or a C420p10 file) carry a PQ or HLG signal in BT.2020 and are tone-mapped to SDR on the device, written with --source-matrix / --source-range (vp8drv_set_source_transfer)")
    ap.add_argument("--source-peak", type=int, default=1000, metavar="N", help="... the peak luminance they were graded for, 400..10000 nits")
    ap.add_argument("--overlay", action="append", default=[], metavar="FILE:WxH:X:Y[:OPACITY]", help="FILE holds W x H pixels of raw BGRA, tight, straight alpha: the layer is burnt into every frame on the device with its top-left pixel at (X, Y) of the coded picture, at OPACITY 0..255 (default 255), read with BT.601 limited range (vp8drv_set_overlay_host); up to four times, applied in order")
    ap.add_argument("--denoise", type=int, choices=(0, 1, 2, 3), default=0, help="temporal noise reduction of the source frames on the device (vp8drv_set_denoise); the history restarts with every GOP")
    ap.add_argument("--deinterlace", choices=("off", "field", "adaptive"), default="off", metavar="MODE", help="interlaced source frames made progressive on the device (vp8drv_set_deinterlace): field = every missing row interpolated, adaptive = what stands still is woven; the history restarts with every GOP")
    ap.add_argument("--field", choices=("top", "bottom"), default="top", help="... the field that is kept")
    ap.add_argument("--surface", default="", metavar="WxH", help="with --yuv: the file's frames are surfaces of this size and the frame is the window of --width x --height at --crop (vp8drv_set_source_window)")
    ap.add_argument("--crop", default="0:0", metavar="X:Y", help="... the window's top-left luma sample (even numbers)")
    ap.add_argument("--rotate", type=int, choices=(0, 90, 180, 270), default=0, help="turn the frames clockwise by this many degrees on the device (vp8drv_set_source_orientation)")
    ap.add_argument("--mirror", action="store_true", help="... behind a left-right flip")
    ap.add_argument("--analysis", default="", metavar="FILE", help="the frame analysis record of every frame as one text line per frame (vp8drv_set_analysis; the line: scripts/native/y4m_to_ivf.cpp): a first-pass file")
    ap.add_argument("--aq", type=int, choices=(0, 1, 2, 3), default=0, metavar="N", help="variance-adaptive quantisation of the inter frames at strength N: flat macroblocks take the finer segments of the quantiser ladder, busy ones the coarser (vp8drv_set_segment_mode, mode 2)")
    ap.add_argument("--segment-map", default="", metavar="FILE", help="the caller's segment map for every inter frame: one byte 0..3 per macroblock of the coded picture, raster order (vp8drv_set_segment_mode, mode 1)")
    ap.add_argument("--arf", default="", metavar="PERIOD[:FRAMES[:STRENGTH]]", help="hidden alternate reference frames made by temporal filtering on the device (vp8drv_set_arf, vp8drv_encode_arf_host): one in front of every group of PERIOD frames of a GOP, centred on the group's last frame, FRAMES frames wide (default 7) at STRENGTH 0..6 (default 3)")
    ap.add_argument("--no-check-ssim", action="store_true", help="cfg.check_ssim = 0, scripts/native/y4m_to_ivf's -no-check-ssim: no check_SSIM behind the inter frames (with --temporal-layers the unreferenced frames are then not loop-filtered)")
    ap.add_argument("--temporal-layers", type=int, choices=(1, 2, 3), default=0, metavar="N", help="a stream of N temporal layers (vp8drv_set_temporal_layers): it still decodes when the frames above a layer are dropped")
    ap.add_argument("--intra-refresh", type=int, default=0, metavar="N", help="cyclic intra refresh with period N, 4..1024 (vp8drv_set_intra_refresh; scripts/native/y4m_to_ivf's -intra-refresh): a few macroblocks of every inter frame coded as intra, the whole picture every N frames that refresh LAST; the phase restarts with every GOP, so chunks give the serial bytes; not with --ssim-target above -1")
    ap.add_argument("--keep-layers", type=int, choices=(0, 1, 2), default=None, metavar="K", help="with --temporal-layers: write only the frames of temporal_id <= K, with their own timestamps")
    ap.add_argument("--scene-detect", action="store_true", help="key frames where the serial program with scene detection puts them: the sequence is scanned first (gop_shard.scan_differences), api.scene_plan gives the chunks")
    ap.add_argument("--scan-batch", type=int, default=8, metavar="N", help="... members of the scanning batch (1..8)")
    ap.add_argument("--canvas", action="store_true", help="compose the picture of --width x --height of the --tile sources on the device (vp8drv_set_canvas)")
    ap.add_argument("--tile", action="append", default=[], metavar="FILE.yuv:INWxINH:X:Y:W:H[:area|lanczos]", help="with --canvas, repeatable, in tile order: FILE holds tight I420 frames of INW x INH, scaled to W x H and placed at (X, Y) of the picture; a file that ends makes its tile absent")
    ap.add_argument("--canvas-bg", default="16,128,128", metavar="Y,U,V", help="... the background: what no tile covers")
    a = ap.parse_args()
    if a.canvas or a.tile:
        return canvas_main(a)
    if a.scene_detect and (a.denoise or a.deinterlace == "adaptive" or a.analysis or a.arf):
        sys.exit("--scene-detect does not go with --denoise, --deinterlace adaptive, --analysis or --arf: their histories follow the frames taken in, the scan would disturb them")
    if not 1 <= a.scan_batch <= 8:
        sys.exit("--scan-batch: 1..8")
    arf = None
    if a.arf:
        try:
            arf = gop_shard.parse_arf(a.arf)
        except ValueError as e:
            sys.exit(f"--arf {a.arf}: {e}")
        if a.denoise or a.deinterlace != "off" or a.analysis or a.surface:
            sys.exit("--arf does not go with --denoise, --deinterlace, --analysis or --surface")
    if a.keep_layers is not None and not a.temporal_layers:
        sys.exit("--keep-layers goes with --temporal-layers")
    if a.temporal_layers and (arf or int(os.environ.get("WORLD_SIZE", 1)) > 1):
        sys.exit("--temporal-layers: one process, and not with --arf (layers never search ALTREF)")
    if a.aq and a.segment_map:
        sys.exit("--aq and --segment-map: one of them picks the segments")
    if a.intra_refresh and (not 4 <= a.intra_refresh <= 1024 or a.ssim_target > -1.0):
        sys.exit("--intra-refresh: a period of 4..1024, and not with --ssim-target above -1 (the SSIM ladder owns the intra fallback)")
    rank, world, local = int(os.environ.get("RANK", 0)), int(os.environ.get("WORLD_SIZE", 1)), int(os.environ.get("LOCAL_RANK", 0))
    dist = None
    if world > 1:      # the library's own process group (vp8hip_group_*: RCCL inside libvp8hip.so, the id through a file): no GPU framework in the host
        from vp8oclenc_amd import api
        dist = api.Group.from_env(local, f"encode_ivf-{os.getppid()}-{os.environ.get('MASTER_PORT', '0')}")
    from vp8oclenc_amd import api
    if a.surface and not a.yuv:
        sys.exit("--surface goes with --yuv")
    surface = tuple(int(x) for x in a.surface.lower().split("x")) if a.surface else None
    try:
        fmt = api.source_format(a.source_format) if a.source_format else None
        if a.y4m and fmt is not None and fmt >= api.FORMAT_YUY2:
            raise ValueError(f"a YUV4MPEG2 frame is planar: {a.source_format} goes with --yuv")
        if a.y4m:
            from vp8oclenc_amd.y4m import Y4mFile
            seq = Y4mFile(a.y4m, fmt)      # (without --source-format: the file's C tag, and ValueError for one the encoder cannot take)
            a.framerate = seq.framerate or a.framerate
        else:
            seq = YuvFile(a.yuv, *(surface or (a.width, a.height)), fmt or 0) if a.yuv else SynthSequence(a.width, a.height, seed=1)
    except ValueError as e:
        sys.exit(f"{a.y4m or a.yuv or '--source-format'}: {e}")
    fmt = getattr(seq, "format", 0)
    if a.source_transfer and (fmt not in (api.FORMAT_P010, api.FORMAT_I010) or not api.PEAK_MIN <= a.source_peak <= api.PEAK_MAX):
        sys.exit(f"--source-transfer {a.source_transfer} --source-peak {a.source_peak}: ten-bit 4:2:0 frames only (--source-format p010 or i010, or a C420p10 file; "
                 f"these are {api.source_format_name(fmt)}) and a peak of {api.PEAK_MIN}..{api.PEAK_MAX} nits")
    if fmt:
        seq = FormatPlanes(seq)
    frames = min(a.frames, seq.n) if (a.yuv or a.y4m) else a.frames
    turns = a.rotate // 90
    raw = (a.width, a.height) if surface else (seq.W, seq.H)      # the frames as they come in: the window of a surface, or the file's
    Win, Hin = raw[::-1] if turns & 1 else raw                    # ... and upright
    window = None
    if surface:
        try:
            x, y = (int(v) for v in a.crop.split(":"))
            window = (api.source_window(fmt, *surface, 0, 0, [2 ** 31 - 1] * 3)[1], x, y)      # (the surface's tight pitch)
            api.source_window(fmt, *raw, x, y, window[0])
            if y + raw[1] > surface[1]:
                raise ValueError("the window ends below the surface")
        except ValueError as e:
            sys.exit(f"--surface {a.surface} --crop {a.crop}: {e}")
    Wd, Hd = (int(x) for x in a.resize.lower().split("x")) if a.resize else (Win, Hin)      # the picture that is coded and displayed ("dst")
    Wc, Hc = (Wd + 15) // 16 * 16, (Hd + 15) // 16 * 16            # the coded ("wrk") size, init.h:375-392
    src = dict(src_width=Wd, src_height=Hd) if (Wc, Hc) != (Wd, Hd) else {}
    if (Wd, Hd) != (Win, Hin):
        src.update(in_width=Win, in_height=Hin, scale_filter=int(a.resize_filter == "lanczos"))
    seg_map = None
    if a.segment_map:
        seg_map = np.fromfile(a.segment_map, np.uint8)
        if seg_map.size != (Wc // 16) * (Hc // 16) or (seg_map.size and seg_map.max() > 3):
            sys.exit(f"--segment-map {a.segment_map}: {(Wc // 16) * (Hc // 16)} bytes of 0..3 are one map of {Wc}x{Hc}")
    try:
        overlays = [api.parse_overlay(o) for o in a.overlay]
    except (ValueError, OSError) as e:
        sys.exit(f"--overlay: {e}")
    if len(overlays) > api.MAX_OVERLAYS or (overlays and arf):
        sys.exit(f"--overlay: at most {api.MAX_OVERLAYS} layers, and not with --arf (the window frames bypass the intake)")
    t0 = time.perf_counter()
    def make_encoder(scan=False):
        enc = gop_shard.NativeEncoder(Wc, Hc, device=local, **src, num_partitions=a.partitions, qi_min=a.qmin, qi_max=a.qmax,
                                      ssim_target=a.ssim_target, check_ssim=int(not a.no_check_ssim), conformant_stream=int(a.conformant),
                                      loop_filter_type=int(a.simple_filter), **(dict(overlap_filter=0) if arf or scan or a.temporal_layers else {}),      # (nor are members of a batch)
                                      **(dict(gop_size=1 << 30, altref_range=(1 << 30) + 1) if a.temporal_layers else {}))      # (a chunk is one GOP; scheduled alt-refs off)
        if a.temporal_layers and not scan:      # every frame's layer next to its bytes
            enc.drv.set_temporal_layers(a.temporal_layers)
            plain_encode = enc.encode

            def encode_layered(y, u, v):
                b = plain_encode(y, u, v)
                tids.append(enc.drv.frame_layer().temporal_id)
                return b
            enc.encode = encode_layered
        if arf:      # (the driver refuses the filter's own stream beside hidden frames)
            enc.drv.set_arf(arf[2] + 1)
        if a.intra_refresh and not scan:      # (a scanning member codes nothing, and a batch refuses a driver with a period)
            enc.drv.set_intra_refresh(a.intra_refresh)
        if a.denoise:
            enc.drv.set_denoise(a.denoise)
        if a.aq:
            enc.drv.set_segment_mode(2, a.aq)
        if seg_map is not None:
            enc.drv.set_segment_mode(1)
            enc.drv.set_segment_map(seg_map)
        if a.deinterlace != "off":
            enc.drv.set_deinterlace(a.deinterlace, a.field)
        if fmt:
            enc.drv.set_source_format(fmt)
            enc.drv.set_source_colour(a.source_matrix, a.source_range)
        if a.source_transfer:
            enc.drv.set_source_transfer(a.source_transfer, a.source_peak)
        for k, (px, ox, oy, opacity) in enumerate(overlays):
            enc.drv.set_overlay(k, px, ox, oy, opacity)
        if turns or a.mirror:
            enc.drv.set_source_orientation(turns, int(a.mirror))
        if window:
            enc.drv.set_source_window(*window)
        if a.analysis:      # every frame's record next to its bytes (the line needs both)
            enc.drv.set_analysis(True)
            plain = enc.encode

            def encode(y, u, v):
                b = plain(y, u, v)
                records.append(enc.drv.frame_analysis().text_line(len(b)).split(" ", 1)[1])      # (the frame number is the file's, not the chunk's)
                return b
            enc.encode = encode
        return enc
    records, tids = [], []
    if a.analysis and world > 1:
        sys.exit("--analysis: one process only (the records are not gathered over ranks)")
    if arf:      # the plain loop with the lookahead the frame source gives: a hidden frame is a record of its own
        if world > 1 or fmt:
            sys.exit("--arf: one process, 8-bit I420 frames")
        recs, hidden = [], 0
        for start, length in gop_shard.gop_chunks(frames, a.gop):
            enc = make_encoder()
            for ev in gop_shard.hidden_frame_events(length, arf[0], arf[1]):
                if ev[0] == "shown":
                    recs.append((start + ev[1], enc.encode(*seq.frame(start + ev[1]))))
                else:
                    _, lo, n, centre, ts = ev
                    enc.drv.encode_arf_host([seq.frame(start + lo + k) for k in range(n)], centre)
                    recs.append((start + ts, enc.drv.get_frame()))
                    hidden += 1
            enc.close()
        n = gop_shard.write_ivf_records(a.out, recs, Wd, Hd, a.framerate)
        el = time.perf_counter() - t0
        print(f"{a.out}: {frames} shown + {hidden} hidden frames {Win}x{Hin}{f' scaled to {Wd}x{Hd}' if a.resize else ''}, {n} bytes, {frames / el:.1f} frames/s including the host-side frame source")
        return
    chunks, plan = gop_shard.chunks_of_rank(frames, a.gop, rank, world), ""
    if a.scene_detect:
        is_key = b""
        if rank == 0:      # one process scans: the frames as the encoders take them in (format, window, orientation, scaling), a batch of scanning members
            t1 = time.perf_counter()
            encs = [make_encoder(scan=True) for _ in range(max(1, min(a.scan_batch, frames)))]
            batch = api.NativeBatch([e.drv for e in encs])
            ud, vd = gop_shard.scan_differences(batch, seq, frames)
            batch.close()
            for e in encs:
                e.close()
            key, by_scene = api.scene_plan(ud, vd, a.gop)
            is_key = key.astype(np.uint8).tobytes()
            plan = f"; scene plan: {int(key.sum())} key ({int(by_scene.sum())} by scene change), scanning {time.perf_counter() - t1:.3f} s"
        if dist is not None:
            is_key = dist.broadcast_bytes(is_key, frames, 0)
        chunks = gop_shard.chunks_from_keys(np.frombuffer(is_key, np.uint8))[rank::world]
    mine = gop_shard.encode_chunks_frames(make_encoder, seq, chunks)
    if a.analysis:
        with open(a.analysis, "w") as f:
            f.write("".join(f"{t} {line}\n" for t, line in enumerate(records)))
    allf = gop_shard.gather_frames(mine, frames, dist)
    if a.temporal_layers:      # (one process: tids[t] is frame t's layer)
        kept = [(t, b) for t, b in enumerate(allf) if a.keep_layers is None or tids[t] <= a.keep_layers]
        if a.keep_layers is None:
            n = gop_shard.write_ivf(a.out, allf, Wd, Hd, a.framerate)
        else:
            n = gop_shard.write_ivf_records(a.out, kept, Wd, Hd, a.framerate, count=len(kept))
        el = time.perf_counter() - t0
        print(f"{a.out}: {len(kept)} of {frames} frames {Win}x{Hin}, {a.temporal_layers} temporal layers (frames in layer 0 / 1 / 2: "
              f"{' / '.join(str(tids.count(k)) for k in range(3))}){'' if a.keep_layers is None else f', layers <= {a.keep_layers} kept'}, {n} bytes, "
              f"{frames / el:.1f} frames/s including the host-side frame source{plan}")
        return
    if rank == 0:
        n = gop_shard.write_ivf(a.out, allf, Wd, Hd, a.framerate)
        el = time.perf_counter() - t0
        print(f"{a.out}: {frames} frames {Win}x{Hin}{f' scaled to {Wd}x{Hd}' if a.resize else ''}, {n} bytes, {world} GPU(s), {frames / el:.1f} frames/s including the host-side frame source{plan}")
    if dist is not None:
        dist.close()


if __name__ == "__main__":
    main()
