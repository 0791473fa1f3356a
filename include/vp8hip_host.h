/*
 * vp8hip_host.h -- host-side mirror (C++ behind a C ABI, no GPU needed) of the reference host
 * code that PRODUCES the parameters of the inter-frame path and sequences it.  The reference keeps
 * this logic in vp8enc.cpp / init.h around its OpenCL calls; a maintainer who swaps the OpenCL calls
 * for include/vp8hip.h keeps those functions as they are.  They are restated here so that the
 * parity tests and bench.py drive the device path with the same numbers the reference would.
 */
#ifndef VP8HIP_HOST_H
#define VP8HIP_HOST_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ParseArgs quantizer ladders, init.h:1585-1603.  Index 0..3 = UQ, HQ, AQ, LQ. */
void vp8host_quantizer_ladders(int qi_min, int qi_max, int32_t lastqi[4], int32_t altrefqi[4]);

/* get_loopfilter_strength(), vp8enc.cpp:96-127: brightness-based divisor and sharpness (0..7) */
void vp8host_loopfilter_strength(const uint8_t *cur_y, int width, int height, int32_t *reductor, int32_t *sharpness);

/* scene_change(), vp8enc.cpp:265-311: the decision on the two chroma differences (vp8hip_chroma_change), with the
 * reference's hold-over (its function-static `holdover`) and frames.last_key_detect in `st`.  Returns 1 when the
 * current frame must be coded as a key frame; the caller then sets st->last_key_detect = frame_number
 * (intra_transform does, intra_part.h:1091-1098). */
typedef struct { int32_t holdover, last_key_detect; } vp8host_scene_state;
int vp8host_scene_change(vp8host_scene_state *st, int Udiff, int Vdiff, int frame_number);

/* prepare_segments_data(), vp8enc.cpp:129-221.  refqi = lastqi or altrefqi (vp8enc.cpp:149-151);
 * update_filter/shrpnss: the second call made from check_SSIM (vp8enc.cpp:260-261). */
void vp8host_prepare_segments_data(int is_key_frame, const int32_t refqi[4], int qi_min, int reductor,
                                   int sharpness, int update_filter, int shrpnss, int32_t sd[44]);

/* The input format: YUV4MPEG2.  OpenYUV420FileAndParseHeader(), init.h:1610-1737, on the first `size` bytes of the stream
 * (128 are plenty: the reference keeps the header in a 128-byte array): the magic word, then the FIRST THREE tags that start
 * with W, H or F -- width, height, frame rate num:denom rounded to (num + denom / 2) / denom -- each ended by a space, then
 * everything up to and including the first "FRAME\n" (a FRAME line with parameters is refused, :1724-1726).  Returns 0 and
 * the offset of the first frame's samples, or -1 as the reference does (not YUV4MPEG2, no size, no plain FRAME line, or the
 * buffer ends first).  Frames follow as tight I420 of width x height, each followed by the next one's 6-byte "FRAME\n"
 * (get_yuv420_frame checks bytes 0 and 4 of it, encIO.h:243-248: vp8host_y4m_frame_marker_ok). */
int vp8host_y4m_parse_header(const uint8_t *data, size_t size, int32_t *width, int32_t *height, int32_t *framerate, size_t *first_frame_offset);
int vp8host_y4m_frame_marker_ok(const uint8_t marker[6]);

/* The tables of the device's scaler (vp8hip_set_source_scaling, include/vp8hip.h): one dimension of one plane, n_in samples to
 * n_out <= n_in <= 16384.  For every output i: the first source sample start[i], and *n_taps (the same for every i, at most
 * VP8HOST_SCALE_MAX_TAPS) signed coefficients coef[i * VP8HOST_SCALE_MAX_TAPS + k] whose sum is exactly 4096; the rest of a row is 0.
 * Taps outside the plane are folded onto the edge sample, so 0 <= start[i] and start[i] + *n_taps <= n_in.  The device applies
 *     t[y][i]   = (sum_k cx[i][k] * src[y][start_x[i] + k] + 32) >> 6                          (arithmetic shift, fits int16)
 *     out[j][i] = clamp((sum_k cy[j][k] * t[start_y[j] + k][i] + (1 << 17)) >> 18, 0, 255).
 * kind 0, area: in units of 1 / n_out of a source sample output i covers [i n_in, (i + 1) n_in), sample j covers
 * [j n_out, (j + 1) n_out); with cum_j the length of output i's interval left of sample j's right end,
 * c[i][j] = floor(4096 cum_j / n_in) - floor(4096 cum_(j-1) / n_in): integers only.  At 2:1 both passes together are
 * (a + b + c + d + 2) >> 2.  kind 1, Lanczos-3 stretched by r = n_in / n_out: centre (i + 0.5) r - 0.5, taps ceil(centre - 3 r) ..
 * floor(centre + 3 r), weights L(d / r), L(x) = sinc(x) sinc(x / 3) for |x| < 3, in double; each rounded to nearest of 4096 w / sum,
 * the remainder added to the row's largest tap.  Returns 0, or -1 for bad arguments, more than VP8HOST_SCALE_MAX_TAPS taps (area
 * beyond about 31:1, Lanczos beyond about 5:1), more taps than samples, or a row whose sum of |c| exceeds 8000. */
#define VP8HOST_SCALE_MAX_TAPS 32
int vp8host_scale_taps(int n_in, int n_out, int kind, int32_t *n_taps, int32_t *start /* [n_out] */, int16_t *coef /* [n_out * 32] */);

/* CANVAS: a frame composed of scaled video tiles (vp8hip_set_canvas, vp8hip_compose_current_*, include/vp8hip.h; k_compose_b), bit for
 * bit.  The project's own: the reference takes one source per frame.
 * The canvas is the PICTURE pw x ph, both even: the size given to vp8hip_set_source_size, or the coded size.
 * Tiles.  Up to VP8HIP_MAX_TILES tiles {in_w, in_h, x, y, w, h, filter}: frames of in_w x in_h are scaled to w x h and placed with
 * their top-left sample at (x, y) of the picture.  A tile is valid when all six sizes and positions are even, w, h >= 2, 0 <= x,
 * x + w <= pw, 0 <= y, y + h <= ph, w <= in_w <= 16384, h <= in_h <= 16384, filter is 0 (area) or 1 (Lanczos-3), and
 * vp8host_scale_taps accepts in_w -> w, in_h -> h, in_w / 2 -> w / 2 and in_h / 2 -> h / 2 with that filter.  No upscaling; equal
 * sizes are the identity.  The background (bg_y, bg_u, bg_v) is three values 0 .. 255.
 * Per frame a tile has three planes, 8-bit I420 of in_w x in_h: a pointer and a pitch each (0 = tight, otherwise at least the plane's
 * width; neither pointer nor pitch needs any alignment; nothing behind the last sample of the last row is read).  y == NULL: the tile
 * is absent this frame and leaves what is under it.
 * Composition.  (1) Every sample of the three planes is the background.  (2) For each tile in index order that is present, each of
 * its three planes is scaled on its own by the two passes written next to vp8host_scale_taps above, with vp8host_scale_taps' own
 * tables for the plane's two pairs (luma: in_w -> w, in_h -> h; chroma: in_w / 2 -> w / 2, in_h / 2 -> h / 2).  (3) The scaled plane
 * REPLACES the rectangle: luma (x, y, w, h), chroma (x / 2, y / 2, w / 2, h / 2).  Later tiles lie on top of earlier ones; overlaps
 * are allowed.  No blending, no alpha, no rounding beyond the scaler's.  (4) On the device the padding behind the picture's last
 * column and row repeats the composed picture's edge: copy_with_padding of the result.
 * vp8host_compose_frame writes the picture, tight planes of pw x ph and (pw / 2) x (ph / 2).  Returns 0, or -1 with nothing written
 * for a null pointer, an odd or non-positive picture size, n outside 0 .. VP8HIP_MAX_TILES, a background value outside 0 .. 255, an
 * invalid tile, or a pitch below its plane's width. */
#define VP8HIP_MAX_TILES 16
typedef struct { int32_t in_w, in_h, x, y, w, h, filter; } vp8hip_tile;
typedef struct { const uint8_t *y, *u, *v; int32_t pitch_y, pitch_u, pitch_v; } vp8hip_tile_planes;
int vp8host_tile_valid(int pw, int ph, const vp8hip_tile *tile);      /* 1: valid inside a picture of pw x ph */
int vp8host_compose_frame(int pw, int ph, const vp8hip_tile *tiles, int n, int bg_y, int bg_u, int bg_v,
                          const vp8hip_tile_planes *src /* [n] */, uint8_t *out_y, uint8_t *out_u, uint8_t *out_v);

/* The rule of the device's temporal denoiser (vp8hip_set_denoise, include/vp8hip.h; k_denoise_b), bit for bit.  The project's own: the
 * reference never did anything about noise.
 * History and pass-through.  A context with denoising on keeps a history: the previous frame as it left the denoiser, Y, U and V at
 * the coded size, padding included.  The denoiser works on the frame after pack / pad / scale, on whole coded macroblocks, before
 * anything else reads the frame.  Without a history (first frame, after a restart, after the level changed) the frame passes through
 * unchanged and becomes the history.
 * Per sample, with k = level (1, 2, 3), source S and history R: d = R - S, a = |d|, and the step c is
 *     a <= 2 + k: c = d (the output is R);   else a <= 7: c = sign(d) (2 + k);   else a <= 15: c = sign(d) (3 + k);
 *     else: c = sign(d) (5 + k).
 * With k = 1 these are libvpx's VP8 denoiser steps, 3 / 4 / 6 above a threshold of 3.  |c| <= a and c has d's sign, so S + c lies
 * between S and R and needs no clamp.
 * Per 16x16 luma macroblock: T = sum of c over its 256 samples, sad = sum of a.  The macroblock is FILTERED iff
 * |T| <= VP8HOST_DENOISE_SUM_Y (16 * 16 * 2, libvpx's) and sad <= VP8HOST_DENOISE_SAD_Y; otherwise it is COPIED: output = source.
 * The two 8x8 chroma blocks of a filtered macroblock are filtered by the same per-sample rule, each on its own and only if its
 * |T_c| <= VP8HOST_DENOISE_SUM_C; a copied macroblock's chroma blocks are copied.  Output of a filtered block = S + c.  The whole
 * output frame is the new history.
 * vp8host_denoise_frame: the rule on tight planes of the coded size (width, height multiples of 16; chroma width / 2 x height / 2).
 * have_history 0 or level 0: out = src, *mbs_filtered = 0.  With level != 0 the history planes are replaced by the output (in-out);
 * with level 0 they are left alone.  out may be src or the history itself.  Returns 0, or -1 for bad arguments. */
#define VP8HOST_DENOISE_SUM_Y 512
#define VP8HOST_DENOISE_SAD_Y 2560
#define VP8HOST_DENOISE_SUM_C 128
int vp8host_denoise_frame(const uint8_t *src_y, const uint8_t *src_u, const uint8_t *src_v, uint8_t *hist_y, uint8_t *hist_u, uint8_t *hist_v,
                          uint8_t *out_y, uint8_t *out_u, uint8_t *out_v, int width, int height, int level, int have_history,
                          int32_t *mbs_filtered);

/* The formats source frames may come in (vp8hip_set_source_format, include/vp8hip.h; k_convert_b) and the ONE integer rule that makes
 * 8-bit I420 of the same width and height of each of them.  The project's own: the reference reads tight 8-bit I420 and nothing else.
 * All planes are tight, width and height are even.  "16-bit" = little-endian words, two bytes per sample.
 *     I420 (0)  Y, U, V; chroma w/2 x h/2                     8-bit        (the default: nothing is converted)
 *     NV12 (1)  Y, interleaved UV (U first), w/2 x h/2 pairs  8-bit        (the third pointer is not read)
 *     I422 (2)  Y, U, V; chroma w/2 x h                       8-bit
 *     I444 (3)  Y, U, V; chroma w x h                         8-bit
 *     P010 (4)  as NV12                                       16-bit, the value in the TOP ten bits: s = word >> 6
 *     I010 (5)  as I420                                       16-bit, the value in the LOW ten bits: s = word & 1023
 *     I210 (6)  as I422                                       as I010
 *     I410 (7)  as I444                                       as I010
 * With d the depth (8 or 10) and s a sample's value at that depth, every output sample is
 *     out = min(255, (S + (1 << (k - 1))) >> k)        (out = S when k is 0),        k = log2(n) + d - 8,
 * where S is the sum of the n source samples the output sample covers: n = 1 for luma and for the chroma of the 4:2:0 formats; n = 2,
 * the two vertically adjacent samples (rows 2r and 2r + 1), for the chroma of 4:2:2; n = 4, the 2x2 block, for the chroma of 4:4:4.
 * One rounding step, never two; chroma siting is not modelled; no colour matrix for these eight (the planar family, numbers below
 * VP8HOST_FORMAT_COUNT).  The clamp matters at ten bits only: 1023 gives (1023 + 2) >> 2 = 256.  The low six bits of a P010 word and
 * the high six of the other 16-bit formats' words are ignored.
 *
 * THE PACKED FAMILY, numbers VP8HOST_FORMAT_PACKED_FIRST .. VP8HOST_FORMAT_PACKED_END - 1 (8 .. 15 are no format and are refused
 * everywhere): ONE plane, tight, 8-bit, width and height even.  The second and third pointers are never read.
 *     YUY2 (16)  per pixel pair the four bytes Y0 U Y1 V        2 w h bytes      (k_convert_packed_b)
 *     UYVY (17)  per pixel pair the four bytes U Y0 V Y1        2 w h bytes
 *     BGRA (18)  per pixel the four bytes B G R A               4 w h bytes      (A never influences anything)
 *     RGBA (19)  per pixel the four bytes R G B A               4 w h bytes
 * YUY2 / UYVY are the I422 rule on the samples they carry: luma is copied, chroma is (c[2r][x] + c[2r + 1][x] + 1) >> 1, so a YUY2
 * frame converts to exactly what the I422 frame holding the same samples converts to.
 * BGRA / RGBA take a colour matrix m (enum vp8host_colour_matrix; vp8hip_set_source_colour): an offset and nine coefficients, times 256,
 * in the order R, G, B:
 *     m                   off    Y             U               V
 *     0 BT601_LIMITED     16     66 129  25    -38  -74 112    112  -94 -18        (the default)
 *     1 BT709_LIMITED     16     47 157  16    -26  -86 112    112 -102 -10
 *     2 BT601_FULL         0     77 150  29    -43  -84 127    127 -106 -21
 *     3 BT709_FULL         0     54 183  19    -29  -98 127    127 -116 -11
 *     Y = off + ((cR R + cG G + cB B + 128) >> 8)                       per pixel, with the Y row
 *     U = (S + 131072 + 512) >> 10                                      S = the sum of cR R + cG G + cB B, with the U row, over the four
 *     V = the same with the V row                                           pixels of the 2x2 block
 * One rounding step on the summed block, never two; >> is the arithmetic shift of a number that is never negative here.  No clamp is
 * needed and none is applied.  What the tables guarantee (tests/test_packed_format_cpu.py asserts each): luma rows sum to 220 (limited)
 * and 256 (full), so R = G = B = v gives Y = v at the full matrices; every chroma row sums to 0, so grey gives exactly 128; over the
 * RGB cube limited output stays in [16, 235] / [16, 240] and full output in [0, 255] / [1, 255]; S + 131584 is never negative.  The
 * distance from the floating-point BT.601 / BT.709 definition, measured on 100 000 random pixels, is about 1.6 (full, where 0.5 is
 * carried as 127 / 256) and about 1.1 (limited); the test bounds it by 2.  Every chroma coefficient fits a signed byte and every luma coefficient an unsigned byte -- the device forms the sums with
 * byte dot products -- so keep both properties and the sums if a coefficient is ever changed.  No gamma, no primaries, no siting. */
typedef enum {
    VP8HOST_FORMAT_I420 = 0, VP8HOST_FORMAT_NV12 = 1, VP8HOST_FORMAT_I422 = 2, VP8HOST_FORMAT_I444 = 3,
    VP8HOST_FORMAT_P010 = 4, VP8HOST_FORMAT_I010 = 5, VP8HOST_FORMAT_I210 = 6, VP8HOST_FORMAT_I410 = 7,
    VP8HOST_FORMAT_COUNT = 8,      /* the planar family ends here */
    VP8HOST_FORMAT_PACKED_FIRST = 16,
    VP8HOST_FORMAT_YUY2 = 16, VP8HOST_FORMAT_UYVY = 17, VP8HOST_FORMAT_BGRA = 18, VP8HOST_FORMAT_RGBA = 19,
    VP8HOST_FORMAT_PACKED_END = 20
} vp8host_source_format;
typedef enum {
    VP8HOST_COLOUR_BT601_LIMITED = 0, VP8HOST_COLOUR_BT709_LIMITED = 1, VP8HOST_COLOUR_BT601_FULL = 2, VP8HOST_COLOUR_BT709_FULL = 3,
    VP8HOST_COLOUR_COUNT = 4
} vp8host_colour_matrix;
/* bytes of the planes a frame of width x height hands in (bytes[2] is 0 for the two-plane formats, bytes[1] and bytes[2] for the
 * packed ones).  0, or -1: unknown format, a size that is odd or not positive */
int vp8host_source_plane_bytes(int format, int width, int height, size_t bytes[3]);
/* the rule as plain C++: p0, p1, p2 = the format's planes (p2 is not read for NV12 / P010, p1 and p2 are not read -- and may be null
 * -- for the packed formats, which take matrix 0), y, u, v = tight I420 of width x height.
 * 0, or -1 for what vp8host_source_plane_bytes refuses or a null pointer. */
int vp8host_convert_frame(int format, int width, int height, const uint8_t *p0, const uint8_t *p1, const uint8_t *p2,
                          uint8_t *y, uint8_t *u, uint8_t *v);
/* the same with the colour matrix BGRA / RGBA are read with (the other formats check it and do not use it).  -1 also for a matrix
 * that is none of the four */
int vp8host_convert_frame_colour(int format, int matrix, int width, int height, const uint8_t *p0, const uint8_t *p1, const uint8_t *p2,
                                 uint8_t *y, uint8_t *u, uint8_t *v);
/* the table above: c = the Y, U and V rows one after the other, each in the order R, G, B.  0, or -1: unknown matrix, null pointer */
int vp8host_colour_coefficients(int matrix, int32_t c[9], int32_t *y_offset);

/* OVERLAYS (vp8hip_set_overlay_host / _device, include/vp8hip.h; k_overlay_prepare, k_overlay_b): the ONE integer rule that burns a
 * layer -- a station logo, a watermark, a subtitle, a timecode -- into a frame on its way in.  The project's own.  A LAYER is a plane of
 * lw x lh pixels (1 .. 16384 each) of four bytes, format BGRA (18) or RGBA (19) and no other, STRAIGHT (not premultiplied) alpha, rows
 * `pitch` bytes apart (pitch >= 4 lw; the bytes between the rows are never read), with the position (x, y) of its top-left pixel in
 * PICTURE coordinates (any integers in -16384 .. 16384, odd ones included), an opacity 0 .. 255 and a colour matrix of its own (enum
 * vp8host_colour_matrix; vp8hip_set_source_colour has no say).  The PICTURE is the upright frame the pack or scale launch writes, pw x ph,
 * both even: the source size or the scaler's destination.  Layer pixels outside [0, pw) x [0, ph) are dropped.  Every division below
 * truncates and every operand is non-negative.
 *     e   = (a * opacity + 127) / 255                              the effective alpha of a layer pixel; a picture pixel that no layer
 *                                                                  pixel covers has e = 0
 *     Yo  = off + ((cR R + cG G + cB B + 128) >> 8)                the BGRA rule above, the Y row of the LAYER's matrix
 *     Y   = (src * (255 - e) + Yo * e + 127) / 255                 per picture pixel
 *     c_i = cR R_i + cG G_i + cB B_i + 32768                       per layer pixel, with the U row
 *     E   = sum of e_i (0 .. 1020),  T = sum of e_i c_i            over the four picture pixels (2cx .. 2cx + 1, 2cy .. 2cy + 1) of a
 *                                                                  chroma sample, whatever the parity of x and y
 *     N   = src * 256 * (1020 - E) + T                             below 2^31
 *     U   = ((N + 130560) >> 10) / 255                             V the same with the V row
 * One rounding step per plane and layer; no clamp is needed and none is applied.  Several layers: slots 0 .. VP8HIP_MAX_OVERLAYS - 1 are
 * applied in slot order, each on the result of the one before.  PADDING: the composed coded frame is the composed picture padded as
 * copy_with_padding pads it -- sample (x, y) of the coded surface is composed sample (min(x, pw - 1), min(y, ph - 1)) -- so a layer
 * that touches the picture's last column or row changes the padding samples behind it.
 * What the rule guarantees (tests/test_overlay_cpu.py asserts each): (n + 127) / 255 equals t = n + 128; (t + (t >> 8)) >> 8 for every
 * n in 0 .. 65025, and q / 255 equals (q * 0x8081) >> 23 for every q below 66299 (the chroma q never exceeds 65408), so the device
 * never divides; for an opaque layer (a = 255, opacity = 255) at even x, y with even size the chroma rule is exactly the BGRA rule's
 * (S + 131584) >> 10 and luma is Yo, so such a layer replaces its rectangle with vp8host_convert_frame_colour(BGRA, matrix, ...) of
 * itself, byte for byte; e = 0 changes nothing; over the RGB cube chroma stays in [16, 240] (limited) and [1, 255] (full).
 * Out of scope: premultiplied alpha, 24-bit RGB and YUVA layers, scaling or rotating a layer, text rendering, reading PNG, hidden
 * alt-ref frames (the window frames bypass the intake) and by-reference splits. */
#define VP8HOST_OVERLAY_MAX_SIZE 16384
#define VP8HOST_OVERLAY_MAX_POS 16384
/* the rule as plain C++: ONE layer composed in place onto tight I420 of the picture size pw x ph.  0, or -1 for anything refused: a
 * format other than BGRA / RGBA, an unknown matrix, a size, pitch, position or opacity out of range, a picture size that is odd or not
 * positive, a null pointer */
int vp8host_overlay_frame(int format, int matrix, int lw, int lh, int pitch, const uint8_t *pixels, int x, int y, int opacity, int pw, int ph,
                          uint8_t *yp, uint8_t *up, uint8_t *vp);

/* HDR SOURCES MADE SDR (vp8hip_set_source_transfer, include/vp8hip.h; k_tonemap_b): the ONE integer rule that makes 8-bit SDR I420 of
 * a ten-bit PQ (SMPTE ST 2084, HDR10) or HLG (BT.2100) frame.  The project's own: without it the planar rule above keeps the PQ or HLG
 * signal and the BT.2020 primaries, and a VP8 player, which shows BT.601 / BT.709 SDR, shows PQ grey and flat and HLG dim and
 * desaturated.  It applies to formats P010 (4) and I010 (5) ONLY; with I420 (0) in force a transfer is held and nothing reads it;
 * every other format refuses it.  transfer = one of enum vp8host_transfer; peak P = the display peak the source was graded for, an
 * integer number of nits, 400 .. 10000 (the tools default to 1000).  The source is BT.2020 non-constant-luminance, limited range, ten
 * bits; chroma is the 2x2 block's one (Cb, Cr) pair for all four pixels (no siting, as everywhere here).
 *
 * Per pixel, with y = Y' - 64, cb = Cb - 512, cr = Cr - 512 (every ten-bit code is accepted, those outside 64 .. 940 included; the
 * low six bits of a P010 word and the high six of an I010 word are ignored); >> is the arithmetic shift:
 *     R' = clamp((38295 y            + 55209 cr + 4096) >> 13, 0, 4095)       12-bit full-range BT.2020 R'G'B'
 *     G' = clamp((38295 y -  6161 cb - 21391 cr + 4096) >> 13, 0, 4095)       (every term and sum fits int32)
 *     B' = clamp((38295 y + 70440 cb            + 4096) >> 13, 0, 4095)
 *     m  = max(R', G', B');  g = gain[m];  aR = lin[R'], aG = lin[G'], aB = lin[B']       20-bit linear light, 2^20 = peak
 *     tR = max(0, ( 1701 aR -  602 aG -   75 aB + 512) >> 10)      BT.2020 -> BT.709 primaries, times 1024; every row sums to 1024,
 *     tG = max(0, ( -128 aR + 1161 aG -    9 aB + 512) >> 10)      so grey stays grey exactly; every sum fits int32
 *     tB = max(0, (  -19 aR -  103 aG + 1146 aB + 512) >> 10)
 *     o  = min(65535, (t * g + 2^19) >> 20)       per component; a 64-bit product (at most 21 + 23 bits); 65535 = SDR white, linear
 *     c8 = o < 4096 ? lo[o] : hi[o >> 4]          8-bit full-range R, G, B
 * The I420 output is exactly the BGRA rule above applied to the pixel (B, G, R) = the three c8: Y = off + ((cR R + cG G + cB B + 128)
 * >> 8), U and V from the 2x2 sums, with the colour matrix of vp8hip_set_source_colour (default BT.601 limited).  So a tone-mapped
 * frame EQUALS vp8host_convert_frame_colour(BGRA, matrix, ...) of the c8 picture, byte for byte (tests/test_tonemap_cpu.py holds it
 * to that).
 *
 * The four tables are computed on the host in double, once per (transfer, peak), with e = i / 4095, i = 0 .. 4095:
 *     PQ   p = e^(1/m2),  N = 10000 (max(p - c1, 0) / (c2 - c3 p))^(1/m1) nits  (m1 = 2610/16384, m2 = 128 * 2523/4096, c1 = 3424/4096,
 *          c2 = 32 * 2413/4096, c3 = 32 * 2392/4096);  D = min(N, P) nits;  s = D / P
 *     HLG  s = e^2 / 3 for e <= 1/2, else (exp((e - c) / a) + b) / 12  (a = 0.17883277, b = 0.28466892, c = 0.55991073: BT.2100's inverse
 *          OETF);  D = P s^gamma,  gamma = 1.2 + 0.42 log10(P / 1000).  HERE THE RULE DEPARTS FROM BT.2100: its OOTF takes the
 *          luminance term on Ys = 0.2627 R + 0.6780 G + 0.0593 B, this one takes it on the LARGEST component, m above.  That lets one
 *          gain table, indexed by one scalar, serve both transfers (PQ's tone curve is applied on the largest component too, which
 *          keeps hue and never clips a component the curve has not seen); on grey the two agree exactly, on saturated colours this
 *          one is somewhat darker.
 *     tone curve   x = D / 203 (BT.2408's reference white), w = P / 203,  T = x (1 + x / w^2) / (1 + x): slope 1 at black, T(w) = 1
 *     lin[i]  = min(2^20 - 1, rint(2^20 s))
 *     gain[i] = rint(65535 * 2^20 * T / lin[i]) where lin[i] > 0; the entries below the first non-zero lin take that entry's gain
 *     lo[j]   = rint(255 (j / 65535)^(1/2.4))                          j = 0 .. 4095
 *     hi[j]   = rint(255 (min(16 j + 8, 65535) / 65535)^(1/2.4))       j = 0 .. 4095
 * What the rule guarantees for PQ at 1000, 4000 and 10000 nits and HLG at 400 and 1000 (tests/test_tonemap_cpu.py asserts each): lin,
 * the grey ramp's o and its c8 never decrease; lin[0] = 0 and code 4095 gives c8 = 255; lin stays below 2^20 and gain below 2^23, so t is
 * below 2^21 and t * g below 2^44, far inside 64 bits; grey in (Cb = Cr = 512) gives U = V = 128 exactly.  Measured when the rule was written: 254 of the 256 c8 values
 * occur on the grey ramp, the largest step between neighbouring 12-bit codes is 3, at the very bottom; PQ 203 nits gives c8 191 .. 194
 * and HLG 75 % gives 194; on 100 000 random pixels the matrix sums lie in -0.71e9 .. 1.78e9.  Keep these if a constant is ever
 * changed. */
typedef enum { VP8HOST_TRANSFER_SDR = 0, VP8HOST_TRANSFER_PQ = 1, VP8HOST_TRANSFER_HLG = 2 } vp8host_transfer;
#define VP8HOST_PEAK_MIN 400
#define VP8HOST_PEAK_MAX 10000
/* the four tables of (transfer, peak).  0, or -1: a transfer other than PQ or HLG, a peak outside 400 .. 10000, a null pointer */
int vp8host_tonemap_tables(int transfer, int peak, uint32_t lin[4096], uint32_t gain[4096], uint8_t lo[4096], uint8_t hi[4096]);
/* the rule as plain C++ on those tables: p0, p1, p2 = the planes of a P010 or I010 frame (p2 is not read for P010), y, u, v = tight
 * I420 of width x height.  0, or -1: a format other than P010 or I010, what vp8host_tonemap_tables refuses, an unknown matrix, a size
 * vp8host_source_plane_bytes refuses, a null pointer */
int vp8host_tonemap_frame(int format, int transfer, int peak, int matrix, int width, int height, const uint8_t *p0, const uint8_t *p1,
                          const uint8_t *p2, uint8_t *y, uint8_t *u, uint8_t *v);
/* The C tag of a YUV4MPEG2 header (which vp8host_y4m_parse_header, the reference's parser, never looks at): the header line is the
 * bytes up to the first line feed, its tags are separated by spaces, the first tag that starts with C counts.  No C tag, C420,
 * C420jpeg, C420mpeg2, C420paldv: I420; C422: I422; C444: I444; C420p10: I010; C422p10: I210; C444p10: I410.  Returns 0 and the
 * format, or -1: anything else (Cmono, C444alpha, 12 and 16 bits, ...), no YUV4MPEG2 magic word, or no line feed in the buffer. */
int vp8host_y4m_colourspace(const uint8_t *data, size_t size, int32_t *format);
/* The I tag of the same header line, read the same way (the first tag that starts with I counts).  No I tag, Ip, I?: progressive;
 * It: top field first; Ib: bottom field first.  Returns 0 and one of enum vp8host_field_order, or -1: Im (mixed: the field order is
 * a per-frame parameter this reader does not follow) and any other I tag, no YUV4MPEG2 magic word, or no line feed in the buffer. */
typedef enum { VP8HOST_FIELDS_PROGRESSIVE = 0, VP8HOST_FIELDS_TOP_FIRST = 1, VP8HOST_FIELDS_BOTTOM_FIRST = 2 } vp8host_field_order;
int vp8host_y4m_interlace(const uint8_t *data, size_t size, int32_t *field_order);

/* The rule of the device's deinterlacer (vp8hip_set_deinterlace, include/vp8hip.h; k_deinterlace_b), bit for bit, integers only.  The
 * project's own: VP8 has no interlaced coding tools and the reference does not know what a field is.
 * It applies to each of the three tight I420 planes of the INCOMING size (the scaler's incoming size, else the source size, else the
 * coded size) on its own, after format conversion and before padding, scaling and denoising.  One output frame per input frame: no
 * rate doubling.  keep = the field that survives and defines the output frame's instant: 0 = the top field (rows 0, 2, 4, ...),
 * 1 = the bottom field (rows 1, 3, 5, ...); the same parity in the chroma planes' rows.  With h the plane's rows:
 * KEPT ROWS, y = keep (mod 2), are copied unchanged.
 * SPATIAL VALUE s of a sample of a MISSING row y: the kept rows are K[j] = row 2 j + keep, j = 0 .. n - 1; with
 *     j0 = floor((y - 1 - keep) / 2)          (-1 for y = 0 when keep = 1)
 * the taps are a0 .. a3 = K[j0 - 1], K[j0], K[j0 + 1], K[j0 + 2] in the sample's column, every index clamped to 0 .. n - 1, and
 *     s = clamp(0, 255, (-a0 + 9 a1 + 9 a2 - a3 + 8) >> 4)          (arithmetic shift).
 * MODE 1, field: output = s.  No history.
 * MODE 2, adaptive: a history P is kept, the previous frame taken in as the deinterlacer RECEIVED it (both fields, unprocessed).
 * With cur the frame received, wv = cur[y][x], d(r) = |cur[r][x] - P[r][x]| and m = max(d(y), d(max(y - 1, 0)), d(min(y + 1, h - 1))):
 *     output = min(max(s, wv - m), wv + m).
 * It lies between s and wv: no clamp.  A static sample (m = 0) is woven at full vertical resolution, a moving one gets the field
 * interpolation; there is no threshold.  Without a history -- the first frame, after a restart, after the mode or the parity changed,
 * after the incoming size changed -- output = s, the frame equals mode 1's, and the frame as received becomes the history.
 * The record of a frame: woven = the LUMA samples of missing rows whose output equals wv (0 in mode 1 and without a history),
 * missing = the luma samples of missing rows.  A height below 4 is refused: every plane then has a row of each field.
 * vp8host_deinterlace_frame: the rule on tight planes of width x height (both even, height >= 4; chroma width / 2 x height / 2).
 * mode 0: out = src, *woven = 0, the history is left alone.  mode 1: the history is not read, not written and may be null.  mode 2:
 * the history planes are read when have_history != 0 and are replaced by src (in-out).  out must not overlap src or the history.
 * Returns 0, or -1 for bad arguments. */
int vp8host_deinterlace_frame(const uint8_t *src_y, const uint8_t *src_u, const uint8_t *src_v, uint8_t *hist_y, uint8_t *hist_u,
                              uint8_t *hist_v, uint8_t *out_y, uint8_t *out_u, uint8_t *out_v, int width, int height, int mode, int keep,
                              int have_history, int32_t *woven);

/* The geometry of the input side (vp8hip_set_source_window, vp8hip_set_source_orientation, include/vp8hip.h; k_window_b, k_orient_b),
 * bit for bit: pure data movement.  The project's own: the reference reads tight upright I420.
 * THE WINDOW.  The three pointers of a frame are the plane bases of a SURFACE in the source format whose rows are pitch[p] bytes
 * apart; the frame is the window of width x height luma samples whose top-left luma sample is (x, y).  Plane p of a format has a
 * horizontal shift hs, a vertical shift vs and bytes per element bpe:
 *     I420  0,0,1  1,1,1  1,1,1        P010  0,0,2  1,1,4  -            YUY2, UYVY  1,0,4  -  -
 *     NV12  0,0,1  1,1,2  -            I010  0,0,2  1,1,2  1,1,2        BGRA, RGBA  0,0,4  -  -
 *     I422  0,0,1  1,0,1  1,0,1        I210  0,0,2  1,0,2  1,0,2
 *     I444  0,0,1  0,0,1  0,0,1        I410  0,0,2  0,0,2  0,0,2
 * and of the window it holds rows[p] = height >> vs rows of row_bytes[p] = (width >> hs) * bpe bytes; row r starts at byte
 *     offset[p] + r * pitch[p],   offset[p] = (y >> vs) * pitch[p] + (x >> hs) * bpe
 * of the plane.  The rows end to end are the tight planes vp8host_source_plane_bytes describes (rows * row_bytes is its entry).  No
 * byte outside the window is read; the surface's own size is no parameter; pitch and base need no alignment.
 * vp8host_source_window: the table and the validation.  -1: an unknown format, width or height odd or not positive, x or y negative
 * or odd (even values keep 4:2:0 chroma, YUY2 pairs and field parity whole), a null pointer, or for a plane the format has
 * pitch[p] < ((x + width) >> hs) * bpe.  pitch entries of planes the format lacks are ignored; their offset, row_bytes and rows are 0.
 * vp8host_window_frame: the rule on planes in host memory; out0..out2 = the tight planes (pointers of planes the format lacks are
 * not looked at). */
int vp8host_source_window(int format, int width, int height, int x, int y, const int32_t pitch[3], size_t offset[3],
                          int32_t row_bytes[3], int32_t rows[3]);
int vp8host_window_frame(int format, int width, int height, int x, int y, const int32_t pitch[3], const uint8_t *p0, const uint8_t *p1,
                         const uint8_t *p2, uint8_t *out0, uint8_t *out1, uint8_t *out2);
/* THE ORIENTATION.  turns = 0..3 clockwise quarter turns, mirror = 0 or 1: a left-right flip of the incoming frame FIRST, then the
 * rotation.  For each of the three tight 8-bit I420 planes, `in` the plane as it comes in, rw samples wide and rh high, and
 * s(x, y) = in(mirror ? rw - 1 - x : x, y):
 *     turns 0:  out(x, y) = s(x, y)                      out is rw x rh
 *     turns 1:  out(x, y) = s(y, rh - 1 - x)             out is rh x rw
 *     turns 2:  out(x, y) = s(rw - 1 - x, rh - 1 - y)    out is rw x rh
 *     turns 3:  out(x, y) = s(rw - 1 - y, x)             out is rh x rw
 * The chroma planes take the same rule at their own size (raw_width / 2 x raw_height / 2); both dimensions are even, so 4:2:0 stays
 * exact.  Siting is not modelled.  raw_width x raw_height: the luma size of the planes that come in.  out must not overlap in.
 * Returns 0, or -1: turns or mirror out of range, a size odd or below 2, a null pointer. */
int vp8host_orient_frame(int turns, int mirror, int raw_width, int raw_height, const uint8_t *in_y, const uint8_t *in_u,
                         const uint8_t *in_v, uint8_t *out_y, uint8_t *out_u, uint8_t *out_v);

/* The rules of the frame analysis record (vp8hip_set_analysis, include/vp8hip.h; k_analyse_src_b, k_analyse_mb_b), bit for bit.  The
 * project's own: libvpx's first-pass statistics cut to what this encoder knows.  Every field is an exact integer; no floats anywhere.
 *
 * SOURCE SIDE, once per frame taken in.  cur = the luma plane at the coded size (width and height whole 16x16 macroblocks) as the
 * searches read it: after format conversion, padding or scaling, and denoising; the padding counts because the search sees it.
 * prev = the same plane of the previous frame taken in (the context's history).  With x a sample of cur and p the sample of prev at
 * the same place:
 *     spatial       sum over the macroblocks of  256 * (sum of x * x over its 256 samples) - (sum of x over them) squared,
 *                   i.e. 256 * 256 times the macroblock's variance; uint64
 *     temporal_sse  sum over the plane of (x - p) * (x - p)
 *     temporal_sad  sum over the plane of |x - p|
 *     static_mbs    macroblocks whose sum of |x - p| is 0
 *     have_prev     1; or 0 when there is no history -- the first frame after analysis was turned on or restarted -- and then
 *                   temporal_sse = temporal_sad = static_mbs = 0
 * vp8host_analyse_luma is the rule in plain C++ on tight planes (row stride = width); prev may be NULL (no history).  Returns 0, or
 * -1: cur or out NULL, width or height below 16 or not a multiple of 16.
 *
 * CODING SIDE, a pure function of the per-macroblock arrays of the frame's FINAL coding attempt (a frame check_SSIM sent back and that
 * was coded again as a key frame has the key frame's record), macroblocks in raster order:
 *     parts[MBs]      MB_parts of vp8hip_results: 0 = 16x16, 1 = 8x8
 *     ref[MBs]        MB_reference_frame: 0 LAST, 1 GOLDEN, 2 ALTREF
 *     vec[MBs][4][2]  MB_vectors: the four 8x8 blocks TL, TR, BL, BR, each {x, y} in quarter pixels, int16
 *     nz[MBs]         the non-zero-coefficient counts vp8hip_prepare_filter_mask returns (MB_non_zero_coeffs)
 *     seg[MBs]        MB_segment_id, 0..3 (only the low two bits are looked at)
 *     is_inter[MBs]   the flags vp8hip_download_intra returns, 0 where check_SSIM's fallback replaced the macroblock by an intra one.
 *                     They count only for an inter frame on which check_SSIM ran AND reported replaced > 0; otherwise (no check, or
 *                     nothing replaced: the fallback then leaves the array stale) every macroblock of an inter frame is inter.
 * A macroblock is INTRA in a key frame, and in an inter frame where is_inter counts and is 0; otherwise it is INTER.
 *     mbs_total       MBs
 *     mbs_intra       intra macroblocks (all of a key frame)
 *     mbs_ref[r]      inter macroblocks with ref == r, r = 0, 1, 2 (an inter macroblock with another value is counted in none)
 *     mbs_split       inter macroblocks with parts == 1
 *     mbs_zero_mv     inter macroblocks whose eight vector components are all 0
 *     mv_abs_sum[k]   sum of |vec[mb][b][k]| over b = 0..3 of every inter macroblock, k = 0 (x), 1 (y), whatever parts says; uint64
 *     mv_sum[k]       the same sum without the absolute value; int64
 *     mv_sq_sum       sum of x * x + y * y over the same vectors; uint64
 *     nz_coeffs       sum of nz over ALL macroblocks; uint64
 *     mbs_no_coeffs   macroblocks (all of them) with nz == 0
 *     segment_mbs[s]  macroblocks (all of them) with (seg & 3) == s
 * so mbs_intra + mbs_ref[0] + mbs_ref[1] + mbs_ref[2] = mbs_total = the sum of segment_mbs; in a key frame the five inter fields
 * and mbs_ref are 0. */
typedef struct {
    uint64_t spatial, temporal_sse, temporal_sad;
    int32_t static_mbs, have_prev;
} vp8host_luma_analysis;
int vp8host_analyse_luma(const uint8_t *cur, const uint8_t *prev_or_null, int width, int height, vp8host_luma_analysis *out);

/* The rule of the per-macroblock quantiser (vp8hip_set_segment_mode, include/vp8hip.h; k_aq_map_b, k_aq_seg_b, k_mb_p_map), bit for
 * bit.  The project's own.  Mode 0 is off, mode 1 the caller's map, mode 2 variance-adaptive with strength 1..3.
 *
 * In mode 1 or 2 a macroblock of an INTER frame is coded once, in segment map[mb] & 3, with that segment's row of the segment data in
 * force: the arithmetic of the default's pass with the segment given instead of found.  MB_segment_id[mb] is that value; MB_SSIM is
 * still computed.  Key frames stay as they are (segment 0, no segmentation in the header).
 *
 * Mode 2 makes the map from the coded luma of the current frame as the searches read it (behind window, convert, deinterlace, orient,
 * scale or pack, and denoise; the padded area counts).  All integers:
 *     v(mb)  = 256 * (sum of x * x over the macroblock's 256 samples) - (sum of x over them) squared: the analysis record's
 *              "256 * 256 times the variance", at most 1 065 369 600
 *     n      = v + 1, p = the position of its leading one (n >> p == 1)
 *     frac   = p >= 3 ? (n >> (p - 3)) & 7 : (n << (3 - p)) & 7
 *     e(mb)  = 8 * p + frac: log2 in eighths, piecewise linear, 0 for a flat macroblock, 239 at the largest v
 *     E      = floor(sum of e(mb) over the frame's macroblocks / their number)
 *     W      = 24, 16, 12 for strength 1, 2, 3
 *     seg    = clamp(2 + floor((e - E) / W), 0, 3), the division rounding towards minus infinity
 * so a macroblock of mean activity takes segment 2, flatter ones 1 and then 0 (finer), busier ones 3.
 * vp8host_aq_segment is the last line; vp8host_aq_segment_map is the whole rule in plain C++ on a luma plane of `stride` bytes per row
 * (width and height whole macroblocks): map_out[MBs], e_out[MBs] (may be NULL), raster order.  Returns 0, or -1: luma or map_out
 * NULL, width or height below 16 or not a multiple of 16, stride below width, strength outside 1..3. */
int vp8host_aq_segment(int e, int E, int W);
int vp8host_aq_segment_map(const uint8_t *luma, int stride, int width, int height, int strength, uint8_t *map_out, uint8_t *e_out);

/* The rule of the temporal filter that makes a hidden alternate reference frame (vp8hip_arf_filter_device, include/vp8hip.h;
 * k_arf_filter_b), bit for bit, integers only.  The project's own, after libvpx's --auto-alt-ref / --arnr-maxframes / --arnr-strength:
 * the reference never codes a frame it does not show.
 * IN: n frames (1 <= n <= VP8HOST_ARF_MAX_FRAMES) of tight 8-bit I420 of one size w x h, both even; a centre index c in 0 .. n - 1; a
 * strength s in 0 .. 6.  OUT: one tight I420 frame of w x h.
 * EXTENSION: every plane is read as if extended to We x He = 16 ceil(w / 16) x 16 ceil(h / 16) luma samples (chroma: half of that) by
 * repeating its last column and its last row.  Only the w x h samples are written; there are no partial-tile special cases.
 * PER 16x16 LUMA TILE of the centre frame (top-left (x0, y0), both multiples of 16) AND PER FRAME k != c: a full-pel search over
 * dx, dy in [-8, 7].  A candidate counts only if its block lies inside the extended picture: 0 <= x0 + dx, x0 + dx + 16 <= We,
 * 0 <= y0 + dy, y0 + dy + 16 <= He.  SAD = the sum of |centre - frame k| over the 256 samples.  The winner is the lexicographic minimum
 * of (SAD, |dx| + |dy|, dy, dx), i.e. the minimum of the 29-bit key
 *     SAD << 13 | (|dx| + |dy|) << 8 | (dy + 8) << 4 | (dx + 8).
 * SSE = the sum of squared differences of the winning block against the centre tile, and the BLOCK WEIGHT
 *     bw = 2 if SSE < 10000, 1 if SSE < 20000, else 0          (libvpx's THRESH_LOW and THRESH_HIGH).
 * The centre frame itself has bw = 2 and the zero vector.  The tile's two 8x8 chroma blocks take the full-pel vector
 * (dx >> 1, dy >> 1), arithmetic shifts.
 * PER SAMPLE of every plane, with o the centre frame's sample and, for each frame with bw > 0, p its predicted sample:
 *     d = o - p,   m = (3 d d + r) >> s with r = s ? 1 << (s - 1) : 0,   m = 16 - min(m, 16),   count += m bw,   acc += m bw p
 * and the output sample is (acc + count / 2) / count, integer divisions.  count is at least 32 (the centre gives 16 * 2) and at most
 * 224; acc is at most 255 count, below 65536.  n = 1 returns the centre frame unchanged.
 * THE DIVISION is exact and made by a reciprocal multiply, the same two macros on the host and on the device:
 * VP8HOST_ARF_DIVIDE(acc + count / 2, VP8HOST_ARF_RECIPROCAL(count)).  With R = floor((2^32 - 1) / count) + 1 the error
 * R count - 2^32 lies in [0, count), so floor(x R / 2^32) = floor(x / count) while x count < 2^32: x < 65536 + 112, count <= 224.
 * vp8host_arf_round_divide applies the pair to arrays (for a test that walks every pair that can occur).
 * vp8host_arf_filter_frame: the rule in plain C++.  frames[3 k + p] = plane p of frame k.  weights (may be NULL) receives, for
 * b = 0, 1, 2, the number of (tile, frame k != c) pairs with bw = b; vectors (may be NULL) receives for tile t in raster order and
 * frame k the winner as vectors[(t n + k) 2 + 0] = dx, [.. + 1] = dy (0, 0 for k = c).  out must not overlap a source frame.  Returns 0,
 * or -1: a null pointer, n, centre or strength out of range, w or h odd or below 2. */
#define VP8HOST_ARF_MAX_FRAMES 7
#define VP8HOST_ARF_THRESH_LOW 10000
#define VP8HOST_ARF_THRESH_HIGH 20000
#define VP8HOST_ARF_RECIPROCAL(count) (0xFFFFFFFFu / (uint32_t)(count) + 1u)
#define VP8HOST_ARF_DIVIDE(x, recip) ((uint32_t)(((uint64_t)(uint32_t)(x) * (uint32_t)(recip)) >> 32))
int vp8host_arf_filter_frame(const uint8_t *const *frames, int n, int centre, int strength, int width, int height, uint8_t *out_y,
                             uint8_t *out_u, uint8_t *out_v, int32_t weights[3], int8_t *vectors);
void vp8host_arf_round_divide(const uint32_t *acc, const uint32_t *count, size_t n, uint32_t *out);

/* frames.skip_prob, loop_filter.h:37-44 */
int vp8host_skip_prob(const int32_t *MB_non_zero_coeffs, int mb_count);

/* frame-type state machine, vp8enc.cpp:340-344, 364-374 and intra_part.h:1091-1098 */
typedef struct {
    int32_t gop_size, altref_range;
    int32_t frame_number, frames_until_key, frames_until_altref;
    int32_t golden_frame_number, altref_frame_number;
    int32_t current_is_key, current_is_golden, current_is_altref;
    int32_t prev_is_key, prev_is_golden, prev_is_altref;
} vp8host_gop;

void vp8host_gop_init(vp8host_gop *g, int gop_size, int altref_range);
/* advance to the next input frame; fills the current_* / prev_* flags */
void vp8host_gop_next(vp8host_gop *g);
/* what intra_transform() does to the counters when the current frame is (or is forced to be) a key frame */
void vp8host_gop_key_coded(vp8host_gop *g);
/* flags of inter_transform(), inter_part.h:103-104 */
void vp8host_gop_inter_flags(const vp8host_gop *g, int32_t *use_golden, int32_t *use_altref);
/* ++frames.frame_number at the end of the loop body, vp8enc.cpp:487 */
void vp8host_gop_frame_done(vp8host_gop *g);

/* TEMPORAL LAYERS: which references a shown frame searches, which buffer its reconstruction refreshes and which temporal layer it
 * belongs to, so that a forwarding unit can drop every frame above a layer and what is left still decodes (the patterns WebRTC runs
 * VP8 with).  p = the number of shown frames coded since the last key frame AS FINALLY CODED: the key frame itself is p = 0, and a
 * frame that is forced to be a key frame, or sent back and coded again as one, restarts p -- so the pattern restarts at every key
 * frame, and a closed GOP coded as a chunk of its own gives the bytes the serial program gives.  ref_mask bit 0: GOLDEN may be searched
 * (vp8drv_config.ref_mask).
 *   layers = 1:  every frame temporal_id 0, searches LAST, refreshes LAST.
 *   layers = 2 (period 2):
 *     p % 2 == 0:  temporal_id 0, searches LAST, refreshes LAST
 *     p % 2 == 1:  temporal_id 1, searches LAST, refreshes NONE, layer_sync 1
 *   layers = 3 (period 4):
 *     p % 4 == 0:  temporal_id 0, searches LAST, refreshes LAST
 *     p % 4 == 1:  temporal_id 2, searches LAST, refreshes NONE, layer_sync 1
 *     p % 4 == 2:  temporal_id 1, searches LAST, refreshes GOLDEN only, layer_sync 1
 *     p % 4 == 3:  temporal_id 2, searches LAST and (with ref_mask & 1) GOLDEN, refreshes NONE, layer_sync = !use_golden
 *   p = 0, the key frame:  temporal_id 0, searches nothing, refresh = VP8HOST_REFRESH_ALL, layer_sync 0, whatever `layers`.
 * ALTREF is never searched, and every layer takes its quantisers from the lastqi ladder (vp8host_quantizer_ladders).  layer_sync = 1:
 * the frame depends on temporal layer 0 only, so a receiver may start taking its layer at it.  LAST always holds a temporal_id 0 frame
 * and GOLDEN a frame of temporal_id <= 1 that is newer than LAST when it is searched: a frame never reads a frame of a higher layer.
 * Returns 0, or -1 and leaves *out alone: layers outside 1 .. 3, p < 0, out NULL.  Plain C, no state. */
#define VP8HOST_REFRESH_LAST 0
#define VP8HOST_REFRESH_GOLDEN 1
#define VP8HOST_REFRESH_NONE 2
#define VP8HOST_REFRESH_ALL 3
typedef struct {
    int32_t temporal_id, use_golden, refresh, layer_sync;
} vp8host_temporal;
int vp8host_temporal_step(int layers, int p, int ref_mask, vp8host_temporal *out);

/* CYCLIC INTRA REFRESH: which macroblocks of an inter frame are coded as intra whatever the inter pass made of them, so that a receiver
 * that lost a frame has the whole picture back within one period without a key frame (vp8hip_intra_refresh, include/vp8hip.h;
 * vp8drv_set_intra_refresh, include/vp8hip_driver.h; k_intra_refresh).  The project's own; the reference has no such mode.
 *   P = the period, 4 .. 1024 (VP8HOST_INTRA_REFRESH_MIN / _MAX).
 *   q = the phase of the frame: the number of inter frames since the last key frame AS FINALLY CODED that refreshed LAST, counted
 *       before this frame -- the first inter frame behind a key frame has q = 0, and any key frame (scheduled, forced, a scene cut, a
 *       frame sent back and coded again as one) restarts it.  Frames that refresh GOLDEN only or nothing, and hidden frames, neither
 *       count nor force anything.
 *   Macroblock (r, c) -- row r, column c -- of a shown inter frame that refreshes LAST is FORCED iff (c + 2 r) mod P == q mod P.
 * A forced macroblock is coded as an inter macroblock first, as ever, and then replaced unconditionally by ONE intra attempt, the one
 * check_SSIM's fallback makes: B_PRED luma by pick_luma_predictor, TM_PRED chroma, predicted from the unfiltered reconstruction, with
 * the quantisers of the segment the inter pass left the macroblock in (MB_segment_id: 3 by default, the caller's map or the AQ
 * segment in segment modes 1 and 2); the segment id does not change.  What is written is what the fallback writes: coefficients
 * (blocks 0 .. 23), the unfiltered reconstruction, MB_parts = 2, MB_SSIM = the attempt's value, is_inter = 0, the sixteen sub-block
 * modes, the non-zero count (sum of |coefficient| over blocks 0 .. 23) and filter mask -1.  Every macroblock that is not forced has
 * is_inter = 1 and its sixteen modes 0.
 * Why 2 r: the left, above, above-left and above-right neighbours of a forced macroblock have phases -1, -2, -3 and -1 relative to
 * it, none of which is 0 modulo P for P >= 4 -- so intra prediction (the above-right samples that sub-block rows 1 to 3 take from the
 * row above the macroblock included) reads inter-coded reconstruction only, and the forced macroblocks of a frame may be coded in
 * any order or all at once.  And every macroblock is forced exactly once in any P consecutive phases.
 * Motion vectors are not constrained to the refreshed area, and GOLDEN / ALTREF may carry damage back in: a receiver's recovery
 * within a period is not guaranteed: it depends on the motion (measured: profiles/README.md, "Intra refresh").
 * vp8host_intra_refresh_forced: 1 or 0; -1: period outside 4 .. 1024, or q, r or c negative.
 * vp8host_intra_refresh_count: the forced macroblocks of a frame of mbw x mbh macroblocks at phase q (the sum of the predicate); -1:
 * a bad period, q negative, mbw or mbh below 1.  Plain C, no state. */
#define VP8HOST_INTRA_REFRESH_MIN 4
#define VP8HOST_INTRA_REFRESH_MAX 1024
int vp8host_intra_refresh_forced(int period, int q, int r, int c);
int vp8host_intra_refresh_count(int mbw, int mbh, int period, int q);

/* The key-frame schedule of a whole file with scene detection on, from the chroma differences of its frames alone: nothing but the
 * frame loop's own steps (vp8enc.cpp:364-416, 487), for t = 0 .. nframes - 1:
 *     vp8host_gop_next;
 *     key = current_is_key; a frame that is NOT a scheduled key frame is shown to vp8host_scene_change(udiff[t], vdiff[t], t), and is
 *           a key frame when that says so (a scheduled key frame is never shown to it: its differences are not looked at);
 *     on a key frame: last_key_detect = t, vp8host_gop_key_coded;
 *     vp8host_gop_frame_done.
 * udiff[t], vdiff[t]: vp8hip_chroma_change of frame t against frame t - 1 as taken in; entry 0 is unused.  is_key[t] = 1 for a key frame,
 * by_scene[t] = 1 for one scene_change asked for (by_scene may be NULL).  Returns the number of key frames, or -1: udiff, vdiff or is_key
 * NULL, nframes < 0 or gop_size < 1.  Plain C++, no allocation.  Frames that check_SSIM sends back as key frames are not the schedule's:
 * with an SSIM target the serial program may code more key frames than this plan has. */
int vp8host_scene_plan(const int32_t *udiff, const int32_t *vdiff, int nframes, int gop_size, uint8_t *is_key, uint8_t *by_scene);

#ifdef __cplusplus
}
#endif
#endif
