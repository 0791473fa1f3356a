// vp8hip_dev.h -- shared declarations of the gfx950 inter-frame kernels (internal, not the ABI).
//
// Surfaces: every plane lives in HBM with a PAD-pixel margin on all four sides and a row
// stride that is a multiple of 64 B, so pixel (0,0) is 32-byte aligned, rows of an 8x8 block
// are one aligned 8-byte load, and a search window that hangs over the frame edge is an
// ordinary load (the margin of a reference plane holds the replicated edge = the reference's
// CLK_ADDRESS_CLAMP_TO_EDGE sampler, src/GPU_kernels.cl:562).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/vp8hip.h"

namespace vp8 {

// Per-kernel timing (vp8hip_profile_enable): the launchers of the single-kernel stages go through VP8_LAUNCH, which hands
// the dispatch a start and a stop event when the API layer has set them for this host thread.  Events recorded BY the
// dispatch carry the kernel's own begin / end timestamps (what rocprofv3's kernel trace shows); events recorded around it
// with hipEventRecord also count the time the packet waits for the queue to be scheduled, which with sixteen streams on the
// part is as long again as the kernel (loop filter: 0.70 ms bracketed vs 0.39 ms in the trace).
struct LaunchTiming { hipEvent_t start = nullptr, stop = nullptr; int launches = 0; };
extern thread_local LaunchTiming tl_timing;
#define VP8_LAUNCH(kernel, grid, block, shmem, stream, ...)                                                                               \
    do {                                                                                                                                  \
        ++::vp8::tl_timing.launches;                                                                                                      \
        hipExtLaunchKernelGGL(kernel, grid, block, shmem, stream, ::vp8::tl_timing.start, ::vp8::tl_timing.stop, 0, __VA_ARGS__);         \
    } while (0)

constexpr int PAD = 32;        // allocated margin (pixels) around every plane
constexpr int EXT = 8;         // replicated-edge width actually filled (max reach of any filter: 3)
constexpr int LF_ERR_WORD = 1536;   // int index inside the loop filter's progress buffer of its time-out flag
constexpr int LF_SIMPLE_WORD = 512;  // ... of the simple loop filter's band counters (form 3's sit at 0, the diagnostic stamps at 1024)
constexpr int LF_SIMPLE_WORDS = 512;
constexpr int S2_CLOCK_WORD = LF_ERR_WORD + 32;   // ... and of k_search2's launch clock (five 64-bit words, see launch_clock_end)
constexpr int CLOCK_SAMPLE = 64;    // every 64th workgroup of a launch stamps the clock
constexpr int SD_INTS = 11;    // ints per segment_data, src/vp8enc.h:80-92
enum { SD_Y_AC_I = 0, SD_Y_DC_IDELTA, SD_Y2_DC_IDELTA, SD_Y2_AC_IDELTA, SD_UV_DC_IDELTA, SD_UV_AC_IDELTA,
       SD_LOOP_FILTER_LEVEL, SD_MBEDGE_LIMIT, SD_SUB_BEDGE_LIMIT, SD_INTERIOR_LIMIT, SD_HEV_THRESHOLD };

struct Plane {
    uint8_t *p;   // address of pixel (0,0)
    int stride;   // bytes per row
    int w, h;
};

struct Frame {
    Plane Y[5];   // Y[l] = luma downsampled by 2^l
    Plane U, V;
};

struct RefSet {            // what one search/predict launch needs to know about the references
    Frame ref[3];          // LAST, GOLDEN, ALTREF
    int use[3];
};

// per-reference motion state: two short2 nets (ping-pong, src/init.h:672-854) and the block costs
struct NetSet {
    int16_t *net[3][2];
    int32_t *bdiff[3];
};

struct MBOut {
    int32_t *parts, *ref, *seg, *nz, *mask;
    int16_t *vec;      // [MBs][4][2]
    int16_t *coeffs;   // [MBs][25][16]
    float *ssim;
    int32_t *flags;    // [0]: set by k_mb when a macroblock's SSIM is below the target, i.e. check_SSIM's fallback has work to do;
                       //      cleared by the loop filter launch that carries the verdict (zero at rest)
};

struct SegData { int32_t v[4 * SD_INTS]; };

// ---- batched launches -------------------------------------------------------------------------------------------------
// Measured on MI355X (scripts/ubench/concurrency.hip, and the kernel trace of sixteen GOP chunks on sixteen streams): the
// part runs FOUR TO FIVE kernels at once however many streams offer work, and with more than ~8 active streams the
// hardware queues are time-sliced.  Sixteen chunks each launching its own narrow kernels therefore leave the chip with
// one wide kernel at a time (loop filters of 9 workgroups hold two of the slots on average).  So the same kernels also
// exist in a batched form: ONE launch does a stage for up to MAX_BATCH contexts of equal geometry (blockIdx.z = context),
// the argument blocks of the single form travel as an array in the kernel arguments, and a few streams carry what sixteen did.
constexpr int MAX_BATCH = 8;
template <typename A> struct BatchOf { int n; A item[MAX_BATCH]; };
// What a batched launcher takes is ONE array of member records and what all members share: (stream, const Item *, n, ...).  A context
// on its own is a batch of one.  The intake stages have a record each (PlanesItem, DeinterlaceItem, DenoiseItem, AnalysisSrcItem);
// the coding chain has three, each filled by one function of the API layer from a context (the pointers are the context's own and
// outlive the launch call), and the launchers make the kernels' argument blocks of them:
//   SourceItem  -- pack / scale: where a member's new frame comes from and the surface it goes into (take_frames);
//   CodingItem  -- searches and k_mb: the frame, its references, the nets and where the results go (coding_item);
//   FilterItem  -- the three loop filters: the reconstruction, its results and the filter's own counters (filter_item);
// and ScanRequest, the parameter scan of one frame (scan_request).

// A launch's duration by the kernel's own clock (s_memrealtime, 100 MHz), for kernels of many workgroups: every CLOCK_SAMPLE-th
// workgroup (in dispatch order, the first one included) stamps w = {earliest start, latest end, sampled workgroups done,
// sum over launches of (end - start), launches}; the last sampled workgroup to finish closes the launch.  HIP events around a
// launch also count the time its packet waits for its hardware queue; this does not, and it is what a rocprofv3 kernel trace
// shows.  w[0] is ~0 at rest.  (Stamping every workgroup would put 150 000 atomics per launch on one cache line.)
#if defined(__HIPCC__)
__device__ __forceinline__ bool launch_clock_sampled() {
    const unsigned wg = (blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    return wg % CLOCK_SAMPLE == 0;
}
__device__ __forceinline__ void launch_clock_begin(unsigned long long *w) {
    // A SCALAR condition (the first wave of a sampled workgroup; the compiler folds the wave's atomics into one): with the per-lane
    // "threadIdx.x == 0" here, hipcc carried the workgroup indices through the branch in VGPRs and k_search2 picked its reference's
    // planes and nets with vector loads and 64-bit vector address arithmetic -- 49 of its 771 vector instructions.
    if (w && launch_clock_sampled() && __builtin_amdgcn_readfirstlane((int)threadIdx.x) == 0)
        atomicMin(&w[0], (unsigned long long)__builtin_amdgcn_s_memrealtime());
}
// The lanes of the workgroup's first thread as a wave mask (1 in the first wave, 0 in the others), taken at the kernel's start and held in
// scalar registers: launch_clock_end then asks for no thread number behind the kernel's body, i.e. no vector register kept across it.
__device__ __forceinline__ unsigned long long launch_clock_first_thread() {
    unsigned long long m = __builtin_amdgcn_ballot_w64(threadIdx.x == 0);
    asm volatile("" : "+s"(m));      // (made here, not where it is used)
    return m;
}
__device__ __forceinline__ void launch_clock_end(unsigned long long *w, unsigned long long first_thread) {   // every thread of the workgroup gets here
    if (!w || !launch_clock_sampled()) return;
    __syncthreads();
    if (first_thread == 0 || __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)) != 0) return;      // the mask's one bit is lane 0's
    atomicMax(&w[1], (unsigned long long)__builtin_amdgcn_s_memrealtime());
    __threadfence();
    const unsigned total = gridDim.x * gridDim.y * gridDim.z, sampled = (total + CLOCK_SAMPLE - 1) / CLOCK_SAMPLE;
    if (atomicAdd(&w[2], 1ull) + 1 == sampled) {
        __threadfence();
        const unsigned long long t1 = atomicExch(&w[1], 0ull), t0 = atomicExch(&w[0], ~0ull);
        atomicExch(&w[2], 0ull);
        atomicAdd(&w[3], t1 - t0);
        atomicAdd(&w[4], 1ull);
    }
}
#endif
// Switches that LEAVE WORK OUT of a launch or a wait (the results are then garbage) exist for same-box timing runs only: they
// are compiled in with -DVP8HIP_EXPERIMENTS (scripts/ab_*.sh build that way) and are constants otherwise, so no environment
// can take work out of a run of the shipped library.  vp8hip_experiments_compiled_in() tells a caller which build it has.
#ifdef VP8HIP_EXPERIMENTS
inline bool experiment_skip(const char *what) { const char *v = getenv("VP8HIP_EXPERIMENT_SKIP"); return v && strstr(v, what) != nullptr; }
inline const char *experiment_env(const char *name) { return getenv(name); }
#else
inline bool experiment_skip(const char *) { return false; }
inline const char *experiment_env(const char *) { return nullptr; }
#endif

// ---- launchers (kernels_*.hip) ---------------------------------------------------------------
void launch_border(hipStream_t s, const Frame &f);
// all four levels of one or two frames; bit z of border_mask: also the replicated edges of surface z (launch_border's work, same launch)
void launch_pyramid(hipStream_t s, const Frame *a, const Frame *b, uint32_t border_mask = 0);
// batched form: nframes <= 2 * MAX_BATCH surfaces
void launch_pyramid_batch(hipStream_t s, const Frame *const *f, int nframes, uint32_t border_mask = 0);
// The parameter scan of one frame: loop-filter strength of the luma plane y + prepare_segments_data, all on the device.  What
// launch_auto_segments launches on its own and what launch_search2_batch lets ride along.
struct ScanRequest { Plane y; uint32_t *partial, *stats; SegData *sd; int32_t *strength_out; int is_key; int32_t refqi[4]; int qi_min; };
// kernels_scale.hip: a frame that comes in LARGER than the coded picture is scaled down into the surfaces instead of packed
// (vp8hip_set_source_scaling).  A plan = the four tables (luma x, luma y, chroma x, chroma y) of include/vp8hip_host.h's
// vp8host_scale_taps, stretched over the padded surface, in one device block.
struct ScaleDim { int n, n_in, n_surf; size_t off_start, off_coef; int max_span[4]; };
struct ScalePlan { int in_w = 0, in_h = 0, kind = 0; ScaleDim d[4] = {}; uint8_t *d_blob = nullptr; };
bool scale_plan_make(ScalePlan *p, int in_w, int in_h, int dst_w, int dst_h, int W, int H, int kind, std::vector<uint8_t> &blob);   // false: refused
// Tile and LDS layout of a plan: tw x th outputs per workgroup (64 x 32 unless the ratio is large), the LDS offsets in bytes, the source
// rows per chunk (kernels_scale.hip, scale_geo).  k_compose_b walks a tile's rectangle in blocks of this shape.
struct ScaleGeo { int tw, th, pitch, rows, span_y, off_t, off_cx, off_cy, off_sx, off_sy; };
ScaleGeo scale_geo(const ScalePlan &p);
// A member's new frame: planes y, u, v (tight I420 in device memory by now) on their way into the surface f, packed or, through the
// member's plan, scaled down.
struct SourceItem { const Frame *f; const void *y, *u, *v; const ScalePlan *plan; };
// sw, sh: luma size of the source planes (0 = the coded size); ssy, ssc: their row strides (0 = tight).  NOTE: the timing-experiment
// switch that leaves the BATCHES' pack out (VP8HIP_EXPERIMENT_SKIP=pack) is take_frames' (api_intake.hip), not this launcher's, where
// the other skip switches sit: the launch of one context, which comes through here too, has never been skipped by it.
void launch_pack_batch(hipStream_t s, const SourceItem *items, int n, int sw = 0, int sh = 0, int ssy = 0, int ssc = 0);
void launch_scale_batch(hipStream_t s, const SourceItem *items, int n);
// kernels_compose.hip: a frame composed of scaled video tiles (vp8hip_set_canvas), ONE launch in the place of the pack or scale launch;
// the rule is include/vp8hip_host.h's ("CANVAS").  A plan = the tiles' geometry, block shapes and tables in one device block, made by
// the setter; a launch passes only the frame's pointers and pitches (pitch > 0; y == nullptr: the tile is absent).
struct ComposePlan { uint8_t *d_blob = nullptr; int n = 0; size_t lds = 0; };
struct ComposeSource { const uint8_t *p[3]; int32_t pitch[3]; };
bool compose_plan_make(ComposePlan *p, const vp8hip_tile *tiles, int n, const int bg[3], std::vector<uint8_t> &blob);   // false: refused
// pw x ph: the picture (the surface beyond it repeats its edge)
void launch_compose(hipStream_t s, const Frame &f, const ComposePlan &plan, int pw, int ph, const ComposeSource *src);
// kernels_denoise.hip: temporal noise reduction of the frame just packed or scaled (vp8hip_set_denoise), in place on `cur` against
// `hist`, the previous current frame as it left this launch; the rule is include/vp8hip_host.h's.  `word` (zero at rest) takes the
// count of filtered macroblocks and the waves' tickets; the wave with the last ticket writes the record into `host`, seq last.
struct DenoiseMirror { int32_t frame_number, mbs_filtered, mbs_total; uint32_t seq; };
struct DenoiseItem { Frame cur, hist; unsigned long long *word; DenoiseMirror *host; uint32_t seq; int32_t frame_number; };
void launch_denoise_batch(hipStream_t s, const DenoiseItem *items, int n, int level);
// kernels_analysis.hip: the frame analysis record (vp8hip_set_analysis); both rules are include/vp8hip_host.h's.
// k_analyse_src_b: the coded luma of the frame just taken in against `hist`, a tight plane of w x h bytes that the same launch then
// overwrites with the luma; have_prev 0: measures `spatial` and copies only.  `acc` (five 64-bit words, zero at rest) takes the
// workgroups' sums and tickets; the workgroup with the last ticket writes the record into `host`, seq last.
// k_analyse_mb_b: one workgroup per frame over the per-macroblock arrays; `replaced` = the device copy of check_SSIM's verdict (word 0:
// macroblocks replaced) when the check ran on this attempt, else nullptr (is_inter is then not read) -- unless `forced`: the attempt
// carries forced intra macroblocks (vp8hip_intra_refresh), whose launch wrote every macroblock's is_inter.
struct AnalysisSrcMirror { uint64_t spatial, sse, sad; int32_t static_mbs, have_prev, frame_number; uint32_t seq; };
struct AnalysisMbMirror {
    int32_t frame_number, is_key, mbs_total, mbs_intra, mbs_split, mbs_zero_mv, mbs_no_coeffs, mbs_ref[3], segment_mbs[4];
    uint64_t mv_abs_sum[2]; int64_t mv_sum[2]; uint64_t mv_sq_sum, nz_coeffs;
    uint32_t seq;
};
struct AnalysisMirror { AnalysisSrcMirror src[2]; AnalysisMbMirror mb; };      // src[frame_number & 1]: a frame handed over early keeps the last one's
struct AnalysisSrcItem { Plane cur; uint8_t *hist; unsigned long long *acc; AnalysisSrcMirror *host; uint32_t seq; int32_t frame_number, have_prev; };
struct AnalysisMbItem {
    const int32_t *parts, *ref, *seg, *nz, *is_inter, *replaced;
    const int16_t *vec;
    AnalysisMbMirror *host;
    uint32_t seq;
    int32_t frame_number, is_key, mbs, forced;
};
void launch_analyse_src_batch(hipStream_t s, const AnalysisSrcItem *items, int n);
void launch_analyse_mb_batch(hipStream_t s, const AnalysisMbItem *items, int n);
// kernels_aq.hip: the variance-adaptive segment map (vp8hip_set_segment_mode, mode 2); the rule is include/vp8hip_host.h's.
// k_aq_map_b: e of every macroblock of the coded luma just taken in, a byte each, and their sum added into `sum` (zero at rest);
// k_aq_seg_b behind it turns them into `map`, a byte per macroblock, and leaves the word zero.  e and map are 256-byte aligned and whole multiples of 256 bytes long.
struct AqItem { Plane cur; uint8_t *e, *map; uint32_t *sum; };
void launch_aq_map_batch(hipStream_t s, const AqItem *items, int n);
void launch_aq_seg_batch(hipStream_t s, const AqItem *items, int n, int strength);      // right behind it, on the same stream
// kernels_convert.hip: source frames in another format than 8-bit I420 (vp8hip_set_source_format), made tight 8-bit I420 of the same
// size IN FRONT of the pack or scale launch, which then reads dst as if the caller had handed it in; the rule is include/vp8hip_host.h's.
// src: the format's planes (src[2] is not read for the two-plane formats, src[1] and src[2] for the packed ones, k_convert_packed_b).
// matrix: the colour matrix BGRA / RGBA are read with (vp8hip_set_source_colour).  Format 0 launches nothing.  false: a format or
// matrix the setters refuse -- nothing was launched and the staging buffer is NOT the frame.
// PlanesItem, the record of every stage in front of the pack or scale launch that has no history: a member's three planes in, its three
// planes (in a staging buffer of the context) out.
struct PlanesItem { const uint8_t *src[3]; uint8_t *dst[3]; };
bool launch_convert_batch(hipStream_t s, int format, int matrix, int w, int h, const PlanesItem *items, int n);
// ... and with a transfer in force (vp8hip_set_source_transfer; P010 / I010 only): k_tonemap_b in k_convert_b's place, the same items,
// the same tight I420 out.  tables: the four tables of vp8host_tonemap_tables end to end in device memory (lin, gain, lo, hi: 40 KiB);
// matrix: the colour matrix the SDR picture is written with.  false: a format or matrix the rule does not cover (nothing was launched)
constexpr int TONEMAP_TABLE_BYTES = 4096 * (4 + 4 + 1 + 1);
bool launch_tonemap_batch(hipStream_t s, int format, int matrix, int w, int h, const uint32_t *tables, const PlanesItem *items, int n);
// kernels_deinterlace.hip: interlaced source frames made progressive (vp8hip_set_deinterlace) BEHIND the convert launch and IN FRONT of
// the pack or scale launch, which then reads dst as it reads a converted frame; the rule is include/vp8hip_host.h's.  src: tight I420
// of w x h; hist: the previous frame as received (all nullptr: no history -- the spatial value everywhere); keep_hist: where this
// frame goes verbatim, the next frame's history (all nullptr in mode 1); none of the four overlap.  `word` (zero at rest) takes the
// count of woven luma samples and the waves' tickets; the wave with the last ticket writes the record into `host`, seq last.
struct DeinterlaceMirror { int32_t frame_number, woven, missing; uint32_t seq; };
struct DeinterlaceItem {
    const uint8_t *src[3], *hist[3];
    uint8_t *dst[3], *keep_hist[3];
    unsigned long long *word;
    DeinterlaceMirror *host;
    uint32_t seq;
    int32_t frame_number;
};
void launch_deinterlace_batch(hipStream_t s, int w, int h, int keep, const DeinterlaceItem *items, int n);
// kernels_geometry.hip: the two geometric stages of the input side; the rules are include/vp8hip_host.h's.  Both move bytes from a
// member's src planes to its dst planes (a staging buffer of the context), which do not overlap.
// k_window_b (vp8hip_set_source_window) IN FRONT of everything: src = the plane bases of a surface, dst = the tight planes of the
// window end to end; offset, pitch, row_bytes, rows: vp8host_source_window's (rows[p] == 0: the format has no plane p).
// k_orient_b (vp8hip_set_source_orientation) BEHIND the deinterlacer and IN FRONT of the pack or scale launch: tight I420 of
// raw_w x raw_h in, tight I420 of the upright size out (raw_h x raw_w for an odd number of turns).
void launch_window_batch(hipStream_t s, const size_t offset[3], const int32_t pitch[3], const int32_t row_bytes[3], const int32_t rows[3],
                         const PlanesItem *items, int n);
void launch_orient_batch(hipStream_t s, int turns, int mirror, int raw_w, int raw_h, const PlanesItem *items, int n);
// kernels_overlay.hip: layers burnt into the frame just packed or scaled (vp8hip_set_overlay_host / _device), in place on the current
// surface IN FRONT of the denoiser; the rule is include/vp8hip_host.h's.  A layer's PREPARED PLANES (k_overlay_prepare, when the layer
// is set or moved) lie in one device buffer: Yo at 0 and e at off_e, lh rows of lstride bytes whose column 0 is picture column X0 =
// x & ~3; E (16 bits) at off_E, T_u and T_v (32 bits) at off_tu and off_tv, crows rows of cstride samples whose sample (0, 0) is chroma
// sample (CX0, cy0) of the picture; both strides are multiples of 4 and every plane starts on a multiple of 256 bytes.
struct OverlayPlanes { int X0, lstride, CX0, cy0, cstride, crows; size_t off_e, off_E, off_tu, off_tv, bytes; };
OverlayPlanes overlay_planes(int lw, int lh, int x, int y);
struct OverlayLayer { const uint8_t *base; size_t off_e, off_E, off_tu, off_tv; int X0, y, lstride, lh, CX0, cy0, cstride, crows; };
// a member's frame and its layers in slot order; ux0 .. ux1, uy0 .. uy1: the box of the layers in units of 8 luma columns and 2 luma
// rows, inside the coded surface
struct OverlayItem { Plane y, u, v; int n, ux0, ux1, uy0, uy1; OverlayLayer layer[VP8HIP_MAX_OVERLAYS]; };
// false: a format or matrix the setters refuse (nothing was launched)
bool launch_overlay_prepare(hipStream_t s, int format, int matrix, const uint8_t *pixels, int lw, int lh, int x, int y, int opacity, uint8_t *planes);
void launch_overlay_batch(hipStream_t s, const OverlayItem *items, int n, int pw, int ph);      // pw x ph: the picture inside the coded surface
// kernels_arf.hip: the temporal filter of a hidden alternate reference frame (vp8hip_arf_filter_device); the rule is
// include/vp8hip_host.h's.  src: n frames of tight I420 of w x h in device memory; dst: the filtered frame, tight, which overlaps none
// of them; weights: ARF_WEIGHT_SLOTS 64-bit words (the caller zeroes them in front of the launch) whose SUM holds the (tile, frame) pairs
// by block weight 0, 1, 2 in three fields of 21 bits (at most 6 pairs a tile: room for 349 000 tiles).
constexpr int ARF_WEIGHT_SLOTS = 32;
struct ArfItem { const uint8_t *src[7][3]; uint8_t *dst[3]; unsigned long long *weights; int w, h, n, centre, strength; };
void launch_arf_filter(hipStream_t s, const ArfItem &item);
// check_SSIM's verdict riding in a loop filter launch (see CheckItem below)
struct LfCheck {
    int on, qi_min;
    int32_t refqi[4];
    const int32_t *is_inter;
    int32_t *strength;       // {reductor, sharpness, sharpness in force}
    int32_t *stats;          // device copy of the verdict (vp8hip_check_ssim's read-back buffer)
    int32_t *verdict;        // host memory the device writes: the five words, then seq
    uint32_t seq;
};
// One member's frame in the searches and k_mb.  recon, out, sd: k_mb's (a launch of the searches alone does not read them).
// scan (or nullptr): the member's parameter scan still waiting for a launch to ride in (launch_search2_batch).
// seg_map: the member's segment map, a byte per macroblock, for the mapped form of k_mb (nullptr there: segment 3 everywhere).
struct CodingItem {
    const Frame *cur;
    RefSet refs;
    const NetSet *nets;
    const Frame *recon;
    const MBOut *out;
    const SegData *sd;
    const ScanRequest *scan;
    const uint8_t *seg_map;
};
// One member's reconstruction in a loop filter launch.  launch_no counts the member's launches of THAT filter (the normal forms share
// one count, the simple filter has its own); handoff: form 4's buffer; chk.on = 0: no check rides along.
struct FilterItem {
    const Frame *recon;
    const MBOut *out;
    SegData *sd;
    int32_t *progress;
    void *handoff;
    unsigned launch_no;
    LfCheck chk;
};
void launch_search1_batch(hipStream_t s, const CodingItem *items, int n, int level, int src_idx, int net_width);
// Members with a scan get their loop-filter strength scan + segment data in this launch.  Returns false if the scans were NOT
// carried (nothing to search, or the persistent form): the caller launches them on their own.
bool launch_search2_batch(hipStream_t s, const CodingItem *items, int n, unsigned long long *clk = nullptr);   // clk: launch clock words (launch_clock_end) or nullptr
// (one context: a batch of one -- the kernel is the same)
// mapped: every macroblock is coded once, in the segment its member's seg_map names (vp8hip_set_segment_mode; the packed form only)
void launch_mb_batch(hipStream_t s, const CodingItem *items, int n, float ssim_target, int mbw, int mbh, bool conformant = false, bool mapped = false);
void launch_loop_filter3_batch(hipStream_t s, const FilterItem *items, int n, int mbw, int mbh, bool conformant = false);   // conformant: vp8hip_conformant_stream, the carried registers saturate
void launch_loop_filter4_batch(hipStream_t s, const FilterItem *items, int n, int mbw, int mbh, bool conformant = false);
void launch_auto_segments_batch(hipStream_t s, const ScanRequest *q, int n);
// The forms of ONE video (kernels of their own; the argument blocks are made as the batched forms make them).
// levels 4, 3, 2, 1 in ONE launch (kernels_me.hip, k_search1_coarse); leaves the level-1 net where the per-level launches leave it
void launch_search1_coarse(hipStream_t s, const CodingItem &it, int net_width);
void launch_search1(hipStream_t s, const CodingItem &it, int level, int src_idx, int net_width);
void launch_search2(hipStream_t s, const CodingItem &it, unsigned long long *clk = nullptr);
void launch_weight_tap(hipStream_t s, const int32_t *d, int n, int32_t *out);
void launch_weight_tap_mfma(hipStream_t s, const int32_t *d, int n, int32_t *out);
void launch_weight_tap_mfma_rows(hipStream_t s, const int32_t *d, int n, int32_t *out);
void launch_round_pack4_tap(hipStream_t s, const int32_t *v, int n, uint32_t *out);   // kernels_s2.hip: n quadruples through round_pack4
void launch_filter_mask(hipStream_t s, const MBOut &o, const SegData *d_sd, int mbs);
// The loop filter exists in two forms with the same results.  Form 3 (lf_banded.h): byte tiles and strips in 46 KB
// of LDS, the worker wave does everything itself -- what batches of GOP chunks launch, and only they (with the part full what counts is the
// instructions and the LDS a launch takes from the other kernels, not its latency).  Form 4: a band-tall plane of dwords in
// 112 KB of LDS, the workers only filter, porter waves feed and drain -- the short dependency chain of ONE video.
void launch_loop_filter4(hipStream_t s, const FilterItem &it, int mbw, int mbh, int stall_test = 0, bool conformant = false);
size_t loop_filter4_handoff_bytes(int mbw, int mbh);   // the HBM buffer form 4 hands a band's bottom rows to the next band through
// The simple loop filter (frame header filter_type 1, kernels_lf_simple.hip): luma only, form 3's data movement (lf_banded.h).  launch_no counts
// the context's simple-filter launches only (its band counters are its own, at LF_SIMPLE_WORD of the progress buffer).
void launch_loop_filter_simple(hipStream_t s, const FilterItem &it, int mbw, int mbh);
void launch_loop_filter_simple_batch(hipStream_t s, const FilterItem *items, int n, int mbw, int mbh);
bool loop_filter_simple_fits(int mbh);   // its band counters fit their window of the progress buffer

// ---- quality of the coded frames (kernels_quality.hip; vp8hip_set_quality_stats) --------------------------------------------
// k_quality: one wave per tile of QUALITY_TILE_COLS x QUALITY_TILE_ROWS 4x4 blocks of one plane, all three planes in one launch; a
// tile's partial sums go to `partial`, and the last wave to finish (an integer ticket) reduces them in a fixed order, folds the
// previous record into the sums when it belongs to another frame, and writes the state (and its host mirror, then `seq`).
constexpr int QUALITY_TILE_COLS = 63;   // block columns a wave owns (lane 63 loads the column right of them for the windows)
constexpr int QUALITY_TILE_ROWS = 8;    // block rows a wave owns (it walks one more for the windows)
struct QualitySums {                    // the frames made final (vp8hip_quality_totals before the means)
    int64_t frames;
    uint64_t sse[3], samples[3];
    double psnr_all_sum, ssim_all_sum, ssim_sum[3], psnr_min;
    int64_t psnr_min_frame;
};
struct QualityState {
    vp8hip_quality pending;             // the last frame measured (not yet in `sums`)
    int32_t has_pending;
    uint32_t seq;                       // host mirror: the launch that wrote it (written last)
    QualitySums sums;
};
struct QualityPartial { unsigned long long sse; double ssim; };
struct QualityPlane { const uint8_t *s, *r; int ss, rs, w, h; };   // source, reconstruction, their strides; the region measured
struct QualityArgs {
    QualityPlane p[3];
    QualityPartial *partial;            // quality_tiles() entries
    unsigned *ticket;                   // zero at rest
    QualityState *state;                // device copy
    QualityState *host;                 // host mirror, or nullptr
    uint32_t seq;
    int32_t frame_number, is_key;
};
int quality_tiles(int w, int h);        // waves of one launch for a luma region of w x h (chroma ((w + 1) / 2) x ((h + 1) / 2))
// the region of `src` (w x h luma) measured against `rec` (planes of the same layout)
QualityArgs quality_args(const Frame &src, const Frame &rec, int w, int h);
void launch_quality(hipStream_t s, const QualityArgs &a);
void launch_quality_batch(hipStream_t s, const QualityArgs *a, int n);
// the host's view of a state: the sums with the pending record folded in, as means
void quality_totals(const QualityState &st, vp8hip_quality_totals *t);

// per-frame parameter scans on the device copy of the current frame (kernels_rc.hip); stats = 4 uint32
size_t rc_partial_words();   // uint32 words of per-workgroup partial sums the three launchers below need
void launch_lf_strength(hipStream_t s, const Frame &cur, uint32_t *partial, uint32_t *stats);    // [0] sum Y, [1] sum of squared deviations
void launch_chroma_sad(hipStream_t s, const Frame &cur, const Frame &prev, uint32_t *partial, uint32_t *stats);   // [2] sum |dU|, [3] sum |dV|
void launch_auto_segments(hipStream_t s, const ScanRequest &q);   // strength + prepare_segments_data, all on the device
// the chroma scan of n <= MAX_BATCH contexts of one geometry in ONE launch, fold included: words[0] = sum |dU|, words[1] = sum |dV| (host memory the device writes)
struct ChromaScan { const Frame *cur, *prev; uint32_t *partial, *words; };
void launch_chroma_sad_batch(hipStream_t s, const ChromaScan *q, int n);

// coefficient entropy stage (kernels_ent.hip): flags + third context + token histogram + probabilities
constexpr int ENT_NCTX = 4 * 8 * 3 * 11;
constexpr int ENT_MAX_PARTITIONS = 8;
#if !defined(VP8HIP_ENT_CHUNK)
#define VP8HIP_ENT_CHUNK 256
#endif
constexpr int ENT_CHUNK = VP8HIP_ENT_CHUNK;   // bools per chunk of the parallel boolean coder (kernels_ent.hip)
void launch_ent_count(hipStream_t s, const MBOut &o, uint8_t *flags, uint8_t *third_ctx, uint32_t *counts, uint32_t *probs,
                      uint32_t *denom0, int mbw, int mbh, int num_partitions, const uint8_t *defaults = nullptr);   // defaults: see hdr_default_coeff_probs
// layout of one frame's bool strings / chunks / output words per partition; written by the device, read by the host
struct EntPlan {
    uint32_t bool_base[ENT_MAX_PARTITIONS + 1], chunk_base[ENT_MAX_PARTITIONS + 1], word_base[ENT_MAX_PARTITIONS + 1];
    uint32_t nbools[ENT_MAX_PARTITIONS], w_end[ENT_MAX_PARTITIONS], nbytes[ENT_MAX_PARTITIONS];
    uint32_t total_chunks, overflow;
};
struct EntBuffers {          // device scratch of the boolean coder (allocated on first use)
    uint32_t *offs, *tile_sum;      // bools per block slot -> exclusive offsets; scan tile sums
    uint16_t *bools;                // (probability | bit << 8) per bool, partition after partition
    uint32_t *maps;                 // [chunk][128 start ranges] -> end range | shifts << 8
    void *start;                    // uint2 [chunk]: true start range and bit position
    void *acc;                      // uint64 per 32 output bits
    uint8_t *bytes;                 // the partitions, at 4 * word_base[p]
    int32_t *sizes;
    EntPlan *plan;
    uint32_t cap_bools, cap_chunks, cap_words;
};
void launch_ent_encode(hipStream_t s, const MBOut &o, const uint8_t *third_ctx, const uint32_t *probs, const EntBuffers &eb,
                       int mbw, int mbh, int P, bool code = true);   // code = false: bool strings only, the coder is launched by the caller

void launch_scan_exclusive(hipStream_t s, uint32_t *v, uint32_t *tile_sum, int n);   // in place, total in v[n]
// the coder on bool strings laid out per eb.plan (accumulators cleared by the emit kernel); eb.maps holds
// cap_chunks chunk maps followed by the super-chunk maps (ent_maps_entries)
void launch_bool_code(hipStream_t s, const EntBuffers &eb, int P);
// the plan (k_ent_plan) of P bool strings laid end to end, eb.offs[0..P] = their prefix sums (vp8hip_debug_bool_code)
void launch_bool_plan(hipStream_t s, const EntBuffers &eb, int P);
// the coder on the coefficient partitions and the first partition at once, its last kernel laying the finished frame
// out (gather_frame): frame[0] = frame size (0 = overflow), frame[1] = first-partition size, frame bytes from frame + 16
void launch_frame_code(hipStream_t s, const EntBuffers &coef, int P, const EntBuffers &hdr, uint32_t head, uint32_t capacity, uint8_t *frame);
inline size_t ent_maps_entries(uint32_t cap_chunks) { return ((size_t)cap_chunks + cap_chunks / 8 + 2 * ENT_MAX_PARTITIONS) * 128; }

// first partition on the device (kernels_hdr.hip): encode_header, src/entropy_host.cpp:709-1256
struct HdrFrame { int is_key, is_golden, is_altref, loop_filter_type, sharpness /* INT32_MIN: the device's */, partitions_log2; };
void launch_default_probs(hipStream_t s, uint32_t *probs, const uint32_t *denom0);   // vp8enc.cpp:69-76
const uint8_t *hdr_default_coeff_probs();   // device address of the default coefficient probabilities [4][8][3][11] (RFC 6386 13.5)
constexpr int HDR_STAT_WORDS = 84;   // per-workgroup partial sums of k_hdr_count
void launch_hdr_encode(hipStream_t s, const MBOut &o, const int32_t *is_inter, const int32_t *modes, const HdrFrame &f, const SegData *d_sd,
                       const int32_t *strength, const uint32_t *probs, const uint32_t *denom0, const EntBuffers &eb, uint32_t *partial,
                       uint8_t *sym, uint32_t *info, int mbw, int mbh, bool code = true);

// the frame path of the entropy stage (kernels_entropy_stage.hip): the same steps sharing launches
struct FrameEntropy {
    MBOut o;
    uint8_t *flags, *third;
    uint32_t *counts, *probs, *denom0;
    const EntBuffers *coef, *hdr;    // coef->offs receives bools per slot, coef->tile_sum the sums per 256 slots
    uint32_t *hdr_partial, *hdr_info;
    uint8_t *hdr_sym;
    const int32_t *is_inter, *modes;
    HdrFrame f;
    const SegData *d_sd;
    const int32_t *strength;
    int mbw, mbh, P;
};
void launch_fe_count(hipStream_t s, const FrameEntropy &e);   // counts, probabilities, layout of the coefficient partitions
void launch_fe_emit(hipStream_t s, const FrameEntropy &e);    // frame header + both bool strings; then launch_frame_code
// the frames of up to MAX_BATCH contexts of one geometry in the same nine launches (blockIdx.z = member; the coder takes
// the job pairs 2m, 2m + 1)
struct FrameOut { uint8_t *frame; uint32_t head, capacity; };
void launch_fe_count_batch(hipStream_t s, const FrameEntropy *e, int n);
void launch_fe_emit_batch(hipStream_t s, const FrameEntropy *e, int n);
void launch_frame_code_batch(hipStream_t s, const FrameEntropy *e, const FrameOut *fo, int n);

// host intra path on the device (kernels_intra.hip): key frames (key = 1) and check_SSIM's intra fallback (key = 0).
// prog: mbh ints (row progress), zeroed by the launcher; err: time-out flag; stats out: {replaced, new_SSIM, min SSIM, time-out flag}
// gen: the launch number on this progress buffer (the rows' counters carry it, so nothing has to be cleared between launches)
void launch_intra(hipStream_t s, const Frame &cur, const Frame &recon, const MBOut &o, const SegData *d_sd, int32_t *modes,
                  int32_t *is_inter, int32_t *prog, unsigned gen, int32_t *err, float target, int key, int mbw, int mbh, int stall_test = 0,
                  int modes_of_kept = 0);   // modes_of_kept: vp8hip_conformant_stream
void launch_ssim_stats(hipStream_t s, const MBOut &o, const int32_t *is_inter, int mbs, const int32_t *err, int32_t *out);   // out[3] = *err
// check_SSIM() (src/vp8enc.cpp:231-263) for up to MAX_BATCH contexts without a host round trip and without a launch that is
// not there anyway.  The intra fallback is a launch of its own whose workgroups leave at once unless k_mb has flagged a
// macroblock below the target (o.flags[0]); it also renews nz / mask of the macroblocks it replaces.  The statistics and what
// the host does with them ride in the loop filter's launch (LfCheck): every band takes the minimum SSIM itself and, above
// 0.95, filters with the segment data prepare_segments_data(1, 7) gives; one extra workgroup sums the frame's SSIM in the
// reference's order, writes the updated segment data back for the entropy stage (strength[2], the sharpness the frame header
// carries, becomes 7), clears the flag and hands {replaced, new_SSIM, min SSIM, time-out flag, filter updated, seq} to the
// host through memory the host polls -- the verdict is there long before the filter has finished.
struct CheckItem {
    const Frame *cur, *recon;
    const MBOut *o;
    const SegData *sd;
    int32_t *modes, *is_inter, *prog, *err;
    unsigned gen;
};
void launch_check_fallback(hipStream_t s, const CheckItem *items, int n, float target, int mbw, int mbh, int modes_of_kept);
void launch_intra_key_batch(hipStream_t s, const CheckItem *items, int n, int mbw, int mbh);   // the key frames of n members of a batch, one launch
// cyclic intra refresh (k_intra_refresh; the rule: include/vp8hip_host.h): the forced macroblocks of an inter frame at phase q of
// `period`, each by a workgroup of its own on a grid of (ceil(mbw / period) + 1, mbh) -- no list, no ordering, no waits -- and
// is_inter = 1 / modes = 0 for every other macroblock by the last workgroup of each row
void launch_intra_refresh(hipStream_t s, const Frame &cur, const Frame &recon, const MBOut &o, const SegData *d_sd, int32_t *modes,
                          int32_t *is_inter, int period, int q, int mbw, int mbh);

// ---- device helpers ---------------------------------------------------------------------------
#if defined(__HIPCC__)
__device__ __forceinline__ int iabs(int v) { return v < 0 ? -v : v; }
__device__ __forceinline__ int sat8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }
__device__ __forceinline__ int imin(int a, int b) { return a < b ? a : b; }
__device__ __forceinline__ int imax(int a, int b) { return a > b ? a : b; }
__device__ __forceinline__ int iclamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ int byte_of(uint32_t w, int k) { return (int)((w >> (8 * k)) & 0xffu); }

// The workgroups of a launch go to the part's eight XCDs round-robin by their linear index, and every XCD has an L2 of its own.  A
// kernel whose workgroup x works on tile x therefore spreads every neighbourhood of the frame over all eight L2s: the reference rows
// two vertically adjacent search windows share, the 128-byte line two horizontally adjacent tiles share, are fetched once per XCD
// that meets them (k_search2: 3.5 x its algorithmic bytes, profiles/pmc_traffic.json of round 3).  With this map the workgroups an
// XCD is given (x = k mod 8) work on ONE contiguous run of tiles -- a band of the frame -- so a line is fetched by the one L2 whose
// band it lies in (and by a neighbour's at a band's edge).  A bijection of [0, n) for any n.
__device__ __forceinline__ int xcd_band(int x, int n) {
#if defined(VP8HIP_NO_XCD_BANDS)
    (void)n;
    return x;
#else
    const int k = x & 7, chunk = n >> 3, rem = n & 7;
    return k * chunk + (k < rem ? k : rem) + (x >> 3);
#endif
}

// VP8 quantiser index -> step tables (RFC 6386 14.1; the reference keeps them at GPU_kernels.cl:58-80)
static __device__ __constant__ const int k_dc_q[128] = {
    4,   5,   6,   7,   8,   9,   10,  10,  11,  12,  13,  14,  15,  16,  17,  17,  18,  19,  20,  20,  21,  21,
    22,  22,  23,  23,  24,  25,  25,  26,  27,  28,  29,  30,  31,  32,  33,  34,  35,  36,  37,  37,  38,  39,
    40,  41,  42,  43,  44,  45,  46,  46,  47,  48,  49,  50,  51,  52,  53,  54,  55,  56,  57,  58,  59,  60,
    61,  62,  63,  64,  65,  66,  67,  68,  69,  70,  71,  72,  73,  74,  75,  76,  76,  77,  78,  79,  80,  81,
    82,  83,  84,  85,  86,  87,  88,  89,  91,  93,  95,  96,  98,  100, 101, 102, 104, 106, 108, 110, 112, 114,
    116, 118, 122, 124, 126, 128, 130, 132, 134, 136, 138, 140, 143, 145, 148, 151, 154, 157};
static __device__ __constant__ const int k_ac_q[128] = {
    4,   5,   6,   7,   8,   9,   10,  11,  12,  13,  14,  15,  16,  17,  18,  19,  20,  21,  22,  23,  24,  25,
    26,  27,  28,  29,  30,  31,  32,  33,  34,  35,  36,  37,  38,  39,  40,  41,  42,  43,  44,  45,  46,  47,
    48,  49,  50,  51,  52,  53,  54,  55,  56,  57,  58,  60,  62,  64,  66,  68,  70,  72,  74,  76,  78,  80,
    82,  84,  86,  88,  90,  92,  94,  96,  98,  100, 102, 104, 106, 108, 110, 112, 114, 116, 119, 122, 125, 128,
    131, 134, 137, 140, 143, 146, 149, 152, 155, 158, 161, 164, 167, 170, 173, 177, 181, 185, 189, 193, 197, 201,
    205, 209, 213, 217, 221, 225, 229, 234, 239, 245, 249, 254, 259, 264, 269, 274, 279, 284};
__device__ __forceinline__ int qi(int v) { return iclamp(v, 0, 127); }

// prepare_segments_data(), src/vp8enc.cpp:129-221, from the strength pair of get_loopfilter_strength (:96-127).
// update_filter: check_SSIM's call prepare_segments_data(1, 7) (:155-159, :260-261): reductor doubled, sharpness 7.
// Returns video.loop_filter_sharpness as it stands afterwards (what the frame header carries).  One thread.
__device__ __forceinline__ int fill_segment_data(SegData *sd, int is_key, const int refqi[4], int qi_min, int reductor, int sharpness,
                                                 bool update_filter) {
    if (update_filter) { reductor *= 2; sharpness = 7; }
    int32_t *v = sd->v;
    for (int i = 0; i < 4 * SD_INTS; ++i) v[i] = 0;
    v[SD_Y_DC_IDELTA] = 15;                         // segment 0 carries the deltas, :133-148
    v[SD_UV_DC_IDELTA] = is_key ? 0 : -15;
    v[SD_UV_AC_IDELTA] = is_key ? 0 : -15;
    for (int i = 0; i < 4; ++i) {
        int32_t *s = v + SD_INTS * i;
        s[SD_Y_AC_I] = is_key ? qi_min : refqi[i];  // :164
        const int y_dc_q = k_dc_q[qi(s[SD_Y_AC_I] + v[SD_Y_DC_IDELTA])];
        int lvl = y_dc_q / reductor;                // :187-189
        lvl = lvl > 63 ? 63 : (lvl < 0 ? 0 : lvl);
        s[SD_LOOP_FILTER_LEVEL] = lvl;
        int il = lvl;                               // :192-199
        if (sharpness) {
            il >>= sharpness > 4 ? 2 : 1;
            if (il > 9 - sharpness) il = 9 - sharpness;
        }
        if (!il) il = 1;
        s[SD_INTERIOR_LIMIT] = il;
        s[SD_MBEDGE_LIMIT] = ((lvl + 2) * 2) + il;
        s[SD_SUB_BEDGE_LIMIT] = (lvl * 2) + il;
        int hev = 0;                                // :204-220
        if (is_key) hev = lvl >= 40 ? 2 : (lvl >= 15 ? 1 : 0);
        else hev = lvl >= 40 ? 3 : (lvl >= 20 ? 2 : (lvl >= 15 ? 1 : 0));
        s[SD_HEV_THRESHOLD] = hev;
    }
    return sharpness;
}

__device__ __forceinline__ uint32_t ld_u32(const uint8_t *p) {  // byte-aligned dword load
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
}
__device__ __forceinline__ uint2 ld_u64(const uint8_t *p) {     // byte-aligned 8-byte load
    uint2 v;
    __builtin_memcpy(&v, p, 8);
    return v;
}

// The block-match metric (src/GPU_kernels.cl:85-190, weight_opt): sum of |coefficients| of a 4x4
// forward transform of the difference block, DC/4.  Column pass keeps the reference's quirk (its b1
// is overwritten; rows 1 and 3 use the raw r2).  d = 4 rows x 4 columns, row-major.
// The two rotations x*2217 + y*5352 + k and y*2217 - x*5352 + k are one v_dot2_i32_i16 each on the
// packed pair (x,y): every operand fits int16 (|x|,|y| <= 16320 in the row pass, <= 4080 in the
// column pass for 8-bit pixel differences).
typedef short s16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t pk16(int lo, int hi) { return __builtin_amdgcn_perm((uint32_t)hi, (uint32_t)lo, 0x05040100u); }
__device__ __forceinline__ int dot2(uint32_t xy, uint32_t k, int c) {
    // clamp (int32 saturation, never reached here) selects the three-address VOP3P form that takes the
    // rounding constant straight from an SGPR; without it hipcc emits v_dot2c + a v_mov per use
    return __builtin_amdgcn_sdot2(__builtin_bit_cast(s16x2, xy), __builtin_bit_cast(s16x2, k), c, true);
}
constexpr uint32_t K_ROT_A = 2217u | (5352u << 16);              // (x, y) . ( 2217, 5352)
constexpr uint32_t K_ROT_B = (uint32_t)(-5352 & 0xffff) | (2217u << 16);  // (x, y) . (-5352, 2217)

typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ s16x2 as_s16x2(uint32_t v) { return __builtin_bit_cast(s16x2, v); }
__device__ __forceinline__ uint32_t as_u32(s16x2 v) { return __builtin_bit_cast(uint32_t, v); }
// sum of |lo| + |hi| of a packed pair of int16, added to acc: one xor + one v_sad_u16
__device__ __forceinline__ uint32_t abs_acc(s16x2 v, uint32_t acc) {
    return __builtin_amdgcn_sad_u16(as_u32(v) ^ 0x80008000u, 0x80008000u, acc);
}

// ---- the form the search kernels use --------------------------------------------------------------------------
// Issue cost on gfx950 (scripts/ubench/valu_cost.hip, profiles/valu_cost.json): only plain VOP1/VOP2 add / sub / logic /
// right shifts issue in ~2.3 SIMD cycles; every SDWA, VOP3 and VOP3P instruction (perm, sad, dot2, dot4, v_pk_*,
// even v_lshlrev_b32) costs ~4.2.  So the metric is organised to need the FEWEST instructions, whatever their kind:
//   * a 4x4 block arrives as four COLUMN dwords (byte r = row r), pixels biased by -128 (signed bytes);
//   * the column pass is linear in the pixels except for two rounding shifts, and the current block is the same for
//     every candidate: its share is computed once per column (weight_pre_column: four dot4) and each candidate only adds
//     the prediction's share with ONE v_dot4_i32_i8 per quantity, the accumulator input carrying the current block's:
//         R0 = 8(r0+r1-r2+r3), R2 = 8(r0-r1+r2+r3), X = 16 r2, Y = 32 (r0-r3)        (r = current - prediction)
//   * the two rotations take (X, Y) as one packed pair: scaled by 16 so that ">> 12" becomes "the high half":
//         R1 = (2217 r2 + 5352*8 (r0-r3) + 14500) >> 12 = (2217 X + 21408 Y + 16*14500) >> 16,
//         R3 = (2217*8 (r0-r3) - 5352 r2 + 7500) >> 12 = (8868 Y - 5352 X + 16*7500) >> 16
//     (|X| <= 4080, |Y| <= 8160, sums < 2^28: exact);
//   * row pass on PAIRS of rows in packed 16-bit (every intermediate fits int16 for 8-bit pixel differences:
//     |R| <= 8160, |a1|,|b1| <= 16320, |a1 +- b1 + 7| <= 32647), |a|+|b| of a pair = xor + one v_sad_u16.
// 9 instructions per column instead of 4 byte subtractions + 13: the device metric is pinned on 200k random and on the
// extreme difference blocks by test_block_match_metric_device_vs_oracle through k_weight_tap.  The search kernels' hot forms run the
// column pass on the matrix cores instead (weight_mfma below; pinned the same way through k_weight_tap_mfma).
constexpr uint32_t pk8s(int a, int b, int c, int d) {
    return (uint32_t)(a & 255) | ((uint32_t)(b & 255) << 8) | ((uint32_t)(c & 255) << 16) | ((uint32_t)(d & 255) << 24);
}
constexpr uint32_t K_W_R0 = pk8s(8, 8, -8, 8), K_W_R2 = pk8s(8, -8, 8, 8), K_W_X = pk8s(0, 0, 16, 0), K_W_Y = pk8s(32, 0, 0, -32);
constexpr uint32_t K_W_R0N = pk8s(-8, -8, 8, -8), K_W_R2N = pk8s(-8, 8, -8, -8), K_W_XN = pk8s(0, 0, -16, 0), K_W_YN = pk8s(-32, 0, 0, 32);
constexpr uint32_t K_ROT16_A = 2217u | (21408u << 16);                       // (X, Y) . (2217, 21408)
constexpr uint32_t K_ROT16_B = (uint32_t)(-5352 & 0xffff) | (8868u << 16);   // (X, Y) . (-5352, 8868)
// clamp (int32 saturation, never reached: |sums| < 2^15) selects the three-address VOP3P form; without it hipcc emits the
// two-address v_dot4c plus a v_mov per use to keep the accumulator input alive
__device__ __forceinline__ int dot4s(uint32_t a, uint32_t k, int c) { return __builtin_amdgcn_sdot4((int)a, (int)k, c, true); }

// the current block's share of one column (ccol = its four rows as biased bytes): {R0, R2, X, Y} parts
__device__ __forceinline__ void weight_pre_column(uint32_t ccol, int pre[4]) {
    pre[0] = dot4s(ccol, K_W_R0, 0);
    pre[1] = dot4s(ccol, K_W_R2, 0);
    pre[2] = dot4s(ccol, K_W_X, 0);
    pre[3] = dot4s(ccol, K_W_Y, 0);
}

// Row pass of the metric on the column pass's output: A[c] = (R0[c], R1[c]) = rows 0,1 of column c, B[c] = rows 2,3.
// |a| + |b| of a packed pair is one v_sad_u16 against a constant once the pair carries a bias that makes it
// unsigned; the biases ride on work that is done anyway: +0x8000 joins the rounding 7 of a1 (then ">> 4" is a LOGICAL
// shift and the pair comes out with +2048: floor((x + 32768) / 16) = floor(x / 16) + 2048), and +2^28 joins the rounding
// constants of the rotations (the high half comes out with +4096; |sums| < 2^28, so nothing saturates).
// ... the part behind the butterfly, for one pair of rows: o0, o2 = (a1 + b1 + 7 + 0x8000) >> 4 and (a1 - b1 + 7 + 0x8000) >> 4 of the pair,
// xy_lo / xy_hi = (c1, d1) of its first / second row, d1 = the pair's d1; adds the pair's eight |coefficients| (with their biases taken off) to acc
__device__ __forceinline__ uint32_t weight_rows_tail(uint32_t o0, uint32_t o2, uint32_t xy_lo, uint32_t xy_hi, uint32_t d1, uint32_t acc) {
    const int t1l = dot2(xy_lo, K_ROT_A, 12000 + (1 << 28)), t1h = dot2(xy_hi, K_ROT_A, 12000 + (1 << 28));
    const int t3l = dot2(xy_lo, K_ROT_B, 51000 + (1 << 28)), t3h = dot2(xy_hi, K_ROT_B, 51000 + (1 << 28));
    // (x >> 16) of both rows = the high halves, packed (+4096 each)
    const uint32_t o1 = __builtin_amdgcn_perm((uint32_t)t1h, (uint32_t)t1l, 0x07060302u);
    const uint32_t o3 = __builtin_amdgcn_perm((uint32_t)t3h, (uint32_t)t3l, 0x07060302u);
    // |o1 + (d1 != 0)| per half: the +1 rides in the subtrahend of the absolute difference.
    // d1 != 0, per half: min(d1 as unsigned, 1), one v_pk_min_u16 (was sub / or / shift / and on the pair).  The 1s pass
    // through an empty asm: min(x, 1) with a constant hipcc can see becomes x != 0, which it scalarises into two v_cmp and
    // two v_cndmask per pair.
    uint32_t ones = 0x00010001u;
    asm("" : "+s"(ones));
    const uint32_t nz = __builtin_bit_cast(uint32_t, __builtin_elementwise_min(__builtin_bit_cast(u16x2, d1), __builtin_bit_cast(u16x2, ones)));
    acc = __builtin_amdgcn_sad_u16(o0, 0x08000800u, acc);
    acc = __builtin_amdgcn_sad_u16(o1, 0x10001000u - nz, acc);
    acc = __builtin_amdgcn_sad_u16(o2, 0x08000800u, acc);
    return __builtin_amdgcn_sad_u16(o3, 0x10001000u, acc);
}
// ... and the end: o00 = the DC in its low half, still carrying its +2048 (the high half may hold anything)
__device__ __forceinline__ int weight_rows_end(uint32_t acc, uint32_t o00) {
    const int a00 = (int)__builtin_amdgcn_sad_u16(o00 & 0xffffu, 2048u, 0u);   // |DC| (the high halves are both zero)
    return (int)acc - (a00 - (a00 >> 2));   // DC counts a quarter (DC_UNSIGNIFICANCE, :83,:183)
}
__device__ __forceinline__ int weight_rows(const s16x2 A[4], const s16x2 B[4]) {
    uint32_t acc = 0, o00 = 0;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const s16x2 *X = h == 0 ? A : B;
        const s16x2 a1 = X[0] + X[3], d1 = X[0] - X[3], b1 = X[1] + X[2], c1 = X[1] - X[2];
        const u16x2 a7 = __builtin_bit_cast(u16x2, a1) + u16x2{0x8007, 0x8007};
        const u16x2 o0 = (a7 + __builtin_bit_cast(u16x2, b1)) >> u16x2{4, 4};
        const u16x2 o2 = (a7 - __builtin_bit_cast(u16x2, b1)) >> u16x2{4, 4};
        const uint32_t xy_lo = __builtin_amdgcn_perm(as_u32(d1), as_u32(c1), 0x05040100u);   // (c1, d1) of the first row
        const uint32_t xy_hi = __builtin_amdgcn_perm(as_u32(d1), as_u32(c1), 0x07060302u);   // ... of the second row
        acc = weight_rows_tail(__builtin_bit_cast(uint32_t, o0), __builtin_bit_cast(uint32_t, o2), xy_lo, xy_hi, as_u32(d1), acc);
        if (h == 0) o00 = __builtin_bit_cast(uint32_t, o0);
    }
    return weight_rows_end(acc, o00);
}

// weight of (current - prediction) for one 4x4 block: pre = weight_pre_column of the four current columns,
// p = the four prediction columns as biased bytes
__device__ __forceinline__ int weight_cols_pre(const int pre[16], const uint32_t p[4]) {
    s16x2 A[4], B[4];   // A[c] = (R0[c], R1[c]) = rows 0,1 of the column-pass output, B[c] = rows 2,3
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int R0 = dot4s(p[c], K_W_R0N, pre[4 * c + 0]);
        const int R2 = dot4s(p[c], K_W_R2N, pre[4 * c + 1]);
        const int X = dot4s(p[c], K_W_XN, pre[4 * c + 2]);
        const int Y = dot4s(p[c], K_W_YN, pre[4 * c + 3]);
        const uint32_t xy = pk16(X, Y);
        const int t1 = dot2(xy, K_ROT16_A, 16 * 14500);
        const int t3 = dot2(xy, K_ROT16_B, 16 * 7500);
        A[c] = as_s16x2(__builtin_amdgcn_perm((uint32_t)t1, (uint32_t)R0, 0x07060100u));   // (low half of R0, high half of t1)
        B[c] = as_s16x2(__builtin_amdgcn_perm((uint32_t)t3, (uint32_t)R2, 0x07060100u));
    }
    return weight_rows(A, B);
}

// ---- the column pass on the matrix cores -------------------------------------------------------------------------
// The 16 dot4 of weight_cols_pre are a product of a constant 16 x 16 int8 table W with the 16 prediction bytes (column-dword order), plus
// the current block's share.  ONE v_mfma_i32_32x32x32_i8 (D = A.B + C) does that for the 64 lanes of a wave at once, each lane
// on its own block (lane maps pinned by scripts/ubench/mfma_i8_layout.hip):
//   * A and B: lane l holds k = 16 (l >> 5) + j, j = 0..15, of row l & 31 (A) or column l & 31 (B);
//   * D: register r of lane l holds row (r & 3) + 8 (r >> 2) + 4 (l >> 5), column l & 31.
// So a lane's 16 result registers are exactly the rows whose bit 2 equals its half h = l >> 5, and its 16 B bytes are exactly the
// k of that half.  A is made BLOCK-DIAGONAL: a row with bit 2 = h reads only k in [16h, 16h + 16), and both diagonal blocks are W,
// with row m = (i & 3) + 8 (i >> 2) + 4h holding W's row i.  Then register i of lane l is W[i] . (its own 16 bytes) + (its own C[i]):
// nothing crosses lanes.  An MFMA runs for the whole wave whatever EXEC says: call weight_mfma only where every lane is active.
// One MFMA holds the SIMD's vector issue for 8 cycles where the 16 dot4 (VOP3P, ~4.2 each) took ~67.
//
// The product is free, so it also does the part of the ROW pass that is linear in the pixels.  Rows 0 and 2 of the column pass (R0[c],
// R2[c]) are linear; rows 1 and 3 come out of the rotations with their rounding shift.  The row pass begins, for every row, with the
// butterfly a1 = R[0] + R[3], b1 = R[1] + R[2], c1 = R[1] - R[2], d1 = R[0] - R[3], then a1 +- b1 + 7: for rows 0 and 2 that is a
// linear function of the 16 bytes, and W delivers it directly.  The 16 quantities of a lane (METRIC_*):
//     s0 = R0[0] + R0[1] + R0[2] + R0[3]   (a1 + b1)      m0 = R0[0] - R0[1] - R0[2] + R0[3]   (a1 - b1)
//     c0 = R0[1] - R0[2]                                  d0 = R0[0] - R0[3]
//     s2, m2, c2, d2: the same over R2;   X[c], Y[c] of the four columns, as in weight_cols_pre.
// Every weight is +-8, +-16 or +-32 (an int8); a row of W has non-zero bytes in up to all four dwords of the lane.  The current
// block's share is the C input (weight_pre_block), and the s and m of it carry the row pass's 7 + 0x8000 (see weight_rows).
// Behind the MFMA the rows are paired (1, 3) and (0, 2): pair (1, 3) is packed from the rotations' high halves and takes the whole row
// pass; pair (0, 2) needs no butterfly at all, only the packing of (s0, s2), (m0, m2), (c0, d0), (c2, d2) and (d0, d2).
// The result is the integer weight_cols_pre computes:
//   * the row pass treats every row alike and the metric is a sum of absolute values: which rows share a packed pair does not matter,
//     and the DC is still the low half of the pair that holds row 0;
//   * ranges, for 8-bit pixel differences: |R0[c]|, |R2[c]| <= 8 * 4 * 255 = 8160, so |c|, |d| <= 16320 fit int16 and the packing of
//     their low halves loses nothing; |s|, |m| <= 4 * 8160 = 32640, |s + 7|, |m + 7| <= 32647 < 2^15: s + 7 + 0x8000 lies in
//     [0, 65536) and its low 16 bits ARE the unsigned 16-bit value (a1 + 7 + 0x8000) + b1 of weight_rows (the sums agree modulo 2^16
//     and both lie in the range), so ">> 4" on the packed low halves sees what it saw; only the low 16 bits of s and m are used.
typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));
// the order of a lane's 16 quantities: result registers of the MFMA, ints of its C input
enum { METRIC_S0, METRIC_M0, METRIC_C0, METRIC_D0, METRIC_S2, METRIC_M2, METRIC_C2, METRIC_D2, METRIC_X /* + c */, METRIC_Y = 12 /* + c */ };
// W: the weights of quantity i on the four rows of prediction column c (the prediction counts negative)
constexpr uint32_t metric_w(int i, int c) {
    if (i >= METRIC_X) return (i & 3) != c ? 0u : i >= METRIC_Y ? K_W_YN : K_W_XN;
    const uint32_t pos = i < METRIC_S2 ? K_W_R0N : K_W_R2N, neg = i < METRIC_S2 ? K_W_R0 : K_W_R2;   // + R[c], - R[c] of the difference
    switch (i & 3) {
    case METRIC_S0: return pos;
    case METRIC_M0: return c == 0 || c == 3 ? pos : neg;
    case METRIC_C0: return c == 1 ? pos : c == 2 ? neg : 0u;
    default: return c == 0 ? pos : c == 3 ? neg : 0u;
    }
}
struct MetricTable { uint32_t w[64][4]; };   // the A operand, lane l's four dwords
constexpr MetricTable make_metric_a() {
    MetricTable t{};
    for (int l = 0; l < 64; ++l) {
        const int m = l & 31, h = l >> 5;
        if (((m >> 2) & 1) != h) continue;                  // off the diagonal: zero
        const int i = (m & 3) + 4 * (m >> 3);               // the result register row m lands in
        for (int c = 0; c < 4; ++c) t.w[l][c] = metric_w(i, c);   // k = 16h + 4c + r: row r of column c
    }
    return t;
}
static __device__ __constant__ const MetricTable K_METRIC_A = make_metric_a();
// this lane's A operand: read once per wave, kept in four registers
__device__ __forceinline__ v4i metric_a(int wave_lane) { return *reinterpret_cast<const v4i *>(K_METRIC_A.w[wave_lane & 63]); }
// The order of k inside a half is free in an int8 product as long as A and B agree.  The same operand for a prediction that arrives as four ROW
// dwords (byte c = column c): k = 16h + 4r + c, so byte c of dword r is the weight on row r of column c -- the per-lane 4x4 byte transpose of
// K_METRIC_A.  The whole-pel search's loop form takes it: a candidate's B operand is then four bytes of each reference row as loaded, no transpose.
// The C input (weight_pre_block) and everything behind the product do not depend on the order of k.
constexpr MetricTable make_metric_a_rows() {
    MetricTable t{};
    for (int l = 0; l < 64; ++l) {
        const int m = l & 31, h = l >> 5;
        if (((m >> 2) & 1) != h) continue;
        const int i = (m & 3) + 4 * (m >> 3);
        for (int r = 0; r < 4; ++r)
            for (int c = 0; c < 4; ++c) t.w[l][r] |= ((metric_w(i, c) >> (8 * r)) & 255u) << (8 * c);
    }
    return t;
}
static __device__ __constant__ const MetricTable K_METRIC_A_ROWS = make_metric_a_rows();
__device__ __forceinline__ v4i metric_a_rows(int wave_lane) { return *reinterpret_cast<const v4i *>(K_METRIC_A_ROWS.w[wave_lane & 63]); }

// The current block's share of the 16 quantities (the C input of weight_mfma), from its four columns (cc[c] = the four rows of column c
// as biased bytes), is two halves of the same shape: {s, m, c, d} of a row + one of X / Y for the four columns, with the weights k_r
// (K_W_R0 or K_W_R2) and k_xy (K_W_X or K_W_Y).  From the per-column R with adds: 8 dot4 + 6 adds for a half, where a dot4 chain per
// quantity would be 16 dot4.  s and m carry the 7 and the bias of the row pass (see weight_rows).
__device__ __forceinline__ void weight_pre_half(const uint32_t cc[4], uint32_t k_r, uint32_t k_xy, int smcd[4], int xy[4]) {
    int R[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        R[c] = dot4s(cc[c], k_r, 0);
        xy[c] = dot4s(cc[c], k_xy, 0);
    }
    const int a7 = R[0] + R[3] + 0x8007, b = R[1] + R[2];
    smcd[METRIC_S0] = a7 + b;
    smcd[METRIC_M0] = a7 - b;
    smcd[METRIC_C0] = R[1] - R[2];
    smcd[METRIC_D0] = R[0] - R[3];
}
__device__ __forceinline__ void weight_pre_block(const uint32_t cc[4], int pre[16]) {
    weight_pre_half(cc, K_W_R0, K_W_X, pre + METRIC_S0, pre + METRIC_X);
    weight_pre_half(cc, K_W_R2, K_W_Y, pre + METRIC_S2, pre + METRIC_Y);
}

// weight of (current - prediction) for one 4x4 block per lane: a = metric_a, c = weight_pre_block of the current block, p = the four
// prediction columns as biased bytes.  The same value as weight_cols_pre.
__device__ __forceinline__ int weight_mfma(v4i a, v16i c, v4i p) {
    const v16i d = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, p, c, 0, 0, 0);
    // rows 1 and 3: the rotations per column, their high halves packed (R1[c], R3[c]), then one h iteration of weight_rows
    s16x2 P[4];
#pragma unroll
    for (int col = 0; col < 4; ++col) {
        const uint32_t xy = pk16(d[METRIC_X + col], d[METRIC_Y + col]);
        const int t1 = dot2(xy, K_ROT16_A, 16 * 14500);
        const int t3 = dot2(xy, K_ROT16_B, 16 * 7500);
        P[col] = as_s16x2(__builtin_amdgcn_perm((uint32_t)t3, (uint32_t)t1, 0x07060302u));
    }
    uint32_t acc = 0;
    {
        const s16x2 a1 = P[0] + P[3], d1 = P[0] - P[3], b1 = P[1] + P[2], c1 = P[1] - P[2];
        const u16x2 a7 = __builtin_bit_cast(u16x2, a1) + u16x2{0x8007, 0x8007};
        const u16x2 o0 = (a7 + __builtin_bit_cast(u16x2, b1)) >> u16x2{4, 4};
        const u16x2 o2 = (a7 - __builtin_bit_cast(u16x2, b1)) >> u16x2{4, 4};
        const uint32_t xy_lo = __builtin_amdgcn_perm(as_u32(d1), as_u32(c1), 0x05040100u);
        const uint32_t xy_hi = __builtin_amdgcn_perm(as_u32(d1), as_u32(c1), 0x07060302u);
        acc = weight_rows_tail(__builtin_bit_cast(uint32_t, o0), __builtin_bit_cast(uint32_t, o2), xy_lo, xy_hi, as_u32(d1), acc);
    }
    // rows 0 and 2: the butterfly came out of the product
    const u16x2 o0 = __builtin_bit_cast(u16x2, pk16(d[METRIC_S0], d[METRIC_S2])) >> u16x2{4, 4};
    const u16x2 o2 = __builtin_bit_cast(u16x2, pk16(d[METRIC_M0], d[METRIC_M2])) >> u16x2{4, 4};
    acc = weight_rows_tail(__builtin_bit_cast(uint32_t, o0), __builtin_bit_cast(uint32_t, o2), pk16(d[METRIC_C0], d[METRIC_D0]),
                           pk16(d[METRIC_C2], d[METRIC_D2]), pk16(d[METRIC_D0], d[METRIC_D2]), acc);
    return weight_rows_end(acc, __builtin_bit_cast(uint32_t, o0));
}
// C of weight_mfma from the 16 ints at pre16 (16-byte aligned): four 16-byte loads
__device__ __forceinline__ v16i load_pre16(const int *pre16) {
    v16i c;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const v4i v = *reinterpret_cast<const v4i *>(pre16 + 4 * j);
        c[4 * j] = v.x; c[4 * j + 1] = v.y; c[4 * j + 2] = v.z; c[4 * j + 3] = v.w;
    }
    return c;
}

// (Tried for the whole-pel search, where a reference column is the prediction column of up to four candidates: the four linear
// quantities of a column made once, as packed pairs (R0, R2) and (X, Y), and a (current, prediction) pair as two packed
// subtractions + the rotations + two permutes.  7 % fewer instructions in k_search1, but 75-79 registers instead of 61 -- six waves per
// SIMD instead of eight -- and the same or a lower rate with the part full: 68.1-68.5 and 67.4-67.7 against 68.4-68.7 M MB/s.)

// 4x4 byte transpose: rows r[0..3] (byte k = column k) -> columns (byte r = row r); eight v_perm
__device__ __forceinline__ void transpose4x4(const uint32_t r[4], uint32_t c[4]) {
    const uint32_t t0 = __builtin_amdgcn_perm(r[1], r[0], 0x05010400u);   // r0.b0 r1.b0 r0.b1 r1.b1
    const uint32_t t1 = __builtin_amdgcn_perm(r[1], r[0], 0x07030602u);   // r0.b2 r1.b2 r0.b3 r1.b3
    const uint32_t t2 = __builtin_amdgcn_perm(r[3], r[2], 0x05010400u);
    const uint32_t t3 = __builtin_amdgcn_perm(r[3], r[2], 0x07030602u);
    c[0] = __builtin_amdgcn_perm(t2, t0, 0x05040100u);
    c[1] = __builtin_amdgcn_perm(t2, t0, 0x07060302u);
    c[2] = __builtin_amdgcn_perm(t3, t1, 0x05040100u);
    c[3] = __builtin_amdgcn_perm(t3, t1, 0x07060302u);
}

// VP8 six-tap filters by 1/8-pel phase, src/GPU_kernels.cl:563-572
static __device__ __constant__ const int8_t k_sixtap[8][8] = {
    {0, 0, 127, 0, 0, 0, 0, 0}, /* phase 0 is the identity: handled explicitly (tap 128 does not fit) */
    {0, -6, 123, 12, -1, 0, 0, 0},   {2, -11, 108, 36, -8, 1, 0, 0}, {0, -9, 93, 50, -6, 0, 0, 0},
    {3, -16, 77, 77, -16, 3, 0, 0},  {0, -6, 50, 93, -9, 0, 0, 0},   {1, -8, 36, 108, -11, 2, 0, 0},
    {0, -1, 12, 123, -6, 0, 0, 0},
};
__device__ __forceinline__ void load_taps(int phase, int f[6]) {
#pragma unroll
    for (int t = 0; t < 6; ++t) f[t] = k_sixtap[phase][t];
    if (phase == 0) f[2] = 128;
}
// sat8(s >> 7), written as clamp-then-shift.  The shift-then-saturate form is pattern-matched by
// hipcc (ROCm 7.2) into v_ashr_pk_u8_i32, whose result the compiler then ORs with further bytes as
// if bits 31:16 were zero; on gfx950 they keep the previous contents of the destination VGPR
// (0xffff after a negative sum), which corrupted two neighbouring pixels.  Found by the parity tests.
__device__ __forceinline__ int sat8_shr7(int s) { return iclamp(s, 0, 32767) >> 7; }
// (sum + 64)/128 with C truncation toward zero
__device__ __forceinline__ int div128(int s) { return (s + ((s >> 31) & 127)) >> 7; }   // s / 128 toward zero
#endif

}  // namespace vp8
