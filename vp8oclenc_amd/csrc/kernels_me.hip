// kernels_me.hip -- motion estimation side of the inter-frame path for gfx950:
//   packing of a new frame into its padded surface, edge replication, pyramid, hierarchical full-pel search
//   (the quarter-pel search is kernels_s2.hip, the reference choice is inside k_mb).
// Behaviour follows the reference kernels cited at each kernel (paths under the reference's src/); the parallel
// decomposition is new (k_search1: a lane per candidate row of an 8x8 block walking five candidates over the
// row's eight bytes -- transposed columns in the dot4 forms, the rows as loaded in the loop forms, whose metric
// is one MFMA per candidate with a row-order A table --, the winner by a minimum of packed (cost, index) keys:
// a shuffle tree, or through LDS in the batched loop form, which packs 51 blocks into a workgroup's 256 lanes,
// s1_fill_layout.h).  Every kernel has a single and a batched form (blockIdx.z = context, vp8hip_dev.h).
#include <stdlib.h>
#include <string.h>

#include "vp8hip_dev.h"
#include "s1_pre_layout.h"
#include "s1_fill_layout.h"

namespace vp8 {

// ------------------------------------------------------------------------------------------------
// Edge replication of a reference frame's Y/U/V planes (replaces the clamp-to-edge image sampler,
// GPU_kernels.cl:562).  grid = (max rows + 2*EXT, 3 planes), block = 64.
// ------------------------------------------------------------------------------------------------
struct BorderItem { Plane y, u, v; };
// one row (-EXT .. h + EXT - 1) of one plane by the 64 lanes of a wave.  Rows start 32-byte aligned and plane widths are multiples
// of 8 (vp8hip_create: frame sizes are multiples of 16), so a row above or below the plane is copied eight bytes per lane and step
// and either margin is ONE eight-byte store of the edge sample (byte by byte a full 1080p row was 30 dependent rounds per lane, and
// the 48 such rows of a frame made the pyramid-and-edges launch twice as long as the pyramid alone).
static_assert(EXT == 8, "border_row stores a margin as one eight-byte word");
__device__ __forceinline__ void border_row(const Plane &pl, int row, int lane) {
    if (row >= pl.h + EXT) return;
    uint8_t *dst = pl.p + (ptrdiff_t)row * pl.stride;
    const uint8_t *src = pl.p + (ptrdiff_t)iclamp(row, 0, pl.h - 1) * pl.stride;
    if (row < 0 || row >= pl.h)
        for (int x = lane * 8; x < pl.w; x += 512) *reinterpret_cast<uint2 *>(dst + x) = *reinterpret_cast<const uint2 *>(src + x);
    if (lane < 2) {
        const uint32_t s4 = (uint32_t)src[lane ? pl.w - 1 : 0] * 0x01010101u;
        *reinterpret_cast<uint2 *>(dst + (lane ? pl.w : -EXT)) = make_uint2(s4, s4);
    }
}
__device__ __forceinline__ void border_body(const BorderItem &a) {
    border_row(blockIdx.y == 0 ? a.y : (blockIdx.y == 1 ? a.u : a.v), (int)blockIdx.x - EXT, threadIdx.x);
}

__global__ __launch_bounds__(64) void k_border(BorderItem a) { border_body(a); }

void launch_border(hipStream_t s, const Frame &f) {
    dim3 grid(f.Y[0].h + 2 * EXT, 3);
    VP8_LAUNCH(k_border, grid, dim3(64), 0, s, BorderItem{f.Y[0], f.U, f.V});
}

// ------------------------------------------------------------------------------------------------
// downsample_x2, GPU_kernels.cl:429-451: dst = (a+b+c+d+2)/4 of each 2x2.
// The whole pyramid in one launch (replaces 4 x downsample_x2 per surface, inter_part.h:11-33).
// A workgroup takes a 64x64 tile of the full-resolution plane and produces the 32x32, 16x16, 8x8 and
// 4x4 tiles below it; every level is computed from the ROUNDED level above it, exactly like the
// reference's cascade of launches.  grid = (ceil(W/64), ceil(H/64), surfaces), block = 256.
// ------------------------------------------------------------------------------------------------
// A surface that has just come out of the loop filter also needs its replicated edges before it serves as a reference; the
// pyramid reads the interior only, so the two do not depend on each other and share the launch (bit z of border_mask: the rows
// of workgroups behind the tiles do surface z's edges, a wave per row of a plane) -- one link less in every frame's chain.
struct PyrArgs { Frame f[2 * MAX_BATCH]; uint32_t border_mask; };   // blockIdx.z picks the surface: one or two of a context, or those of a batch
static int border_jobs(const Frame &f) { return (f.Y[0].h + 2 * EXT) + 2 * (f.U.h + 2 * EXT); }

__global__ __launch_bounds__(256) void k_pyramid(PyrArgs a) {
    __shared__ __attribute__((aligned(4))) uint8_t s2[16][16];
    __shared__ __attribute__((aligned(4))) uint8_t s3[8][8];
    const Frame &f = a.f[blockIdx.z];
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    const Plane &P0 = f.Y[0];
    const int tiles_y = (P0.h + 63) / 64;
    // A tile is 64 bytes wide, a line of memory 128: horizontal neighbours share every line they read, and the rows they write in
    // the levels below are 32, 16, 8 and 4 bytes of one line.  Tiles are therefore handed out so that an XCD gets a run of
    // consecutive tiles (xcd_band, vp8hip_dev.h): the two halves of a line meet in ONE L2.
    const int tile = xcd_band((int)blockIdx.y * (int)gridDim.x + (int)blockIdx.x, tiles_y * (int)gridDim.x);
    const int bx = tile % (int)gridDim.x, by = tile / (int)gridDim.x;
    if ((int)blockIdx.y >= tiles_y) {
        if (!((a.border_mask >> blockIdx.z) & 1)) return;
        int job = (((int)blockIdx.y - tiles_y) * (int)gridDim.x + (int)blockIdx.x) * 4 + (t >> 6);
        const int ny = P0.h + 2 * EXT, nc = f.U.h + 2 * EXT;
        if (job < ny) border_row(P0, job - EXT, t & 63);
        else if (job < ny + nc) border_row(f.U, job - ny - EXT, t & 63);
        else if (job < ny + 2 * nc) border_row(f.V, job - ny - nc - EXT, t & 63);
        return;
    }
    // 4x4 source pixels -> 2x2 of level 1 -> 1 of level 2.  Every address is a plane pointer (uniform: scalar registers) plus a 32-bit
    // offset (a surface is far below 2^31 bytes), and a 2x2 sum is two v_dot4_u32_u8 on the rows as loaded (a byte mask of ones picks the
    // pair, the rounding 2 rides in as the accumulator) -- per-sample byte extraction and 64-bit row products were most of the 216 vector
    // instructions a thread issued.
    // Frame sizes are multiples of 16 (vp8hip_create), so level l is exactly w >> l by h >> l and the thread's 4x4 source pixels lie in
    // the plane all together or not at all: ONE test covers its two rows of level 1 and its sample of level 2 (and a level-3 / level-4
    // sample lies in its plane exactly when all the samples under it do: what a thread outside the plane computes is never stored).
    static_assert(PAD >= 4, "a clamped row is read from its first byte");
    const int x0 = bx * 64 + 4 * tx, sy0 = by * 64 + 4 * ty;
    const bool in = x0 < P0.w && sy0 < P0.h;
    const uint32_t last = (uint32_t)((P0.h - 1) * P0.stride + (P0.w - 4));               // (uniform)
    // (rows and strides are below 2^24 and their products below 2^31: v_mad_u32_u24, where the 32-bit product is a 64-bit multiply-add)
    const uint32_t o0 = __umul24((uint32_t)imin(sy0, P0.h - 1), (uint32_t)P0.stride) + (uint32_t)imin(x0, P0.w - 4);   // <= last
    uint32_t lim = in ? 0xffffffffu : last;   // rows below the plane end at its last dword; they are only met by threads that store nothing
    asm("" : "+v"(lim));                      // (one select, not one per row)
    uint32_t r[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t o = o0 + (uint32_t)(k * P0.stride);
        r[k] = *reinterpret_cast<const uint32_t *>(P0.p + (size_t)(k == 0 ? o : __builtin_elementwise_min(o, lim)));
    }
    uint32_t l1[2][2];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const uint32_t pick = i == 0 ? 0x00000101u : 0x01010000u;
            l1[j][i] = __builtin_amdgcn_udot4(r[2 * j], pick, __builtin_amdgcn_udot4(r[2 * j + 1], pick, 2u, false), false) >> 2;
        }
    const uint32_t l2 = (l1[0][0] + l1[0][1] + l1[1][0] + l1[1][1] + 2) >> 2;
    if (in) {
        const Plane &P1 = f.Y[1];
        const uint32_t o1 = __umul24((uint32_t)(by * 32 + 2 * ty), (uint32_t)P1.stride) + (uint32_t)(bx * 32 + 2 * tx);
#pragma unroll
        for (int j = 0; j < 2; ++j)
            *reinterpret_cast<uint16_t *>(P1.p + (size_t)(o1 + (uint32_t)(j * P1.stride))) = (uint16_t)(l1[j][0] | (l1[j][1] << 8));
        const Plane &P2 = f.Y[2];
        P2.p[(size_t)(__umul24((uint32_t)(by * 16 + ty), (uint32_t)P2.stride) + (uint32_t)(bx * 16 + tx))] = (uint8_t)l2;
    }
    s2[ty][tx] = (uint8_t)l2;
    __syncthreads();
    if (t < 64) {     // (a 2x2 of bytes in LDS: two 16-bit reads, summed by v_sad_u8 against zero)
        const int ux = t & 7, uy = t >> 3;
        const uint32_t a0 = *reinterpret_cast<const uint16_t *>(&s2[2 * uy][2 * ux]), a1 = *reinterpret_cast<const uint16_t *>(&s2[2 * uy + 1][2 * ux]);
        const uint32_t l3 = __builtin_amdgcn_sad_u8(a0, 0u, __builtin_amdgcn_sad_u8(a1, 0u, 2u)) >> 2;
        const Plane &P3 = f.Y[3];
        const int x3 = bx * 8 + ux, y3 = by * 8 + uy;
        if (x3 < P3.w && y3 < P3.h) P3.p[(size_t)(__umul24((uint32_t)y3, (uint32_t)P3.stride) + (uint32_t)x3)] = (uint8_t)l3;
        s3[uy][ux] = (uint8_t)l3;
    }
    __syncthreads();
    if (t < 16) {
        const int ux = t & 3, uy = t >> 2;
        const uint32_t a0 = *reinterpret_cast<const uint16_t *>(&s3[2 * uy][2 * ux]), a1 = *reinterpret_cast<const uint16_t *>(&s3[2 * uy + 1][2 * ux]);
        const uint32_t l4 = __builtin_amdgcn_sad_u8(a0, 0u, __builtin_amdgcn_sad_u8(a1, 0u, 2u)) >> 2;
        const Plane &P4 = f.Y[4];
        const int x4 = bx * 4 + ux, y4 = by * 4 + uy;
        if (x4 < P4.w && y4 < P4.h) P4.p[(size_t)(__umul24((uint32_t)y4, (uint32_t)P4.stride) + (uint32_t)x4)] = (uint8_t)l4;
    }
}

static dim3 pyramid_grid(const Frame &f, int nframes, uint32_t border_mask) {
    const int gx = (f.Y[0].w + 63) / 64, gy = (f.Y[0].h + 63) / 64;
    const int extra = border_mask ? ((border_jobs(f) + 3) / 4 + gx - 1) / gx : 0;
    return dim3(gx, gy + extra, nframes);
}
void launch_pyramid(hipStream_t s, const Frame *a, const Frame *b, uint32_t border_mask) {
    PyrArgs p;
    p.f[0] = *a;
    p.f[1] = b ? *b : *a;
    p.border_mask = border_mask;
    VP8_LAUNCH(k_pyramid, pyramid_grid(*a, b ? 2 : 1, border_mask), dim3(256), 0, s, p);
}
void launch_pyramid_batch(hipStream_t s, const Frame *const *f, int nframes, uint32_t border_mask) {
    if (nframes <= 0) return;
    PyrArgs p;
    for (int i = 0; i < nframes; ++i) p.f[i] = *f[i];
    p.border_mask = border_mask;
    VP8_LAUNCH(k_pyramid, pyramid_grid(*f[0], nframes, border_mask), dim3(256), 0, s, p);
}

// ------------------------------------------------------------------------------------------------
// Tight HBM-resident Y,U,V planes -> the padded surfaces of a frame, one launch.  A workgroup owns a run of rows of ONE plane, a
// wave takes every fourth of them and a lane 16 bytes of a row: which plane and which row are scalar values, and an address is a
// scalar row base plus the lane's 32-bit byte offset.  (A thread used to copy `per` units of 8 bytes that it found by dividing a flat
// unit index by the row's unit count and by a three-way plane select per unit: 41 vector instructions per 8 bytes.)
// A workgroup copies about per x 2 KB, as it always did: with one unit per thread a 1080p frame was 1530 workgroups of next to no
// work, and under load it is the dispatch of workgroups, not the copying, that such a launch waits for (same box, headline with 1 / 8 /
// 16 / 32 units per thread: 62.0 / 62.4 / 62.5 / 62.5 M MB/s).
// ------------------------------------------------------------------------------------------------
// The source may be smaller than the coded ("wrk") size -- 1920x1080 in, 1920x1088 coded: copy_with_padding, encIO.h:141-196,
// happens here.  Rows below the source repeat its last row, samples to its right repeat the row's last sample (what the
// reference does for Y and U and means for V: its V lines read and write U, :180-183, so V's right padding is never
// written -- which bites only when the width is not a multiple of 16, none of BASELINE's configs; there this is the
// intended result, not the reference's undefined one; tests/test_padding.py shows both).  sw, sh: luma size of the source; ssy, ssc: its row strides.
struct PackItem { Plane py, pu, pv; const uint8_t *sy, *su, *sv; int sw, sh, ssy, ssc; };
// rows_y: luma rows per workgroup (a chroma workgroup takes twice as many, the same bytes); wg_y, wg_c: workgroups per luma / chroma plane
struct PackGrid { int rows_y, wg_y, wg_c; };
__device__ __forceinline__ void pack_body(const PackItem &a, const PackGrid &g) {
    int wg = (int)blockIdx.x;
    const int pi = wg < g.wg_y ? 0 : (wg < g.wg_y + g.wg_c ? 1 : 2);
    wg -= pi == 0 ? 0 : (pi == 1 ? g.wg_y : g.wg_y + g.wg_c);
    // (member by member: a pointer into the argument block picked by an index sends the block to scratch memory)
    uint8_t *const dp = pi == 0 ? a.py.p : (pi == 1 ? a.pu.p : a.pv.p);
    const uint8_t *const src = pi == 0 ? a.sy : (pi == 1 ? a.su : a.sv);
    const int dstride = pi == 0 ? a.py.stride : a.pu.stride, dw = pi == 0 ? a.py.w : a.pu.w, dh = pi == 0 ? a.py.h : a.pu.h;
    const int sw = pi == 0 ? a.sw : a.sw >> 1, sh = pi == 0 ? a.sh : a.sh >> 1, ss = pi == 0 ? a.ssy : a.ssc;
    const int rows = pi == 0 ? g.rows_y : 2 * g.rows_y;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = (int)(threadIdx.x & 63);
    const int y_end = imin((wg + 1) * rows, dh);
    const bool aligned = ((ss | (int)(reinterpret_cast<uintptr_t>(src) & 7)) & 7) == 0;   // the source rows are 8-byte aligned
    for (int y = wg * rows + wave; y < y_end; y += 4) {
        const uint8_t *row = src + (size_t)(y < sh ? y : sh - 1) * ss;
        uint8_t *drow = dp + (ptrdiff_t)y * dstride;
        for (int x = lane * 16; x + 16 <= dw; x += 1024) {
            uint4 v;
            if (x + 16 <= sw && aligned) {
                const uint2 v0 = *reinterpret_cast<const uint2 *>(row + (uint32_t)x), v1 = *reinterpret_cast<const uint2 *>(row + (uint32_t)x + 8);
                v = make_uint4(v0.x, v0.y, v1.x, v1.y);
            } else {      // the lane's bytes hang over the source's right edge, or the source rows are not 8-byte aligned
                uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
                for (int j = 0; j < 16; ++j) w[j >> 2] |= (uint32_t)row[x + j < sw ? x + j : sw - 1] << (8 * (j & 3));
                v = make_uint4(w[0], w[1], w[2], w[3]);
            }
            *reinterpret_cast<uint4 *>(drow + (uint32_t)x) = v;
        }
        // plane widths are multiples of 8 (and rows start 32-byte aligned): a row may end in one 8-byte unit, which one lane copies
        if ((dw & 8) && lane == ((dw >> 4) & 63)) {
            const int x = dw & ~15;
            uint2 v;
            if (x + 8 <= sw && aligned) {
                v = *reinterpret_cast<const uint2 *>(row + (uint32_t)x);
            } else {
                uint32_t w[2] = {0, 0};
#pragma unroll
                for (int j = 0; j < 8; ++j) w[j >> 2] |= (uint32_t)row[x + j < sw ? x + j : sw - 1] << (8 * (j & 3));
                v = make_uint2(w[0], w[1]);
            }
            *reinterpret_cast<uint2 *>(drow + (uint32_t)x) = v;
        }
    }
}

__global__ __launch_bounds__(256) void k_pack_b(BatchOf<PackItem> b, PackGrid g) { pack_body(b.item[blockIdx.z], g); }
static int pack_units_per_thread() {
    static const int per = [] { const char *e = getenv("VP8HIP_PACK_UNITS"); const int v = e ? atoi(e) : 16; return v < 1 ? 1 : (v > 64 ? 64 : v); }();
    return per;
}

static PackItem pack_item(const Frame &f, const void *y, const void *u, const void *v, int sw, int sh, int ssy, int ssc) {
    if (sw <= 0) { sw = f.Y[0].w; sh = f.Y[0].h; }
    if (ssy <= 0) { ssy = sw; ssc = sw >> 1; }
    return PackItem{f.Y[0], f.U, f.V, (const uint8_t *)y, (const uint8_t *)u, (const uint8_t *)v, sw, sh, ssy, ssc};
}
// (one context launches a batch of one: the by-value form of the kernel picks the plane through a pointer into its argument block,
// which hipcc answers by copying the block to scratch memory)
void launch_pack_batch(hipStream_t s, const SourceItem *items, int n, int sw, int sh, int ssy, int ssc) {
    BatchOf<PackItem> b;
    b.n = n;
    for (int i = 0; i < n; ++i) b.item[i] = pack_item(*items[i].f, items[i].y, items[i].u, items[i].v, sw, sh, ssy, ssc);
    const Frame &f = *items[0].f;
    PackGrid g;
    g.rows_y = pack_units_per_thread() * 2048 / f.Y[0].w;      // rows of about `per` x 2 KB
    if (g.rows_y < 1) g.rows_y = 1;
    g.wg_y = (f.Y[0].h + g.rows_y - 1) / g.rows_y;
    g.wg_c = (f.U.h + 2 * g.rows_y - 1) / (2 * g.rows_y);
    VP8_LAUNCH(k_pack_b, dim3(g.wg_y + 2 * g.wg_c, 1, n), dim3(256), 0, s, b, g);
}

// ------------------------------------------------------------------------------------------------
// luma_search_1step, GPU_kernels.cl:459-560.  One 8x8 block of one pyramid level per 32 lanes,
// lane = candidate dxy (25 of 32 used).  Cost = sum of 4 weight4x4 (ushort, wraps) + MV penalty;
// out-of-frame candidates can never win (Diff|0x7fff >= initial MinDiff) and are skipped; the
// sequential "first strict minimum" is min over (cost<<8 | dxy).
// grid = (ceil(nblk/8), enabled refs), block = 256.
// ------------------------------------------------------------------------------------------------
struct Search1Args {
    Plane cur;
    Plane ref[3];
    const int16_t *src[3];
    int16_t *dst[3];
    int refmap[3];
    int nrefs;      // enabled references of this context (a batched launch is sized for the largest of its contexts)
    int net_width, w, h, pixel_rate, rate_shift, nblk, bw;
    int pbw, pbh;   // block grid of the coarser level (whose cells of src[] were written this frame)
    uint32_t bw_inv;   // ceil(2^32 / bw)
};

// Two mappings of the same work:
//   SPLIT = false: five lanes per 8x8 block, lane j = candidate row dy = j-2, a loop over the four 4x4 sub-blocks;
//                  12 blocks per wave.  Fewest instructions (the per-block preamble is paid once): the throughput form.
//   SPLIT = true:  twenty lanes per block = (sub-block sb) x (dy); the four sub-block costs of a candidate meet in two
//                  shuffles; 3 blocks per wave.  The same arithmetic in four times as many waves, each a quarter as long
//                  (the preamble is paid per sub-block: +29 % instructions): the latency form.  On the coarse levels,
//                  which have a few hundred blocks, a launch lasts as long as ONE wave: 12 us per level with the loop,
//                  5-6 us split (single video, frame after frame: 73 -> 45 us of a 540 us frame for the five levels).
// In either, a lane loads the 8-byte reference rows of a sub-block at its dy once and walks the five dx candidates over
// them in registers (the window bytes are shared by the five candidates of a row).
template <bool SPLIT>
struct S1Map {
    static constexpr int LANES_PER_BLOCK = SPLIT ? 20 : 5;
    static constexpr int BLOCKS_PER_WAVE = SPLIT ? 3 : 12;
    static constexpr int BLOCKS_PER_WG = 4 * BLOCKS_PER_WAVE;
};

// cost of the five dx candidates of one 4x4 sub-block (sx, sy) for this lane's dy row, added to acc[]
__device__ __forceinline__ void s1_subblock(const uint8_t *cp, int cstride, const uint8_t *rp, int rstride, int acc[5]) {
    uint32_t c[4], q0[4], q1[4];
#pragma unroll
    for (int y = 0; y < 4; ++y) {
        c[y] = *reinterpret_cast<const uint32_t *>(cp + (ptrdiff_t)y * cstride) ^ 0x80808080u;
        const uint2 q = ld_u64(rp + (ptrdiff_t)y * rstride);
        q0[y] = q.x ^ 0x80808080u; q1[y] = q.y ^ 0x80808080u;
    }
    // rows -> columns (byte r = row r), pixels biased: the form weight_cols_pre wants.  Candidate dx = i reads
    // columns i..i+3 of the eight: no byte alignment per candidate, and the current block's share of the metric
    // (16 dot4) is computed once for the five of them.
    uint32_t cc[4], col[8];
    transpose4x4(c, cc);
    transpose4x4(q0, col);
    transpose4x4(q1, col + 4);
    int pre[16];
#pragma unroll
    for (int k = 0; k < 4; ++k) weight_pre_column(cc[k], pre + 4 * k);
#pragma unroll
    for (int i = 0; i < 5; ++i) acc[i] += weight_cols_pre(pre, col + i);
}

// The same with the current block's share of the metric taken from LDS (pre_lds[pre_off ..]: the 16 ints weight_pre_block of this sub-block,
// made once per wave by s1_make_pre below): the five dy lanes of a block -- and every reference -- need the same 16 dot4, 12 adds, 8 permutes and 4 biases
// per sub-block; as instructions of the wave they cost what they cost one lane.  The column pass of a candidate is one MFMA for the whole wave
// (weight_mfma, vp8hip_dev.h; every lane of the wave runs this), B = its four columns, C = the current block's share, read again from LDS for each
// candidate: held in registers next to the 16 results it would cost 16 registers, and the loop form is tuned for eight waves per SIMD.  The
// address passes through an empty asm per candidate so that the compiler cannot see the five reads are the same and keep one copy (it did, and
// then copied 16 registers into the accumulator before every MFMA); hiding the pointer instead makes the reads flat loads.  What passes is the
// lane's BYTE address in the table (pre_addr: s1_pre_c_bytes / s1_fill_c_bytes), in the ONE register that carries it through the sub-block loop:
// each asm hands on what the one before it left and the caller steps it from sub-block to sub-block, so the four ds_read_b128 of a candidate take
// the register as it stands, the quad in their offset field -- no copy and no shift per candidate (an int index hidden afresh from a value kept
// beside it cost a v_mov_b32 and a v_lshlrev_b32 for each of the five).  The B operand of
// a candidate is made right before its MFMA, behind a scheduling barrier: left to itself hipcc built all five quads up front and spilled at 64.
// History: the operand used to be in column order (K_METRIC_A), which cost two 4x4 byte transposes of the window (16 v_perm) and, an MFMA
// operand being an even-aligned register quad, eight v_mov for candidates 1 and 3.  With the A table in row order (wa = metric_a_rows,
// vp8hip_dev.h) candidate dx = i is bytes i..i+3 of the four rows: the low dwords as loaded (i = 0), the high dwords (i = 4), and one
// v_alignbyte per row, written straight into an aligned quad, for the three between -- 12 instructions where 24 stood.
__device__ __forceinline__ void s1_subblock_pre(v4i wa, const int *pre_lds, int &pre_addr, const uint8_t *rp, int rstride, int acc[5]) {
    uint32_t q0[4], q1[4];      // bytes 0..3 and 4..7 of the window's four rows, pixels biased
#pragma unroll
    for (int y = 0; y < 4; ++y) {
        q0[y] = ld_u32(rp + (ptrdiff_t)y * rstride) ^ 0x80808080u;
        q1[y] = ld_u32(rp + (ptrdiff_t)y * rstride + 4) ^ 0x80808080u;
    }
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        asm volatile("" : "+v"(pre_addr));
        __builtin_amdgcn_sched_barrier(0);
        v4i b;
#pragma unroll
        for (int y = 0; y < 4; ++y) b[y] = i == 0 ? (int)q0[y] : i == 4 ? (int)q1[y] : (int)__builtin_amdgcn_alignbyte(q1[y], q0[y], (uint32_t)i);
        acc[i] += weight_mfma(wa, load_pre16(reinterpret_cast<const int *>(reinterpret_cast<const char *>(pre_lds) + pre_addr)), b);
    }
}
// ... made by the wave for its twelve blocks: lane = (block slot, sub-block), 48 of the 64 lanes; 16 ints each into pre_lds[slot][sub-block][16].
// A block slot is S1_PRE_SLOT = 68 ints apart from the next, not 64 (s1_pre_layout.h): in a C read the lanes of a wave differ only in their block slot,
// and slots a whole bank row apart put the five or six blocks of a lane group of the ds_read_b128 on the same four banks.  Checked here with the
// address the kernels index by: every C read of the table costs the LDS the four cycles of a conflict-free read.
static_assert(s1_pre_c_read_worst() == 4 && s1_pre_c_read_best() == 4, "the C reads of the whole-pel search's pre table must be free of LDS bank conflicts");
static_assert(S1_PRE_BLOCKS == S1Map<false>::BLOCKS_PER_WAVE, "s1_pre_layout.h and the loop form's lane map disagree");
__device__ __forceinline__ void s1_make_pre(const Plane &cur, int cx, int cy, int sb, bool on, int *dst16) {
    const int sx = (sb >> 1) * 4, sy = (sb & 1) * 4;      // the order of the cost loop: (0,0), (0,+4 rows), (+4 cols,0), (+4,+4)
    const uint8_t *cp = cur.p + (ptrdiff_t)(cy + sy) * cur.stride + cx + sx;
    uint32_t c[4], cc[4];
#pragma unroll
    for (int y = 0; y < 4; ++y) c[y] = *reinterpret_cast<const uint32_t *>(cp + (ptrdiff_t)y * cur.stride) ^ 0x80808080u;
    transpose4x4(c, cc);
    int pre[16];
    weight_pre_block(cc, pre);
    if (on) {
#pragma unroll
        for (int k = 0; k < 4; ++k) *reinterpret_cast<int4 *>(dst16 + 4 * k) = make_int4(pre[4 * k], pre[4 * k + 1], pre[4 * k + 2], pre[4 * k + 3]);
    }
}

// One 8x8 block of one level against one reference: the lanes of the block (M::LANES_PER_BLOCK of them: `sub` is the lane's number in
// the block, `lane` its number in the wave) search the 25 candidates around the scaled parent vector `pv` (packed short2, 0 = none).
// Returns the block's vector as the net holds it (packed short2, already multiplied by pixel_rate); valid in the lane with sub == 0.
// `live` false: the lanes take part in the shuffles on harmless in-frame data.
// LDS_MIN (the filled loop form, where a block's five lanes may lie in two waves): the minimum over the block's lanes goes through min_lds, one word per
// lane of the workgroup, this lane's at min_lds[sub] -- one store, a barrier, five reads (so EVERY lane of the workgroup must come here), four v_min_u32
// where the shuffle tree is three steps of six instructions.  The caller keeps the next call from overwriting words still being read.
template <bool SPLIT, bool LDS_MIN = false>
__device__ __forceinline__ uint32_t search1_block(const Search1Args &a, int r, int cx, int cy, uint32_t pv, bool live, int sub, int lane,
                                                  const int *pre_lds = nullptr /* loop form: the workgroup's table from s1_make_pre */,
                                                  int pre_off = 0 /* ... and where this block's [sub-block][16] start in it, in BYTES */,
                                                  uint32_t *min_lds = nullptr /* LDS_MIN: the word of this block's first lane */) {
    const int sb0 = sub / 5, j = sub - 5 * sb0;       // SPLIT: this lane's sub-block; otherwise sb0 = 0
    // vector / pixel_rate truncates toward zero (:495-500)
    int v0x = (int16_t)(pv & 0xffffu), v0y = (int16_t)(pv >> 16);
    const int rmask = a.pixel_rate - 1;
    v0x = (v0x + ((v0x >> 31) & rmask)) >> a.rate_shift;
    v0y = (v0y + ((v0y >> 31) & rmask)) >> a.rate_shift;
    if (a.pixel_rate > 8) v0x = v0y = 0;

    const int py = (int16_t)(cy + v0y + (j - 2));
    const bool row_valid = live && py >= 0 && py <= a.h - 8;
    const int xb = cx + v0x - 2;                       // x of candidate dx = -2
    // rows that cannot hold a valid candidate are read at a harmless in-frame position
    const bool loadable = row_valid && xb >= -8 && xb <= a.w - 4;
    const int lx = loadable ? xb : cx, ly = loadable ? py : cy;

    const uint8_t *cp = a.cur.p + (ptrdiff_t)cy * a.cur.stride + cx;
    const uint8_t *rp = a.ref[r].p + (ptrdiff_t)ly * a.ref[r].stride + lx;
    int acc[5] = {0, 0, 0, 0, 0};
    if (SPLIT) {
        const int sx = (sb0 >> 1) * 4, sy = (sb0 & 1) * 4;   // sub-block order (0,0),(0,+4 rows),(+4 cols,0),(+4,+4), :456-458
        s1_subblock(cp + (ptrdiff_t)sy * a.cur.stride + sx, a.cur.stride, rp + (ptrdiff_t)sy * a.ref[r].stride + sx, a.ref[r].stride, acc);
#pragma unroll
        for (int i = 0; i < 5; ++i) {   // lanes sub, sub+5, sub+10, sub+15 of the block: the sums land on sb0 = 0
            acc[i] += __shfl(acc[i], lane + 10, 64);
            acc[i] += __shfl(acc[i], lane + 5, 64);
        }
    } else {
        // one sub-block at a time (loop NOT unrolled: the register footprint decides how many waves a SIMD holds)
        const v4i wa = metric_a_rows(lane);
        int pre_addr = pre_off;     // sub-block 0 of this lane's block; stepped by the loop, in the register the reads take it from
#pragma unroll 1
        for (int sb = 0; sb < 4; ++sb) {
            const int sx = (sb >> 1) * 4, sy = (sb & 1) * 4;
            s1_subblock_pre(wa, pre_lds, pre_addr, rp + (ptrdiff_t)sy * a.ref[r].stride + sx, a.ref[r].stride, acc);
            pre_addr += s1_pre_sub_bytes(1);
        }
    }
    const int pen_mask = a.pixel_rate < 4 ? -1 : 0;     // x 32 on the two finest levels, x 0 above (a shift and a mask: `* pen_scale' with a scale the compiler cannot see compiles to a 64-bit multiply-add per candidate)
    const int pen_y = iabs(iabs(py - cy) - v0y);
    // The five candidates' keys, two candidates to a register (candidates (0, 1), (2, 3) and 4).  The ranges that make 16 bits enough:
    //   * A candidate that is valid has not wrapped: px = cx + v0x - 2 + i lies in [0, w - 8], so px - cx = v0x + i - 2 as integers, and with
    //     cx, px < 8192 (a frame is at most 8192 wide) |px - cx| < 8192 and |v0x| < 8194: v0x + (i - 2), its negation, |px - cx| - v0x (within
    //     +-16386) and the absolute value of that all fit int16 -- v_pk_add_u16, v_pk_sub_i16, v_pk_max_i16 give what the 32-bit forms gave.
    //     pen_y is the same quantity along y for the lane's row, made in 32 bits as before: at most 16386 for a valid row.
    //   * The accumulator is a ushort by definition (& 0xffff), the penalty is added into it modulo 2^16, and x 32 modulo 2^16 is what (<< 5) &
    //     0xffff was: (penalty x scale + acc) in one v_pk_mad_u16, scale = 32 on the two finest levels and 0 above (what pen_mask did).
    //   * An invalid candidate's diff is never looked at, so what its lanes of the arithmetic hold (wrapped, anything) does not matter: its
    //     half gets 0x8000 added behind the clamp to 0x7fff -- its column tested as (uint16)px > w - 8, which is px < 0 || px > w - 8 for the
    //     wrapped 16-bit px = (int16)(xb + i) since w - 8 < 32768 -- and a row that cannot hold a valid candidate loses its whole lane (loadable).
    //   * diff < 0x7fff becomes a clamp: min(diff, 0x7fff), and every key from 0x7fff00 up means "not accepted".  Such keys lose against every
    //     accepted one in the minimum (over the candidates, then over the block's lanes), and when the minimum itself is one of them nothing was
    //     accepted: the test behind the minimum is best < 0x7fff00 where it was best != 0xffffffff.  The same integer wins as before.
    // Only the key (diff << 8 | j * 5 + i: one v_perm_b32 from the pair and a register of the lane's five numbers) and the minimum take 32 bits.
    uint32_t best = 0xffffffffu;
    {
        const u16x2 v0xp = {(unsigned short)v0x, (unsigned short)v0x}, cxp = {(unsigned short)cx, (unsigned short)cx};
        const u16x2 penyp = {(unsigned short)pen_y, (unsigned short)pen_y}, wlim = {(unsigned short)(a.w - 8), (unsigned short)(a.w - 8)};
        const unsigned short sc = (unsigned short)(32 & pen_mask);
        const u16x2 scale = {sc, sc};
        const uint32_t codes03 = (uint32_t)(j * 5) * 0x01010101u + 0x03020100u, code4 = (uint32_t)(j * 5 + 4);
#pragma unroll
        for (int p = 0; p < 3; ++p) {
            const int i0 = 2 * p;
            const s16x2 off = {(short)(i0 - 2), (short)(i0 - 1)};
            const s16x2 rel = __builtin_bit_cast(s16x2, v0xp) + off;
            const s16x2 nrel = -rel, arel = __builtin_elementwise_max(rel, nrel);
            const s16x2 dd = arel - __builtin_bit_cast(s16x2, v0xp), ndd = -dd, e = __builtin_elementwise_max(dd, ndd);
            const u16x2 accp = __builtin_bit_cast(u16x2, pk16(acc[i0], p < 2 ? acc[i0 + 1] : 0));
            u16x2 diff = __builtin_elementwise_min((u16x2)((__builtin_bit_cast(u16x2, e) + penyp) * scale + accp), (u16x2){0x7fff, 0x7fff});
            const u16x2 pxu = cxp + __builtin_bit_cast(u16x2, rel);
            // px - (w - 8) saturating at 0, at most 1, times 0x8000, added: a half whose column is out of the frame comes out >= 0x8000, the
            // others unchanged.  (Inline: written in C the compiler turns the three packed instructions into two compares, two selects, a
            // permute and an or per pair.  Plain vector instructions on plain vector results: no hazard the compiler would have to see.)
            uint32_t d = __builtin_bit_cast(uint32_t, diff), over;
            asm("v_pk_sub_u16 %1, %2, %3 clamp\n\tv_pk_min_u16 %1, %1, 1 op_sel_hi:[1,0]\n\tv_pk_mad_u16 %0, %1, %4, %0"
                : "+v"(d), "=&v"(over) : "v"(__builtin_bit_cast(uint32_t, pxu)), "v"(__builtin_bit_cast(uint32_t, wlim)), "s"(0x80008000u));
            const uint32_t k0 = __builtin_amdgcn_perm(d, p < 2 ? codes03 : code4, p == 1 ? 0x0c050402u : 0x0c050400u);
            best = k0 < best ? k0 : best;
            if (p < 2) {
                const uint32_t k1 = __builtin_amdgcn_perm(d, codes03, p == 1 ? 0x0c070603u : 0x0c070601u);
                best = k1 < best ? k1 : best;
            }
        }
        best = loadable ? best : 0xffffffffu;
    }
    // minimum over the five dy lanes of the block (its sb = 0 lanes hold the full sums): (cost << 8 | dxy) = the
    // reference's first strict minimum
    if (LDS_MIN) {      // (the keys of a block differ in their low byte: the minimum is the same integer whatever the order)
        min_lds[sub] = best;
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const uint32_t o = min_lds[k];
            best = o < best ? o : best;
        }
    } else {
#pragma unroll
        for (int off = 1; off <= 4; off <<= 1) {
            const uint32_t o = (uint32_t)__shfl((int)best, lane + off, 64);
            if (j + off < 5 && o < best) best = o;
        }
    }
    int bx, by;  // best position minus block position
    if (best < (0x7fffu << 8)) {
        const int k = best & 0xff;      // (an accepted key: see the ranges above)
        bx = v0x + (k % 5 - 2);
        by = v0y + (k / 5 - 2);
    } else {  // nothing accepted: "vector" still holds the scaled parent, :501,:551-556
        bx = (int16_t)(v0x - cx);
        by = (int16_t)(v0y - cy);
    }
    const uint32_t ox16 = (uint16_t)(int16_t)((int16_t)bx * (int16_t)a.pixel_rate);
    const uint32_t oy16 = (uint16_t)(int16_t)((int16_t)by * (int16_t)a.pixel_rate);
    return ox16 | (oy16 << 16);
}

// The loop form (SPLIT = false) keeps the current blocks' share of the metric in LDS, made once per wave (s1_make_pre), not by every lane of a block.
// REF_LOOP: a workgroup searches its blocks in EVERY enabled reference, one after the other (grid y = 1), instead of a workgroup per reference:
// the block arithmetic and the current blocks' share of the metric are made once for the two or three of them (batches; one video keeps a
// workgroup per reference: there a launch is as long as one wave)
// FILL (the loop form with REF_LOOP: k_search1_plr_b): blocks numbered across the workgroup, 51 of them in its 256 lanes instead of 4 x 12
// (s1_fill_layout.h): the table is made by the whole workgroup behind one barrier, and the minimum over a block's lanes, three of which blocks lie in
// two waves, goes through LDS (search1_block, LDS_MIN).  Every lane of the workgroup runs every MFMA and meets every barrier: nrefs is the workgroup's.
static_assert(s1_fill_c_read_worst() == 4 && s1_fill_c_read_best() == 4, "the C reads of the filled loop form's pre table must be free of LDS bank conflicts: all four waves, every sub-block and quad");
static_assert(s1_fill_c_read_worst(64) > 4, "the bank model sees the conflicts of unskewed slots");
template <bool SPLIT, bool REF_LOOP = false, bool FILL = false>
__device__ __forceinline__ void search1_body(const Search1Args &a) {
    using M = S1Map<SPLIT>;
    static_assert(!FILL || (!SPLIT && REF_LOOP), "the filled map is the loop form's, with the reference loop");
    if (!REF_LOOP && (int)blockIdx.y >= a.nrefs) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int grp = FILL ? s1_fill_slot_of((int)threadIdx.x) : lane / M::LANES_PER_BLOCK;
    const int sub = FILL ? (int)threadIdx.x - S1_FILL_LANES * grp : lane - M::LANES_PER_BLOCK * grp;
    // (FILL: the block of (workgroup, slot) as s1_fill_layout.h states it, < 0 where the slot has none -- lane 255 and the last workgroup's spare slots)
    const int b_raw = FILL ? s1_fill_block_of(xcd_band(blockIdx.x, gridDim.x), grp, a.nblk) : (xcd_band(blockIdx.x, gridDim.x) * 4 + wave) * M::BLOCKS_PER_WAVE + grp;
    const bool live = FILL ? b_raw >= 0 : grp < M::BLOCKS_PER_WAVE && b_raw < a.nblk;
    const int b = live ? b_raw : a.nblk - 1;
    const int by = a.bw == 1 ? b : (int)__umulhi((uint32_t)b, a.bw_inv), bx = b - by * a.bw;   // b / bw: bw_inv = ceil(2^32 / bw), exact for b * bw < 2^32
    const int cx = bx * 8, cy = by * 8;
    // The reference zeroes the nets every frame (reset_vectors, :404-427) because parent cells beyond the
    // coarser level's block grid are read but never written; reading them as 0 here is the same thing
    // without the extra kernel.
    const int parent = (cy >> 4) * a.net_width + (cx >> 4);
    const bool parent_written = (cx >> 4) < a.pbw && (cy >> 4) < a.pbh;
    const int *pre_lds = nullptr;
    int pre_off = 0;
    uint32_t *min_lds = nullptr;
    if (FILL) {
        // lane t = (block slot, sub-block) of the 204 tasks; the slots are read by other waves than made them: one barrier
        __shared__ __attribute__((aligned(16))) int s_fill[S1_FILL_INTS];
        __shared__ uint32_t s_min[2][S1_FILL_MIN_WORDS];
        const int t = threadIdx.x, slot = s1_fill_task_slot(t), sb = s1_fill_task_sub(t);
        const int tb_raw = xcd_band(blockIdx.x, gridDim.x) * S1_FILL_BLOCKS + slot;
        const int tb = tb_raw < a.nblk ? tb_raw : a.nblk - 1;
        const int tby = a.bw == 1 ? tb : (int)__umulhi((uint32_t)tb, a.bw_inv), tbx = tb - tby * a.bw;
        s1_make_pre(a.cur, tbx * 8, tby * 8, sb, slot < S1_FILL_BLOCKS, s_fill + s1_fill_slot_at(slot) + s1_pre_sub_at(sb));
        __syncthreads();
        pre_lds = s_fill;
        pre_off = s1_fill_c_bytes(t, 0, 0);
        // (lane 255 has no block: never live, it searches the frame's last block with slot 50's C input, and of the five words of the minimum it
        // reads, 256..259 are never written -- uninitialised on purpose, its result is never used)
        min_lds = &s_min[0][s1_fill_min_at(t)];
    } else if (!SPLIT) {
        // the current blocks' share of the metric, once per wave into LDS: lane = (block slot, sub-block).  The stages hand over inside the wave
        // (LDS executes a wave's operations in order): no barrier, the compiler is kept from moving the reads up
        __shared__ __attribute__((aligned(16))) int s_pre[4][S1_PRE_INTS];
        const int slot = lane >> 2, sb = lane & 3;
        const int tb_raw = (xcd_band(blockIdx.x, gridDim.x) * 4 + wave) * M::BLOCKS_PER_WAVE + slot;
        const int tb = tb_raw < a.nblk ? tb_raw : a.nblk - 1;
        const int tby = a.bw == 1 ? tb : (int)__umulhi((uint32_t)tb, a.bw_inv), tbx = tb - tby * a.bw;
        s1_make_pre(a.cur, tbx * 8, tby * 8, sb, slot < M::BLOCKS_PER_WAVE, &s_pre[0][0] + s1_pre_slot_at(wave, slot) + s1_pre_sub_at(sb));
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        pre_lds = &s_pre[0][0];
        pre_off = s1_pre_c_bytes(wave, lane, 0, 0);  // this lane's block slot, in bytes; the sub-block (s1_pre_sub_bytes) is stepped by the loop, the quad (load_pre16) sits in the read
    }
    const int nr = REF_LOOP ? a.nrefs : 1;
#pragma unroll 1
    for (int ri = 0; ri < nr; ++ri) {
        const int r = a.refmap[REF_LOOP ? ri : (int)blockIdx.y];
        const uint32_t pv = parent_written ? reinterpret_cast<const uint32_t *>(a.src[r])[parent] : 0u;
        // (FILL: the minimum's words alternate between two buffers: a wave writes reference ri + 2's only behind the barrier of ri + 1, which every wave
        // passes with its reads of ri done)
        const uint32_t out = search1_block<SPLIT, FILL>(a, r, cx, cy, pv, live, sub, lane, pre_lds, pre_off,
                                                             FILL ? min_lds + (ri & 1) * S1_FILL_MIN_WORDS : nullptr);
        if (sub == 0 && live) {
            const int cell = (cy >> 3) * a.net_width + (cx >> 3);
            reinterpret_cast<uint32_t *>(a.dst[r])[cell] = out;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Levels 4, 3, 2 and 1 of one reference's search in ONE launch, for a single video coded frame after frame: there the five levels are
// five links of the frame's dependency chain, each of the coarse four lasting as long as one wave of it plus a launch (4.5 + 4.8 + 5.0 +
// 7.8 us at 1080p: profiles/r05_single_stream_timeline.txt), and nothing else fills the part.  A workgroup takes a tile of 4 x 4 level-1
// blocks and computes the tile's ANCESTORS itself -- the one level-4 block, the one level-3 block and the 2 x 2 level-2 blocks whose
// vectors the tile descends from (the parent of block (bx, by) is block (bx / 2, by / 2) of the level above) -- keeping their vectors in
// LDS: 6 block searches on top of 16, no workgroup waits for another, and the chain has one link where it had four.  The same routine on
// the same inputs (search1_block), so the level-1 net -- the only one the next launch reads -- is the one four launches leave.
// ------------------------------------------------------------------------------------------------
// (Level 0 in the same launch as well was no faster: the finest level is whole-chip work, profiles/README.md.)
struct CoarseArgs { Search1Args lv[5]; };   // lv[l] = level l
constexpr int COARSE_WAVES = 6;             // 18 block slots of 20 lanes: the tile's 16 level-1 blocks in one pass
// the tile's work: L1..L4 = the four levels' arguments, r = the reference's slot in them
__device__ __forceinline__ void coarse_tile(const Search1Args &L1, const Search1Args &L2, const Search1Args &L3, const Search1Args &L4, int r) {
    using M = S1Map<true>;
    __shared__ uint32_t mv4, mv3, mv2[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int grp = lane / M::LANES_PER_BLOCK, sub = lane - M::LANES_PER_BLOCK * grp;
    const int slot = grp < M::BLOCKS_PER_WAVE ? wave * M::BLOCKS_PER_WAVE + grp : 99;     // block slot of this lane in the workgroup, 0..17
    const int tiles_x = (L1.bw + 3) / 4;
    const int tile = xcd_band(blockIdx.x, gridDim.x);
    const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
    // ---- level 4: block (tx / 2, ty / 2) ----
    {
        const int bx = tx >> 1, by = ty >> 1;
        const bool exists = bx < L4.bw && by * L4.bw + bx < L4.nblk;
        if (wave == 0) {     // (whole waves only: the block's lanes shuffle among themselves)
            const bool live = slot == 0 && exists;
            const uint32_t out = search1_block<true>(L4, r, (live ? bx : 0) * 8, (live ? by : 0) * 8, 0u, live, sub, lane);
            if (slot == 0 && sub == 0) mv4 = exists ? out : 0u;      // (a cell beyond the coarser grid reads as zero: reset_vectors, :404-427)
        }
    }
    __syncthreads();
    // ---- level 3: block (tx, ty) ----
    {
        const bool exists = tx < L3.bw && ty * L3.bw + tx < L3.nblk;
        if (wave == 0) {
            const bool live = slot == 0 && exists;
            const uint32_t out = search1_block<true>(L3, r, (live ? tx : 0) * 8, (live ? ty : 0) * 8, mv4, live, sub, lane);
            if (slot == 0 && sub == 0) mv3 = exists ? out : 0u;
        }
    }
    __syncthreads();
    // ---- level 2: blocks (2 tx + i, 2 ty + j) ----
    if (wave < 2) {
        const int i = slot & 1, j = (slot >> 1) & 1;
        const int bx = 2 * tx + i, by = 2 * ty + j;
        const bool exists = slot < 4 && bx < L2.bw && by * L2.bw + bx < L2.nblk;
        const uint32_t out = search1_block<true>(L2, r, (exists ? bx : 0) * 8, (exists ? by : 0) * 8, mv3, exists, sub, lane);
        if (slot < 4 && sub == 0) mv2[slot] = exists ? out : 0u;
    }
    __syncthreads();
    // ---- level 1: the tile's 4 x 4 blocks; the only net that leaves the workgroup ----
    {
        const int i = slot & 3, j = (slot >> 2) & 3;
        const int bx = 4 * tx + i, by = 4 * ty + j;
        const bool live = slot < 16 && bx < L1.bw && by * L1.bw + bx < L1.nblk;
        const uint32_t pv = mv2[(((j >> 1) & 1) << 1) | ((i >> 1) & 1)];
        const uint32_t out = search1_block<true>(L1, r, (live ? bx : 0) * 8, (live ? by : 0) * 8, pv, live, sub, lane);
        if (sub == 0 && live) reinterpret_cast<uint32_t *>(L1.dst[r])[by * L1.net_width + bx] = out;
    }
}

__global__ __launch_bounds__(64 * COARSE_WAVES) void k_search1_coarse(CoarseArgs a) {
    if ((int)blockIdx.y >= a.lv[1].nrefs) return;
    coarse_tile(a.lv[1], a.lv[2], a.lv[3], a.lv[4], a.lv[1].refmap[blockIdx.y]);
}

// The short-wave form, what a small launch takes (search1_split) ...
__global__ __launch_bounds__(256) void k_search1(Search1Args a) { search1_body<true>(a); }
static_assert(sizeof(BatchOf<Search1Args>) <= 4096 && sizeof(PyrArgs) <= 4096 && sizeof(BatchOf<PackItem>) <= 4096, "a batch's argument blocks travel in the 4 KiB kernel-argument segment");
__global__ __launch_bounds__(256) void k_search1_b(BatchOf<Search1Args> b) { search1_body<true>(b.item[blockIdx.z]); }
// ... and the loop form: one video a workgroup per reference, batches the filled map with the reference loop.
// (the loop form's register budgets pinned, eight waves per SIMD and seven: under a bare launch bound hipcc gives the MFMA results of the metric
// AGPRs and pays a v_accvgpr_read per value)
__global__ __attribute__((amdgpu_waves_per_eu(8, 8))) __launch_bounds__(256) void k_search1_pl(Search1Args a) { search1_body<false>(a); }
__global__ __attribute__((amdgpu_waves_per_eu(7, 8))) __launch_bounds__(256) void k_search1_plr_b(BatchOf<Search1Args> b) { search1_body<false, true, true>(b.item[blockIdx.z]); }
// (the filled map pays where the part is full, the headline's regime.  Alone on the part -- a batch of one 1080p member, three references -- a launch is
// as long as one wave and the barrier per reference costs more than the lanes save: 28.4 us a launch where the twelve-slot map took 27.3, -0.8 % of
// that one-chunk rate; profiles/s1_fill_parent_vs_this.txt, section 4.  Not branched on: a launch cannot see what else runs on the part.)

static Search1Args search1_args(const CodingItem &it, int level, int src_idx, int net_width) {
    const Frame &cur = *it.cur;
    const RefSet &refs = it.refs;
    const NetSet &nets = *it.nets;
    Search1Args a;
    a.cur = cur.Y[level];
    int n = 0;
    for (int r = 0; r < 3; ++r) {
        a.ref[r] = refs.ref[r].Y[level];
        a.src[r] = nets.net[r][src_idx];
        a.dst[r] = nets.net[r][src_idx ^ 1];
        if (refs.use[r]) a.refmap[n++] = r;
    }
    a.nrefs = n;
    for (int i = n; i < 3; ++i) a.refmap[i] = 0;
    a.net_width = net_width;
    a.w = a.cur.w;
    a.h = a.cur.h;
    a.pixel_rate = 1 << level;
    a.rate_shift = level;
    a.bw = a.w / 8;
    a.nblk = (a.w / 8) * (a.h / 8);
    a.bw_inv = a.bw > 0 ? (uint32_t)(((1ull << 32) + a.bw - 1) / a.bw) : 0;
    a.pbw = level < 4 ? cur.Y[level + 1].w / 8 : 0;
    a.pbh = level < 4 ? cur.Y[level + 1].h / 8 : 0;
    return a;
}

static bool search1_skip() {
    static const bool skip = experiment_skip("s1");
    return skip;   // timing experiment only
}
// fewer waves than the chip has SIMDs: the launch is as long as one wave whatever else runs -> the short-wave form.
// VP8HIP_S1_SPLIT=0/1 forces one form (the tests' tap: at their shapes every launch is a small one)
static bool search1_split(size_t blocks_times_refs) {
    static const int forced = [] { const char *v = getenv("VP8HIP_S1_SPLIT"); return v && v[0] ? (v[0] == '1' ? 1 : 0) : -1; }();
    return forced >= 0 ? forced == 1 : blocks_times_refs < (size_t)12 * 1024;
}

void launch_search1(hipStream_t s, const CodingItem &it, int level, int src_idx, int net_width) {
    const Search1Args a = search1_args(it, level, src_idx, net_width);
    const int n = a.nrefs;
    if (a.nblk <= 0 || n == 0 || search1_skip()) return;
    if (search1_split((size_t)a.nblk * n))
        VP8_LAUNCH(k_search1, dim3((a.nblk + S1Map<true>::BLOCKS_PER_WG - 1) / S1Map<true>::BLOCKS_PER_WG, n), dim3(256), 0, s, a);
    else
        VP8_LAUNCH(k_search1_pl, dim3((a.nblk + S1Map<false>::BLOCKS_PER_WG - 1) / S1Map<false>::BLOCKS_PER_WG, n), dim3(256), 0, s, a);
}

// levels 4..1 in one launch (k_search1_coarse); the level-1 net lands where launch_search1 leaves it
void launch_search1_coarse(hipStream_t s, const CodingItem &it, int net_width) {
    CoarseArgs a;
    for (int l = 0; l <= 4; ++l) a.lv[l] = search1_args(it, l, l & 1, net_width);   // src of level l: 0 for 4, 2 and 0; 1 for 3 and 1
    const Search1Args &L0 = a.lv[0], &L1 = a.lv[1];
    if (L0.nblk <= 0 || L0.nrefs == 0 || search1_skip()) return;
    // tiles of 4 x 4 level-1 blocks (a frame of one macroblock row or column has none)
    const int tiles_x = (L1.bw + 3) / 4, tiles_y = (L1.h / 8 + 3) / 4;
    if (tiles_x * tiles_y <= 0) return;
    VP8_LAUNCH(k_search1_coarse, dim3(tiles_x * tiles_y, L0.nrefs), dim3(64 * COARSE_WAVES), 0, s, a);
}

void launch_search1_batch(hipStream_t s, const CodingItem *items, int n, int level, int src_idx, int net_width) {
    BatchOf<Search1Args> b;
    b.n = n;
    int maxrefs = 0, totrefs = 0;
    for (int i = 0; i < n; ++i) {
        b.item[i] = search1_args(items[i], level, src_idx, net_width);
        maxrefs = b.item[i].nrefs > maxrefs ? b.item[i].nrefs : maxrefs;
        totrefs += b.item[i].nrefs;
    }
    const int nblk = b.item[0].nblk;
    if (nblk <= 0 || maxrefs == 0 || search1_skip()) return;
    if (search1_split((size_t)nblk * totrefs))
        VP8_LAUNCH(k_search1_b, dim3((nblk + S1Map<true>::BLOCKS_PER_WG - 1) / S1Map<true>::BLOCKS_PER_WG, maxrefs, n), dim3(256), 0, s, b);
    else      // (68 registers, seven waves per SIMD.  Its twelve-slot predecessor, 70 registers, held to 64 spilled six and was no faster: 73.4-73.6 either way)
        VP8_LAUNCH(k_search1_plr_b, dim3(s1_fill_grid(nblk), 1, n), dim3(256), 0, s, b);      // the filled map: 51 blocks per workgroup (s1_fill_layout.h)
}

// test tap: the block-match metric on caller-supplied difference blocks (n x 16 ints)
__global__ __launch_bounds__(256) void k_weight_tap(const int32_t *d, int n, int32_t *out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    // the production form (weight_cols_pre) on a (current, prediction) byte pair with current - prediction = d:
    // columns as dwords, biased by -128
    uint32_t cc[4], pp[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        cc[c] = pp[c] = 0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int v = d[i * 16 + 4 * r + c];
            const uint32_t cb = (uint32_t)(v > 0 ? v : 0) ^ 0x80u, pb = (uint32_t)(v > 0 ? 0 : -v) ^ 0x80u;
            cc[c] |= cb << (8 * r);
            pp[c] |= pb << (8 * r);
        }
    }
    int pre[16];
#pragma unroll
    for (int c = 0; c < 4; ++c) weight_pre_column(cc[c], pre + 4 * c);
    out[i] = weight_cols_pre(pre, pp);
}
void launch_weight_tap(hipStream_t s, const int32_t *d, int n, int32_t *out) {
    hipLaunchKernelGGL(k_weight_tap, dim3((n + 255) / 256), dim3(256), 0, s, d, n, out);
}
// the same through the form the search kernels run (weight_mfma): a block per lane, every lane of every wave a different one.  The
// lanes past n take the last block again (an MFMA runs for the whole wave) and store nothing
__global__ __attribute__((amdgpu_waves_per_eu(8, 8))) __launch_bounds__(256) void k_weight_tap_mfma(const int32_t *d, int n, int32_t *out) {
    const int i0 = blockIdx.x * 256 + threadIdx.x, i = i0 < n ? i0 : n - 1;
    uint32_t cc[4];
    v4i pp;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        uint32_t cw = 0, pw = 0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int v = d[i * 16 + 4 * r + c];
            const uint32_t cb = (uint32_t)(v > 0 ? v : 0) ^ 0x80u, pb = (uint32_t)(v > 0 ? 0 : -v) ^ 0x80u;
            cw |= cb << (8 * r);
            pw |= pb << (8 * r);
        }
        cc[c] = cw;
        pp[c] = (int)pw;
    }
    int pre[16];
    weight_pre_block(cc, pre);
    v16i c16;
#pragma unroll
    for (int k = 0; k < 16; ++k) c16[k] = pre[k];
    const int w = weight_mfma(metric_a((int)threadIdx.x), c16, pp);
    if (i0 < n) out[i0] = w;
}
void launch_weight_tap_mfma(hipStream_t s, const int32_t *d, int n, int32_t *out) {
    hipLaunchKernelGGL(k_weight_tap_mfma, dim3((n + 255) / 256), dim3(256), 0, s, d, n, out);
}
// ... and through the row-order operand of the whole-pel search's loop form (metric_a_rows): the same blocks, the prediction given as four ROW
// dwords (byte c = column c), the current block's share as before
__global__ __attribute__((amdgpu_waves_per_eu(8, 8))) __launch_bounds__(256) void k_weight_tap_mfma_rows(const int32_t *d, int n, int32_t *out) {
    const int i0 = blockIdx.x * 256 + threadIdx.x, i = i0 < n ? i0 : n - 1;
    uint32_t cc[4] = {0, 0, 0, 0};
    v4i pp = {0, 0, 0, 0};
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        uint32_t pw = 0;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int v = d[i * 16 + 4 * r + c];
            const uint32_t cb = (uint32_t)(v > 0 ? v : 0) ^ 0x80u, pb = (uint32_t)(v > 0 ? 0 : -v) ^ 0x80u;
            cc[c] |= cb << (8 * r);
            pw |= pb << (8 * c);
        }
        pp[r] = (int)pw;
    }
    int pre[16];
    weight_pre_block(cc, pre);
    v16i c16;
#pragma unroll
    for (int k = 0; k < 16; ++k) c16[k] = pre[k];
    const int w = weight_mfma(metric_a_rows((int)threadIdx.x), c16, pp);
    if (i0 < n) out[i0] = w;
}
void launch_weight_tap_mfma_rows(hipStream_t s, const int32_t *d, int n, int32_t *out) {
    hipLaunchKernelGGL(k_weight_tap_mfma_rows, dim3((n + 255) / 256), dim3(256), 0, s, d, n, out);
}

}  // namespace vp8
