// kernels_compose.hip -- a frame composed of scaled video tiles on its way into the padded surfaces (vp8hip_set_canvas): the grid of a
// conference, a speaker with thumbnails, a film with bars.  The project's own: the reference takes one source per frame.
//
// k_compose_b stands where k_pack_b and k_scale_b stand: ONE launch per frame writes Y[0], U and V of the surface.  The arithmetic is
// include/vp8hip_host.h's ("CANVAS"): the background, then every present tile in index order through the scaler's two table-driven
// passes (vp8host_scale_taps' own tables) into its rectangle, then copy_with_padding.
//
// Mapping: a workgroup of 256 owns an output tile of 64 x 32 samples of one plane of the SURFACE, and keeps it in LDS.  It fills it
// with the background and walks the tiles that intersect it in index order (from the last one that covers it whole: what lies
// under that one is never seen).  For each it walks the intersection in blocks of the shape scale_geo gives that tile's ratio
// (64 x 32 outputs unless the ratio is large), starting where the intersection starts -- the plan's spans are taken over every
// offset, not only the aligned ones, so a block's source rectangle is never larger than the plan allows: the block's rows of the two
// tables into LDS, the source rectangle through LDS in dwords (bytes when the plane's base, pitch or width is off a dword), in chunks
// of `rows` source rows, the horizontal pass into an int16 block, the vertical pass out of that into the output tile (a tile of equal
// sizes under the area filter is the identity and is copied, no pass is run).  A later tile overwrites an earlier one in LDS, behind
// a barrier: overlaps need no atomics and no second pass over memory.  Then the samples right of and below the picture repeat its edge (the edge lies in the same
// output tile as its padding: the picture is fewer than 16 samples smaller than the surface, and 64 and 32 are multiples of 16), and
// the tile is stored once, in 8-byte units as k_pack_b stores.  Every source sample an output tile needs comes from memory once per
// tile that holds it; every surface byte is written exactly once.
//
// The tiles' geometry, block shapes and tables live in a device blob made by vp8hip_set_canvas (sixteen tiles' descriptors do not fit
// the 4 KiB argument segment next to their tables' pointers and the frame's planes); a launch passes only the frame's pointers and pitches.
#include <algorithm>
#include <vector>

#include "../../include/vp8hip_host.h"
#include "vp8hip_dev.h"

namespace vp8 {

namespace compose {

constexpr int TW = 64, TH = 32;      // the output tile
constexpr int OUT_BYTES = TW * TH;

struct Head { int32_t n, bg[3]; };
// one tile: its rectangle, the incoming size, the block shape and LDS layout, and its four tables (luma x, luma y, chroma x, chroma y)
// as byte offsets into the blob
struct TileDesc { int32_t x, y, w, h, in_w, in_h; ScaleGeo g; uint32_t off_start[4], off_coef[4]; int32_t taps[4]; };
constexpr size_t TABLES_AT = (sizeof(Head) + VP8HIP_MAX_TILES * sizeof(TileDesc) + 15) / 16 * 16;
struct Args { Plane out[3]; int32_t tiles_x[3], tiles[3], pw, ph; const uint8_t *blob; ComposeSource src[VP8HIP_MAX_TILES]; };
struct Tab { const int32_t *start; const int16_t *coef; int n; };

// outputs [cx0, cx1) x [cy0, cy1) of one plane of one tile (the tile's own coordinates; at most g.tw x g.th of them) into dst, rows TW apart
__device__ __forceinline__ void block(const uint8_t *src, int pitch, bool dwords, const Tab &X, const Tab &Y, const ScaleGeo &g, int cx0, int cx1, int cy0,
                                      int cy1, uint8_t *work, uint8_t *dst) {
    const int tid = (int)threadIdx.x;
    const int tw = cx1 - cx0, th = cy1 - cy0, nx = X.n, ny = Y.n;
    uint8_t *s_src = work;                                                  // [rows][pitch]
    int16_t *s_t = reinterpret_cast<int16_t *>(work + g.off_t);             // [span_y][g.tw]
    int16_t *s_cx = reinterpret_cast<int16_t *>(work + g.off_cx);           // [g.tw][nx]
    int16_t *s_cy = reinterpret_cast<int16_t *>(work + g.off_cy);           // [g.th][ny]
    int32_t *s_sx = reinterpret_cast<int32_t *>(work + g.off_sx);           // [g.tw]
    int32_t *s_sy = reinterpret_cast<int32_t *>(work + g.off_sy);           // [g.th]
    // the source rectangle: columns [sx0, sx1) with sx0 rounded down to a dword on the dword path, rows [sy0, sy1)
    const int sx0 = dwords ? X.start[cx0] & ~3 : X.start[cx0], sx1 = X.start[cx1 - 1] + nx;
    const int sy0 = Y.start[cy0], sy1 = Y.start[cy1 - 1] + ny;
    __syncthreads();      // (whatever read the work area or wrote the output tile before this block has finished)
    for (int i = tid; i < tw; i += 256) s_sx[i] = X.start[cx0 + i] - sx0;
    for (int i = tid; i < th; i += 256) s_sy[i] = Y.start[cy0 + i] - sy0;
    for (int i = tid; i < tw * nx; i += 256) s_cx[i] = X.coef[(size_t)cx0 * nx + i];
    for (int i = tid; i < th * ny; i += 256) s_cy[i] = Y.coef[(size_t)cy0 * ny + i];
    const int dpr = (sx1 - sx0 + 3) >> 2, bpr = sx1 - sx0;
    for (int r0 = sy0; r0 < sy1; r0 += g.rows) {
        const int nr = min(g.rows, sy1 - r0);
        __syncthreads();      // (the tables are in; the previous chunk has been read)
        if (dwords) {
            for (int i = tid; i < nr * dpr; i += 256) {
                const int r = i / dpr, c = i - r * dpr;
                *reinterpret_cast<uint32_t *>(s_src + r * g.pitch + 4 * c) = *reinterpret_cast<const uint32_t *>(src + (size_t)(r0 + r) * pitch + sx0 + 4 * c);
            }
        } else {
            for (int i = tid; i < nr * bpr; i += 256) {
                const int r = i / bpr, c = i - r * bpr;
                s_src[r * g.pitch + c] = src[(size_t)(r0 + r) * pitch + sx0 + c];
            }
        }
        __syncthreads();
        // horizontal: t[y][i] = (sum_k cx[i][k] * src[y][start_x[i] + k] + 32) >> 6
        for (int i = tid; i < nr * tw; i += 256) {
            const int r = i / tw, x = i - r * tw;
            const uint8_t *s = s_src + r * g.pitch + s_sx[x];
            const int16_t *c = s_cx + x * nx;
            int acc = 32;
            for (int k = 0; k < nx; ++k) acc += (int)c[k] * (int)s[k];
            s_t[(r0 - sy0 + r) * g.tw + x] = (int16_t)(acc >> 6);
        }
    }
    __syncthreads();
    // vertical: out[j][i] = clamp((sum_k cy[j][k] * t[start_y[j] + k][i] + (1 << 17)) >> 18, 0, 255)
    for (int i = tid; i < th * tw; i += 256) {
        const int j = i / tw, x = i - j * tw;
        const int16_t *t = s_t + s_sy[j] * g.tw + x;
        const int16_t *c = s_cy + j * ny;
        int acc = 1 << 17;
        for (int k = 0; k < ny; ++k) acc += (int)c[k] * (int)t[k * g.tw];
        acc >>= 18;
        dst[j * TW + x] = (uint8_t)(acc < 0 ? 0 : (acc > 255 ? 255 : acc));
    }
}

__device__ __forceinline__ void compose_body(const Args &a, uint8_t *lds) {
    int tile = (int)blockIdx.x, p = 0;
    if (tile >= a.tiles[0]) { tile -= a.tiles[0]; p = 1; if (tile >= a.tiles[1]) { tile -= a.tiles[1]; p = 2; } }
    const Plane &out = a.out[p];
    const int sub = p ? 1 : 0;      // chroma: every size and position halved
    const Head &hd = *reinterpret_cast<const Head *>(a.blob);
    const TileDesc *td = reinterpret_cast<const TileDesc *>(a.blob + sizeof(Head));
    const int tid = (int)threadIdx.x;
    const int pw = a.pw >> sub, ph = a.ph >> sub;
    const int x0 = (tile % a.tiles_x[p]) * TW, y0 = (tile / a.tiles_x[p]) * TH;
    const int tw = min(TW, out.w - x0), th = min(TH, out.h - y0);
    const int px1 = min(x0 + tw, pw), py1 = min(y0 + th, ph);      // the picture's part of the output tile: [x0, px1) x [y0, py1), never empty
    uint8_t *s_out = lds;      // [TH][TW]
    uint8_t *work = lds + OUT_BYTES;
    for (int i = tid; i < OUT_BYTES / 4; i += 256) reinterpret_cast<uint32_t *>(s_out)[i] = (uint32_t)hd.bg[p] * 0x01010101u;
    int first = 0;      // the last present tile that covers the picture's part whole
    for (int k = 0; k < hd.n; ++k) {
        const TileDesc &T = td[k];
        const int rx = T.x >> sub, ry = T.y >> sub;
        if (a.src[k].p[0] && rx <= x0 && ry <= y0 && rx + (T.w >> sub) >= px1 && ry + (T.h >> sub) >= py1) first = k;
    }
    for (int k = first; k < hd.n; ++k) {
        if (!a.src[k].p[0]) continue;      // absent this frame
        const TileDesc &T = td[k];
        const int rx = T.x >> sub, ry = T.y >> sub;
        const int lx0 = max(x0, rx) - rx, lx1 = min(px1, rx + (T.w >> sub)) - rx, ly0 = max(y0, ry) - ry, ly1 = min(py1, ry + (T.h >> sub)) - ry;
        if (lx0 >= lx1 || ly0 >= ly1) continue;
        const ScaleGeo &g = T.g;
        const int kx = p ? 2 : 0, ky = p ? 3 : 1;
        const Tab X{reinterpret_cast<const int32_t *>(a.blob + T.off_start[kx]), reinterpret_cast<const int16_t *>(a.blob + T.off_coef[kx]), T.taps[kx]};
        const Tab Y{reinterpret_cast<const int32_t *>(a.blob + T.off_start[ky]), reinterpret_cast<const int16_t *>(a.blob + T.off_coef[ky]), T.taps[ky]};
        const uint8_t *src = a.src[k].p[p];
        const int pitch = a.src[k].pitch[p];
        const bool dwords = (((uintptr_t)src | (uintptr_t)pitch | (uintptr_t)(T.in_w >> sub)) & 3) == 0;      // every row starts and ends on a dword
        if (T.in_w == T.w && T.in_h == T.h && X.n == 1 && Y.n == 1) {
            // equal sizes under the area filter: one tap of 4096 on sample i for output i in both tables, and (4096 * 64 s + 2^17) >> 18
            // is s -- the rectangle is copied, no pass is run (Lanczos-3 at equal sizes has seven taps and takes the passes: the same bytes)
            uint8_t *dst = s_out + (ly0 + ry - y0) * TW + (lx0 + rx - x0);
            const uint8_t *s = src + (size_t)ly0 * pitch + lx0;
            const int cw = lx1 - lx0, ch = ly1 - ly0;
            const int whole = (dwords && ((lx0 | (lx0 + rx - x0)) & 3) == 0) ? cw & ~3 : 0, rest = cw - whole;      // columns copied as dwords / as bytes
            __syncthreads();      // (whatever wrote the output tile before has finished)
            for (int i = tid; i < ch * (whole >> 2); i += 256) {
                const int r = i / (whole >> 2), c = 4 * (i - r * (whole >> 2));
                *reinterpret_cast<uint32_t *>(dst + r * TW + c) = *reinterpret_cast<const uint32_t *>(s + (size_t)r * pitch + c);
            }
            for (int i = tid; i < ch * rest; i += 256) {
                const int r = i / rest, c = whole + i - r * rest;
                dst[r * TW + c] = s[(size_t)r * pitch + c];
            }
            continue;
        }
        for (int by = ly0; by < ly1; by += g.th)
            for (int bx = lx0; bx < lx1; bx += g.tw) {
                const int cx1 = min(bx + g.tw, lx1), cy1 = min(by + g.th, ly1);
                block(src, pitch, dwords, X, Y, g, bx, cx1, by, cy1, work, s_out + (by + ry - y0) * TW + (bx + rx - x0));
            }
    }
    __syncthreads();
    if (px1 < x0 + tw || py1 < y0 + th) {      // copy_with_padding: right of and below the picture, its edge (samples inside the picture are not written here)
        const int ex = px1 - 1 - x0, ey = py1 - 1 - y0;
        for (int i = tid; i < th * tw; i += 256) {
            const int j = i / tw, x = i - j * tw;
            if (x > ex || j > ey) s_out[j * TW + x] = s_out[min(j, ey) * TW + min(x, ex)];
        }
        __syncthreads();
    }
    const int upr = tw >> 3;      // 8-byte units per row of the tile (surface widths are multiples of 8)
    for (int i = tid; i < th * upr; i += 256) {
        const int j = i / upr, x = (i - j * upr) * 8;
        *reinterpret_cast<uint2 *>(out.p + (ptrdiff_t)(y0 + j) * out.stride + x0 + x) = *reinterpret_cast<const uint2 *>(s_out + j * TW + x);
    }
}

}  // namespace compose

static_assert(sizeof(compose::Args) <= 4096, "the frame's pointers and pitches travel in the 4 KiB kernel-argument segment");
__global__ __launch_bounds__(256) void k_compose_b(compose::Args a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t compose_lds[];
    compose::compose_body(a, compose_lds);
}

// ---- host side: the blob of one canvas, and the launch -----------------------------------------------------------------------------

bool compose_plan_make(ComposePlan *p, const vp8hip_tile *tiles, int n, const int bg[3], std::vector<uint8_t> &blob) {
    using namespace compose;
    if (n < 1 || n > VP8HIP_MAX_TILES) return false;
    blob.assign(TABLES_AT, 0);
    Head hd{};
    hd.n = n;
    for (int k = 0; k < 3; ++k) hd.bg[k] = bg[k];
    size_t lds = 0;
    std::vector<TileDesc> td((size_t)VP8HIP_MAX_TILES);
    for (int i = 0; i < n; ++i) {
        const vp8hip_tile &t = tiles[i];
        ScalePlan sp;      // the tile's four tables as long as the tile is wide and high: nothing is stretched over a padding
        std::vector<uint8_t> tb;
        if (!scale_plan_make(&sp, t.in_w, t.in_h, t.w, t.h, t.w, t.h, t.filter, tb)) return false;
        for (int k = 0; k < 4; ++k) {      // the most source samples ANY 8 << j outputs in a row touch: a block starts where a seam puts it
            const int32_t *start = reinterpret_cast<const int32_t *>(tb.data() + sp.d[k].off_start);
            const int n_out = sp.d[k].n_surf;
            for (int j = 0; j < 4; ++j)
                for (int a = 0; a < n_out; ++a)
                    sp.d[k].max_span[j] = std::max(sp.d[k].max_span[j], start[std::min(a + (8 << j), n_out) - 1] + sp.d[k].n - start[a]);
        }
        const size_t base = blob.size();      // (a multiple of 16, as every table's size is)
        blob.insert(blob.end(), tb.begin(), tb.end());
        TileDesc &T = td[(size_t)i];
        T = TileDesc{};
        T.x = t.x; T.y = t.y; T.w = t.w; T.h = t.h; T.in_w = t.in_w; T.in_h = t.in_h;
        T.g = scale_geo(sp);
        for (int k = 0; k < 4; ++k) {
            T.off_start[k] = (uint32_t)(base + sp.d[k].off_start);
            T.off_coef[k] = (uint32_t)(base + sp.d[k].off_coef);
            T.taps[k] = sp.d[k].n;
        }
        lds = std::max(lds, (size_t)OUT_BYTES + (size_t)T.g.off_sy + (size_t)T.g.th * 4);
    }
    memcpy(blob.data(), &hd, sizeof(hd));
    memcpy(blob.data() + sizeof(Head), td.data(), td.size() * sizeof(TileDesc));
    p->n = n;
    p->lds = (lds + 15) / 16 * 16;
    return true;
}

void launch_compose(hipStream_t s, const Frame &f, const ComposePlan &plan, int pw, int ph, const ComposeSource *src) {
    using namespace compose;
    Args a{};
    const Plane *out[3] = {&f.Y[0], &f.U, &f.V};
    int tiles = 0;
    for (int k = 0; k < 3; ++k) {
        a.out[k] = *out[k];
        a.tiles_x[k] = (out[k]->w + TW - 1) / TW;
        a.tiles[k] = a.tiles_x[k] * ((out[k]->h + TH - 1) / TH);
        tiles += a.tiles[k];
    }
    a.blob = plan.d_blob;
    a.pw = pw;
    a.ph = ph;
    for (int k = 0; k < plan.n; ++k) a.src[k] = src[k];
    VP8_LAUNCH(k_compose_b, dim3(tiles), dim3(256), plan.lds, s, a);
}

}  // namespace vp8
