// kernels_scale.hip -- source frames larger than the coded picture, scaled down on their way into the padded surfaces.
// The branch of get_yuv420_frame the reference planned and never wrote ("== no resize", encIO.h:228; the buffer for "the resized
// input frame (and padded along the way, to avoid double-copy)", init.h:414-417; dst = src "for now", init.h:1731-1732).
//
// k_scale_b stands where k_pack_b stands: tight planes of the incoming size -> Y[0], U, V of a frame, all three planes and every
// member of a batch in one launch.  The arithmetic is include/vp8hip_host.h's (vp8host_scale_taps): separable, table-driven,
// horizontal pass into int16, vertical pass out of it.  copy_with_padding (encIO.h:141-196) costs nothing extra: the tables the
// kernel is given are as long as the SURFACE is wide and high, their last entry repeated over the padding, so the samples right
// of and below the scaled picture are computed like any other and come out as repeats of its edge.
//
// Mapping: a workgroup of 256 owns a tile of tw x th output samples of one plane (64 x 32 unless the ratio is large).  It copies
// its rows of the two tables into LDS once, brings the source rectangle the tile needs through LDS in dwords, coalesced along the
// rows (in chunks of `rows` source rows when the rectangle is larger than the LDS set aside for it), runs the horizontal pass
// into an int16 tile, the vertical pass out of that into a byte tile, and stores 8-byte units as k_pack_b does.
#include <algorithm>
#include <vector>

#include "../../include/vp8hip_host.h"
#include "vp8hip_dev.h"

namespace vp8 {

namespace scale {

struct Tab { const int32_t *start; const int16_t *coef; int n; };      // coef: n per output, rows end to end
struct PlaneJob { Plane out; const uint8_t *src; int in_w, in_h; Tab x, y; int tiles_x, tiles; };
struct Item { PlaneJob p[3]; };
// the launch's geometry, the same for every member: tile size, LDS layout (byte offsets), source rows per chunk
using Geo = ScaleGeo;

__device__ __forceinline__ void scale_body(const Item &a, const Geo &g, uint8_t *lds) {
    int tile = (int)blockIdx.x;
    const PlaneJob *pj = &a.p[0];
    if (tile >= pj->tiles) { tile -= pj->tiles; pj = &a.p[1]; if (tile >= pj->tiles) { tile -= pj->tiles; pj = &a.p[2]; } }
    const PlaneJob &P = *pj;
    const int tid = (int)threadIdx.x;
    const int x0 = (tile % P.tiles_x) * g.tw, y0 = (tile / P.tiles_x) * g.th;
    const int tw = min(g.tw, P.out.w - x0), th = min(g.th, P.out.h - y0);
    const int nx = P.x.n, ny = P.y.n;
    uint8_t *s_src = lds;                                                  // [rows][pitch], later the finished tile [th][g.tw]
    int16_t *s_t = reinterpret_cast<int16_t *>(lds + g.off_t);             // [span_y][g.tw]
    int16_t *s_cx = reinterpret_cast<int16_t *>(lds + g.off_cx);           // [g.tw][nx]
    int16_t *s_cy = reinterpret_cast<int16_t *>(lds + g.off_cy);           // [g.th][ny]
    int32_t *s_sx = reinterpret_cast<int32_t *>(lds + g.off_sx);           // [g.tw]
    int32_t *s_sy = reinterpret_cast<int32_t *>(lds + g.off_sy);           // [g.th]
    // the source rectangle: columns [sx0, sx1) with sx0 rounded down to a dword, rows [sy0, sy1)
    const int sx0 = P.x.start[x0] & ~3, sx1 = P.x.start[x0 + tw - 1] + nx;
    const int sy0 = P.y.start[y0], sy1 = P.y.start[y0 + th - 1] + ny;
    for (int i = tid; i < tw; i += 256) s_sx[i] = P.x.start[x0 + i] - sx0;
    for (int i = tid; i < th; i += 256) s_sy[i] = P.y.start[y0 + i] - sy0;
    for (int i = tid; i < tw * nx; i += 256) s_cx[i] = P.x.coef[(size_t)x0 * nx + i];
    for (int i = tid; i < th * ny; i += 256) s_cy[i] = P.y.coef[(size_t)y0 * ny + i];
    const bool dwords = (((uintptr_t)P.src | (uintptr_t)P.in_w) & 3) == 0;     // every source row starts on a dword
    const int dpr = (sx1 - sx0 + 3) >> 2;                                       // dwords per row of the rectangle
    for (int r0 = sy0; r0 < sy1; r0 += g.rows) {
        const int nr = min(g.rows, sy1 - r0);
        __syncthreads();      // (the tables are in; the previous chunk has been read)
        if (dwords) {
            for (int i = tid; i < nr * dpr; i += 256) {
                const int r = i / dpr, c = i - r * dpr;
                *reinterpret_cast<uint32_t *>(s_src + r * g.pitch + 4 * c) =
                    *reinterpret_cast<const uint32_t *>(P.src + (size_t)(r0 + r) * P.in_w + sx0 + 4 * c);
            }
        } else {
            const int bpr = sx1 - sx0;
            for (int i = tid; i < nr * bpr; i += 256) {
                const int r = i / bpr, c = i - r * bpr;
                s_src[r * g.pitch + c] = P.src[(size_t)(r0 + r) * P.in_w + sx0 + c];
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
        s_src[j * g.tw + x] = (uint8_t)(acc < 0 ? 0 : (acc > 255 ? 255 : acc));
    }
    __syncthreads();
    const int upr = tw >> 3;      // 8-byte units per row of the tile (surface widths are multiples of 8)
    for (int i = tid; i < th * upr; i += 256) {
        const int j = i / upr, x = (i - j * upr) * 8;
        *reinterpret_cast<uint2 *>(P.out.p + (ptrdiff_t)(y0 + j) * P.out.stride + x0 + x) = *reinterpret_cast<const uint2 *>(s_src + j * g.tw + x);
    }
}

}  // namespace scale

static_assert(sizeof(BatchOf<scale::Item>) + sizeof(scale::Geo) <= 4096, "a batch's argument blocks travel in the 4 KiB kernel-argument segment");
__global__ __launch_bounds__(256) void k_scale_b(BatchOf<scale::Item> b, scale::Geo g) {
    extern __shared__ __attribute__((aligned(16))) uint8_t scale_lds[];
    scale::scale_body(b.item[blockIdx.z], g, scale_lds);
}

// ---- host side: the tables of one context, and the launch ------------------------------------------------------------------------

// One dimension of one plane: the table of vp8host_scale_taps for n_in -> n_out, stretched to n_surf entries (the last one repeated:
// copy_with_padding) and packed to n taps per row.  Appends to `blob`, 16-byte aligned; returns false if the table is refused.
static bool scale_table(int n_in, int n_out, int n_surf, int kind, std::vector<uint8_t> &blob, ScaleDim *d) {
    std::vector<int32_t> start((size_t)n_out);
    std::vector<int16_t> coef((size_t)n_out * VP8HOST_SCALE_MAX_TAPS);
    int32_t n = 0;
    if (vp8host_scale_taps(n_in, n_out, kind, &n, start.data(), coef.data()) != 0) return false;
    d->n = n;
    d->n_in = n_in;
    d->n_surf = n_surf;
    for (int k = 0; k < 4; ++k) {      // the most source samples a tile of 8 << k outputs touches
        const int t = 8 << k;
        d->max_span[k] = 0;
        for (int x0 = 0; x0 < n_surf; x0 += t) {
            const int a = start[std::min(x0, n_out - 1)], b = start[std::min(std::min(x0 + t, n_surf) - 1, n_out - 1)] + n;
            d->max_span[k] = std::max(d->max_span[k], b - a);
        }
    }
    d->off_start = blob.size();
    blob.resize(blob.size() + ((size_t)n_surf * 4 + 15) / 16 * 16);
    d->off_coef = blob.size();
    blob.resize(blob.size() + ((size_t)n_surf * n * 2 + 15) / 16 * 16);
    int32_t *s = reinterpret_cast<int32_t *>(blob.data() + d->off_start);
    int16_t *c = reinterpret_cast<int16_t *>(blob.data() + d->off_coef);
    for (int i = 0; i < n_surf; ++i) {
        const int j = std::min(i, n_out - 1);
        s[i] = start[j];
        for (int k = 0; k < n; ++k) c[(size_t)i * n + k] = coef[(size_t)j * VP8HOST_SCALE_MAX_TAPS + k];
    }
    return true;
}

bool scale_plan_make(ScalePlan *p, int in_w, int in_h, int dst_w, int dst_h, int W, int H, int kind, std::vector<uint8_t> &blob) {
    blob.clear();
    p->in_w = in_w; p->in_h = in_h; p->kind = kind;
    return scale_table(in_w, dst_w, W, kind, blob, &p->d[0]) && scale_table(in_h, dst_h, H, kind, blob, &p->d[1]) &&
           scale_table(in_w / 2, dst_w / 2, W / 2, kind, blob, &p->d[2]) && scale_table(in_h / 2, dst_h / 2, H / 2, kind, blob, &p->d[3]);
}

static scale::Tab scale_tab(const ScalePlan &p, int k) {
    return scale::Tab{reinterpret_cast<const int32_t *>(p.d_blob + p.d[k].off_start), reinterpret_cast<const int16_t *>(p.d_blob + p.d[k].off_coef), p.d[k].n};
}

// Tile and LDS layout for a plan: 64 x 32 outputs, halved (height first) until the int16 tile and the tables fit 24 KB; the source
// rectangle gets what is left of 40 KB, in whole rows.  Luma decides (the chroma planes' spans are never larger).
ScaleGeo scale_geo(const ScalePlan &p) {
    int kx = 3, ky = 2;      // tile = (8 << kx) x (8 << ky)
    scale::Geo g{};
    for (;;) {
        g.tw = 8 << kx;
        g.th = 8 << ky;
        g.span_y = std::max(p.d[1].max_span[ky], p.d[3].max_span[ky]);
        const int span_x = std::max(p.d[0].max_span[kx], p.d[2].max_span[kx]);
        g.pitch = (span_x + 3 + 3) / 4 * 4 + 4;      // (the rectangle starts up to three samples early: dword alignment)
        const int nx = std::max(p.d[0].n, p.d[2].n), ny = std::max(p.d[1].n, p.d[3].n);
        const int t_bytes = (g.span_y * g.tw * 2 + 15) / 16 * 16, cx = (g.tw * nx * 2 + 15) / 16 * 16, cy = (g.th * ny * 2 + 15) / 16 * 16;
        const int fixed = t_bytes + cx + cy + g.tw * 4 + g.th * 4;
        const int out_bytes = g.tw * g.th;
        if (fixed > 24 * 1024 && (kx > 0 || ky > 0)) {      // (8 x 8 always fits: at most 288 rows of 8 int16 and two tables of 8 x 32)
            if (ky > 0) --ky; else --kx;
            continue;
        }
        int src_bytes = 40 * 1024 - fixed;
        g.rows = std::max(1, std::min(g.span_y, src_bytes / g.pitch));
        src_bytes = std::max(g.rows * g.pitch, out_bytes);
        src_bytes = (src_bytes + 15) / 16 * 16;
        g.off_t = src_bytes;
        g.off_cx = g.off_t + t_bytes;
        g.off_cy = g.off_cx + cx;
        g.off_sx = g.off_cy + cy;
        g.off_sy = g.off_sx + g.tw * 4;
        return g;
    }
}

void launch_scale_batch(hipStream_t s, const SourceItem *items, int n) {
    if (n <= 0) return;
    const scale::Geo g = scale_geo(*items[0].plan);
    BatchOf<scale::Item> b;
    b.n = n;
    int tiles = 0;
    for (int i = 0; i < n; ++i) {
        const ScalePlan &p = *items[i].plan;
        const Frame &f = *items[i].f;
        const Plane *out[3] = {&f.Y[0], &f.U, &f.V};
        const void *src[3] = {items[i].y, items[i].u, items[i].v};
        tiles = 0;
        for (int k = 0; k < 3; ++k) {
            scale::PlaneJob &j = b.item[i].p[k];
            j.out = *out[k];
            j.src = static_cast<const uint8_t *>(src[k]);
            j.in_w = k ? p.in_w / 2 : p.in_w;
            j.in_h = k ? p.in_h / 2 : p.in_h;
            j.x = scale_tab(p, k ? 2 : 0);
            j.y = scale_tab(p, k ? 3 : 1);
            j.tiles_x = (j.out.w + g.tw - 1) / g.tw;
            j.tiles = j.tiles_x * ((j.out.h + g.th - 1) / g.th);
            tiles += j.tiles;
        }
    }
    const size_t lds = (size_t)g.off_sy + (size_t)g.th * 4;
    VP8_LAUNCH(k_scale_b, dim3(tiles, 1, n), dim3(256), lds, s, b, g);
}

}  // namespace vp8
