// kernels_overlay.hip -- layers burnt into the source frames (vp8hip_set_overlay_host / _device): logos, watermarks, subtitles.  The
// reference has nothing of the kind; the rule is the project's own and is stated bit for bit in include/vp8hip_host.h
// (vp8host_overlay_frame is its plain C++ form).
//
// k_overlay_prepare runs when a layer is set or moved, never per frame.  From the retained BGRA / RGBA copy it makes the layer's PREPARED
// PLANES, everything of the rule that does not depend on the frame: Yo and e, a byte each per luma pixel, and E (16 bits), T_u and T_v
// (32 bits) per chroma sample of the PICTURE's chroma grid -- so they depend on the parity of x and y, on the opacity and on the matrix.
// The planes lie on the picture's 4-sample grid: luma column j of a plane is picture column X0 + j with X0 = x rounded DOWN to a
// multiple of 4, chroma column j is chroma column CX0 + j with CX0 = (x >> 1) rounded down likewise, both strides are multiples of 4 and
// the margins hold e = 0 / E = 0.  A thread takes one chroma sample: its four layer pixels (a dword each), the byte dot products of the
// BGRA converter (v_dot4_u32_u8 for luma, v_dot4_i32_i8 on p - 128 for chroma), two 16-bit stores per luma plane, one store per chroma plane.
//
// k_overlay_b is the per-frame launch, ONE for all members of a batch (member = blockIdx.z), behind the pack or scale launch and in
// front of the denoiser, IN PLACE on the current surface.  A sample of the coded surface at (x, y) is composed from itself -- the pack
// has made it a copy of picture sample (min(x, pw - 1), min(y, ph - 1)) -- and the layers' values at that clamped position, so the
// kernel is element-wise, the padding included, and in place is race-free.
// Mapping (memory-bound: no LDS, no atomics, everything in registers):
//   * a lane owns a UNIT: 8 consecutive luma samples of two rows (two 8-byte accesses) and the 4 + 4 chroma samples under them (a
//     dword of U, a dword of V).  The coded width is a multiple of 16 and the surfaces are 16-byte aligned: a unit never straddles the
//     surface's edge, whatever the picture's width, so the frame side has no ragged unit;
//   * the grid covers the bounding box of the member's layers in units, clipped to the picture and widened over the padding where it
//     touches the last two columns or rows (the last chroma sample); it is sized by the largest box of the call, and workgroups outside a member's box leave at once;
//   * a lane reads its unit once, applies every layer that covers it in slot order, and writes once; a layer's planes are read with
//     the same aligned accesses (a dword of Yo and of e per 4 luma samples; 8 bytes of E and 16 of T_u and T_v per 4 chroma samples):
//     4-sample groups are wholly inside or wholly outside a plane.  Only groups that reach into the padding (the picture's width is
//     even, not a multiple of 4 or 8) take their layer values sample by sample, clamped;
//   * the divisions by 255 are the two identities of the header, in 32-bit multiply-adds and shifts.
#include "../../include/vp8hip_host.h"
#include "vp8hip_dev.h"

namespace vp8 {

namespace overlay {

struct PrepareArgs {
    const uint8_t *pixels;      // the retained copy: tight rows of lw pixels
    uint8_t *yo, *e;            // luma planes: lh rows of lstride bytes
    uint16_t *E;                // chroma planes: crows rows of cstride samples
    uint32_t *tu, *tv;
    int lw, lh, x, y, X0, lstride, CX0, cy0, cstride, crows, opacity;
    uint32_t cy, cu, cv, off, bias_u, bias_v;      // the matrix as byte rows at the pixel's byte positions, and the accumulators' starts
    int alpha_shift;            // bit position of A in a pixel's dword (24 for both formats)
};

struct Geo { int pw, ph, units_x, units_y; };

// (n + 127) / 255 for n in 0 .. 65025
__device__ __forceinline__ uint32_t div255_round(uint32_t n) {
    const uint32_t t = n + 128u;
    return (t + (t >> 8)) >> 8;
}

// four luma samples (a dword) composed with four Yo and four e
__device__ __forceinline__ uint32_t blend4(uint32_t s, uint32_t yo, uint32_t e) {
    uint32_t o = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t sk = (s >> (8 * k)) & 255u, yk = (yo >> (8 * k)) & 255u, ek = (e >> (8 * k)) & 255u;
        o |= div255_round(sk * (255u - ek) + yk * ek) << (8 * k);
    }
    return o;
}

// one chroma sample: N = src * 256 * (1020 - E) + T, ((N + 130560) >> 10) / 255
__device__ __forceinline__ uint32_t blendc(uint32_t s, uint32_t E, uint32_t T) {
    const uint32_t q = (s * 256u * (1020u - E) + T + 130560u) >> 10;      // at most 65408
    return (q * 0x8081u) >> 23;
}

__device__ __forceinline__ void overlay_body(const OverlayItem &it, const Geo &g) {
    const int bx = it.ux0 + (int)blockIdx.x * 32, by = it.uy0 + (int)blockIdx.y * 8;
    if (bx >= it.ux1 || by >= it.uy1) return;      // (the grid is the call's largest box)
    const int ux = bx + ((int)threadIdx.x & 31), uy = by + ((int)threadIdx.x >> 5);
    if (ux >= it.ux1 || uy >= it.uy1 || ux < 0 || uy < 0 || ux >= g.units_x || uy >= g.units_y) return;
    const int col = ux * 8, row = uy * 2, cw = g.pw >> 1, ch = g.ph >> 1;
    uint8_t *py0 = it.y.p + (ptrdiff_t)row * it.y.stride + col, *py1 = py0 + it.y.stride;
    uint8_t *pu = it.u.p + (ptrdiff_t)uy * it.u.stride + ux * 4, *pv = it.v.p + (ptrdiff_t)uy * it.v.stride + ux * 4;
    uint2 y01[2] = {*reinterpret_cast<const uint2 *>(py0), *reinterpret_cast<const uint2 *>(py1)};
    uint32_t u = *reinterpret_cast<const uint32_t *>(pu), v = *reinterpret_cast<const uint32_t *>(pv);
    bool wy = false, wc = false;
#pragma unroll
    for (int l = 0; l < VP8HIP_MAX_OVERLAYS; ++l) {
        if (l >= it.n) break;
        const OverlayLayer &L = it.layer[l];
        // luma: two rows of two 4-sample groups
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int lr = imin(row + r, g.ph - 1) - L.y;
            if (lr < 0 || lr >= L.lh) continue;
            const uint8_t *yo_row = L.base + (size_t)lr * (size_t)L.lstride, *e_row = yo_row + L.off_e;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int c = col + 4 * h;
                uint32_t yo4 = 0, e4 = 0;
                if (c + 4 <= g.pw) {
                    const int j = c - L.X0;
                    if (j < 0 || j >= L.lstride) continue;
                    e4 = *reinterpret_cast<const uint32_t *>(e_row + j);      // (both loads before the test: one round trip, not two)
                    yo4 = *reinterpret_cast<const uint32_t *>(yo_row + j);
                    if (!e4) continue;
                } else {      // the group reaches into the padding: the layer's values at the clamped column
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int j = imin(c + k, g.pw - 1) - L.X0;
                        if (j < 0 || j >= L.lstride) continue;
                        e4 |= (uint32_t)e_row[j] << (8 * k);
                        yo4 |= (uint32_t)yo_row[j] << (8 * k);
                    }
                    if (!e4) continue;
                }
                uint32_t &d = h ? y01[r].y : y01[r].x;
                d = blend4(d, yo4, e4);
                wy = true;
            }
        }
        // chroma: one group of four samples in each plane
        const int lc = imin(uy, ch - 1) - L.cy0;
        if (lc < 0 || lc >= L.crows) continue;
        const size_t at = (size_t)lc * (size_t)L.cstride;
        const uint16_t *E_row = reinterpret_cast<const uint16_t *>(L.base + L.off_E) + at;
        const uint32_t *tu_row = reinterpret_cast<const uint32_t *>(L.base + L.off_tu) + at, *tv_row = reinterpret_cast<const uint32_t *>(L.base + L.off_tv) + at;
        const int cc = ux * 4;
        uint32_t E[4] = {0, 0, 0, 0}, tu[4] = {0, 0, 0, 0}, tv[4] = {0, 0, 0, 0};
        if (cc + 4 <= cw) {
            const int j = cc - L.CX0;
            if (j < 0 || j >= L.cstride) continue;
            const uint2 e2 = *reinterpret_cast<const uint2 *>(E_row + j);
            const uint4 a = *reinterpret_cast<const uint4 *>(tu_row + j), b = *reinterpret_cast<const uint4 *>(tv_row + j);
            if (!(e2.x | e2.y)) continue;
            E[0] = e2.x & 0xffffu; E[1] = e2.x >> 16; E[2] = e2.y & 0xffffu; E[3] = e2.y >> 16;
            tu[0] = a.x; tu[1] = a.y; tu[2] = a.z; tu[3] = a.w;
            tv[0] = b.x; tv[1] = b.y; tv[2] = b.z; tv[3] = b.w;
        } else {
            uint32_t any = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int j = imin(cc + k, cw - 1) - L.CX0;
                if (j < 0 || j >= L.cstride) continue;
                E[k] = E_row[j]; tu[k] = tu_row[j]; tv[k] = tv_row[j];
                any |= E[k];
            }
            if (!any) continue;
        }
        uint32_t ou = 0, ov = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            ou |= blendc((u >> (8 * k)) & 255u, E[k], tu[k]) << (8 * k);
            ov |= blendc((v >> (8 * k)) & 255u, E[k], tv[k]) << (8 * k);
        }
        u = ou; v = ov;
        wc = true;
    }
    if (wy) {
        *reinterpret_cast<uint2 *>(py0) = y01[0];
        *reinterpret_cast<uint2 *>(py1) = y01[1];
    }
    if (wc) {
        *reinterpret_cast<uint32_t *>(pu) = u;
        *reinterpret_cast<uint32_t *>(pv) = v;
    }
}

}  // namespace overlay

__global__ __launch_bounds__(256) void k_overlay_prepare(overlay::PrepareArgs a) {
    const int ci = (int)blockIdx.x * 64 + ((int)threadIdx.x & 63), cj = (int)blockIdx.y * 4 + ((int)threadIdx.x >> 6);
    if (ci >= a.cstride || cj >= a.crows) return;
    uint32_t E = 0;
    int tu = 0, tv = 0;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int py = 2 * (a.cy0 + cj) + r, ly = py - a.y;      // picture row, layer row
        const int px = 2 * (a.CX0 + ci), lx = px - a.x, j = px - a.X0;
        uint32_t yo2 = 0, e2 = 0;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            if (ly < 0 || ly >= a.lh || lx + i < 0 || lx + i >= a.lw) continue;
            const uint32_t p = *reinterpret_cast<const uint32_t *>(a.pixels + ((size_t)ly * (size_t)a.lw + (size_t)(lx + i)) * 4);
            const uint32_t alpha = (p >> a.alpha_shift) & 255u;
            const uint32_t n = alpha * (uint32_t)a.opacity, t = n + 128u;      // (n + 127) / 255
            const uint32_t e = (t + (t >> 8)) >> 8;
            const uint32_t yo = (__builtin_amdgcn_udot4(p, a.cy, 128u, false) >> 8) + a.off;
            const int s = (int)(p ^ 0x80808080u);
            E += e;
            tu += (int)e * __builtin_amdgcn_sdot4(s, (int)a.cu, (int)a.bias_u, false);
            tv += (int)e * __builtin_amdgcn_sdot4(s, (int)a.cv, (int)a.bias_v, false);
            e2 |= e << (8 * i);
            yo2 |= yo << (8 * i);
        }
        // (the planes' columns start and end on multiples of 4: a pair is inside or outside as a whole; margins take e = 0)
        if (ly >= 0 && ly < a.lh && j >= 0 && j < a.lstride) {
            const size_t at = (size_t)ly * (size_t)a.lstride + (size_t)j;
            *reinterpret_cast<uint16_t *>(a.yo + at) = (uint16_t)yo2;
            *reinterpret_cast<uint16_t *>(a.e + at) = (uint16_t)e2;
        }
    }
    const size_t at = (size_t)cj * (size_t)a.cstride + (size_t)ci;
    a.E[at] = (uint16_t)E;
    a.tu[at] = (uint32_t)tu;
    a.tv[at] = (uint32_t)tv;
}

static_assert(sizeof(BatchOf<OverlayItem>) + sizeof(overlay::Geo) <= 4096, "a batch's argument blocks travel in the 4 KiB kernel-argument segment");
__global__ __launch_bounds__(256) void k_overlay_b(BatchOf<OverlayItem> b, overlay::Geo g) {
    overlay::overlay_body(b.item[blockIdx.z], g);
}

OverlayPlanes overlay_planes(int lw, int lh, int x, int y) {
    OverlayPlanes p;
    p.X0 = x & ~3;
    p.lstride = ((x + lw + 3) & ~3) - p.X0;
    p.CX0 = (x >> 1) & ~3;
    p.cstride = ((((x + lw - 1) >> 1) + 1 + 3) & ~3) - p.CX0;
    p.cy0 = y >> 1;
    p.crows = ((y + lh - 1) >> 1) + 1 - p.cy0;
    const size_t nl = ((size_t)p.lstride * (size_t)lh + 255) & ~(size_t)255, nc = (size_t)p.cstride * (size_t)p.crows;
    p.off_e = nl;
    p.off_E = 2 * nl;
    p.off_tu = p.off_E + ((2 * nc + 255) & ~(size_t)255);
    p.off_tv = p.off_tu + ((4 * nc + 255) & ~(size_t)255);
    p.bytes = p.off_tv + ((4 * nc + 255) & ~(size_t)255);
    return p;
}

bool launch_overlay_prepare(hipStream_t s, int format, int matrix, const uint8_t *pixels, int lw, int lh, int x, int y, int opacity, uint8_t *planes) {
    int32_t c[9], off;
    if ((format != VP8HOST_FORMAT_BGRA && format != VP8HOST_FORMAT_RGBA) || vp8host_colour_coefficients(matrix, c, &off) != 0 || !pixels || !planes) return false;
    const OverlayPlanes p = overlay_planes(lw, lh, x, y);
    overlay::PrepareArgs a = {};
    a.pixels = pixels;
    a.yo = planes;
    a.e = planes + p.off_e;
    a.E = reinterpret_cast<uint16_t *>(planes + p.off_E);
    a.tu = reinterpret_cast<uint32_t *>(planes + p.off_tu);
    a.tv = reinterpret_cast<uint32_t *>(planes + p.off_tv);
    a.lw = lw; a.lh = lh; a.x = x; a.y = y; a.opacity = opacity;
    a.X0 = p.X0; a.lstride = p.lstride; a.CX0 = p.CX0; a.cy0 = p.cy0; a.cstride = p.cstride; a.crows = p.crows;
    const int at[3] = {format == VP8HOST_FORMAT_BGRA ? 16 : 0, 8, format == VP8HOST_FORMAT_BGRA ? 0 : 16};      // R, G, B in a pixel's dword
    int sum_u = 0, sum_v = 0;
    for (int k = 0; k < 3; ++k) {
        a.cy |= (uint32_t)(uint8_t)c[k] << at[k];
        a.cu |= (uint32_t)(uint8_t)(int8_t)c[3 + k] << at[k];
        a.cv |= (uint32_t)(uint8_t)(int8_t)c[6 + k] << at[k];
        sum_u += c[3 + k];
        sum_v += c[6 + k];
    }
    a.off = (uint32_t)off;
    a.bias_u = (uint32_t)(32768 + 128 * sum_u);      // the dot product sees p - 128
    a.bias_v = (uint32_t)(32768 + 128 * sum_v);
    a.alpha_shift = 24;
    VP8_LAUNCH(k_overlay_prepare, dim3((p.cstride + 63) / 64, (p.crows + 3) / 4, 1), dim3(256), 0, s, a);
    return true;
}

void launch_overlay_batch(hipStream_t s, const OverlayItem *items, int n, int pw, int ph) {
    if (n <= 0) return;
    BatchOf<OverlayItem> b;
    b.n = n;
    int gx = 0, gy = 0;
    for (int i = 0; i < n; ++i) {
        b.item[i] = items[i];
        gx = items[i].ux1 - items[i].ux0 > gx ? items[i].ux1 - items[i].ux0 : gx;
        gy = items[i].uy1 - items[i].uy0 > gy ? items[i].uy1 - items[i].uy0 : gy;
    }
    if (gx <= 0 || gy <= 0) return;
    overlay::Geo g;
    g.pw = pw; g.ph = ph;
    g.units_x = items[0].y.w / 8;
    g.units_y = items[0].y.h / 2;
    VP8_LAUNCH(k_overlay_b, dim3((gx + 31) / 32, (gy + 7) / 8, n), dim3(256), 0, s, b, g);
}

}  // namespace vp8
