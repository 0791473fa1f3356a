// kernels_geometry.hip -- the two geometric stages of the input side: the window of a pitched surface (vp8hip_set_source_window,
// k_window_b, in front of everything) and quarter turns with a mirror (vp8hip_set_source_orientation, k_orient_b, behind the
// deinterlacer and in front of the pack or scale launch).  Pure data movement; the rules are stated bit for bit in
// include/vp8hip_host.h (vp8host_source_window, vp8host_window_frame, vp8host_orient_frame are their plain C++ forms).  The project's
// own: the reference reads tight upright I420.
//
// k_window_b copies rows.  It knows no format: offset, pitch, row bytes and rows of up to three planes are kernel arguments (the
// table of include/vp8hip_host.h, evaluated by vp8host_source_window on the host).  A lane owns 16 bytes of one row; 64 consecutive
// lanes are 1 KiB of the row (or the ends of consecutive rows).  Neither pitch nor base is aligned, and the tight rows it writes are
// not either: loads and stores are unaligned vector accesses.  The last strip of a row that is no multiple of 16 bytes long goes byte
// by byte.  Bound: a lane reads src + offset + r * pitch + [x0, x0 + n) with r < rows, x0 + n <= row_bytes -- the window -- and writes
// dst + r * row_bytes + [x0, x0 + n) < rows * row_bytes.
//
// k_orient_b, the turns that do not transpose (turns 0 with the mirror, turns 2 with and without): an output row is an input row,
// reversed or not.  A lane owns 16 bytes of an output row, loads the 16 bytes they come from with one access, reverses them in
// registers (v_perm_b32) and stores them with one access; tails go byte by byte.
// The turns that transpose (1 and 3, with and without the mirror): out(x, y) = in(fy ? rw - 1 - y : y, fx ? rh - 1 - x : x).  A
// workgroup owns a tile of 64 x 64 input samples.
//   * Fill: lane t loads the dword (row t / 16 + 16 k, dword t % 16) of the tile, k = 0..3: 16 lanes are 64 contiguous bytes of an
//     input row.  It goes into LDS as it is, at dword row * 17 + t % 16.
//   * Drain: lane l of wave w owns the 4 x 4 byte block (rows 4 j .. 4 j + 3, dword i) with i = 4 w + l % 4, j = l / 4.  It reads its
//     four dwords, transposes the block in registers (eight v_perm_b32) and stores four dwords, one to each of four output rows:
//     the 16 lanes of one i are 64 contiguous bytes of an output row.
//   * LDS banks (ds_write_b32 and ds_read_b32: bank = dword address mod 32, lanes 0-31 and 32-63 are serviced apart).  The row
//     pitch is 17 dwords.  Fill, 32 lanes = rows r, r + 1, dwords 0..15: banks 17 r + c and 17 r + 17 + c, c = 0..15 -- 32 addresses
//     on 32 banks but for 17 r + 32 = 17 r (mod 32): one 2-way conflict, which a ds_write_b32 hides behind its data transfer.
//     Drain, 32 lanes = j0 .. j0 + 7, i0 .. i0 + 3, one a: address (4 j + a) * 17 + i = 68 j + 17 a + i = 4 j + i + const (mod 32):
//     j - j0 = 0..7 and i - i0 = 0..3 give 32 different banks.  No conflict.  (A pitch of 16 would put all j on one bank.)
//   * Edges: a dword of the fill that crosses the row end is gathered from the bytes that exist; rows below the plane are not loaded.
//     A 4 x 4 block of the drain with fewer than four input rows stores its bytes one by one; output rows beyond the plane (input
//     columns >= rw) are not stored.  Tight planes of any width: the dword accesses are unaligned.
// Bound: every input byte is read once and every output byte written once; nothing outside [0, rw * rh) of either plane is touched.
// One launch for Y, U, V and all members of a batch: workgroups are numbered luma first, blockIdx.z is the member.
#include "../../include/vp8hip_host.h"
#include "vp8hip_dev.h"

namespace vp8 {

namespace geometry {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef u32x4 u32x4_u __attribute__((aligned(1)));      // at any byte: one global_load / global_store_dwordx4 all the same
typedef uint32_t u32_u __attribute__((aligned(1)));
__device__ __forceinline__ u32x4 load16(const uint8_t *p) { return *reinterpret_cast<const u32x4_u *>(p); }
__device__ __forceinline__ void store16(uint8_t *p, u32x4 v) { *reinterpret_cast<u32x4_u *>(p) = v; }
__device__ __forceinline__ uint32_t load4(const uint8_t *p) { return *reinterpret_cast<const u32_u *>(p); }
__device__ __forceinline__ void store4(uint8_t *p, uint32_t v) { *reinterpret_cast<u32_u *>(p) = v; }
__device__ __forceinline__ uint32_t reverse4(uint32_t v) { return __builtin_amdgcn_perm(0u, v, 0x00010203u); }

constexpr int TILE = 64;            // input samples a side
constexpr int TILE_PITCH = 17;      // dwords between the tile's rows in LDS (16 hold samples)

struct WindowGeo {
    unsigned long long off[3];
    int pitch[3], row_bytes[3], rows[3], sx[3], units[3];      // sx: strips of 16 bytes per row; units = sx * rows
};

__device__ __forceinline__ void window_body(const PlanesItem &it, const WindowGeo &g) {
    int unit = (int)blockIdx.x * 256 + (int)threadIdx.x, p = 0;
    if (unit >= g.units[0]) {
        unit -= g.units[0];
        p = 1;
        if (unit >= g.units[1]) { unit -= g.units[1]; p = 2; }
    }
    if (unit >= g.units[p]) return;
    const int r = unit / g.sx[p], x0 = (unit - r * g.sx[p]) * 16, n = imin(16, g.row_bytes[p] - x0);
    const uint8_t *s = it.src[p] + (size_t)g.off[p] + (size_t)r * (size_t)g.pitch[p] + (size_t)x0;
    uint8_t *d = it.dst[p] + (size_t)r * (size_t)g.row_bytes[p] + (size_t)x0;
    if (n == 16) store16(d, load16(s));
    else
        for (int i = 0; i < n; ++i) d[i] = s[i];
}

// tx: tiles (transposing) or strips of 16 bytes (not) per input row; blocks: workgroups of the plane
struct OrientPlane { int rw, rh, tx, blocks; };
struct OrientGeo { OrientPlane y, c; int transpose, fx, fy; };

// turns 0 and 2: out(x, y) = in(fx ? rw - 1 - x : x, fy ? rh - 1 - y : y)
__device__ __forceinline__ void flip_unit(const uint8_t *src, uint8_t *dst, const OrientPlane &p, int fx, int fy, int unit) {
    if (unit >= p.tx * p.rh) return;
    const int y = unit / p.tx, x0 = (unit - y * p.tx) * 16, n = imin(16, p.rw - x0);
    const uint8_t *s = src + (size_t)(fy ? p.rh - 1 - y : y) * (size_t)p.rw;
    uint8_t *d = dst + (size_t)y * (size_t)p.rw + (size_t)x0;
    if (!fx) {
        s += x0;
        if (n == 16) store16(d, load16(s));
        else
            for (int i = 0; i < n; ++i) d[i] = s[i];
        return;
    }
    s += p.rw - x0 - n;      // out [x0, x0 + n) is in [rw - x0 - n, rw - x0), last byte first
    if (n == 16) {
        const u32x4 v = load16(s);
        store16(d, u32x4{reverse4(v.w), reverse4(v.z), reverse4(v.y), reverse4(v.x)});
    } else {
        for (int i = 0; i < n; ++i) d[i] = s[n - 1 - i];
    }
}

// turns 1 and 3: out(x, y) = in(fy ? rw - 1 - y : y, fx ? rh - 1 - x : x); out is rh wide and rw high
__device__ __forceinline__ void transpose_tile(const uint8_t *src, uint8_t *dst, const OrientPlane &p, int fx, int fy, int t, uint32_t *tile) {
    const int tid = (int)threadIdx.x;
    const int trow = t / p.tx, R0 = trow * TILE, C0 = (t - trow * p.tx) * TILE;
    {
        const int c = tid & 15, x = C0 + 4 * c;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int row = (tid >> 4) + 16 * k, r = R0 + row;
            uint32_t v = 0;
            if (r < p.rh) {
                const uint8_t *s = src + (size_t)r * (size_t)p.rw + (size_t)x;
                if (x + 4 <= p.rw) v = load4(s);
                else
                    for (int b = 0; x + b < p.rw; ++b) v |= (uint32_t)s[b] << (8 * b);
            }
            tile[row * TILE_PITCH + c] = v;
        }
    }
    __syncthreads();
    const int i = 4 * (tid >> 6) + (tid & 3), j = (tid & 63) >> 2;
    uint32_t d[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) d[a] = tile[(4 * j + a) * TILE_PITCH + i];
    // byte b of d[a] is in(C0 + 4 i + b, R0 + 4 j + a); byte a of o[b] is the same sample
    const uint32_t lo01 = __builtin_amdgcn_perm(d[1], d[0], 0x05010400u), hi01 = __builtin_amdgcn_perm(d[1], d[0], 0x07030602u);
    const uint32_t lo23 = __builtin_amdgcn_perm(d[3], d[2], 0x05010400u), hi23 = __builtin_amdgcn_perm(d[3], d[2], 0x07030602u);
    const uint32_t o[4] = {__builtin_amdgcn_perm(lo23, lo01, 0x05040100u), __builtin_amdgcn_perm(lo23, lo01, 0x07060302u),
                           __builtin_amdgcn_perm(hi23, hi01, 0x05040100u), __builtin_amdgcn_perm(hi23, hi01, 0x07060302u)};
    const int r0 = R0 + 4 * j, nv = imin(4, p.rh - r0);      // input rows of the block that exist
    if (nv <= 0) return;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const int cx = C0 + 4 * i + b;
        if (cx >= p.rw) continue;
        uint8_t *drow = dst + (size_t)(fy ? p.rw - 1 - cx : cx) * (size_t)p.rh;
        if (nv == 4) {
            if (fx) store4(drow + (p.rh - 4 - r0), reverse4(o[b]));
            else store4(drow + r0, o[b]);
        } else {
            for (int a = 0; a < nv; ++a) drow[fx ? p.rh - 1 - (r0 + a) : r0 + a] = (uint8_t)(o[b] >> (8 * a));
        }
    }
}

__device__ __forceinline__ void orient_body(const PlanesItem &it, const OrientGeo &g, uint32_t *tile) {
    int block = (int)blockIdx.x, plane = 0;      // (uniform in the workgroup: every lane reaches the barrier or none does)
    if (block >= g.y.blocks) {
        block -= g.y.blocks;
        plane = 1;
        if (block >= g.c.blocks) { block -= g.c.blocks; plane = 2; }
    }
    const OrientPlane &p = plane ? g.c : g.y;
    if (g.transpose) transpose_tile(it.src[plane], it.dst[plane], p, g.fx, g.fy, block, tile);
    else flip_unit(it.src[plane], it.dst[plane], p, g.fx, g.fy, block * 256 + (int)threadIdx.x);
}

}  // namespace geometry

static_assert(sizeof(BatchOf<PlanesItem>) + sizeof(geometry::WindowGeo) <= 4096, "a batch's argument blocks travel in the 4 KiB kernel-argument segment");
__global__ __launch_bounds__(256) void k_window_b(BatchOf<PlanesItem> b, geometry::WindowGeo g) { geometry::window_body(b.item[blockIdx.z], g); }

__global__ __launch_bounds__(256) void k_orient_b(BatchOf<PlanesItem> b, geometry::OrientGeo g) {
    __shared__ uint32_t tile[geometry::TILE * geometry::TILE_PITCH];
    geometry::orient_body(b.item[blockIdx.z], g, tile);
}

void launch_window_batch(hipStream_t s, const size_t offset[3], const int32_t pitch[3], const int32_t row_bytes[3], const int32_t rows[3],
                         const PlanesItem *items, int n) {
    if (n <= 0) return;
    BatchOf<PlanesItem> b;
    b.n = n;
    for (int i = 0; i < n; ++i) b.item[i] = items[i];
    geometry::WindowGeo g;
    long units = 0;
    for (int p = 0; p < 3; ++p) {
        g.off[p] = offset[p];
        g.pitch[p] = rows[p] ? pitch[p] : 0;
        g.row_bytes[p] = row_bytes[p];
        g.rows[p] = rows[p];
        g.sx[p] = (row_bytes[p] + 15) / 16;
        g.units[p] = g.sx[p] * rows[p];
        units += g.units[p];
    }
    if (!units) return;
    VP8_LAUNCH(k_window_b, dim3((unsigned)((units + 255) / 256), 1, n), dim3(256), 0, s, b, g);
}

void launch_orient_batch(hipStream_t s, int turns, int mirror, int raw_w, int raw_h, const PlanesItem *items, int n) {
    if (n <= 0 || (!turns && !mirror)) return;
    BatchOf<PlanesItem> b;
    b.n = n;
    for (int i = 0; i < n; ++i) b.item[i] = items[i];
    geometry::OrientGeo g;
    g.transpose = turns & 1;
    if (g.transpose) {      // turns 1: out(x, y) = s(y, rh - 1 - x); turns 3: out(x, y) = s(rw - 1 - y, x)
        g.fx = turns == 1;
        g.fy = turns == 1 ? mirror : !mirror;
    } else {                // turns 0: out(x, y) = s(x, y); turns 2: out(x, y) = s(rw - 1 - x, rh - 1 - y)
        g.fx = turns == 0 ? mirror : !mirror;
        g.fy = turns == 2;
    }
    auto plane = [&g](int rw, int rh) {
        geometry::OrientPlane p;
        p.rw = rw;
        p.rh = rh;
        if (g.transpose) {
            p.tx = (rw + geometry::TILE - 1) / geometry::TILE;
            p.blocks = p.tx * ((rh + geometry::TILE - 1) / geometry::TILE);
        } else {
            p.tx = (rw + 15) / 16;
            p.blocks = (p.tx * rh + 255) / 256;
        }
        return p;
    };
    g.y = plane(raw_w, raw_h);
    g.c = plane(raw_w / 2, raw_h / 2);
    VP8_LAUNCH(k_orient_b, dim3(g.y.blocks + 2 * g.c.blocks, 1, n), dim3(256), 0, s, b, g);
}

}  // namespace vp8
