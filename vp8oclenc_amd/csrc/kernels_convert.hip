// kernels_convert.hip -- source frames that are not tight 8-bit I420 (vp8hip_set_source_format): NV12, P010, 4:2:2, 4:4:4 and 10-bit
// planar (k_convert_b, below) and the packed YUY2, UYVY, BGRA and RGBA (k_convert_packed_b, further down) made 8-bit I420 of the same
// width and height, the first stage of the input side, in front of the pack (k_pack_b) or the
// scaler (k_scale_b).  The reference reads I420 and nothing else; the rule is the project's own and is stated bit for bit in
// include/vp8hip_host.h (vp8host_convert_frame is its plain C++ form): out = min(255, (S + (1 << (k - 1))) >> k) with S the sum of the
// 1, 2 or 4 source samples an output sample covers and k = log2(n) + depth - 8.
//
// k_convert_b writes tight planes into a staging buffer of the context; the pack or scale launch behind it on the same stream reads
// them as if the caller had handed in device I420, so padding, scaling, denoising and everything downstream see what they see today.
//
// Mapping (memory-bound: no LDS, 16-byte loads, 16-byte stores, everything in registers):
//   * a lane makes 16 adjacent output samples of one row of one plane -- or, for the interleaved chroma of NV12 / P010, 16 of U and
//     the 16 of V beside them -- and loads the 16 to 128 source bytes it needs for that itself (both rows of a vertical sum included);
//   * samples travel as packed 16-bit pairs: bytes are widened and interleaved chroma is taken apart with v_perm_b32, 10-bit words
//     are masked or shifted two at a time, sums (at most 4 * 1023) never carry between the halves, the clamp is v_pk_min_u16;
//   * tight planes of any even width: rows start at any byte, so loads and stores are unaligned vector accesses; the last unit of a
//     row that is no multiple of 16 wide is moved LEFT until it ends with the row (it rewrites a few samples of its neighbour with
//     the same values) instead of reading past the row -- or the plane -- end;
//   * rows of fewer than 16 outputs (pictures narrower than 16, or than 32 for chroma) have one unit that walks them sample by sample;
//   * one launch for Y, U, V and all members of a batch: units are numbered luma first, blockIdx.z is the member.
// The kernel is a template over (layout, depth): no format pays for another's branches.
#include "../../include/vp8hip_host.h"
#include "vp8hip_dev.h"

namespace vp8 {

namespace convert {

enum Layout { PLANAR420, NV, PLANAR422, PLANAR444 };      // NV: interleaved chroma, 4:2:0 (at 10 bits: P010, the value in a word's top bits)

struct Geo { int w, h, cw, ch, units_x, units_cx, luma_units, chroma_units; };      // chroma_units: per chroma job (NV: one job makes U and V)

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef u32x4 u32x4_u __attribute__((aligned(1)));      // at any byte: one global_load / global_store_dwordx4 all the same
__device__ __forceinline__ uint4 load16(const uint8_t *p) {
    const u32x4 v = *reinterpret_cast<const u32x4_u *>(p);
    return make_uint4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void store16(uint8_t *p, uint4 v) { *reinterpret_cast<u32x4_u *>(p) = u32x4{v.x, v.y, v.z, v.w}; }

// the two 10-bit values of a dword of two words, as a packed pair
template <bool TOP> __device__ __forceinline__ uint32_t ten(uint32_t d) { return (TOP ? d >> 6 : d) & 0x03ff03ffu; }

// Sixteen samples of one source row as eight packed pairs, added to acc.  HPAIR: every sample is the sum of two horizontally
// adjacent source samples (4:4:4 chroma), so the row segment is twice as long.
template <int DEPTH, bool TOP, bool HPAIR> __device__ __forceinline__ void row16(const uint8_t *p, uint32_t acc[8]) {
    if constexpr (DEPTH == 8 && !HPAIR) {
        const uint4 a = load16(p);
        const uint32_t d[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            acc[2 * i] += __builtin_amdgcn_perm(0u, d[i], 0x0c010c00u);
            acc[2 * i + 1] += __builtin_amdgcn_perm(0u, d[i], 0x0c030c02u);
        }
    } else if constexpr (DEPTH == 8) {
        const uint4 a = load16(p), b = load16(p + 16);
        const uint32_t d[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] += (d[i] & 0x00ff00ffu) + ((d[i] >> 8) & 0x00ff00ffu);
    } else if constexpr (!HPAIR) {
        const uint4 a = load16(p), b = load16(p + 16);
        const uint32_t d[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] += ten<TOP>(d[i]);
    } else {
        const uint4 a = load16(p), b = load16(p + 16), c = load16(p + 32), e = load16(p + 48);
        const uint32_t d[16] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w, e.x, e.y, e.z, e.w};
#pragma unroll
        for (int i = 0; i < 8; ++i) {      // a dword is one output sample's two words: (lo0, lo1) + (hi0, hi1)
            const uint32_t t0 = ten<TOP>(d[2 * i]), t1 = ten<TOP>(d[2 * i + 1]);
            acc[i] += __builtin_amdgcn_perm(t1, t0, 0x05040100u) + __builtin_amdgcn_perm(t1, t0, 0x07060302u);
        }
    }
}

// Sixteen interleaved (U, V) pairs of one row as eight packed pairs of U and eight of V
template <int DEPTH> __device__ __forceinline__ void row16_uv(const uint8_t *p, uint32_t u[8], uint32_t v[8]) {
    if constexpr (DEPTH == 8) {
        const uint4 a = load16(p), b = load16(p + 16);
        const uint32_t d[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
        for (int i = 0; i < 8; ++i) {      // U0 V0 U1 V1
            u[i] = __builtin_amdgcn_perm(0u, d[i], 0x0c020c00u);
            v[i] = __builtin_amdgcn_perm(0u, d[i], 0x0c030c01u);
        }
    } else {
        const uint4 a = load16(p), b = load16(p + 16), c = load16(p + 32), e = load16(p + 48);
        const uint32_t d[16] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w, e.x, e.y, e.z, e.w};
#pragma unroll
        for (int i = 0; i < 8; ++i) {      // a dword is (U word, V word)
            const uint32_t t0 = ten<true>(d[2 * i]), t1 = ten<true>(d[2 * i + 1]);
            u[i] = __builtin_amdgcn_perm(t1, t0, 0x05040100u);
            v[i] = __builtin_amdgcn_perm(t1, t0, 0x07060302u);
        }
    }
}

// eight packed pairs of sums -> sixteen output bytes: the one rounding step, the clamp (ten bits only: eight-bit sums cannot pass 255)
template <int K, bool CLAMP> __device__ __forceinline__ uint4 finish16(const uint32_t s[8]) {
    uint32_t o[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        uint32_t t = s[i];
        if (K > 0) t = ((t + (0x00010001u << (K > 0 ? K - 1 : 0))) >> K) & ((0xffffu >> K) * 0x00010001u);
        if (CLAMP) t = __builtin_bit_cast(uint32_t, __builtin_elementwise_min(__builtin_bit_cast(u16x2, t), u16x2{255, 255}));
        o[i] = t;
    }
    return make_uint4(__builtin_amdgcn_perm(o[1], o[0], 0x06040200u), __builtin_amdgcn_perm(o[3], o[2], 0x06040200u),
                      __builtin_amdgcn_perm(o[5], o[4], 0x06040200u), __builtin_amdgcn_perm(o[7], o[6], 0x06040200u));
}

// sample i of a plane at the format's depth, and the rule on one sum: the walk over rows too narrow for a unit of sixteen
template <int DEPTH, bool TOP> __device__ __forceinline__ int sample(const uint8_t *p, size_t i) {
    if (DEPTH == 8) return p[i];
    const int word = p[2 * i] | (p[2 * i + 1] << 8);
    return TOP ? word >> 6 : word & 1023;
}
template <int K> __device__ __forceinline__ uint8_t finish1(int S) {
    const int o = K > 0 ? (S + (1 << (K > 0 ? K - 1 : 0))) >> K : S;
    return (uint8_t)(o > 255 ? 255 : o);
}

template <int LAYOUT, int DEPTH> __device__ __forceinline__ void convert_body(const PlanesItem &it, const Geo &g) {
    constexpr bool TOP = LAYOUT == NV;                      // (of the two-plane formats only P010 has words)
    constexpr int B = DEPTH == 8 ? 1 : 2;                   // bytes per sample
    constexpr int KY = DEPTH - 8;
    constexpr int NX = LAYOUT == PLANAR444 ? 2 : 1, NY = (LAYOUT == PLANAR422 || LAYOUT == PLANAR444) ? 2 : 1;
    constexpr int KC = DEPTH - 8 + (NX == 2) + (NY == 2);
    int unit = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (unit < g.luma_units) {
        const int r = unit / g.units_x, ux = unit - r * g.units_x;
        uint8_t *out = it.dst[0] + (size_t)r * g.w;
        const uint8_t *src = it.src[0] + (size_t)r * g.w * B;
        if (g.w < 16) {
            for (int x = 0; x < g.w; ++x) out[x] = finish1<KY>(sample<DEPTH, TOP>(src, x));
            return;
        }
        const int x0 = min(ux * 16, g.w - 16);
        if (DEPTH == 8) {
            store16(out + x0, load16(src + x0));
        } else {
            uint32_t s[8] = {};
            row16<DEPTH, TOP, false>(src + (size_t)x0 * B, s);
            store16(out + x0, finish16<KY, true>(s));
        }
        return;
    }
    unit -= g.luma_units;
    int plane = 1;
    if (LAYOUT != NV && unit >= g.chroma_units) { unit -= g.chroma_units; plane = 2; }
    if (unit >= g.chroma_units) return;
    const int r = unit / g.units_cx, ux = unit - r * g.units_cx;
    const size_t pitch = (size_t)g.cw * NX;                 // samples (NV: pairs) per source chroma row
    if (LAYOUT == NV) {
        const uint8_t *src = it.src[1] + (size_t)r * pitch * 2 * B;
        uint8_t *ou = it.dst[1] + (size_t)r * g.cw, *ov = it.dst[2] + (size_t)r * g.cw;
        if (g.cw < 16) {
            for (int x = 0; x < g.cw; ++x) {
                ou[x] = finish1<KC>(sample<DEPTH, TOP>(src, 2 * x));
                ov[x] = finish1<KC>(sample<DEPTH, TOP>(src, 2 * x + 1));
            }
            return;
        }
        const int x0 = min(ux * 16, g.cw - 16);
        uint32_t u[8], v[8];
        row16_uv<DEPTH>(src + (size_t)x0 * 2 * B, u, v);
        store16(ou + x0, finish16<KC, DEPTH != 8>(u));
        store16(ov + x0, finish16<KC, DEPTH != 8>(v));
        return;
    }
    const uint8_t *src = it.src[plane] + (size_t)r * NY * pitch * B;
    uint8_t *out = it.dst[plane] + (size_t)r * g.cw;
    if (g.cw < 16) {
        for (int x = 0; x < g.cw; ++x) {
            int S = 0;
#pragma unroll
            for (int j = 0; j < NY; ++j)
#pragma unroll
                for (int i = 0; i < NX; ++i) S += sample<DEPTH, TOP>(src, (size_t)j * pitch + (size_t)(x * NX + i));
            out[x] = finish1<KC>(S);
        }
        return;
    }
    const int x0 = min(ux * 16, g.cw - 16);
    uint32_t s[8] = {};
#pragma unroll
    for (int j = 0; j < NY; ++j) row16<DEPTH, TOP, NX == 2>(src + ((size_t)j * pitch + (size_t)x0 * NX) * B, s);
    store16(out + x0, finish16<KC, DEPTH != 8>(s));
}

// ---- the packed family: YUY2, UYVY, BGRA, RGBA (one plane; the rule is include/vp8hip_host.h's) ---------------------------------------
// Mapping (memory-bound again: every source byte is loaded ONCE, by the lane that needs it; no LDS):
//   * a lane owns 16 pixels of TWO adjacent rows -- the rows of one chroma row -- loads both with 16-byte loads (4 per row for RGB, 2
//     for 4:2:2) and stores 2 x 16 luma bytes and 8 + 8 chroma bytes;
//   * RGB: luma is v_dot4_u32_u8 of the pixel's dword with the Y row as a dword of unsigned bytes (the alpha byte's coefficient is 0),
//     the rounding 128 in the accumulator, the shift a byte permute (the sum fits 16 bits), the offset added to four packed bytes at
//     once; chroma is v_dot4_i32_i8 of the pixel with its sign bits flipped (p - 128 as a signed byte) with the U or V row as signed
//     bytes, the four pixels of a block chained through the accumulator, which starts at 131072 + 512 + 4 * 128 * (the row's sum: each
//     of the four pixels is seen 128 too low; 0 for every table of the header).  BGRA and RGBA differ in where the host puts the coefficients in their dwords and in nothing else;
//   * 4:2:2: luma is a byte permute, chroma the rounded-up byte average of the two rows' dwords, (a | b) - (((a ^ b) >> 1) & 0x7f7f7f7f),
//     and two rounds of byte permutes; YUY2 and UYVY differ in the two selectors and in nothing else;
//   * so the matrix and the byte order are kernel ARGUMENTS of a few dwords: two code objects, not sixteen;
//   * edges as above: a row's last unit moves left, rows narrower than 16 pixels are walked pixel pair by pixel pair.
struct PackedArgs {
    int w, h, units_x, units;                 // units = units_x * h / 2
    uint32_t cy, cu, cv;                      // RGB: the rows as bytes at the pixel's byte positions
    uint32_t off4, bias_u, bias_v;            // the luma offset in all four bytes; the chroma accumulators' start
    uint32_t sel_y, sel_c;                    // 4:2:2: the luma bytes of two dwords; (U, U, V, V) of two dwords
    int shift_y, shift_u;                     // 4:2:2, the walk: bit positions of Y0 and U in a pair's dword (Y1 and V: 16 above)
};

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef u32x2 u32x2_u __attribute__((aligned(1)));
typedef uint32_t u32_u __attribute__((aligned(1)));
__device__ __forceinline__ void store8(uint8_t *p, uint32_t a, uint32_t b) { *reinterpret_cast<u32x2_u *>(p) = u32x2{a, b}; }
__device__ __forceinline__ uint32_t load4(const uint8_t *p) { return *reinterpret_cast<const u32_u *>(p); }

__device__ __forceinline__ uint32_t luma1(uint32_t px, const PackedArgs &g) { return __builtin_amdgcn_udot4(px, g.cy, 128u, false); }      // (Y - off) * 256 + fraction
__device__ __forceinline__ int chroma1(uint32_t px, uint32_t c, int acc) { return __builtin_amdgcn_sdot4((int)(px ^ 0x80808080u), (int)c, acc, false); }

// sixteen RGB pixels of one row -> sixteen luma bytes
__device__ __forceinline__ uint4 rgb_luma16(const uint32_t p[16], const PackedArgs &g) {
    uint32_t o[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t lo = __builtin_amdgcn_perm(luma1(p[4 * i + 1], g), luma1(p[4 * i], g), 0x0c0c0501u);
        const uint32_t hi = __builtin_amdgcn_perm(luma1(p[4 * i + 3], g), luma1(p[4 * i + 2], g), 0x0c0c0501u);
        o[i] = __builtin_amdgcn_perm(hi, lo, 0x05040100u) + g.off4;      // (no byte carries: Y <= 255)
    }
    return make_uint4(o[0], o[1], o[2], o[3]);
}

// the RGB pixels of one 2x2 block (a, b: the upper row's; c, d: the lower row's) -> four luma bytes, one U, one V: the walk's step
__device__ __forceinline__ void rgb_store_block(uint32_t a, uint32_t b, uint32_t c, uint32_t d, const PackedArgs &g, uint8_t *y0, uint8_t *y1,
                                                uint8_t *ou, uint8_t *ov) {
    const uint32_t off = g.off4 & 255u;
    y0[0] = (uint8_t)((luma1(a, g) >> 8) + off);
    y0[1] = (uint8_t)((luma1(b, g) >> 8) + off);
    y1[0] = (uint8_t)((luma1(c, g) >> 8) + off);
    y1[1] = (uint8_t)((luma1(d, g) >> 8) + off);
    *ou = (uint8_t)(chroma1(d, g.cu, chroma1(c, g.cu, chroma1(b, g.cu, chroma1(a, g.cu, (int)g.bias_u)))) >> 10);
    *ov = (uint8_t)(chroma1(d, g.cv, chroma1(c, g.cv, chroma1(b, g.cv, chroma1(a, g.cv, (int)g.bias_v)))) >> 10);
}

// sixteen RGB pixels of each of two rows (a: the upper, b: the lower) -> 2 x 16 luma bytes and 8 + 8 chroma bytes, stored
__device__ __forceinline__ void rgb_store16(const uint32_t a[16], const uint32_t b[16], const PackedArgs &g, uint8_t *y0, uint8_t *y1, uint8_t *ou,
                                            uint8_t *ov) {
    store16(y0, rgb_luma16(a, g));
    store16(y1, rgb_luma16(b, g));
    uint32_t u[2] = {}, v[2] = {};
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int su = chroma1(b[2 * i + 1], g.cu, chroma1(b[2 * i], g.cu, chroma1(a[2 * i + 1], g.cu, chroma1(a[2 * i], g.cu, (int)g.bias_u))));
        const int sv = chroma1(b[2 * i + 1], g.cv, chroma1(b[2 * i], g.cv, chroma1(a[2 * i + 1], g.cv, chroma1(a[2 * i], g.cv, (int)g.bias_v))));
        // (S + bias never negative and below 2^18: bits 10..17 are the byte)
        u[i >> 2] |= (((uint32_t)su >> 10) & 255u) << (8 * (i & 3));
        v[i >> 2] |= (((uint32_t)sv >> 10) & 255u) << (8 * (i & 3));
    }
    store8(ou, u[0], u[1]);
    store8(ov, v[0], v[1]);
}

template <bool RGB> __device__ __forceinline__ void packed_body(const PlanesItem &it, const PackedArgs &g) {
    constexpr int B = RGB ? 4 : 2;            // bytes per pixel
    const int unit = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (unit >= g.units) return;
    const int r = unit / g.units_x, ux = unit - r * g.units_x, cw = g.w >> 1;
    const size_t pitch = (size_t)g.w * B;
    const uint8_t *s0 = it.src[0] + (size_t)(2 * r) * pitch, *s1 = s0 + pitch;
    uint8_t *y0 = it.dst[0] + (size_t)(2 * r) * g.w, *y1 = y0 + g.w;
    uint8_t *ou = it.dst[1] + (size_t)r * cw, *ov = it.dst[2] + (size_t)r * cw;
    if (g.w < 16) {
        for (int x = 0; x < cw; ++x) {
            if constexpr (RGB) {
                rgb_store_block(load4(s0 + 8 * x), load4(s0 + 8 * x + 4), load4(s1 + 8 * x), load4(s1 + 8 * x + 4), g, y0 + 2 * x, y1 + 2 * x, ou + x, ov + x);
            } else {
                const uint32_t a = load4(s0 + 4 * x), b = load4(s1 + 4 * x);
                y0[2 * x] = (uint8_t)(a >> g.shift_y);
                y0[2 * x + 1] = (uint8_t)(a >> (g.shift_y + 16));
                y1[2 * x] = (uint8_t)(b >> g.shift_y);
                y1[2 * x + 1] = (uint8_t)(b >> (g.shift_y + 16));
                ou[x] = (uint8_t)((((a >> g.shift_u) & 255u) + ((b >> g.shift_u) & 255u) + 1u) >> 1);
                ov[x] = (uint8_t)((((a >> (g.shift_u + 16)) & 255u) + ((b >> (g.shift_u + 16)) & 255u) + 1u) >> 1);
            }
        }
        return;
    }
    const int x0 = min(ux * 16, g.w - 16);      // even: the widths are
    s0 += (size_t)x0 * B;
    s1 += (size_t)x0 * B;
    if constexpr (RGB) {
        uint32_t a[16], b[16];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint4 t = load16(s0 + 16 * i), q = load16(s1 + 16 * i);
            a[4 * i] = t.x; a[4 * i + 1] = t.y; a[4 * i + 2] = t.z; a[4 * i + 3] = t.w;
            b[4 * i] = q.x; b[4 * i + 1] = q.y; b[4 * i + 2] = q.z; b[4 * i + 3] = q.w;
        }
        rgb_store16(a, b, g, y0 + x0, y1 + x0, ou + (x0 >> 1), ov + (x0 >> 1));
    } else {
        const uint4 t0 = load16(s0), t1 = load16(s0 + 16), q0 = load16(s1), q1 = load16(s1 + 16);
        const uint32_t a[8] = {t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w}, b[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
        store16(y0 + x0, make_uint4(__builtin_amdgcn_perm(a[1], a[0], g.sel_y), __builtin_amdgcn_perm(a[3], a[2], g.sel_y),
                                    __builtin_amdgcn_perm(a[5], a[4], g.sel_y), __builtin_amdgcn_perm(a[7], a[6], g.sel_y)));
        store16(y1 + x0, make_uint4(__builtin_amdgcn_perm(b[1], b[0], g.sel_y), __builtin_amdgcn_perm(b[3], b[2], g.sel_y),
                                    __builtin_amdgcn_perm(b[5], b[4], g.sel_y), __builtin_amdgcn_perm(b[7], b[6], g.sel_y)));
        uint32_t c[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t m0 = (a[2 * i] | b[2 * i]) - (((a[2 * i] ^ b[2 * i]) >> 1) & 0x7f7f7f7fu);
            const uint32_t m1 = (a[2 * i + 1] | b[2 * i + 1]) - (((a[2 * i + 1] ^ b[2 * i + 1]) >> 1) & 0x7f7f7f7fu);
            c[i] = __builtin_amdgcn_perm(m1, m0, g.sel_c);      // U, U, V, V
        }
        store8(ou + (x0 >> 1), __builtin_amdgcn_perm(c[1], c[0], 0x05040100u), __builtin_amdgcn_perm(c[3], c[2], 0x05040100u));
        store8(ov + (x0 >> 1), __builtin_amdgcn_perm(c[1], c[0], 0x07060302u), __builtin_amdgcn_perm(c[3], c[2], 0x07060302u));
    }
}

// ---- HDR sources made SDR: P010 / I010 with a transfer in force (vp8hip_set_source_transfer; the rule is include/vp8hip_host.h's) -------
// k_tonemap_b stands where k_convert_b stands and writes the same tight I420.  The first kernel of the input side that is not data
// movement: about 70 vector instructions and 7 table lookups per pixel.
// Mapping:
//   * a lane owns 16 pixels of TWO adjacent rows, as packed_body does: it loads its 2 x 16 Y' words (2 x 2 loads of 16 bytes) and its 8
//     (Cb, Cr) pairs (P010: 2 loads of interleaved words, the value in the top ten bits; I010: one load per plane, the low ten bits)
//     once, forms the three chroma terms of R'G'B' once per 2x2 block, and stores 2 x 16 luma bytes and 8 + 8 chroma bytes;
//   * the four tables (TM_TABLE_BYTES, 40 KiB: lin and gain as dwords, lo and hi as bytes behind them, in the layout the setter uploads)
//     are copied into LDS at kernel start, 10 loads of 16 bytes per lane, and looked up there: a lookup's index is a pixel value, so
//     neighbouring lanes mostly hit neighbouring dwords (other banks) or the same one (a broadcast).  Dword entries for lin and gain:
//     16-bit entries could not hold 20 and 23 bits; lo and hi are one byte table of 8192 (the index picks the half), read with
//     ds_read_u8;
//   * a workgroup of 256 lanes makes 8192 pixels, about 2300 vector instructions per lane against the 20 of the copy; it reads 24 KiB of
//     frame and writes 12 KiB beside the 40 KiB of tables, which come from L2.  Four workgroups' tables fit a CU's 160 KiB, and 124
//     VGPRs allow the same four waves per SIMD.  No larger workgroup share: a 1920x1080 frame is 254 workgroups, one per CU;
//   * t * g is one 64-bit multiply-add (v_mad_u64_u32); the closing RGB -> YUV step is rgb_store16 on the (B, G, R, 0) dwords built in
//     registers: the byte dot products of the BGRA kernel, so the matrix is the same few argument dwords;
//   * edges as above: a row's last unit moves left, rows narrower than 16 pixels are walked 2x2 block by 2x2 block.
constexpr int TM_TABLE_BYTES = TONEMAP_TABLE_BYTES, TM_GAIN_AT = 4096, TM_C8_AT = 8192;      // dwords from the start: lin at 0, gain, then lo | hi as bytes

struct TmChroma { int r, g, b; };      // what (Cb, Cr) adds to 38295 y + 4096 for R', G' and B'
__device__ __forceinline__ TmChroma tm_chroma(int cb, int cr) {
    cb -= 512;
    cr -= 512;
    return TmChroma{55209 * cr, -6161 * cb - 21391 * cr, 70440 * cb};
}
__device__ __forceinline__ int tm_clamp12(int a) { return min(max(a, 0), 4095); }
__device__ __forceinline__ uint32_t tm_out8(int sum, uint32_t gain, const uint8_t *c8) {      // one component: a row of the primaries -> c8
    const uint32_t t = (uint32_t)max(sum >> 10, 0);
    const uint32_t o = min((uint32_t)(((uint64_t)t * gain + 524288u) >> 20), 65535u);      // (the product is below 2^44: 24 bits are left)
    return c8[o < 4096u ? o : 4096u + (o >> 4)];
}
// one pixel -> the dword of a BGRA pixel (alpha 0).  tab: the tables in LDS
__device__ __forceinline__ uint32_t tm_pixel(int y10, const TmChroma &c, const uint32_t *tab) {
    const uint8_t *c8 = reinterpret_cast<const uint8_t *>(tab + TM_C8_AT);
    const int yy = 38295 * (y10 - 64) + 4096;
    const int R1 = tm_clamp12((yy + c.r) >> 13), G1 = tm_clamp12((yy + c.g) >> 13), B1 = tm_clamp12((yy + c.b) >> 13);
    const uint32_t gain = tab[TM_GAIN_AT + max(R1, max(G1, B1))];
    // (lin is below 2^20: the mask changes no value and lets the nine products be full-rate 24-bit multiplies)
    const int aR = (int)(tab[R1] & 0xfffffu), aG = (int)(tab[G1] & 0xfffffu), aB = (int)(tab[B1] & 0xfffffu);
    const uint32_t R = tm_out8(1701 * aR - 602 * aG - 75 * aB + 512, gain, c8), G = tm_out8(-128 * aR + 1161 * aG - 9 * aB + 512, gain, c8),
                   B = tm_out8(-19 * aR - 103 * aG + 1146 * aB + 512, gain, c8);
    return B | (G << 8) | (R << 16);
}

template <bool TOP> __device__ __forceinline__ void tonemap_body(const PlanesItem &it, const PackedArgs &g, const uint32_t *tab) {
    const int unit = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (unit >= g.units) return;
    const int r = unit / g.units_x, ux = unit - r * g.units_x, cw = g.w >> 1;
    const size_t pitch = (size_t)g.w * 2;       // bytes of a luma row, and of P010's chroma row
    const uint8_t *s0 = it.src[0] + (size_t)(2 * r) * pitch, *s1 = s0 + pitch;
    const uint8_t *sc = it.src[1] + (size_t)r * (TOP ? pitch : (size_t)cw * 2);
    const uint8_t *sv = TOP ? sc : it.src[2] + (size_t)r * cw * 2;
    uint8_t *y0 = it.dst[0] + (size_t)(2 * r) * g.w, *y1 = y0 + g.w;
    uint8_t *ou = it.dst[1] + (size_t)r * cw, *ov = it.dst[2] + (size_t)r * cw;
    if (g.w < 16) {
        for (int x = 0; x < cw; ++x) {
            const TmChroma c = TOP ? tm_chroma(sample<10, true>(sc, 2 * x), sample<10, true>(sc, 2 * x + 1))
                                   : tm_chroma(sample<10, false>(sc, x), sample<10, false>(sv, x));
            rgb_store_block(tm_pixel(sample<10, TOP>(s0, 2 * x), c, tab), tm_pixel(sample<10, TOP>(s0, 2 * x + 1), c, tab),
                            tm_pixel(sample<10, TOP>(s1, 2 * x), c, tab), tm_pixel(sample<10, TOP>(s1, 2 * x + 1), c, tab), g, y0 + 2 * x, y1 + 2 * x,
                            ou + x, ov + x);
        }
        return;
    }
    const int x0 = min(ux * 16, g.w - 16);      // even: the widths are
    const uint4 t0 = load16(s0 + 2 * x0), t1 = load16(s0 + 2 * x0 + 16), q0 = load16(s1 + 2 * x0), q1 = load16(s1 + 2 * x0 + 16);
    const uint32_t ya[8] = {t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w}, yb[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
    uint32_t cc[8];      // the block's pair: Cb in the low half, Cr in the high half
    if constexpr (TOP) {
        const uint4 c0 = load16(sc + 2 * x0), c1 = load16(sc + 2 * x0 + 16);
        const uint32_t d[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
#pragma unroll
        for (int i = 0; i < 8; ++i) cc[i] = ten<true>(d[i]);
    } else {
        const uint4 c0 = load16(sc + x0), c1 = load16(sv + x0);      // eight words of each plane, at sample x0 / 2
        const uint32_t du[4] = {c0.x, c0.y, c0.z, c0.w}, dv[4] = {c1.x, c1.y, c1.z, c1.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t u2 = ten<false>(du[i]), v2 = ten<false>(dv[i]);
            cc[2 * i] = __builtin_amdgcn_perm(v2, u2, 0x05040100u);
            cc[2 * i + 1] = __builtin_amdgcn_perm(v2, u2, 0x07060302u);
        }
    }
    uint32_t a[16], b[16];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const TmChroma c = tm_chroma((int)(cc[i] & 0xffffu), (int)(cc[i] >> 16));
        const uint32_t p = ten<TOP>(ya[i]), q = ten<TOP>(yb[i]);
        a[2 * i] = tm_pixel((int)(p & 0xffffu), c, tab);
        a[2 * i + 1] = tm_pixel((int)(p >> 16), c, tab);
        b[2 * i] = tm_pixel((int)(q & 0xffffu), c, tab);
        b[2 * i + 1] = tm_pixel((int)(q >> 16), c, tab);
    }
    rgb_store16(a, b, g, y0 + x0, y1 + x0, ou + (x0 >> 1), ov + (x0 >> 1));
}

}  // namespace convert

static_assert(sizeof(BatchOf<PlanesItem>) + sizeof(convert::PackedArgs) + sizeof(void *) <= 4096, "a batch's argument blocks travel in the 4 KiB kernel-argument segment");
// tables: convert::TM_TABLE_BYTES of the context's device buffer (lin, gain, lo, hi end to end), 16-byte aligned
template <bool TOP> __global__ __launch_bounds__(256) void k_tonemap_b(BatchOf<PlanesItem> b, convert::PackedArgs g, const uint32_t *tables) {
    __shared__ convert::u32x4 tab[convert::TM_TABLE_BYTES / 16];
    for (int i = (int)threadIdx.x; i < convert::TM_TABLE_BYTES / 16; i += 256) tab[i] = reinterpret_cast<const convert::u32x4 *>(tables)[i];
    __syncthreads();      // (in front of every return: all 256 lanes arrive)
    convert::tonemap_body<TOP>(b.item[blockIdx.z], g, reinterpret_cast<const uint32_t *>(tab));
}

// the matrix of an RGB pixel's dword as the byte rows and accumulator starts of luma1 / chroma1 (format: BGRA or RGBA, where R and B sit)
static bool rgb_matrix_args(int format, int matrix, convert::PackedArgs &g) {
    int32_t c[9], off;
    if (vp8host_colour_coefficients(matrix, c, &off) != 0) return false;      // (vp8hip_set_source_colour refuses it: the caller fails the frame)
    const int at[3] = {format == VP8HOST_FORMAT_BGRA ? 16 : 0, 8, format == VP8HOST_FORMAT_BGRA ? 0 : 16};      // R, G, B in a pixel's dword
    int sum_u = 0, sum_v = 0;
    for (int k = 0; k < 3; ++k) {
        g.cy |= (uint32_t)(uint8_t)c[k] << at[k];
        g.cu |= (uint32_t)(uint8_t)(int8_t)c[3 + k] << at[k];
        g.cv |= (uint32_t)(uint8_t)(int8_t)c[6 + k] << at[k];
        sum_u += c[3 + k];
        sum_v += c[6 + k];
    }
    g.off4 = (uint32_t)off * 0x01010101u;
    g.bias_u = (uint32_t)(131072 + 512 + 4 * 128 * sum_u);      // the dot product sees p - 128, four pixels of it
    g.bias_v = (uint32_t)(131072 + 512 + 4 * 128 * sum_v);
    return true;
}

bool launch_tonemap_batch(hipStream_t s, int format, int matrix, int w, int h, const uint32_t *tables, const PlanesItem *items, int n) {
    if (n <= 0) return true;
    if ((format != VP8HOST_FORMAT_P010 && format != VP8HOST_FORMAT_I010) || !tables) return false;      // (the setters refuse it: the caller fails the frame)
    BatchOf<PlanesItem> b;
    b.n = n;
    for (int i = 0; i < n; ++i) b.item[i] = items[i];
    convert::PackedArgs g = {};
    g.w = w; g.h = h;
    g.units_x = w < 16 ? 1 : (w + 15) / 16;
    g.units = g.units_x * (h / 2);
    if (!rgb_matrix_args(VP8HOST_FORMAT_BGRA, matrix, g)) return false;      // (the pixel's dword is built as BGRA's)
    const dim3 grid((g.units + 255) / 256, 1, n), block(256);
    if (format == VP8HOST_FORMAT_P010) VP8_LAUNCH((k_tonemap_b<true>), grid, block, 0, s, b, g, tables);
    else VP8_LAUNCH((k_tonemap_b<false>), grid, block, 0, s, b, g, tables);
    return true;
}

static_assert(sizeof(BatchOf<PlanesItem>) + sizeof(convert::PackedArgs) <= 4096, "a batch's argument blocks travel in the 4 KiB kernel-argument segment");
template <bool RGB> __global__ __launch_bounds__(256) void k_convert_packed_b(BatchOf<PlanesItem> b, convert::PackedArgs g) {
    convert::packed_body<RGB>(b.item[blockIdx.z], g);
}

static bool launch_convert_packed(hipStream_t s, int format, int matrix, int w, int h, const BatchOf<PlanesItem> &b) {
    convert::PackedArgs g = {};
    g.w = w; g.h = h;
    g.units_x = w < 16 ? 1 : (w + 15) / 16;
    g.units = g.units_x * (h / 2);
    const bool rgb = format == VP8HOST_FORMAT_BGRA || format == VP8HOST_FORMAT_RGBA;
    if (rgb) {
        if (!rgb_matrix_args(format, matrix, g)) return false;
    } else {
        const bool yuy2 = format == VP8HOST_FORMAT_YUY2;
        g.sel_y = yuy2 ? 0x06040200u : 0x07050301u;
        g.sel_c = yuy2 ? 0x07030501u : 0x06020400u;
        g.shift_y = yuy2 ? 0 : 8;
        g.shift_u = yuy2 ? 8 : 0;
    }
    const dim3 grid((g.units + 255) / 256, 1, b.n), block(256);
    if (rgb) VP8_LAUNCH((k_convert_packed_b<true>), grid, block, 0, s, b, g);
    else VP8_LAUNCH((k_convert_packed_b<false>), grid, block, 0, s, b, g);
    return true;
}

static_assert(sizeof(BatchOf<PlanesItem>) + sizeof(convert::Geo) <= 4096, "a batch's argument blocks travel in the 4 KiB kernel-argument segment");
template <int LAYOUT, int DEPTH> __global__ __launch_bounds__(256) void k_convert_b(BatchOf<PlanesItem> b, convert::Geo g) {
    convert::convert_body<LAYOUT, DEPTH>(b.item[blockIdx.z], g);
}

bool launch_convert_batch(hipStream_t s, int format, int matrix, int w, int h, const PlanesItem *items, int n) {
    if (n <= 0 || format == VP8HOST_FORMAT_I420) return true;
    BatchOf<PlanesItem> b;
    b.n = n;
    for (int i = 0; i < n; ++i) b.item[i] = items[i];
    if (format >= VP8HOST_FORMAT_PACKED_FIRST && format < VP8HOST_FORMAT_PACKED_END) return launch_convert_packed(s, format, matrix, w, h, b);
    convert::Geo g;
    g.w = w; g.h = h; g.cw = w / 2; g.ch = h / 2;
    g.units_x = g.w < 16 ? 1 : (g.w + 15) / 16;
    g.units_cx = g.cw < 16 ? 1 : (g.cw + 15) / 16;
    g.luma_units = g.units_x * g.h;
    g.chroma_units = g.units_cx * g.ch;
    const bool nv = format == VP8HOST_FORMAT_NV12 || format == VP8HOST_FORMAT_P010;
    const int units = g.luma_units + (nv ? 1 : 2) * g.chroma_units;
    const dim3 grid((units + 255) / 256, 1, n), block(256);
    using namespace convert;
    switch (format) {
        case VP8HOST_FORMAT_NV12: VP8_LAUNCH((k_convert_b<NV, 8>), grid, block, 0, s, b, g); break;
        case VP8HOST_FORMAT_I422: VP8_LAUNCH((k_convert_b<PLANAR422, 8>), grid, block, 0, s, b, g); break;
        case VP8HOST_FORMAT_I444: VP8_LAUNCH((k_convert_b<PLANAR444, 8>), grid, block, 0, s, b, g); break;
        case VP8HOST_FORMAT_P010: VP8_LAUNCH((k_convert_b<NV, 10>), grid, block, 0, s, b, g); break;
        case VP8HOST_FORMAT_I010: VP8_LAUNCH((k_convert_b<PLANAR420, 10>), grid, block, 0, s, b, g); break;
        case VP8HOST_FORMAT_I210: VP8_LAUNCH((k_convert_b<PLANAR422, 10>), grid, block, 0, s, b, g); break;
        case VP8HOST_FORMAT_I410: VP8_LAUNCH((k_convert_b<PLANAR444, 10>), grid, block, 0, s, b, g); break;
        default: return false;      // (vp8hip_set_source_format refuses it)
    }
    return true;
}

}  // namespace vp8
