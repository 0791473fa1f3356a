// kernels_deinterlace.hip -- interlaced source frames made progressive (vp8hip_set_deinterlace), a stage of the input side between the
// format converter (k_convert_b) and the pack (k_pack_b) or the scaler (k_scale_b).  VP8 has no interlaced coding tools and the
// reference does not know what a field is; the rule is the project's own and is stated bit for bit in include/vp8hip_host.h
// (vp8host_deinterlace_frame is its plain C++ form): the rows of one field are kept, every sample of the other field's rows is the
// four-tap value s of the kept rows around it (mode 1) or, with the previous frame as received for a history, s clamped into
// [wv - m, wv + m] around the sample that came in (mode 2: what stands still is woven).
//
// k_deinterlace_b reads tight I420 of the incoming size (the caller's planes, the converter's staging buffer or an upload's) and writes
// tight I420 into a staging buffer of the context; the pack or scale launch behind it on the same stream reads that as if the caller
// had handed it in.  The history is the frame AS RECEIVED: the launch copies it verbatim into the one of the context's two history
// buffers it does not read (rows y - 1 and y + 1 of one lane are rows y of others, so nothing is updated in place).
//
// Mapping (memory-bound: no LDS, 16-byte loads and stores, everything in registers):
//   * a lane owns a strip 16 bytes wide and RP row pairs (2 RP rows) high of one plane; 64 consecutive lanes are 64 consecutive strips
//     of the same rows, 1 KiB per picture row and wave-instruction;
//   * it loads the RP + 3 kept rows its taps reach (the RP of its own pairs among them; every row index clamped, as the rule clamps
//     it) and, in mode 2, its RP missing rows and the 2 RP + 1 history rows under its missing rows and their vertical neighbours -- the
//     neighbours are the two inner taps -- all before the first is used (a 1080p frame is 380 waves: less than one per SIMD);
//   * bytes are widened to packed 16-bit pairs (v_perm_b32) once per row, the taps slide through those registers from pair to pair,
//     s, |cur - P|, the maximum and the clamp are packed 16-bit arithmetic (-510 <= 9 (a1 + a2) - (a0 + a3) + 8 <= 4598);
//   * tight planes of any width: rows start at any byte, so loads and stores are unaligned vector accesses; the last strip of a row
//     that is no multiple of 16 wide is moved LEFT until it ends with the row (it rewrites samples of its neighbour with the same
//     values and leaves them out of its count) instead of reading past the row -- or the plane -- end; a plane narrower than 16 has
//     one lane per RP row pairs that walks them sample by sample;
//   * one launch for Y, U, V and all members of a batch: units are numbered luma first, blockIdx.z is the member;
//   * the count of woven luma samples and the "last wave" ticket are ONE 64-bit vector atomic per wave (count << 32 | 1); the wave
//     that draws the last ticket writes the record into host memory, the sequence number last.
// Bound: every byte of the frame is read once from memory (the RP + 3 for RP kept rows and the one shared history row are the
// neighbour lanes' rows: cache hits), of the history once, and output and new history are written once: 4 frame sizes in mode 2
// (12.4 MB at 1920x1080), 1.5 in mode 1 (the missing rows are not read).
#include "../../include/vp8hip_host.h"
#include "vp8hip_dev.h"

namespace vp8 {

namespace deinterlace {

constexpr int RP = 4;      // row pairs per lane

struct PlaneGeo { int w, h, n, pairs, sx, units; };      // n: kept rows; pairs: ceil(h / 2); sx: strips per row
struct Geo { PlaneGeo y, c; int keep, waves, missing; };

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef u32x4 u32x4_u __attribute__((aligned(1)));      // at any byte: one global_load / global_store_dwordx4 all the same
__device__ __forceinline__ uint4 load16(const uint8_t *p) {
    const u32x4 v = *reinterpret_cast<const u32x4_u *>(p);
    return make_uint4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void store16(uint8_t *p, uint4 v) { *reinterpret_cast<u32x4_u *>(p) = u32x4{v.x, v.y, v.z, v.w}; }

struct Row { s16x2 p[8]; };      // sixteen samples as packed pairs: p[2 d] = bytes (0, 1) of dword d, p[2 d + 1] = bytes (2, 3)
__device__ __forceinline__ Row widen(uint4 v) {
    const uint32_t d[4] = {v.x, v.y, v.z, v.w};
    Row r;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        r.p[2 * i] = as_s16x2(__builtin_amdgcn_perm(0u, d[i], 0x0c010c00u));
        r.p[2 * i + 1] = as_s16x2(__builtin_amdgcn_perm(0u, d[i], 0x0c030c02u));
    }
    return r;
}
__device__ __forceinline__ uint4 narrow(const Row &r) {      // (every half holds a byte)
    return make_uint4(__builtin_amdgcn_perm(as_u32(r.p[1]), as_u32(r.p[0]), 0x06040200u), __builtin_amdgcn_perm(as_u32(r.p[3]), as_u32(r.p[2]), 0x06040200u),
                      __builtin_amdgcn_perm(as_u32(r.p[5]), as_u32(r.p[4]), 0x06040200u), __builtin_amdgcn_perm(as_u32(r.p[7]), as_u32(r.p[6]), 0x06040200u));
}
__device__ __forceinline__ Row absdiff(const Row &a, const Row &b) {
    Row r;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const s16x2 d = a.p[i] - b.p[i];
        r.p[i] = __builtin_elementwise_max(d, -d);
    }
    return r;
}
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// One strip of a plane at least 16 wide.  Returns the samples of its missing rows that were woven (HIST only; its own samples only).
template <int KEEP, bool HIST>
__device__ __forceinline__ unsigned strip_unit(const uint8_t *src, const uint8_t *hist, uint8_t *dst, uint8_t *kh, const PlaneGeo &g, int seg, int strip) {
    const int x0 = imin(strip * 16, g.w - 16), skip = strip * 16 - x0;      // bytes [0, skip) of the strip are the neighbour's
    const int jA = seg * RP;
    const size_t w = (size_t)g.w;
    // kept rows K[jA - KEEP - 1 + i], i = 0 .. RP + 2: pair q's taps are i = q .. q + 3, its own kept row is i = q + KEEP + 1, the
    // vertical neighbours of its missing row are i = q + 1 and q + 2 (where the rule clamps a neighbour onto the missing row itself,
    // the clamped tap is the OTHER neighbour: the maximum is the same)
    size_t ok[RP + 3], om[RP];
    uint4 K[RP + 3], M[RP], HK[RP + 1], HM[RP];
#pragma unroll
    for (int i = 0; i < RP + 3; ++i) {
        ok[i] = (size_t)(2 * clampi(jA - KEEP - 1 + i, 0, g.n - 1) + KEEP) * w + (size_t)x0;
        K[i] = load16(src + ok[i]);
    }
#pragma unroll
    for (int q = 0; q < RP; ++q) {      // (mode 1 never reads the missing rows)
        om[q] = (size_t)imin(2 * (jA + q) + 1 - KEEP, g.h - 1) * w + (size_t)x0;
        if (HIST || kh) M[q] = load16(src + om[q]);
    }
    if constexpr (HIST) {
#pragma unroll
        for (int i = 0; i < RP + 1; ++i) HK[i] = load16(hist + ok[i + 1]);
#pragma unroll
        for (int q = 0; q < RP; ++q) HM[q] = load16(hist + om[q]);
    }
    // the kept rows pass through, and every row as received is the next frame's history
#pragma unroll
    for (int q = 0; q < RP; ++q) {
        const int yk = 2 * (jA + q) + KEEP, ym = 2 * (jA + q) + 1 - KEEP;
        if (yk < g.h) {
            store16(dst + ok[q + KEEP + 1], K[q + KEEP + 1]);
            if (kh) store16(kh + ok[q + KEEP + 1], K[q + KEEP + 1]);
        }
        if (kh && ym < g.h) store16(kh + om[q], M[q]);
    }
    Row k[RP + 3], dk[RP + 1];
#pragma unroll
    for (int i = 0; i < RP + 3; ++i) k[i] = widen(K[i]);
    if constexpr (HIST) {
#pragma unroll
        for (int i = 0; i < RP + 1; ++i) dk[i] = absdiff(k[i + 1], widen(HK[i]));
    }
    // (the 1s pass through an empty asm: min(x, 1) with a constant hipcc can see becomes x != 0, which it scalarises -- kernels_denoise.hip)
    uint32_t ones = 0x00010001u;
    asm("" : "+s"(ones));
    const u16x2 one = __builtin_bit_cast(u16x2, ones);
    u16x2 mask[8], ne = {0, 0};
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int b = 4 * (i >> 1) + 2 * (i & 1);
        mask[i] = u16x2{(unsigned short)(b >= skip), (unsigned short)(b + 1 >= skip)};
    }
    int rows = 0;
#pragma unroll
    for (int q = 0; q < RP; ++q) {
        const int ym = 2 * (jA + q) + 1 - KEEP;
        if (ym >= g.h) continue;
        ++rows;
        Row o, wv, dm;
        if constexpr (HIST) {
            wv = widen(M[q]);
            dm = absdiff(wv, widen(HM[q]));
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const s16x2 t = (k[q + 1].p[i] + k[q + 2].p[i]) * s16x2{9, 9} - (k[q].p[i] + k[q + 3].p[i]) + s16x2{8, 8};
            s16x2 s = __builtin_elementwise_min(__builtin_elementwise_max(t >> s16x2{4, 4}, s16x2{0, 0}), s16x2{255, 255});
            if constexpr (HIST) {
                const s16x2 m = __builtin_elementwise_max(dm.p[i], __builtin_elementwise_max(dk[q].p[i], dk[q + 1].p[i]));
                s = __builtin_elementwise_min(__builtin_elementwise_max(s, wv.p[i] - m), wv.p[i] + m);      // between s and wv: a byte
                ne += __builtin_elementwise_min(__builtin_bit_cast(u16x2, s ^ wv.p[i]), one) & mask[i];
            }
            o.p[i] = s;
        }
        store16(dst + om[q], narrow(o));
    }
    return HIST ? (unsigned)(rows * (16 - skip)) - ((unsigned)ne.x + (unsigned)ne.y) : 0u;
}

// RP row pairs of a plane narrower than 16, sample by sample (the rule as include/vp8hip_host.h writes it)
__device__ __forceinline__ unsigned narrow_unit(const uint8_t *src, const uint8_t *hist, uint8_t *dst, uint8_t *kh, const PlaneGeo &g, int keep, int seg) {
    unsigned woven = 0;
    for (int j = seg * RP; j < imin(seg * RP + RP, g.pairs); ++j) {
        const int yk = 2 * j + keep, ym = 2 * j + 1 - keep;
        if (yk < g.h)
            for (int x = 0; x < g.w; ++x) {
                const uint8_t v = src[(size_t)yk * g.w + x];
                dst[(size_t)yk * g.w + x] = v;
                if (kh) kh[(size_t)yk * g.w + x] = v;
            }
        if (ym >= g.h) continue;
        const int j0 = j - keep;      // floor((ym - 1 - keep) / 2)
        const uint8_t *a0 = src + (size_t)(2 * clampi(j0 - 1, 0, g.n - 1) + keep) * g.w, *a1 = src + (size_t)(2 * clampi(j0, 0, g.n - 1) + keep) * g.w;
        const uint8_t *a2 = src + (size_t)(2 * clampi(j0 + 1, 0, g.n - 1) + keep) * g.w, *a3 = src + (size_t)(2 * clampi(j0 + 2, 0, g.n - 1) + keep) * g.w;
        const size_t om = (size_t)ym * g.w, oa = (size_t)(ym > 0 ? ym - 1 : 0) * g.w, ob = (size_t)imin(ym + 1, g.h - 1) * g.w;
        for (int x = 0; x < g.w; ++x) {
            int s = clampi((-(int)a0[x] + 9 * (int)a1[x] + 9 * (int)a2[x] - (int)a3[x] + 8) >> 4, 0, 255);
            const int wv = src[om + x];
            if (hist) {
                const int m = imax(iabs(wv - (int)hist[om + x]), imax(iabs((int)src[oa + x] - (int)hist[oa + x]), iabs((int)src[ob + x] - (int)hist[ob + x])));
                s = clampi(s, wv - m, wv + m);
                woven += s == wv;
            }
            dst[om + x] = (uint8_t)s;
            if (kh) kh[om + x] = (uint8_t)wv;
        }
    }
    return woven;
}

template <int KEEP> __device__ __forceinline__ void deinterlace_body(const DeinterlaceItem &it, const Geo &g) {
    int unit = (int)blockIdx.x * 256 + (int)threadIdx.x, plane = 0;
    if (unit >= g.y.units) {
        unit -= g.y.units;
        plane = 1;
        if (unit >= g.c.units) { unit -= g.c.units; plane = 2; }
    }
    const PlaneGeo &p = plane ? g.c : g.y;
    unsigned woven = 0;
    if (unit < p.units) {
        const uint8_t *src = it.src[plane], *hist = it.hist[plane];
        uint8_t *dst = it.dst[plane], *kh = it.keep_hist[plane];
        const int seg = unit / p.sx, strip = unit - seg * p.sx;
        if (p.w < 16) woven = narrow_unit(src, hist, dst, kh, p, KEEP, seg);
        else if (hist) woven = strip_unit<KEEP, true>(src, hist, dst, kh, p, seg, strip);
        else (void)strip_unit<KEEP, false>(src, hist, dst, kh, p, seg, strip);
        if (plane) woven = 0;      // the record counts luma
    }
#pragma unroll
    for (int o = 32; o; o >>= 1) woven += (unsigned)__shfl_xor((int)woven, o);
    if (((int)threadIdx.x & 63) != 0) return;
    // count and ticket in one 64-bit atomic: nothing but the word itself passes between the waves, so no fence
    const unsigned long long old = atomicAdd(it.word, ((unsigned long long)woven << 32) | 1ull);
    if ((unsigned)(old & 0xffffffffull) + 1u != (unsigned)g.waves) return;
    atomicExch(it.word, 0ull);        // zero at rest
    it.host->frame_number = it.frame_number;
    it.host->woven = (int32_t)((old >> 32) + woven);
    it.host->missing = g.missing;
    __hip_atomic_store(&it.host->seq, it.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);   // the host polls this word
}

}  // namespace deinterlace

static_assert(sizeof(BatchOf<DeinterlaceItem>) + sizeof(deinterlace::Geo) <= 4096, "a batch's argument blocks travel in the 4 KiB kernel-argument segment");
template <int KEEP> __global__ __launch_bounds__(256) void k_deinterlace_b(BatchOf<DeinterlaceItem> b, deinterlace::Geo g) {
    deinterlace::deinterlace_body<KEEP>(b.item[blockIdx.z], g);
}

void launch_deinterlace_batch(hipStream_t s, int w, int h, int keep, const DeinterlaceItem *items, int n) {
    if (n <= 0) return;
    BatchOf<DeinterlaceItem> b;
    b.n = n;
    for (int i = 0; i < n; ++i) b.item[i] = items[i];
    deinterlace::Geo g;
    auto plane = [keep](int pw, int ph) {
        deinterlace::PlaneGeo p;
        p.w = pw;
        p.h = ph;
        p.n = (ph - keep + 1) / 2;
        p.pairs = (ph + 1) / 2;
        p.sx = pw < 16 ? 1 : (pw + 15) / 16;
        p.units = p.sx * ((p.pairs + deinterlace::RP - 1) / deinterlace::RP);
        return p;
    };
    g.y = plane(w, h);
    g.c = plane(w / 2, h / 2);
    g.keep = keep;
    g.missing = w * (h / 2);
    const int blocks = (g.y.units + 2 * g.c.units + 255) / 256;
    g.waves = blocks * 4;
    if (keep) VP8_LAUNCH(k_deinterlace_b<1>, dim3(blocks, 1, n), dim3(256), 0, s, b, g);
    else VP8_LAUNCH(k_deinterlace_b<0>, dim3(blocks, 1, n), dim3(256), 0, s, b, g);
}

}  // namespace vp8
