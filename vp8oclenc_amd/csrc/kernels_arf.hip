// kernels_arf.hip -- the motion-compensated temporal filter that makes a hidden alternate reference frame (vp8hip_arf_filter_device).
// The reference never codes a frame it does not show; the rule is the project's own, after libvpx's ARNR filter, and is stated bit
// for bit in include/vp8hip_host.h (vp8host_arf_filter_frame is its plain C++ form).
//
// k_arf_filter_b, one launch per hidden frame: a wave takes one 16x16 luma tile of the centre frame with its two 8x8 chroma blocks, a
// workgroup four tiles.  Mapping:
//   * the centre tile is 64 dwords, one per lane (row lane >> 2, dword lane & 3), and stays in that register; the search reads it
//     through v_readlane with constant lane numbers, i.e. as scalar operands of v_sad_u8;
//   * per neighbour frame the wave stages the 31 x 31 search window (rows y0 - 8 .. y0 + 22, bytes x0 - 8 .. x0 + 23) in LDS as
//     31 rows of 8 dwords, every coordinate clamped into the picture: that IS the extension by the last column and row, and the
//     bytes left of or above the picture belong to candidates that do not count;
//   * the 256 candidates are four per lane: lane = 4 (dy + 8) + g holds dx + 8 = 4 g .. 4 g + 3, so per tile row it reads the five
//     dwords g .. g + 4 of window row dy + 8 + r once, and the four candidates are those dwords as they are and shifted by one,
//     two, three bytes (v_alignbyte): 5 LDS reads, 12 v_alignbyte and 16 v_sad_u8 per row and lane;
//   * LDS pitch 12 dwords: ds_read_b32 is served in halves of 32 lanes on 32 banks, a half reads 8 window rows x 4 consecutive
//     dwords, and 12 row mod 32 = 0, 12, 24, 4, 16, 28, 8, 20 for the eight rows: multiples of four, all different -- no two lanes of
//     a half share a bank (pitch 8 would be 4-way);
//   * the winner is the minimum of the 29-bit key SAD << 13 | (|dx| + |dy|) << 8 | (dy + 8) << 4 | (dx + 8) over the lane's four, then
//     over the wave: four DPP steps inside the rows of 16 (the idiom of kernels_s2.hip) and the four rows' values as scalars;
//   * SSE, block weight and the per-sample sums: every lane takes the winner's dword of ITS four samples out of the window, the
//     chroma lanes (plane lane >> 5, row (lane >> 2) & 7, two samples each) theirs from memory; count and acc stay in registers
//     across the loop over the frames;
//   * the division is include/vp8hip_host.h's reciprocal multiply, the reciprocals of 0 .. 255 in LDS (one division per thread).
//   * the (tile, frame) pairs by block weight: one 64-bit atomic per workgroup into one of 32 words (see the end of the kernel).
// A wave beyond the last tile works on the last tile again and stores nothing (barriers and DPP want every lane of every wave).
#include "../../include/vp8hip_host.h"
#include "vp8hip_dev.h"

namespace vp8 {

namespace arf {

constexpr int TILES = 4;                       // tiles, i.e. waves, per workgroup
constexpr int WIN_ROWS = 31, WIN_DW = 8;       // the search window: rows, dwords per row
constexpr int PITCH = 12;                      // dwords between the window's rows in LDS (see above)

constexpr int DPP_XOR1 = 0xB1, DPP_XOR2 = 0x4E, DPP_HALF_MIRROR = 0x141, DPP_MIRROR = 0x140;
template <int CTRL> __device__ __forceinline__ uint32_t dpp_min(uint32_t v) {
    const uint32_t o = (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)v, CTRL, 0xf, 0xf, false);
    return o < v ? o : v;
}
template <int CTRL> __device__ __forceinline__ uint32_t dpp_add(uint32_t v) {
    return v + (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xf, 0xf, false);
}
// over the wave, in scalars: the rows of 16 reduce with DPP, their four values meet through v_readlane
__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
    v = dpp_min<DPP_XOR1>(v);
    v = dpp_min<DPP_XOR2>(v);
    v = dpp_min<DPP_HALF_MIRROR>(v);
    v = dpp_min<DPP_MIRROR>(v);
    const uint32_t a = (uint32_t)__builtin_amdgcn_readlane((int)v, 0), b = (uint32_t)__builtin_amdgcn_readlane((int)v, 16);
    const uint32_t c = (uint32_t)__builtin_amdgcn_readlane((int)v, 32), d = (uint32_t)__builtin_amdgcn_readlane((int)v, 48);
    const uint32_t ab = a < b ? a : b, cd = c < d ? c : d;
    return ab < cd ? ab : cd;
}
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
    v = dpp_add<DPP_XOR1>(v);
    v = dpp_add<DPP_XOR2>(v);
    v = dpp_add<DPP_HALF_MIRROR>(v);
    v = dpp_add<DPP_MIRROR>(v);
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 0) + (uint32_t)__builtin_amdgcn_readlane((int)v, 16) +
           (uint32_t)__builtin_amdgcn_readlane((int)v, 32) + (uint32_t)__builtin_amdgcn_readlane((int)v, 48);
}

// sample (x, y) of a tight plane of w x h, the coordinates clamped into it: no read outside the plane, whatever x and y
__device__ __forceinline__ uint32_t at(const uint8_t *p, int w, int h, int x, int y) {
    return p[(size_t)iclamp(y, 0, h - 1) * (size_t)w + (size_t)iclamp(x, 0, w - 1)];
}
// the four samples (x .. x + 3, y) as a dword, first sample in the low byte
__device__ __forceinline__ uint32_t at4(const uint8_t *p, int w, int h, int x, int y) {
    if (x >= 0 && x + 3 < w) {
        uint32_t v;
        __builtin_memcpy(&v, p + (size_t)iclamp(y, 0, h - 1) * (size_t)w + (size_t)x, 4);
        return v;
    }
    return at(p, w, h, x, y) | at(p, w, h, x + 1, y) << 8 | at(p, w, h, x + 2, y) << 16 | at(p, w, h, x + 3, y) << 24;
}

// one sample's share of one frame: d = o - p, m = 16 - min((3 d d + r) >> s, 16), count += m bw, acc += m bw p
__device__ __forceinline__ void add_sample(uint32_t o, uint32_t p, int bw, int strength, int round, uint32_t &acc, uint32_t &count) {
    const int d = (int)o - (int)p;
    const int m = 16 - imin((3 * d * d + round) >> strength, 16);
    const uint32_t wgt = (uint32_t)(m * bw);
    count += wgt;
    acc += wgt * p;
}

__device__ __forceinline__ uint32_t rounded_quotient(uint32_t acc, uint32_t count, const uint32_t *recip) {
    return VP8HOST_ARF_DIVIDE(acc + count / 2, recip[count]);
}

}  // namespace arf

__global__ __launch_bounds__(256) void k_arf_filter_b(ArfItem it) {
    using namespace arf;
    __shared__ uint32_t s_win[TILES][WIN_ROWS * PITCH];
    __shared__ uint32_t s_recip[256];
    __shared__ uint32_t s_nbw[TILES];
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const int w = it.w, h = it.h, cw = w >> 1, ch = h >> 1;
    const int tw = (w + 15) >> 4, th = (h + 15) >> 4, tiles = tw * th;
    int tile = (int)blockIdx.x * TILES + wave;
    const bool live = tile < tiles;
    tile = live ? tile : tiles - 1;
    const int ty = tile / tw, tx = tile - ty * tw;
    const int x0 = tx * 16, y0 = ty * 16, cx0 = x0 >> 1, cy0 = y0 >> 1, We = tw * 16, He = th * 16;
    s_recip[threadIdx.x] = VP8HOST_ARF_RECIPROCAL(threadIdx.x ? threadIdx.x : 1u);
    uint32_t *win = s_win[wave];
    const uint8_t *const *C = it.src[it.centre];
    const int strength = it.strength, round = strength ? 1 << (strength - 1) : 0;

    // the lane's samples of the centre frame, and its sums with the centre's share (bw 2, d 0: m = 16)
    const int lrow = lane >> 2, lq = lane & 3;                                     // luma: row and dword of the tile
    const int cpl = lane >> 5, crow = (lane >> 2) & 7, ccol = (lane & 3) * 2;      // chroma: plane, row, first of two samples
    const uint32_t cd = at4(C[0], w, h, x0 + 4 * lq, y0 + lrow);
    const uint8_t *Cc = cpl ? C[2] : C[1];
    const uint32_t co[2] = {at(Cc, cw, ch, cx0 + ccol, cy0 + crow), at(Cc, cw, ch, cx0 + ccol + 1, cy0 + crow)};
    uint32_t acc[4], count[4], cacc[2], ccount[2];
#pragma unroll
    for (int b = 0; b < 4; ++b) { count[b] = 32u; acc[b] = 32u * (uint32_t)byte_of(cd, b); }
#pragma unroll
    for (int b = 0; b < 2; ++b) { ccount[b] = 32u; cacc[b] = 32u * co[b]; }
    uint32_t nbw[3] = {0u, 0u, 0u};

    // the lane's four candidates: dy + 8 = dyi, dx + 8 = 4 g + s
    const int dyi = lane >> 2, g = lane & 3;
    const bool dy_ok = y0 + dyi - 8 >= 0 && y0 + dyi - 8 + 16 <= He;
    const uint32_t *cand = win + dyi * PITCH + g;
    __syncthreads();      // (the reciprocals)
    for (int k = 0; k < it.n; ++k) {
        if (k == it.centre) continue;
        const uint8_t *const *F = it.src[k];
        __syncthreads();      // (the window of the frame before has been read)
#pragma unroll
        for (int i = lane; i < WIN_ROWS * WIN_DW; i += 64) {
            const int wr = i >> 3, d = i & 7;
            win[wr * PITCH + d] = at4(F[0], w, h, x0 - 8 + 4 * d, y0 - 8 + wr);
        }
        __syncthreads();
        uint32_t sad[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            uint32_t wv[5];
#pragma unroll
            for (int j = 0; j < 5; ++j) wv[j] = cand[r * PITCH + j];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t c = (uint32_t)__builtin_amdgcn_readlane((int)cd, r * 4 + j);
                sad[0] = __builtin_amdgcn_sad_u8(wv[j], c, sad[0]);
                sad[1] = __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(wv[j + 1], wv[j], 1u), c, sad[1]);
                sad[2] = __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(wv[j + 1], wv[j], 2u), c, sad[2]);
                sad[3] = __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(wv[j + 1], wv[j], 3u), c, sad[3]);
            }
        }
        uint32_t key = 0xFFFFFFFFu;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int dxi = 4 * g + s;
            const bool ok = dy_ok && x0 + dxi - 8 >= 0 && x0 + dxi - 8 + 16 <= We;
            const uint32_t ks = sad[s] << 13 | (uint32_t)(iabs(dxi - 8) + iabs(dyi - 8)) << 8 | (uint32_t)dyi << 4 | (uint32_t)dxi;
            key = ok && ks < key ? ks : key;
        }
        key = wave_min(key);      // (the zero vector always counts: a key is there)
        const int wdx = (int)(key & 15u), wdy = (int)((key >> 4) & 15u), dx = wdx - 8, dy = wdy - 8;
        // the winner's dword of the lane's four luma samples
        const uint32_t *pw = win + (wdy + lrow) * PITCH + (wdx >> 2) + lq;
        const uint32_t pd = __builtin_amdgcn_alignbyte(pw[1], pw[0], (uint32_t)(wdx & 3));
        uint32_t sq = 0u;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int d = byte_of(cd, b) - byte_of(pd, b);
            sq += (uint32_t)(d * d);
        }
        const uint32_t sse = wave_sum(sq);
        const int bw = sse < VP8HOST_ARF_THRESH_LOW ? 2 : (sse < VP8HOST_ARF_THRESH_HIGH ? 1 : 0);
        nbw[0] += bw == 0;
        nbw[1] += bw == 1;
        nbw[2] += bw == 2;
        if (bw) {      // (wave-uniform)
#pragma unroll
            for (int b = 0; b < 4; ++b) add_sample((uint32_t)byte_of(cd, b), (uint32_t)byte_of(pd, b), bw, strength, round, acc[b], count[b]);
            const uint8_t *Fc = cpl ? F[2] : F[1];
            const int ux = cx0 + ccol + (dx >> 1), uy = cy0 + crow + (dy >> 1);
#pragma unroll
            for (int b = 0; b < 2; ++b) add_sample(co[b], at(Fc, cw, ch, ux + b, uy), bw, strength, round, cacc[b], ccount[b]);
        }
    }
    {   // the block weights: the four waves' counts (at most 6 each, 8 bits a field) meet in LDS and leave as ONE 64-bit atomic per workgroup,
        // three fields of 21 bits, into one of ARF_WEIGHT_SLOTS words.  (A 32-bit atomic per wave and weight on three shared words was
        // 24 000 atomics on three addresses per 1080p frame: they queue up one behind the other, and that queue, not the search, was
        // three quarters of the launch's time.)
        if (lane == 0) s_nbw[wave] = live ? (nbw[0] | nbw[1] << 8 | nbw[2] << 16) : 0u;
        __syncthreads();
        if (threadIdx.x == 0) {
            const uint32_t p = s_nbw[0] + s_nbw[1] + s_nbw[2] + s_nbw[3];
            const unsigned long long f = (unsigned long long)(p & 255u) | (unsigned long long)((p >> 8) & 255u) << 21 | (unsigned long long)((p >> 16) & 255u) << 42;
            atomicAdd(it.weights + (blockIdx.x % ARF_WEIGHT_SLOTS), f);
        }
    }
    if (!live) return;
    {   // the lane's four luma samples, those of them inside the picture
        const int x = x0 + 4 * lq, y = y0 + lrow;
        uint32_t o = 0u;
#pragma unroll
        for (int b = 0; b < 4; ++b) o |= rounded_quotient(acc[b], count[b], s_recip) << (8 * b);
        uint8_t *d = it.dst[0] + (size_t)y * (size_t)w + (size_t)x;
        if (y < h && x + 3 < w) {
            __builtin_memcpy(d, &o, 4);
        } else if (y < h) {
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if (x + b < w) d[b] = (uint8_t)(o >> (8 * b));
        }
    }
    {   // its two chroma samples
        const int x = cx0 + ccol, y = cy0 + crow;
        uint8_t *d = (cpl ? it.dst[2] : it.dst[1]) + (size_t)y * (size_t)cw + (size_t)x;
#pragma unroll
        for (int b = 0; b < 2; ++b)
            if (y < ch && x + b < cw) d[b] = (uint8_t)rounded_quotient(cacc[b], ccount[b], s_recip);
    }
}

void launch_arf_filter(hipStream_t s, const ArfItem &item) {
    const int tiles = ((item.w + 15) / 16) * ((item.h + 15) / 16);
    VP8_LAUNCH(k_arf_filter_b, dim3((tiles + arf::TILES - 1) / arf::TILES), dim3(256), 0, s, item);
}

}  // namespace vp8
