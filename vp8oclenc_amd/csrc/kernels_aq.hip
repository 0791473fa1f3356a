// kernels_aq.hip -- the variance-adaptive segment map (vp8hip_set_segment_mode, mode 2).  The rule is stated bit for bit in
// include/vp8hip_host.h (vp8host_aq_segment_map is the same in plain C++); every number is an exact integer, so the order the workgroups
// finish in does not matter and a context alone or in a batch gives the same bytes.
//
// k_aq_map_b, once per frame taken in, at the end of the intake chain on its stream (behind the denoiser and the analysis launch: the
// luma as the searches will read it): ONE read of the coded luma, w h bytes, and one byte written per macroblock.  Memory-bound:
//   * the lanes are laid out as in k_analyse_src_b: a lane takes one 16-byte row of a macroblock (global_load_dwordx4), 16 lanes = one
//     DPP row = one macroblock, a wave = four horizontally adjacent macroblocks by 16 rows -- whole 64-byte runs of 16 rows -- and QPW such
//     quads per wave, all loads issued first;
//   * sum x is v_sad_u8 against zero and sum x^2 v_dot4_u32_u8 on the dwords as they came; a macroblock's sums are four DPP steps
//     inside the row; 256 sum x^2 <= 4 261 478 400 and the difference to (sum x)^2 fit 32 bits;
//   * the row's leader makes e (v_ffbh_u32 for the leading one) and stores it as a byte; a workgroup adds its e up in LDS and thread 0
//     adds the sum to the frame's word with one vector atomic (239 MBs < 2^32 for any frame this encoder takes).
// k_aq_seg_b, right behind it on the same stream: ONE workgroup per frame reads the word (and leaves zero: zero at rest), forms
// E = floor(sum / MBs) and turns e into the segment, sixteen macroblocks per lane and step, with three comparisons and no division.  The launch boundary is what makes every
// workgroup's e and the whole sum visible; the map is exact whatever ran first.
#include "vp8hip_dev.h"

namespace vp8 {

namespace aq {

constexpr int QPW = 4;      // quads (of four macroblocks) per wave

struct Geo { int mbw, mbh, qrow, nquads, mbs, W; };

constexpr int DPP_XOR1 = 0xB1, DPP_XOR2 = 0x4E, DPP_HALF_MIRROR = 0x141, DPP_MIRROR = 0x140;
template <int CTRL> __device__ __forceinline__ uint32_t dpp_add(uint32_t v) {
    return v + (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xf, 0xf, false);
}
__device__ __forceinline__ uint32_t row_sum(uint32_t v) {
    v = dpp_add<DPP_XOR1>(v);
    v = dpp_add<DPP_XOR2>(v);
    v = dpp_add<DPP_HALF_MIRROR>(v);
    return dpp_add<DPP_MIRROR>(v);
}
// e of the rule: log2(v + 1) in eighths, piecewise linear
__device__ __forceinline__ uint32_t log2_eighths(uint32_t v) {
    const uint32_t n = v + 1u;                       // (v <= 1 065 369 600: no wrap, n >= 1)
    const int p = 31 - __builtin_clz(n);
    const uint32_t frac = p >= 3 ? (n >> (p - 3)) & 7u : (n << (3 - p)) & 7u;
    return 8u * (uint32_t)p + frac;
}
// the rule's last line (vp8host_aq_segment) for the four e of a dword.  With d = e - E, floor(d / W) >= k is d >= k W, so
// clamp(2 + floor(d / W), 0, 3) = (d >= -W) + (d >= 0) + (d >= W): no division, and the rounding towards minus infinity is built in.
__device__ __forceinline__ uint32_t segments_of(uint32_t e4, int E, int W) {
    uint32_t m = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int d = (int)((e4 >> (8 * k)) & 0xffu) - E;
        m |= (uint32_t)((d >= -W) + (d >= 0) + (d >= W)) << (8 * k);
    }
    return m;
}

}  // namespace aq

static_assert(sizeof(BatchOf<AqItem>) + sizeof(aq::Geo) <= 4096, "a batch's argument blocks travel in the 4 KiB kernel-argument segment");

__global__ __launch_bounds__(256) void k_aq_map_b(BatchOf<AqItem> b, aq::Geo g) {
    using namespace aq;
    __shared__ uint32_t s_red[4];
    const AqItem &it = b.item[blockIdx.z];
    const int lane = (int)threadIdx.x & 63, wv = (int)threadIdx.x >> 6;
    const int wave = (int)blockIdx.x * 4 + wv;
    const int lmb = lane >> 4, lrow = lane & 15;      // macroblock of the quad, row of the macroblock
    uint4 X[QPW];
    int mbi[QPW];
    bool ok[QPW];
#pragma unroll
    for (int k = 0; k < QPW; ++k) {
        int q = wave * QPW + k;
        const bool live = q < g.nquads;
        q = live ? q : g.nquads - 1;      // (a wave's spare quads read the last quad again; their e is dropped, they store nothing)
        const int mby = q / g.qrow, mbx0 = (q - mby * g.qrow) * 4;
        ok[k] = live && mbx0 + lmb < g.mbw;
        const int lx = imin(mbx0 + lmb, g.mbw - 1), row = mby * 16 + lrow;
        mbi[k] = mby * g.mbw + lx;
        X[k] = *reinterpret_cast<const uint4 *>(it.cur.p + (ptrdiff_t)row * it.cur.stride + lx * 16);
    }
    uint32_t total = 0;      // the wave's sum of e, in the row leaders
#pragma unroll
    for (int k = 0; k < QPW; ++k) {
        // a lane: sum x <= 4080, sum x^2 <= 16 * 255^2; a macroblock: 65280 and 2^24 -- nothing wraps
        uint32_t xs = __builtin_amdgcn_sad_u8(X[k].x, 0u, 0u);
        xs = __builtin_amdgcn_sad_u8(X[k].y, 0u, xs);
        xs = __builtin_amdgcn_sad_u8(X[k].z, 0u, xs);
        xs = __builtin_amdgcn_sad_u8(X[k].w, 0u, xs);
        uint32_t xx = __builtin_amdgcn_udot4(X[k].x, X[k].x, 0u, false);
        xx = __builtin_amdgcn_udot4(X[k].y, X[k].y, xx, false);
        xx = __builtin_amdgcn_udot4(X[k].z, X[k].z, xx, false);
        xx = __builtin_amdgcn_udot4(X[k].w, X[k].w, xx, false);
        xs = row_sum(xs);
        xx = row_sum(xx);
        if (lrow == 0 && ok[k]) {
            const uint32_t e = log2_eighths(256u * xx - xs * xs);
            it.e[mbi[k]] = (uint8_t)e;
            total += e;
        }
    }
    total += __shfl_xor(total, 16, 64);
    total += __shfl_xor(total, 32, 64);
    if (lane == 0) s_red[wv] = total;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(it.sum, s_red[0] + s_red[1] + s_red[2] + s_red[3]);
}

__global__ __launch_bounds__(1024) void k_aq_seg_b(BatchOf<AqItem> b, aq::Geo g) {
    const AqItem &it = b.item[blockIdx.z];
    const uint32_t sum = __hip_atomic_load(it.sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();                        // every lane has the sum ...
    if (threadIdx.x == 0) *it.sum = 0u;     // ... zero at rest
    const int E = (int)(sum / (uint32_t)g.mbs);
    // (both arrays are whole multiples of 256 bytes long and 256-byte aligned, vp8hip_set_segment_mode: the spare bytes behind the
    // last macroblock are nobody's)
    const uint4 *e16 = reinterpret_cast<const uint4 *>(it.e);
    uint4 *m16 = reinterpret_cast<uint4 *>(it.map);
    for (int i = (int)threadIdx.x; i < (g.mbs + 15) / 16; i += 1024) {
        const uint4 e = e16[i];
        m16[i] = make_uint4(aq::segments_of(e.x, E, g.W), aq::segments_of(e.y, E, g.W), aq::segments_of(e.z, E, g.W), aq::segments_of(e.w, E, g.W));
    }
}

static aq::Geo aq_geo(const AqItem &it, int strength) {
    aq::Geo g;
    g.mbw = it.cur.w / 16;
    g.mbh = it.cur.h / 16;
    g.qrow = (g.mbw + 3) / 4;
    g.nquads = g.qrow * g.mbh;
    g.mbs = g.mbw * g.mbh;
    g.W = strength == 1 ? 24 : (strength == 2 ? 16 : 12);
    return g;
}

void launch_aq_map_batch(hipStream_t s, const AqItem *items, int n) {
    if (n <= 0) return;
    BatchOf<AqItem> b;
    b.n = n;
    for (int i = 0; i < n; ++i) b.item[i] = items[i];
    const aq::Geo g = aq_geo(items[0], 1);
    const int waves = (g.nquads + aq::QPW - 1) / aq::QPW;
    VP8_LAUNCH(k_aq_map_b, dim3((waves + 3) / 4, 1, n), dim3(256), 0, s, b, g);
}

void launch_aq_seg_batch(hipStream_t s, const AqItem *items, int n, int strength) {
    if (n <= 0) return;
    BatchOf<AqItem> b;
    b.n = n;
    for (int i = 0; i < n; ++i) b.item[i] = items[i];
    VP8_LAUNCH(k_aq_seg_b, dim3(1, 1, n), dim3(1024), 0, s, b, aq_geo(items[0], strength));
}

}  // namespace vp8
