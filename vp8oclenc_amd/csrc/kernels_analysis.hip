// kernels_analysis.hip -- the frame analysis record (vp8hip_set_analysis): what a rate controller measures, on the device, with nobody
// waiting.  Both rules are stated bit for bit in include/vp8hip_host.h (vp8host_analyse_luma is the source side in plain C++); every
// sum is an exact integer, so the order the workgroups finish in does not matter and a context measured alone or in a batch gives
// the same bits.
//
// k_analyse_src_b, once per frame taken in, behind the convert / pack / scale / denoise launches on their stream: ONE pass over the
// coded luma X against the history plane P (the luma of the previous frame taken in, tight, the context's own), and the same lane
// writes X into the history: 3 w h bytes of traffic (X read, P read, P written; 2 w h without a history), nothing else.  Memory-bound:
//   * a lane takes one 16-byte row of a macroblock of X and of P (global_load_dwordx4 each) and stores the 16 bytes of X into P; 16 lanes
//     = one DPP row = one macroblock, a wave = four horizontally adjacent macroblocks, QPW such quads per wave, all loads issued first;
//   * sum x and sum |x - p| are v_sad_u8 on the dwords as they came, sum x^2, sum p^2 and sum x p are v_dot4_u32_u8, and
//     sum (x - p)^2 = sum x^2 + sum p^2 - 2 sum x p; a lane's sums fit 32 bits with room (16 samples);
//   * the macroblock's sums are four DPP steps inside the row (sum x and the SAD share a register: both stay below 2^16 per
//     macroblock); (sum x)^2 is formed per macroblock, in 64 bits, as the rule demands;
//   * a workgroup adds its four waves up in LDS and thread 0 adds the four frame sums to `acc` with 64-bit atomics, then draws a
//     ticket; the workgroup with the last ticket takes the sums (leaving zeros) and writes the record into host memory, seq last;
//   * no history (first frame, after a restart): a template branch, uniform per member, that reads X only and stores it.
// k_analyse_mb_b, behind the loop filter of every coding attempt on the filter's stream: one workgroup per frame walks the
// per-macroblock arrays (a few dozen bytes per macroblock), sums in registers, shuffles, LDS, and writes the record, seq last.
#include "vp8hip_dev.h"

namespace vp8 {

namespace analysis {

constexpr int QPW = 4;      // quads (of four macroblocks) per wave

struct Geo { int mbw, mbh, qrow, nquads, blocks; };

// DPP controls as in kernels_denoise.hip: applied in this order to a sum they are the butterfly over 2, 4, 8, 16 lanes of a row
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
__device__ __forceinline__ uint32_t sad16(const uint4 &a, const uint4 &b) {
    uint32_t s = __builtin_amdgcn_sad_u8(a.x, b.x, 0u);
    s = __builtin_amdgcn_sad_u8(a.y, b.y, s);
    s = __builtin_amdgcn_sad_u8(a.z, b.z, s);
    return __builtin_amdgcn_sad_u8(a.w, b.w, s);
}
__device__ __forceinline__ uint32_t dot16(const uint4 &a, const uint4 &b) {
    uint32_t s = __builtin_amdgcn_udot4(a.x, b.x, 0u, false);
    s = __builtin_amdgcn_udot4(a.y, b.y, s, false);
    s = __builtin_amdgcn_udot4(a.z, b.z, s, false);
    return __builtin_amdgcn_udot4(a.w, b.w, s, false);
}
// the four row leaders (lanes 0, 16, 32, 48) hold a value, every other lane 0: lane 0 gets the sum
__device__ __forceinline__ unsigned long long leaders_sum(unsigned long long v) {
    v += __shfl_xor(v, 16, 64);
    return v + __shfl_xor(v, 32, 64);
}

template <bool PREV> __device__ __forceinline__ void src_body(const AnalysisSrcItem &it, const Geo &g) {
    __shared__ unsigned long long s_red[4][4];
    const int lane = (int)threadIdx.x & 63, wv = (int)threadIdx.x >> 6;
    const int wave = (int)blockIdx.x * 4 + wv;
    const int lmb = lane >> 4, lrow = lane & 15;      // macroblock of the quad, row of the macroblock
    const int hstride = g.mbw * 16;
    const uint4 zero = {0u, 0u, 0u, 0u};
    uint4 X[QPW], P[QPW];
    uint8_t *hp[QPW];
    bool ok[QPW];
#pragma unroll
    for (int k = 0; k < QPW; ++k) {
        int q = wave * QPW + k;
        const bool live = q < g.nquads;
        q = live ? q : g.nquads - 1;      // (a wave's spare quads read the last quad again; their sums are dropped, they store nothing)
        const int mby = q / g.qrow, mbx0 = (q - mby * g.qrow) * 4;
        ok[k] = live && mbx0 + lmb < g.mbw;
        const int lx = imin(mbx0 + lmb, g.mbw - 1), row = mby * 16 + lrow;
        X[k] = *reinterpret_cast<const uint4 *>(it.cur.p + (ptrdiff_t)row * it.cur.stride + lx * 16);
        hp[k] = it.hist + (ptrdiff_t)row * hstride + lx * 16;
        P[k] = PREV ? *reinterpret_cast<const uint4 *>(hp[k]) : zero;
    }
    unsigned long long spatial = 0, sse = 0, sad = 0, stat = 0;      // the wave's sums, in the row leaders
#pragma unroll
    for (int k = 0; k < QPW; ++k) {
        if (ok[k]) *reinterpret_cast<uint4 *>(hp[k]) = X[k];          // the history from now on
        // a lane: sum x <= 4080, SAD <= 4080, the dot products <= 16 * 255^2; a macroblock: 65280, 65280, 2^24 -- neither half of
        // the shared register carries, nothing wraps
        uint32_t xs = sad16(X[k], zero), xx = dot16(X[k], X[k]), d1 = 0, d2 = 0;
        if (PREV) {
            d1 = sad16(X[k], P[k]);
            d2 = xx + dot16(P[k], P[k]) - 2u * dot16(X[k], P[k]);
        }
        const uint32_t both = row_sum(xs | (d1 << 16));
        xx = row_sum(xx);
        if (PREV) d2 = row_sum(d2);
        if (lrow == 0 && ok[k]) {
            const unsigned long long sx = both & 0xffffu;
            spatial += 256ull * xx - sx * sx;
            if (PREV) {
                sse += d2;
                sad += both >> 16;
                stat += (both >> 16) == 0u;
            }
        }
    }
    spatial = leaders_sum(spatial);
    if (PREV) {
        sse = leaders_sum(sse);
        sad = leaders_sum(sad);
        stat = leaders_sum(stat);
    }
    if (lane == 0) {
        s_red[wv][0] = spatial;
        s_red[wv][1] = sse;
        s_red[wv][2] = sad;
        s_red[wv][3] = stat;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    unsigned long long t[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) t[i] = s_red[0][i] + s_red[1][i] + s_red[2][i] + s_red[3][i];
    atomicAdd(it.acc + 0, t[0]);
    if (PREV) {
        atomicAdd(it.acc + 1, t[1]);
        atomicAdd(it.acc + 2, t[2]);
        atomicAdd(it.acc + 3, t[3]);
    }
    __threadfence();      // the sums before the ticket
    if (atomicAdd(it.acc + 4, 1ull) + 1ull != (unsigned long long)g.blocks) return;
    __threadfence();
#pragma unroll
    for (int i = 0; i < 4; ++i) t[i] = atomicExch(it.acc + i, 0ull);      // zero at rest
    atomicExch(it.acc + 4, 0ull);
    it.host->spatial = t[0];
    it.host->sse = t[1];
    it.host->sad = t[2];
    it.host->static_mbs = (int32_t)t[3];
    it.host->have_prev = PREV ? 1 : 0;
    it.host->frame_number = it.frame_number;
    __hip_atomic_store(&it.host->seq, it.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);   // the host polls this word
}

template <typename T> __device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

constexpr int NCNT = 11, NBIG = 6;
enum { C_INTRA, C_SPLIT, C_ZERO, C_NOCOEF, C_REF0, C_REF1, C_REF2, C_SEG0, C_SEG1, C_SEG2, C_SEG3 };
enum { B_ABSX, B_ABSY, B_SUMX, B_SUMY, B_SQ, B_NZ };

__device__ __forceinline__ void mb_body(const AnalysisMbItem &it) {
    __shared__ int s_cnt[4][NCNT];
    __shared__ long long s_big[4][NBIG];
    const int lane = (int)threadIdx.x & 63, wv = (int)threadIdx.x >> 6;
    // is_inter counts only when check_SSIM ran on this attempt and replaced something (otherwise the array is stale), or when the
    // attempt carries forced intra macroblocks (k_intra_refresh wrote the whole array)
    const bool flags = !it.is_key && (it.forced || (it.replaced && __builtin_nontemporal_load(it.replaced) > 0));
    int cnt[NCNT] = {};
    long long big[NBIG] = {};
    for (int mb = (int)threadIdx.x; mb < it.mbs; mb += 256) {
        const int nz = it.nz[mb], seg = it.seg[mb] & 3;
        big[B_NZ] += nz;
        cnt[C_NOCOEF] += nz == 0;
        cnt[C_SEG0] += seg == 0;
        cnt[C_SEG1] += seg == 1;
        cnt[C_SEG2] += seg == 2;
        cnt[C_SEG3] += seg == 3;
        const bool inter = !it.is_key && (!flags || it.is_inter[mb] != 0);
        if (!inter) {
            ++cnt[C_INTRA];
            continue;
        }
        const int r = it.ref[mb];
        cnt[C_REF0] += r == 0;
        cnt[C_REF1] += r == 1;
        cnt[C_REF2] += r == 2;
        cnt[C_SPLIT] += it.parts[mb] == 1;
        const uint4 v = *reinterpret_cast<const uint4 *>(it.vec + (size_t)mb * 8);      // TL, TR, BL, BR: x | y << 16
        cnt[C_ZERO] += (v.x | v.y | v.z | v.w) == 0u;
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int x = (int16_t)(w[b] & 0xffffu), y = (int16_t)(w[b] >> 16);
            big[B_ABSX] += iabs(x);
            big[B_ABSY] += iabs(y);
            big[B_SUMX] += x;
            big[B_SUMY] += y;
            big[B_SQ] += (long long)x * x + (long long)y * y;
        }
    }
#pragma unroll
    for (int i = 0; i < NCNT; ++i) cnt[i] = wave_sum(cnt[i]);
#pragma unroll
    for (int i = 0; i < NBIG; ++i) big[i] = wave_sum(big[i]);
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < NCNT; ++i) s_cnt[wv][i] = cnt[i];
#pragma unroll
        for (int i = 0; i < NBIG; ++i) s_big[wv][i] = big[i];
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
#pragma unroll
    for (int i = 0; i < NCNT; ++i) cnt[i] = s_cnt[0][i] + s_cnt[1][i] + s_cnt[2][i] + s_cnt[3][i];
#pragma unroll
    for (int i = 0; i < NBIG; ++i) big[i] = s_big[0][i] + s_big[1][i] + s_big[2][i] + s_big[3][i];
    AnalysisMbMirror *h = it.host;
    h->frame_number = it.frame_number;
    h->is_key = it.is_key;
    h->mbs_total = it.mbs;
    h->mbs_intra = cnt[C_INTRA];
    h->mbs_split = cnt[C_SPLIT];
    h->mbs_zero_mv = cnt[C_ZERO];
    h->mbs_no_coeffs = cnt[C_NOCOEF];
    h->mbs_ref[0] = cnt[C_REF0];
    h->mbs_ref[1] = cnt[C_REF1];
    h->mbs_ref[2] = cnt[C_REF2];
    h->segment_mbs[0] = cnt[C_SEG0];
    h->segment_mbs[1] = cnt[C_SEG1];
    h->segment_mbs[2] = cnt[C_SEG2];
    h->segment_mbs[3] = cnt[C_SEG3];
    h->mv_abs_sum[0] = (uint64_t)big[B_ABSX];
    h->mv_abs_sum[1] = (uint64_t)big[B_ABSY];
    h->mv_sum[0] = big[B_SUMX];
    h->mv_sum[1] = big[B_SUMY];
    h->mv_sq_sum = (uint64_t)big[B_SQ];
    h->nz_coeffs = (uint64_t)big[B_NZ];
    __hip_atomic_store(&h->seq, it.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);   // the host polls this word
}

}  // namespace analysis

static_assert(sizeof(BatchOf<AnalysisSrcItem>) + sizeof(analysis::Geo) <= 4096 && sizeof(BatchOf<AnalysisMbItem>) <= 4096,
              "a batch's argument blocks travel in the 4 KiB kernel-argument segment");
__global__ __launch_bounds__(256) void k_analyse_src_b(BatchOf<AnalysisSrcItem> b, analysis::Geo g) {
    const AnalysisSrcItem &it = b.item[blockIdx.z];
    if (it.have_prev) analysis::src_body<true>(it, g);      // (uniform per member)
    else analysis::src_body<false>(it, g);
}
__global__ __launch_bounds__(256) void k_analyse_mb_b(BatchOf<AnalysisMbItem> b) { analysis::mb_body(b.item[blockIdx.z]); }

void launch_analyse_src_batch(hipStream_t s, const AnalysisSrcItem *items, int n) {
    if (n <= 0) return;
    BatchOf<AnalysisSrcItem> b;
    b.n = n;
    for (int i = 0; i < n; ++i) b.item[i] = items[i];
    analysis::Geo g;
    g.mbw = items[0].cur.w / 16;
    g.mbh = items[0].cur.h / 16;
    g.qrow = (g.mbw + 3) / 4;
    g.nquads = g.qrow * g.mbh;
    const int waves = (g.nquads + analysis::QPW - 1) / analysis::QPW;
    g.blocks = (waves + 3) / 4;
    VP8_LAUNCH(k_analyse_src_b, dim3(g.blocks, 1, n), dim3(256), 0, s, b, g);
}

void launch_analyse_mb_batch(hipStream_t s, const AnalysisMbItem *items, int n) {
    if (n <= 0) return;
    BatchOf<AnalysisMbItem> b;
    b.n = n;
    for (int i = 0; i < n; ++i) b.item[i] = items[i];
    VP8_LAUNCH(k_analyse_mb_b, dim3(1, 1, n), dim3(256), 0, s, b);
}

}  // namespace vp8
