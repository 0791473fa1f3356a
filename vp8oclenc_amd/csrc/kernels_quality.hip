// kernels_quality.hip -- PSNR and SSIM of a coded frame on the device (gfx950): the filtered reconstruction against the source
// region of the current frame, all three planes in one launch (vp8hip_set_quality_stats).
//
// Bound by memory traffic: the kernel reads the source region and the reconstruction region once (2 x 1.5 x w x h bytes, 6.2 MB per
// 1080p frame) plus one block row per tile again.  A lane walks down a column of 4x4 blocks, one aligned dword per row and image
// (surface rows are 64-byte aligned behind a 32-pixel margin), and forms a block's five sums with v_dot4_u32_u8: sum s, sum r against
// 0x01010101, sum s^2, sum r^2, sum s r.  A window of libvpx's SSIM (8x8, every 4 samples) is 2x2 blocks: the right neighbours come
// from the next lane, the blocks above are kept from the previous step.  A block's squared error is sum s^2 + sum r^2 - 2 sum s r;
// samples outside the region are 0 in both images, so partial blocks at the region's edge count toward it and whole windows never
// touch the edge.
//
// Deterministic: every wave writes its partial sums, the last wave to take the ticket adds them up in a fixed order; no floating-point
// atomics.  A context measured alone and as a batch member runs the same waves, so the results are the same bits.
#include "vp8hip_dev.h"

namespace vp8 {

namespace {

__host__ __device__ inline double quality_psnr(uint64_t sse, uint64_t samples) {
    return sse == 0 ? 100.0 : 10.0 * log10((double)samples * 65025.0 / (double)sse);
}

__host__ __device__ inline void quality_fold(QualitySums &t, const vp8hip_quality &q) {
    t.frames += 1;
    for (int p = 0; p < 3; ++p) {
        t.sse[p] += q.sse[p];
        t.samples[p] += q.samples[p];
        t.ssim_sum[p] += q.ssim[p];
    }
    t.psnr_all_sum += q.psnr_all;
    t.ssim_all_sum += q.ssim_all;
    if (t.frames == 1 || q.psnr_all < t.psnr_min) {
        t.psnr_min = q.psnr_all;
        t.psnr_min_frame = q.frame_number;
    }
}

struct BlockSums { uint32_t s, r, ss, rr, sr; };

__device__ __forceinline__ uint32_t shift_down(uint32_t v) { return (uint32_t)__shfl_down((int)v, 1, 64); }

// block (bx, by) of plane P; a block outside the region, or its part outside, is 0 in both images
__device__ __forceinline__ BlockSums block_sums(const QualityPlane &P, int bx, int by) {
    BlockSums b{0u, 0u, 0u, 0u, 0u};
    const int x = bx * 4, left = P.w - x;
    const uint32_t m = left >= 4 ? 0xffffffffu : (left <= 0 ? 0u : (1u << (8 * left)) - 1u);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int y = by * 4 + k;
        uint32_t s = 0u, r = 0u;
        if (m && y < P.h) {
            s = *reinterpret_cast<const uint32_t *>(P.s + (size_t)y * P.ss + x) & m;
            r = *reinterpret_cast<const uint32_t *>(P.r + (size_t)y * P.rs + x) & m;
        }
        b.s = __builtin_amdgcn_udot4(s, 0x01010101u, b.s, false);
        b.r = __builtin_amdgcn_udot4(r, 0x01010101u, b.r, false);
        b.ss = __builtin_amdgcn_udot4(s, s, b.ss, false);
        b.rr = __builtin_amdgcn_udot4(r, r, b.rr, false);
        b.sr = __builtin_amdgcn_udot4(s, r, b.sr, false);
    }
    return b;
}

// libvpx's integer SSIM of one 8x8 window (vpx_dsp/ssim.c, similarity for 8-bit samples): both products exact in 64 bits
__device__ __forceinline__ double window_ssim(uint32_t S, uint32_t R, uint32_t SS, uint32_t RR, uint32_t SR) {
    const int64_t s = S, r = R, c1 = 26634, c2 = 239708;
    const int64_t num = (2 * s * r + c1) * (128 * (int64_t)SR - 2 * s * r + c2);
    const int64_t den = (s * s + r * r + c1) * (64 * (int64_t)SS - s * s + 64 * (int64_t)RR - r * r + c2);
    return (double)num / (double)den;
}

__device__ __forceinline__ int plane_tiles(int w, int h) {
    const int nbc = (w + 3) / 4, nbr = (h + 3) / 4;
    return ((nbc + QUALITY_TILE_COLS - 1) / QUALITY_TILE_COLS) * ((nbr + QUALITY_TILE_ROWS - 1) / QUALITY_TILE_ROWS);
}

template <typename T> __device__ __forceinline__ T wave_sum_fixed(T v) {   // the same butterfly every time: the same bits
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// the last wave of the launch (of the member): partials in a fixed order, the record, the fold, the state and its mirror
__device__ void quality_final(const QualityArgs &a, const int (&tiles)[3]) {
    const int lane = threadIdx.x;
    vp8hip_quality q;
    q.frame_number = a.frame_number;
    q.is_key = a.is_key;
    int base = 0;
    uint64_t sse_all = 0, n_all = 0;
    for (int p = 0; p < 3; ++p) {
        unsigned long long sse = 0;
        double ssim = 0.0;
        for (int t = base + lane; t < base + tiles[p]; t += 64) {
            sse += a.partial[t].sse;
            ssim += a.partial[t].ssim;
        }
        sse = wave_sum_fixed(sse);
        ssim = wave_sum_fixed(ssim);
        base += tiles[p];
        const int w = a.p[p].w, h = a.p[p].h;
        const int64_t wx = w / 4 - 1, wy = h / 4 - 1, windows = wx > 0 && wy > 0 ? wx * wy : 0;
        q.sse[p] = sse;
        q.samples[p] = (uint64_t)w * (uint64_t)h;
        q.psnr[p] = quality_psnr(q.sse[p], q.samples[p]);
        q.ssim[p] = windows ? ssim / (double)windows : (sse == 0 ? 1.0 : 0.0);
        sse_all += q.sse[p];
        n_all += q.samples[p];
    }
    q.psnr_all = quality_psnr(sse_all, n_all);
    q.ssim_all = 0.8 * q.ssim[0] + 0.1 * (q.ssim[1] + q.ssim[2]);
    if (lane != 0) return;
    QualityState st = *a.state;
    if (st.has_pending && st.pending.frame_number != q.frame_number) quality_fold(st.sums, st.pending);   // (the same frame again: replaced)
    st.pending = q;
    st.has_pending = 1;
    st.seq = a.seq;
    *a.state = st;
    *a.ticket = 0u;
    if (a.host) {
        a.host->pending = st.pending;
        a.host->has_pending = 1;
        a.host->sums = st.sums;
        __hip_atomic_store(&a.host->seq, a.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);   // the host polls this word
    }
}

__device__ __forceinline__ void quality_body(const QualityArgs &a) {
    const int lane = threadIdx.x;
    const int tiles[3] = {plane_tiles(a.p[0].w, a.p[0].h), plane_tiles(a.p[1].w, a.p[1].h), plane_tiles(a.p[2].w, a.p[2].h)};
    int t = blockIdx.x, plane = 0;
    if (t >= tiles[0]) { t -= tiles[0]; plane = 1; }
    if (plane == 1 && t >= tiles[1]) { t -= tiles[1]; plane = 2; }
    const QualityPlane P = a.p[plane];
    const int nbc = (P.w + 3) / 4, nbr = (P.h + 3) / 4, fbc = P.w / 4, fbr = P.h / 4;
    const int ntx = (nbc + QUALITY_TILE_COLS - 1) / QUALITY_TILE_COLS;
    const int tx = t % ntx, ty = t / ntx;
    const int bx = tx * QUALITY_TILE_COLS + lane, by0 = ty * QUALITY_TILE_ROWS;
    const int own_end = min(by0 + QUALITY_TILE_ROWS, nbr), walk_end = min(by0 + QUALITY_TILE_ROWS + 1, nbr);
    const bool own_col = lane < QUALITY_TILE_COLS && bx < nbc;
    const bool win_col = lane < QUALITY_TILE_COLS && bx + 1 < fbc;
    uint32_t sse = 0u;
    double ssim = 0.0;
    BlockSums up{0u, 0u, 0u, 0u, 0u}, upr{0u, 0u, 0u, 0u, 0u};
    for (int by = by0; by < walk_end; ++by) {
        const BlockSums b = block_sums(P, bx, by);
        const BlockSums br{shift_down(b.s), shift_down(b.r), shift_down(b.ss), shift_down(b.rr), shift_down(b.sr)};
        if (own_col && by < own_end) sse += b.ss + b.rr - 2u * b.sr;
        if (by > by0 && win_col && by < fbr)   // the window whose top-left block is (bx, by - 1)
            ssim += window_ssim(up.s + upr.s + b.s + br.s, up.r + upr.r + b.r + br.r, up.ss + upr.ss + b.ss + br.ss,
                                up.rr + upr.rr + b.rr + br.rr, up.sr + upr.sr + b.sr + br.sr);
        up = b;
        upr = br;
    }
    // a wave's squared error fits 32 bits: 63 lanes x 8 blocks x 16 x 255^2 < 2^32
    sse = wave_sum_fixed(sse);
    ssim = wave_sum_fixed(ssim);
    unsigned ticket = 0u;
    if (lane == 0) {
        a.partial[blockIdx.x] = QualityPartial{sse, ssim};
        __threadfence();
        ticket = atomicAdd(a.ticket, 1u);
    }
    ticket = __shfl(ticket, 0, 64);
    if (ticket + 1u != (unsigned)(tiles[0] + tiles[1] + tiles[2])) return;
    __threadfence();
    quality_final(a, tiles);
}

}  // namespace

__global__ __launch_bounds__(64) void k_quality(QualityArgs a) { quality_body(a); }

__global__ __launch_bounds__(64) void k_quality_b(BatchOf<QualityArgs> b) { quality_body(b.item[blockIdx.y]); }

int quality_tiles(int w, int h) {
    auto plane = [](int pw, int ph) {
        const int nbc = (pw + 3) / 4, nbr = (ph + 3) / 4;
        return ((nbc + QUALITY_TILE_COLS - 1) / QUALITY_TILE_COLS) * ((nbr + QUALITY_TILE_ROWS - 1) / QUALITY_TILE_ROWS);
    };
    return plane(w, h) + 2 * plane((w + 1) / 2, (h + 1) / 2);
}

QualityArgs quality_args(const Frame &src, const Frame &rec, int w, int h) {
    QualityArgs a{};
    const int cw = (w + 1) / 2, ch = (h + 1) / 2;
    a.p[0] = QualityPlane{src.Y[0].p, rec.Y[0].p, src.Y[0].stride, rec.Y[0].stride, w, h};
    a.p[1] = QualityPlane{src.U.p, rec.U.p, src.U.stride, rec.U.stride, cw, ch};
    a.p[2] = QualityPlane{src.V.p, rec.V.p, src.V.stride, rec.V.stride, cw, ch};
    return a;
}

void launch_quality(hipStream_t s, const QualityArgs &a) {
    hipLaunchKernelGGL(k_quality, dim3(quality_tiles(a.p[0].w, a.p[0].h)), dim3(64), 0, s, a);
}

void launch_quality_batch(hipStream_t s, const QualityArgs *a, int n) {
    if (n <= 0) return;
    BatchOf<QualityArgs> b{};
    b.n = n;
    for (int i = 0; i < n; ++i) b.item[i] = a[i];   // (members of a batch share one geometry and one source size)
    hipLaunchKernelGGL(k_quality_b, dim3(quality_tiles(a[0].p[0].w, a[0].p[0].h), n), dim3(64), 0, s, b);
}

void quality_totals(const QualityState &st, vp8hip_quality_totals *t) {
    QualitySums u = st.sums;
    if (st.has_pending) quality_fold(u, st.pending);
    memset(t, 0, sizeof(*t));
    t->frames = u.frames;
    t->psnr_min_frame = -1;
    uint64_t sse = 0, n = 0;
    for (int p = 0; p < 3; ++p) {
        t->sse[p] = u.sse[p];
        t->samples[p] = u.samples[p];
        sse += u.sse[p];
        n += u.samples[p];
    }
    if (!u.frames) return;
    for (int p = 0; p < 3; ++p) {
        t->psnr[p] = quality_psnr(u.sse[p], u.samples[p]);
        t->ssim[p] = u.ssim_sum[p] / (double)u.frames;
    }
    t->psnr_all = quality_psnr(sse, n);
    t->psnr_avg = u.psnr_all_sum / (double)u.frames;
    t->ssim_all = u.ssim_all_sum / (double)u.frames;
    t->psnr_min = u.psnr_min;
    t->psnr_min_frame = u.psnr_min_frame;
}

}  // namespace vp8
