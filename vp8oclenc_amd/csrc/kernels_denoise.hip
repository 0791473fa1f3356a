// kernels_denoise.hip -- temporal noise reduction of the source frames (vp8hip_set_denoise), the third stage of the input side
// next to the pack (k_pack_b) and the scaler (k_scale_b).  The reference never did anything about noise; the rule is the
// project's own and is stated bit for bit in include/vp8hip_host.h (vp8host_denoise_frame is its plain C++ form).
//
// k_denoise_b runs directly behind the pack or scale launch on the same stream and works IN PLACE on the current frame's
// surfaces: S = the frame as packed, R = the history = the previous current frame as it left this kernel.  A context keeps two
// current surfaces that trade places on every frame taken in (next_current, for vp8hip_chroma_change), so the history is the
// OTHER surface and costs no copy: a frame is read twice (S and R) and written at most once, and a macroblock that is copied
// is not written at all.  Every macroblock reads and writes only its own samples: in place is race-free.
//
// Mapping (memory-bound: no LDS, 16-byte accesses, everything in registers):
//   * luma: a lane takes one 16-byte row of a macroblock (global_load_dwordx4 of S and of R), 16 lanes = one DPP row = one
//     macroblock, a wave = four horizontally adjacent macroblocks (64 contiguous bytes per picture row);
//   * the bytes are widened to packed 16-bit pairs (v_perm_b32), the step is packed 16-bit arithmetic, sad is v_sad_u8 on the
//     dwords as they came; T and sad travel in ONE register ((T + bias) | sad << 16) through four DPP steps inside the row;
//   * chroma: the same wave, with the luma verdicts in a ballot: 64 lanes = 2 planes x 4 macroblocks x 8 rows of 8 bytes;
//     T_c is reduced inside 8 lanes (three DPP steps);
//   * a wave does QPW such quads, all loads issued before the first is used (a wave per SIMD is all a 1080p frame gives);
//   * the count of filtered macroblocks and the "last wave" ticket are ONE 64-bit vector atomic per wave (count << 32 | 1); the
//     wave that draws the last ticket writes the record into host memory, the sequence number last.
#include "../../include/vp8hip_host.h"
#include "vp8hip_dev.h"

namespace vp8 {

namespace denoise {

constexpr int QPW = 4;      // quads (of four macroblocks) per wave

struct Geo { int mbw, mbh, qrow, nquads, waves, level; };

// DPP controls: quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror (lane i <-> 7 - i), row_mirror (i <-> 15 - i).  Applied in
// this order to a sum they are the butterfly over 2, 4, 8, 16 lanes: afterwards every lane holds the total of its group.
constexpr int DPP_XOR1 = 0xB1, DPP_XOR2 = 0x4E, DPP_HALF_MIRROR = 0x141, DPP_MIRROR = 0x140;
template <int CTRL> __device__ __forceinline__ int dpp_add(int v) {      // (unsigned: the packed T | sad sum uses all 32 bits)
    return (int)((unsigned)v + (unsigned)__builtin_amdgcn_update_dpp(0, v, CTRL, 0xf, 0xf, false));
}

// Four samples of S and R (one dword each) -> the four samples S + c; the steps c are added to tacc pairwise.
// Per sample (include/vp8hip_host.h): d = R - S, a = |d|, |c| = min(a, 2 + k + (a > 7) + 2 (a > 15)), c has d's sign.
__device__ __forceinline__ uint32_t step4(uint32_t S, uint32_t R, u16x2 base, s16x2 &tacc) {
    uint32_t o[2];
    // (the 1s and 2s pass through an empty asm: min(x, 1) with a constant hipcc can see becomes x != 0, which it scalarises into two
    // v_cmp and two v_cndmask per pair -- see weight_rows, vp8hip_dev.h)
    uint32_t ones = 0x00010001u, twos = 0x00020002u;
    asm("" : "+s"(ones));
    asm("" : "+s"(twos));
    const u16x2 one = __builtin_bit_cast(u16x2, ones), two = __builtin_bit_cast(u16x2, twos);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const uint32_t sel = h ? 0x0c030c02u : 0x0c010c00u;      // bytes (0, 1) or (2, 3) into the low bytes of the two halves
        const s16x2 s = as_s16x2(__builtin_amdgcn_perm(0u, S, sel)), r = as_s16x2(__builtin_amdgcn_perm(0u, R, sel));
        const s16x2 d = r - s;
        const u16x2 a = __builtin_bit_cast(u16x2, __builtin_elementwise_max(d, -d));
        const u16x2 hi = a >> u16x2{3, 3};                        // >= 1: a > 7; >= 2: a > 15
        const u16x2 m = base + __builtin_elementwise_min(hi, one) + __builtin_elementwise_min(hi & u16x2{0xfffe, 0xfffe}, two);
        const s16x2 mag = __builtin_bit_cast(s16x2, __builtin_elementwise_min(a, m));
        const s16x2 sg = d >> s16x2{15, 15};                      // 0 or -1
        const s16x2 c = (mag ^ sg) - sg;
        tacc += c;
        o[h] = as_u32(s + c);                                     // between S and R: a byte, no clamp
    }
    return __builtin_amdgcn_perm(o[1], o[0], 0x06040200u);
}
__device__ __forceinline__ int pair_sum(s16x2 v) { return (int)v.x + (int)v.y; }

__device__ __forceinline__ void denoise_body(const DenoiseItem &it, const Geo &g) {
    const int lane = (int)threadIdx.x & 63;
    const int wave = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
    if (wave >= g.waves) return;      // (wave-uniform: every lane of a wave that works stays active, the DPP steps need that)
    const u16x2 base = {(unsigned short)(2 + g.level), (unsigned short)(2 + g.level)};
    // luma: macroblock lane >> 4 of the quad, row lane & 15; chroma: plane lane >> 5, macroblock (lane >> 3) & 3, row lane & 7
    const int lmb = lane >> 4, lrow = lane & 15, cpl = lane >> 5, cmb = (lane >> 3) & 3, crow = lane & 7;
    const Plane &cp = cpl ? it.cur.V : it.cur.U;
    const uint8_t *hist_c = cpl ? it.hist.V.p : it.hist.U.p;
    const int hist_cs = cpl ? it.hist.V.stride : it.hist.U.stride;
    uint4 S[QPW], R[QPW];
    uint2 Sc[QPW], Rc[QPW];
    uint8_t *py[QPW], *pc[QPW];
    bool vy[QPW], vc[QPW];
#pragma unroll
    for (int k = 0; k < QPW; ++k) {
        int q = wave * QPW + k;
        const bool live = q < g.nquads;
        q = live ? q : g.nquads - 1;      // (a wave's spare quads compute the last quad again and store nothing)
        const int mby = q / g.qrow, mbx0 = (q - mby * g.qrow) * 4;
        vy[k] = live && mbx0 + lmb < g.mbw;
        vc[k] = live && mbx0 + cmb < g.mbw;
        const int lx = imin(mbx0 + lmb, g.mbw - 1), cx = imin(mbx0 + cmb, g.mbw - 1);
        const ptrdiff_t oy = (ptrdiff_t)(mby * 16 + lrow) * it.cur.Y[0].stride + lx * 16;
        const ptrdiff_t hy = (ptrdiff_t)(mby * 16 + lrow) * it.hist.Y[0].stride + lx * 16;
        py[k] = it.cur.Y[0].p + oy;
        S[k] = *reinterpret_cast<const uint4 *>(py[k]);
        R[k] = *reinterpret_cast<const uint4 *>(it.hist.Y[0].p + hy);
        pc[k] = cp.p + (ptrdiff_t)(mby * 8 + crow) * cp.stride + cx * 8;
        Sc[k] = *reinterpret_cast<const uint2 *>(pc[k]);
        Rc[k] = *reinterpret_cast<const uint2 *>(hist_c + (ptrdiff_t)(mby * 8 + crow) * hist_cs + cx * 8);
    }
    unsigned filtered = 0;
#pragma unroll
    for (int k = 0; k < QPW; ++k) {
        s16x2 t = {0, 0};
        uint4 o;
        o.x = step4(S[k].x, R[k].x, base, t);
        o.y = step4(S[k].y, R[k].y, base, t);
        o.z = step4(S[k].z, R[k].z, base, t);
        o.w = step4(S[k].w, R[k].w, base, t);
        uint32_t sad = __builtin_amdgcn_sad_u8(S[k].x, R[k].x, 0u);
        sad = __builtin_amdgcn_sad_u8(S[k].y, R[k].y, sad);
        sad = __builtin_amdgcn_sad_u8(S[k].z, R[k].z, sad);
        sad = __builtin_amdgcn_sad_u8(S[k].w, R[k].w, sad);
        // a lane's T lies in [-128, 128] (16 steps of at most 8), its sad in [0, 4080]: (T + 128) | sad << 16 summed over 16 lanes
        // is (T_mb + 2048) | sad_mb << 16 with sad_mb <= 65280 -- neither half carries
        int ts = (int)((uint32_t)(pair_sum(t) + 128) | (sad << 16));
        ts = dpp_add<DPP_XOR1>(ts);
        ts = dpp_add<DPP_XOR2>(ts);
        ts = dpp_add<DPP_HALF_MIRROR>(ts);
        ts = dpp_add<DPP_MIRROR>(ts);
        const int T = (ts & 0xffff) - 2048, sad_mb = (int)((uint32_t)ts >> 16);
        const bool f = iabs(T) <= VP8HOST_DENOISE_SUM_Y && sad_mb <= VP8HOST_DENOISE_SAD_Y;
        const unsigned long long fm = __ballot(f);                 // bit 16 m: macroblock m of the quad is filtered
        if (f && vy[k]) *reinterpret_cast<uint4 *>(py[k]) = o;     // (a copied macroblock keeps the bytes it has)
        filtered += (unsigned)__popcll(__ballot(f && vy[k]) & 0x0001000100010001ull);
        // the quad's chroma blocks, each on its own sum
        s16x2 tc = {0, 0};
        uint2 oc;
        oc.x = step4(Sc[k].x, Rc[k].x, base, tc);
        oc.y = step4(Sc[k].y, Rc[k].y, base, tc);
        int Tc = pair_sum(tc);
        Tc = dpp_add<DPP_XOR1>(Tc);
        Tc = dpp_add<DPP_XOR2>(Tc);
        Tc = dpp_add<DPP_HALF_MIRROR>(Tc);
        const bool luma_f = ((fm >> (16 * cmb)) & 1ull) != 0;
        if (luma_f && vc[k] && iabs(Tc) <= VP8HOST_DENOISE_SUM_C) *reinterpret_cast<uint2 *>(pc[k]) = oc;
    }
    if (lane != 0) return;
    // count and ticket in one 64-bit atomic: nothing but the word itself passes between the waves, so no fence
    const unsigned long long old = atomicAdd(it.word, ((unsigned long long)filtered << 32) | 1ull);
    if ((unsigned)(old & 0xffffffffull) + 1u != (unsigned)g.waves) return;
    atomicExch(it.word, 0ull);        // zero at rest
    it.host->frame_number = it.frame_number;
    it.host->mbs_filtered = (int32_t)((old >> 32) + filtered);
    it.host->mbs_total = g.mbw * g.mbh;
    __hip_atomic_store(&it.host->seq, it.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);   // the host polls this word
}

}  // namespace denoise

static_assert(sizeof(BatchOf<DenoiseItem>) + sizeof(denoise::Geo) <= 4096, "a batch's argument blocks travel in the 4 KiB kernel-argument segment");
__global__ __launch_bounds__(256) void k_denoise_b(BatchOf<DenoiseItem> b, denoise::Geo g) {
    denoise::denoise_body(b.item[blockIdx.z], g);
}

void launch_denoise_batch(hipStream_t s, const DenoiseItem *items, int n, int level) {
    if (n <= 0) return;
    BatchOf<DenoiseItem> b;
    b.n = n;
    for (int i = 0; i < n; ++i) b.item[i] = items[i];
    denoise::Geo g;
    g.mbw = items[0].cur.Y[0].w / 16;
    g.mbh = items[0].cur.Y[0].h / 16;
    g.qrow = (g.mbw + 3) / 4;
    g.nquads = g.qrow * g.mbh;
    g.waves = (g.nquads + denoise::QPW - 1) / denoise::QPW;
    g.level = level;
    VP8_LAUNCH(k_denoise_b, dim3((g.waves + 3) / 4, 1, n), dim3(256), 0, s, b, g);
}

}  // namespace vp8
