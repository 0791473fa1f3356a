// lf_shared.h -- what the loop-filter kernels have in common, once: the sample helpers and the normal filter's edge arithmetic
// (lf_banded.h's form 3, kernels_lf4.hip), the bounded wait, check_SSIM's tail riding in the filter's launch (the prologue every
// workgroup runs and the verdict workgroup), the end of the launch clock and the counter window of a launch.  The callers are the
// banded byte-tile body (lf_banded.h: kernels_lf3.hip, kernels_lf_simple.hip) and the dword-plane body of kernels_lf4.hip.
// Everything here is inlined into the one kernel body of its caller: a call would put the argument block into scratch memory.
#pragma once
#include "vp8hip_dev.h"

namespace vp8 {
namespace lf {

constexpr int BIAS = 256;   // samples carry +256 in registers: |a-b| is one v_sad_u16 even when an unsaturated carry dips below zero

__device__ __forceinline__ int ad(int a, int b) { return (int)__builtin_amdgcn_sad_u16((uint32_t)a, (uint32_t)b, 0u); }
__device__ __forceinline__ int c128(int v) { return iclamp(v, -128, 127); }
__device__ __forceinline__ int max3i(int a, int b, int c) { return imax(imax(a, b), c); }
// biased sample -> biased saturated sample; its low byte is the pixel (BIAS = 256)
__device__ __forceinline__ int satb(int v) { return iclamp(v, BIAS, BIAS + 255); }

// ---- the normal filter's edges (CPU_kernels.cl:829-926) -------------------------------------------------------------------
struct EdgeRegs { int p3, p2, p1, p0, q0, q1, q2, q3; };
struct Limits { int mb_delta, b_delta, hev_thr; };   // *_delta = interior limit - 2*edge limit - 1, see edge_masks

// 2|p0-q0| + (|p1-q1| >> 1) <= E  <=>  |p1-q1| + 4|p0-q0| <= 2E + 1  <=>  that sum + (I - 2E - 1) <= I, so the
// edge test joins the six interior tests (each |a-b| <= I) in one max3 and one compare.  edge_delta = I-2E-1.
// I == -1 switches the edge off: the interior differences are >= 0, so the mask can never be true.
__device__ __forceinline__ void edge_masks(const EdgeRegs &e, int int_lim, int edge_delta, int hev_thr, bool &mask,
                                           bool &hev) {
    const int d10 = ad(e.p1, e.p0), dq10 = ad(e.q1, e.q0);
    const int m1 = max3i(ad(e.p3, e.p2), ad(e.p2, e.p1), d10);
    const int m2 = max3i(dq10, ad(e.q2, e.q1), ad(e.q3, e.q2));
    const int edge = (int)__builtin_amdgcn_sad_u16((uint32_t)e.p1, (uint32_t)e.q1, (uint32_t)((ad(e.p0, e.q0) << 2) + edge_delta));
    mask = max3i(m1, m2, edge) <= int_lim;
    hev = imax(d10, dq10) > hev_thr;
}
__device__ __forceinline__ void filter_mb_edge(EdgeRegs &e, const Limits &L, int int_lim) {  // :829-883
    bool mask, hev;
    edge_masks(e, int_lim, L.mb_delta, L.hev_thr, mask, hev);
    int w = c128(e.p1 - e.q1);
    w = c128(w + (e.q0 - e.p0) * 3);
    w = mask ? w : 0;
    int a = imin(hev ? w : 0, 123);   // min(a + 4, 127) >> 3 and min(a + 3, 127) >> 3 are both 15 from 123 on: one min for the two
    const int b = (a + 3) >> 3;
    a = (a + 4) >> 3;
    e.q0 -= a; e.p0 += b;
    w = hev ? 0 : w;
    a = (w * 27 + 63) >> 7; e.q0 -= a; e.p0 += a;
    a = (w * 18 + 63) >> 7; e.q1 -= a; e.p1 += a;
    a = (w * 9 + 63) >> 7;  e.q2 -= a; e.p2 += a;
}
__device__ __forceinline__ void filter_b_edge(EdgeRegs &e, const Limits &L, int int_lim) {  // :885-926
    bool mask, hev;
    edge_masks(e, int_lim, L.b_delta, L.hev_thr, mask, hev);
    int a = c128(e.p1 - e.q1);
    a = hev ? a : 0;
    a = iclamp(a + (e.q0 - e.p0) * 3, -128, 123);   // the clamp to 127 and the two min(.., 127) >> 3 behind it in one (see filter_mb_edge)
    a = mask ? a : 0;
    const int b = (a + 3) >> 3;
    a = (a + 4) >> 3;
    e.q0 -= a; e.p0 += b;
    a = (a + 1) >> 1;
    a = hev ? 0 : a;
    e.q1 -= a; e.p1 += a;
}

// One line of biased samples t[0..19] (t[0..3] precede the macroblock edge) through the MB edge and the three
// inner edges, each under its own interior limit (-1 = edge switched off).  t[] receives the UNSATURATED results (the reference saturates when it
// stores); the p/q registers handed from edge to edge stay unsaturated too (:1024, :1062).  t[0], t[18], t[19] are never written.
// (Form 4 runs the same line in two parts, line_pre / line_post in kernels_lf4.hip.)
// SAT (vp8hip_conformant_stream, NOT the reference): the registers an edge hands to the next one -- three from the macroblock edge, two
// from an inner edge -- are saturated at the hand-over, as a decoder finds them in the plane.  t[] still receives unsaturated results.
template <bool SAT = false>
__device__ __forceinline__ void filter_line(int (&t)[20], const Limits &L, int il_mb, int il4, int il8) {
    EdgeRegs e;
    e.p3 = t[0]; e.p2 = t[1]; e.p1 = t[2]; e.p0 = t[3];
    e.q0 = t[4]; e.q1 = t[5]; e.q2 = t[6]; e.q3 = t[7];
    filter_mb_edge(e, L, il_mb);
    t[1] = e.p2; t[2] = e.p1; t[3] = e.p0;
    t[4] = e.q0; t[5] = e.q1; t[6] = e.q2;
#pragma unroll
    for (int k = 4; k < 16; k += 4) {
        e.p3 = e.q0; e.p2 = e.q1; e.p1 = e.q2; e.p0 = e.q3;
        if (SAT) { e.p3 = satb(e.p3); e.p2 = satb(e.p2); if (k == 4) e.p1 = satb(e.p1); }
        e.q0 = t[4 + k]; e.q1 = t[5 + k]; e.q2 = t[6 + k]; e.q3 = t[7 + k];
        filter_b_edge(e, L, k == 4 ? il4 : il8);
        t[2 + k] = e.p1; t[3 + k] = e.p0; t[4 + k] = e.q0; t[5 + k] = e.q1;
    }
}

// ---- flags and waits ------------------------------------------------------------------------------------------------------
// The flags are polled: the accesses must be volatile, and a volatile access through HIP's generic pointers stays a FLAT
// instruction (the address-space inference pass leaves volatile accesses alone) -- a flat load that resolves to LDS takes the
// vector-memory path, returns on vmcnt behind the wave's prefetch loads and block stores, and four of them one after the other
// were the 450 cycles of every step's poll.  Through an LDS-qualified pointer they are ds_read / ds_write on lgkmcnt.
typedef __attribute__((address_space(3))) volatile int lds_flag_t;
// everything this wave has written to / read from LDS is done, and the compiler moves no memory access across this point
__device__ __forceinline__ void lds_fence() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// Every wait in these kernels is bounded (dispatch order and co-residency of workgroups are not architecturally
// guaranteed): a wait that is still unsatisfied after SPIN_LIMIT polls (>= 0.3 s; a frame takes < 1 ms) raises the
// workgroup's abort flag and the error word in HBM, and every wave that sees the flag leaves the kernel.  The
// frame is then invalid -- reported as VP8HIP_ERR_TIMEOUT -- but nothing hangs.
// The macro works on its caller's `flag` (lds_flag_t *), F_ABORT and `a` (the argument block).  fence_after: no memory access
// of the caller moves up across the end of the wait (form 4, whose plane accesses carry no dependence on the flags).
constexpr int SPIN_LIMIT = 1 << 22;
#define LF_BOUNDED_WAIT(cond_unsatisfied, nap, fence_after)                         \
    {                                                                               \
        int spins_ = 0;                                                             \
        while ((cond_unsatisfied) && !flag[F_ABORT]) {                              \
            __builtin_amdgcn_s_sleep(nap);                                          \
            if (++spins_ > SPIN_LIMIT / (nap)) { flag[F_ABORT] = 1; *a.err = 1; }   \
        }                                                                           \
        if (flag[F_ABORT]) return;                                                  \
        if (fence_after) asm volatile("" ::: "memory");                             \
    }

// ---- check_SSIM's tail in the filter's launch -----------------------------------------------------------------------------
// vp8enc.cpp:252-261: `if (min1 > 0.95) prepare_segments_data(1, 7)`.  Every workgroup takes the frame's minimum SSIM itself
// (8 160 floats at 1080p: a few microseconds) and, above 0.95, filters with the segment data that call produces -- nobody waits
// for a kernel that would have done it.  Returns the segment data in force: sh.sd.v if the update applies, else a.sd->v.
// For launches with a.chk.on: all NWAVES waves of the workgroup call it, each with its wave index as it keeps it.  The kernel:
//     const int32_t *sdv = a.sd->v;
//     if (a.chk.on) {
//         sdv = check_ssim_segments<NWAVES>(a, sh, wave);
//         if (band >= a.nbands) { verdict_workgroup<NWAVES>(a, sh, sdv != a.sd->v, staging); return; }
//     } else if (band >= a.nbands) return;
template <int NWAVES, typename Args, typename Shared>
__device__ __forceinline__ const int32_t *check_ssim_segments(const Args &a, Shared &sh, int wave) {
    const int32_t *sdv = a.sd->v;
    const int lane = threadIdx.x & 63;
    float mn = 2.0f;
    const int mbs_all = a.mbw * a.mbh;
    for (int i = threadIdx.x; i < mbs_all; i += NWAVES * 64) { const float v = a.o.ssim[i]; mn = v < mn ? v : mn; }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) { const float o = __shfl_xor(mn, m, 64); mn = o < mn ? o : mn; }
    if (lane == 0) sh.red[wave] = mn;
    __syncthreads();
    mn = sh.red[0];
#pragma unroll
    for (int w = 1; w < NWAVES; ++w) mn = sh.red[w] < mn ? sh.red[w] : mn;
    if (mn > 0.95f) {   // (the reference compares with the double 0.95: no float lies between 0.95f and 0.95)
        if (threadIdx.x == 0) {
            const int refqi[4] = {a.chk.refqi[0], a.chk.refqi[1], a.chk.refqi[2], a.chk.refqi[3]};
            fill_segment_data(&sh.sd, 0, refqi, a.chk.qi_min, a.chk.strength[0], a.chk.strength[1], true);
        }
        sdv = sh.sd.v;
        __syncthreads();
    }
    return sdv;
}

// The workgroup behind the last band, present when check_SSIM rides in the launch: what check_SSIM reports (vp8enc.cpp:237-258:
// replaced count, the raster-order float sum / count, the minimum), the updated segment data back to where the entropy stage
// reads them, and the verdict to the host.  The sum must be the reference's -- one float accumulator over the macroblocks in
// raster order -- so the values are staged in LDS by all threads and one thread adds them, four per ds_read_b128.
// s_val: VERDICT_CHUNK floats of LDS, 16-byte aligned, that this workgroup has no other use for (the caller asserts the size).
constexpr int VERDICT_CHUNK = 8192;
template <int NWAVES, typename Args, typename Shared>
__device__ __forceinline__ void verdict_workgroup(const Args &a, Shared &sh, bool updated, float *s_val) {
    constexpr int NT = NWAVES * 64, CHUNK = VERDICT_CHUNK;
    const int mbs = a.mbw * a.mbh, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (threadIdx.x == 0) sh.repl = 0;
    int repl = 0;
    float mn = 2.0f, sum = 0.0f;
    for (int base = 0; base < mbs; base += CHUNK) {
        const int n = imin(CHUNK, mbs - base);
        __syncthreads();
        for (int i = threadIdx.x; i < CHUNK; i += NT) {
            float v = 0.0f;
            if (i < n) {
                v = a.o.ssim[base + i];
                repl += a.chk.is_inter[base + i] == 0;
                mn = v < mn ? v : mn;
            }
            s_val[i] = v;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            const float4 *q = reinterpret_cast<const float4 *>(s_val);
            int i = 0;
            for (; i + 32 <= n; i += 32) {   // eight reads in flight, then the 32 dependent additions
                float4 v[8];
#pragma unroll
                for (int k2 = 0; k2 < 8; ++k2) v[k2] = q[(i >> 2) + k2];
#pragma unroll
                for (int k2 = 0; k2 < 8; ++k2) sum = __fadd_rn(__fadd_rn(__fadd_rn(__fadd_rn(sum, v[k2].x), v[k2].y), v[k2].z), v[k2].w);
            }
            for (; i + 4 <= n; i += 4) {
                const float4 v = q[i >> 2];
                sum = __fadd_rn(__fadd_rn(__fadd_rn(__fadd_rn(sum, v.x), v.y), v.z), v.w);
            }
            for (; i < n; ++i) sum = __fadd_rn(sum, s_val[i]);
        }
    }
    // with no macroblock flagged the fallback left is_inter untouched (stale): nothing was replaced
    const bool fallback_ran = __builtin_nontemporal_load(a.o.flags) != 0;
    if (fallback_ran) atomicAdd(&sh.repl, repl);
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) { const float o = __shfl_xor(mn, m, 64); mn = o < mn ? o : mn; }
    __syncthreads();            // (sh.red was last read before this function)
    if (lane == 0) sh.red[wave] = mn;
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int w = 0; w < NWAVES; ++w) mn = sh.red[w] < mn ? sh.red[w] : mn;
    if (updated) {
        for (int i = 0; i < 4 * SD_INTS; ++i) a.sd->v[i] = sh.sd.v[i];
        a.chk.strength[2] = 7;      // video.loop_filter_sharpness after prepare_segments_data(1, 7)
    }
    a.o.flags[0] = 0;               // the fallback has run (the launch before this one): zero at rest
    const int32_t w[5] = {sh.repl, __float_as_int(__fdiv_rn(sum, (float)mbs)), __float_as_int(mn), *a.err, updated ? 1 : 0};
    for (int i = 0; i < 5; ++i) {
        a.chk.stats[i] = w[i];
        __hip_atomic_store(&a.chk.verdict[i], w[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    __hip_atomic_store(&a.chk.verdict[5], (int32_t)a.chk.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);   // the host polls this word
}

// ---- the kernel's own clock (constant 100 MHz) ----------------------------------------------------------------------------
// Band 0 stamps the start, the wave that finishes the frame's last real work adds end - start to an accumulator the host reads
// with the profile (vp8hip_profile_read_clock); hipEvents around a launch also count the time its packet waits for the queue
// when many streams share the part.  clk = the 64-bit words from the error word + 4 ints on:
//   {start, sum of ticks, launches, sum of shader-clock cycles per tick x 1000, launches left out of that sum, launches whose
//    last wave changed slots}
// How the start gets into the sum of ticks and how the last wave computes its ratio is the form's own business (form 4 keeps
// loads and a 64-bit division off the tail of its chain); what the last wave then does with them is LF_CLOCK_RATIO.
// ratio: s_memtime cycles per 100 MHz tick x 1000 while the wave ran (MI355X_MICROARCH.md, DVFS (6)).  A wave that was
// context-switched (the hardware scheduler rotating an oversubscribed set of queues) comes back on another slot (hwid0: its
// hw_slot() at the start), whose cycle counter is another one: such launches are counted, not averaged.
__device__ __forceinline__ uint32_t hw_slot() { return __builtin_amdgcn_s_getreg((4) | (0 << 6) | (31 << 11)); }   // HW_REG_HW_ID
#define LF_CLOCK_RATIO(clk, ratio, hwid0)                                                   \
    {                                                                                       \
        const uint32_t hwid1_ = hw_slot();                                                  \
        if ((ratio) > 100000ull) atomicAdd((clk) + 4, 1ull); else atomicAdd((clk) + 3, ratio); \
        if (hwid1_ != (hwid0)) atomicAdd((clk) + 5, 1ull);                                  \
    }

}  // namespace lf

// Band counters and hand-off tags are never reset: launch n of a context counts inside its own window (gbase, gbase + mbw + 2].
// Returns gbase; 0 means the window index has wrapped (after ~2^31/(mbw+2) launches, and at the first one) and the caller zeroes
// its counters in the stream first.
inline int lf_window_base(unsigned launch_no, int mbw) {
    const unsigned window = 0x7fffffffu / (unsigned)(mbw + 2) - 1;
    return (int)((launch_no % window) * (unsigned)(mbw + 2));
}

}  // namespace vp8
