// kernels_lf_simple.hip -- VP8 simple loop filter (RFC 6386 section 15.2, frame header filter_type = 1): the banded
// byte-tile body of lf_banded.h (see there for the data movement) under the simple filter's edges.
//
// The simple filter touches luma only, reads p1..q1 and writes only p0 and q0, and has no hev branch.  The order the
// format defines (raster order; per macroblock: left MB edge, vertical inner edges 4/8/12, top MB edge, horizontal inner
// edges) is still a chain: MB(x,y) needs MB(x-1,y) complete and, for its horizontal edges, the vertical edges of MB(x,y-1)
// and MB(x+1,y-1).  But the four vertical edges of a macroblock no longer depend on each other (edge c writes columns
// c-1, c and reads c-2..c+1), nor do its four horizontal edges, so every phase of a macroblock step is four INDEPENDENT
// edge filters per lane instead of the normal filter's four dependent ones.
//
// Differences in semantics from the normal forms: a macroblock whose segment has loop_filter_level 0 is skipped and the
// rest of the plane is filtered (the format, libvpx, libwebp); the reference's "level 0 ends the plane" belongs to its
// normal filter.  The edge limits are the segment's mbedge_limit / sub_bedge_limit (= 2(L+2)+I and 2L+I, RFC 6386
// section 15.2); interior_limit and hev_threshold are unused.  The band counters are the simple filter's own
// (LF_SIMPLE_WORD in the progress buffer, its own launch count), so a context may alternate filter types frame by frame.
#include "lf_banded.h"

namespace vp8 {

namespace lfs {

using namespace lfb;

// One edge of the simple filter (RFC 6386 section 15.2: simple_segment, common_adjust(1, ...)) on biased saturated samples.
// 2|p0-q0| + (|p1-q1| >> 1) <= E  <=>  |p1-q1| + 4|p0-q0| <= 2E + 1: one v_sad_u16 with the second difference as its
// accumulator.  lim2 = 2E + 1; -1 switches the edge off (the sum is >= 0).  The differences of biased samples are those
// of the signed samples (u ^ 0x80), and saturating the biased result is the format's s2u(c(...)).
__device__ __forceinline__ void simple_edge(int &p0, int &q0, int p1, int q1, int lim2) {
    const int sum = (int)__builtin_amdgcn_sad_u16((uint32_t)p1, (uint32_t)q1, (uint32_t)(ad(p0, q0) << 2));
    int w = c128(c128(p1 - q1) + __mul24(q0 - p0, 3));
    w = sum <= lim2 ? w : 0;
    w = imin(w, 123);   // c(w + 4) >> 3 and c(w + 3) >> 3 are both 15 from 123 on: one min for the two (w + 3 >= -125 below)
    q0 = satb(q0 - ((w + 4) >> 3));
    p0 = satb(p0 + ((w + 3) >> 3));
}

// One line of biased samples t[0..19] (t[0..3] precede the macroblock edge) through the MB edge and the three inner
// edges.  The four edges read and write disjoint samples (edge k: reads t[k-2..k+1], writes t[k-1], t[k]), so they are
// independent of each other and their order does not matter.  lim2_* as in simple_edge.
__device__ __forceinline__ void simple_line(int (&t)[20], int lim2_mb, int lim2_in) {
#pragma unroll
    for (int k = 4; k < 20; k += 4) simple_edge(t[k - 1], t[k], t[k - 2], t[k + 1], k == 4 ? lim2_mb : lim2_in);
}

struct SimpleFilter {
    static constexpr bool CHROMA = false;
    static constexpr bool LEVEL0_ENDS_PLANE = false;
    typedef int2 Lim;   // {2 mbedge_limit + 1, 2 sub_bedge_limit + 1}, -1 for level 0 (simple_edge)
    static __device__ __forceinline__ Lim limits(const int32_t *sd) {
        const bool on = sd[SD_LOOP_FILTER_LEVEL] != 0;   // level 0: the macroblock is skipped, the plane goes on
        return make_int2(on ? (sd[SD_MBEDGE_LIMIT] & 0xff) * 2 + 1 : -1, on ? (sd[SD_SUB_BEDGE_LIMIT] & 0xff) * 2 + 1 : -1);
    }
    struct Step { int lim_mb, lim_in; };
    static __device__ __forceinline__ Step step(const Lim &lim, bool inner, bool) { return Step{lim.x, inner ? lim.y : -1}; }
    static __device__ __forceinline__ void line(int (&t)[20], const Step &s, bool mb_edge) { simple_line(t, mb_edge ? s.lim_mb : -1, s.lim_in); }
};

__global__ __launch_bounds__(NWAVES * 64) void k_loop_filter_simple(Args a) { loop_filter_body<SimpleFilter>(a); }
__global__ __launch_bounds__(NWAVES * 64) void k_loop_filter_simple_b(BatchOf<Args> b) { loop_filter_body<SimpleFilter>(b.item[blockIdx.z]); }

}  // namespace lfs

bool loop_filter_simple_fits(int mbh) { return (mbh + 1 + lfb::ROWS - 1) / lfb::ROWS + 1 <= LF_SIMPLE_WORDS; }

void launch_loop_filter_simple(hipStream_t s, const FilterItem &it, int mbw, int mbh) {
    const lfb::Args a = lfb::make_args(s, it, LF_SIMPLE_WORD, mbw, mbh);
    VP8_LAUNCH(lfs::k_loop_filter_simple, dim3(a.nbands + (a.chk.on ? 1 : 0)), dim3(lfb::NWAVES * 64), 0, s, a);   // + the verdict workgroup
}

void launch_loop_filter_simple_batch(hipStream_t s, const FilterItem *items, int n, int mbw, int mbh) {
    lfb::launch_batch(lfs::k_loop_filter_simple_b, s, items, n, LF_SIMPLE_WORD, mbw, mbh);
}

}  // namespace vp8
