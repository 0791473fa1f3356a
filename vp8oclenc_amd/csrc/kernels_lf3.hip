// kernels_lf3.hip -- VP8 normal loop filter, form 3: the banded byte-tile body of lf_banded.h (see there for the data
// movement) under the normal filter's edges.  What batches of GOP chunks launch; one video uses form 4 (kernels_lf4.hip).
//
// Same arithmetic and ordering semantics as loop_filter_frame_luma/_chroma (CPU_kernels.cl:970-1075, :1333-1439; edge
// filters :829-926, lf_shared.h).  All three planes are filtered; the eight edge filters of a macroblock are a chain (an
// unsaturated carry from edge to edge, reference quirk, :1024/:1062).  A macroblock whose segment has loop_filter_level 0
// ends the plane (:990).
// History (1080p, one frame): v1 one wave per row through HBM 1.9 ms; v2 (git history) banded, two-step lag,
// writer wave 0.71 ms; this form 0.36 ms.
#include "lf_banded.h"

namespace vp8 {

namespace lf3 {

using namespace lfb;

// SAT: vp8hip_conformant_stream -- the registers handed from edge to edge saturate (lf_shared.h, filter_line)
template <bool SAT> struct NormalFilterT {
    static constexpr bool CHROMA = true;
    static constexpr bool LEVEL0_ENDS_PLANE = true;
    typedef int4 Lim;   // {interior limit, mb_delta, b_delta, hev threshold} (struct Limits)
    static __device__ __forceinline__ Lim limits(const int32_t *sd) {
        const int il = sd[SD_INTERIOR_LIMIT] & 0xff;
        return make_int4(il, il - (sd[SD_MBEDGE_LIMIT] & 0xff) * 2 - 1, il - (sd[SD_SUB_BEDGE_LIMIT] & 0xff) * 2 - 1, sd[SD_HEV_THRESHOLD] & 0xff);
    }
    // an edge that does not apply gets interior limit -1: its mask can never be true
    struct Step { Limits L; int int_lim, il4, il8; };   // il4, il8: the inner edges at 4 and at 8, 12 (chroma has none there)
    static __device__ __forceinline__ Step step(const Lim &lim, bool inner, bool luma) {
        Step s;
        s.int_lim = lim.x;
        s.L.mb_delta = lim.y;
        s.L.b_delta = lim.z;
        s.L.hev_thr = lim.w;
        s.il4 = inner ? s.int_lim : -1;
        s.il8 = inner && luma ? s.int_lim : -1;
        return s;
    }
    static __device__ __forceinline__ void line(int (&t)[20], const Step &s, bool mb_edge) { filter_line<SAT>(t, s.L, mb_edge ? s.int_lim : -1, s.il4, s.il8); }
};
typedef NormalFilterT<false> NormalFilter;

__global__ __launch_bounds__(NWAVES * 64) void k_loop_filter3_b(BatchOf<Args> b) { loop_filter_body<NormalFilter>(b.item[blockIdx.z]); }
__global__ __launch_bounds__(NWAVES * 64) void k_loop_filter3_b_conformant(BatchOf<Args> b) { loop_filter_body<NormalFilterT<true>>(b.item[blockIdx.z]); }

}  // namespace lf3

static bool lf_skip() {
    static const bool skip = experiment_skip("lf");
    return skip;   // timing experiment only
}

void launch_loop_filter3_batch(hipStream_t s, const FilterItem *items, int n, int mbw, int mbh, bool conformant) {
    lfb::launch_batch(conformant ? lf3::k_loop_filter3_b_conformant : lf3::k_loop_filter3_b, s, items, n, 0, mbw, mbh, lf_skip());
}

}  // namespace vp8
