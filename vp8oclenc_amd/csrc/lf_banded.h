// lf_banded.h -- the banded byte-tile loop filter: one kernel body for the normal filter's form 3 (kernels_lf3.hip, what
// batches launch) and the simple filter (kernels_lf_simple.hip), which differ in a filter policy only (gfx950).
//
// A loop filter is a chain of dependent edge filters: MB(x,y) needs MB(x-1,y) complete and, for its horizontal edges only,
// the vertical MB edge of MB(x+1,y-1).  A single wave issues one VALU instruction every ~5.5 cycles no matter what
// (scripts/ubench/valu_rates.hip), so the frame time is (steps on the critical path) x (instructions per step); both are
// what this body cuts:
//
//   * Each macroblock step has two phases: P1 = vertical edges (lane = pixel row, registers), P2 = horizontal
//     edges (lane = pixel column, through an LDS tile).  P2 of MB(x,y) needs only P1 of MB(x+1,y-1), so row y
//     runs ONE macroblock behind row y-1 (x = S - r at step S) with a hand-off in the middle of the step:
//     mb_w + mb_h steps per frame instead of mb_w + 2*mb_h.
//   * A workgroup owns a band of ROWS MB rows; a wave runs two rows (32 lanes each: 0-15 luma, 16-23 U,
//     24-31 V), so every second hand-off is inside a wave and costs nothing.
//   * Branch-free edge filters: edges that do not apply (frame border, chroma lanes, skipped inner edges,
//     level 0) run with their limit forced to -1 instead of being jumped over, which removes the
//     divergent control flow (and its register shuffling) from the instruction stream.
//   * Bottom strips of each row live in an LDS ring.  A finished 16x16 block (shifted by (-4,-4)) is stored to
//     HBM by its own row at the top of the NEXT step, right behind the prefetch of the next macroblock, so the
//     stores have a full step to retire before the wave waits on vmcnt again (gfx9 counts loads and stores in
//     one counter).  The strip between bands goes through the frame (sc1 = write-through) with a loader and a
//     publisher wave per band; the loader also stores the rows it loaded once row 0 has filtered across them,
//     because a write-through store takes longer than a step to retire.
//   * One LDS poll per step (middle of the step) covers every dependency.
//
// A filter policy is a struct of compile-time constants and static functions (NormalFilter in kernels_lf3.hip,
// SimpleFilter in kernels_lf_simple.hip):
//   CHROMA             U and V are filtered and stored.  If not, their lanes of the lane map stay, with every edge off, and
//                      store nothing (publisher, loader and worker drain): U and V are never written.
//   LEVEL0_ENDS_PLANE  a macroblock whose segment has loop_filter_level 0 ends the plane (the reference's normal filter,
//                      CPU_kernels.cl:990).  If not, what level 0 means is up to limits() (the simple filter: edges off).
//   Lim, limits(sd)    a segment's entry of the limit table in LDS, made from its segment data
//   Step, step(lim, inner, luma)
//                      what the two phases of a macroblock step need of that entry: inner = the macroblock's inner edges are
//                      filtered (it is filtered at all and the filter mask says so), luma = the lane is a luma lane
//   line(t, step, mb_edge)
//                      one line of twenty biased samples through the MB edge (if mb_edge) and the three inner edges
// Every choice is `if constexpr` or a constant: no run-time branch or select enters the step loop for it.
#pragma once
#include "lf_shared.h"

namespace vp8 {
namespace lfb {

using namespace lf;

constexpr int WORKERS = 4;             // worker waves per band (one per SIMD)
constexpr int ROWS = 2 * WORKERS;      // MB rows per band
constexpr int RING_MB = 16;            // strip ring length in macroblocks
// One layout for all three planes (chroma simply uses half of it), so that every LDS access of the worker
// loop is base + immediate offset and nothing in it depends on the plane of the lane:
constexpr int SROW = RING_MB * 16;                     // strip row stride; ring width = RING_MB * msz pixels
constexpr int STRIP_PLANE = 4 * SROW;                  // four pixel rows per plane
constexpr int STRIP_BYTES = 3 * STRIP_PLANE;           // Y, U, V bottom strips of one MB row
constexpr int TILE_S = 24;                             // work-tile row stride: 4 carried columns + 16 + pad
constexpr int TILE_PLANE = 16 * TILE_S;
constexpr int TILE_BYTES = 3 * TILE_PLANE;
constexpr int TILE_SLOTS = 2;          // a finished tile is drained to HBM at the top of the next step
constexpr int NWAVES = WORKERS + 2;    // workers + loader + publisher

enum { F_TOP = WORKERS, F_PUB, F_ABORT = 7 };   // flag[0..WORKERS-1] = 2*step + phase of each worker

__device__ __forceinline__ uint32_t pack4(int a, int b, int c, int d) {
    const uint32_t lo = __builtin_amdgcn_perm((uint32_t)satb(b), (uint32_t)satb(a), 0x0c0c0400u);
    const uint32_t hi = __builtin_amdgcn_perm((uint32_t)satb(d), (uint32_t)satb(c), 0x0c0c0400u);
    return __builtin_amdgcn_perm(hi, lo, 0x05040100u);
}
__device__ __forceinline__ int ub(uint32_t w, int k) { return byte_of(w, k) | BIAS; }

__device__ __forceinline__ uint32_t ld_sc1(const uint32_t *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_sc1(uint32_t *p, uint32_t v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
constexpr int WAIT_LGKM0 = 0xc07f;   // s_waitcnt lgkmcnt(0) as the builtin's immediate: the compiler's own waitcnt pass sees it
#define LF_WAIT(cond_unsatisfied, nap) LF_BOUNDED_WAIT(cond_unsatisfied, nap, false)

struct Args {
    Plane Y, U, V;
    MBOut o;
    SegData *sd;      // read; written only by the verdict workgroup when check_SSIM's filter update applies (chk)
    LfCheck chk;
    int32_t *gprog;   // [bands] gbase + macroblocks of the band's bottom strip published so far
    int gbase;        // counters only grow: launch n uses the range (n*(mbw+2), (n+1)*(mbw+2)], so no memset
    int mbw, mbh, nbands;
    int32_t *err;     // set to 1 if a bounded wait expired (the host reports VP8HIP_ERR_TIMEOUT)
};
static_assert(sizeof(BatchOf<Args>) <= 4096, "a batch's argument blocks travel in the 4 KiB kernel-argument segment");

template <typename Filter> struct Shared {
    uint8_t strip[ROWS + 1][STRIP_BYTES];         // strip[r] = bottom rows of the MB row ABOVE local row r
    uint8_t tile[ROWS][TILE_SLOTS][TILE_BYTES];   // work tiles: this step's and the previous one's (being drained)
    int flag[8];                                  // worker progress, F_TOP, F_PUB; [F_ABORT]: a bounded wait expired somewhere in
                                                  // this workgroup, everybody leaves.  Read and written through `flag` below.
    uint32_t dummy[WORKERS * 64];                 // sink for stores of lanes that have nothing to store
    SegData sd;                                   // the segment data check_SSIM's filter update gives, when it applies (chk)
    float red[8];
    int repl;
    int first_lf0;                                // LEVEL0_ENDS_PLANE: first macroblock whose segment has loop_filter_level 0 (:990)
    typename Filter::Lim lim[4];                  // per segment, see Filter::limits
};

template <typename Filter> __device__ __forceinline__ void loop_filter_body(const Args &a) {
    __shared__ __attribute__((aligned(16))) Shared<Filter> sh;
    const int band = blockIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    lds_flag_t *const flag = (lds_flag_t *)sh.flag;
    if (threadIdx.x < 8) flag[threadIdx.x] = 0;
    if constexpr (Filter::LEVEL0_ENDS_PLANE) {
        if (threadIdx.x == 0) sh.first_lf0 = 0x7fffffff;
    }
    const int32_t *sdv = a.sd->v;
    if (a.chk.on) {
        sdv = check_ssim_segments<NWAVES>(a, sh, wave);
        if (band >= a.nbands) {   // the workgroup behind the last band: the strips and tiles are its staging area
            static_assert(sizeof(sh.strip) + sizeof(sh.tile) >= VERDICT_CHUNK * sizeof(float), "staging area");
            verdict_workgroup<NWAVES>(a, sh, sdv != a.sd->v, reinterpret_cast<float *>(&sh.strip[0][0]));
            return;
        }
    } else if (band >= a.nbands) {
        return;
    }
    if (threadIdx.x < 4)   // a table read per macroblock: selecting among four registers by a per-lane index compiles to branches
        sh.lim[threadIdx.x] = Filter::limits(sdv + threadIdx.x * SD_INTS);
    // The launch clock (lf_shared.h): band 0 stamps the start, the wave that runs the frame's last row (the virtual flush row)
    // adds end - start.
    unsigned long long *clk = reinterpret_cast<unsigned long long *>(a.err + 4);
    if (band == 0 && threadIdx.x == 0) __hip_atomic_store(clk, __builtin_amdgcn_s_memrealtime(), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long cyc0 = __builtin_amdgcn_s_memtime(), tick0 = __builtin_amdgcn_s_memrealtime();
    const uint32_t hwid0 = hw_slot();
    __syncthreads();
    const int mbw = a.mbw, mbh = a.mbh;
    const int band_row0 = band * ROWS;
    if constexpr (Filter::LEVEL0_ENDS_PLANE) {
        // Levels are >= 1 for every quantizer the host produces, so the scan over segment ids runs only if one IS zero.
        const bool any0 = sdv[SD_LOOP_FILTER_LEVEL] == 0 || sdv[SD_INTS + SD_LOOP_FILTER_LEVEL] == 0 ||
                          sdv[2 * SD_INTS + SD_LOOP_FILTER_LEVEL] == 0 || sdv[3 * SD_INTS + SD_LOOP_FILTER_LEVEL] == 0;
        if (any0) {
            int first = 0x7fffffff;
            for (int mb = threadIdx.x; mb < mbw * mbh; mb += NWAVES * 64)
                if (sdv[a.o.seg[mb] * SD_INTS + SD_LOOP_FILTER_LEVEL] == 0) { first = mb; break; }
            if (first != 0x7fffffff) atomicMin(&sh.first_lf0, first);
            __syncthreads();
        }
    }

    // ---------------------------------------------------------------------------------------------
    // publisher wave: bottom strip of the band's last row (strip[ROWS]) -> the frame (sc1, write-
    // through) -> HBM counter.  Keeps the store drain (s_waitcnt vmcnt(0)) off the workers' path.
    // ---------------------------------------------------------------------------------------------
    if (wave == WORKERS + 1) {
        if (band + 1 >= a.nbands) return;
        // lane < 44: one dword of 4 rows x (5 + 3 + 3) dwords = columns x0-4 .. x0+msz-1 of Y, U, V; without CHROMA only the
        // luma lanes (< 20) store (the next band's loader reads U and V from the frame as they are)
        constexpr int STORE_LANES = Filter::CHROMA ? 44 : 20;
        const int pl = lane < 20 ? 0 : (lane < 32 ? 1 : 2);
        const int k = pl == 0 ? lane : (pl == 1 ? lane - 20 : lane - 32);
        const int ndw = pl == 0 ? 5 : 3;
        const int rr = k / ndw, j = k % ndw;
        const Plane &P = pl == 0 ? a.Y : (pl == 1 ? a.U : a.V);
        const int msz = pl == 0 ? 16 : 8, rmask = RING_MB * msz - 1;
        const int y = (band_row0 + ROWS - 1) * msz + (msz - 4) + rr;
        const uint8_t *sp = sh.strip[ROWS] + pl * STRIP_PLANE + rr * SROW;
        for (int x = 0; x <= mbw; ++x) {
            const int done = 2 * (x + ROWS - 1) + 2;   // the last row has finished macroblock x
            LF_WAIT(flag[WORKERS - 1] < done, 3)
            if (lane < STORE_LANES) {
                const uint32_t v = *reinterpret_cast<const uint32_t *>(sp + ((x * msz - 4 + 4 * j) & rmask));
                st_sc1(reinterpret_cast<uint32_t *>(P.p + (ptrdiff_t)y * P.stride + x * msz - 4) + j, v);
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            if (lane == 0) {
                flag[F_PUB] = x + 1;
                __hip_atomic_store(&a.gprog[band], a.gbase + x + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        return;
    }

    // ---------------------------------------------------------------------------------------------
    // loader wave: previous band's bottom strip (in the frame, written with sc1) -> strip[0]
    // ---------------------------------------------------------------------------------------------
    if (wave == WORKERS) {
        if (band == 0) return;
        const int l = lane & 31;
        // lane l < 32: one dword of the 4 x (16 + 8 + 8) pixels above macroblock x
        const int pl = l < 16 ? 0 : (l < 24 ? 1 : 2);
        const int k = pl == 0 ? l : (pl == 1 ? l - 16 : l - 24);     // dword index inside the plane's 4 rows
        const int nd = pl == 0 ? 4 : 2;                               // dwords per row
        const int r = k / nd, j = k % nd;
        const Plane &P = pl == 0 ? a.Y : (pl == 1 ? a.U : a.V);
        const int msz = pl == 0 ? 16 : 8, rmask = RING_MB * msz - 1;
        const int y = band_row0 * msz - 4 + r;
        uint8_t *sp = sh.strip[0] + pl * STRIP_PLANE + r * SROW;
        uint8_t *gp = P.p + (ptrdiff_t)y * P.stride + 4 * j;
        // The four pixel rows above this band share cache lines with the previous band's hand-off, so every access
        // to them inside the launch is sc1 -- including their final store once row 0 has filtered across them.
        // That store is done here, not by worker 0: a write-through store takes longer than a step to retire and
        // would sit in front of every vmcnt wait of the worker.  Block m = columns m0-4 .. m0+msz-5, final when
        // row 0 has finished macroblock m (row 0: step == macroblock).
        constexpr int DRAIN_LANES = Filter::CHROMA ? 32 : 16;
#define DRAIN_TOP(m)                                                                                        \
    {                                                                                                       \
        LF_WAIT(flag[0] < 2 * (m) + 2, 8)                                                                    \
        if (lane < DRAIN_LANES) st_sc1(reinterpret_cast<uint32_t *>(gp + (m) * msz - 4),                    \
                              *reinterpret_cast<const uint32_t *>(sp + (((m) * msz - 4 + 4 * j) & rmask))); \
    }
        for (int x = 0; x < mbw; ++x) {
            // columns x0+13..15 are final once the previous band's last row has run P1 of macroblock x+1
            const int need = imin(x + 2, mbw + 1);
            LF_WAIT(__hip_atomic_load(&a.gprog[band - 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - a.gbase < need, 2)
            // ring space: the slot still holds macroblock x-RING_MB, whose last four columns belong to the block
            // of macroblock x-RING_MB+1
            if (x >= RING_MB - 1) DRAIN_TOP(x - (RING_MB - 1))
            if (lane < 32) *reinterpret_cast<uint32_t *>(sp + ((x * msz + 4 * j) & rmask)) = ld_sc1(reinterpret_cast<const uint32_t *>(gp + x * msz));
            lds_fence();
            if (lane == 0) flag[F_TOP] = x + 1;
        }
        for (int m = imax(mbw - (RING_MB - 1), 0); m <= mbw; ++m) DRAIN_TOP(m)
#undef DRAIN_TOP
        return;
    }

    // ---------------------------------------------------------------------------------------------
    // worker waves
    // ---------------------------------------------------------------------------------------------
    // the loader and publisher waves share SIMDs with workers 0 and 1: let them issue only in idle slots
    __builtin_amdgcn_s_setprio(3);
    const int half = lane >> 5, l32 = lane & 31;
    const int r = 2 * wave + half;              // local MB row
    const int gr = band_row0 + r;               // global MB row (gr == mbh: virtual row that only flushes)
    const bool row_real = gr < mbh, row_any = gr <= mbh;
    const int pl = l32 < 16 ? 0 : (l32 < 24 ? 1 : 2);
    const int li = pl == 0 ? l32 : (pl == 1 ? l32 - 16 : l32 - 24);
    const int msz = pl == 0 ? 16 : 8, nd = msz / 4;
    const Plane &P = pl == 0 ? a.Y : (pl == 1 ? a.U : a.V);
    const int rmask = RING_MB * msz - 1;
    uint8_t *top = sh.strip[r] + pl * STRIP_PLANE;       // 4 rows: bottom of the row above
    uint8_t *bot = sh.strip[r + 1] + pl * STRIP_PLANE;   // 4 rows: our own bottom rows
    // P1 hands columns x0-4..x0-1 of the bottom four pixel rows to the row below; the other lanes aim the
    // same store at a private dummy word instead of branching around it
    const bool bottom_lane = li >= msz - 4;
    uint8_t *botw = bottom_lane ? bot + (li - (msz - 4)) * SROW : reinterpret_cast<uint8_t *>(&sh.dummy[lane]);
    const int botw_mask = bottom_lane ? rmask : 0;
    const int tile_lane = pl * TILE_PLANE + li * TILE_S;    // this lane's row of the tile (P1)
    const int tile_col = pl * TILE_PLANE + 4 + li;          // this lane's column of the tile (P2)
    // Drain: the block that became final in a step -- 16x16 (8x8) shifted by (-4,-4) = four pixel rows of the
    // strip above (lanes li < 4) + msz-4 rows of the tile (lanes li >= 4) -- is stored at the top of the NEXT
    // step, right behind the prefetch, so the stores have a whole step to retire before anything waits on vmcnt.
    const bool from_top = li < 4;
    const bool drain_lane = (Filter::CHROMA || pl == 0) && row_any && (from_top ? gr > 0 && !(r == 0 && band > 0) : row_real);   // (the loader stores those)
    const uint8_t *dr_src = from_top ? top + li * SROW : sh.tile[r][0] + pl * TILE_PLANE + (li - 4) * TILE_S;
    const int dr_slot = from_top ? 0 : TILE_BYTES;          // tile lanes alternate between the two slots
    const int dr_and = from_top ? rmask : 0xffff;            // strip lanes wrap around the ring
    const int dr_col = from_top ? -1 : 0;                    // ... and start at column x0-4
    uint8_t *dr_g = P.p + (ptrdiff_t)(gr * msz - 4 + li) * P.stride - 4;
    const bool has_top = gr > 0;
    const bool publishes = band + 1 < a.nbands;   // a next band exists: every row of this band is real
    [[maybe_unused]] int first_lf0 = 0x7fffffff;
    if constexpr (Filter::LEVEL0_ENDS_PLANE) first_lf0 = sh.first_lf0;
    // Prefetch of macroblock 0.  Every lane loads 16 bytes (chroma lanes use 8 of them; at the right frame edge
    // the rest is margin).  The loads stay inside a branch on purpose: hoisted to the top of the loop body, hipcc
    // parks an s_waitcnt vmcnt(0) right behind them (measured: +700 cycles per step).
    const uint8_t *pf_p = P.p + (ptrdiff_t)(imin(gr, mbh - 1) * msz + li) * P.stride;
    const int32_t *pf_seg = a.o.seg + imin(gr, mbh - 1) * mbw, *pf_mask = a.o.mask + imin(gr, mbh - 1) * mbw;
    uint4 nxt = make_uint4(0, 0, 0, 0);
    int nxt_seg = 0, nxt_mask = 0;
    if (row_real) {
        nxt = *reinterpret_cast<const uint4 *>(pf_p);
        nxt_seg = pf_seg[0];
        nxt_mask = pf_mask[0];
    }
    uint32_t left4 = 0;
    const int steps = mbw + ROWS + 1;   // + one step that only drains
    for (int S = 0; S < steps; ++S) {
        uint8_t *tile = sh.tile[r][S & 1];
        const int x = S - r;
        // (`&`, not `&&`: one predicate, one exec mask -- short-circuit evaluation nests the regions)
        const bool p1_on = row_real & (x >= 0) & (x <= mbw);   // a real macroblock or the flush column behind the last one
        const bool mbstep = p1_on & (x < mbw);
        const int x0 = x * msz;
        // the prefetched macroblock is unpacked HERE, before the next prefetch is issued into the same registers: taking a
        // copy of the sixteen bytes + segment + mask instead cost nine moves per step
        int t[20];
#pragma unroll
        for (int k = 0; k < 16; ++k) t[4 + k] = ub(k < 4 ? nxt.x : (k < 8 ? nxt.y : (k < 12 ? nxt.z : nxt.w)), k & 3);
        const int seg = nxt_seg, maskv = nxt_mask;
        // (Under a predicate on purpose.  Unconditional loads from a clamped position would save the moves that keep the old
        // registers alive for the lanes that do not load, but hipcc then waits for the loads it has just issued -- s_waitcnt
        // vmcnt(4) and vmcnt(3) a few instructions further down: +9 % on the whole kernel.)
        if (mbstep & (x + 1 < mbw)) {   // prefetch the next macroblock of this row
            nxt = *reinterpret_cast<const uint4 *>(pf_p + x0 + msz);
            nxt_seg = pf_seg[x + 1];
            nxt_mask = pf_mask[x + 1];
        }
        if (drain_lane & (x >= 1) & (x <= mbw + 1)) {   // the block of macroblock x-1 (or the flush column)
            const int c0 = ((x - 1) * msz - 4) & dr_col;
            const uint8_t *src = dr_src + ((S - 1) & 1) * dr_slot;
            uint32_t v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = *reinterpret_cast<const uint32_t *>(src + ((c0 + 4 * j) & dr_and));
            uint32_t *g = reinterpret_cast<uint32_t *>(dr_g + (x - 1) * msz);
            *reinterpret_cast<uint2 *>(g) = make_uint2(v[0], v[1]);
            if (pl == 0) *reinterpret_cast<uint2 *>(g + 2) = make_uint2(v[2], v[3]);
        }
        // an edge that does not apply (frame border, chroma lanes, skipped inner edges, level 0) gets limit -1
        const typename Filter::Lim lim = sh.lim[seg & 3];
        bool do_filter = mbstep;
        if constexpr (Filter::LEVEL0_ENDS_PLANE) do_filter = mbstep & ((gr * mbw + x) < first_lf0);
        if constexpr (!Filter::CHROMA) do_filter = do_filter & (pl == 0);
        const typename Filter::Step fs = Filter::step(lim, do_filter & (maskv != 0), pl == 0);
        uint32_t *trow = reinterpret_cast<uint32_t *>(tile + tile_lane);
        // ---- P1: vertical edges, lane = pixel row, in registers ---------------------------------
        // The flush column (x == mbw) takes the same path with every edge off: the filters are then the identity and the
        // carried four columns land in the tile's first dword unchanged; the rest of its tile row is margin.
        if (p1_on) {
#pragma unroll
            for (int k = 0; k < 4; ++k) t[k] = ub(left4, k);
            Filter::line(t, fs, do_filter & (x > 0));
            const uint32_t d0 = pack4(t[0], t[1], t[2], t[3]);
            trow[0] = d0;
#pragma unroll
            for (int j = 1; j < 5; ++j) trow[j] = pack4(t[4 * j], t[4 * j + 1], t[4 * j + 2], t[4 * j + 3]);
            // the row below reads columns x0-4..x0-1 of our bottom rows in P2 of this very step
            *reinterpret_cast<uint32_t *>(botw + ((x0 - 4) & botw_mask)) = d0;
        }
        __builtin_amdgcn_s_waitcnt(WAIT_LGKM0);
        flag[wave] = 2 * S + 1;   // (every lane, the same word: no exec mask to set up and restore)
        // ---- the one poll of the step ------------------------------------------------------------
        {
            const int need_up = 2 * S + 1;                       // P1 of the rows above (their macroblock x+1)
            // ring space below: our second row is about to overwrite, in its bottom strip, the slot of macroblock
            // x-RING_MB, whose last columns the wave below stores at the top of its step S-(RING_MB-3)
            const int need_dn = wave + 1 < WORKERS ? 2 * (S - (RING_MB - 3)) + 1 : 0;
            const int x_r0 = S - 2 * wave;                        // macroblock of this wave's first row
            const bool top_dep = wave == 0 && band > 0 && x_r0 >= 0 && x_r0 <= mbw && band_row0 <= mbh;
            const int need_top = imin(x_r0 + 1, mbw);
            // last wave: the publisher must have drained what the second row is about to overwrite in strip[ROWS]
            const int need_pub = (wave + 1 == WORKERS && publishes) ? S - (ROWS - 1) - (RING_MB - 2) : 0;
            // Everything the poll compares is the same in all lanes; readfirstlane says so to the compiler, which otherwise
            // builds the loop out of exec-mask bookkeeping (a third of the poll's instructions on the path of every step).
            const int up = imax(wave - 1, 0), dn = imin(wave + 1, WORKERS - 1);
            for (int spins = 0;; ++spins) {
                // (unconditional loads: five ds_read_b32 in flight at once)
                const int f_up = flag[up], f_dn = flag[dn], f_top = flag[F_TOP], f_pub = flag[F_PUB], f_abort = flag[F_ABORT];
                const bool ok = (wave == 0 || f_up >= need_up) && (wave + 1 == WORKERS || f_dn >= need_dn) && (!top_dep || f_top >= need_top) &&
                                f_pub >= need_pub;
                const int state = __builtin_amdgcn_readfirstlane(f_abort ? 2 : (ok ? 1 : 0));
                if (state == 1) break;
                if (state == 2) return;
                if (spins > SPIN_LIMIT) { flag[F_ABORT] = 1; *a.err = 1; }
                if (spins < 32) asm volatile("s_nop 3"); else __builtin_amdgcn_s_sleep(1);   // the flag is usually a few hundred cycles away: a tight poll first, naps when it is not
            }
        }
        // ---- P2: horizontal edges, lane = pixel column ---------------------------------------------
        if (mbstep) {
            int t[20];
            const int rc = (x0 + li) & rmask;
            uint8_t *tp = top + rc, *bp = bot + rc, *tc = tile + tile_col;
#pragma unroll
            for (int k = 0; k < 4; ++k) t[k] = (int)tp[k * SROW];
#pragma unroll
            for (int k = 0; k < 16; ++k) t[4 + k] = (int)tc[k * TILE_S];   // chroma lanes: rows 8-15 are don't-care
            __builtin_amdgcn_s_waitcnt(WAIT_LGKM0);   // one wait for the twenty loads instead of one per use
#pragma unroll
            for (int k = 0; k < 20; ++k) t[k] |= BIAS;
            Filter::line(t, fs, do_filter & has_top);
            // rows 1-3 of the strip above (row 0 of the frame: a scratch strip nobody reads)
            tp[1 * SROW] = (uint8_t)satb(t[1]); tp[2 * SROW] = (uint8_t)satb(t[2]); tp[3 * SROW] = (uint8_t)satb(t[3]);
            int s[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) { s[k] = satb(t[4 + k]); tc[k * TILE_S] = (uint8_t)s[k]; }
#pragma unroll
            for (int j = 0; j < 4; ++j) bp[j * SROW] = (uint8_t)(pl == 0 ? s[12 + j] : s[4 + j]);   // our bottom rows -> row below
            left4 = trow[nd];   // columns msz-4 .. msz-1 of this macroblock after both phases (next P1's left side)
        }
        __builtin_amdgcn_s_waitcnt(WAIT_LGKM0);
        flag[wave] = 2 * S + 2;
    }
    if (gr == mbh && l32 == 0) {   // the frame's last row: this wave is the last to finish real work
        const unsigned long long t0 = __hip_atomic_load(clk, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned long long t1 = __builtin_amdgcn_s_memrealtime();
        atomicAdd(clk + 1, t1 - t0);
        atomicAdd(clk + 2, 1ull);
        const unsigned long long ratio = (__builtin_amdgcn_s_memtime() - cyc0) * 1000ull / (t1 - tick0 + 1);
        LF_CLOCK_RATIO(clk, ratio, hwid0)
    }
}

// The argument block of one launch.  counter_word: where in the progress buffer this filter's band counters sit; they and
// launch_no are a filter's own, so launches of the other forms in between leave its windows valid.
inline Args make_args(hipStream_t s, const FilterItem &it, int counter_word, int mbw, int mbh) {
    Args a;
    a.chk = it.chk;      // (only `on` is read when it is 0)
    a.Y = it.recon->Y[0];
    a.U = it.recon->U;
    a.V = it.recon->V;
    a.o = *it.out;
    a.sd = it.sd;
    a.gprog = it.progress + counter_word;
    a.mbw = mbw;
    a.mbh = mbh;
    a.nbands = (mbh + 1 + ROWS - 1) / ROWS;   // + the virtual flush row
    a.gbase = lf_window_base(it.launch_no, mbw);
    if (a.gbase == 0) (void)hipMemsetAsync(a.gprog, 0, sizeof(int32_t) * (a.nbands + 1), s);
    a.err = it.progress + LF_ERR_WORD;
    return a;
}

// One launch for a batch: blockIdx.z = the batch's item; + the verdict workgroup if check_SSIM rides with any of them.
// skip: everything but the launch itself (a timing experiment).
template <typename Kernel>
inline void launch_batch(Kernel kernel, hipStream_t s, const FilterItem *items, int n, int counter_word, int mbw, int mbh, bool skip = false) {
    BatchOf<Args> b;
    b.n = n;
    bool any = false;
    for (int i = 0; i < n; ++i) {
        b.item[i] = make_args(s, items[i], counter_word, mbw, mbh);
        any = any || b.item[i].chk.on;
    }
    if (skip) return;
    VP8_LAUNCH(kernel, dim3(b.item[0].nbands + (any ? 1 : 0), 1, n), dim3(NWAVES * 64), 0, s, b);
}

}  // namespace lfb
}  // namespace vp8
