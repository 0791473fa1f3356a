// kernels_s2.hip -- quarter-pel refinement (luma_search_2step, src/GPU_kernels.cl:1094-1203): the two six-tap passes as int8
// products on the matrix cores, the block match on the vector ALUs, lane = candidate.
//
// The search kernels are VALU-issue bound on gfx950 (scripts/ubench/valu_cost.hip, profiles/r04_issue_cycles_by_opcode.json), so
// the kernel is built around what the vector pipe has to issue.  Pixels travel as signed bytes p - 128: every tap set sums to 128,
// so a filter pass computes sum((p - 128) * f) = sum(p * f) - 128 * 128 and sat_i8((sum + 64) >> 7) IS the biased byte of the
// reference's clamped sample (v_ashr_pk_i8_i32: no bias to undo).
//   * 32 lanes per 8x8 block (2 blocks per wave, 8 per workgroup).  In batches a workgroup takes its blocks through every enabled
//     reference of its context, one after the other (grid y = 1): the blocks' coordinates, the current block's load and byte scatter
//     and its share of the metric are made once for the two or three of them.  One video: one reference per blockIdx.y.
//   * The 16 x 32-byte window around the 1x winner is staged in LDS by ONE unaligned 16-byte global load per lane (the window
//     starts at its own first byte).
//   * Horizontal pass = one v_mfma_i32_32x32x32_i8: A = the two blocks' window rows, B = the taps of the four fractional x cases
//     x 8 columns (a constant operand table, make_bh below), the rounding 64 as one more product (k = 31: mfma_round).  A lane comes out with a
//     column and four groups of four consecutive rows = four dwords of the TRANSPOSED H array, which go to LDS.
//   * Vertical pass = three MFMAs over the wave's 2 x 5 x 8 columns: A = the taps of the four y cases (make_av), B = 32 columns of
//     16 bytes, one ds_read_b128 each; a lane comes out with, per y case, one dword of the prediction: four rows of one column, stored
//     [4x4 block][candidate][column] so that a (candidate, 4x4 block) task of the cost phase is 16 contiguous bytes.  The whole-pel cases
//     are copies, and the zero-vector block is candidate 25 of the same array.
//   * Then lane k = candidate (dx, dy) of the 25 (+ the zero-vector candidate): the block-match metric on four 4x4 blocks, the
//     current block's share of its column pass made once per block into LDS (weight_pre_block) and the column pass of 64 (candidate,
//     4x4 block) tasks of a wave as ONE more MFMA, the current block's share its C input (weight_mfma, vp8hip_dev.h); the minimum over
//     the 32 lanes by four DPP steps + one ds_swizzle, in every lane, over a key whose low byte holds the candidate's number as
//     (dy + 2) * 8 + (dx + 2): keys are unique in a block, and the lane whose own key is the minimum writes the block's result from what it holds.
// The operand and result lane maps of the MFMA are pinned by scripts/ubench/mfma_i8_layout.hip, the results by the whole parity
// suite.  History per 1080p frame and reference: 32-bit multiply-adds 0.156 ms; both passes on v_dot4_i32_i8 0.091 (892 vector
// instructions per wave; git history, ae32ece^); with the metric's column pass on the matrix cores 522 vector instructions per wave, group of
// eight blocks and reference; with the reference loop 475 per reference + 53 per group = 493 at three references
// (tests/test_search2_instruction_budget.py); with the row butterfly of rows 0 and 2 of the metric folded into its MFMA 443 per reference + 70 per
// group = 466 (tests/test_metric_instruction_budget.py); with the filter bytes packed without permutes (round_pack4) and the result written by the
// winning lane 411 per reference (392 issued: the rest is a branch waves skip) + 69 per group = 434 (tests/test_search2_pack_tail_budget.py); with
// the lane addresses of a reference's head read from a table (s2_lane_layout.h) and its global loads addressed by a uniform base and a 32-bit lane
// offset 371 per reference + 75 per group = 396 (tests/test_search_lane_budget.py).
#include <stdlib.h>
#include <string.h>

#include "vp8hip_dev.h"
#include "kernels_rc_dev.h"
#include "s2_lane_layout.h"

namespace vp8 {

namespace {

constexpr uint32_t pk8(int a, int b, int c, int d) {
    return (uint32_t)(a & 255) | ((uint32_t)(b & 255) << 8) | ((uint32_t)(c & 255) << 16) | ((uint32_t)(d & 255) << 24);
}
// the six taps of quarter-pel offset -2..2 (phases 4, 6, (0), 2, 4 of the 1/8-pel table, GPU_kernels.cl:563-572); case 2 is the copy
constexpr int TAPS[5][6] = {{3, -16, 77, 77, -16, 3}, {1, -8, 36, 108, -11, 2}, {0, 0, 128, 0, 0, 0}, {2, -11, 108, 36, -8, 1}, {3, -16, 77, 77, -16, 3}};
// The two six-tap passes as products on the matrix cores (v_mfma_i32_32x32x32_i8: D[32][32] = A[32][32] . B[32][32] + C, signed bytes
// in, int32 out -- exact; lane maps checked by scripts/ubench/mfma_i8_layout.hip).  A filter pass IS a banded matrix product:
//   horizontal: D[window row][(x case, column)] = sum_k window[row][k] * BH[k][(x case, column)],  BH[k][n] = tap_xc[k - c - s]
//   vertical:   D[(y case, row)][column]        = sum_k AV[(y case, row)][k] * H[k][column],       AV[m][k] = tap_yc[k - i - s]
// (s = 1 for the positive offsets, whose six taps start one sample later).  A lane holds 16 consecutive k of one row (A) or one
// column (B): lanes 0-31 k = 0..15, lanes 32-63 k = 16..31.
struct OperandTable { uint32_t w[64][4]; };
constexpr OperandTable make_bh() {   // B of the horizontal pass: lane l -> column n = l & 31 = xi * 8 + c, k = 16 * (l >> 5) + j
    OperandTable t{};
    for (int l = 0; l < 64; ++l) {
        const int n = l & 31, xi = n >> 3, c = n & 7, xc = xi + (xi >> 1), s = xc >= 2 ? 1 : 0;
        for (int j = 0; j < 16; ++j) {
            const int k = 16 * (l >> 5) + j, tap = k - c - s;
            const int v = k == 31 ? 64 : (tap >= 0 && tap < 6) ? TAPS[xc][tap] : 0;      // k = 31: the rounding (see mfma_round)
            t.w[l][j >> 2] |= (uint32_t)(v & 255) << (8 * (j & 3));
        }
    }
    return t;
}
constexpr OperandTable make_av() {   // A of the vertical pass: lane l -> row m = l & 31 = f * 8 + i (y case f + (f >> 1)), k = 16 * (l >> 5) + j
    OperandTable t{};
    for (int l = 0; l < 64; ++l) {
        const int m = l & 31, f = m >> 3, i = m & 7, yc = f + (f >> 1), s = yc >= 2 ? 1 : 0;
        for (int j = 0; j < 16; ++j) {
            const int k = 16 * (l >> 5) + j, tap = k - i - s;
            const int v = k == 31 ? 64 : (tap >= 0 && tap < 6) ? TAPS[yc][tap] : 0;
            t.w[l][j >> 2] |= (uint32_t)(v & 255) << (8 * (j & 3));
        }
    }
    return t;
}
static __device__ __constant__ const OperandTable K_BH = make_bh();
static __device__ __constant__ const OperandTable K_AV = make_av();

// The layout constants of the three LDS arrays (HT_XC, V_CAND, V_ROW, V_SLOT, V_ZERO, PRE_SLOT, WIN_ROW) and every lane's place in them: s2_lane_layout.h.
// What of it a wave would compute again for every reference, it reads from this table instead: lane t's row, the fields 16 bits each.
static __device__ __constant__ const S2LaneTable K_S2_LANE = make_s2_lane();
typedef int v2i __attribute__((ext_vector_type(2)));
template <class T>
__device__ __forceinline__ T *lds_at(uint32_t *array, uint32_t bytes) { return reinterpret_cast<T *>(reinterpret_cast<char *>(array) + bytes); }
// Every LDS array of the kernel is indexed by the block's slot g, and the two blocks of a wave sit in ITS lanes: the stages
// hand data over inside a wave, so a wave-level "my LDS writes have landed" is all the synchronisation there is
__device__ __forceinline__ void lds_fence() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

struct S2Args {
    Plane cur;
    Plane ref[3];
    const int16_t *net_in[3];
    int16_t *net_out[3];
    int32_t *bdiff[3];
    int refmap[3];
    int nrefs;       // enabled references of this context (a batched launch is sized for the largest of its contexts)
    int w, h, nblk, bw;
    uint32_t bw_inv;   // ceil(2^32 / bw)
    unsigned long long *clk;   // launch clock (launch_clock_end, vp8hip_dev.h) or nullptr; a batched launch uses its first member's
};

// minimum over the 32 lanes of a block, in every one of them: four DPP steps inside the 16-lane rows (the lanes a step pairs hold, after
// it, the same value: mirrors do as well as butterflies), then the two rows of the block trade their minima through ds_swizzle_b32 (lane ^ 16
// inside each group of 32: the LDS crossbar, no memory and no vector instruction -- DPP has no step that reaches the LOWER row).
// (__shfl_xor is a ds_bpermute_b32 with five instructions of address arithmetic around it, per step.)
__device__ __forceinline__ uint32_t umin(uint32_t a, uint32_t b) { return a < b ? a : b; }
template <int CTRL, int ROW_MASK = 0xf>
__device__ __forceinline__ uint32_t dpp(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, CTRL, ROW_MASK, 0xf, false);   // lanes without a source keep their own value
}
// (a lane without a source takes the minimum's identity: written so, hipcc folds the move into the minimum -- one v_min_u32_dpp per step where
// "keeps its own value" cost a copy, the move and the minimum)
template <int CTRL, int ROW_MASK = 0xf>
__device__ __forceinline__ uint32_t dpp_or_max(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)v, CTRL, ROW_MASK, 0xf, false);
}
__device__ __forceinline__ uint32_t block_min(uint32_t key) {
    key = umin(key, dpp_or_max<0xb1>(key));         // quad_perm [1,0,3,2]
    key = umin(key, dpp_or_max<0x4e>(key));         // quad_perm [2,3,0,1]
    key = umin(key, dpp_or_max<0x141>(key));        // row_half_mirror
    key = umin(key, dpp_or_max<0x140>(key));        // row_mirror
    return umin(key, (uint32_t)__builtin_amdgcn_ds_swizzle((int)key, 0x401f));   // bit mode: and 0x1f, or 0, xor 0x10
}

// sat_i8(a >> 7) in byte 0, sat_i8(b >> 7) in byte 1 (v_ashr_pk_i8_i32; as a 16-bit value the undefined bits 31:16 stay explicit).
// Pixels travel as signed bytes p - 128 and every tap set sums to 128, so a pass computes sum((p-128) f) = sum(p f) - 128 * 128, and
//     sat_i8((sum(p f) - 16384 + 64) >> 7) = sat_u8((sum(p f) + 64) >> 7) - 128:
// the signed saturation of the biased sum IS the biased byte of the reference's clamped sample; the rounding 64 rides in the product (mfma_round).
typedef unsigned short us2 __attribute__((ext_vector_type(2)));
typedef short ss2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned short ashr7_pk_i8(int a, int b) { return __builtin_amdgcn_ashr_pk_i8_i32(a, b, 7); }
// four consecutive results of one lane (rows 4q .. 4q + 3 of its column) as four biased bytes: row 4q in byte 0 .. row 4q + 3 in byte 3.
// The second v_ashr_pk_i8_i32 writes the UPPER half of the first one's register (its destination-half select, op_sel[3]; bits 15:0 stay): no
// v_perm_b32 to join two halves.  The lower half's upper bits are left undefined to the compiler (a zero-extension would cost a v_and_b32).
// Order, for the hazards: the lower half comes from the builtin and the inline instruction is tied to its result ("+v"), so that the compiler's own
// MFMA-to-VALU wait stands in front of the builtin and the inline instruction reads its registers of the same MFMA result strictly later.  An
// MFMA result must never be read FIRST from inline assembly: the compiler's hazard pass does not look into it.
__device__ __forceinline__ uint32_t round_pack4(const v16i &acc, int q) {
    const us2 lo = __builtin_shufflevector(us2{ashr7_pk_i8(acc[4 * q], acc[4 * q + 1]), 0}, us2{0, 0}, 0, -1);
    uint32_t r = __builtin_bit_cast(uint32_t, lo);
    asm("v_ashr_pk_i8_i32 %0, %1, %2, 7 op_sel:[0,0,0,1]" : "+v"(r) : "v"(acc[4 * q + 2]), "v"(acc[4 * q + 3]));
    return r;
}
// The rounding 64 of a pass rides in the product: k = 31 of the tap operand is 64 (make_bh, make_av; no tap reaches that far) and k = 31 of
// the data operand is made 1 here -- byte 15 of the lanes of the upper k half, which otherwise meets a zero tap.  (As the C input the
// constant cost sixteen registers: hipcc does not fold a splat into the instruction's inline-constant field.)  `keep`: s2_k31_keep of the lane,
// all ones or all but the last byte; the one goes where nothing is kept (s2_k31_one).
__device__ __forceinline__ v4i one_at_k31(v4i d, uint32_t keep) {
    d.w = (int)(((uint32_t)d.w & keep) | (~keep & 0x01000000u));
    return d;
}
__device__ __forceinline__ v16i mfma_round(v4i a, v4i b) {
    const v16i c = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    return __builtin_amdgcn_mfma_i32_32x32x32_i8(a, b, c, 0, 0, 0);
}

// The cost phase's 26 x 4 (candidate, 4x4 block) tasks of a block are spread over ALL 32 lanes of its half-wave and, for what is left, over
// one wave of the workgroup.  A lane takes its own candidate's 4x4 blocks 0..2 in three rounds; the six lanes of a block's 32 that have no
// candidate take the FOURTH 4x4 block of candidates 0..17 during those rounds, and the fourth 4x4 block of candidates 18..25 of all eight
// blocks -- 64 tasks -- is one round of one wave alone: 3.25 rounds per wave on average where lane = candidate throughout would issue 4.  The
// costs meet in LDS (in the H array's dead bytes), two workgroup barriers around the one wave's extra round.
// ALLREFS: the workgroup takes its eight blocks through EVERY enabled reference of its context, one after the other (the batched forms, grid
// y = 1); what does not depend on the reference is made once, ahead of the loop: the blocks' coordinates, the current block's load, its byte
// scatter and its share of the metric (the pre table, which therefore has an array of its own: the H array's bytes are the next reference's).
// Otherwise one reference, ref_idx (the one-video form: one reference per blockIdx.y).
// Lane arithmetic: every LDS address and every small integer of a global address is a function of the thread's number alone, stated once in
// s2_lane_layout.h.  A register of it kept across the loops is one a wave of the SIMD cannot have, so only what the later stages use is kept (the H
// store, the vertical pass and the cost phase: made from threadIdx.x, the compiler holds them).  What the head of a reference uses -- the window,
// the zero-vector block, the operands' rows and the whole-pel column, 37 vector instructions to compute -- the ALLREFS form reads: the lane's row
// of K_S2_LANE, its first two dwords, which the window's load and store hang on, once per group and kept across the reference loop, the rest per
// reference in one load beside the net vector's -- a field taken out where it is used.  The one-reference form computes the fields from tn by the
// functions the table was made from: its workgroup comes here once, nothing is made twice, and the row's registers would only add to its count.
// tn: the thread's number -- in the ALLREFS form as a value the compiler cannot follow (search2_two_groups), for the once-per-group part, which is made
// again per group.
template <bool ALLREFS>
__device__ __forceinline__ void search2_body(const S2Args &a, int wg_x, int ref_idx, int tn) {
    if (ALLREFS ? a.nrefs == 0 : ref_idx >= a.nrefs) return;
    __shared__ __attribute__((aligned(16))) uint32_t s_HT[8][5 * HT_XC];
    __shared__ __attribute__((aligned(16))) uint32_t s_V[8][V_SLOT];   // vertical pass results and the zero-MV block: [4x4 block][candidate][column], biased bytes
    // (the staged window, 16 rows x 32 B, is the first 512 bytes of the block's V slot: dead once the horizontal pass has read it)
    // the current block's share of the metric, [4x4 block][the 16 quantities of weight_mfma], made once per group of blocks; 4x4 block 3 three times over
    // (ints 48.., 64.., 80..), so that an idle lane of the cost phase, which stays on block 3, steps through the table as the others do.
    // (LDS per workgroup decides how many workgroups a CU holds: 21.6 KB = seven.)
    __shared__ __attribute__((aligned(16))) uint32_t s_pre[8][PRE_SLOT];
    // (q3, [candidate]: the cost of its fourth 4x4 block, made by another lane, lives in the H array's bytes, dead once the vertical pass has read them)
    static_assert(S2_EXT == EXT, "s2_lane_layout.h restates the planes' edge width");
    static_assert(sizeof(s_HT) == S2_HT_BYTES && sizeof(s_V) == S2_V_BYTES && sizeof(s_pre) == S2_PRE_BYTES, "s2_lane_layout.h states these arrays");
    uint32_t *const HT = &s_HT[0][0], *const V = &s_V[0][0], *const PRE = &s_pre[0][0];
    const int t = (int)threadIdx.x, g = s2_slot(t), lane = s2_lane(t);
    const int b = imin(wg_x * 8 + g, a.nblk - 1);
    const bool live = wg_x * 8 + g < a.nblk;
    const int by = a.bw == 1 ? b : (int)__umulhi((uint32_t)b, a.bw_inv), bx = b - by * a.bw;   // b / bw: bw_inv = ceil(2^32 / bw), exact for b * bw < 2^32
    const int cx = bx * 8, cy = by * 8;
    // the block's cell in the nets and in the cost array as a byte offset: read and written through it.  (Through an empty asm per reference, in
    // place: seen as a loop invariant it is widened to a 64-bit pair once and every access pays a 64-bit add.)
    uint32_t boff = (uint32_t)b * 4u;
    // the lane's row of K_S2_LANE as a byte offset, a new value per reference as far as the compiler can tell (in place, too: no copy) -- its loads
    // would otherwise leave the loop and their eight registers stay
    uint32_t trow = (uint32_t)tn * (uint32_t)(S2_LANE_DWORDS * 4);
    // the first two dwords of that row, what the head of a reference needs first: read here, once per group, and kept across the reference loop
    v2i lk = {0, 0};
    if (ALLREFS) lk = *reinterpret_cast<const v2i *>(reinterpret_cast<const char *>(K_S2_LANE.w) + trow);
    {   // current block: lanes 0-15 one dword each, scattered as column bytes [row half][column] (16 dwords, in the table's last 64 bytes): the four
        // columns of 4x4 block (m*2 + n) -- the order the cost loop below walks them: row half m, column half n -- are four consecutive dwords.  Then
        // its share of the metric (vp8hip_dev.h, weight_pre_half), half a 4x4 block per lane: lane = (copy, half): the 4x4 blocks 0, 1, 2, 3 and the two
        // further copies of block 3 (copies 3, 4, 5), the quantities of row 0 + X or those of row 2 + Y.  No lane is masked: the lanes past the twelfth
        // make and store the last copy's halves again.
        if (s2_lane(tn) < 16) {
            const uint32_t coff = __umul24((uint32_t)(cy + s2_cur_row(tn)), (uint32_t)a.cur.stride) + (uint32_t)(cx + s2_cur_half_bytes(tn));
            const uint32_t v = *reinterpret_cast<const uint32_t *>(a.cur.p + coff) ^ 0x80808080u;
            uint8_t *cz = lds_at<uint8_t>(PRE, s2_cur_scatter(tn));
#pragma unroll
            for (int j = 0; j < 4; ++j) cz[j * 4] = (uint8_t)(v >> (8 * j));
        }
        lds_fence();
        const int hf = s2_pre_half(tn);
        const v4i cv = *lds_at<const v4i>(PRE, s2_pre_cols(tn));   // (every lane of the wave reads before any of them writes: LDS takes a wave's operations in order)
        const uint32_t cc[4] = {(uint32_t)cv.x, (uint32_t)cv.y, (uint32_t)cv.z, (uint32_t)cv.w};
        int smcd[4], xy[4];
        weight_pre_half(cc, hf ? K_W_R2 : K_W_R0, hf ? K_W_Y : K_W_X, smcd, xy);
        int *dst = lds_at<int>(PRE, s2_pre_store(tn));
        *reinterpret_cast<v4i *>(dst) = v4i{smcd[0], smcd[1], smcd[2], smcd[3]};
        *reinterpret_cast<v4i *>(dst + METRIC_X) = v4i{xy[0], xy[1], xy[2], xy[3]};
    }
    // ---- lane = candidate: what of it does not depend on the reference ------------------------------
    // its number in the key's low byte as (dy + 2) * 8 + (dx + 2), 40 for the zero vector: the same order as k, and the lane
    // that writes the block's result takes the winner's offsets out of it with a mask and a shift
    const int k = lane;
    const int dx = k % 5 - 2, dy = k / 5 - 2;
    // (with the candidate's vector-cost penalty, :1176-1178, above it: cost and number go into the key with one shift-and-add)
    const uint32_t kcode = k < 25 ? (uint32_t)((iabs(dx) + iabs(dy)) * 32 * 256 + (dy + 2) * 8 + dx + 2) : 40u;
    const us2 dxy = {(unsigned short)dx, (unsigned short)dy};     // its offsets as a 16-bit pair
    const v4i wa = metric_a(s2_wave_lane(t));        // the metric's column pass on the matrix cores (weight_mfma, vp8hip_dev.h): every lane of the wave is here

    // ---- everything below is per reference ------------------------------------------------------------------------------
    // From the part above it uses: live, cx, cy, boff (the block), k, dxy, kcode, wa (the lane's candidate) and the pre table.
    // Its LDS reuse rests on one rule -- LDS executes a wave's operations in program order, and every array slot is written only by the
    // wave whose lanes own it (the one wave of the fourth-block round only reads other slots, between the two barriers; s2_lane_layout_check.cpp
    // walks every address of s2_lane_layout.h for it):
    //   * the window lives in the first 512 bytes of the block's V slot; candidate 25 of 4x4 block 0 (bytes 400..415) lies inside them, so
    //     the zero-MV scatter comes after the last read of the window and before the vertical pass's stores;
    //   * q3 (the fourth-block costs) lives in words 64..95 of the block's H slot, written after the vertical pass has read the H array and
    //     read back before the next reference's horizontal pass writes it; words 29..31 of q3 take the stores nobody reads;
    //   * the pre table is only read here.
    auto one_reference = [&](int ri) {
        asm volatile("" : "+v"(trow), "+v"(boff));
        const int r = a.refmap[ri];
        // The rest of the lane's row, at the top with the net vector's load; its first two dwords were read once per group (lk, above) and are
        // kept: nothing the window's load and store hang on is waited for, and the zero-vector block's load comes behind the window's.
        v4i lb = {0, 0, 0, 0};
        if (ALLREFS) lb = *reinterpret_cast<const v4i *>(reinterpret_cast<const char *>(K_S2_LANE.w) + trow + 4 * S2_LANE_KEPT_DWORDS);
        auto fld = [&](int f) -> uint32_t {      // (f is a constant wherever this is called: a register and one v_and_b32 or v_lshrrev_b32)
            if (!ALLREFS) return s2_field(tn, f);
            const uint32_t w = (uint32_t)(f < 2 * S2_LANE_KEPT_DWORDS ? lk[(f >> 1) & 1] : lb[((f >> 1) - S2_LANE_KEPT_DWORDS) & 3]);
            return (f & 1) ? w >> 16 : w & 0xffffu;
        };
        // The three global loads of a reference -- the net vector, the window, the zero-vector block -- go by a uniform base and the lane's unsigned
        // 32-bit byte offset, as the result write does: one load each, no 64-bit address per lane.  The products are v_mad_u32_u24: a row and a stride
        // are below 2^24 (a plane is a few thousand pixels each way), and an offset below 2^32.
        const uint32_t nv = *reinterpret_cast<const uint32_t *>(reinterpret_cast<const char *>(a.net_in[r]) + boff);
        const us2 v0 = __builtin_bit_cast(us2, nv) * (unsigned short)4;      // the whole-pel vector in quarter pels, (int16)(n * 4) per half
        // (the vector the window is placed by is the one the candidates are placed by, (int16)(4 n) / 4: n itself for every vector a search hands
        // down, and for a written net whose 4 n passes int16 the place the reference's wrap lands on)
        const ss2 nw = __builtin_bit_cast(ss2, v0) >> 2;
        const int nx = nw.x, ny = nw.y;
        // window origin; a garbage vector (possible only when every candidate is out of frame) is clamped
        // so that the loads stay inside the allocated margin
        const int Lx = iclamp(cx + nx, 3 - EXT, a.w + EXT - 11), Ly = iclamp(cy + ny, 3 - EXT, a.h + EXT - 11);
        const Plane rf = a.ref[r];
        // The window from its own first byte (Lx - 3: any alignment; the part's global loads need none): lane = (row, half) takes 16
        // bytes, 16 rows of 32 bytes -- the six-tap passes need 14 x 19, the rest stays inside the planes' allocated margin (PAD) and
        // meets zero taps.  One load and one ds_write_b128 per lane, no loop.
        // The window starts up to EXT - 3 rows and columns outside the frame (Lx - 3, Ly - 3 >= -EXT): the scalar base moves back by EXT rows and
        // EXT columns, once per reference, and the lane's row and column move forward by as much (in the table's fields: s2_win_row_biased,
        // s2_win_half_biased), so that its offset is never negative.
        {
            const uint8_t *const wbase = rf.p - (ptrdiff_t)EXT * rf.stride - EXT;
            const uint32_t woff = __umul24((uint32_t)Ly + fld(S2F_WIN_ROW), (uint32_t)rf.stride) + ((uint32_t)Lx + fld(S2F_WIN_HALF));
            v4i v;
            __builtin_memcpy(&v, wbase + woff, 16);
            *lds_at<v4i>(V, fld(S2F_WIN_STORE)) = v ^ (int)0x80808080u;
        }
        // zero-MV block: one dword per lane (both halves of the block's lanes load the same eight rows: no branch), scattered below, once the
        // window -- whose bytes its place in the V array shares -- has been read
        const uint32_t zoff = __umul24((uint32_t)cy + fld(S2F_ZERO_ROW), (uint32_t)rf.stride) + ((uint32_t)cx + fld(S2F_ZERO_HALF));
        const uint32_t zv = *reinterpret_cast<const uint32_t *>(rf.p + zoff) ^ 0x80808080u;
        lds_fence();
        const uint32_t k_row = !ALLREFS ? (uint32_t)s2_k_row(tn) : (uint32_t)lb[(S2F_K_ROW >> 1) - S2_LANE_KEPT_DWORDS];                     // the lane's row of K_BH and of K_AV: S2F_K_ROW, alone in its dword
        const uint32_t k31_keep = !ALLREFS ? s2_k31_keep(tn) : (uint32_t)lk[S2F_K31_KEEP_HI >> 1] | 0xffffu;        // one_at_k31's mask, all of the operand's last dword or all but its last byte: S2F_K31_KEEP_HI above 0xffff

        // ---- horizontal pass: ONE MFMA for the wave's two blocks ------------------------------------------------------------
        // A = the windows (row m = 16 * block + window row; rows 14, 15 and bytes 20..31 of a row hold whatever the LDS held: they
        // meet zero taps or land in bytes nobody reads), B = the taps of the four fractional x cases (K_BH).  A lane comes out with
        // column n = (x case, c) and four groups of four consecutive rows: each group one dword of the TRANSPOSED H array.
        {
            const v4i aw = *lds_at<const v4i>(V, fld(S2F_AW_READ));
            const v4i bh = *reinterpret_cast<const v4i *>(reinterpret_cast<const char *>(K_BH.w) + k_row);
            const v16i acc = mfma_round(one_at_k31(aw, k31_keep), bh);
            const int ht = s2_ht_store(t);   // rows 4 * kh .. of column c; + 8 bytes: rows 8 + 4 * kh ..; next slot: the other block
#pragma unroll
            for (int q = 0; q < 4; ++q) *lds_at<uint32_t>(HT, ht + s2_ht_store_step(q)) = round_pack4(acc, q);
        }
        {   // whole-pel x case: column c of the window, rows 4*rg..4*rg+3 (rows 14, 15 -- staged like the others -- only ever meet zero taps)
            const uint8_t *wb = lds_at<const uint8_t>(V, fld(S2F_WP_READ));
            uint32_t v = 0;
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) v |= (uint32_t)wb[rr * (4 * WIN_ROW)] << (8 * rr);
            *lds_at<uint32_t>(HT, fld(S2F_WP_STORE)) = v;
        }
        {   // the zero-MV block as candidate 25 of the V array: the lane's dword = row `row`, columns 4 * half .. + 3 -> byte row & 3 of the four
            // column dwords of 4x4 block (row >> 2, half).  (Behind the window's reads: LDS takes a wave's operations in order.)
            uint8_t *z = lds_at<uint8_t>(V, fld(S2F_ZERO_SCATTER));
#pragma unroll
            for (int j = 0; j < 4; ++j) z[j * 4] = (uint8_t)(zv >> (8 * j));
        }
        lds_fence();

        // ---- vertical pass: three MFMAs for the wave's 2 x 5 x 8 columns ------------------------------------------------------
        // A = the taps of the four fractional y cases (K_AV: row m = (y case, output row)), B = 32 columns of the H arrays, 16 bytes
        // each (the lanes of the upper k half read the same column: their A entries are zero).  A lane comes out with its column and, per
        // y case, the four rows 4 * kh .. 4 * kh + 3: one dword of the prediction, column c & 3 of 4x4 block (kh, c >> 2).  The whole-pel y case is a copy.
        {
            const v4i av = *reinterpret_cast<const v4i *>(reinterpret_cast<const char *>(K_AV.w) + k_row);
            const int kh = s2_k_half(t);
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const v4i hv = *lds_at<const v4i>(HT, s2_hv_read(t, i));
                const v16i acc = mfma_round(av, one_at_k31(hv, k31_keep));
                if (s2_v_on(t, i)) {
                    const int sv = s2_sv_store(t, i);
#pragma unroll
                    for (int f = 0; f < 4; ++f) *lds_at<uint32_t>(V, sv + s2_sv_store_step(f + (f >> 1))) = round_pack4(acc, f);
                    // whole-pel dy: rows 3..10 of the column, the lower lane half rows 3..6, the upper 7..10
                    *lds_at<uint32_t>(V, sv + s2_sv_store_step(2)) = kh ? __builtin_amdgcn_alignbyte((uint32_t)hv[2], (uint32_t)hv[1], 3)
                                                                        : __builtin_amdgcn_alignbyte((uint32_t)hv[1], (uint32_t)hv[0], 3);
                }
            }
        }
        lds_fence();

        // ---- cost: lane = candidate --------------------------------------------------------------------
        // The candidate's vector as a 16-bit pair, (int16)(v0x + dx) per half ((0, 0) for the zero candidate), and its position, the block's own
        // added to it.  (int16)(4 cx + v0x + dx), as :1143 has it, differs from this sum only where it passes 32767: negative there, past the
        // frame's last position here -- out of the frame either way (a frame is narrower than 8192 pixels: 4 w - 32 fits an int16).
        const uint32_t vq = k == 25 ? 0u : __builtin_bit_cast(uint32_t, (us2)(v0 + dxy));
        const int qx = cx * 4 + (int16_t)(vq & 0xffffu), qy = cy * 4 + ((int)vq >> 16);
        const bool valid = live && k < 26 && qx >= 0 && qx <= a.w * 4 - 32 && qy >= 0 && qy <= a.h * 4 - 32;
        int diff = 0;
        // a task = 16 bytes of the V array (the B operand: one ds_read_b128) and 16 ints of the pre table (the C input)
        auto metric = [&](int src, int pre16) { return weight_mfma(wa, load_pre16(lds_at<const int>(PRE, pre16)), *lds_at<const v4i>(V, src)); };
        // (branch-free: a lane's own candidate, 4x4 block j in round j, or, for the idle lanes, 4x4 block 3 of candidate 3 (lane - 26) + j: one
        // base address and one stride per lane, the table's copies of block 3 one block apart like the others; the idle lanes' costs go to q3,
        // everybody else's to the table's unused words 29..31, and an idle lane's own sum is never looked at: `valid` is false there)
        const int src = s2_cost_src(t), step = s2_cost_step(t), pre = s2_cost_pre(t);
        int *dst = lds_at<int>(HT, s2_cost_dst(t));
#pragma unroll
        for (int j = 0; j < 3; ++j) {       // rounds 0..2: a candidate's own lane its 4x4 blocks 0..2, the idle lanes block 3 of candidates 0..17
            const int c = metric(src + j * step, pre + 64 * j);
            dst[j] = c;
            diff += c;
        }
        __syncthreads();                    // every wave's V and pre arrays (and the idle lanes' costs) are in LDS
        if (s2_wave(t) == (wg_x & 3)) {      // ONE wave (taking turns from workgroup to workgroup: the waves of a workgroup sit on different SIMDs): block 3 of candidates 18..25 of all eight block slots
            *lds_at<int>(HT, s2_extra_dst(t)) = metric(s2_extra_src(t), s2_extra_pre(t));
        }
        __syncthreads();
        diff += *lds_at<const int>(HT, s2_cost_q3_read(t));
        uint32_t key = ((uint32_t)diff << 8) + kcode;     // (diff + penalty) << 8 | number
        const bool ok = valid && key < (0x7fffu << 8);
        key = ok ? key : 0xffffffffu;
        const uint32_t kmin = block_min(key);
        // (results by base + 32-bit byte offset: a uniform base and a lane's unsigned offset are one store each, no 64-bit address per lane.  The
        // offset is the one the net vector was read by: one register across the loop, where the block's number as a 64-bit index took two.  Through
        // the empty asm again, in place: the stores sit in a block of their own, where the compiler otherwise meets the offset already widened)
        auto result_write = [&](uint32_t v, int md) {
            asm volatile("" : "+v"(boff));
            *reinterpret_cast<uint32_t *>(reinterpret_cast<char *>(a.net_out[r]) + boff) = v;
            *reinterpret_cast<int *>(reinterpret_cast<char *>(a.bdiff[r]) + boff) = md;
        };
        // The winning lane writes: keys are unique in a block (the candidate's number is the low byte), so exactly one lane holds the minimum, and
        // it holds all the result is made of.  A candidate in the frame has not wrapped: its vector is (v0x + dx, v0y + dy) as 16-bit sums -- one
        // packed add -- or (0, 0) for the zero candidate; its penalty, (|dx| + |dy|) * 32, sits in the key and not in `diff`, and :1195-1197 take it
        // back unless the vector is (0, 0): diff for a vector that is not, key >> 8 -- what the reference keeps -- for one that is (the zero candidate,
        // or the zero offset on a zero vector: v0 is a multiple of 4, so no other offset leads there, and both carry a penalty of 0).
        if (ok && key == kmin) {
            result_write(vq, vq != 0 ? diff : (int)(key >> 8));
        }
        // :1136-1137: with no candidate accepted the result is the frame's last position, as a vector: (int16)((int16)(4 w - 32) - 4 cx), cost 0x7fff
        // less the penalty of THAT vector.  Kept as the reference has it, behind a branch that waves skip: the zero candidate is in the frame for every
        // block and costs less than 0x7fff whatever the pixels (tests/test_gpu_search2_pack_tail.py, test_no_block_can_cost_0x7fff), so nothing gets here.
        if (kmin == 0xffffffffu && lane == 16 && live) {
            const int vx = (int16_t)((int16_t)(a.w * 4 - 32) - cx * 4), vy = (int16_t)((int16_t)(a.h * 4 - 32) - cy * 4);
            const int v0x = (int16_t)v0.x, v0y = (int16_t)v0.y;
            int md = 0x7fff;
            if ((vx != 0) | (vy != 0)) md -= (iabs(vx - v0x) + iabs(vy - v0y)) * 32;  // :1195-1197
            result_write((uint32_t)(uint16_t)vx | ((uint32_t)(uint16_t)vy << 16), md);
        }
    };
    if (ALLREFS) {
#pragma unroll 1
        for (int ri = 0; ri < a.nrefs; ++ri) one_reference(ri);
    } else {
        one_reference(ref_idx);
    }
}

// The batched forms: a workgroup takes two consecutive groups of eight blocks, one after the other, each through every enabled reference -- up to
// six passes of the body per workgroup (four groups took the registers past seven waves per SIMD, and a workgroup of twelve passes makes the
// launch's end ragged).  A third of what a wave issues for a group does not depend on the group -- the lane's place in the operand tables of
// the two passes and the tables themselves, its LDS addresses in every stage, its candidate's offset and penalty -- and the compiler keeps in
// registers across the loop what search2_body makes from threadIdx.x (the price: registers, i.e. waves per SIMD).  What it makes from tn --
// the once-per-group part's addresses, and the byte offset of the lane's row of K_S2_LANE -- starts anew with every group: the empty asm below
// is the one place the thread's number is hidden at; per reference the body hides the row's offset again, in place.
__device__ __forceinline__ void search2_two_groups(const S2Args &a, int grp) {
#pragma unroll 1
    for (int it = 0; it < 2; ++it) {
        int tn = (int)threadIdx.x;
        asm volatile("" : "+v"(tn));     // (the same number, as far as the compiler can tell a new one per group)
        search2_body<true>(a, grp * 2 + it, 0, tn);
    }
}
// One video: grid (groups, references), one group and one reference per workgroup -- its launch is a few rounds of workgroups long, and
// longer workgroups make its end ragged (53.0 against 54.3 us with two groups each).
// (waves_per_eu, here as on the batched forms: left to __launch_bounds__(256, 4) the register allocator takes 74 registers for the two-group
// form -- six waves per SIMD -- where it fits the same code into 72 when told to; this form has 57 either way.  The MFMAs' results still
// land in VGPRs, no v_accvgpr_read per result: tests/test_kernel_resources.py pins zero AGPRs.)
__global__ __attribute__((amdgpu_waves_per_eu(7, 8))) __launch_bounds__(256) void k_search2(S2Args a) {
    const unsigned long long first = launch_clock_first_thread();
    launch_clock_begin(a.clk);
    search2_body<false>(a, xcd_band(blockIdx.x, gridDim.x), blockIdx.y, (int)threadIdx.x);
    launch_clock_end(a.clk, first);
}
static_assert(sizeof(BatchOf<S2Args>) <= 4096, "a batch's argument blocks travel in the 4 KiB kernel-argument segment");
// The batched forms: grid (pairs of groups, 1, contexts), every enabled reference of the context inside the workgroup
__global__ __attribute__((amdgpu_waves_per_eu(7, 8))) __launch_bounds__(256) void k_search2_b(BatchOf<S2Args> b) {
    const unsigned long long first = launch_clock_first_thread();
    launch_clock_begin(b.item[0].clk);
    search2_two_groups(b.item[blockIdx.z], xcd_band(blockIdx.x, gridDim.x));
    launch_clock_end(b.item[0].clk, first);
}
// The same launch carrying the loop-filter strength scans of its members' NEW frames (kernels_rc_dev.h): the workgroups behind the
// nbx searching workgroups.  With the part full a launch of the scan's own holds the batch's stream for 0.4-0.7 ms where its
// work is 15 us (every workgroup waits for a place) -- the headline without that launch: +4 %, scripts/ab_flags_experiments.sh -- and
// the shorter launches of the chain cannot absorb it either (in the pyramid's launch it made THAT link the long one: -2 %).  This is
// the frame's longest launch, the scan's result is wanted by k_mb, which comes next, and the scan's 136 workgroups per frame ride
// behind the launch's search workgroups.
struct S2Scans { rc::ScanCore item[MAX_BATCH]; uint32_t mask; int nbx, wgs; };
static_assert(sizeof(BatchOf<S2Args>) + sizeof(S2Scans) <= 4096, "the kernel-argument segment");
// (waves_per_eu: with the scans' body in the same function the register allocator otherwise settles at 76 -- six waves per SIMD; told to, it fits the same code into 70)
__global__ __attribute__((amdgpu_waves_per_eu(7, 8))) __launch_bounds__(256) void k_search2_bs(BatchOf<S2Args> b, S2Scans sc) {
    if ((int)blockIdx.x >= sc.nbx) {
        const int wg = (int)blockIdx.x - sc.nbx;
        if (((sc.mask >> blockIdx.z) & 1) && wg < sc.wgs) rc::strength_segments_body(b.item[blockIdx.z].cur, sc.item[blockIdx.z], wg, sc.wgs);
        return;
    }
    const unsigned long long first = launch_clock_first_thread();
    launch_clock_begin(b.item[0].clk);
    search2_two_groups(b.item[blockIdx.z], xcd_band(blockIdx.x, sc.nbx));
    launch_clock_end(b.item[0].clk, first);
}

// test tap: round_pack4 over caller-supplied values, a lane four quadruples (its "sixteen results" of an MFMA: q = 0..3 as the passes call it)
__global__ __launch_bounds__(256) void k_round_pack4_tap(const int32_t *v, int n, uint32_t *out) {
    const int t = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    v16i acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 16; ++j)
        if (4 * t + (j >> 2) < n) acc[j] = v[16 * t + j];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint32_t r = round_pack4(acc, q);
        if (4 * t + q < n) out[4 * t + q] = r;
    }
}

}  // namespace

void launch_round_pack4_tap(hipStream_t s, const int32_t *v, int n, uint32_t *out) {
    VP8_LAUNCH(k_round_pack4_tap, dim3((n + 1023) / 1024), dim3(256), 0, s, v, n, out);
}

static S2Args search2_args(const CodingItem &it, unsigned long long *clk) {
    const Frame &cur = *it.cur;
    const RefSet &refs = it.refs;
    const NetSet &nets = *it.nets;
    S2Args a;
    a.clk = clk;
    a.cur = cur.Y[0];
    int n = 0;
    for (int r = 0; r < 3; ++r) {
        a.ref[r] = refs.ref[r].Y[0];
        a.net_in[r] = nets.net[r][1];   // vnet2 holds the 1x result, init.h:832-854
        a.net_out[r] = nets.net[r][0];
        a.bdiff[r] = nets.bdiff[r];
        if (refs.use[r]) a.refmap[n++] = r;
    }
    a.nrefs = n;
    for (int i = n; i < 3; ++i) a.refmap[i] = 0;
    a.w = a.cur.w;
    a.h = a.cur.h;
    a.bw = a.w / 8;
    a.bw_inv = (uint32_t)(((1ull << 32) + a.bw - 1) / a.bw);
    a.nblk = a.w * a.h / 64;
    return a;
}
static bool search2_skip() {
    static const bool skip = experiment_skip("s2");
    return skip;   // timing experiment only
}

void launch_search2(hipStream_t s, const CodingItem &it, unsigned long long *clk) {
    const S2Args a = search2_args(it, clk);
    if (a.nrefs == 0 || search2_skip()) return;
    VP8_LAUNCH(k_search2, dim3((a.nblk + 7) / 8, a.nrefs), dim3(256), 0, s, a);
}

bool launch_search2_batch(hipStream_t s, const CodingItem *items, int n, unsigned long long *clk) {
    BatchOf<S2Args> b;
    b.n = n;
    int maxrefs = 0;
    for (int i = 0; i < n; ++i) {
        b.item[i] = search2_args(items[i], clk);
        maxrefs = b.item[i].nrefs > maxrefs ? b.item[i].nrefs : maxrefs;
    }
    if (maxrefs == 0 || search2_skip()) return false;
    S2Scans sc;
    sc.mask = 0;
    for (int i = 0; i < n; ++i) {      // (a request's plane is the member's current luma: what the kernel reads as b.item[i].cur)
        if (!items[i].scan) continue;
        sc.mask |= 1u << i;
        sc.item[i] = rc::scan_core(*items[i].scan);
    }
    const int ngrp = ((b.item[0].nblk + 7) / 8 + 1) / 2;     // workgroups that search: each takes two groups of eight blocks
    if (!sc.mask) {
        VP8_LAUNCH(k_search2_b, dim3(ngrp, 1, n), dim3(256), 0, s, b);
        return false;
    }
    sc.nbx = ngrp;
    sc.wgs = (b.item[0].h + rc::ROWS_PER_BLOCK - 1) / rc::ROWS_PER_BLOCK;
    VP8_LAUNCH(k_search2_bs, dim3(ngrp + sc.wgs, 1, n), dim3(256), 0, s, b, sc);
    return true;
}

}  // namespace vp8
