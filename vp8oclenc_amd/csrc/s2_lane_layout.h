// Where a lane of the quarter-pel search (kernels_s2.hip: search2_body, every k_search2* form) reads and writes in the kernel's three LDS arrays, and
// the small integers its global addresses are made of.  All of it is a function of the thread's number t (0..255) and of the layout constants below,
// nothing else: 32 lanes per 8x8 block, block slot g = t >> 5, two slots to a wave.  Every quantity is stated ONCE, here, as a constexpr function of
// t; search2_body indexes by these functions and by nothing else (scripts/native/s2_lane_layout_check.cpp walks every one of them).  What a wave would otherwise compute again for every reference (because holding
// it across the metric costs registers, i.e. waves per SIMD) it reads instead: K_S2_LANE[t] (kernels_s2.hip) is make_s2_lane() below, the fields
// 16 bits each, two to a dword, and a field comes out of its dword with one v_and_b32 or one v_lshrrev_b32 where it is used.
// All offsets are BYTES from the first byte of their array (s_HT, s_V -- whose first 512 bytes per slot are also the staged window -- and s_pre):
// the arrays' own addresses are link-time constants and ride in the offset field of the ds_* instruction.
// In a header of its own so that the kernel, the compile-time checks below and the host program of tests/test_s2_lane_layout.py (scripts/native/
// s2_lane_layout_check.cpp) share one statement of every address.
#pragma once
#include <stdint.h>

#if defined(__HIP__) || defined(__HIPCC__) || defined(__CUDACC__)
#define S2_LANE_HD __host__ __device__
#else
#define S2_LANE_HD
#endif

constexpr int HT_XC = 36;            // dwords per x case in the transposed H array: 8 columns x 16 B + 16 B bank skew
// The V array (vertical pass results = the predictions of the 25 candidates, + the zero-vector block as candidate 25) is ordered
// [4x4 block][candidate][column]: a (candidate, 4x4 block) task of the cost phase is 16 contiguous bytes, one ds_read_b128, and the
// 16 lanes such a read serves at a time take 16 consecutive candidates = 256 consecutive bytes = every bank once, with no skew.
constexpr int V_CAND = 4;              // dwords per task: the four columns of a 4x4 block, four rows each
constexpr int V_ROW = 26 * V_CAND;     // dwords per 4x4 block: 25 candidates (y case * 5 + x case) + the zero-vector block
constexpr int V_SLOT = 4 * V_ROW;      // dwords per 8x8 block: 4x4 block b = 2 * (row half) + (column half)
constexpr int V_ZERO = 25;
constexpr int PRE_SLOT = 96;           // ints per 8x8 block in the pre table: 4x4 blocks 0, 1, 2, 3, 3, 3 x 16 (see search2_body)
constexpr int WIN_ROW = 8;             // dwords per row of the staged window: 20 bytes loaded, 32 so that a row half is one aligned ds_read_b128

constexpr int S2_THREADS = 256, S2_SLOTS = 8;
constexpr int S2_HT_SLOT_BYTES = 5 * HT_XC * 4, S2_V_SLOT_BYTES = V_SLOT * 4, S2_PRE_SLOT_BYTES = PRE_SLOT * 4;
constexpr int S2_HT_BYTES = S2_SLOTS * S2_HT_SLOT_BYTES, S2_V_BYTES = S2_SLOTS * S2_V_SLOT_BYTES, S2_PRE_BYTES = S2_SLOTS * S2_PRE_SLOT_BYTES;
constexpr int S2_WIN_BYTES = 16 * WIN_ROW * 4;      // the staged window of a slot: 16 rows x 32 B, the first bytes of its V slot
constexpr int S2_Q3_WORD = 64;                      // q3 (the fourth-block costs of a slot): words 64..95 of its H slot

// ---- the lane's places ---------------------------------------------------------------------------------------------------------------------
S2_LANE_HD constexpr int s2_slot(int t) { return t >> 5; }                 // g: the lane's block slot
S2_LANE_HD constexpr int s2_lane(int t) { return t & 31; }                 // its number in the block = its candidate k
S2_LANE_HD constexpr int s2_wave_lane(int t) { return t & 63; }            // wl
S2_LANE_HD constexpr int s2_k_half(int t) { return (t & 63) >> 5; }        // kh: its k half in an MFMA operand
S2_LANE_HD constexpr int s2_wave_slot(int t) { return (t >> 5) & ~1; }     // gp: the first slot of its wave
S2_LANE_HD constexpr int s2_wave(int t) { return t >> 6; }

// ---- the window: one 16-byte global load and one ds_write_b128 per lane, lane = (row, half) ------------------------------------------------------
S2_LANE_HD constexpr int s2_win_row(int t) { return s2_lane(t) >> 1; }                 // window row 0..15
S2_LANE_HD constexpr int s2_win_half_bytes(int t) { return 16 * (s2_lane(t) & 1); }    // byte column of the lane's half: 0 or 16
// The window starts up to S2_EXT - 3 rows and columns outside the plane, and the kernel moves the plane's base back by S2_EXT rows and columns so that
// a lane's offset from it is never negative: the row and the column the lane adds to the window's origin (Ly, Lx: its sample (3, 3)) carry the rest
constexpr int S2_EXT = 8;      // = EXT (vp8hip_dev.h): the replicated-edge width of a plane
S2_LANE_HD constexpr int s2_win_row_biased(int t) { return s2_win_row(t) + S2_EXT - 3; }
S2_LANE_HD constexpr int s2_win_half_biased(int t) { return s2_win_half_bytes(t) + S2_EXT - 3; }
S2_LANE_HD constexpr int s2_win_store(int t) {                                         // s_V (the window's bytes)
    return s2_slot(t) * S2_V_SLOT_BYTES + (s2_win_row(t) * WIN_ROW) * 4 + s2_win_half_bytes(t);
}
// ---- the zero-vector block: one dword per lane, both halves of a block's lanes the same eight rows ---------------------------------------------
S2_LANE_HD constexpr int s2_zero_row(int t) { return (s2_lane(t) >> 1) & 7; }
S2_LANE_HD constexpr int s2_zero_half_bytes(int t) { return 4 * (s2_lane(t) & 1); }
// its scatter as candidate 25 of the V array: byte row & 3 of the four column dwords (+ 4 j) of 4x4 block (row >> 2, half)
S2_LANE_HD constexpr int s2_zero_scatter(int t) {
    return s2_slot(t) * S2_V_SLOT_BYTES + ((((s2_zero_row(t) >> 2) * 2 + (s2_lane(t) & 1)) * V_ROW + V_ZERO * V_CAND) * 4) + (s2_zero_row(t) & 3);
}
// ---- horizontal pass: A row m = 16 * block + window row -------------------------------------------------------------------------------------
S2_LANE_HD constexpr int s2_aw_read(int t) {                                           // s_V (the window): s_win[gp + (m >> 4)][(m & 15) * WIN_ROW + 4 * kh]
    return (s2_wave_slot(t) + ((t & 31) >> 4)) * S2_V_SLOT_BYTES + (((t & 15) * WIN_ROW) + 4 * s2_k_half(t)) * 4;
}
// the lane's column n = (x case, c): rows 4 * kh .. of column c; + 8 bytes: rows 8 + 4 * kh ..; + a slot: the other block
S2_LANE_HD constexpr int s2_ht_store(int t) {                                          // s_HT
    const int m = t & 31, xi = m >> 3, c = m & 7, xc = xi + (xi >> 1);
    return s2_wave_slot(t) * S2_HT_SLOT_BYTES + (xc * HT_XC + c * 4 + s2_k_half(t)) * 4;
}
S2_LANE_HD constexpr int s2_ht_store_step(int q) { return ((q >> 1) * (5 * HT_XC) + 2 * (q & 1)) * 4; }     // result group q = 0..3 of the lane
// whole-pel x case: column c of the window, rows 4 * rg .. 4 * rg + 3, a byte each (+ 32 rr)
S2_LANE_HD constexpr int s2_wp_read(int t) {                                           // s_V (the window)
    return s2_slot(t) * S2_V_SLOT_BYTES + 3 + (s2_lane(t) & 7) + (s2_lane(t) >> 3) * (16 * WIN_ROW);
}
S2_LANE_HD constexpr int s2_wp_store(int t) {                                          // s_HT
    return s2_slot(t) * S2_HT_SLOT_BYTES + (2 * HT_XC + (s2_lane(t) & 7) * 4 + (s2_lane(t) >> 3)) * 4;
}
// ---- vertical pass: three MFMAs (i = 0..2) over the wave's 2 x 5 x 8 columns ---------------------------------------------------------------------
S2_LANE_HD constexpr int s2_v_col(int t, int i) { return 32 * i + (t & 31); }          // column number 0..79 (+ 16 idle in the third)
S2_LANE_HD constexpr bool s2_v_on(int t, int i) { return i < 2 || (t & 31) < 16; }
S2_LANE_HD constexpr int s2_hv_read(int t, int i) {                                    // s_HT: 16 bytes, the 16 rows of column c of x case xc
    const int ng = s2_v_col(t, i), blk = ng >= 40 ? 1 : 0, rem = s2_v_on(t, i) ? ng - 40 * blk : 0, xc = rem >> 3, c = rem & 7;
    return (s2_wave_slot(t) + blk) * S2_HT_SLOT_BYTES + (xc * HT_XC + c * 4) * 4;
}
// column c & 3 of 4x4 block (kh, c >> 2), x case xc; y case yc at + s2_sv_store_step(yc)
S2_LANE_HD constexpr int s2_sv_store(int t, int i) {                                   // s_V
    const int ng = s2_v_col(t, i), blk = ng >= 40 ? 1 : 0, rem = s2_v_on(t, i) ? ng - 40 * blk : 0, xc = rem >> 3, c = rem & 7;
    return (s2_wave_slot(t) + blk) * S2_V_SLOT_BYTES + ((s2_k_half(t) * 2 + (c >> 2)) * V_ROW + xc * V_CAND + (c & 3)) * 4;
}
S2_LANE_HD constexpr int s2_sv_store_step(int yc) { return yc * 5 * V_CAND * 4; }
// ---- cost phase: lane = candidate; the idle lanes (26..31) take 4x4 block 3 of candidates 3 (lane - 26) + j ------------------------------------------
S2_LANE_HD constexpr bool s2_cost_helper(int t) { return s2_lane(t) >= 26; }
S2_LANE_HD constexpr int s2_cost_src(int t) {                                          // s_V: round j at + j * s2_cost_step
    return s2_slot(t) * S2_V_SLOT_BYTES + (s2_cost_helper(t) ? 3 * V_ROW + (s2_lane(t) - 26) * 3 * V_CAND : s2_lane(t) * V_CAND) * 4;
}
S2_LANE_HD constexpr int s2_cost_step(int t) { return (s2_cost_helper(t) ? V_CAND : V_ROW) * 4; }
S2_LANE_HD constexpr int s2_cost_pre(int t) { return s2_slot(t) * S2_PRE_SLOT_BYTES + (s2_cost_helper(t) ? 48 : 0) * 4; }     // s_pre: round j at + 64 j
S2_LANE_HD constexpr int s2_cost_dst(int t) {                                          // s_HT (q3): round j at + 4 j; words 29..31 take the stores nobody reads
    return s2_slot(t) * S2_HT_SLOT_BYTES + (S2_Q3_WORD + (s2_cost_helper(t) ? (s2_lane(t) - 26) * 3 : 29)) * 4;
}
S2_LANE_HD constexpr int s2_cost_q3_read(int t) {                                      // s_HT (q3): the candidate's fourth-block cost
    return s2_slot(t) * S2_HT_SLOT_BYTES + (S2_Q3_WORD + (s2_lane(t) < 26 ? s2_lane(t) : 31)) * 4;
}
// the one wave of the fourth-block round: 4x4 block 3 of candidates 18..25 of all eight slots, lane = (slot, candidate)
S2_LANE_HD constexpr int s2_extra_slot(int t) { return s2_wave_lane(t) >> 3; }
S2_LANE_HD constexpr int s2_extra_cand(int t) { return 18 + (t & 7); }
S2_LANE_HD constexpr int s2_extra_src(int t) { return s2_extra_slot(t) * S2_V_SLOT_BYTES + (3 * V_ROW + s2_extra_cand(t) * V_CAND) * 4; }   // s_V
S2_LANE_HD constexpr int s2_extra_pre(int t) { return s2_extra_slot(t) * S2_PRE_SLOT_BYTES + 48 * 4; }                                    // s_pre
S2_LANE_HD constexpr int s2_extra_dst(int t) { return s2_extra_slot(t) * S2_HT_SLOT_BYTES + (S2_Q3_WORD + s2_extra_cand(t)) * 4; }        // s_HT (q3)
// ---- the current block, once per group: lanes 0..15 a dword each, scattered as column bytes into the pre table's last 64 bytes, then read back ------
S2_LANE_HD constexpr int s2_cur_row(int t) { return s2_lane(t) >> 1; }                 // (lanes 0..15: rows 0..7)
S2_LANE_HD constexpr int s2_cur_half_bytes(int t) { return 4 * (s2_lane(t) & 1); }
S2_LANE_HD constexpr int s2_cur_tmp(int t) { return s2_slot(t) * S2_PRE_SLOT_BYTES + 80 * 4; }      // s_pre: the 16 dwords of the scattered block
S2_LANE_HD constexpr int s2_cur_scatter(int t) {                                       // s_pre: byte (+ 4 j) of lane < 16
    return s2_cur_tmp(t) + (s2_cur_row(t) >> 2) * 32 + (s2_lane(t) & 1) * 16 + (s2_cur_row(t) & 3);
}
S2_LANE_HD constexpr int s2_pre_half(int t) { return s2_lane(t) & 1; }                 // hf: the quantities of row 0 + X, or those of row 2 + Y
S2_LANE_HD constexpr int s2_pre_copy(int t) { return (s2_lane(t) >> 1) < 5 ? (s2_lane(t) >> 1) : 5; }     // 4x4 blocks 0, 1, 2, 3 and block 3 twice more
S2_LANE_HD constexpr int s2_pre_cols(int t) { return s2_cur_tmp(t) + 16 * (s2_pre_copy(t) < 3 ? s2_pre_copy(t) : 3); }     // s_pre: the four columns of its 4x4 block
S2_LANE_HD constexpr int s2_pre_store(int t) { return s2_slot(t) * S2_PRE_SLOT_BYTES + (16 * s2_pre_copy(t) + 4 * s2_pre_half(t)) * 4; }   // s_pre; X / Y at + 32 bytes
// ---- the operand tables and the rounding one ------------------------------------------------------------------------------------------------
S2_LANE_HD constexpr int s2_k_row(int t) { return s2_wave_lane(t) * 16; }              // byte offset of the lane's row of K_BH / K_AV
// one_at_k31: byte 15 of a data operand becomes 1 in the lanes of the upper k half -- (d.w & keep) | one
S2_LANE_HD constexpr uint32_t s2_k31_keep(int t) { return s2_k_half(t) ? 0x00ffffffu : 0xffffffffu; }
S2_LANE_HD constexpr uint32_t s2_k31_one(int t) { return s2_k_half(t) ? 0x01000000u : 0u; }

// ---- the table ---------------------------------------------------------------------------------------------------------------------------------
// What the loops read instead of computing: field f of lane t is bits 16 (f & 1) .. + 15 of dword f >> 1 of its row.  The row has two halves.
// Dwords 0..1 are what the head of a reference needs FIRST (the window's load and its store hang on them): read once per group of blocks and
// kept across the reference loop, two registers (all four of the first half kept took the two-group forms to 72 registers and 12 bytes of scratch).
// Dwords 2..5 are read per reference, at the top: the zero-vector block's load comes behind the window's, the rest once the window stands in LDS.
// Two fields come out without a shift or a mask of their own: S2F_K31_KEEP_HI, the upper half of one_at_k31's mask (whose lower half is 0xffff),
// is the UPPER field of its dword, so the whole mask is one v_or_b32 with 0xffff away; and S2F_K_ROW is alone in its dword (S2F_NONE beside it
// is always 0), which is the offset as it stands.
enum S2Field {
    S2F_WIN_STORE, S2F_K31_KEEP_HI, S2F_WIN_HALF, S2F_WIN_ROW, S2F_ZERO_HALF, S2F_ZERO_ROW, S2F_K_ROW, S2F_NONE,     // dwords 0..1: kept across the reference loop; 2..: read per reference
    S2F_AW_READ, S2F_WP_READ, S2F_WP_STORE, S2F_ZERO_SCATTER,
    S2F_COUNT
};
constexpr int S2_LANE_KEPT_DWORDS = 2;
static_assert((S2F_K31_KEEP_HI & 1) == 1 && (S2F_K_ROW & 1) == 0 && S2F_NONE == S2F_K_ROW + 1, "the two fields that are used as whole dwords");
static_assert(S2F_WIN_ROW == 2 * S2_LANE_KEPT_DWORDS - 1 && S2F_COUNT == 2 * (S2_LANE_KEPT_DWORDS + 4), "the row's two parts: two dwords and four");
constexpr int S2_LANE_DWORDS = 8;      // a row is 32 bytes: the address of lane t's is t << 5
static_assert(S2F_COUNT <= 2 * S2_LANE_DWORDS, "the fields fit the row");
S2_LANE_HD constexpr uint32_t s2_field(int t, int f) {
    switch (f) {
    case S2F_WIN_STORE: return (uint32_t)s2_win_store(t);
    case S2F_K_ROW: return (uint32_t)s2_k_row(t);
    case S2F_WIN_HALF: return (uint32_t)s2_win_half_biased(t);
    case S2F_WIN_ROW: return (uint32_t)s2_win_row_biased(t);
    case S2F_ZERO_HALF: return (uint32_t)s2_zero_half_bytes(t);
    case S2F_ZERO_ROW: return (uint32_t)s2_zero_row(t);
    case S2F_AW_READ: return (uint32_t)s2_aw_read(t);
    case S2F_WP_READ: return (uint32_t)s2_wp_read(t);
    case S2F_WP_STORE: return (uint32_t)s2_wp_store(t);
    case S2F_ZERO_SCATTER: return (uint32_t)s2_zero_scatter(t);
    case S2F_K31_KEEP_HI: return s2_k31_keep(t) >> 16;
    default: return 0;
    }
}
struct S2LaneTable { uint32_t w[S2_THREADS][S2_LANE_DWORDS]; };
constexpr S2LaneTable make_s2_lane() {
    S2LaneTable tab{};
    for (int t = 0; t < S2_THREADS; ++t)
        for (int f = 0; f < S2F_COUNT; ++f) tab.w[t][f >> 1] |= (s2_field(t, f) & 0xffffu) << (16 * (f & 1));
    return tab;
}
S2_LANE_HD constexpr uint32_t s2_unpack(const uint32_t *row, int f) { return (f & 1) ? row[f >> 1] >> 16 : row[f >> 1] & 0xffffu; }

// ---- what can be said at compile time ---------------------------------------------------------------------------------------------------------
constexpr bool s2_fields_fit() {
    for (int t = 0; t < S2_THREADS; ++t)
        for (int f = 0; f < S2F_COUNT; ++f)
            if (s2_field(t, f) > 0xffffu) return false;
    return true;
}
constexpr bool s2_table_unpacks() {
    const S2LaneTable tab = make_s2_lane();
    for (int t = 0; t < S2_THREADS; ++t)
        for (int f = 0; f < S2F_COUNT; ++f)
            if (s2_unpack(tab.w[t], f) != s2_field(t, f)) return false;
    return true;
}
constexpr bool s2_aligned16() {      // the 16-byte reads and stores
    for (int t = 0; t < S2_THREADS; ++t) {
        if ((s2_win_store(t) | s2_aw_read(t) | s2_cost_src(t) | s2_cost_step(t) | s2_cost_pre(t) | s2_extra_src(t) | s2_extra_pre(t) |
             s2_pre_cols(t) | s2_pre_store(t) | s2_k_row(t)) & 15) return false;
        for (int i = 0; i < 3; ++i)
            if (s2_hv_read(t, i) & 15) return false;
    }
    return true;
}
static_assert(s2_fields_fit(), "a field of the lane table passes 16 bits");
static_assert(s2_table_unpacks(), "the lane table does not unpack to the named functions");
static_assert(s2_aligned16(), "a 16-byte LDS access of the quarter-pel search is not 16-byte aligned");
static_assert(S2_WIN_BYTES == 512 && V_ZERO * V_CAND * 4 == 400 && V_ZERO * V_CAND * 4 + 16 <= S2_WIN_BYTES,
              "candidate 25 of 4x4 block 0 (bytes 400..415 of the V slot) lies inside the window's 512 bytes");
static_assert((S2_Q3_WORD + 32) * 4 <= S2_HT_SLOT_BYTES, "q3 is words 64..95 of the H slot");
static_assert(s2_k31_one(32) == (~s2_k31_keep(32) & 0x01000000u) && s2_k31_one(0) == (~s2_k31_keep(0) & 0x01000000u), "one_at_k31: the one sits where nothing is kept");
