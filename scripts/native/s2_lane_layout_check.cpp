// The lane map of the quarter-pel search (csrc/s2_lane_layout.h: what search2_body indexes its three LDS arrays by, and the table K_S2_LANE its
// reference loop reads) walked on the host for all 256 threads, under the address and undefined-behaviour sanitizers; no GPU:
//     g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -I vp8oclenc_amd/csrc scripts/native/s2_lane_layout_check.cpp -o t && ./t
// The three arrays are real arrays here, read and written through the header's addresses: an access out of range is the sanitizer's.
// One `name value` pair per line (tests/test_s2_lane_layout.py reads them); every *_bad is a count of violations:
//   fields_bad       table fields that do not unpack to their named function's value, or whose value passes 16 bits
//   range_bad        accesses that leave their array, or the slot / the part of the slot (window, q3) the kernel's comment gives them
//   align_bad        16-byte accesses that are not 16-byte aligned
//   owner_bad        bytes of s_V, s_HT, s_pre written by a lane of another wave than the slot's (the fourth-block round apart, which is checked to
//                    write only the words 18..25 of q3, which nobody else writes)
//   overlap_bad      the byte ranges search2_body's comment names: the window = bytes 0..511 of the V slot, candidate 25 of 4x4 block 0 = bytes
//                    400..415 of it, q3 = words 64..95 of the H slot
//   once_bad         bytes of the V array's predictions (26 candidates x 4 blocks x 16 B per slot) and of the pre table not written exactly once per
//                    pass, words of the H array not written exactly once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "s2_lane_layout.h"

namespace {
long fields_bad = 0, range_bad = 0, align_bad = 0, owner_bad = 0, overlap_bad = 0, once_bad = 0;

struct Array {
    std::vector<uint8_t> bytes;       // the array itself (touched through every address)
    std::vector<int> writes;          // per byte: writes of the pass being counted
    int slot_bytes;
    Array(int n, int slot) : bytes(n, 0), writes(n, 0), slot_bytes(slot) {}
    // an access of `size` bytes at `at` by thread t; `slot`: the slot it must stay in (-1: any), lo..hi: the byte range of that slot it must stay in
    void touch(int t, int at, int size, bool write, int slot, int lo, int hi, bool own_wave = true) {
        if (at < 0 || at + size > (int)bytes.size()) { ++range_bad; return; }
        if (size == 16 && (at & 15)) ++align_bad;
        const int s = at / slot_bytes, off = at - s * slot_bytes;
        if ((at + size - 1) / slot_bytes != s) ++range_bad;
        if (slot >= 0 && s != slot) ++range_bad;
        if (off < lo || off + size > hi) ++range_bad;
        if (write && own_wave && (s >> 1) != s2_wave(t)) ++owner_bad;
        for (int i = 0; i < size; ++i) {
            if (write) { bytes[at + i] = (uint8_t)t; ++writes[at + i]; }
            else (void)(volatile uint8_t &)bytes[at + i];
        }
    }
    void clear() { std::fill(writes.begin(), writes.end(), 0); }
};
}  // namespace

int main() {
    static_assert(s2_fields_fit() && s2_table_unpacks() && s2_aligned16(), "the header's own checks");
    static constexpr S2LaneTable tab = make_s2_lane();
    Array HT(S2_HT_BYTES, S2_HT_SLOT_BYTES), V(S2_V_BYTES, S2_V_SLOT_BYTES), PRE(S2_PRE_BYTES, S2_PRE_SLOT_BYTES);

    // ---- the table ----
    for (int t = 0; t < S2_THREADS; ++t) {
        const uint32_t want[S2F_COUNT] = {
            (uint32_t)s2_win_store(t), s2_k31_keep(t) >> 16, (uint32_t)s2_win_half_biased(t), (uint32_t)s2_win_row_biased(t), (uint32_t)s2_zero_half_bytes(t),
            (uint32_t)s2_zero_row(t), (uint32_t)s2_k_row(t), 0u, (uint32_t)s2_aw_read(t), (uint32_t)s2_wp_read(t), (uint32_t)s2_wp_store(t), (uint32_t)s2_zero_scatter(t)};
        static_assert(S2F_WIN_STORE == 0 && S2F_K31_KEEP_HI == 1 && S2F_WIN_HALF == 2 && S2F_WIN_ROW == 3 && S2F_ZERO_HALF == 4 && S2F_ZERO_ROW == 5 &&
                      S2F_K_ROW == 6 && S2F_NONE == 7 && S2F_AW_READ == 8 && S2F_WP_READ == 9 && S2F_WP_STORE == 10 && S2F_ZERO_SCATTER == 11 && S2F_COUNT == 12, "the order of `want`");
        for (int f = 0; f < S2F_COUNT; ++f) {
            if (want[f] > 0xffffu) ++fields_bad;
            if (s2_unpack(tab.w[t], f) != want[f] || s2_field(t, f) != want[f]) ++fields_bad;
        }
        for (int d = (S2F_COUNT + 1) / 2; d < S2_LANE_DWORDS; ++d) fields_bad += tab.w[t][d] != 0;      // the rest of the row is empty
        // the two fields the kernel uses as whole dwords
        if ((tab.w[t][S2F_K31_KEEP_HI >> 1] | 0xffffu) != s2_k31_keep(t)) ++fields_bad;
        if (tab.w[t][S2F_K_ROW >> 1] != (uint32_t)s2_k_row(t)) ++fields_bad;
        if (((~s2_k31_keep(t)) & 0x01000000u) != s2_k31_one(t)) ++fields_bad;
        if (s2_k_row(t) < 0 || s2_k_row(t) + 16 > 64 * 16) ++range_bad;                                 // K_BH, K_AV: 64 rows of 16 bytes
        if (s2_win_row(t) < 0 || s2_win_row(t) > 15 || (s2_win_half_bytes(t) != 0 && s2_win_half_bytes(t) != 16)) ++range_bad;
        if (s2_win_row_biased(t) < 0 || s2_win_half_biased(t) < 0) ++range_bad;                         // the lane's offset from the moved base never goes down
        if (s2_zero_row(t) < 0 || s2_zero_row(t) > 7 || (s2_zero_half_bytes(t) != 0 && s2_zero_half_bytes(t) != 4)) ++range_bad;
    }

    // ---- once per group: the current block's scatter, its read back, the pre table ----
    for (int t = 0; t < S2_THREADS; ++t)
        if (s2_lane(t) < 16)
            for (int j = 0; j < 4; ++j) PRE.touch(t, s2_cur_scatter(t) + 4 * j, 1, true, s2_slot(t), 80 * 4, 96 * 4);
    for (int s = 0; s < S2_SLOTS; ++s)
        for (int i = 80 * 4; i < 96 * 4; ++i) once_bad += PRE.writes[s * S2_PRE_SLOT_BYTES + i] != 1;       // the block's 64 bytes, once each
    PRE.clear();
    for (int t = 0; t < S2_THREADS; ++t) PRE.touch(t, s2_pre_cols(t), 16, false, s2_slot(t), 80 * 4, 96 * 4);
    for (int t = 0; t < S2_THREADS; ++t) {
        PRE.touch(t, s2_pre_store(t), 16, true, s2_slot(t), 0, S2_PRE_SLOT_BYTES);
        PRE.touch(t, s2_pre_store(t) + 32, 16, true, s2_slot(t), 0, S2_PRE_SLOT_BYTES);
    }
    for (int s = 0; s < S2_SLOTS; ++s)
        for (int i = 0; i < S2_PRE_SLOT_BYTES; ++i) {      // copies 0..4 by one lane each, the last copy by the lanes 10, 12, 14.. / 11, 13, 15..: eleven times
            const int w = PRE.writes[s * S2_PRE_SLOT_BYTES + i];
            once_bad += i < 80 * 4 ? w != 1 : w != 11;
        }

    // ---- per reference ----
    // the window: stored, read by the horizontal pass and by the whole-pel column, all inside bytes 0..511 of the V slot
    for (int t = 0; t < S2_THREADS; ++t) V.touch(t, s2_win_store(t), 16, true, s2_slot(t), 0, S2_WIN_BYTES);
    for (int s = 0; s < S2_SLOTS; ++s)
        for (int i = 0; i < S2_V_SLOT_BYTES; ++i) overlap_bad += V.writes[s * S2_V_SLOT_BYTES + i] != (i < S2_WIN_BYTES ? 1 : 0);     // exactly the first 512 bytes
    V.clear();
    for (int t = 0; t < S2_THREADS; ++t) {
        const int m = t & 31;
        V.touch(t, s2_aw_read(t), 16, false, s2_wave_slot(t) + (m >> 4), 0, S2_WIN_BYTES);
        if ((s2_aw_read(t) % S2_V_SLOT_BYTES) != (m & 15) * 32 + 16 * s2_k_half(t)) ++range_bad;      // row m & 15 of the window, its k half
        for (int rr = 0; rr < 4; ++rr) V.touch(t, s2_wp_read(t) + 32 * rr, 1, false, s2_slot(t), 0, S2_WIN_BYTES);
    }
    // the H array: the horizontal pass's four dwords per lane and the whole-pel column's one -- every word of x cases 0..4, columns 0..7, once
    for (int t = 0; t < S2_THREADS; ++t) {
        for (int q = 0; q < 4; ++q) {
            const int at = s2_ht_store(t) + s2_ht_store_step(q);
            HT.touch(t, at, 4, true, s2_wave_slot(t) + (q >> 1), 0, S2_HT_SLOT_BYTES);
        }
        HT.touch(t, s2_wp_store(t), 4, true, s2_slot(t), 2 * HT_XC * 4, 3 * HT_XC * 4);
    }
    for (int s = 0; s < S2_SLOTS; ++s)
        for (int xc = 0; xc < 5; ++xc)
            for (int i = 0; i < HT_XC * 4; ++i) once_bad += HT.writes[s * S2_HT_SLOT_BYTES + xc * HT_XC * 4 + i] != (i < 8 * 16 ? 1 : 0);     // (the skew's 16 bytes stay unwritten)
    HT.clear();
    // the zero-vector block: candidate 25 of the four 4x4 blocks; of block 0, bytes 400..415 of the slot
    for (int t = 0; t < S2_THREADS; ++t)
        for (int j = 0; j < 4; ++j) V.touch(t, s2_zero_scatter(t) + 4 * j, 1, true, s2_slot(t), 0, S2_V_SLOT_BYTES);
    for (int s = 0; s < S2_SLOTS; ++s)
        for (int i = 0; i < S2_V_SLOT_BYTES; ++i) {
            const int blk = i / (V_ROW * 4), in = i - blk * V_ROW * 4;
            const bool zero = in >= V_ZERO * V_CAND * 4;        // the last 16 bytes of a 4x4 block's row
            // (both halves of a block's lanes scatter the same eight rows: twice each)
            if (V.writes[s * S2_V_SLOT_BYTES + i] != (zero ? 2 : 0)) ++once_bad;
            if (blk == 0 && zero && !(i >= 400 && i < 416)) ++overlap_bad;
        }
    if (!(V_ZERO * V_CAND * 4 == 400 && 416 <= S2_WIN_BYTES)) ++overlap_bad;
    V.clear();
    // the vertical pass: 16-byte reads of the H array, five dwords per active lane into the V array -- every prediction byte of candidates 0..24 once
    for (int t = 0; t < S2_THREADS; ++t)
        for (int i = 0; i < 3; ++i) {
            HT.touch(t, s2_hv_read(t, i), 16, false, -1, 0, 5 * HT_XC * 4);
            if ((s2_hv_read(t, i) / S2_HT_SLOT_BYTES) >> 1 != s2_wave(t)) ++range_bad;       // a slot of its own wave
            if (!s2_v_on(t, i)) continue;
            for (int yc = 0; yc < 5; ++yc) {
                const int at = s2_sv_store(t, i) + s2_sv_store_step(yc);
                V.touch(t, at, 4, true, -1, 0, S2_V_SLOT_BYTES);
            }
        }
    for (int s = 0; s < S2_SLOTS; ++s)
        for (int i = 0; i < S2_V_SLOT_BYTES; ++i) {
            const int in = i % (V_ROW * 4);
            once_bad += V.writes[s * S2_V_SLOT_BYTES + i] != (in < V_ZERO * V_CAND * 4 ? 1 : 0);
        }
    V.clear();
    // the cost phase: three rounds per lane, q3 in words 64..95 of the H slot, then the one wave's fourth-block round, then the read back
    for (int t = 0; t < S2_THREADS; ++t)
        for (int j = 0; j < 3; ++j) {
            V.touch(t, s2_cost_src(t) + j * s2_cost_step(t), 16, false, s2_slot(t), 0, S2_V_SLOT_BYTES);
            PRE.touch(t, s2_cost_pre(t) + 64 * j, 64, false, s2_slot(t), 0, S2_PRE_SLOT_BYTES);
            HT.touch(t, s2_cost_dst(t) + 4 * j, 4, true, s2_slot(t), S2_Q3_WORD * 4, (S2_Q3_WORD + 32) * 4);
        }
    for (int t = 0; t < 64; ++t) {       // (whichever wave takes the round: its lanes' numbers in the wave decide)
        V.touch(t, s2_extra_src(t), 16, false, s2_extra_slot(t), 3 * V_ROW * 4, S2_V_SLOT_BYTES);
        PRE.touch(t, s2_extra_pre(t), 64, false, s2_extra_slot(t), 48 * 4, 64 * 4);
        HT.touch(t, s2_extra_dst(t), 4, true, s2_extra_slot(t), (S2_Q3_WORD + 18) * 4, (S2_Q3_WORD + 26) * 4, false);
        for (int w = 1; w < 4; ++w)
            if (s2_extra_src(t + 64 * w) != s2_extra_src(t) || s2_extra_pre(t + 64 * w) != s2_extra_pre(t) || s2_extra_dst(t + 64 * w) != s2_extra_dst(t)) ++range_bad;
    }
    for (int s = 0; s < S2_SLOTS; ++s)
        for (int w = 0; w < 5 * HT_XC; ++w) {     // candidates 0..25 once, words 29..31 by the 26 lanes nobody reads, nothing else
            const int n = HT.writes[s * S2_HT_SLOT_BYTES + 4 * w], q = w - S2_Q3_WORD;
            const int want = q >= 0 && q < 26 ? 1 : q >= 29 && q < 32 ? 26 : 0;
            if (n != want) { ++once_bad; if (q >= 18 && q < 26) ++owner_bad; }
        }
    for (int t = 0; t < S2_THREADS; ++t) HT.touch(t, s2_cost_q3_read(t), 4, false, s2_slot(t), S2_Q3_WORD * 4, (S2_Q3_WORD + 32) * 4);
    if (!((S2_Q3_WORD + 32) * 4 <= S2_HT_SLOT_BYTES)) ++overlap_bad;

    std::printf("fields_bad %ld\nrange_bad %ld\nalign_bad %ld\nowner_bad %ld\noverlap_bad %ld\nonce_bad %ld\n", fields_bad, range_bad, align_bad, owner_bad, overlap_bad, once_bad);
    std::printf("threads %d\nfields %d\nrow_bytes %d\nlds_bytes %d\n", S2_THREADS, (int)S2F_COUNT, S2_LANE_DWORDS * 4, S2_HT_BYTES + S2_V_BYTES + S2_PRE_BYTES);
    return 0;
}
