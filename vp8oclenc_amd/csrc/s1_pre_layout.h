// Where the whole-pel search's loop form (kernels_me.hip: k_search1_pl, k_search1_plr_b) keeps the current blocks' share of the metric
// in LDS: s_pre[wave][block slot][sub-block][16 ints], twelve block slots per wave, made by s1_make_pre and read back as the C input of the
// metric's MFMA, 16 ints = four ds_read_b128 per candidate.  Lane l of a wave reads block slot l / 5 (five lanes per block; lanes 60-63 have no block
// and read slot 0), while the sub-block sb and the quad j are the same for the whole wave: the lanes of one read differ ONLY in their slot.
// With a slot of 64 ints (256 bytes: the whole bank row) every slot starts at bank 0 and the five or six slots that meet in a lane group of the read
// queue up on the same four banks: 22 LDS cycles for the wave where a conflict-free read takes 4 (lds_bank_model.h).  With 68 ints (272 bytes, still
// 16-byte aligned) slot s starts at bank 4 s mod 64: twelve slots, twelve different bank quads.
// In a header of its own so that the kernels, the compile-time check next to them and the host program of tests/test_lds_bank_model.py (scripts/native/
// lds_bank_model.cpp) share one statement of the address.
#pragma once
#include "lds_bank_model.h"

constexpr int S1_PRE_BLOCKS = 12;                        // block slots per wave (S1Map<false>::BLOCKS_PER_WAVE)
constexpr int S1_PRE_SLOT = 68;                          // ints per block slot: 4 sub-blocks x 16 + 4 of bank skew
constexpr int S1_PRE_INTS = S1_PRE_BLOCKS * S1_PRE_SLOT; // ints per wave

// int index, in s_pre, of block slot `slot` of wave `wave` (a slot past the twelfth: slot 0) ...
LDS_MODEL_HD constexpr int s1_pre_slot_at(int wave, int slot, int slot_ints = S1_PRE_SLOT) {
    return wave * (S1_PRE_BLOCKS * slot_ints) + (slot < S1_PRE_BLOCKS ? slot : 0) * slot_ints;
}
// ... and of quad j of sub-block sb inside a slot
LDS_MODEL_HD constexpr int s1_pre_sub_at(int sb, int j = 0) { return 16 * sb + 4 * j; }
// the C read of a lane: the int index of the j-th ds_read_b128 of sub-block sb
LDS_MODEL_HD constexpr int s1_pre_c_at(int wave, int lane, int sb, int j, int slot_ints = S1_PRE_SLOT) {
    return s1_pre_slot_at(wave, lane / 5, slot_ints) + s1_pre_sub_at(sb, j);
}
// The same two as BYTE offsets, the form the kernels carry: a lane's address goes to the ds_read_b128 as it stands, the quad in the instruction's
// offset field, with no shift per read
LDS_MODEL_HD constexpr int s1_pre_sub_bytes(int sb, int j = 0) { return 4 * s1_pre_sub_at(sb, j); }
LDS_MODEL_HD constexpr int s1_pre_c_bytes(int wave, int lane, int sb, int j, int slot_ints = S1_PRE_SLOT) {
    return 4 * s1_pre_slot_at(wave, lane / 5, slot_ints) + s1_pre_sub_bytes(sb, j);
}

// LDS cycles of that read for the whole wave
LDS_MODEL_HD constexpr int s1_pre_c_read_cycles(int wave, int sb, int j, int slot_ints = S1_PRE_SLOT, unsigned long long exec = ~0ull) {
    lds_model::WaveAddrs w{};
    for (int l = 0; l < 64; ++l) w.a[l] = (unsigned)s1_pre_c_bytes(wave, l, sb, j, slot_ints);
    return lds_model::ds_read_b128_cycles(w, exec);
}
// the most any C read of the table costs: every wave, sub-block and quad
LDS_MODEL_HD constexpr int s1_pre_c_read_worst(int slot_ints = S1_PRE_SLOT, unsigned long long exec = ~0ull) {
    int worst = 0;
    for (int wave = 0; wave < 4; ++wave)
        for (int sb = 0; sb < 4; ++sb)
            for (int j = 0; j < 4; ++j) {
                const int c = s1_pre_c_read_cycles(wave, sb, j, slot_ints, exec);
                worst = c > worst ? c : worst;
            }
    return worst;
}
LDS_MODEL_HD constexpr int s1_pre_c_read_best(int slot_ints = S1_PRE_SLOT, unsigned long long exec = ~0ull) {
    int best = 1 << 30;
    for (int wave = 0; wave < 4; ++wave)
        for (int sb = 0; sb < 4; ++sb)
            for (int j = 0; j < 4; ++j) {
                const int c = s1_pre_c_read_cycles(wave, sb, j, slot_ints, exec);
                best = c < best ? c : best;
            }
    return best;
}
static_assert(S1_PRE_SLOT % 4 == 0 && S1_PRE_SLOT >= 64, "a block slot of the pre table holds 4 x 16 ints and keeps its 16-byte alignment");
