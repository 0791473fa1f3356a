// The lane map and the LDS table of the whole-pel search's FILLED loop form (kernels_me.hip: k_search1_plr_b, the form batches launch).  Five lanes
// per 8x8 block give twelve blocks to a wave of 64 lanes and leave four lanes idle, while the metric's MFMA and everything behind it are issued for the
// whole wave.  Numbered across the workgroup instead, the 256 lanes hold 51 blocks x 5 lanes = 255 lanes: lane t has block slot t / 5 and candidate row
// t % 5, and the workgroup `tile` takes blocks tile * 51 + slot.  Slots 12, 25 and 38 lie in two waves.  Lane 255 has no block: like every lane
// whose slot has none it searches the frame's LAST block (harmless in-frame data, nothing stored), and its C reads go to the last slot with its
// neighbours' (parked on slot 0 it would meet slot 48 on one bank quad).
// The current blocks' share of the metric, s_pre[block slot][sub-block][16 ints], is made by the whole workgroup (lane t < 204: slot t >> 2, sub-block
// t & 3) and read back, behind a barrier, as the C input of the metric's MFMA: the lanes of a wave's ds_read_b128 differ only in their slot, 13 or 14
// consecutive ones.  The slot stride is S1_PRE_SLOT = 68 ints, as in s1_pre_layout.h and for its reason: slot s starts at bank 4 s mod 64, and 14
// consecutive slots start on 14 different bank quads of the 16.
// In a header of its own so that the kernel, the compile-time check next to it and the host program of tests/test_s1_fill_layout.py (scripts/native/
// s1_fill_layout_sanitize.cpp) share one statement of the map and of the address.
#pragma once
#include "s1_pre_layout.h"

constexpr int S1_FILL_LANES = 5;                                  // lanes per block: one per candidate row
constexpr int S1_FILL_BLOCKS = 51;                                // block slots per workgroup of 256 lanes
constexpr int S1_FILL_INTS = S1_FILL_BLOCKS * S1_PRE_SLOT;        // ints of the workgroup's table
constexpr int S1_FILL_MIN_WORDS = 256 + S1_FILL_LANES - 1;        // words of one buffer of the block minimum: every lane reads the five from its block's first

// the block slot of workgroup lane t (0..51; 51 = lane 255: no block) and its candidate row
LDS_MODEL_HD constexpr int s1_fill_slot_of(int t) { return t / S1_FILL_LANES; }
LDS_MODEL_HD constexpr int s1_fill_sub_of(int t) { return t % S1_FILL_LANES; }
// workgroups of a launch over nblk blocks, and the block of (workgroup, slot): < 0 where the slot has none
LDS_MODEL_HD constexpr int s1_fill_grid(int nblk) { return (nblk + S1_FILL_BLOCKS - 1) / S1_FILL_BLOCKS; }
LDS_MODEL_HD constexpr int s1_fill_block_of(int tile, int slot, int nblk) {
    return slot < S1_FILL_BLOCKS && tile * S1_FILL_BLOCKS + slot < nblk ? tile * S1_FILL_BLOCKS + slot : -1;
}
// the first of the five words of the block minimum that workgroup lane t reads, in a buffer of S1_FILL_MIN_WORDS; its own word is
// s1_fill_min_at(t) + s1_fill_sub_of(t) = t.  (Lane 255 reads words 255..259, of which 256..259 are never written: its minimum is never used.)
LDS_MODEL_HD constexpr int s1_fill_min_at(int t) { return t - s1_fill_sub_of(t); }
// int index, in s_pre, of block slot `slot` (a slot past the last: the last)
LDS_MODEL_HD constexpr int s1_fill_slot_at(int slot, int slot_ints = S1_PRE_SLOT) { return (slot < S1_FILL_BLOCKS ? slot : S1_FILL_BLOCKS - 1) * slot_ints; }
// the producer's task of workgroup lane t: (slot, sub-block); lanes 204..255 have none
LDS_MODEL_HD constexpr int s1_fill_task_slot(int t) { return t >> 2; }
LDS_MODEL_HD constexpr int s1_fill_task_sub(int t) { return t & 3; }
// the C read of workgroup lane t: the int index of the j-th ds_read_b128 of sub-block sb (s1_pre_sub_at: s1_pre_layout.h)
LDS_MODEL_HD constexpr int s1_fill_c_at(int t, int sb, int j, int slot_ints = S1_PRE_SLOT) {
    return s1_fill_slot_at(s1_fill_slot_of(t), slot_ints) + s1_pre_sub_at(sb, j);
}
// ... and its byte offset, which is what the kernel carries (s1_pre_sub_bytes: s1_pre_layout.h)
LDS_MODEL_HD constexpr int s1_fill_c_bytes(int t, int sb, int j, int slot_ints = S1_PRE_SLOT) {
    return 4 * s1_fill_slot_at(s1_fill_slot_of(t), slot_ints) + s1_pre_sub_bytes(sb, j);
}

// LDS cycles of that read for wave `wave` of the workgroup
LDS_MODEL_HD constexpr int s1_fill_c_read_cycles(int wave, int sb, int j, int slot_ints = S1_PRE_SLOT, unsigned long long exec = ~0ull) {
    lds_model::WaveAddrs w{};
    for (int l = 0; l < 64; ++l) w.a[l] = (unsigned)s1_fill_c_bytes(64 * wave + l, sb, j, slot_ints);
    return lds_model::ds_read_b128_cycles(w, exec);
}
// the most and the least any C read of the table costs: every wave, sub-block and quad
LDS_MODEL_HD constexpr int s1_fill_c_read_worst(int slot_ints = S1_PRE_SLOT, unsigned long long exec = ~0ull) {
    int worst = 0;
    for (int wave = 0; wave < 4; ++wave)
        for (int sb = 0; sb < 4; ++sb)
            for (int j = 0; j < 4; ++j) {
                const int c = s1_fill_c_read_cycles(wave, sb, j, slot_ints, exec);
                worst = c > worst ? c : worst;
            }
    return worst;
}
LDS_MODEL_HD constexpr int s1_fill_c_read_best(int slot_ints = S1_PRE_SLOT, unsigned long long exec = ~0ull) {
    int best = 1 << 30;
    for (int wave = 0; wave < 4; ++wave)
        for (int sb = 0; sb < 4; ++sb)
            for (int j = 0; j < 4; ++j) {
                const int c = s1_fill_c_read_cycles(wave, sb, j, slot_ints, exec);
                best = c < best ? c : best;
            }
    return best;
}
static_assert(S1_FILL_BLOCKS * S1_FILL_LANES <= 256 && (S1_FILL_BLOCKS + 1) * S1_FILL_LANES > 256, "as many whole blocks as a workgroup of 256 lanes holds");
static_assert(4 * S1_FILL_BLOCKS <= 256, "the workgroup makes its table in one pass: a lane per (slot, sub-block)");
