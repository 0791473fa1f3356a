// The LDS bank model (csrc/lds_bank_model.h) on the reads the two search kernels feed their metric's MFMA with; host code, no GPU:
//     c++ -std=c++17 -I vp8oclenc_amd/csrc scripts/native/lds_bank_model.cpp -o lds_bank_model && ./lds_bank_model
// One `name value` pair per line (tests/test_lds_bank_model.py reads them):
//   s1_c_*        the C read of the whole-pel search's loop form (s1_pre_layout.h: the address the kernels use), LDS cycles of one ds_read_b128 of
//                 the wave, the same for every wave, sub-block and quad (min = max is printed as one number, otherwise as min..max):
//                 with block slots of 64 ints, as they were, and with the table's stride as it is; `live`: only the sixty lanes that have a block
//                 (the count the layout was first judged by), otherwise the whole wave as the kernel issues the read, lanes 60-63 parked on slot 0
//   s2_b_*, s2_c_* k_search2's cost phase (kernels_s2.hip, SPREAD), rounds j = 0..2: the B read of a task's 16 prediction bytes and the four C reads;
//                 reported, not bounded.  The address arithmetic is restated here from search2_body (V_CAND, V_ROW, V_SLOT, PRE_SLOT).
#include <cstdio>

#include "s1_pre_layout.h"

static void print_range(const char *name, int lo, int hi) {
    if (lo == hi) std::printf("%s %d\n", name, lo);
    else std::printf("%s %d..%d\n", name, lo, hi);
}

int main() {
    constexpr unsigned long long LIVE = (1ull << 60) - 1;     // lanes 0..59: twelve blocks of five lanes
    print_range("s1_c_stride64_live", s1_pre_c_read_best(64, LIVE), s1_pre_c_read_worst(64, LIVE));
    print_range("s1_c_stride64_wave", s1_pre_c_read_best(64), s1_pre_c_read_worst(64));
    std::printf("s1_stride %d\n", S1_PRE_SLOT);
    print_range("s1_c_stride_live", s1_pre_c_read_best(S1_PRE_SLOT, LIVE), s1_pre_c_read_worst(S1_PRE_SLOT, LIVE));
    print_range("s1_c_stride_wave", s1_pre_c_read_best(), s1_pre_c_read_worst());
    static_assert(s1_pre_c_read_worst() == 4, "checked where the kernels are compiled too");

    // k_search2, cost phase: a wave = two block slots g (lanes 0-31, 32-63); lane k < 26 = candidate k, 4x4 block j in round j; lanes 26-31 help
    // with 4x4 block 3 of candidate 3 (lane - 26) + j
    constexpr int V_CAND = 4, V_ROW = 26 * V_CAND, V_SLOT = 4 * V_ROW, PRE_SLOT = 96;
    for (int j = 0; j < 3; ++j) {
        lds_model::WaveAddrs b{};
        for (int l = 0; l < 64; ++l) {
            const int g = l >> 5, k = l & 31;
            const bool helper = k >= 26;
            const int dw = g * V_SLOT + (helper ? 3 * V_ROW + (k - 26) * 3 * V_CAND + j * V_CAND : k * V_CAND + j * V_ROW);
            b.a[l] = 4u * (unsigned)dw;
        }
        std::printf("s2_b_round%d %d\n", j, lds_model::ds_read_b128_cycles(b));
        int lo = 1 << 30, hi = 0;
        for (int q = 0; q < 4; ++q) {
            lds_model::WaveAddrs c{};
            for (int l = 0; l < 64; ++l) c.a[l] = 4u * (unsigned)((l >> 5) * PRE_SLOT + ((l & 31) >= 26 ? 48 : 0) + 16 * j + 4 * q);
            const int cyc = lds_model::ds_read_b128_cycles(c);
            lo = cyc < lo ? cyc : lo;
            hi = cyc > hi ? cyc : hi;
        }
        char name[32];
        std::snprintf(name, sizeof name, "s2_c_round%d", j);
        print_range(name, lo, hi);
    }
    return 0;
}
