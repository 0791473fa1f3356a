// The filled loop form's lane map and LDS table (csrc/s1_fill_layout.h: what k_search1_plr_b indexes by) walked on the host, under the address and
// undefined-behaviour sanitizers; no GPU:
//     g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -I vp8oclenc_amd/csrc scripts/native/s1_fill_layout_sanitize.cpp -o t && ./t
// One `name value` pair per line (tests/test_s1_fill_layout.py reads them):
//   owners_bad       over nblk = 1..400: blocks NOT owned by exactly five lanes (candidate rows 0..4, once each) of exactly one workgroup
//   slots_bad        lanes that address a table slot >= 51, a table int outside [0, S1_FILL_INTS) or a word of the minimum outside its buffer
//   tasks_bad        (workgroup, slot < 51) pairs whose table slot is not made by exactly four producer lanes (sub-blocks 0..3, once each)
//   straddling       the slots whose five lanes lie in two waves
//   c_stride         the slot stride in ints, c_read the LDS cycles of a C read (min = max printed as one number), c_read_stride64 the same with
//                    slots of 64 ints (the check can fail)
// The table and the minimum's buffer are real arrays here, written and read through the header's addresses: an index out of range is the sanitizer's.
#include <cstdio>
#include <vector>

#include "s1_fill_layout.h"

static void print_range(const char *name, int lo, int hi) {
    if (lo == hi) std::printf("%s %d\n", name, lo);
    else std::printf("%s %d..%d\n", name, lo, hi);
}

int main() {
    long owners_bad = 0, slots_bad = 0, tasks_bad = 0;
    for (int nblk = 1; nblk <= 400; ++nblk) {
        const int grid = s1_fill_grid(nblk);
        std::vector<int> rows(nblk, 0), lanes(nblk, 0), wg(nblk, -1);      // per block: the candidate rows met (bits), the lanes, the workgroup
        for (int tile = 0; tile < grid; ++tile) {
            std::vector<int> table(S1_FILL_INTS, 0);           // how many producer lanes wrote each int
            std::vector<unsigned> mins(S1_FILL_MIN_WORDS, 0u);
            for (int t = 0; t < 256; ++t) {                    // the producers: lane t = (slot, sub-block), 16 ints
                const int slot = s1_fill_task_slot(t), sb = s1_fill_task_sub(t);
                if (slot >= S1_FILL_BLOCKS) continue;
                for (int k = 0; k < 16; ++k) ++table[s1_fill_slot_at(slot) + s1_pre_sub_at(sb) + k];
            }
            for (int slot = 0; slot < S1_FILL_BLOCKS; ++slot)
                for (int k = 0; k < 64; ++k) tasks_bad += table[slot * S1_PRE_SLOT + k] != 1;
            for (int t = 0; t < 256; ++t) {                    // the consumers
                const int slot = s1_fill_slot_of(t), sub = s1_fill_sub_of(t);
                for (int sb = 0; sb < 4; ++sb)
                    for (int j = 0; j < 4; ++j) {
                        const int at = s1_fill_c_at(t, sb, j);
                        if (at < 0 || at + 4 > S1_FILL_INTS || at / S1_PRE_SLOT >= S1_FILL_BLOCKS) { ++slots_bad; continue; }
                        if (slot < S1_FILL_BLOCKS && (at / S1_PRE_SLOT != slot || table[at] != 1)) ++slots_bad;
                    }
                const int first = s1_fill_min_at(t);           // the minimum: this lane's word, and the five it reads
                if (first < 0 || first + sub != t || first + S1_FILL_LANES > S1_FILL_MIN_WORDS) ++slots_bad;
                else {
                    mins[first + sub] += 1u;
                    for (int k = 0; k < S1_FILL_LANES; ++k) (void)mins[first + k];
                }
                const int b = s1_fill_block_of(tile, slot, nblk);
                if (b < 0) continue;
                if (b >= nblk) { ++owners_bad; continue; }
                rows[b] |= 1 << sub;
                ++lanes[b];
                if (wg[b] >= 0 && wg[b] != tile) ++owners_bad;
                wg[b] = tile;
            }
            for (int t = 0; t < 256; ++t) slots_bad += mins[t] != 1u;      // every lane has a word of its own
        }
        for (int b = 0; b < nblk; ++b) owners_bad += !(rows[b] == 31 && lanes[b] == 5 && wg[b] == b / S1_FILL_BLOCKS);
    }
    std::printf("owners_bad %ld\nslots_bad %ld\ntasks_bad %ld\n", owners_bad, slots_bad, tasks_bad);
    std::printf("straddling");
    const char *sep = " ";
    for (int slot = 0; slot < S1_FILL_BLOCKS; ++slot)
        if ((slot * S1_FILL_LANES) / 64 != (slot * S1_FILL_LANES + S1_FILL_LANES - 1) / 64) {
            std::printf("%s%d", sep, slot);
            sep = ",";
        }
    std::printf("\nc_stride %d\n", S1_PRE_SLOT);
    print_range("c_read", s1_fill_c_read_best(), s1_fill_c_read_worst());
    print_range("c_read_stride64", s1_fill_c_read_best(64), s1_fill_c_read_worst(64));
    std::printf("lds_bytes %d\n", (int)(4 * (S1_FILL_INTS + 2 * S1_FILL_MIN_WORDS)));
    return 0;
}
