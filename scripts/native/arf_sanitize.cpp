// arf_sanitize.cpp -- vp8host_arf_filter_frame under the host sanitizers.  Every plane of every frame of the window, the three output
// planes, the weights and the vector list are heap blocks of exactly their size: a read outside a source plane (the search window
// reaches 8 samples over every edge and the extension 15 past the last column and row) or a write past an output is a heap overflow.
// Sizes with whole, cut and single tiles, windows of 1, 2, 4 and 7 frames, every centre, strengths 0, 3 and 6, noise and flat
// content, every refusal; the division helper over every pair of the rule.  No GPU, no library: it is linked with vp8_host.cpp alone.
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include scripts/native/arf_sanitize.cpp \
//       vp8oclenc_amd/csrc/vp8_host.cpp -o arf_sanitize && ./arf_sanitize
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "vp8hip_host.h"

int main() {
    unsigned seed = 1;
    auto next = [&] { seed = seed * 1664525u + 1013904223u; return (uint8_t)(seed >> 24); };
    const int sizes[][2] = {{2, 2}, {16, 16}, {18, 14}, {40, 24}, {64, 48}, {56, 40}}, counts[] = {1, 2, 4, 7}, strengths[] = {0, 3, 6};
    long checked = 0;
    for (const auto &sz : sizes)
        for (int n : counts)
            for (int strength : strengths)
                for (int content = 0; content < 2; ++content) {
                    const int w = sz[0], h = sz[1], tiles = ((w + 15) / 16) * ((h + 15) / 16);
                    const size_t ny = (size_t)w * h, nc = (size_t)(w / 2) * (h / 2);
                    std::vector<std::unique_ptr<uint8_t[]>> planes;
                    std::vector<const uint8_t *> table;
                    for (int k = 0; k < n; ++k)
                        for (int p = 0; p < 3; ++p) {
                            const size_t bytes = p ? nc : ny;
                            planes.emplace_back(new uint8_t[bytes]);
                            for (size_t i = 0; i < bytes; ++i) planes.back()[i] = content ? (uint8_t)(100 + k) : (uint8_t)(128 + (next() >> 3) + (i % 7) * 9);
                            table.push_back(planes.back().get());
                        }
                    std::unique_ptr<uint8_t[]> oy(new uint8_t[ny]), ou(new uint8_t[nc]), ov(new uint8_t[nc]);
                    std::unique_ptr<int32_t[]> weights(new int32_t[3]);
                    std::unique_ptr<int8_t[]> vectors(new int8_t[(size_t)tiles * n * 2]);
                    for (int centre = 0; centre < n; ++centre) {
                        if (vp8host_arf_filter_frame(table.data(), n, centre, strength, w, h, oy.get(), ou.get(), ov.get(), weights.get(), vectors.get()) != 0 ||
                            vp8host_arf_filter_frame(table.data(), n, centre, strength, w, h, oy.get(), ou.get(), ov.get(), nullptr, nullptr) != 0) {
                            fprintf(stderr, "refused: %dx%d n %d centre %d strength %d\n", w, h, n, centre, strength);
                            return 1;
                        }
                        if (weights[0] + weights[1] + weights[2] != tiles * (n - 1)) { fprintf(stderr, "weights do not add up\n"); return 1; }
                        if (content == 1)      // flat frames: every candidate ties, the zero vector wins, and the output lies between the frames
                            for (size_t i = 0; i < (size_t)tiles * n * 2; ++i)
                                if (vectors[i]) { fprintf(stderr, "flat frames: a vector that is not zero\n"); return 1; }
                        if (n == 1 && (memcmp(oy.get(), table[0], ny) || memcmp(ou.get(), table[1], nc) || memcmp(ov.get(), table[2], nc))) {
                            fprintf(stderr, "n = 1 did not return the centre frame\n");
                            return 1;
                        }
                        checked += tiles;
                    }
                }
    {   // the division: every count of the rule, every acc below 65536
        std::vector<uint32_t> acc(65536), count(65536), out(65536);
        for (uint32_t c = 32; c <= 224; ++c) {
            for (uint32_t a = 0; a < 65536; ++a) { acc[a] = a; count[a] = c; }
            vp8host_arf_round_divide(acc.data(), count.data(), acc.size(), out.data());
            for (uint32_t a = 0; a < 65536; ++a)
                if (out[a] != (a + c / 2) / c) { fprintf(stderr, "division: acc %u count %u gives %u\n", a, c, out[a]); return 1; }
        }
    }
    {   // the refusals
        uint8_t y[256] = {0}, o[256];
        const uint8_t *one[3] = {y, y, y}, *hole[3] = {y, nullptr, y};
        const int bad[][5] = {{0, 0, 3, 16, 16}, {8, 0, 3, 16, 16}, {1, 1, 3, 16, 16}, {1, -1, 3, 16, 16}, {1, 0, 7, 16, 16}, {1, 0, -1, 16, 16},
                              {1, 0, 3, 15, 16}, {1, 0, 3, 16, 15}, {1, 0, 3, 0, 16}};      // n, centre, strength, width, height
        for (const auto &b : bad)
            if (vp8host_arf_filter_frame(one, b[0], b[1], b[2], b[3], b[4], o, o, o, nullptr, nullptr) == 0) {
                fprintf(stderr, "not refused: %d %d %d %d %d\n", b[0], b[1], b[2], b[3], b[4]);
                return 1;
            }
        if (vp8host_arf_filter_frame(nullptr, 1, 0, 3, 16, 16, o, o, o, nullptr, nullptr) == 0 || vp8host_arf_filter_frame(hole, 1, 0, 3, 16, 16, o, o, o, nullptr, nullptr) == 0 ||
            vp8host_arf_filter_frame(one, 1, 0, 3, 16, 16, nullptr, o, o, nullptr, nullptr) == 0) {
            fprintf(stderr, "a null pointer was not refused\n");
            return 1;
        }
    }
    printf("clean (%ld)\n", checked);
    return 0;
}
