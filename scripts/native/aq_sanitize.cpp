// aq_sanitize.cpp -- vp8host_aq_segment_map under the host sanitizers.  The luma plane is a heap block that ends with the LAST sample
// of the last row (a stride larger than the width leaves no spare bytes behind it), the map and e are blocks of exactly one byte per
// macroblock: a read behind the plane or a write past either array is a heap overflow.  Four sizes, three strides, three strengths,
// flat and extreme content, every refusal.  No GPU, no library: it is linked with vp8_host.cpp alone.
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include scripts/native/aq_sanitize.cpp \
//       vp8oclenc_amd/csrc/vp8_host.cpp -o aq_sanitize && ./aq_sanitize
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "vp8hip_host.h"

int main() {
    unsigned seed = 1;
    auto next = [&] { seed = seed * 1664525u + 1013904223u; return (uint8_t)(seed >> 24); };
    const int sizes[][2] = {{16, 16}, {48, 32}, {80, 48}, {176, 144}}, extra[] = {0, 5, 64};
    long checked = 0;
    for (const auto &sz : sizes)
        for (int ex : extra)
            for (int strength = 1; strength <= 3; ++strength)
                for (int content = 0; content < 3; ++content) {
                    const int w = sz[0], h = sz[1], stride = w + ex, mbs = (w / 16) * (h / 16);
                    const size_t span = (size_t)(h - 1) * stride + w;
                    std::unique_ptr<uint8_t[]> y(new uint8_t[span]), map(new uint8_t[mbs]), e(new uint8_t[mbs]);
                    for (size_t i = 0; i < span; ++i) y[i] = content == 0 ? next() : (content == 1 ? 77 : ((i / 8) & 1 ? 255 : 0));
                    if (vp8host_aq_segment_map(y.get(), stride, w, h, strength, map.get(), e.get()) != 0 ||
                        vp8host_aq_segment_map(y.get(), stride, w, h, strength, map.get(), nullptr) != 0) {
                        fprintf(stderr, "refused: %dx%d stride %d strength %d\n", w, h, stride, strength);
                        return 1;
                    }
                    long total = 0;
                    for (int i = 0; i < mbs; ++i) total += e[i];
                    const int W = strength == 1 ? 24 : (strength == 2 ? 16 : 12), E = (int)(total / mbs);
                    for (int i = 0; i < mbs; ++i) {
                        if (e[i] > 239 || map[i] > 3 || map[i] != vp8host_aq_segment(e[i], E, W)) { fprintf(stderr, "macroblock %d: e %d, segment %d\n", i, e[i], map[i]); return 1; }
                        if (content == 1 && (e[i] != 0 || map[i] != 2)) { fprintf(stderr, "a flat macroblock: e %d, segment %d\n", e[i], map[i]); return 1; }
                    }
                    checked += mbs;
                }
    {   // the refusals
        uint8_t y[256] = {0}, m[1];
        const int bad[][4] = {{15, 16, 16, 1}, {16, 16, 15, 1}, {16, 16, 0, 1}, {16, 32, 16, 1}, {32, 24, 16, 1}, {16, 16, 24, 1}, {16, 16, 16, 0}, {16, 16, 16, 4}};      // stride, width, height, strength
        for (const auto &b : bad)
            if (vp8host_aq_segment_map(y, b[0], b[1], b[2], b[3], m, nullptr) == 0) { fprintf(stderr, "not refused: %d %d %d %d\n", b[0], b[1], b[2], b[3]); return 1; }
        if (vp8host_aq_segment_map(nullptr, 16, 16, 16, 1, m, nullptr) == 0 || vp8host_aq_segment_map(y, 16, 16, 16, 1, nullptr, nullptr) == 0) {
            fprintf(stderr, "a null pointer was not refused\n");
            return 1;
        }
    }
    printf("clean (%ld)\n", checked);
    return 0;
}
