// compose_sanitize.cpp -- vp8host_compose_frame under the host sanitizers: the layouts of tests/compose_ref.py (identity, a grid whose
// seams fall off every unit, a letterbox with an overlap in both orders, a 31-tap tile, sixteen tiles with two absent and one of a
// single chroma sample), every source plane and every output plane in a heap block of exactly its size (a read or write past an end is
// a heap overflow), tight and pitched -- the last row of a pitched plane ends with its last sample, so a read of the bytes between the
// rows runs off the block -- with random, all-zero and all-ones samples (the sums of the two passes must stay inside their types).
// No GPU, no library: it is linked with vp8_host.cpp alone.
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include scripts/native/compose_sanitize.cpp \
//       vp8oclenc_amd/csrc/vp8_host.cpp -o compose_sanitize && ./compose_sanitize
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "vp8hip_host.h"

namespace {

struct Layout { int pw, ph; std::vector<vp8hip_tile> tiles; int bg[3]; unsigned absent; };

std::vector<Layout> layouts() {
    std::vector<Layout> l;
    for (int f = 0; f < 2; ++f) l.push_back({64, 48, {{64, 48, 0, 0, 64, 48, f}}, {16, 128, 128}, 0});
    for (int f = 0; f < 2; ++f) l.push_back({176, 144, {{352, 288, 0, 0, 88, 72, f}, {352, 288, 88, 0, 88, 72, f}, {352, 288, 0, 72, 88, 72, f}, {352, 288, 88, 72, 88, 72, f}}, {16, 128, 128}, 0});
    const vp8hip_tile a{100, 100, 42, 10, 36, 36, 1}, b{66, 34, 0, 14, 64, 32, 0};
    l.push_back({78, 46, {a, b}, {81, 90, 240}, 0});
    l.push_back({78, 46, {b, a}, {81, 90, 240}, 0});
    l.push_back({64, 48, {{992, 992, 16, 8, 32, 32, 0}}, {0, 255, 0}, 0});
    Layout g{64, 64, {}, {255, 0, 255}, (1u << 3) | (1u << 9)};
    for (int k = 0; k < 15; ++k) g.tiles.push_back({32, 32, 16 * (k % 4), 16 * (k / 4), 16, 16, 0});
    g.tiles.push_back({62, 62, 6, 10, 2, 2, 0});
    l.push_back(g);
    l.push_back({2, 2, {{2, 2, 0, 0, 2, 2, 0}}, {1, 2, 3}, 0});      // the smallest picture and tile (Lanczos-3 has more taps than such a plane has samples)
    return l;
}

}  // namespace

int main() {
    unsigned seed = 1;
    auto next = [&] { seed = seed * 1664525u + 1013904223u; return (uint8_t)(seed >> 24); };
    long checked = 0;
    for (const Layout &l : layouts())
        for (int pitched = 0; pitched < 2; ++pitched)
            for (int fill = 0; fill < 3; ++fill) {      // random bytes; all zero; all ones
                const int n = (int)l.tiles.size();
                std::vector<std::unique_ptr<uint8_t[]>> blocks;
                std::vector<vp8hip_tile_planes> src((size_t)n);
                for (int k = 0; k < n; ++k) {
                    src[(size_t)k] = vp8hip_tile_planes{};
                    if ((l.absent >> k) & 1u) continue;
                    const uint8_t *ptr[3];
                    int pitch[3];
                    for (int p = 0; p < 3; ++p) {
                        const int w = p ? l.tiles[(size_t)k].in_w / 2 : l.tiles[(size_t)k].in_w, h = p ? l.tiles[(size_t)k].in_h / 2 : l.tiles[(size_t)k].in_h;
                        pitch[p] = pitched ? w + (p ? 5 : 12) : 0;
                        const size_t nb = (size_t)(pitched ? pitch[p] : w) * (h - 1) + (size_t)w;      // exactly: nothing behind the last sample
                        blocks.emplace_back(new uint8_t[nb]);
                        for (size_t i = 0; i < nb; ++i) blocks.back()[i] = fill == 0 ? next() : (fill == 1 ? 0 : 255);
                        ptr[p] = blocks.back().get();
                    }
                    src[(size_t)k] = vp8hip_tile_planes{ptr[0], ptr[1], ptr[2], pitch[0], pitch[1], pitch[2]};
                }
                const size_t ob[3] = {(size_t)l.pw * l.ph, (size_t)(l.pw / 2) * (l.ph / 2), (size_t)(l.pw / 2) * (l.ph / 2)};
                std::unique_ptr<uint8_t[]> o[3];
                for (int k = 0; k < 3; ++k) o[k].reset(new uint8_t[ob[k]]);
                if (vp8host_compose_frame(l.pw, l.ph, l.tiles.data(), n, l.bg[0], l.bg[1], l.bg[2], src.data(), o[0].get(), o[1].get(), o[2].get()) != 0) {
                    fprintf(stderr, "refused: a layout of %d tiles on %dx%d\n", n, l.pw, l.ph);
                    return 1;
                }
                for (int k = 0; k < 3; ++k)
                    for (size_t i = 0; i < ob[k]; ++i) checked += o[k][i];
            }
    // the refusals touch nothing: one byte stands for every buffer
    uint8_t one[4] = {};
    const vp8hip_tile_planes p1{one, one, one, 0, 0, 0}, low{one, one, one, 1, 0, 0};
    const vp8hip_tile ok{2, 2, 0, 0, 2, 2, 0}, odd{2, 2, 1, 0, 2, 2, 0}, out{2, 2, 2, 0, 2, 2, 0}, up{2, 2, 0, 0, 4, 2, 0}, filter{2, 2, 0, 0, 2, 2, 2}, taps{66, 2, 0, 0, 2, 2, 0};
    const vp8hip_tile many[VP8HIP_MAX_TILES + 1] = {};
    if (vp8host_compose_frame(2, 2, &ok, 1, 0, 0, 0, &p1, one, one, one) != 0 || vp8host_compose_frame(2, 2, &odd, 1, 0, 0, 0, &p1, one, one, one) != -1 ||
        vp8host_compose_frame(2, 2, &out, 1, 0, 0, 0, &p1, one, one, one) != -1 || vp8host_compose_frame(4, 2, &up, 1, 0, 0, 0, &p1, one, one, one) != -1 ||
        vp8host_compose_frame(2, 2, &filter, 1, 0, 0, 0, &p1, one, one, one) != -1 || vp8host_compose_frame(2, 2, &taps, 1, 0, 0, 0, &p1, one, one, one) != -1 ||
        vp8host_compose_frame(2, 2, &ok, 1, 256, 0, 0, &p1, one, one, one) != -1 || vp8host_compose_frame(2, 2, &ok, 1, 0, -1, 0, &p1, one, one, one) != -1 ||
        vp8host_compose_frame(3, 2, &ok, 1, 0, 0, 0, &p1, one, one, one) != -1 || vp8host_compose_frame(2, 2, &ok, 1, 0, 0, 0, &low, one, one, one) != -1 ||
        vp8host_compose_frame(2, 2, many, VP8HIP_MAX_TILES + 1, 0, 0, 0, &p1, one, one, one) != -1 || vp8host_compose_frame(2, 2, &ok, 1, 0, 0, 0, &p1, nullptr, one, one) != -1 ||
        vp8host_compose_frame(2, 2, nullptr, 0, 7, 8, 9, nullptr, one, one, one) != 0 || one[0] != 9) {
        fprintf(stderr, "a refusal was not refused, or an empty canvas was\n");
        return 1;
    }
    printf("clean (%ld)\n", checked);
    return 0;
}
