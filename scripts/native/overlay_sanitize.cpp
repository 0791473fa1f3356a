// overlay_sanitize.cpp -- vp8host_overlay_frame under the host sanitizers: both formats and every colour matrix at the pictures, layers
// and positions of tests/test_overlay_cpu.py, the layer and every plane in a heap block of exactly its size (a read or write past an
// end is a heap overflow), tight and pitched layers -- the last row of a pitched layer ends with its last pixel, so a read of the bytes
// between the rows runs off the block -- at negative and overhanging positions, and the extremes of every operand (the sums of the
// rule must stay inside int32).  No GPU, no library: it is linked with vp8_host.cpp alone.
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include scripts/native/overlay_sanitize.cpp \
//       vp8oclenc_amd/csrc/vp8_host.cpp -o overlay_sanitize && ./overlay_sanitize
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "vp8hip_host.h"

int main() {
    const int pictures[][2] = {{40, 26}, {34, 18}, {2, 2}};
    const int layers[][2] = {{1, 1}, {5, 3}, {16, 16}, {37, 21}, {64, 40}};
    const int opacities[] = {0, 1, 128, 254, 255};
    unsigned seed = 1;
    auto next = [&] { seed = seed * 1664525u + 1013904223u; return (uint8_t)(seed >> 24); };
    long checked = 0;
    int n = 0;
    for (const auto &pic : pictures)
        for (const auto &l : layers)
            for (int extra = 0; extra < 2; ++extra)
                for (int fill = 0; fill < 3; ++fill) {      // random bytes; all zero; all ones
                    const int pw = pic[0], ph = pic[1], lw = l[0], lh = l[1], pitch = 4 * lw + 12 * extra;
                    const int pos[][2] = {{0, 0}, {1, 1}, {3, 2}, {-3, -2}, {pw - 5, ph - 3}, {pw - 1, ph - 1}, {pw, 0}, {-lw, -lh}, {-lw + 1, ph - 1}, {-16384, 16384}, {16384, -16384}};
                    const size_t nb = (size_t)pitch * (lh - 1) + (size_t)4 * lw;      // exactly: nothing behind the last pixel
                    std::unique_ptr<uint8_t[]> px(new uint8_t[nb]);
                    for (size_t i = 0; i < nb; ++i) px[i] = fill == 0 ? next() : (fill == 1 ? 0 : 255);
                    for (const auto &p : pos) {
                        const size_t ob[3] = {(size_t)pw * ph, (size_t)(pw / 2) * (ph / 2), (size_t)(pw / 2) * (ph / 2)};
                        std::unique_ptr<uint8_t[]> o[3];
                        for (int k = 0; k < 3; ++k) {
                            o[k].reset(new uint8_t[ob[k]]);
                            for (size_t i = 0; i < ob[k]; ++i) o[k][i] = fill == 0 ? next() : (fill == 1 ? 255 : 0);
                        }
                        const int format = (n & 1) ? VP8HOST_FORMAT_RGBA : VP8HOST_FORMAT_BGRA, matrix = (n >> 1) % VP8HOST_COLOUR_COUNT, opacity = opacities[n % 5];
                        ++n;
                        if (vp8host_overlay_frame(format, matrix, lw, lh, pitch, px.get(), p[0], p[1], opacity, pw, ph, o[0].get(), o[1].get(), o[2].get()) != 0) {
                            fprintf(stderr, "refused: %dx%d at (%d, %d) on %dx%d\n", lw, lh, p[0], p[1], pw, ph);
                            return 1;
                        }
                        for (int k = 0; k < 3; ++k)
                            for (size_t i = 0; i < ob[k]; ++i) checked += o[k][i];
                    }
                }
    // the refusals touch nothing: one byte stands for every buffer
    uint8_t one[4] = {};
    if (vp8host_overlay_frame(VP8HOST_FORMAT_YUY2, 0, 1, 1, 4, one, 0, 0, 255, 2, 2, one, one, one) != -1 ||
        vp8host_overlay_frame(VP8HOST_FORMAT_BGRA, 4, 1, 1, 4, one, 0, 0, 255, 2, 2, one, one, one) != -1 ||
        vp8host_overlay_frame(VP8HOST_FORMAT_BGRA, 0, 16385, 1, 4 * 16385, one, 0, 0, 255, 2, 2, one, one, one) != -1 ||
        vp8host_overlay_frame(VP8HOST_FORMAT_BGRA, 0, 2, 1, 7, one, 0, 0, 255, 2, 2, one, one, one) != -1 ||
        vp8host_overlay_frame(VP8HOST_FORMAT_BGRA, 0, 1, 1, 4, one, 16385, 0, 255, 2, 2, one, one, one) != -1 ||
        vp8host_overlay_frame(VP8HOST_FORMAT_BGRA, 0, 1, 1, 4, one, 0, 0, 256, 2, 2, one, one, one) != -1 ||
        vp8host_overlay_frame(VP8HOST_FORMAT_BGRA, 0, 1, 1, 4, one, 0, 0, 255, 3, 2, one, one, one) != -1 ||
        vp8host_overlay_frame(VP8HOST_FORMAT_BGRA, 0, 1, 1, 4, nullptr, 0, 0, 255, 2, 2, one, one, one) != -1) {
        fprintf(stderr, "a refusal was not refused\n");
        return 1;
    }
    printf("clean (%ld)\n", checked);
    return 0;
}
