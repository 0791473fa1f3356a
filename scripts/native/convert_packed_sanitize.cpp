// convert_packed_sanitize.cpp -- vp8host_convert_frame_colour, vp8host_convert_frame and vp8host_colour_coefficients on the packed formats
// (YUY2, UYVY, BGRA, RGBA) under the host sanitizers: every format and every matrix at the sizes of tests/test_packed_format_cpu.py, the
// plane in a heap block of exactly vp8host_source_plane_bytes bytes (a read past its end is a heap overflow), the second and third
// pointers null (they must not be read), the outputs in blocks of exactly their size.  No GPU, no library: linked with vp8_host.cpp alone.
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include scripts/native/convert_packed_sanitize.cpp \
//       vp8oclenc_amd/csrc/vp8_host.cpp -o convert_packed_sanitize && ./convert_packed_sanitize
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "vp8hip_host.h"

int main() {
    const int sizes[][2] = {{34, 18}, {16, 16}, {10, 6}, {2, 2}, {200, 120}};
    unsigned seed = 1;
    auto next = [&] { seed = seed * 1664525u + 1013904223u; return (uint8_t)(seed >> 24); };
    long checked = 0;
    for (int format = VP8HOST_FORMAT_PACKED_FIRST; format < VP8HOST_FORMAT_PACKED_END; ++format)
        for (const auto &s : sizes)
            for (int fill = 0; fill < 3; ++fill) {      // random, all 255, all 0
                const int w = s[0], h = s[1];
                size_t nb[3];
                if (vp8host_source_plane_bytes(format, w, h, nb) != 0 || nb[1] || nb[2]) { fprintf(stderr, "plane bytes: format %d %dx%d\n", format, w, h); return 1; }
                std::unique_ptr<uint8_t[]> p(new uint8_t[nb[0]]), o[3], q[3];
                for (size_t i = 0; i < nb[0]; ++i) p[i] = fill == 0 ? next() : fill == 1 ? 255 : 0;
                const size_t ob[3] = {(size_t)w * h, (size_t)(w / 2) * (h / 2), (size_t)(w / 2) * (h / 2)};
                for (int k = 0; k < 3; ++k) { o[k].reset(new uint8_t[ob[k]]); q[k].reset(new uint8_t[ob[k]]); }
                for (int m = 0; m < VP8HOST_COLOUR_COUNT; ++m) {
                    if (vp8host_convert_frame_colour(format, m, w, h, p.get(), nullptr, nullptr, o[0].get(), o[1].get(), o[2].get()) != 0) {
                        fprintf(stderr, "convert refused: format %d matrix %d %dx%d\n", format, m, w, h);
                        return 1;
                    }
                    for (int k = 0; k < 3; ++k)
                        for (size_t i = 0; i < ob[k]; ++i) checked += o[k][i];
                    if (m == 0) {      // the form without a matrix is matrix 0
                        if (vp8host_convert_frame(format, w, h, p.get(), nullptr, nullptr, q[0].get(), q[1].get(), q[2].get()) != 0) return 1;
                        for (int k = 0; k < 3; ++k)
                            if (memcmp(o[k].get(), q[k].get(), ob[k])) { fprintf(stderr, "matrix 0 differs: format %d %dx%d plane %d\n", format, w, h, k); return 1; }
                    }
                }
            }
    uint8_t one[16] = {}, out[3][4];
    for (int format = VP8HOST_FORMAT_COUNT; format <= VP8HOST_FORMAT_PACKED_END; ++format) {
        const bool packed = format >= VP8HOST_FORMAT_PACKED_FIRST && format < VP8HOST_FORMAT_PACKED_END;
        if ((vp8host_convert_frame(format, 2, 2, one, one, one, out[0], out[1], out[2]) == 0) != packed) { fprintf(stderr, "format %d\n", format); return 1; }
    }
    for (int m = -1; m <= VP8HOST_COLOUR_COUNT; ++m) {
        int32_t c[9], off = -1;
        const bool known = m >= 0 && m < VP8HOST_COLOUR_COUNT;
        if ((vp8host_colour_coefficients(m, c, &off) == 0) != known) { fprintf(stderr, "matrix %d\n", m); return 1; }
        if ((vp8host_convert_frame_colour(VP8HOST_FORMAT_BGRA, m, 2, 2, one, nullptr, nullptr, out[0], out[1], out[2]) == 0) != known) return 1;
        if (known) checked += off + c[0] + c[8];
    }
    printf("clean (%ld)\n", checked);
    return 0;
}
