// geometry_sanitize.cpp -- vp8host_source_window, vp8host_window_frame and vp8host_orient_frame under the host sanitizers.  A surface
// is a heap block that starts at the window's FIRST byte and ends with its LAST one (the plane base handed to the function lies in
// front of the block): a read of any byte in front of the window or behind it is a heap overflow, and so is a write past a tight
// plane of exactly its size.  All twelve formats, two sizes, three origins, three pitches; all eight orientations on planes with odd
// chroma width and odd chroma height; every refusal.  No GPU, no library: it is linked with vp8_host.cpp alone.
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include scripts/native/geometry_sanitize.cpp \
//       vp8oclenc_amd/csrc/vp8_host.cpp -o geometry_sanitize && ./geometry_sanitize
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "vp8hip_host.h"

int main() {
    unsigned seed = 1;
    auto next = [&] { seed = seed * 1664525u + 1013904223u; return (uint8_t)(seed >> 24); };
    const int formats[] = {0, 1, 2, 3, 4, 5, 6, 7, 16, 17, 18, 19};
    const int sizes[][2] = {{48, 32}, {50, 36}}, origins[][2] = {{0, 0}, {2, 6}, {14, 2}}, extra[] = {0, 3, 64};
    long checked = 0;
    for (int format : formats)
        for (const auto &sz : sizes)
            for (const auto &o : origins)
                for (int e : extra) {
                    const int w = sz[0], h = sz[1], x = o[0], y = o[1], sw = 80;      // a surface 80 samples wide
                    int32_t huge[3] = {1 << 20, 1 << 20, 1 << 20}, pitch[3], rb[3], rows[3];
                    size_t off[3], nb[3];
                    if (vp8host_source_window(format, sw, h, 0, 0, huge, off, rb, rows) != 0) { fprintf(stderr, "refused: format %d\n", format); return 1; }
                    for (int p = 0; p < 3; ++p) pitch[p] = rows[p] ? rb[p] + e : 0;      // (the surface's tight pitch, plus)
                    if (vp8host_source_window(format, w, h, x, y, pitch, off, rb, rows) != 0 || vp8host_source_plane_bytes(format, w, h, nb) != 0) {
                        fprintf(stderr, "refused: format %d %dx%d at (%d, %d)\n", format, w, h, x, y);
                        return 1;
                    }
                    std::unique_ptr<uint8_t[]> s[3], d[3];
                    const uint8_t *base[3] = {nullptr, nullptr, nullptr};
                    for (int p = 0; p < 3; ++p) {
                        if ((size_t)rows[p] * (size_t)rb[p] != nb[p]) { fprintf(stderr, "rows * row_bytes: format %d plane %d\n", format, p); return 1; }
                        if (!rows[p]) continue;
                        const size_t span = (size_t)(rows[p] - 1) * pitch[p] + rb[p];
                        s[p].reset(new uint8_t[span]);
                        d[p].reset(new uint8_t[nb[p]]);
                        for (size_t i = 0; i < span; ++i) s[p][i] = next();
                        base[p] = s[p].get() - off[p];
                    }
                    if (vp8host_window_frame(format, w, h, x, y, pitch, base[0], base[1], base[2], d[0].get(), d[1].get(), d[2].get()) != 0) {
                        fprintf(stderr, "window_frame refused: format %d\n", format);
                        return 1;
                    }
                    for (int p = 0; p < 3; ++p)
                        for (int r = 0; r < rows[p]; ++r)
                            if (memcmp(d[p].get() + (size_t)r * rb[p], s[p].get() + (size_t)r * pitch[p], rb[p])) { fprintf(stderr, "row %d of plane %d differs\n", r, p); return 1; }
                    checked += rows[0];
                }
    {   // the refusals
        int32_t pitch[3] = {80, 40, 40}, rb[3], rows[3];
        size_t off[3];
        const int bad[][5] = {{0, 48, 32, -2, 0}, {0, 48, 32, 0, -2}, {0, 48, 32, 1, 0}, {0, 48, 32, 0, 3}, {0, 48, 32, 34, 0}, {0, 47, 32, 0, 0}, {0, 48, 0, 0, 0}, {9, 48, 32, 0, 0},
                                {1, 48, 32, 0, 0} /* NV12 chroma rows are 48 bytes: pitch 40 */, {18, 48, 32, 0, 0} /* BGRA: 192 bytes */};
        for (const auto &b : bad)
            if (vp8host_source_window(b[0], b[1], b[2], b[3], b[4], pitch, off, rb, rows) == 0) { fprintf(stderr, "not refused: %d %d %d %d %d\n", b[0], b[1], b[2], b[3], b[4]); return 1; }
        if (vp8host_source_window(0, 48, 32, 32, 0, pitch, off, rb, rows) != 0) { fprintf(stderr, "a window that ends with the pitch was refused\n"); return 1; }
        if (vp8host_source_window(0, 48, 32, 0, 0, nullptr, off, rb, rows) == 0) { fprintf(stderr, "a null pitch was not refused\n"); return 1; }
    }
    const int osizes[][2] = {{50, 36}, {36, 70}, {2, 2}, {16, 16}};      // chroma 25 wide; chroma 35 high
    for (const auto &sz : osizes)
        for (int turns = 0; turns < 4; ++turns)
            for (int mirror = 0; mirror < 2; ++mirror) {
                const int w = sz[0], h = sz[1];
                const size_t nb[3] = {(size_t)w * h, (size_t)(w / 2) * (h / 2), (size_t)(w / 2) * (h / 2)};
                std::unique_ptr<uint8_t[]> s[3], d[3], back[3];
                for (int p = 0; p < 3; ++p) {
                    s[p].reset(new uint8_t[nb[p]]); d[p].reset(new uint8_t[nb[p]]); back[p].reset(new uint8_t[nb[p]]);
                    for (size_t i = 0; i < nb[p]; ++i) s[p][i] = next();
                }
                if (vp8host_orient_frame(turns, mirror, w, h, s[0].get(), s[1].get(), s[2].get(), d[0].get(), d[1].get(), d[2].get()) != 0) { fprintf(stderr, "orient refused\n"); return 1; }
                // undone: without a mirror by the remaining turns; with one, the same orientation again (a mirrored turn is an involution)
                const int ow = turns & 1 ? h : w, oh = turns & 1 ? w : h;
                if (vp8host_orient_frame(mirror ? turns : (4 - turns) & 3, mirror, ow, oh, d[0].get(), d[1].get(), d[2].get(), back[0].get(), back[1].get(), back[2].get()) != 0) {
                    fprintf(stderr, "orient back refused\n");
                    return 1;
                }
                for (int p = 0; p < 3; ++p)
                    if (memcmp(back[p].get(), s[p].get(), nb[p])) { fprintf(stderr, "turns %d mirror %d and back is not the identity (plane %d)\n", turns, mirror, p); return 1; }
                checked += d[0][0];
            }
    if (vp8host_orient_frame(4, 0, 16, 16, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == 0 || vp8host_orient_frame(0, 2, 16, 16, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == 0) {
        fprintf(stderr, "orient: out of range not refused\n");
        return 1;
    }
    printf("clean (%ld)\n", checked);
    return 0;
}
