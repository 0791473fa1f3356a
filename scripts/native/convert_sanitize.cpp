// convert_sanitize.cpp -- vp8host_convert_frame and vp8host_y4m_colourspace under the host sanitizers: every format at the sizes of
// tests/test_source_format_cpu.py, every plane in a heap block of exactly vp8host_source_plane_bytes bytes (a read past a plane's end is
// a heap overflow), the headers in blocks of exactly their length.  No GPU, no library: it is linked with vp8_host.cpp alone.
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include scripts/native/convert_sanitize.cpp \
//       vp8oclenc_amd/csrc/vp8_host.cpp -o convert_sanitize && ./convert_sanitize
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "vp8hip_host.h"

int main() {
    const int sizes[][2] = {{2, 2}, {18, 10}, {34, 18}, {64, 48}};
    unsigned seed = 1;
    auto next = [&] { seed = seed * 1664525u + 1013904223u; return (uint8_t)(seed >> 24); };
    long checked = 0;
    for (int format = 0; format < VP8HOST_FORMAT_COUNT; ++format)
        for (const auto &s : sizes) {
            const int w = s[0], h = s[1];
            size_t nb[3];
            if (vp8host_source_plane_bytes(format, w, h, nb) != 0) { fprintf(stderr, "plane bytes refused: format %d %dx%d\n", format, w, h); return 1; }
            std::unique_ptr<uint8_t[]> p[3], o[3];
            for (int k = 0; k < 3; ++k) {
                p[k].reset(new uint8_t[nb[k] ? nb[k] : 1]);
                for (size_t i = 0; i < nb[k]; ++i) p[k][i] = next();
            }
            const size_t ob[3] = {(size_t)w * h, (size_t)(w / 2) * (h / 2), (size_t)(w / 2) * (h / 2)};
            for (int k = 0; k < 3; ++k) o[k].reset(new uint8_t[ob[k]]);
            // (the two-plane formats get a null third pointer: it must not be read)
            if (vp8host_convert_frame(format, w, h, p[0].get(), p[1].get(), nb[2] ? p[2].get() : nullptr, o[0].get(), o[1].get(), o[2].get()) != 0) {
                fprintf(stderr, "convert refused: format %d %dx%d\n", format, w, h);
                return 1;
            }
            for (int k = 0; k < 3; ++k)
                for (size_t i = 0; i < ob[k]; ++i) checked += o[k][i];
        }
    const char *heads[] = {"YUV4MPEG2 W34 H18 F25:1 Ip A1:1\n", "YUV4MPEG2 W34 H18 F25:1 C420jpeg XYSCSS=420JPEG\n", "YUV4MPEG2 C422 W2 H2 F1:1\n",
                           "YUV4MPEG2 W2 H2 F1:1 C444p10\n", "YUV4MPEG2 W2 H2 F1:1 Cmono\n", "YUV4MPEG2 W2 H2 F1:1 C420p12\n", "YUV4MPEG2\n", "YUV4MPEG2 C",
                           "YUV4MPEG2 C\n", "YUV4MPEG", "", "YUV4MPEG2  C444 \n", "YUV4MPEG2 W2 H2 F1:1 C444alpha\nFRAME\n"};
    for (const char *hd : heads) {
        const size_t n = strlen(hd);
        for (size_t cut = 0; cut <= n; ++cut) {      // every prefix, in a block of exactly its length
            std::unique_ptr<uint8_t[]> b(new uint8_t[cut ? cut : 1]);
            memcpy(b.get(), hd, cut);
            int32_t format = -1;
            const int rc = vp8host_y4m_colourspace(b.get(), cut, &format);
            if (rc == 0 && (format < 0 || format >= VP8HOST_FORMAT_COUNT)) { fprintf(stderr, "format %d from \"%s\"\n", format, hd); return 1; }
            checked += rc;
        }
    }
    printf("clean (%ld)\n", checked);
    return 0;
}
