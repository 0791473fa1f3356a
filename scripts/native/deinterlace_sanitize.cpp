// deinterlace_sanitize.cpp -- vp8host_deinterlace_frame and vp8host_y4m_interlace under the host sanitizers, at the sizes where tails
// and clamps bite: heights 4 and 6 (chroma of 2 and 3 rows: every tap clamped, an odd number of rows), width 2 (chroma 1 wide), an odd
// chroma width (50: 25), both parities, both modes, with and without a history; every plane in a heap block of exactly its size (a read
// or write past a plane's end is a heap overflow), the headers in blocks of exactly their length.  No GPU, no library: it is linked
// with vp8_host.cpp alone.
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include scripts/native/deinterlace_sanitize.cpp \
//       vp8oclenc_amd/csrc/vp8_host.cpp -o deinterlace_sanitize && ./deinterlace_sanitize
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "vp8hip_host.h"

int main() {
    const int sizes[][2] = {{2, 4}, {2, 6}, {16, 4}, {50, 36}, {50, 6}, {56, 40}, {64, 48}};
    unsigned seed = 1;
    auto next = [&] { seed = seed * 1664525u + 1013904223u; return (uint8_t)(seed >> 24); };
    long checked = 0;
    for (const auto &s : sizes)
        for (int mode = 0; mode <= 2; ++mode)
            for (int keep = 0; keep <= 1; ++keep) {
                const int w = s[0], h = s[1];
                const size_t nb[3] = {(size_t)w * h, (size_t)(w / 2) * (h / 2), (size_t)(w / 2) * (h / 2)};
                std::unique_ptr<uint8_t[]> src[3], hist[3], out[3];
                for (int k = 0; k < 3; ++k) {
                    src[k].reset(new uint8_t[nb[k]]);
                    hist[k].reset(new uint8_t[nb[k]]);
                    out[k].reset(new uint8_t[nb[k]]);
                    memset(hist[k].get(), 0, nb[k]);
                }
                for (int t = 0; t < 3; ++t) {      // frame 0 without a history, then two with one
                    for (int k = 0; k < 3; ++k)
                        for (size_t i = 0; i < nb[k]; ++i) src[k][i] = t == 2 && (i & 2) ? src[k][i] : next();      // (frame 2: half of it stands still)
                    int32_t woven = -1;
                    const bool with_hist = mode == 2;      // (mode 1 gets null history pointers: they must not be touched)
                    if (vp8host_deinterlace_frame(src[0].get(), src[1].get(), src[2].get(), with_hist ? hist[0].get() : nullptr,
                                                  with_hist ? hist[1].get() : nullptr, with_hist ? hist[2].get() : nullptr, out[0].get(), out[1].get(),
                                                  out[2].get(), w, h, mode, keep, t > 0, &woven) != 0) {
                        fprintf(stderr, "refused: %dx%d mode %d keep %d\n", w, h, mode, keep);
                        return 1;
                    }
                    if (woven < 0 || woven > w * h / 2 || (mode != 2 && woven) || (t == 0 && woven)) { fprintf(stderr, "woven %d: %dx%d mode %d\n", woven, w, h, mode); return 1; }
                    for (int k = 0; k < 3; ++k) {
                        if (with_hist && memcmp(hist[k].get(), src[k].get(), nb[k])) { fprintf(stderr, "the history is not the frame as received\n"); return 1; }
                        for (size_t i = 0; i < nb[k]; ++i) checked += out[k][i];
                    }
                    checked += woven;
                }
            }
    {   // what is refused is refused before anything is read
        uint8_t one[8] = {};
        int32_t woven = 0;
        const int bad[][4] = {{2, 2, 1, 0}, {3, 4, 1, 0}, {2, 5, 1, 0}, {2, 4, 3, 0}, {2, 4, 1, 2}, {0, 4, 1, 0}};
        for (const auto &b : bad)
            if (vp8host_deinterlace_frame(one, one, one, one, one, one, one, one, one, b[0], b[1], b[2], b[3], 0, &woven) != -1) { fprintf(stderr, "not refused\n"); return 1; }
        if (vp8host_deinterlace_frame(one, one, one, nullptr, nullptr, nullptr, one, one, one, 2, 4, 2, 0, 0, &woven) != -1) { fprintf(stderr, "not refused\n"); return 1; }
    }
    const char *heads[] = {"YUV4MPEG2 W34 H18 F25:1 Ip A1:1\n", "YUV4MPEG2 W34 H18 F25:1 It A1:1 C420jpeg\n", "YUV4MPEG2 Ib W2 H4 F1:1\n",
                           "YUV4MPEG2 W2 H4 F1:1 Im\n", "YUV4MPEG2 W2 H4 F1:1 I?\n", "YUV4MPEG2 W2 H4 F1:1 I\n", "YUV4MPEG2 W2 H4 F1:1 Itt\n", "YUV4MPEG2\n",
                           "YUV4MPEG2 I", "YUV4MPEG2 I\n", "YUV4MPEG", "", "YUV4MPEG2  It \n", "YUV4MPEG2 W2 H4 F1:1 XI=It\nFRAME\nIb "};
    for (const char *hd : heads) {
        const size_t n = strlen(hd);
        for (size_t cut = 0; cut <= n; ++cut) {      // every prefix, in a block of exactly its length
            std::unique_ptr<uint8_t[]> b(new uint8_t[cut ? cut : 1]);
            memcpy(b.get(), hd, cut);
            int32_t order = -1;
            const int rc = vp8host_y4m_interlace(b.get(), cut, &order);
            if (rc == 0 && (order < VP8HOST_FIELDS_PROGRESSIVE || order > VP8HOST_FIELDS_BOTTOM_FIRST)) { fprintf(stderr, "order %d from \"%s\"\n", order, hd); return 1; }
            if (rc != 0 && cut == n && n && hd[n - 1] == '\n' && !strstr(hd, " Im") && !strstr(hd, " I\n") && !strstr(hd, "Itt")) { fprintf(stderr, "refused \"%s\"\n", hd); return 1; }
            checked += rc;
        }
    }
    printf("clean (%ld)\n", checked);
    return 0;
}
