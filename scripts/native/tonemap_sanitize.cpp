// tonemap_sanitize.cpp -- vp8host_tonemap_tables and vp8host_tonemap_frame under the host sanitizers: both formats, both transfers and
// every colour matrix at the sizes of tests/test_tonemap_cpu.py, every plane and every table in a heap block of exactly its size (a read
// or write past an end is a heap overflow; a table index out of range is one too), with random ten-bit codes and with the extremes of
// all three samples.  No GPU, no library: it is linked with vp8_host.cpp alone.
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include scripts/native/tonemap_sanitize.cpp \
//       vp8oclenc_amd/csrc/vp8_host.cpp -o tonemap_sanitize && ./tonemap_sanitize
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "vp8hip_host.h"

int main() {
    const int sizes[][2] = {{2, 2}, {18, 10}, {34, 6}, {130, 66}};
    const int pairs[][2] = {{VP8HOST_TRANSFER_PQ, 400}, {VP8HOST_TRANSFER_PQ, 1000}, {VP8HOST_TRANSFER_PQ, 10000}, {VP8HOST_TRANSFER_HLG, 400},
                            {VP8HOST_TRANSFER_HLG, 1000}, {VP8HOST_TRANSFER_HLG, 10000}};
    unsigned seed = 1;
    auto next = [&] { seed = seed * 1664525u + 1013904223u; return (uint8_t)(seed >> 24); };
    long checked = 0;
    for (const auto &tp : pairs) {
        std::unique_ptr<uint32_t[]> lin(new uint32_t[4096]), gain(new uint32_t[4096]);
        std::unique_ptr<uint8_t[]> lo(new uint8_t[4096]), hi(new uint8_t[4096]);
        if (vp8host_tonemap_tables(tp[0], tp[1], lin.get(), gain.get(), lo.get(), hi.get()) != 0) { fprintf(stderr, "tables refused: %d %d\n", tp[0], tp[1]); return 1; }
        for (int i = 0; i < 4096; ++i) {
            if (lin[i] >= (1u << 20) || gain[i] >= (1u << 23) || (i && lin[i] < lin[i - 1])) { fprintf(stderr, "table entry %d of (%d, %d)\n", i, tp[0], tp[1]); return 1; }
            checked += lin[i] + gain[i] + lo[i] + hi[i];
        }
        for (int format = VP8HOST_FORMAT_P010; format <= VP8HOST_FORMAT_I010; ++format)
            for (const auto &s : sizes)
                for (int fill = 0; fill < 4; ++fill) {      // random bytes; all zero; all ones (code 1023); Y' at the top with chroma at the bottom
                    const int w = s[0], h = s[1], matrix = (fill + format) % VP8HOST_COLOUR_COUNT;
                    size_t nb[3];
                    if (vp8host_source_plane_bytes(format, w, h, nb) != 0) { fprintf(stderr, "plane bytes refused: format %d %dx%d\n", format, w, h); return 1; }
                    std::unique_ptr<uint8_t[]> p[3], o[3];
                    for (int k = 0; k < 3; ++k) {
                        p[k].reset(new uint8_t[nb[k] ? nb[k] : 1]);
                        for (size_t i = 0; i < nb[k]; ++i) p[k][i] = fill == 0 ? next() : (fill == 1 ? 0 : (fill == 2 || k == 0 ? 255 : 0));
                    }
                    const size_t ob[3] = {(size_t)w * h, (size_t)(w / 2) * (h / 2), (size_t)(w / 2) * (h / 2)};
                    for (int k = 0; k < 3; ++k) o[k].reset(new uint8_t[ob[k]]);
                    // (P010 gets a null third pointer: it must not be read)
                    if (vp8host_tonemap_frame(format, tp[0], tp[1], matrix, w, h, p[0].get(), p[1].get(), nb[2] ? p[2].get() : nullptr, o[0].get(), o[1].get(),
                                              o[2].get()) != 0) {
                        fprintf(stderr, "tone mapping refused: format %d (%d, %d) %dx%d\n", format, tp[0], tp[1], w, h);
                        return 1;
                    }
                    for (int k = 0; k < 3; ++k)
                        for (size_t i = 0; i < ob[k]; ++i) checked += o[k][i];
                }
    }
    // the refusals touch nothing
    uint8_t one[8] = {};
    if (vp8host_tonemap_tables(0, 1000, nullptr, nullptr, nullptr, nullptr) != -1 || vp8host_tonemap_tables(VP8HOST_TRANSFER_PQ, 399, nullptr, nullptr, nullptr, nullptr) != -1 ||
        vp8host_tonemap_frame(VP8HOST_FORMAT_I210, VP8HOST_TRANSFER_PQ, 1000, 0, 2, 2, one, one, one, one, one, one) != -1 ||
        vp8host_tonemap_frame(VP8HOST_FORMAT_P010, VP8HOST_TRANSFER_PQ, 1000, 4, 2, 2, one, one, one, one, one, one) != -1 ||
        vp8host_tonemap_frame(VP8HOST_FORMAT_P010, VP8HOST_TRANSFER_HLG, 10001, 0, 2, 2, one, one, one, one, one, one) != -1 ||
        vp8host_tonemap_frame(VP8HOST_FORMAT_P010, VP8HOST_TRANSFER_HLG, 1000, 0, 3, 2, one, one, one, one, one, one) != -1) {
        fprintf(stderr, "a refusal was not refused\n");
        return 1;
    }
    printf("clean (%ld)\n", checked);
    return 0;
}
