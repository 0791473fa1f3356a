// analysis_sanitize.cpp -- vp8host_analyse_luma and the quantizer-ladder path of vp8drv_set_quantizer under the host sanitizers: the
// sizes of tests/test_analysis_cpu.py, every plane in a heap block of exactly width x height bytes (a read past a plane's end is a heap
// overflow), the widest sums there are (samples 0 and 255), with and without a previous plane, and every quantizer pair 0..127 x
// 0..127 through vp8host_quantizer_ladders and vp8host_prepare_segments_data as the driver feeds them.  No GPU, no library: it is
// linked with vp8_host.cpp alone.
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include scripts/native/analysis_sanitize.cpp \
//       vp8oclenc_amd/csrc/vp8_host.cpp -o analysis_sanitize && ./analysis_sanitize
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "vp8hip_host.h"

int main() {
    const int sizes[][2] = {{16, 16}, {48, 32}, {176, 144}, {1920, 1088}};
    unsigned seed = 1;
    auto next = [&] { seed = seed * 1664525u + 1013904223u; return (uint8_t)(seed >> 24); };
    unsigned long long checked = 0;
    for (const auto &s : sizes) {
        const int w = s[0], h = s[1];
        const size_t n = (size_t)w * h;
        for (int kind = 0; kind < 3; ++kind) {      // random, extremes (0 / 255), cur == prev
            std::unique_ptr<uint8_t[]> cur(new uint8_t[n]), prev(new uint8_t[n]);
            for (size_t i = 0; i < n; ++i) {
                cur[i] = kind == 1 ? (uint8_t)(next() & 1 ? 255 : 0) : next();
                prev[i] = kind == 1 ? (uint8_t)(255 - cur[i]) : (kind == 2 ? cur[i] : next());
            }
            vp8host_luma_analysis a, b;
            if (vp8host_analyse_luma(cur.get(), prev.get(), w, h, &a) != 0 || vp8host_analyse_luma(cur.get(), nullptr, w, h, &b) != 0) {
                fprintf(stderr, "refused: %dx%d\n", w, h);
                return 1;
            }
            if (a.spatial != b.spatial || !a.have_prev || b.have_prev || b.temporal_sse || b.temporal_sad || b.static_mbs) { fprintf(stderr, "no-history record wrong: %dx%d\n", w, h); return 1; }
            if (kind == 1 && a.temporal_sse != 65025ull * n) { fprintf(stderr, "sse %llu at %dx%d\n", (unsigned long long)a.temporal_sse, w, h); return 1; }
            if (kind == 2 && (a.temporal_sad || a.static_mbs != (w / 16) * (h / 16))) { fprintf(stderr, "static count wrong: %dx%d\n", w, h); return 1; }
            checked += a.spatial + a.temporal_sse + a.temporal_sad + (unsigned long long)a.static_mbs;
        }
    }
    {   // refusals touch nothing
        uint8_t one[1] = {0};
        vp8host_luma_analysis a;
        if (vp8host_analyse_luma(one, nullptr, 24, 16, &a) != -1 || vp8host_analyse_luma(nullptr, nullptr, 16, 16, &a) != -1 ||
            vp8host_analyse_luma(one, nullptr, 16, 16, nullptr) != -1 || vp8host_analyse_luma(one, one, 0, 0, &a) != -1) {
            fprintf(stderr, "a bad argument was accepted\n");
            return 1;
        }
    }
    for (int qmin = 0; qmin < 128; ++qmin)
        for (int qmax = 0; qmax < 128; ++qmax) {      // what vp8drv_set_quantizer does with a pair, then what a frame does with the ladders
            int32_t lastqi[4], altrefqi[4], sd[44];
            vp8host_quantizer_ladders(qmin, qmax, lastqi, altrefqi);
            const int lo = qmin < qmax ? qmin : qmax, hi = qmin < qmax ? qmax : qmin;
            for (int k = 0; k < 4; ++k)
                if (lastqi[k] < lo || lastqi[k] > hi || altrefqi[k] < 0 || altrefqi[k] > hi) { fprintf(stderr, "ladder out of range: %d %d\n", qmin, qmax); return 1; }
            vp8host_prepare_segments_data(0, lastqi, lo, 4, 3, 0, 0, sd);
            vp8host_prepare_segments_data(0, altrefqi, lo, 4, 3, 1, 7, sd);
            vp8host_prepare_segments_data(1, altrefqi, lo, 1, 0, 0, 0, sd);
            for (int k = 0; k < 44; ++k) checked += (unsigned)sd[k];
        }
    printf("clean (%llu)\n", checked);
    return 0;
}
