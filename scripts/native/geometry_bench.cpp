// geometry_bench.cpp -- what k_window_b and k_orient_b cost, next to a device-to-device copy of the same bytes.  A context of
// WxH (default 3840x2160; 1080p is too close to the launch floor) takes N frames in from device memory: first plain (the pack
// launch alone), then through a window (an NV12 surface of pitch P, default 4096: k_window_b and k_convert_b in front of the pack),
// then at each of the eight orientations (k_orient_b in front of the pack), then N hipMemcpyAsync of one frame's 1.5 W H bytes.
// Each leg is timed with a pair of HIP events around its N frames (launch gaps included); the kernels' own times come from a
// kernel trace of the run, in which the legs appear in this order:
//   hipcc -O2 -std=c++17 -I include scripts/native/geometry_bench.cpp -o geometry_bench -L vp8oclenc_amd -lvp8hip -Wl,-rpath,$PWD/vp8oclenc_amd
//   rocprofv3 --kernel-trace --memory-copy-trace --stats -d out -- ./geometry_bench [W H N P]
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <vector>

#include "vp8hip.h"
#include "vp8hip_host.h"

#define CK(x) do { int rc_ = (x); if (rc_ != 0) { fprintf(stderr, "%s -> %d\n", #x, rc_); return 1; } } while (0)

int main(int argc, char **argv) {
    const int W = argc > 1 ? atoi(argv[1]) : 3840, H = argc > 2 ? atoi(argv[2]) : 2160, N = argc > 3 ? atoi(argv[3]) : 20, P = argc > 4 ? atoi(argv[4]) : 4096;
    if (W % 16 || H % 16 || P < W || N < 1) { fprintf(stderr, "W and H whole macroblocks, P >= W\n"); return 2; }
    const size_t frame = (size_t)W * H * 3 / 2, surface = (size_t)P * H * 3 / 2;
    uint8_t *src = nullptr, *dst = nullptr;
    CK(hipMalloc(&src, surface));
    CK(hipMalloc(&dst, frame));
    {
        std::vector<uint8_t> h(surface);
        unsigned seed = 1;
        for (auto &b : h) { seed = seed * 1664525u + 1013904223u; b = (uint8_t)(seed >> 24); }
        CK(hipMemcpy(src, h.data(), surface, hipMemcpyHostToDevice));
    }
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    auto leg = [&](const char *name, vp8hip_ctx *c, const uint8_t *y, const uint8_t *u, const uint8_t *v) -> int {
        CK(vp8hip_set_current_device(c, y, u, v));      // (buffers grown, code loaded)
        CK(vp8hip_synchronize(c));
        CK(hipEventRecord(e0, nullptr));
        for (int i = 0; i < N; ++i) CK(vp8hip_set_current_device(c, y, u, v));
        CK(vp8hip_synchronize(c));
        CK(hipEventRecord(e1, nullptr));
        CK(hipEventSynchronize(e1));
        float ms = 0;
        CK(hipEventElapsedTime(&ms, e0, e1));
        printf("%-28s %8.1f us per frame\n", name, ms * 1000.0f / N);
        return 0;
    };
    vp8hip_ctx *c = nullptr;
    CK(vp8hip_create(&c, W, H, -1.0f, 0));
    const uint8_t *y = src, *u = src + (size_t)W * H, *v = u + (size_t)(W / 2) * (H / 2);
    if (leg("pack alone", c, y, u, v)) return 1;
    {
        const int32_t pitch[3] = {P, P, 0};
        CK(vp8hip_set_source_format(c, VP8HOST_FORMAT_NV12));
        CK(vp8hip_set_source_window(c, pitch, 0, 0));
        if (leg("window (NV12) + convert", c, src, src + (size_t)P * H, src + (size_t)P * H)) return 1;
        CK(vp8hip_set_source_window(c, nullptr, 0, 0));
        if (leg("convert (NV12)", c, src, src + (size_t)W * H, src + (size_t)W * H)) return 1;
        CK(vp8hip_set_source_format(c, VP8HOST_FORMAT_I420));
    }
    for (int turns = 0; turns < 4; ++turns)
        for (int mirror = 0; mirror < 2; ++mirror) {
            if (!turns && !mirror) continue;
            // (the upright frame stays WxH: under an odd number of turns the planes that come in are H wide and W high -- the same bytes)
            CK(vp8hip_set_source_orientation(c, turns, mirror));
            char name[64];
            snprintf(name, sizeof name, "orient turns %d mirror %d", turns, mirror);
            if (leg(name, c, y, u, v)) return 1;
        }
    CK(vp8hip_set_source_orientation(c, 0, 0));
    vp8hip_destroy(c);
    CK(hipMemcpyAsync(dst, src, frame, hipMemcpyDeviceToDevice, nullptr));
    CK(hipDeviceSynchronize());
    CK(hipEventRecord(e0, nullptr));
    for (int i = 0; i < N; ++i) CK(hipMemcpyAsync(dst, src, frame, hipMemcpyDeviceToDevice, nullptr));
    CK(hipEventRecord(e1, nullptr));
    CK(hipEventSynchronize(e1));
    float ms = 0;
    CK(hipEventElapsedTime(&ms, e0, e1));
    printf("%-28s %8.1f us per frame (%zu bytes)\n", "hipMemcpyAsync device-device", ms * 1000.0f / N, frame);
    (void)hipFree(src);
    (void)hipFree(dst);
    return 0;
}
