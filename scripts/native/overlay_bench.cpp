// overlay_bench.cpp -- what k_overlay_b and k_overlay_prepare cost, next to a device-to-device copy that moves the same bytes.  A
// context of WxH (default 1920x1080) takes N frames in from device memory: first plain (the pack launch alone), then with each of three
// layers of random BGRA with random alpha -- a 256x128 logo, a W x 200 subtitle band, a full-frame layer -- N frames each (k_overlay_b
// behind the pack), then N moves of the layer by one pixel with a frame behind each (k_overlay_prepare in front of k_overlay_b), then N
// hipMemcpyAsync of HALF the bytes each of the two launches reads plus writes (a copy reads and writes every byte it moves).
// Bytes, with B the layer's pixels inside the picture: k_overlay_b reads and writes the frame under the layer (2 x 1.5 B) and reads the
// prepared planes (2 B of Yo and e, 2.5 B of E, T_u, T_v): 5.5 B; k_overlay_prepare reads the pixels (4 B) and writes the planes (4.5 B).
// Each leg is timed with a pair of HIP events around its N frames (launch gaps included); the kernels' own times come from a kernel
// trace of the run, in which the legs appear in this order:
//   hipcc -O2 -std=c++17 -I include scripts/native/overlay_bench.cpp -o overlay_bench -L vp8oclenc_amd -lvp8hip -Wl,-rpath,$PWD/vp8oclenc_amd
//   rocprofv3 --kernel-trace --memory-copy-trace --stats -d out -- ./overlay_bench [W H N]
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <vector>

#include "vp8hip.h"
#include "vp8hip_host.h"

#define CK(x) do { int rc_ = (x); if (rc_ != 0) { fprintf(stderr, "%s -> %d\n", #x, rc_); return 1; } } while (0)

int main(int argc, char **argv) {
    const int W = argc > 1 ? atoi(argv[1]) : 1920, H = argc > 2 ? atoi(argv[2]) : 1080, N = argc > 3 ? atoi(argv[3]) : 20;
    if (W % 2 || H % 2 || W < 256 || H < 200 || N < 1) { fprintf(stderr, "W and H even, at least 256x200\n"); return 2; }
    const int Wc = (W + 15) / 16 * 16, Hc = (H + 15) / 16 * 16;
    const size_t frame = (size_t)W * H * 3 / 2, layer_bytes = (size_t)W * H * 4;
    uint8_t *src = nullptr, *dst = nullptr, *layer = nullptr;
    CK(hipMalloc(&src, layer_bytes * 2));
    CK(hipMalloc(&dst, layer_bytes * 2));
    CK(hipMalloc(&layer, layer_bytes));
    {
        std::vector<uint8_t> h(layer_bytes);
        unsigned seed = 1;
        for (auto &b : h) { seed = seed * 1664525u + 1013904223u; b = (uint8_t)(seed >> 24); }
        CK(hipMemcpy(src, h.data(), layer_bytes, hipMemcpyHostToDevice));
        for (auto &b : h) { seed = seed * 1664525u + 1013904223u; b = (uint8_t)(seed >> 24); }
        CK(hipMemcpy(layer, h.data(), layer_bytes, hipMemcpyHostToDevice));
    }
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    vp8hip_ctx *c = nullptr;
    CK(vp8hip_create(&c, Wc, Hc, -1.0f, 0));
    if (Wc != W || Hc != H) CK(vp8hip_set_source_size(c, W, H));
    const uint8_t *y = src, *u = src + (size_t)W * H, *v = u + (size_t)(W / 2) * (H / 2);
    // move: 0 = the layer stands still; 1 = it moves by a pixel in front of every frame (a prepare launch per frame)
    auto leg = [&](const char *name, int x, int yy, int move) -> int {
        CK(vp8hip_set_current_device(c, y, u, v));      // (buffers grown, code loaded, planes prepared)
        CK(vp8hip_synchronize(c));
        CK(hipEventRecord(e0, nullptr));
        for (int i = 0; i < N; ++i) {
            if (move) CK(vp8hip_set_overlay_placement(c, 0, x + (i & 1), yy + ((i >> 1) & 1), 255 - (i & 3)));
            CK(vp8hip_set_current_device(c, y, u, v));
        }
        CK(vp8hip_synchronize(c));
        CK(hipEventRecord(e1, nullptr));
        CK(hipEventSynchronize(e1));
        float ms = 0;
        CK(hipEventElapsedTime(&ms, e0, e1));
        printf("%-44s %8.1f us per frame\n", name, ms * 1000.0f / N);
        return 0;
    };
    if (leg("pack alone", 0, 0, 0)) return 1;
    const struct { const char *name; int lw, lh, x, y; } layers[3] = {{"logo 256x128", 256, 128, W - 256 - 64, 64}, {"subtitle band Wx200", W, 200, 0, H - 200 - 20}, {"full frame", W, H, 0, 0}};
    for (const auto &l : layers) {
        CK(vp8hip_set_overlay_device(c, 0, VP8HOST_FORMAT_BGRA, 0, layer, l.lw, l.lh, 4 * l.lw, l.x, l.y, 255));
        char name[96];
        snprintf(name, sizeof name, "%s: pack + overlay", l.name);
        if (leg(name, l.x, l.y, 0)) return 1;
        snprintf(name, sizeof name, "%s: pack + prepare + overlay", l.name);
        if (leg(name, l.x, l.y, 1)) return 1;
    }
    CK(vp8hip_clear_overlay(c, -1));
    vp8hip_destroy(c);
    for (const auto &l : layers)
        for (int k = 0; k < 2; ++k) {      // the copies that move what k_overlay_b (5.5 B) and k_overlay_prepare (8.5 B) move
            const size_t B = (size_t)l.lw * l.lh, moved = k ? B * 17 / 2 : B * 11 / 2, n = moved / 2;
            CK(hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToDevice, nullptr));
            CK(hipDeviceSynchronize());
            CK(hipEventRecord(e0, nullptr));
            for (int i = 0; i < N; ++i) CK(hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToDevice, nullptr));
            CK(hipEventRecord(e1, nullptr));
            CK(hipEventSynchronize(e1));
            float ms = 0;
            CK(hipEventElapsedTime(&ms, e0, e1));
            printf("%-44s %8.1f us per copy (%zu bytes copied, %zu moved)\n", k ? "  copy beside the prepare launch" : "  copy beside the overlay launch", ms * 1000.0f / N, n, moved);
        }
    (void)frame;
    (void)hipFree(src);
    (void)hipFree(dst);
    (void)hipFree(layer);
    return 0;
}
