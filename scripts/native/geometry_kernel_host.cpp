// geometry_kernel_host.cpp -- the kernel bodies of vp8oclenc_amd/csrc/kernels_geometry.hip (k_window_b, k_orient_b), the file as it
// stands, compiled for the HOST and held to vp8host_window_frame / vp8host_orient_frame under the address and undefined-behaviour
// sanitizers.  No GPU, no library.  A workgroup is 256 OS threads that meet at the barrier of the transposing tile (__syncthreads);
// LDS is a static array, v_perm_b32 is plain C++; workgroups run one after the other.  Every surface window, plane and staging buffer
// sits in a heap block of exactly its size at an ODD address offset: a lane that reads a byte outside the window or writes past a
// plane is a heap overflow, and no access is aligned by luck.  A surface is allocated from the window's first byte to its last byte,
// so what lies between the rows is inside the block but nothing in front of the window or behind it is.
// Checked: the window for all twelve formats, 48x32 and 50x36 at origins (0, 0), (2, 6), (14, 2) with pitches tight + 0, 3, 64, two
// batch members; all eight orientations at 16x16, 48x32, 50x36, 200x70, 128x96, 2x2, 2x130, 130x2 and 258x66.
//   clang++ -std=c++20 -O1 -g -pthread -fsanitize=address,undefined -fno-sanitize=alignment -fno-sanitize-recover=all \
//       -I scripts/native/host_stub -I include scripts/native/geometry_kernel_host.cpp vp8oclenc_amd/csrc/vp8_host.cpp \
//       -o geometry_kernel_host && ./geometry_kernel_host
// (-fno-sanitize=alignment: the kernels' 4- and 16-byte accesses are unaligned vector accesses on the device.)
#include <stdint.h>
#include <stddef.h>
#include <string.h>
#include <barrier>
#include <functional>
#include <thread>
#include <vector>
struct dim3 { unsigned x, y, z; dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {} };
typedef void *hipStream_t; typedef void *hipEvent_t;
#define __global__
#define __device__
#define __host__
#define __shared__ static
#define __forceinline__ inline
#define __launch_bounds__(n)
extern thread_local dim3 threadIdx, blockIdx;
extern std::barrier<> *emu_block_bar;
inline void __syncthreads() { emu_block_bar->arrive_and_wait(); }
inline uint32_t emu_perm(uint32_t s0, uint32_t s1, uint32_t sel) {      // v_perm_b32: bytes 0-3 = s1, 4-7 = s0, 12 = 0x00
    const uint64_t all = ((uint64_t)s0 << 32) | s1;
    uint32_t out = 0;
    for (int i = 0; i < 4; ++i) {
        const uint32_t k = (sel >> (8 * i)) & 255;
        const uint32_t b = k < 8 ? (uint32_t)(all >> (8 * k)) & 255 : (k == 12 ? 0u : 0xdeu);
        out |= b << (8 * i);
    }
    return out;
}
#define __builtin_amdgcn_perm emu_perm
inline int imin(int a, int b) { return a < b ? a : b; }
inline int imax(int a, int b) { return a > b ? a : b; }
void emu_launch(dim3 grid, dim3 block, const std::function<void()> &body);
#define hipExtLaunchKernelGGL(kernel, grid, block, shmem, stream, e0, e1, flags, ...) emu_launch(grid, block, [&] { kernel(__VA_ARGS__); })

// ---- the kernels, then the checks ----
#include "../../vp8oclenc_amd/csrc/kernels_geometry.hip"
#include <stdio.h>
#include <memory>
thread_local dim3 threadIdx, blockIdx;
std::barrier<> *emu_block_bar;
namespace vp8 { thread_local LaunchTiming tl_timing; }
void emu_launch(dim3 grid, dim3 block, const std::function<void()> &body) {
    for (unsigned z = 0; z < grid.z; ++z)
        for (unsigned x = 0; x < grid.x; ++x) {
            std::barrier<> bar(block.x);
            emu_block_bar = &bar;
            std::vector<std::thread> th;
            for (unsigned t = 0; t < block.x; ++t)
                th.emplace_back([&, t] {
                    threadIdx = dim3(t);
                    blockIdx = dim3(x, 0, z);
                    body();
                    emu_block_bar->arrive_and_drop();      // (a lane that left before the barrier does not hold the others up)
                });
            for (auto &t : th) t.join();
        }
}
using namespace vp8;
static unsigned seed = 11;
static uint8_t rnd() { seed = seed * 1664525u + 1013904223u; return (uint8_t)(seed >> 24); }
// a heap block of exactly n bytes whose first byte sits at an odd address
struct Block {
    std::unique_ptr<uint8_t[]> mem;
    size_t n;
    explicit Block(size_t bytes) : mem(new uint8_t[bytes + 1]), n(bytes) {}
    uint8_t *p() const { return mem.get() + (((uintptr_t)mem.get() & 1) ? 0 : 1); }      // (one spare byte in FRONT or behind, never both used)
};

static int check_window() {
    const int formats[] = {0, 1, 2, 3, 4, 5, 6, 7, 16, 17, 18, 19};
    const int sizes[][2] = {{48, 32}, {50, 36}}, origins[][2] = {{0, 0}, {2, 6}, {14, 2}}, extra[] = {0, 3, 64};
    long checked = 0;
    for (int format : formats)
        for (const auto &sz : sizes)
            for (const auto &o : origins)
                for (int e : extra) {
                    const int w = sz[0], h = sz[1], x = o[0], y = o[1], n = 2;
                    int32_t tight[3] = {1 << 20, 1 << 20, 1 << 20}, pitch[3], rb[3], rows[3];
                    size_t off[3];
                    // the tight pitch of a surface that just holds the window's right edge
                    if (vp8host_source_window(format, w, h, x, y, tight, off, rb, rows) != 0) { fprintf(stderr, "the rule refused format %d\n", format); return 1; }
                    for (int p = 0; p < 3; ++p) pitch[p] = rows[p] ? rb[p] + (int32_t)(off[p] % (1 << 20)) + e : 0;
                    if (vp8host_source_window(format, w, h, x, y, pitch, off, rb, rows) != 0) { fprintf(stderr, "the rule refused format %d pitch\n", format); return 1; }
                    std::vector<Block> src, dst, want;
                    PlanesItem it[2];
                    for (int m = 0; m < n; ++m)
                        for (int p = 0; p < 3; ++p) {
                            // from the window's first byte to its last: base = block - off
                            const size_t span = rows[p] ? (size_t)(rows[p] - 1) * pitch[p] + rb[p] : 0, tb = (size_t)rows[p] * rb[p];
                            src.emplace_back(span); dst.emplace_back(tb); want.emplace_back(tb);
                            for (size_t i = 0; i < span; ++i) src.back().p()[i] = rnd();
                            memset(dst.back().p(), 0xaa, tb);
                            it[m].src[p] = src.back().p() - off[p];
                            it[m].dst[p] = dst.back().p();
                        }
                    launch_window_batch(nullptr, off, pitch, rb, rows, it, n);
                    for (int m = 0; m < n; ++m) {
                        if (vp8host_window_frame(format, w, h, x, y, pitch, it[m].src[0], it[m].src[1], it[m].src[2], want[3 * m].p(), want[3 * m + 1].p(), want[3 * m + 2].p()) != 0) {
                            fprintf(stderr, "window_frame refused format %d\n", format);
                            return 1;
                        }
                        for (int p = 0; p < 3; ++p)
                            if (memcmp(dst[3 * m + p].p(), want[3 * m + p].p(), want[3 * m + p].n)) {
                                fprintf(stderr, "WINDOW MISMATCH format %d %dx%d at (%d, %d) pitch +%d member %d plane %d\n", format, w, h, x, y, e, m, p);
                                return 1;
                            }
                        checked += 3;
                    }
                }
    printf("window clean (%ld)\n", checked);
    return 0;
}

static int check_orient() {
    const int sizes[][2] = {{16, 16}, {48, 32}, {50, 36}, {200, 70}, {128, 96}, {2, 2}, {2, 130}, {130, 2}, {258, 66}};
    long checked = 0;
    for (const auto &s : sizes)
        for (int turns = 0; turns < 4; ++turns)
            for (int mirror = 0; mirror < 2; ++mirror) {
                if (!turns && !mirror) continue;
                const int w = s[0], h = s[1], n = 2;
                const size_t nb[3] = {(size_t)w * h, (size_t)(w / 2) * (h / 2), (size_t)(w / 2) * (h / 2)};
                std::vector<Block> src, dst, want;
                PlanesItem it[2];
                for (int m = 0; m < n; ++m)
                    for (int p = 0; p < 3; ++p) {
                        src.emplace_back(nb[p]); dst.emplace_back(nb[p]); want.emplace_back(nb[p]);
                        for (size_t i = 0; i < nb[p]; ++i) src.back().p()[i] = rnd();
                        memset(dst.back().p(), 0xaa, nb[p]);
                        it[m].src[p] = src.back().p();
                        it[m].dst[p] = dst.back().p();
                    }
                launch_orient_batch(nullptr, turns, mirror, w, h, it, n);
                for (int m = 0; m < n; ++m) {
                    if (vp8host_orient_frame(turns, mirror, w, h, it[m].src[0], it[m].src[1], it[m].src[2], want[3 * m].p(), want[3 * m + 1].p(), want[3 * m + 2].p()) != 0) {
                        fprintf(stderr, "orient_frame refused %dx%d\n", w, h);
                        return 1;
                    }
                    for (int p = 0; p < 3; ++p)
                        if (memcmp(dst[3 * m + p].p(), want[3 * m + p].p(), nb[p])) {
                            size_t i = 0;
                            while (dst[3 * m + p].p()[i] == want[3 * m + p].p()[i]) ++i;
                            fprintf(stderr, "ORIENT MISMATCH %dx%d turns %d mirror %d member %d plane %d at byte %zu: %d for %d\n", w, h, turns, mirror, m, p, i,
                                    dst[3 * m + p].p()[i], want[3 * m + p].p()[i]);
                            return 1;
                        }
                    checked += 3;
                }
            }
    printf("orient clean (%ld)\n", checked);
    return 0;
}

int main() { return check_window() || check_orient(); }
