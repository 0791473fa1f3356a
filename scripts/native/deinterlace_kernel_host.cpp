// deinterlace_kernel_host.cpp -- the kernel body of vp8oclenc_amd/csrc/kernels_deinterlace.hip, the file as it stands, compiled for the
// HOST and held to vp8host_deinterlace_frame under the address and undefined-behaviour sanitizers.  No GPU, no library.
// A workgroup is 256 OS threads that meet at the one cross-lane operation (the shuffle of the wave's count); v_perm_b32 and the 64-bit
// atomics are plain C++; workgroups run one after the other.  Every plane, staging buffer and history sits in a heap block of exactly
// its size at an ODD address offset: a lane that reads or writes past one is a heap overflow, and no access is aligned by luck.
// Checked: output, new history, the record and the count word at rest, two batch members (one with, one without a history in mode 2),
// both parities, both modes, at 16x16, 48x32, 56x40, 50x36, 128x96, 16x4, 2x4, 34x6 and 1920x8.
//   clang++ -std=c++20 -O1 -g -pthread -fsanitize=address,undefined -fno-sanitize=alignment -fno-sanitize-recover=all \
//       -I scripts/native/host_stub -I include scripts/native/deinterlace_kernel_host.cpp vp8oclenc_amd/csrc/vp8_host.cpp \
//       -o deinterlace_kernel_host && ./deinterlace_kernel_host
// (-fno-sanitize=alignment: the kernel's 16-byte accesses are unaligned vector accesses on the device.)
#include <stdint.h>
#include <stddef.h>
#include <string.h>
#include <atomic>
#include <barrier>
#include <functional>
#include <thread>
#include <vector>
struct dim3 { unsigned x, y, z; dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {} };
struct uint4 { uint32_t x, y, z, w; };
inline uint4 make_uint4(uint32_t x, uint32_t y, uint32_t z, uint32_t w) { return uint4{x, y, z, w}; }
typedef void *hipStream_t; typedef void *hipEvent_t;
#define __global__
#define __device__
#define __host__
#define __forceinline__ inline
#define __launch_bounds__(n)
#define asm(...) (void)0      /* (the empty asm that hides a constant from hipcc) */
extern thread_local dim3 threadIdx, blockIdx;
extern std::barrier<> *emu_wave_bar[4];
extern uint64_t emu_slot[4][64];
inline int __shfl_xor(int v, int m) {
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    emu_slot[w][l] = (uint32_t)v;
    emu_wave_bar[w]->arrive_and_wait();
    const int out = (int)emu_slot[w][l ^ m];
    emu_wave_bar[w]->arrive_and_wait();
    return out;
}
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
inline unsigned long long atomicAdd(unsigned long long *p, unsigned long long v) { return __atomic_fetch_add(p, v, __ATOMIC_SEQ_CST); }
inline unsigned long long atomicExch(unsigned long long *p, unsigned long long v) { return __atomic_exchange_n(p, v, __ATOMIC_SEQ_CST); }
#define __HIP_MEMORY_SCOPE_SYSTEM 0
#define __hip_atomic_store(p, v, order, scope) __atomic_store_n(p, v, order)
inline int imin(int a, int b) { return a < b ? a : b; }
inline int imax(int a, int b) { return a > b ? a : b; }
inline int iabs(int v) { return v < 0 ? -v : v; }
typedef short s16x2 __attribute__((ext_vector_type(2)));
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
inline s16x2 as_s16x2(uint32_t v) { return __builtin_bit_cast(s16x2, v); }
inline uint32_t as_u32(s16x2 v) { return __builtin_bit_cast(uint32_t, v); }
void emu_launch(dim3 grid, dim3 block, const std::function<void()> &body);
#define hipExtLaunchKernelGGL(kernel, grid, block, shmem, stream, e0, e1, flags, ...) emu_launch(grid, block, [&] { kernel(__VA_ARGS__); })

// ---- the kernel, then the checks ----
#include "../../vp8oclenc_amd/csrc/kernels_deinterlace.hip"
#include <stdio.h>
#include <memory>
thread_local dim3 threadIdx, blockIdx;
std::barrier<> *emu_wave_bar[4];
uint64_t emu_slot[4][64];
namespace vp8 { thread_local LaunchTiming tl_timing; }
void emu_launch(dim3 grid, dim3 block, const std::function<void()> &body) {
    for (unsigned z = 0; z < grid.z; ++z)
        for (unsigned x = 0; x < grid.x; ++x) {
            std::barrier<> w0(64), w1(64), w2(64), w3(64);
            emu_wave_bar[0] = &w0; emu_wave_bar[1] = &w1; emu_wave_bar[2] = &w2; emu_wave_bar[3] = &w3;
            std::vector<std::thread> th;
            for (unsigned t = 0; t < block.x; ++t)
                th.emplace_back([&, t] { threadIdx = dim3(t); blockIdx = dim3(x, 0, z); body(); });
            for (auto &t : th) t.join();
        }
}
using namespace vp8;
static unsigned seed = 7;
static uint8_t rnd() { seed = seed * 1664525u + 1013904223u; return (uint8_t)(seed >> 24); }
// a heap block of exactly n bytes whose first byte sits at an odd address
struct Block {
    std::unique_ptr<uint8_t[]> mem;
    size_t n;
    explicit Block(size_t bytes) : mem(new uint8_t[bytes + 1]), n(bytes) {}
    uint8_t *p() const { return mem.get() + (((uintptr_t)mem.get() & 1) ? 0 : 1); }      // (one spare byte in FRONT or behind, never both used)
};
int main() {
    const int sizes[][2] = {{16, 16}, {48, 32}, {56, 40}, {50, 36}, {128, 96}, {16, 4}, {2, 4}, {34, 6}, {1920, 8}};
    long checked = 0;
    for (const auto &s : sizes)
        for (int mode = 1; mode <= 2; ++mode)
            for (int keep = 0; keep <= 1; ++keep) {
                const int w = s[0], h = s[1], n = 2;
                const size_t nb[3] = {(size_t)w * h, (size_t)(w / 2) * (h / 2), (size_t)(w / 2) * (h / 2)};
                std::vector<Block> src, hist, hist0, dst, kh, want;
                alignas(8) unsigned long long word[2] = {0, 0};
                DeinterlaceMirror host[2] = {};
                DeinterlaceItem it[2];
                for (int m = 0; m < n; ++m)
                    for (int k = 0; k < 3; ++k) {
                        src.emplace_back(nb[k]); hist.emplace_back(nb[k]); hist0.emplace_back(nb[k]); dst.emplace_back(nb[k]); kh.emplace_back(nb[k]); want.emplace_back(nb[k]);
                        for (size_t i = 0; i < nb[k]; ++i) {
                            src.back().p()[i] = rnd() & 3 ? rnd() : (rnd() & 1 ? 255 : 0);
                            hist.back().p()[i] = hist0.back().p()[i] = (i / 3) & 1 ? src.back().p()[i] : rnd();      // (runs of three stand still)
                        }
                        memset(dst.back().p(), 0xaa, nb[k]); memset(kh.back().p(), 0xbb, nb[k]);
                    }
                for (int m = 0; m < n; ++m) {
                    const bool have = mode == 2 && m == 0;
                    for (int k = 0; k < 3; ++k) {
                        it[m].src[k] = src[3 * m + k].p();
                        it[m].hist[k] = have ? hist[3 * m + k].p() : nullptr;
                        it[m].dst[k] = dst[3 * m + k].p();
                        it[m].keep_hist[k] = mode == 2 ? kh[3 * m + k].p() : nullptr;
                    }
                    it[m].word = &word[m]; it[m].host = &host[m]; it[m].seq = 5 + m; it[m].frame_number = 3;
                }
                launch_deinterlace_batch(nullptr, w, h, keep, it, n);
                for (int m = 0; m < n; ++m) {
                    const bool have = mode == 2 && m == 0;
                    int32_t woven = -1;
                    uint8_t *hp[3] = {mode == 2 ? hist0[3 * m].p() : nullptr, mode == 2 ? hist0[3 * m + 1].p() : nullptr, mode == 2 ? hist0[3 * m + 2].p() : nullptr};
                    if (vp8host_deinterlace_frame(src[3 * m].p(), src[3 * m + 1].p(), src[3 * m + 2].p(), hp[0], hp[1], hp[2], want[3 * m].p(), want[3 * m + 1].p(),
                                                  want[3 * m + 2].p(), w, h, mode, keep, have, &woven) != 0) { fprintf(stderr, "the rule refused %dx%d\n", w, h); return 1; }
                    for (int k = 0; k < 3; ++k) {
                        if (memcmp(dst[3 * m + k].p(), want[3 * m + k].p(), nb[k])) {
                            size_t i = 0;
                            while (dst[3 * m + k].p()[i] == want[3 * m + k].p()[i]) ++i;
                            const size_t pw = k ? w / 2 : w;
                            fprintf(stderr, "MISMATCH %dx%d mode %d keep %d member %d plane %d at (%zu, %zu): %d for %d\n", w, h, mode, keep, m, k, i / pw, i % pw,
                                    dst[3 * m + k].p()[i], want[3 * m + k].p()[i]);
                            return 1;
                        }
                        if (mode == 2 && memcmp(kh[3 * m + k].p(), src[3 * m + k].p(), nb[k])) { fprintf(stderr, "the new history is not the frame as received: %dx%d plane %d\n", w, h, k); return 1; }
                    }
                    if (host[m].seq != 5u + m || host[m].frame_number != 3 || host[m].woven != woven || host[m].missing != w * h / 2 || word[m]) {
                        fprintf(stderr, "RECORD %dx%d mode %d keep %d member %d: seq %u woven %d / %d missing %d word %llu\n", w, h, mode, keep, m, host[m].seq, host[m].woven, woven,
                                host[m].missing, word[m]);
                        return 1;
                    }
                    if (have && w > 2 && woven == 0) { fprintf(stderr, "nothing woven: the check is not about weaving\n"); return 1; }
                    checked += woven + 1;
                }
            }
    printf("clean (%ld)\n", checked);
    return 0;
}
