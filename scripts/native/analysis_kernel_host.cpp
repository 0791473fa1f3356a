// analysis_kernel_host.cpp -- the two kernel bodies of vp8oclenc_amd/csrc/kernels_analysis.hip, the file as it stands, compiled for the
// HOST and held to the rules of include/vp8hip_host.h under the address and undefined-behaviour sanitizers.  No GPU, no library.
// A workgroup is 256 OS threads that meet at every cross-lane operation (DPP, shuffle) and barrier, so the lanes run in lockstep where
// it matters; v_sad_u8, v_dot4_u32_u8 and the 64-bit atomics are plain C++; workgroups run one after the other.  Planes and the history
// sit in heap blocks of exactly their size: a lane that reads or writes past one is a heap overflow.  Checked: the source side against
// vp8host_analyse_luma at 16x16, 48x32, 80x48, 176x144 and 320x16 (two batch members, with and without a history; random samples,
// 0 / 255 only, half the macroblocks static), the history plane afterwards, the sum words zero at rest; the coding side against a plain
// loop for key frames, inter frames without and with the fallback's flags.
//   clang++ -std=c++20 -O1 -g -pthread -fsanitize=address,undefined -fno-sanitize=alignment -fno-sanitize-recover=all \
//       -I scripts/native/host_stub -I include scripts/native/analysis_kernel_host.cpp vp8oclenc_amd/csrc/vp8_host.cpp \
//       -o analysis_kernel_host && ./analysis_kernel_host
// (-fno-sanitize=alignment: the kernel's 16-byte accesses are typed uint4 on 16-byte-aligned addresses of the device; the host's
// stand-in type is aligned to 4.)
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
typedef void *hipStream_t; typedef void *hipEvent_t;
#define __global__
#define __device__
#define __host__
#define __forceinline__ inline
#define __launch_bounds__(n)
#define __shared__ static
#define __constant__
extern thread_local dim3 threadIdx, blockIdx;
extern std::barrier<> *emu_block_bar, *emu_wave_bar[4];
extern uint64_t emu_slot[4][64];
inline void __syncthreads() { emu_block_bar->arrive_and_wait(); }
inline void __threadfence() { std::atomic_thread_fence(std::memory_order_seq_cst); }
template <typename T> inline T emu_xlane(T v, int src_lane) {
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    uint64_t raw = 0; memcpy(&raw, &v, sizeof(T));
    emu_slot[w][l] = raw;
    emu_wave_bar[w]->arrive_and_wait();
    raw = emu_slot[w][src_lane];
    emu_wave_bar[w]->arrive_and_wait();
    T out; memcpy(&out, &raw, sizeof(T));
    return out;
}
template <typename T> inline T __shfl_xor(T v, int m, int) { return emu_xlane(v, (int)(threadIdx.x & 63) ^ m); }
inline int emu_update_dpp(int, int src, int ctrl, int, int, bool) {
    const int l = threadIdx.x & 63;
    int from;
    if (ctrl == 0x141) from = (l & ~7) | (7 - (l & 7));
    else if (ctrl == 0x140) from = (l & ~15) | (15 - (l & 15));
    else from = (l & ~3) | ((ctrl >> (2 * (l & 3))) & 3);
    return emu_xlane(src, from);
}
inline uint32_t emu_sad_u8(uint32_t a, uint32_t b, uint32_t c) { for (int i = 0; i < 4; ++i) { int x = (a >> 8 * i) & 255, y = (b >> 8 * i) & 255; c += x > y ? x - y : y - x; } return c; }
inline uint32_t emu_udot4(uint32_t a, uint32_t b, uint32_t c, bool) { for (int i = 0; i < 4; ++i) c += ((a >> 8 * i) & 255) * ((b >> 8 * i) & 255); return c; }
#define __builtin_amdgcn_update_dpp emu_update_dpp
#define __builtin_amdgcn_sad_u8 emu_sad_u8
#define __builtin_amdgcn_udot4 emu_udot4
inline unsigned long long atomicAdd(unsigned long long *p, unsigned long long v) { return __atomic_fetch_add(p, v, __ATOMIC_SEQ_CST); }
inline unsigned long long atomicExch(unsigned long long *p, unsigned long long v) { return __atomic_exchange_n(p, v, __ATOMIC_SEQ_CST); }
#define __HIP_MEMORY_SCOPE_SYSTEM 0
#define __hip_atomic_store(p, v, order, scope) __atomic_store_n(p, v, order)
inline int imin(int a, int b) { return a < b ? a : b; }
inline int iabs(int v) { return v < 0 ? -v : v; }
void emu_launch(dim3 grid, dim3 block, const std::function<void()> &body);
#define hipExtLaunchKernelGGL(kernel, grid, block, shmem, stream, e0, e1, flags, ...) emu_launch(grid, block, [&] { kernel(__VA_ARGS__); })

// ---- the kernels, then the checks ----
#include "../../vp8oclenc_amd/csrc/kernels_analysis.hip"
#include "vp8hip_host.h"
#include <stdio.h>
#include <memory>
thread_local dim3 threadIdx, blockIdx;
std::barrier<> *emu_block_bar, *emu_wave_bar[4];
uint64_t emu_slot[4][64];
namespace vp8 { thread_local LaunchTiming tl_timing; }
void emu_launch(dim3 grid, dim3 block, const std::function<void()> &body) {
    for (unsigned z = 0; z < grid.z; ++z)
        for (unsigned x = 0; x < grid.x; ++x) {
            std::barrier<> bb(block.x), w0(64), w1(64), w2(64), w3(64);
            emu_block_bar = &bb; emu_wave_bar[0] = &w0; emu_wave_bar[1] = &w1; emu_wave_bar[2] = &w2; emu_wave_bar[3] = &w3;
            std::vector<std::thread> th;
            for (unsigned t = 0; t < block.x; ++t)
                th.emplace_back([&, t] { threadIdx = dim3(t); blockIdx = dim3(x, 0, z); body(); });
            for (auto &t : th) t.join();
        }
}
using namespace vp8;
static unsigned seed = 7;
static uint8_t rnd() { seed = seed * 1664525u + 1013904223u; return (uint8_t)(seed >> 24); }
int main() {
    const int sizes[][2] = {{16, 16}, {48, 32}, {80, 48}, {176, 144}, {320, 16}};
    long checked = 0;
    for (const auto &s : sizes)
        for (int kind = 0; kind < 3; ++kind) {
            const int w = s[0], h = s[1], stride = (w + 63) / 64 * 64 , n = 2;
            std::unique_ptr<uint8_t[]> cur[2], hist[2], hist0[2];
            alignas(8) unsigned long long acc[2][5] = {};
            AnalysisSrcMirror host[2] = {};
            AnalysisSrcItem it[2];
            for (int m = 0; m < n; ++m) {
                cur[m].reset(new uint8_t[(size_t)stride * (h - 1) + w]);      // (exactly up to the last sample: a read past it is a heap overflow)
                hist[m].reset(new uint8_t[(size_t)w * h]); hist0[m].reset(new uint8_t[(size_t)w * h]);
                for (size_t i = 0; i < (size_t)stride * (h - 1) + w; ++i) cur[m][i] = kind == 1 ? (rnd() & 1 ? 255 : 0) : rnd();
                for (int y = 0; y < h; ++y) for (int x = 0; x < w; ++x) {
                    uint8_t c = cur[m][(size_t)y * stride + x];
                    hist0[m][(size_t)y * w + x] = hist[m][(size_t)y * w + x] = kind == 1 ? 255 - c : (kind == 2 && (x / 16 + y / 16) % 2 ? c : rnd());
                }
                it[m].cur = Plane{cur[m].get(), stride, w, h};
                it[m].hist = hist[m].get(); it[m].acc = acc[m]; it[m].host = &host[m]; it[m].seq = 5 + m; it[m].frame_number = 3; it[m].have_prev = m == 0 || kind == 2;
            }
            launch_analyse_src_batch(nullptr, it, n);
            for (int m = 0; m < n; ++m) {
                std::unique_ptr<uint8_t[]> tight(new uint8_t[(size_t)w * h]);
                for (int y = 0; y < h; ++y) memcpy(tight.get() + (size_t)y * w, cur[m].get() + (size_t)y * stride, w);
                vp8host_luma_analysis want;
                vp8host_analyse_luma(tight.get(), it[m].have_prev ? hist0[m].get() : nullptr, w, h, &want);
                if (host[m].seq != 5u + m || host[m].frame_number != 3 || host[m].spatial != want.spatial || host[m].sse != want.temporal_sse || host[m].sad != want.temporal_sad ||
                    host[m].static_mbs != want.static_mbs || host[m].have_prev != want.have_prev || memcmp(hist[m].get(), tight.get(), (size_t)w * h) != 0) {
                    fprintf(stderr, "MISMATCH %dx%d kind %d member %d: spatial %llu/%llu sse %llu/%llu sad %llu/%llu static %d/%d\n", w, h, kind, m, (unsigned long long)host[m].spatial,
                            (unsigned long long)want.spatial, (unsigned long long)host[m].sse, (unsigned long long)want.temporal_sse, (unsigned long long)host[m].sad, (unsigned long long)want.temporal_sad, host[m].static_mbs, want.static_mbs);
                    return 1;
                }
                for (int i = 0; i < 5; ++i) if (acc[m][i]) { fprintf(stderr, "acc not zero at rest\n"); return 1; }
                checked += want.static_mbs + 1;
            }
        }
    // the coding side against a plain loop
    for (int mbs : {1, 6, 99, 300, 1000})
        for (int mode = 0; mode < 3; ++mode) {      // key; inter without flags; inter with flags
            std::vector<int32_t> parts(mbs), ref(mbs), seg(mbs), nz(mbs), inter(mbs);
            std::unique_ptr<int16_t[]> vec(new int16_t[(size_t)mbs * 8]);
            int32_t replaced = 0;
            for (int i = 0; i < mbs; ++i) {
                parts[i] = rnd() & 1; ref[i] = rnd() % 3; seg[i] = rnd() & 3; nz[i] = rnd() % 5 ? rnd() : 0; inter[i] = rnd() % 4 != 0;
                replaced += !inter[i];
                for (int k = 0; k < 8; ++k) vec[(size_t)i * 8 + k] = rnd() % 3 ? (int16_t)((rnd() << 8 | rnd()) ) : 0;
                if (rnd() % 5 == 0) for (int k = 0; k < 8; ++k) vec[(size_t)i * 8 + k] = 0;
            }
            if (mbs > 2) { for (int k = 0; k < 8; ++k) vec[k] = -32768; }
            int32_t rep[1] = {mode == 2 ? replaced : 0};
            AnalysisMbMirror got{};
            AnalysisMbItem it{parts.data(), ref.data(), seg.data(), nz.data(), inter.data(), mode == 0 ? nullptr : rep, vec.get(), &got, 9u, 4, mode == 0, mbs};
            launch_analyse_mb_batch(nullptr, &it, 1);
            AnalysisMbMirror w{};
            w.frame_number = 4; w.is_key = mode == 0; w.mbs_total = mbs; w.seq = 9;
            for (int i = 0; i < mbs; ++i) {
                w.nz_coeffs += nz[i]; w.mbs_no_coeffs += nz[i] == 0; w.segment_mbs[seg[i]]++;
                const bool in = mode != 0 && !(mode == 2 && replaced > 0 && !inter[i]);
                if (!in) { w.mbs_intra++; continue; }
                w.mbs_ref[ref[i]]++; w.mbs_split += parts[i] == 1;
                bool z = true;
                for (int b = 0; b < 4; ++b) for (int k = 0; k < 2; ++k) {
                    const int v = vec[(size_t)i * 8 + b * 2 + k];
                    z = z && v == 0; w.mv_abs_sum[k] += v < 0 ? -v : v; w.mv_sum[k] += v; w.mv_sq_sum += (int64_t)v * v;
                }
                w.mbs_zero_mv += z;
            }
            if (memcmp(&w, &got, sizeof(w)) != 0) { fprintf(stderr, "MB MISMATCH mbs %d mode %d: intra %d/%d zero %d/%d sq %llu/%llu\n", mbs, mode, got.mbs_intra, w.mbs_intra, got.mbs_zero_mv, w.mbs_zero_mv, (unsigned long long)got.mv_sq_sum, (unsigned long long)w.mv_sq_sum); return 1; }
            ++checked;
        }
    printf("kernel bodies equal the rules (%ld)\n", checked);
    return 0;
}
