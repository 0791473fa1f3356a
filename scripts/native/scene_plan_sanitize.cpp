// scene_plan_sanitize.cpp -- vp8host_scene_plan under the host sanitizers.  The two difference arrays and the two result arrays are heap
// blocks of exactly nframes entries: a read or a write past any of them is a heap overflow.  Random difference sequences (a detection in
// about one frame of seven), every GOP length from 1 to 12, lengths 0 to 61, with and without by_scene; every result is held against the
// frame loop's own steps (vp8host_gop_*, vp8host_scene_change) taken one by one, and the constructed case of tests/test_scene_plan_cpu.py
// against its list.  No GPU, no library: it is linked with vp8_host.cpp alone.
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include scripts/native/scene_plan_sanitize.cpp \
//       vp8oclenc_amd/csrc/vp8_host.cpp -o scene_plan_sanitize && ./scene_plan_sanitize
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "vp8hip_host.h"

int main() {
    unsigned seed = 7;
    auto next = [&] { seed = seed * 1664525u + 1013904223u; return seed >> 8; };
    long checked = 0;
    for (int n = 0; n <= 61; ++n)
        for (int g = 1; g <= 12; ++g)
            for (int with_scene = 0; with_scene < 2; ++with_scene) {
                std::unique_ptr<int32_t[]> ud(new int32_t[n]), vd(new int32_t[n]);
                std::unique_ptr<uint8_t[]> key(new uint8_t[n]), scene(new uint8_t[n]);
                for (int t = 0; t < n; ++t) {
                    const bool cut = next() % 7 == 0;
                    ud[t] = cut ? 8 + (int32_t)(next() % 200) : (int32_t)(next() % 6);      // (a detection: Udiff > 7)
                    vd[t] = (int32_t)(next() % 5);                                            // (never one by itself: U + V <= 9 without a cut)
                }
                memset(key.get(), 0xee, (size_t)n);
                memset(scene.get(), 0xee, (size_t)n);
                const int keys = vp8host_scene_plan(ud.get(), vd.get(), n, g, key.get(), with_scene ? scene.get() : nullptr);
                vp8host_gop gop;
                vp8host_scene_state st{};
                vp8host_gop_init(&gop, g, 5);
                int want_keys = 0;
                for (int t = 0; t < n; ++t) {
                    vp8host_gop_next(&gop);
                    int k = gop.current_is_key, s = 0;
                    if (!k && vp8host_scene_change(&st, ud[t], vd[t], gop.frame_number)) k = s = 1;
                    if (k) { st.last_key_detect = gop.frame_number; vp8host_gop_key_coded(&gop); }
                    vp8host_gop_frame_done(&gop);
                    want_keys += k;
                    if (key[t] != k || (with_scene && scene[t] != s)) { fprintf(stderr, "n %d g %d frame %d: key %d (stepped %d), by scene %d (stepped %d)\n", n, g, t, key[t], k, scene[t], s); return 1; }
                }
                if (keys != want_keys || (n > 0 && !key[0])) { fprintf(stderr, "n %d g %d: %d key frames, stepped %d\n", n, g, keys, want_keys); return 1; }
                checked += n;
            }
    {   // g = 9, 34 frames, cuts at 6, 8, 21, 22, 33
        int32_t ud[34] = {0}, vd[34] = {0};
        uint8_t key[34], scene[34];
        const int cuts[] = {6, 8, 21, 22, 33}, want[] = {0, 6, 12, 21, 26, 33};
        for (int c : cuts) ud[c] = 40;
        if (vp8host_scene_plan(ud, vd, 34, 9, key, scene) != 6) { fprintf(stderr, "the constructed case: not 6 key frames\n"); return 1; }
        int k = 0;
        for (int t = 0; t < 34; ++t)
            if (key[t] && (k >= 6 || want[k++] != t)) { fprintf(stderr, "the constructed case: a key frame at %d\n", t); return 1; }
    }
    {   // the refusals
        int32_t d[1] = {0};
        uint8_t k[1];
        if (vp8host_scene_plan(nullptr, d, 1, 5, k, nullptr) != -1 || vp8host_scene_plan(d, nullptr, 1, 5, k, nullptr) != -1 || vp8host_scene_plan(d, d, 1, 5, nullptr, nullptr) != -1 ||
            vp8host_scene_plan(d, d, -1, 5, k, nullptr) != -1 || vp8host_scene_plan(d, d, 1, 0, k, nullptr) != -1) {
            fprintf(stderr, "a bad argument was not refused\n");
            return 1;
        }
    }
    printf("clean (%ld)\n", checked);
    return 0;
}
