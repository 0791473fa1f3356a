// canvas_rule_check.cpp -- the canvas fields of vp8oclenc_amd/csrc/intake_settings.h through the one validity rule, for
// tests/test_compose_cpu.py: every line of standard input is one complete candidate,
//     W H src_w src_h in_w in_h scale_kind src_fmt win_on or_turns or_mirror di_mode bg_y bg_u bg_v n_tiles {in_w in_h x y w h filter} ...
// (a window is the tight one of the incoming size at (0, 0)), and every line of output its verdict: "ok" or "refused", then whether
// the candidate excludes hidden alt-ref frames, a by-reference split and a batch ("arf", "shard", "batch"), then whether its canonical
// form equals the canonical form of the same candidate without its canvas ("plain").  Pure host code: no GPU, no library.
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include scripts/native/canvas_rule_check.cpp
//       vp8oclenc_amd/csrc/vp8_host.cpp -o canvas_rule_check && ./canvas_rule_check < cases      (one command line)
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "../../vp8oclenc_amd/csrc/intake_settings.h"

using namespace vp8;

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        int W, H, win_on;
        IntakeSettings s;
        if (!(in >> W >> H >> s.src_w >> s.src_h >> s.in_w >> s.in_h >> s.scale_kind >> s.src_fmt >> win_on >> s.or_turns >> s.or_mirror >> s.di_mode >> s.bg[0] >>
              s.bg[1] >> s.bg[2] >> s.n_tiles)) {
            fprintf(stderr, "a line that is no candidate: %s\n", line.c_str());
            return 1;
        }
        for (int k = 0; k < s.n_tiles && k < VP8HIP_MAX_TILES; ++k) {
            vp8hip_tile &t = s.tile[k];
            if (!(in >> t.in_w >> t.in_h >> t.x >> t.y >> t.w >> t.h >> t.filter)) {
                fprintf(stderr, "a line that ends inside a tile: %s\n", line.c_str());
                return 1;
            }
        }
        if (win_on) {
            int w, h;
            incoming_size(s, W, H, &w, &h);
            s.win_on = true;
            s.win_pitch[0] = w;
            s.win_pitch[1] = s.win_pitch[2] = w / 2;
        }
        const IntakeSettings c = canonical(s, W, H);
        IntakeSettings plain = s;
        plain.n_tiles = 0;
        printf("%s%s%s%s%s\n", intake_valid(W, H, c) == INTAKE_OK ? "ok" : "refused", excludes_arf(c) ? " arf" : "", excludes_shard(c) ? " shard" : "",
               excludes_batch(c) ? " batch" : "", c == canonical(plain, W, H) ? " plain" : "");
    }
    return 0;
}
