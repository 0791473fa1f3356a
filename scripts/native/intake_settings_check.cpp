// intake_settings_check.cpp -- vp8oclenc_amd/csrc/intake_settings.h on the host, under the sanitizers: the one validity rule against the
// verdicts the GPU suites assert of the setters (literals, copied from tests/test_gpu_geometry.py, test_gpu_tonemap.py,
// test_gpu_deinterlace.py, test_gpu_scale.py and test_gpu_source_format.py: nothing here is computed by the header), the equality field
// by field, the canonical form, needs_device_planes against its six terms, and the size helpers under an odd turn.  No GPU, no library.
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include scripts/native/intake_settings_check.cpp
//       vp8oclenc_amd/csrc/vp8_host.cpp -o intake_settings_check && ./intake_settings_check      (one command line)
#include <cstdio>
#include <functional>
#include <initializer_list>
#include <utility>
#include <vector>

#include "../../vp8oclenc_amd/csrc/intake_settings.h"

using namespace vp8;

namespace {

int failures = 0;
void expect(bool ok, const char *what, int k = -1) {
    if (ok) return;
    fprintf(stderr, "FAILED: %s (%d)\n", what, k);
    ++failures;
}

IntakeSettings window(IntakeSettings s, int p0, int p1, int p2, int x, int y) {
    s.win_on = true;
    s.win_pitch[0] = p0; s.win_pitch[1] = p1; s.win_pitch[2] = p2;
    s.win_x = x; s.win_y = y;
    return s;
}
IntakeSettings orientation(IntakeSettings s, int turns, int mirror) { s.or_turns = turns; s.or_mirror = mirror; return s; }
IntakeSettings format(IntakeSettings s, int f) { s.src_fmt = f; return s; }
IntakeSettings transfer(IntakeSettings s, int t, int peak) { s.src_transfer = t; s.src_peak = peak; return s; }
IntakeSettings size(IntakeSettings s, int w, int h) { s.src_w = w; s.src_h = h; s.in_w = s.in_h = s.scale_kind = 0; return s; }
IntakeSettings scaling(IntakeSettings s, int iw, int ih, int dw, int dh, int kind) { s.src_w = dw; s.src_h = dh; s.in_w = iw; s.in_h = ih; s.scale_kind = kind; return s; }
IntakeSettings deinterlace(IntakeSettings s, int mode, int keep) { s.di_mode = mode; s.di_keep = keep; return s; }

struct Case { const char *what; int W, H; IntakeSettings s; bool ok; };

// (a) complete settings and the verdict each must get
void verdicts() {
    std::vector<Case> t;
    const IntakeSettings none;
    {   // test_gpu_geometry.py::test_a_refused_setting_leaves_the_previous_one_in_force: 48x32, the window of pitch 83 at (2, 6), turned twice behind a mirror
        const IntakeSettings g = orientation(window(none, 83, 43, 43, 2, 6), 2, 1);
        t.push_back({"geometry: in force", 48, 32, g, true});
        t.push_back({"window x odd", 48, 32, window(g, 83, 43, 43, 1, 6), false});
        t.push_back({"window y odd", 48, 32, window(g, 83, 43, 43, 2, 5), false});
        t.push_back({"window x negative", 48, 32, window(g, 83, 43, 43, -2, 6), false});
        t.push_back({"window y negative", 48, 32, window(g, 83, 43, 43, 2, -2), false});
        t.push_back({"luma pitch 49", 48, 32, window(g, 49, 43, 43, 2, 6), false});
        t.push_back({"u pitch 24", 48, 32, window(g, 83, 24, 43, 2, 6), false});
        t.push_back({"v pitch 24", 48, 32, window(g, 83, 43, 24, 2, 6), false});
        t.push_back({"window x 36", 48, 32, window(g, 83, 43, 43, 36, 6), false});
        t.push_back({"turns 4", 48, 32, orientation(g, 4, 0), false});
        t.push_back({"turns -1", 48, 32, orientation(g, -1, 0), false});
        t.push_back({"mirror 2", 48, 32, orientation(g, 0, 2), false});
        t.push_back({"mirror -1", 48, 32, orientation(g, 1, -1), false});
        t.push_back({"BGRA: rows of 200 bytes in a pitch of 83", 48, 32, format(g, VP8HOST_FORMAT_BGRA), false});
        t.push_back({"scaling from 96x64: rows of 98 bytes", 48, 32, scaling(g, 96, 64, 48, 32, 0), false});
        t.push_back({"one turn: 32 wide, the window fits", 48, 32, orientation(g, 1, 0), true});
        const IntakeSettings tall = window(none, 34, 17, 17, 2, 0);      // 32x48
        t.push_back({"tall: in force", 32, 48, tall, true});
        t.push_back({"tall, one turn: raw 48 wide, rows of 50 bytes", 32, 48, orientation(tall, 1, 0), false});
        t.push_back({"tall, two turns", 32, 48, orientation(tall, 2, 0), true});
        const IntakeSettings thin = deinterlace(size(none, 2, 16), 1, 0);      // 16x16, the picture 2x16
        t.push_back({"thin: in force", 16, 16, thin, true});
        t.push_back({"thin, one turn: a raw height of 2 under a deinterlacer", 16, 16, orientation(thin, 1, 0), false});
        t.push_back({"thin, two turns and a mirror", 16, 16, orientation(thin, 2, 1), true});
    }
    {   // test_gpu_tonemap.py::test_setter_rules: 34x18 inside 48x32, I010 under HLG at 1000 nits
        const IntakeSettings hdr = transfer(format(size(none, 34, 18), VP8HOST_FORMAT_I010), VP8HOST_TRANSFER_HLG, 1000);
        t.push_back({"tone map: in force", 48, 32, hdr, true});
        for (int f : {6, 7, 1, 16}) t.push_back({"a transfer in force, a format it does not cover", 48, 32, format(hdr, f), false});
        t.push_back({"peak 399", 48, 32, transfer(hdr, VP8HOST_TRANSFER_HLG, 399), false});
        t.push_back({"peak 10001", 48, 32, transfer(hdr, VP8HOST_TRANSFER_PQ, 10001), false});
        t.push_back({"transfer 3", 48, 32, transfer(hdr, 3, 1000), false});
        t.push_back({"transfer -1", 48, 32, transfer(hdr, -1, 1000), false});
        for (int f : {6, 7, 1, 16}) {
            t.push_back({"no transfer: any format", 48, 32, format(transfer(hdr, 0, 0), f), true});
            t.push_back({"that format in force, a transfer", 48, 32, transfer(format(hdr, f), VP8HOST_TRANSFER_PQ, 1000), false});
        }
    }
    {   // test_gpu_deinterlace.py::test_errors
        for (auto bad : std::initializer_list<std::pair<int, int>>{{3, 0}, {-1, 0}, {1, 2}, {2, -1}}) t.push_back({"deinterlace: mode or parity", 64, 48, deinterlace(none, bad.first, bad.second), false});
        t.push_back({"deinterlace 2, 1", 64, 48, deinterlace(none, 2, 1), true});
        t.push_back({"height 2: the chroma planes have one row", 16, 16, deinterlace(size(none, 16, 2), 1, 0), false});
        t.push_back({"height 4", 16, 16, deinterlace(size(none, 16, 4), 1, 0), true});
    }
    {   // test_gpu_scale.py::test_switching_between_frames_gives_what_fresh_contexts_give: 320x240 (the 6:1 Lanczos case is the plan's refusal, not this rule's)
        t.push_back({"640x480 to 320x240, area", 320, 240, scaling(none, 640, 480, 0, 0, 0), true});      // (a dst equal to the coded size is stored as 0)
        t.push_back({"480x360 to 316x236, Lanczos", 320, 240, scaling(none, 480, 360, 316, 236, 1), true});
        t.push_back({"filter 2", 320, 240, scaling(none, 640, 480, 320, 240, 2), false});
        t.push_back({"incoming width odd", 320, 240, scaling(none, 641, 480, 320, 240, 0), false});
        t.push_back({"20 below the coded width", 320, 240, scaling(none, 640, 480, 300, 240, 0), false});
        t.push_back({"above the coded width", 320, 240, scaling(none, 640, 480, 322, 240, 0), false});
        t.push_back({"scaling up", 320, 240, scaling(none, 300, 480, 320, 240, 0), false});
        t.push_back({"16386 wide", 320, 240, scaling(none, 16386, 480, 320, 240, 0), false});
        t.push_back({"height 0", 320, 240, scaling(none, 640, 480, 320, 0, 0), false});
    }
    for (int f : {8, -1, 1 << 20}) t.push_back({"test_gpu_source_format.py::test_argument_errors", 64, 48, format(none, f), false});
    t.push_back({"nothing set", 64, 48, none, true});
    for (size_t k = 0; k < t.size(); ++k) expect((intake_valid(t[k].W, t[k].H, t[k].s) == INTAKE_OK) == t[k].ok, t[k].what, (int)k);
}

// every field, through one edit each (a field this list lacks fails the sizeof check below)
std::vector<std::function<void(IntakeSettings &)>> edits() {
    return {[](IntakeSettings &s) { s.src_w -= 2; }, [](IntakeSettings &s) { s.src_h -= 2; }, [](IntakeSettings &s) { s.in_w += 2; }, [](IntakeSettings &s) { s.in_h += 2; },
            [](IntakeSettings &s) { s.scale_kind ^= 1; }, [](IntakeSettings &s) { s.src_fmt = VP8HOST_FORMAT_P010; }, [](IntakeSettings &s) { s.src_colour ^= 1; },
            [](IntakeSettings &s) { s.src_transfer = VP8HOST_TRANSFER_PQ; }, [](IntakeSettings &s) { s.src_peak += 1; }, [](IntakeSettings &s) { s.win_on = false; },
            [](IntakeSettings &s) { s.win_pitch[0] += 1; }, [](IntakeSettings &s) { s.win_pitch[1] += 1; }, [](IntakeSettings &s) { s.win_pitch[2] += 1; },
            [](IntakeSettings &s) { s.win_x += 2; }, [](IntakeSettings &s) { s.win_y += 2; }, [](IntakeSettings &s) { s.or_turns ^= 2; }, [](IntakeSettings &s) { s.or_mirror ^= 1; },
            [](IntakeSettings &s) { s.di_mode ^= 3; }, [](IntakeSettings &s) { s.di_keep ^= 1; }, [](IntakeSettings &s) { s.dn_level ^= 1; }, [](IntakeSettings &s) { s.an_on = false; },
            [](IntakeSettings &s) { s.seg_mode = 1; }, [](IntakeSettings &s) { s.seg_strength ^= 1; },
            // the canvas (tests/test_compose_cpu.py has its verdicts): the count, the background, a tile's seven fields, the last tile
            [](IntakeSettings &s) { s.n_tiles += 1; }, [](IntakeSettings &s) { s.bg[0] += 1; }, [](IntakeSettings &s) { s.bg[1] += 1; }, [](IntakeSettings &s) { s.bg[2] += 1; },
            [](IntakeSettings &s) { s.tile[0].in_w += 2; }, [](IntakeSettings &s) { s.tile[0].in_h += 2; }, [](IntakeSettings &s) { s.tile[0].x += 2; },
            [](IntakeSettings &s) { s.tile[0].y += 2; }, [](IntakeSettings &s) { s.tile[0].w += 2; }, [](IntakeSettings &s) { s.tile[0].h += 2; },
            [](IntakeSettings &s) { s.tile[0].filter ^= 1; }, [](IntakeSettings &s) { s.tile[VP8HIP_MAX_TILES - 1].filter ^= 1; }};
}

IntakeSettings all_on() {      // 64x48: everything on at once
    IntakeSettings s = scaling(IntakeSettings{}, 96, 80, 60, 44, 1);
    s = deinterlace(orientation(window(transfer(format(s, VP8HOST_FORMAT_I010), VP8HOST_TRANSFER_HLG, 1000), 300, 150, 150, 2, 4), 1, 1), 2, 1);
    s.src_colour = 2;
    s.dn_level = 2;
    s.an_on = true;
    s.seg_mode = 2;
    s.seg_strength = 3;
    return s;
}

// (b) changing any one field alone makes == false
void equality() {
    const IntakeSettings a = all_on();
    expect(intake_valid(64, 48, a) == INTAKE_OK && a == canonical(a, 64, 48) && a == all_on(), "the all-on setting is valid, canonical and equal to itself");
    // 18 ints, three pitches of 32 bits and two bools, then the canvas: a count, three background values and VP8HIP_MAX_TILES tiles of
    // seven ints -- a field added to the struct and not to edits() changes the size
    static_assert(sizeof(IntakeSettings) == (23 + 4 + 7 * VP8HIP_MAX_TILES) * 4, "a new field: add it to operator== and to edits()");
    const auto e = edits();
    expect(e.size() == 23 + 4 + 7 + 1, "one edit per field (of the tiles: the first one's seven and the last one's last)");
    for (size_t k = 0; k < e.size(); ++k) {
        IntakeSettings b = a;
        e[k](b);
        expect(!(a == b) && !(b == a), "a field changed alone", (int)k);
    }
}

// (c) a stage switched off leaves nothing behind: equal to a setting that never had it on
void canonical_form() {
    const int W = 64, H = 48;
    const IntakeSettings never;
    IntakeSettings s = canonical(deinterlace(never, 1, 1), W, H);
    expect(canonical(deinterlace(s, 0, 1), W, H) == never, "deinterlace(1, 1) then (0, 1)");
    expect(canonical(deinterlace(deinterlace(never, 1, 0), 0, 1), W, H) == canonical(deinterlace(never, 0, 0), W, H), "deinterlace(1, 0) then (0, 1): the batch that was refused");
    s = transfer(never, VP8HOST_TRANSFER_PQ, 4000);
    s.src_transfer = 0;
    expect(canonical(s, W, H) == never, "the transfer off, a peak left");
    s = window(never, 80, 40, 40, 2, 2);
    s.win_on = false;
    expect(canonical(s, W, H) == never, "the window off, pitches and origin left");
    s = scaling(never, 128, 96, 64, 48, 1);
    s.in_w = s.in_h = 0;
    expect(canonical(s, W, H) == never, "the scaler off, its filter and a source size equal to the coded size left");
    s = never;
    s.seg_mode = 2; s.seg_strength = 3;
    s.seg_mode = 1;
    IntakeSettings one = never;
    one.seg_mode = 1;
    expect(canonical(s, W, H) == one, "segment mode 2 then 1, a strength left");
    expect(canonical(size(never, W, H), W, H) == never && !(canonical(size(never, W, H - 2), W, H) == never), "a source size equal to the coded size is none");
    expect(canonical(all_on(), W, H) == all_on(), "nothing of a switch that is on is touched");
}

// (d) needs_device_planes: true exactly when one of the six terms is
void device_planes() {
    for (int k = 0; k < 64; ++k) {
        IntakeSettings s;
        if (k & 1) s.src_fmt = VP8HOST_FORMAT_NV12;
        if (k & 2) s.di_mode = 1;
        if (k & 4) { s.in_w = 128; s.in_h = 96; }
        if (k & 8) s.win_on = true;
        if (k & 16) s.or_turns = 2;
        if (k & 32) s.or_mirror = 1;
        s.src_w = 60; s.src_colour = 1; s.dn_level = 3; s.an_on = true; s.seg_mode = 2; s.seg_strength = 1;      // (none of these is a term)
        expect(needs_device_planes(s) == (k != 0), "needs_device_planes", k);
    }
}

// (e) the size helpers at an odd turn
void sizes() {
    const int W = 64, H = 48;
    int w, h;
    size_t nb[3];
    IntakeSettings s = orientation(size(IntakeSettings{}, 60, 40), 1, 0);
    picture_size(s, W, H, &w, &h);
    expect(w == 60 && h == 40, "picture_size is the upright picture");
    upright_size(s, W, H, &w, &h);
    expect(w == 60 && h == 40, "upright_size without a scaler");
    incoming_size(s, W, H, &w, &h);
    expect(w == 40 && h == 60, "incoming_size: traded under one turn");
    incoming_bytes(s, W, H, nb);
    expect(nb[0] == 2400 && nb[1] == 600 && nb[2] == 600, "incoming_bytes, I420");
    s = orientation(scaling(s, 120, 90, 60, 40, 0), 3, 1);
    picture_size(s, W, H, &w, &h);
    expect(w == 60 && h == 40, "picture_size under a scaler");
    upright_size(s, W, H, &w, &h);
    expect(w == 120 && h == 90, "upright_size: the scaler's incoming size");
    incoming_size(s, W, H, &w, &h);
    expect(w == 90 && h == 120, "incoming_size: traded under three turns");
    incoming_bytes(format(s, VP8HOST_FORMAT_NV12), W, H, nb);
    expect(nb[0] == 10800 && nb[1] == 5400 && nb[2] == 0, "incoming_bytes, NV12");
    incoming_size(orientation(s, 2, 1), W, H, &w, &h);
    expect(w == 120 && h == 90, "incoming_size under two turns");
    incoming_size(IntakeSettings{}, W, H, &w, &h);
    expect(w == 64 && h == 48, "nothing set: the coded size");
    size_t off[3];
    int32_t rb[3], rows[3];
    expect(window_rule(orientation(window(size(IntakeSettings{}, 60, 40), 50, 25, 25, 2, 2), 1, 0), W, H, off, rb, rows) == 0 && rb[0] == 40 && rows[0] == 60 && off[0] == 102 && off[1] == 26,
           "window_rule at the raw size");
}

}  // namespace

int main() {
    verdicts();
    equality();
    canonical_form();
    device_planes();
    sizes();
    if (failures) return 1;
    printf("clean\n");
    return 0;
}
