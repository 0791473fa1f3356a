// driver_rule_check.cpp -- the driver's refusal table (vp8oclenc_amd/csrc/driver_settings.h) from outside, for
// tests/test_driver_rule_cpu.py: every line of standard input is one candidate, the fields of DriverSettings in the order of FIELDS
// below, then the feature asked for and whether it is asked for (1) or dropped (0),
//     qi_min qi_max num_partitions loop_filter_type in_width in_height scale_filter check_ssim denoise deinterlace field format colour
//     transfer peak analysis seg_mode seg_strength device_params overlap_filter scene_detect quality_stats ssim_target scheduled_altref
//     window canvas arf tl_layers tl_next tl_flags ir_period in_batch hidden_shapes_refs shard overlays FEATURE on
// and every line of output its verdict: '.' (VP8HIP_OK), 'A' (VP8HIP_ERR_ARG) or 'S' (VP8HIP_ERR_STATE).  FEATURE '*' asks for all
// seven, in the order of the enum, and then drops all seven: fourteen letters.  With the argument "agree" the lines come in pairs
// (FEATURE and on are read and ignored) and the output says whether the two may share a batch: "same" or "differ".
// Pure host code: no GPU, no library.
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include scripts/native/driver_rule_check.cpp
//       -o driver_rule_check && ./driver_rule_check < candidates      (one command line)
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../vp8oclenc_amd/csrc/driver_settings.h"

using namespace vp8;

static const char *const FEATURES[] = {"ARF", "LAYERS", "INTRA_REFRESH", "CANVAS", "INTAKE_SETTER", "BATCH_MEMBER", "SCAN"};
constexpr int N_FIELDS = 35;

static void fill(DriverSettings &s, const long v[N_FIELDS]) {
    int k = 0;
    int *const ints[] = {&s.qi_min, &s.qi_max, &s.num_partitions, &s.loop_filter_type, &s.in_width, &s.in_height, &s.scale_filter};
    for (int *p : ints) *p = (int)v[k++];
    s.check_ssim = v[k++] != 0;
    int *const intake[] = {&s.denoise, &s.deinterlace, &s.field, &s.format, &s.colour, &s.transfer, &s.peak};
    for (int *p : intake) *p = (int)v[k++];
    s.analysis = v[k++] != 0;
    s.seg_mode = (int)v[k++];
    s.seg_strength = (int)v[k++];
    bool *const config[] = {&s.device_params, &s.overlap_filter, &s.scene_detect, &s.quality_stats, &s.ssim_target, &s.scheduled_altref, &s.window};
    for (bool *p : config) *p = v[k++] != 0;
    int *const set[] = {&s.canvas, &s.arf, &s.tl_layers, &s.tl_next, &s.tl_flags, &s.ir_period};
    for (int *p : set) *p = (int)v[k++];
    bool *const moving[] = {&s.in_batch, &s.hidden_shapes_refs, &s.shard, &s.overlays};
    for (bool *p : moving) *p = v[k++] != 0;
}

static char letter(int rc) { return rc == VP8HIP_OK ? '.' : (rc == VP8HIP_ERR_ARG ? 'A' : (rc == VP8HIP_ERR_STATE ? 'S' : '?')); }

// one line -> the settings, the feature (-1: all of them) and on; false: the line is no candidate
static bool parse(char *line, DriverSettings &s, int &feature, bool &on) {
    long v[N_FIELDS];
    char *p = line;
    for (int k = 0; k < N_FIELDS; ++k) {
        char *end;
        v[k] = strtol(p, &end, 10);
        if (end == p) return false;
        p = end;
    }
    fill(s, v);
    char name[32];
    int flag = 0;
    if (sscanf(p, " %31s %d", name, &flag) != 2) return false;
    on = flag != 0;
    feature = -2;
    if (!strcmp(name, "*")) feature = -1;
    for (int f = 0; f < 7; ++f)
        if (!strcmp(name, FEATURES[f])) feature = f;
    return feature != -2;
}

int main(int argc, char **argv) {
    const bool agree = argc > 1 && !strcmp(argv[1], "agree");
    char line[1024];
    DriverSettings s, first;
    bool have_first = false;
    while (fgets(line, sizeof line, stdin)) {
        int feature;
        bool on;
        s = DriverSettings{};
        if (!parse(line, s, feature, on)) {
            fprintf(stderr, "a line that is no candidate: %s", line);
            return 1;
        }
        if (agree) {
            if (have_first) {
                const BatchShared &a = first, &b = s;
                puts(a == b ? "same" : "differ");
            }
            first = s;
            have_first = !have_first;
        } else if (feature >= 0) {
            printf("%c\n", letter(refusal(s, (Feature)feature, on)));
        } else {
            char out[16];
            for (int f = 0; f < 7; ++f) {
                out[f] = letter(refusal(s, (Feature)f, true));
                out[7 + f] = letter(refusal(s, (Feature)f, false));
            }
            out[14] = '\n';
            fwrite(out, 1, 15, stdout);
        }
    }
    return have_first ? 1 : 0;      // (a pair that was never completed)
}
