// temporal_sanitize.cpp -- the temporal-layer rule (vp8host_temporal_step) and the host first-partition coder (vp8bs_encode_header) with the
// header values of a layered frame (is_golden = 2: GOLDEN only, 3: nothing) under the host sanitizers.  Every input of the coder -- segment
// data, segment ids, non-zero counts, reference frames, partitioning, vectors, probabilities -- is a heap block of exactly its size, and the
// output is a heap block of exactly the size the coder said it needed: a read outside an input or a write past the output is a heap
// overflow.  The frames differ in nothing but is_golden -- two header bools at the most -- so the first partitions differ by a byte at
// the most, and the output one byte too small must be refused, not overrun.  The rule: every argument it takes, and every refusal.  No GPU, no library: linked with
// vp8_host.cpp and vp8_bitstream.cpp alone.
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include scripts/native/temporal_sanitize.cpp \
//       vp8oclenc_amd/csrc/vp8_host.cpp vp8oclenc_amd/csrc/vp8_bitstream.cpp -o temporal_sanitize && ./temporal_sanitize
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "vp8hip_bitstream.h"
#include "vp8hip_host.h"

template <class T>
static std::unique_ptr<T[]> block(size_t n) { return std::unique_ptr<T[]>(new T[n]); }

int main() {
    unsigned seed = 7;
    auto next = [&] { seed = seed * 1664525u + 1013904223u; return seed >> 8; };
    long checked = 0;
    // ---- the rule ----
    for (int layers = 1; layers <= 3; ++layers)
        for (int p = 0; p <= 64; ++p)
            for (int mask = 0; mask <= 3; ++mask) {
                std::unique_ptr<vp8host_temporal> t(new vp8host_temporal);
                if (vp8host_temporal_step(layers, p, mask, t.get()) != 0) { fprintf(stderr, "refused: %d %d %d\n", layers, p, mask); return 1; }
                if (t->temporal_id < 0 || t->temporal_id >= layers || t->refresh < VP8HOST_REFRESH_LAST || t->refresh > VP8HOST_REFRESH_ALL ||
                    (t->use_golden && !(mask & 1)) || (t->temporal_id == 0) != (t->refresh == VP8HOST_REFRESH_LAST || t->refresh == VP8HOST_REFRESH_ALL)) {
                    fprintf(stderr, "the rule: %d %d %d -> %d %d %d %d\n", layers, p, mask, t->temporal_id, t->use_golden, t->refresh, t->layer_sync);
                    return 1;
                }
                ++checked;
            }
    {
        vp8host_temporal t{9, 9, 9, 9};
        const int bad[][2] = {{0, 0}, {4, 0}, {-1, 3}, {2, -1}, {3, -5}};
        for (const auto &b : bad)
            if (vp8host_temporal_step(b[0], b[1], 3, &t) != -1 || t.temporal_id != 9) { fprintf(stderr, "not refused: %d %d\n", b[0], b[1]); return 1; }
        if (vp8host_temporal_step(2, 1, 3, nullptr) != -1) { fprintf(stderr, "a null pointer was not refused\n"); return 1; }
    }
    // ---- the header coder ----
    const int sizes[][2] = {{1, 1}, {4, 3}, {6, 4}, {11, 2}};
    for (const auto &sz : sizes)
        for (int with_intra = 0; with_intra < 2; ++with_intra) {
            const int mbw = sz[0], mbh = sz[1], mbs = mbw * mbh;
            auto sd = block<int32_t>(44);
            auto seg = block<int32_t>(mbs), nz = block<int32_t>(mbs), ref = block<int32_t>(mbs), parts = block<int32_t>(mbs), inter = block<int32_t>(mbs);
            auto modes = block<int32_t>((size_t)mbs * 16);
            auto vec = block<int16_t>((size_t)mbs * 8);
            auto probs = block<uint32_t>(VP8BS_NUM_COEFF_PROBS), denom = block<uint32_t>(VP8BS_NUM_COEFF_PROBS);
            for (int i = 0; i < 44; ++i) sd[i] = 0;
            for (int s = 0; s < 4; ++s) { sd[s * 11 + 0] = 20 + 10 * s; sd[s * 11 + 6] = 5 + s; }
            int replaced = 0;
            for (int i = 0; i < mbs; ++i) {
                seg[i] = next() & 3;
                nz[i] = (next() & 3) ? (int)(next() % 300) : 0;
                ref[i] = next() % 3 == 0 ? 1 : 0;      // LAST and GOLDEN, as a layered frame uses them
                parts[i] = next() & 1;
                inter[i] = with_intra ? (next() % 5 != 0) : 1;
                replaced += !inter[i];
                for (int k = 0; k < 8; ++k) vec[(size_t)i * 8 + k] = (int16_t)((int)(next() % 61) - 30);
                if (!parts[i]) for (int k = 2; k < 8; ++k) vec[(size_t)i * 8 + k] = vec[(size_t)i * 8 + (k & 1)];
                for (int k = 0; k < 16; ++k) modes[(size_t)i * 16 + k] = next() % 10;
            }
            for (int i = 0; i < VP8BS_NUM_COEFF_PROBS; ++i) { probs[i] = 1 + next() % 255; denom[i] = (next() & 1) ? 2 + next() % 900 : 0; }
            vp8bs_default_probs(probs.get(), denom.get());
            vp8bs_frame f{};
            f.width = mbw * 16; f.height = mbh * 16; f.mb_width = mbw; f.mb_height = mbh;
            f.loop_filter_sharpness = 3; f.partitions_log2 = 1;
            f.skip_prob = vp8host_skip_prob(nz.get(), mbs);
            f.replaced = with_intra ? replaced : 0;
            f.segments = sd.get(); f.MB_segment_id = seg.get(); f.MB_non_zero_coeffs = nz.get(); f.MB_reference_frame = ref.get();
            f.MB_parts = parts.get(); f.MB_vectors = vec.get(); f.is_inter_mb = with_intra ? inter.get() : nullptr; f.modes = with_intra ? modes.get() : nullptr;
            f.new_probs = probs.get(); f.new_probs_denom = denom.get();
            size_t want = 0;
            for (int is_golden = 0; is_golden <= 3; ++is_golden) {
                if (is_golden == 1) continue;      // (an inter frame that refreshes GOLDEN and LAST: not a value the driver gives)
                f.is_golden = is_golden;
                std::vector<uint8_t> big((size_t)mbs * 400 + 16384);
                const size_t n = vp8bs_encode_header(&f, big.data(), big.size(), nullptr);
                if (!n || n == (size_t)-1) { fprintf(stderr, "%dx%d is_golden %d: no header\n", mbw, mbh, is_golden); return 1; }
                if (!want) want = n;
                if (n + 1 < want || n > want + 1) { fprintf(stderr, "%dx%d is_golden %d: %zu bytes, %zu with is_golden 0\n", mbw, mbh, is_golden, n, want); return 1; }
                if (!(big[0] & 0x10) || (big[0] & 1) != 1) { fprintf(stderr, "is_golden %d: not a shown inter frame\n", is_golden); return 1; }
                auto exact = block<uint8_t>(n);      // exactly what it needs: the same bytes ...
                if (vp8bs_encode_header(&f, exact.get(), n, nullptr) != n || memcmp(exact.get(), big.data(), n)) {
                    fprintf(stderr, "%dx%d is_golden %d: the exactly-sized buffer differs\n", mbw, mbh, is_golden);
                    return 1;
                }
                auto tight = block<uint8_t>(n - 1);  // ... and one byte less is refused, not overrun
                if (vp8bs_encode_header(&f, tight.get(), n - 1, nullptr) != 0) { fprintf(stderr, "is_golden %d: a short buffer was not refused\n", is_golden); return 1; }
                ++checked;
            }
        }
    printf("clean (%ld)\n", checked);
    return 0;
}
