// vp8_host.cpp -- host-side mirror of the reference's parameter producers and frame sequencing
// (include/vp8hip_host.h).  Plain C++, no HIP calls: usable (and tested) without a GPU.
#include "../../include/vp8hip_host.h"

#include <math.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <vector>

namespace {

// src/vp8enc.h:17-39 (same tables as the kernels use)
const int dc_q[128] = {
    4,   5,   6,   7,   8,   9,   10,  10,  11,  12,  13,  14,  15,  16,  17,  17,  18,  19,  20,  20,  21,  21,
    22,  22,  23,  23,  24,  25,  25,  26,  27,  28,  29,  30,  31,  32,  33,  34,  35,  36,  37,  37,  38,  39,
    40,  41,  42,  43,  44,  45,  46,  46,  47,  48,  49,  50,  51,  52,  53,  54,  55,  56,  57,  58,  59,  60,
    61,  62,  63,  64,  65,  66,  67,  68,  69,  70,  71,  72,  73,  74,  75,  76,  76,  77,  78,  79,  80,  81,
    82,  83,  84,  85,  86,  87,  88,  89,  91,  93,  95,  96,  98,  100, 101, 102, 104, 106, 108, 110, 112, 114,
    116, 118, 122, 124, 126, 128, 130, 132, 134, 136, 138, 140, 143, 145, 148, 151, 154, 157};

inline int clamp_qi(int q) { return q > 127 ? 127 : (q < 0 ? 0 : q); }

}  // namespace

extern "C" {

void vp8host_quantizer_ladders(int qi_min, int qi_max, int32_t lastqi[4], int32_t altrefqi[4]) {
    if (qi_max < qi_min) {  // init.h:1585-1592
        const int t = qi_max;
        qi_max = qi_min;
        qi_min = t;
    }
    lastqi[0] = (qi_max + qi_min * 3 + 2) / 4;  // init.h:1593-1596
    lastqi[1] = (qi_max + qi_min + 1) / 2;
    lastqi[2] = (qi_max * 3 + qi_min + 2) / 4;
    lastqi[3] = qi_max;
    altrefqi[0] = lastqi[0] / 4;  // init.h:1598-1603
    altrefqi[1] = lastqi[1] / 3;
    altrefqi[2] = lastqi[2] / 3;
    altrefqi[3] = lastqi[3] / 2;
    if (altrefqi[0] < qi_min) altrefqi[0] = qi_min;
}

void vp8host_loopfilter_strength(const uint8_t *y, int width, int height, int32_t *reductor, int32_t *sharpness) {
    // vp8enc.cpp:96-127.  The reference's accumulators are `int`; the second one overflows on large noisy
    // frames.  They are kept modulo 2^32 here -- what that overflow does on every compiler the reference was
    // built with, and order-independent, so the device reduction (kernels_rc.hip) can match it.
    const int n = width * height;
    uint32_t sum = 0;
    for (int i = 0; i < n; ++i) sum += y[i];
    int avg = (int32_t)sum;
    avg += n / 2;
    avg /= n;
    *reductor = (avg * 5 / 255) + 3;
    uint32_t acc = 0;
    for (int i = 1; i < height - 1; ++i)
        for (int j = 1; j < width - 1; ++j) {
            const int p = i * width + j;
            int a = y[p - width - 1] + y[p - width] + y[p - width + 1] + y[p - 1] + y[p + 1] + y[p + width - 1] +
                    y[p + width] + y[p + width + 1];
            a /= 8;
            acc += (uint32_t)((y[p] - a) * (y[p] - a));
        }
    int div = (int32_t)acc;
    div += (height - 1) * (width - 1) / 2;
    div /= (height - 1) * (width - 1);
    int sh = div / 8;
    *sharpness = sh > 7 ? 7 : sh;
}

// OpenYUV420FileAndParseHeader, init.h:1610-1737, as a walk over a buffer: `next` stands for its fread of one char
int vp8host_y4m_parse_header(const uint8_t *data, size_t size, int32_t *width, int32_t *height, int32_t *framerate, size_t *first_frame_offset) {
    if (!data || !width || !height || !framerate || !first_frame_offset) return -1;
    static const char magic[] = "YUV4MPEG2 ";
    size_t j = 0;
    int ch = 0;
    auto next = [&]() -> bool {
        if (j >= size) return false;
        ch = data[j++];
        return true;
    };
    // The reference accumulates whatever bytes follow a tag (ch - 0x30, no digit check) in an int; here the same arithmetic
    // modulo 2^32 (what its overflow does, without the undefined behaviour), and a size outside the format's 14 bits is
    // refused at the end -- the one deviation: the reference would go on with it.
    auto digit = [&](int &acc) -> bool {
        acc = (int)((uint32_t)acc * 10u + (uint32_t)(ch - 0x30));
        return true;
    };
    int w = 0, h = 0, fps = 0;
    for (int i = 0; i < 10; ++i) {
        if (!next() || ch != magic[i]) return -1;
    }
    for (int i = 0; i < 3; ++i) {                    // three tags, whichever of W / H / F come first (:1634-1690)
        while (ch != 'W' && ch != 'H' && ch != 'F')
            if (!next()) return -1;
        if (ch == 'W') {
            for (;;) {
                if (!next()) return -1;
                if (ch == 0x20) break;
                if (!digit(w)) return -1;
            }
        } else if (ch == 'H') {
            for (;;) {
                if (!next()) return -1;
                if (ch == 0x20) break;
                if (!digit(h)) return -1;
            }
        } else {
            int num = 0, denom = 0;
            for (;;) {
                if (!next()) return -1;
                if (ch == ':') break;
                if (!digit(num)) return -1;
            }
            for (;;) {
                if (!next()) return -1;
                if (ch == 0x20) break;
                if (!digit(denom)) return -1;
            }
            if (denom == 0) return -1;               // the reference divides by it (:1688)
            fps = (num + denom / 2) / denom;
        }
    }
    if (w + h == 0) return -1;
    if (w < 1 || h < 1 || w > 16383 || h > 16383) return -1;   // RFC 6386 section 9.1: 14 bits each
    for (;;) {                                       // the first "FRAME" followed by a line feed (:1696-1728)
        while (ch != 'F')
            if (!next()) return -1;
        if (!next()) return -1;
        if (ch != 'R') continue;
        if (!next()) return -1;
        if (ch != 'A') continue;
        if (!next()) return -1;
        if (ch != 'M') continue;
        if (!next()) return -1;
        if (ch != 'E') continue;
        if (!next()) return -1;
        if (ch != 0x0A) return -1;
        break;
    }
    *width = w;
    *height = h;
    *framerate = fps;
    *first_frame_offset = j;
    return 0;
}

int vp8host_y4m_frame_marker_ok(const uint8_t m[6]) { return m && m[0] == 'F' && m[4] == 'E'; }   // encIO.h:245

// the header line's C tag (include/vp8hip_host.h); the reference's parser above never looks at it
int vp8host_y4m_colourspace(const uint8_t *data, size_t size, int32_t *format) {
    if (!data || !format) return -1;
    static const char magic[] = "YUV4MPEG2";
    size_t end = 0;
    while (end < size && data[end] != 0x0A) ++end;
    if (end == size || end < 9 || memcmp(data, magic, 9) != 0 || (end > 9 && data[9] != 0x20)) return -1;
    static const struct { const char *tag; int format; } known[] = {
        {"C420", VP8HOST_FORMAT_I420}, {"C420jpeg", VP8HOST_FORMAT_I420}, {"C420mpeg2", VP8HOST_FORMAT_I420}, {"C420paldv", VP8HOST_FORMAT_I420},
        {"C422", VP8HOST_FORMAT_I422}, {"C444", VP8HOST_FORMAT_I444}, {"C420p10", VP8HOST_FORMAT_I010}, {"C422p10", VP8HOST_FORMAT_I210},
        {"C444p10", VP8HOST_FORMAT_I410}};
    for (size_t a = 9; a < end;) {
        while (a < end && data[a] == 0x20) ++a;
        size_t b = a;
        while (b < end && data[b] != 0x20) ++b;
        if (b > a && data[a] == 'C') {
            for (const auto &k : known)
                if (strlen(k.tag) == b - a && memcmp(k.tag, data + a, b - a) == 0) {
                    *format = k.format;
                    return 0;
                }
            return -1;
        }
        a = b;
    }
    *format = VP8HOST_FORMAT_I420;
    return 0;
}

// the header line's I tag, read as the C tag is
int vp8host_y4m_interlace(const uint8_t *data, size_t size, int32_t *field_order) {
    if (!data || !field_order) return -1;
    static const char magic[] = "YUV4MPEG2";
    size_t end = 0;
    while (end < size && data[end] != 0x0A) ++end;
    if (end == size || end < 9 || memcmp(data, magic, 9) != 0 || (end > 9 && data[9] != 0x20)) return -1;
    for (size_t a = 9; a < end;) {
        while (a < end && data[a] == 0x20) ++a;
        size_t b = a;
        while (b < end && data[b] != 0x20) ++b;
        if (b > a && data[a] == 'I') {
            if (b - a != 2) return -1;
            switch (data[a + 1]) {
                case 'p': case '?': *field_order = VP8HOST_FIELDS_PROGRESSIVE; return 0;
                case 't': *field_order = VP8HOST_FIELDS_TOP_FIRST; return 0;
                case 'b': *field_order = VP8HOST_FIELDS_BOTTOM_FIRST; return 0;
                default: return -1;      // Im: mixed
            }
        }
        a = b;
    }
    *field_order = VP8HOST_FIELDS_PROGRESSIVE;
    return 0;
}

namespace {

// what a format is made of: two planes (interleaved chroma) or three, chroma subsampled horizontally / vertically, depth, and
// where a 16-bit word keeps its ten bits
struct SourceLayout { bool nv; int sub_x, sub_y, depth; bool top; };
bool source_layout(int format, SourceLayout *l) {
    switch (format) {
        case VP8HOST_FORMAT_I420: *l = {false, 1, 1, 8, false}; return true;
        case VP8HOST_FORMAT_NV12: *l = {true, 1, 1, 8, false}; return true;
        case VP8HOST_FORMAT_I422: *l = {false, 1, 0, 8, false}; return true;
        case VP8HOST_FORMAT_I444: *l = {false, 0, 0, 8, false}; return true;
        case VP8HOST_FORMAT_P010: *l = {true, 1, 1, 10, true}; return true;
        case VP8HOST_FORMAT_I010: *l = {false, 1, 1, 10, false}; return true;
        case VP8HOST_FORMAT_I210: *l = {false, 1, 0, 10, false}; return true;
        case VP8HOST_FORMAT_I410: *l = {false, 0, 0, 10, false}; return true;
        default: return false;
    }
}

// the colour matrices of BGRA / RGBA, include/vp8hip_host.h: offset, then the Y, U and V rows, each R, G, B
const int32_t colour_table[VP8HOST_COLOUR_COUNT][10] = {
    {16, 66, 129, 25, -38, -74, 112, 112, -94, -18},
    {16, 47, 157, 16, -26, -86, 112, 112, -102, -10},
    {0, 77, 150, 29, -43, -84, 127, 127, -106, -21},
    {0, 54, 183, 19, -29, -98, 127, 127, -116, -11},
};
bool packed_format(int format) { return format >= VP8HOST_FORMAT_PACKED_FIRST && format < VP8HOST_FORMAT_PACKED_END; }

}  // namespace

int vp8host_colour_coefficients(int matrix, int32_t c[9], int32_t *y_offset) {
    if (matrix < 0 || matrix >= VP8HOST_COLOUR_COUNT || !c || !y_offset) return -1;
    *y_offset = colour_table[matrix][0];
    for (int i = 0; i < 9; ++i) c[i] = colour_table[matrix][1 + i];
    return 0;
}

int vp8host_source_plane_bytes(int format, int width, int height, size_t bytes[3]) {
    SourceLayout l;
    if (bytes && packed_format(format) && width > 0 && height > 0 && !(width & 1) && !(height & 1)) {
        const bool rgb = format == VP8HOST_FORMAT_BGRA || format == VP8HOST_FORMAT_RGBA;
        bytes[0] = (size_t)width * (size_t)height * (rgb ? 4 : 2);
        bytes[1] = bytes[2] = 0;
        return 0;
    }
    if (!bytes || !source_layout(format, &l) || width <= 0 || height <= 0 || (width & 1) || (height & 1)) return -1;
    const size_t b = l.depth > 8 ? 2 : 1;
    const size_t chroma = (size_t)(width >> l.sub_x) * (size_t)(height >> l.sub_y) * b;
    bytes[0] = (size_t)width * (size_t)height * b;
    bytes[1] = l.nv ? 2 * chroma : chroma;
    bytes[2] = l.nv ? 0 : chroma;
    return 0;
}

// the packed family: one plane; YUY2 / UYVY by the I422 rule on the samples they carry, BGRA / RGBA through the matrix
static int convert_packed(int format, int matrix, int width, int height, const uint8_t *p, uint8_t *y, uint8_t *u, uint8_t *v) {
    const int cw = width / 2, ch = height / 2;
    if (format == VP8HOST_FORMAT_YUY2 || format == VP8HOST_FORMAT_UYVY) {
        const int ly = format == VP8HOST_FORMAT_YUY2 ? 0 : 1, lu = format == VP8HOST_FORMAT_YUY2 ? 1 : 0;      // V sits two bytes behind U
        for (int r = 0; r < height; ++r)
            for (int x = 0; x < width; ++x) y[(size_t)r * width + x] = p[((size_t)r * width + x) * 2 + ly];
        for (int r = 0; r < ch; ++r)
            for (int x = 0; x < cw; ++x) {
                const uint8_t *a = p + ((size_t)(2 * r) * cw + x) * 4, *b = a + (size_t)cw * 4;
                u[(size_t)r * cw + x] = (uint8_t)((a[lu] + b[lu] + 1) >> 1);
                v[(size_t)r * cw + x] = (uint8_t)((a[lu + 2] + b[lu + 2] + 1) >> 1);
            }
        return 0;
    }
    const int32_t *m = colour_table[matrix];
    const int ir = format == VP8HOST_FORMAT_BGRA ? 2 : 0, ib = 2 - ir;
    for (int r = 0; r < height; ++r)
        for (int x = 0; x < width; ++x) {
            const uint8_t *q = p + ((size_t)r * width + x) * 4;
            y[(size_t)r * width + x] = (uint8_t)(m[0] + ((m[1] * q[ir] + m[2] * q[1] + m[3] * q[ib] + 128) >> 8));
        }
    for (int r = 0; r < ch; ++r)
        for (int x = 0; x < cw; ++x) {
            int32_t su = 0, sv = 0;
            for (int j = 0; j < 2; ++j)
                for (int i = 0; i < 2; ++i) {
                    const uint8_t *q = p + ((size_t)(2 * r + j) * width + (2 * x + i)) * 4;
                    su += m[4] * q[ir] + m[5] * q[1] + m[6] * q[ib];
                    sv += m[7] * q[ir] + m[8] * q[1] + m[9] * q[ib];
                }
            u[(size_t)r * cw + x] = (uint8_t)((su + 131072 + 512) >> 10);
            v[(size_t)r * cw + x] = (uint8_t)((sv + 131072 + 512) >> 10);
        }
    return 0;
}

int vp8host_convert_frame_colour(int format, int matrix, int width, int height, const uint8_t *p0, const uint8_t *p1, const uint8_t *p2,
                                 uint8_t *y, uint8_t *u, uint8_t *v) {
    if (matrix < 0 || matrix >= VP8HOST_COLOUR_COUNT) return -1;
    if (!packed_format(format)) return vp8host_convert_frame(format, width, height, p0, p1, p2, y, u, v);
    size_t bytes[3];
    if (vp8host_source_plane_bytes(format, width, height, bytes) != 0 || !p0 || !y || !u || !v) return -1;
    return convert_packed(format, matrix, width, height, p0, y, u, v);
}

// OVERLAYS, include/vp8hip_host.h: one layer composed onto tight I420 of the picture size, in place
int vp8host_overlay_frame(int format, int matrix, int lw, int lh, int pitch, const uint8_t *pixels, int x, int y, int opacity, int pw, int ph,
                          uint8_t *yp, uint8_t *up, uint8_t *vp) {
    if ((format != VP8HOST_FORMAT_BGRA && format != VP8HOST_FORMAT_RGBA) || matrix < 0 || matrix >= VP8HOST_COLOUR_COUNT || lw < 1 || lh < 1 ||
        lw > VP8HOST_OVERLAY_MAX_SIZE || lh > VP8HOST_OVERLAY_MAX_SIZE || pitch < 4 * lw || x < -VP8HOST_OVERLAY_MAX_POS || x > VP8HOST_OVERLAY_MAX_POS ||
        y < -VP8HOST_OVERLAY_MAX_POS || y > VP8HOST_OVERLAY_MAX_POS || opacity < 0 || opacity > 255 || pw <= 0 || ph <= 0 || (pw & 1) || (ph & 1) || !pixels ||
        !yp || !up || !vp)
        return -1;
    const int32_t *m = colour_table[matrix];
    const int ir = format == VP8HOST_FORMAT_BGRA ? 2 : 0, ib = 2 - ir;
    // the layer pixel at picture position (px, py), or nullptr where the layer has none
    auto at = [&](int px, int py) -> const uint8_t * {
        const int lx = px - x, ly = py - y;
        return lx >= 0 && lx < lw && ly >= 0 && ly < lh ? pixels + (size_t)ly * (size_t)pitch + (size_t)lx * 4 : nullptr;
    };
    const int x0 = x > 0 ? x : 0, y0 = y > 0 ? y : 0, x1 = x + lw < pw ? x + lw : pw, y1 = y + lh < ph ? y + lh : ph;
    for (int py = y0; py < y1; ++py)
        for (int px = x0; px < x1; ++px) {
            const uint8_t *q = at(px, py);
            const int32_t e = (q[3] * opacity + 127) / 255;
            const int32_t yo = m[0] + ((m[1] * q[ir] + m[2] * q[1] + m[3] * q[ib] + 128) >> 8);
            uint8_t *d = yp + (size_t)py * pw + px;
            *d = (uint8_t)((*d * (255 - e) + yo * e + 127) / 255);
        }
    const int cw = pw / 2;
    for (int cy = y0 >> 1; cy < (y1 + 1) >> 1; ++cy)
        for (int cx = x0 >> 1; cx < (x1 + 1) >> 1; ++cx) {
            int32_t E = 0, tu = 0, tv = 0;
            for (int j = 0; j < 2; ++j)
                for (int i = 0; i < 2; ++i) {
                    const uint8_t *q = at(2 * cx + i, 2 * cy + j);
                    if (!q) continue;
                    const int32_t e = (q[3] * opacity + 127) / 255;
                    E += e;
                    tu += e * (m[4] * q[ir] + m[5] * q[1] + m[6] * q[ib] + 32768);
                    tv += e * (m[7] * q[ir] + m[8] * q[1] + m[9] * q[ib] + 32768);
                }
            uint8_t *du = up + (size_t)cy * cw + cx, *dv = vp + (size_t)cy * cw + cx;
            *du = (uint8_t)(((*du * 256 * (1020 - E) + tu + 130560) >> 10) / 255);
            *dv = (uint8_t)(((*dv * 256 * (1020 - E) + tv + 130560) >> 10) / 255);
        }
    return 0;
}

int vp8host_convert_frame(int format, int width, int height, const uint8_t *p0, const uint8_t *p1, const uint8_t *p2,
                          uint8_t *y, uint8_t *u, uint8_t *v) {
    if (packed_format(format))return vp8host_convert_frame_colour(format, VP8HOST_COLOUR_BT601_LIMITED, width, height, p0, p1, p2, y, u, v);
    SourceLayout l;
    size_t bytes[3];
    if (vp8host_source_plane_bytes(format, width, height, bytes) != 0 || !source_layout(format, &l)) return -1;
    if (!p0 || !p1 || (!l.nv && !p2) || !y || !u || !v) return -1;
    // sample i of a plane, at the format's depth
    auto sample = [&](const uint8_t *p, size_t i) -> int {
        if (l.depth == 8) return p[i];
        const int word = p[2 * i] | (p[2 * i + 1] << 8);
        return l.top ? word >> 6 : word & 1023;
    };
    auto round_off = [](int S, int k) -> uint8_t {
        const int o = k ? (S + (1 << (k - 1))) >> k : S;
        return (uint8_t)(o > 255 ? 255 : o);
    };
    const int ky = l.depth - 8;
    for (size_t i = 0; i < (size_t)width * height; ++i) y[i] = round_off(sample(p0, i), ky);
    const int cw = width / 2, ch = height / 2;
    const int nx = 2 - l.sub_x, ny = 2 - l.sub_y;                  // source samples per output sample, across and down
    const int kc = l.depth - 8 + (nx == 2) + (ny == 2);
    const size_t pitch = (size_t)cw * nx;                          // samples (NV: pairs) per source chroma row
    for (int r = 0; r < ch; ++r)
        for (int x = 0; x < cw; ++x) {
            int su = 0, sv = 0;
            for (int j = 0; j < ny; ++j)
                for (int i = 0; i < nx; ++i) {
                    const size_t at = (size_t)(r * ny + j) * pitch + (size_t)(x * nx + i);
                    if (l.nv) { su += sample(p1, 2 * at); sv += sample(p1, 2 * at + 1); }
                    else { su += sample(p1, at); sv += sample(p2, at); }
                }
            u[(size_t)r * cw + x] = round_off(su, kc);
            v[(size_t)r * cw + x] = round_off(sv, kc);
        }
    return 0;
}

// ---- HDR sources made SDR: the tables and the rule of include/vp8hip_host.h ------------------------------------------------------------
int vp8host_tonemap_tables(int transfer, int peak, uint32_t lin[4096], uint32_t gain[4096], uint8_t lo[4096], uint8_t hi[4096]) {
    if ((transfer != VP8HOST_TRANSFER_PQ && transfer != VP8HOST_TRANSFER_HLG) || peak < VP8HOST_PEAK_MIN || peak > VP8HOST_PEAK_MAX ||
        !lin || !gain || !lo || !hi)
        return -1;
    const double P = peak, w = P / 203.0;
    const double m1 = 2610.0 / 16384.0, m2 = 128.0 * 2523.0 / 4096.0, c1 = 3424.0 / 4096.0, c2 = 32.0 * 2413.0 / 4096.0, c3 = 32.0 * 2392.0 / 4096.0;
    const double ha = 0.17883277, hb = 0.28466892, hc = 0.55991073, gamma = 1.2 + 0.42 * std::log10(P / 1000.0);
    int first = -1;
    for (int i = 0; i < 4096; ++i) {
        const double e = i / 4095.0;
        double s, D;
        if (transfer == VP8HOST_TRANSFER_PQ) {
            const double p = std::pow(e, 1.0 / m2);
            const double N = 10000.0 * std::pow(std::max(p - c1, 0.0) / (c2 - c3 * p), 1.0 / m1);
            D = std::min(N, P);
            s = D / P;
        } else {
            s = e <= 0.5 ? e * e / 3.0 : (std::exp((e - hc) / ha) + hb) / 12.0;
            D = P * std::pow(s, gamma);
        }
        const double x = D / 203.0, T = x * (1.0 + x / (w * w)) / (1.0 + x);
        lin[i] = (uint32_t)std::min(1048575.0, std::rint(1048576.0 * s));
        gain[i] = 0;
        if (lin[i] > 0) {
            gain[i] = (uint32_t)std::rint(65535.0 * 1048576.0 * T / (double)lin[i]);
            if (first < 0) first = i;
        }
    }
    for (int i = 0; i < first; ++i) gain[i] = gain[first];      // (black: lin is 0 there, the product too)
    for (int j = 0; j < 4096; ++j) {
        lo[j] = (uint8_t)std::rint(255.0 * std::pow(j / 65535.0, 1.0 / 2.4));
        hi[j] = (uint8_t)std::rint(255.0 * std::pow(std::min(16 * j + 8, 65535) / 65535.0, 1.0 / 2.4));
    }
    return 0;
}

int vp8host_tonemap_frame(int format, int transfer, int peak, int matrix, int width, int height, const uint8_t *p0, const uint8_t *p1,
                          const uint8_t *p2, uint8_t *y, uint8_t *u, uint8_t *v) {
    const bool nv = format == VP8HOST_FORMAT_P010;
    size_t bytes[3];
    if ((!nv && format != VP8HOST_FORMAT_I010) || matrix < 0 || matrix >= VP8HOST_COLOUR_COUNT ||
        vp8host_source_plane_bytes(format, width, height, bytes) != 0 || !p0 || !p1 || (!nv && !p2) || !y || !u || !v)
        return -1;
    std::vector<uint32_t> lin(4096), gain(4096);
    std::vector<uint8_t> lo(4096), hi(4096);
    if (vp8host_tonemap_tables(transfer, peak, lin.data(), gain.data(), lo.data(), hi.data()) != 0) return -1;
    auto sample = [&](const uint8_t *p, size_t i) -> int32_t {
        const int word = p[2 * i] | (p[2 * i + 1] << 8);
        return nv ? word >> 6 : word & 1023;
    };
    auto clamp12 = [](int32_t a) -> int32_t { return a < 0 ? 0 : (a > 4095 ? 4095 : a); };
    auto out8 = [&](int32_t sum, uint32_t g) -> int32_t {      // one component: primaries' row sum -> tone curve -> SDR transfer
        const int64_t t = sum >> 10 < 0 ? 0 : sum >> 10;
        const int64_t o = std::min<int64_t>(65535, (t * (int64_t)g + 524288) >> 20);
        return o < 4096 ? lo[(size_t)o] : hi[(size_t)(o >> 4)];
    };
    const int32_t *m = colour_table[matrix];
    const int cw = width / 2, ch = height / 2;
    for (int r = 0; r < ch; ++r)
        for (int x = 0; x < cw; ++x) {
            const size_t at = (size_t)r * cw + x;
            const int32_t cb = (nv ? sample(p1, 2 * at) : sample(p1, at)) - 512, cr = (nv ? sample(p1, 2 * at + 1) : sample(p2, at)) - 512;
            int32_t su = 0, sv = 0;
            for (int j = 0; j < 2; ++j)
                for (int i = 0; i < 2; ++i) {
                    const size_t px = (size_t)(2 * r + j) * width + (2 * x + i);
                    const int32_t yy = 38295 * (sample(p0, px) - 64) + 4096;
                    const int32_t R1 = clamp12((yy + 55209 * cr) >> 13), G1 = clamp12((yy - 6161 * cb - 21391 * cr) >> 13), B1 = clamp12((yy + 70440 * cb) >> 13);
                    const uint32_t g = gain[std::max(R1, std::max(G1, B1))];
                    const int32_t aR = (int32_t)lin[R1], aG = (int32_t)lin[G1], aB = (int32_t)lin[B1];
                    const int32_t R = out8(1701 * aR - 602 * aG - 75 * aB + 512, g), G = out8(-128 * aR + 1161 * aG - 9 * aB + 512, g),
                                  B = out8(-19 * aR - 103 * aG + 1146 * aB + 512, g);
                    y[px] = (uint8_t)(m[0] + ((m[1] * R + m[2] * G + m[3] * B + 128) >> 8));
                    su += m[4] * R + m[5] * G + m[6] * B;
                    sv += m[7] * R + m[8] * G + m[9] * B;
                }
            u[at] = (uint8_t)((su + 131072 + 512) >> 10);
            v[at] = (uint8_t)((sv + 131072 + 512) >> 10);
        }
    return 0;
}

int vp8host_scene_change(vp8host_scene_state *st, int Udiff, int Vdiff, int frame_number) {
    // vp8enc.cpp:285-310
    const int detect = (Udiff > 7) || (Vdiff > 7) || (Udiff + Vdiff > 10);
    const bool recent = (frame_number - st->last_key_detect) < 4;   // "workaround to exclude serial intra_frames"
    if (detect && recent) {
        st->last_key_detect = frame_number;
        st->holdover = 1;
        return 0;
    }
    if (detect) return 1;            // last_key_detect is set when the key frame is coded
    if (st->holdover && recent) return 0;
    if (st->holdover) {
        st->holdover = 0;
        return 1;
    }
    return 0;
}

void vp8host_prepare_segments_data(int is_key_frame, const int32_t refqi[4], int qi_min, int reductor, int sharpness,
                                   int update_filter, int shrpnss, int32_t sd[44]) {
    for (int i = 0; i < 44; ++i) sd[i] = 0;
    // segment 0 carries the deltas shared by all segments, vp8enc.cpp:133-148
    sd[1] = 15;                      // y_dc_idelta
    sd[2] = 0;                       // y2_dc_idelta
    sd[3] = 0;                       // y2_ac_idelta
    sd[4] = is_key_frame ? 0 : -15;  // uv_dc_idelta
    sd[5] = is_key_frame ? 0 : -15;  // uv_ac_idelta
    if (update_filter) {             // vp8enc.cpp:155-159
        reductor *= 2;
        sharpness = shrpnss;
    }
    for (int i = 0; i < 4; ++i) {
        int32_t *s = sd + 11 * i;
        s[0] = is_key_frame ? qi_min : refqi[i];  // y_ac_i, :164
        const int y_dc_q = dc_q[clamp_qi(s[0] + sd[1])];
        int lvl = y_dc_q / reductor;  // :187-189
        lvl = lvl > 63 ? 63 : (lvl < 0 ? 0 : lvl);
        s[6] = lvl;
        int il = lvl;  // :192-199
        if (sharpness) {
            il >>= sharpness > 4 ? 2 : 1;
            if (il > 9 - sharpness) il = 9 - sharpness;
        }
        if (!il) il = 1;
        s[9] = il;
        s[7] = ((lvl + 2) * 2) + il;  // mbedge_limit
        s[8] = (lvl * 2) + il;        // sub_bedge_limit
        s[10] = 0;                    // hev_threshold, :204-220
        if (is_key_frame) {
            if (lvl >= 40) s[10] = 2;
            else if (lvl >= 15) s[10] = 1;
        } else {
            if (lvl >= 40) s[10] = 3;
            else if (lvl >= 20) s[10] = 2;
            else if (lvl >= 15) s[10] = 1;
        }
    }
}

int vp8host_skip_prob(const int32_t *nz, int mb_count) {
    int p = 0;
    for (int i = 0; i < mb_count; ++i)
        if (nz[i] > 0) ++p;
    p *= 256;
    p /= mb_count;
    p = p > 254 ? 254 : p;
    return p < 2 ? 2 : p;
}

void vp8host_gop_init(vp8host_gop *g, int gop_size, int altref_range) {
    *g = vp8host_gop{};
    g->gop_size = gop_size;
    g->altref_range = altref_range;
    g->frames_until_key = 1;     // vp8enc.cpp:340-344
    g->frames_until_altref = 2;
    g->frame_number = 0;
    g->golden_frame_number = -1;
    g->altref_frame_number = -1;
}

void vp8host_gop_next(vp8host_gop *g) {  // vp8enc.cpp:364-374
    g->prev_is_key = g->current_is_key;
    g->prev_is_golden = g->current_is_golden;
    g->prev_is_altref = g->current_is_altref;
    --g->frames_until_key;
    --g->frames_until_altref;
    g->current_is_key = g->frames_until_key < 1;
    g->current_is_golden = g->current_is_key;
    g->current_is_altref = (g->frames_until_altref < 1) || g->current_is_key;
    g->frames_until_altref = ((g->frames_until_altref < 1) || g->current_is_key) ? g->altref_range : g->frames_until_altref;
    g->golden_frame_number = g->current_is_golden ? g->frame_number : g->golden_frame_number;
    g->altref_frame_number = g->current_is_altref ? g->frame_number : g->altref_frame_number;
}

void vp8host_gop_key_coded(vp8host_gop *g) {  // intra_part.h:1091-1098
    g->current_is_key = 1;
    g->frames_until_key = g->gop_size;
    g->frames_until_altref = g->altref_range;
    g->current_is_golden = 1;
    g->current_is_altref = 1;
    g->golden_frame_number = g->frame_number;
    g->altref_frame_number = g->frame_number;
}

void vp8host_gop_inter_flags(const vp8host_gop *g, int32_t *use_golden, int32_t *use_altref) {  // inter_part.h:103-104
    *use_golden = !g->prev_is_golden;
    *use_altref = (!g->prev_is_altref) && (g->altref_frame_number != g->golden_frame_number);
}

void vp8host_gop_frame_done(vp8host_gop *g) { ++g->frame_number; }

int vp8host_temporal_step(int layers, int p, int ref_mask, vp8host_temporal *out) {  // the rule: include/vp8hip_host.h
    if (!out || layers < 1 || layers > 3 || p < 0) return -1;
    vp8host_temporal t{0, 0, VP8HOST_REFRESH_LAST, 0};
    if (p == 0) {
        t.refresh = VP8HOST_REFRESH_ALL;
    } else if (layers == 2) {
        if (p % 2 == 1) t = vp8host_temporal{1, 0, VP8HOST_REFRESH_NONE, 1};
    } else if (layers == 3) {
        switch (p % 4) {
            case 1: t = vp8host_temporal{2, 0, VP8HOST_REFRESH_NONE, 1}; break;
            case 2: t = vp8host_temporal{1, 0, VP8HOST_REFRESH_GOLDEN, 1}; break;
            case 3: t = vp8host_temporal{2, ref_mask & 1, VP8HOST_REFRESH_NONE, !(ref_mask & 1)}; break;
            default: break;
        }
    }
    *out = t;
    return 0;
}

int vp8host_intra_refresh_forced(int period, int q, int r, int c) {  // the rule: include/vp8hip_host.h
    if (period < VP8HOST_INTRA_REFRESH_MIN || period > VP8HOST_INTRA_REFRESH_MAX || q < 0 || r < 0 || c < 0) return -1;
    return (int)(((long long)c + 2ll * r) % period == q % period);
}

int vp8host_intra_refresh_count(int mbw, int mbh, int period, int q) {
    if (period < VP8HOST_INTRA_REFRESH_MIN || period > VP8HOST_INTRA_REFRESH_MAX || q < 0 || mbw < 1 || mbh < 1) return -1;
    int n = 0;
    for (int r = 0; r < mbh; ++r) {
        const int first = (int)((((long long)q - 2ll * r) % period + period) % period);      // the row's first forced column
        if (first < mbw) n += (mbw - first + period - 1) / period;
    }
    return n;
}

int vp8host_scene_plan(const int32_t *udiff, const int32_t *vdiff, int nframes, int gop_size, uint8_t *is_key, uint8_t *by_scene) {
    if (!udiff || !vdiff || !is_key || nframes < 0 || gop_size < 1) return -1;
    vp8host_gop g;
    vp8host_scene_state sc{};
    vp8host_gop_init(&g, gop_size, 1);      // (the alt-ref period does not reach the key-frame counters)
    int keys = 0;
    for (int t = 0; t < nframes; ++t) {
        vp8host_gop_next(&g);
        bool key = g.current_is_key != 0, scene = false;
        if (!key && vp8host_scene_change(&sc, udiff[t], vdiff[t], g.frame_number)) key = scene = true;
        if (key) {
            sc.last_key_detect = g.frame_number;
            vp8host_gop_key_coded(&g);
            ++keys;
        }
        vp8host_gop_frame_done(&g);
        is_key[t] = key ? 1 : 0;
        if (by_scene) by_scene[t] = scene ? 1 : 0;
    }
    return keys;
}

// The two filter tables of the device's scaler (include/vp8hip_host.h): integer-only for the area filter, `double` for Lanczos-3.
int vp8host_scale_taps(int n_in, int n_out, int kind, int32_t *n_taps, int32_t *start, int16_t *coef) {
    constexpr int MAXT = VP8HOST_SCALE_MAX_TAPS;
    if (!n_taps || !start || !coef || n_in < 1 || n_out < 1 || n_out > n_in || n_in > 16384 || (kind != 0 && kind != 1)) return -1;
    *n_taps = 0;
    const double r = (double)n_in / n_out, pi = 3.14159265358979323846;
    // first and last source sample output i touches
    auto span = [&](int i, int *first, int *last) {
        if (kind == 0) {
            *first = (int)((int64_t)i * n_in / n_out);
            *last = (int)((((int64_t)i + 1) * n_in - 1) / n_out);
        } else {
            const double c = (i + 0.5) * r - 0.5;
            *first = (int)ceil(c - 3.0 * r);
            *last = (int)floor(c + 3.0 * r);
        }
    };
    int n = 0;
    for (int i = 0; i < n_out; ++i) {
        int a, b;
        span(i, &a, &b);
        if (b - a + 1 > n) n = b - a + 1;
    }
    if (n > MAXT || n > n_in) return -1;
    for (int i = 0; i < n_out; ++i) {
        int a, b;
        span(i, &a, &b);
        const int cnt = b - a + 1;
        int32_t w[MAXT];
        if (kind == 0) {
            int64_t prev = 0;
            for (int k = 0; k < cnt; ++k) {
                int64_t cum = ((int64_t)a + k + 1) * n_out - (int64_t)i * n_in;      // of output i's interval, what lies left of this sample's right end
                if (cum > n_in) cum = n_in;
                const int64_t q = 4096 * cum / n_in;
                w[k] = (int32_t)(q - prev);
                prev = q;
            }
        } else {
            const double c = (i + 0.5) * r - 0.5;
            double f[MAXT], sum = 0.0;
            for (int k = 0; k < cnt; ++k) {
                const double x = (a + k - c) / r;
                double v = 0.0;
                if (fabs(x) < 3.0) v = x == 0.0 ? 1.0 : (sin(pi * x) / (pi * x)) * (sin(pi * x / 3.0) / (pi * x / 3.0));
                f[k] = v;
                sum += v;
            }
            for (int k = 0; k < cnt; ++k) w[k] = (int32_t)floor(4096.0 * f[k] / sum + 0.5);
        }
        // taps outside the plane fold onto the edge sample; the row then starts where all n taps are inside
        int s = a < 0 ? 0 : a;
        if (s > n_in - n) s = n_in - n;
        int32_t row[MAXT] = {0};
        for (int k = 0; k < cnt; ++k) {
            int j = a + k;
            j = j < 0 ? 0 : (j > n_in - 1 ? n_in - 1 : j);
            row[j - s] += w[k];
        }
        if (kind == 1) {      // the rounding's remainder goes to the largest tap
            int total = 0, big = 0;
            for (int k = 0; k < n; ++k) {
                total += row[k];
                if (row[k] > row[big]) big = k;
            }
            row[big] += 4096 - total;
        }
        int mag = 0;
        for (int k = 0; k < n; ++k) mag += row[k] < 0 ? -row[k] : row[k];
        if (mag > 8000) return -1;      // 255 * 8000 / 64 = 31 875: the horizontal pass stays inside int16
        start[i] = s;
        for (int k = 0; k < MAXT; ++k) coef[(size_t)i * MAXT + k] = (int16_t)(k < n ? row[k] : 0);
    }
    *n_taps = n;
    return 0;
}

}  // extern "C"

// A canvas of scaled video tiles in plain C++ (include/vp8hip_host.h, "CANVAS").
namespace {

struct TapTable { int32_t n = 0; std::vector<int32_t> start; std::vector<int16_t> coef; };

bool tap_table(int n_in, int n_out, int kind, TapTable *t) {
    if (n_out < 1) return false;
    t->start.resize((size_t)n_out);
    t->coef.resize((size_t)n_out * VP8HOST_SCALE_MAX_TAPS);
    return vp8host_scale_taps(n_in, n_out, kind, &t->n, t->start.data(), t->coef.data()) == 0;
}

// one plane of one tile through the two passes, into the rectangle of `out` (rows `stride` apart) whose first sample is `out`
void compose_plane(const uint8_t *src, int pitch, int in_h, const TapTable &tx, const TapTable &ty, int w, int h, uint8_t *out, int stride) {
    std::vector<int16_t> t((size_t)in_h * w);
    for (int r = 0; r < in_h; ++r)
        for (int i = 0; i < w; ++i) {
            const uint8_t *s = src + (size_t)r * pitch + tx.start[i];
            const int16_t *c = &tx.coef[(size_t)i * VP8HOST_SCALE_MAX_TAPS];
            int acc = 32;
            for (int k = 0; k < tx.n; ++k) acc += (int)c[k] * (int)s[k];
            t[(size_t)r * w + i] = (int16_t)(acc >> 6);
        }
    for (int j = 0; j < h; ++j)
        for (int i = 0; i < w; ++i) {
            const int16_t *c = &ty.coef[(size_t)j * VP8HOST_SCALE_MAX_TAPS];
            int acc = 1 << 17;
            for (int k = 0; k < ty.n; ++k) acc += (int)c[k] * (int)t[(size_t)(ty.start[j] + k) * w + i];
            acc >>= 18;
            out[(size_t)j * stride + i] = (uint8_t)(acc < 0 ? 0 : (acc > 255 ? 255 : acc));
        }
}

}  // namespace

extern "C" {

int vp8host_tile_valid(int pw, int ph, const vp8hip_tile *t) {
    if (!t || pw < 2 || ph < 2 || ((pw | ph) & 1)) return 0;
    if ((t->in_w | t->in_h | t->x | t->y | t->w | t->h) & 1) return 0;
    if (t->w < 2 || t->h < 2 || t->x < 0 || t->y < 0 || t->w > pw || t->h > ph || t->x > pw - t->w || t->y > ph - t->h) return 0;
    if (t->in_w < t->w || t->in_h < t->h || t->in_w > 16384 || t->in_h > 16384 || (t->filter != 0 && t->filter != 1)) return 0;
    TapTable tab;
    return tap_table(t->in_w, t->w, t->filter, &tab) && tap_table(t->in_h, t->h, t->filter, &tab) &&
           tap_table(t->in_w / 2, t->w / 2, t->filter, &tab) && tap_table(t->in_h / 2, t->h / 2, t->filter, &tab);
}

int vp8host_compose_frame(int pw, int ph, const vp8hip_tile *tiles, int n, int bg_y, int bg_u, int bg_v, const vp8hip_tile_planes *src,
                          uint8_t *out_y, uint8_t *out_u, uint8_t *out_v) {
    if (!out_y || !out_u || !out_v || pw < 2 || ph < 2 || ((pw | ph) & 1) || n < 0 || n > VP8HIP_MAX_TILES || (n && (!tiles || !src))) return -1;
    if (((bg_y | bg_u | bg_v) & ~255) != 0) return -1;
    for (int k = 0; k < n; ++k) {      // everything that can be refused, before anything is written
        if (!vp8host_tile_valid(pw, ph, &tiles[k])) return -1;
        const vp8hip_tile_planes &p = src[k];
        if (!p.y) continue;
        if (!p.u || !p.v) return -1;
        if ((p.pitch_y && p.pitch_y < tiles[k].in_w) || (p.pitch_u && p.pitch_u < tiles[k].in_w / 2) || (p.pitch_v && p.pitch_v < tiles[k].in_w / 2)) return -1;
    }
    const int cw = pw / 2, ch = ph / 2;
    memset(out_y, bg_y, (size_t)pw * ph);
    memset(out_u, bg_u, (size_t)cw * ch);
    memset(out_v, bg_v, (size_t)cw * ch);
    for (int k = 0; k < n; ++k) {
        const vp8hip_tile &t = tiles[k];
        const vp8hip_tile_planes &p = src[k];
        if (!p.y) continue;
        TapTable x, y, xc, yc;
        if (!tap_table(t.in_w, t.w, t.filter, &x) || !tap_table(t.in_h, t.h, t.filter, &y) || !tap_table(t.in_w / 2, t.w / 2, t.filter, &xc) ||
            !tap_table(t.in_h / 2, t.h / 2, t.filter, &yc))
            return -1;      // (vp8host_tile_valid has said otherwise)
        compose_plane(p.y, p.pitch_y ? p.pitch_y : t.in_w, t.in_h, x, y, t.w, t.h, out_y + (size_t)t.y * pw + t.x, pw);
        compose_plane(p.u, p.pitch_u ? p.pitch_u : t.in_w / 2, t.in_h / 2, xc, yc, t.w / 2, t.h / 2, out_u + (size_t)(t.y / 2) * cw + t.x / 2, cw);
        compose_plane(p.v, p.pitch_v ? p.pitch_v : t.in_w / 2, t.in_h / 2, xc, yc, t.w / 2, t.h / 2, out_v + (size_t)(t.y / 2) * cw + t.x / 2, cw);
    }
    return 0;
}

}  // extern "C"

// The device's temporal denoiser in plain C++ (include/vp8hip_host.h has the rule).
namespace {

inline int denoise_step(int s, int r, int k, int *a_out) {
    const int d = r - s, a = d < 0 ? -d : d;
    *a_out = a;
    if (a <= 2 + k) return d;
    const int m = a <= 7 ? 2 + k : (a <= 15 ? 3 + k : 5 + k);
    return d < 0 ? -m : m;
}

// one n x n block: the steps into c[], returns T; *sad gets the sum of |d|
int denoise_block(const uint8_t *s, const uint8_t *r, int stride, int n, int k, int *c, int *sad) {
    int T = 0;
    *sad = 0;
    for (int y = 0; y < n; ++y)
        for (int x = 0; x < n; ++x) {
            int a;
            const int v = denoise_step(s[y * stride + x], r[y * stride + x], k, &a);
            c[y * n + x] = v;
            T += v;
            *sad += a;
        }
    return T;
}

void denoise_put(const uint8_t *s, uint8_t *o, int stride, int n, const int *c) {
    for (int y = 0; y < n; ++y)
        for (int x = 0; x < n; ++x) o[y * stride + x] = (uint8_t)(s[y * stride + x] + (c ? c[y * n + x] : 0));
}

}  // namespace

extern "C" int vp8host_denoise_frame(const uint8_t *src_y, const uint8_t *src_u, const uint8_t *src_v, uint8_t *hist_y, uint8_t *hist_u,
                                     uint8_t *hist_v, uint8_t *out_y, uint8_t *out_u, uint8_t *out_v, int width, int height, int level,
                                     int have_history, int32_t *mbs_filtered) {
    if (!src_y || !src_u || !src_v || !out_y || !out_u || !out_v || !mbs_filtered || width < 16 || height < 16 || (width & 15) || (height & 15) ||
        level < 0 || level > 3 || (level && (!hist_y || !hist_u || !hist_v)))
        return -1;
    const int cw = width / 2, ch = height / 2;
    const size_t ny = (size_t)width * height, nc = (size_t)cw * ch;
    *mbs_filtered = 0;
    if (!level || !have_history) {
        if (out_y != src_y) memmove(out_y, src_y, ny);
        if (out_u != src_u) memmove(out_u, src_u, nc);
        if (out_v != src_v) memmove(out_v, src_v, nc);
    } else {
        int c[256], cc[64], sad, unused;
        for (int my = 0; my < height / 16; ++my)
            for (int mx = 0; mx < width / 16; ++mx) {
                const size_t oy = (size_t)my * 16 * width + mx * 16, oc = (size_t)my * 8 * cw + mx * 8;
                const int T = denoise_block(src_y + oy, hist_y + oy, width, 16, level, c, &sad);
                const bool f = (T < 0 ? -T : T) <= VP8HOST_DENOISE_SUM_Y && sad <= VP8HOST_DENOISE_SAD_Y;
                denoise_put(src_y + oy, out_y + oy, width, 16, f ? c : nullptr);
                *mbs_filtered += f;
                const uint8_t *sp[2] = {src_u + oc, src_v + oc}, *hp[2] = {hist_u + oc, hist_v + oc};
                uint8_t *op[2] = {out_u + oc, out_v + oc};
                for (int p = 0; p < 2; ++p) {
                    const int Tc = denoise_block(sp[p], hp[p], cw, 8, level, cc, &unused);
                    denoise_put(sp[p], op[p], cw, 8, f && (Tc < 0 ? -Tc : Tc) <= VP8HOST_DENOISE_SUM_C ? cc : nullptr);
                }
            }
    }
    if (level) {
        if (hist_y != out_y) memmove(hist_y, out_y, ny);
        if (hist_u != out_u) memmove(hist_u, out_u, nc);
        if (hist_v != out_v) memmove(hist_v, out_v, nc);
    }
    return 0;
}

// The device's deinterlacer in plain C++ (include/vp8hip_host.h has the rule).
namespace {

// one tight plane of w x h; hist = nullptr: no history (output = the spatial value).  Returns the samples of missing rows left as they came.
int deinterlace_plane(const uint8_t *src, const uint8_t *hist, uint8_t *out, int w, int h, int keep) {
    const int n = (h - keep + 1) / 2;      // kept rows: 2 j + keep < h
    int woven = 0;
    for (int y = 0; y < h; ++y) {
        const uint8_t *row = src + (size_t)y * w;
        uint8_t *o = out + (size_t)y * w;
        if ((y & 1) == keep) {
            memcpy(o, row, (size_t)w);
            continue;
        }
        const int j0 = (y - 1 - keep) >> 1;      // (arithmetic: -1 for y = 0, keep = 1)
        const uint8_t *tap[4];
        for (int k = 0; k < 4; ++k) {
            int j = j0 - 1 + k;
            j = j < 0 ? 0 : (j > n - 1 ? n - 1 : j);
            tap[k] = src + (size_t)(2 * j + keep) * w;
        }
        const int ya = y > 0 ? y - 1 : 0, yb = y < h - 1 ? y + 1 : h - 1;
        for (int x = 0; x < w; ++x) {
            int s = (-tap[0][x] + 9 * tap[1][x] + 9 * tap[2][x] - tap[3][x] + 8) >> 4;
            s = s < 0 ? 0 : (s > 255 ? 255 : s);
            if (hist) {
                auto d = [&](int r) { const int v = (int)src[(size_t)r * w + x] - (int)hist[(size_t)r * w + x]; return v < 0 ? -v : v; };
                int m = d(y);
                if (d(ya) > m) m = d(ya);
                if (d(yb) > m) m = d(yb);
                const int wv = row[x], lo = wv - m, hi = wv + m;
                s = s < lo ? lo : (s > hi ? hi : s);
                woven += s == wv;
            }
            o[x] = (uint8_t)s;
        }
    }
    return woven;
}

}  // namespace

extern "C" int vp8host_deinterlace_frame(const uint8_t *src_y, const uint8_t *src_u, const uint8_t *src_v, uint8_t *hist_y, uint8_t *hist_u,
                                         uint8_t *hist_v, uint8_t *out_y, uint8_t *out_u, uint8_t *out_v, int width, int height, int mode,
                                         int keep, int have_history, int32_t *woven) {
    if (!src_y || !src_u || !src_v || !out_y || !out_u || !out_v || !woven || width < 2 || height < 4 || (width & 1) || (height & 1) ||
        mode < 0 || mode > 2 || (keep != 0 && keep != 1) || (mode == 2 && (!hist_y || !hist_u || !hist_v)))
        return -1;
    const int cw = width / 2, ch = height / 2;
    const size_t ny = (size_t)width * height, nc = (size_t)cw * ch;
    *woven = 0;
    if (!mode) {
        if (out_y != src_y) memmove(out_y, src_y, ny);
        if (out_u != src_u) memmove(out_u, src_u, nc);
        if (out_v != src_v) memmove(out_v, src_v, nc);
        return 0;
    }
    const bool h = mode == 2 && have_history;
    *woven = deinterlace_plane(src_y, h ? hist_y : nullptr, out_y, width, height, keep);
    (void)deinterlace_plane(src_u, h ? hist_u : nullptr, out_u, cw, ch, keep);
    (void)deinterlace_plane(src_v, h ? hist_v : nullptr, out_v, cw, ch, keep);
    if (mode == 2) {
        memmove(hist_y, src_y, ny);
        memmove(hist_u, src_u, nc);
        memmove(hist_v, src_v, nc);
    }
    return 0;
}

// The source side of the frame analysis record in plain C++ (include/vp8hip_host.h has the rule).
extern "C" int vp8host_analyse_luma(const uint8_t *cur, const uint8_t *prev, int width, int height, vp8host_luma_analysis *out) {
    if (!cur || !out || width < 16 || height < 16 || (width & 15) || (height & 15)) return -1;
    vp8host_luma_analysis r{};
    r.have_prev = prev ? 1 : 0;
    for (int my = 0; my < height / 16; ++my)
        for (int mx = 0; mx < width / 16; ++mx) {
            const size_t o = (size_t)my * 16 * (size_t)width + (size_t)mx * 16;
            uint64_t s = 0, ss = 0, sad = 0, sse = 0;
            for (int y = 0; y < 16; ++y)
                for (int x = 0; x < 16; ++x) {
                    const size_t i = o + (size_t)y * (size_t)width + (size_t)x;
                    const int v = cur[i];
                    s += (uint64_t)v;
                    ss += (uint64_t)(v * v);
                    if (prev) {
                        const int d = v - (int)prev[i];
                        sad += (uint64_t)(d < 0 ? -d : d);
                        sse += (uint64_t)(d * d);
                    }
                }
            r.spatial += 256u * ss - s * s;
            r.temporal_sse += sse;
            r.temporal_sad += sad;
            if (prev && sad == 0) r.static_mbs++;
        }
    *out = r;
    return 0;
}

// The variance-adaptive segment map in plain C++ (include/vp8hip_host.h has the rule; k_aq_map_b and k_aq_seg_b are the device's form).
extern "C" int vp8host_aq_segment(int e, int E, int W) {
    if (W <= 0) return 2;
    const int d = e - E;
    const int q = d >= 0 ? d / W : -((-d + W - 1) / W);
    const int s = 2 + q;
    return s < 0 ? 0 : (s > 3 ? 3 : s);
}

extern "C" int vp8host_aq_segment_map(const uint8_t *luma, int stride, int width, int height, int strength, uint8_t *map_out, uint8_t *e_out) {
    if (!luma || !map_out || width < 16 || height < 16 || (width & 15) || (height & 15) || stride < width || strength < 1 || strength > 3) return -1;
    const int mbw = width / 16, mbs = mbw * (height / 16);
    const int W = strength == 1 ? 24 : (strength == 2 ? 16 : 12);
    int64_t total = 0;      // (e waits in map_out for the frame's mean: no allocation)
    for (int mb = 0; mb < mbs; ++mb) {
        const uint8_t *o = luma + (size_t)(mb / mbw) * 16 * (size_t)stride + (size_t)(mb % mbw) * 16;
        uint32_t s = 0, ss = 0;
        for (int y = 0; y < 16; ++y)
            for (int x = 0; x < 16; ++x) {
                const uint32_t v = o[(size_t)y * (size_t)stride + (size_t)x];
                s += v;
                ss += v * v;
            }
        const uint32_t n = 256u * ss - s * s + 1u;
        int p = 0;
        while ((n >> p) > 1u) ++p;
        const uint32_t frac = p >= 3 ? (n >> (p - 3)) & 7u : (n << (3 - p)) & 7u;
        map_out[mb] = (uint8_t)(8 * p + (int)frac);
        total += map_out[mb];
    }
    const int E = (int)(total / mbs);
    for (int mb = 0; mb < mbs; ++mb) {
        const uint8_t e = map_out[mb];
        if (e_out) e_out[mb] = e;
        map_out[mb] = (uint8_t)vp8host_aq_segment(e, E, W);
    }
    return 0;
}

// The geometry of the input side in plain C++ (include/vp8hip_host.h has the rule): the window of a surface, and quarter turns.
extern "C" int vp8host_source_window(int format, int width, int height, int x, int y, const int32_t pitch[3], size_t offset[3],
                                     int32_t row_bytes[3], int32_t rows[3]) {
    // per plane: horizontal shift, vertical shift, bytes per element (0: the format has no such plane)
    struct PlaneRule { int hs, vs, bpe; };
    PlaneRule r[3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
    SourceLayout l;
    if (format == VP8HOST_FORMAT_YUY2 || format == VP8HOST_FORMAT_UYVY) r[0] = {1, 0, 4};
    else if (format == VP8HOST_FORMAT_BGRA || format == VP8HOST_FORMAT_RGBA) r[0] = {0, 0, 4};
    else if (source_layout(format, &l)) {
        const int b = l.depth > 8 ? 2 : 1;
        r[0] = {0, 0, b};
        r[1] = {l.sub_x, l.sub_y, l.nv ? 2 * b : b};
        if (!l.nv) r[2] = r[1];
    } else return -1;
    if (!pitch || !offset || !row_bytes || !rows || width <= 0 || height <= 0 || (width & 1) || (height & 1) || x < 0 || y < 0 || (x & 1) || (y & 1))
        return -1;
    for (int p = 0; p < 3; ++p)
        if (r[p].bpe && (int64_t)pitch[p] < (int64_t)((x + width) >> r[p].hs) * r[p].bpe) return -1;
    for (int p = 0; p < 3; ++p) {
        offset[p] = 0;
        row_bytes[p] = rows[p] = 0;
        if (!r[p].bpe) continue;
        rows[p] = height >> r[p].vs;
        row_bytes[p] = (width >> r[p].hs) * r[p].bpe;
        offset[p] = (size_t)(y >> r[p].vs) * (size_t)pitch[p] + (size_t)(x >> r[p].hs) * (size_t)r[p].bpe;
    }
    return 0;
}

extern "C" int vp8host_window_frame(int format, int width, int height, int x, int y, const int32_t pitch[3], const uint8_t *p0,
                                    const uint8_t *p1, const uint8_t *p2, uint8_t *out0, uint8_t *out1, uint8_t *out2) {
    size_t off[3];
    int32_t rb[3], rows[3];
    if (vp8host_source_window(format, width, height, x, y, pitch, off, rb, rows) != 0) return -1;
    const uint8_t *src[3] = {p0, p1, p2};
    uint8_t *dst[3] = {out0, out1, out2};
    for (int p = 0; p < 3; ++p)
        if (rows[p] && (!src[p] || !dst[p])) return -1;
    for (int p = 0; p < 3; ++p)
        for (int r = 0; r < rows[p]; ++r)
            memcpy(dst[p] + (size_t)r * (size_t)rb[p], src[p] + off[p] + (size_t)r * (size_t)pitch[p], (size_t)rb[p]);
    return 0;
}

namespace {

void orient_plane(const uint8_t *in, uint8_t *out, int rw, int rh, int turns, int mirror) {
    const bool odd = turns & 1;
    const int ow = odd ? rh : rw, oh = odd ? rw : rh;
    for (int y = 0; y < oh; ++y)
        for (int x = 0; x < ow; ++x) {
            int sx, sy;      // where out(x, y) sits in s, the mirrored frame
            switch (turns) {
                case 0: sx = x; sy = y; break;
                case 1: sx = y; sy = rh - 1 - x; break;
                case 2: sx = rw - 1 - x; sy = rh - 1 - y; break;
                default: sx = rw - 1 - y; sy = x; break;
            }
            if (mirror) sx = rw - 1 - sx;
            out[(size_t)y * (size_t)ow + (size_t)x] = in[(size_t)sy * (size_t)rw + (size_t)sx];
        }
}

}  // namespace

extern "C" int vp8host_orient_frame(int turns, int mirror, int raw_width, int raw_height, const uint8_t *in_y, const uint8_t *in_u,
                                    const uint8_t *in_v, uint8_t *out_y, uint8_t *out_u, uint8_t *out_v) {
    if (turns < 0 || turns > 3 || (mirror != 0 && mirror != 1) || raw_width < 2 || raw_height < 2 || (raw_width & 1) || (raw_height & 1) ||
        !in_y || !in_u || !in_v || !out_y || !out_u || !out_v)
        return -1;
    orient_plane(in_y, out_y, raw_width, raw_height, turns, mirror);
    orient_plane(in_u, out_u, raw_width / 2, raw_height / 2, turns, mirror);
    orient_plane(in_v, out_v, raw_width / 2, raw_height / 2, turns, mirror);
    return 0;
}

// The temporal filter of the hidden alternate reference frame in plain C++ (include/vp8hip_host.h has the rule).
namespace {

// sample (x, y) of a tight plane of w x h extended by its last column and row (coordinates below 0 never count, they are clamped too)
inline int arf_at(const uint8_t *p, int w, int h, int x, int y) {
    x = x < 0 ? 0 : (x > w - 1 ? w - 1 : x);
    y = y < 0 ? 0 : (y > h - 1 ? h - 1 : y);
    return p[(size_t)y * w + x];
}

// one block of bs x bs samples at (bx, by) of plane `o` (centre) against `p` displaced by (dx, dy), block weight bw: into acc / count
void arf_accumulate(const uint8_t *o, const uint8_t *p, int w, int h, int bx, int by, int bs, int dx, int dy, int bw, int strength,
                    uint32_t *acc, uint32_t *count) {
    const int r = strength ? 1 << (strength - 1) : 0;
    for (int y = 0; y < bs; ++y)
        for (int x = 0; x < bs; ++x) {
            const int ov = arf_at(o, w, h, bx + x, by + y), pv = arf_at(p, w, h, bx + x + dx, by + y + dy);
            const int d = ov - pv;
            int m = (3 * d * d + r) >> strength;
            m = 16 - (m < 16 ? m : 16);
            count[y * bs + x] += (uint32_t)(m * bw);
            acc[y * bs + x] += (uint32_t)(m * bw * pv);
        }
}

void arf_put(uint8_t *out, int w, int h, int bx, int by, int bs, const uint32_t *acc, const uint32_t *count) {
    for (int y = 0; y < bs && by + y < h; ++y)
        for (int x = 0; x < bs && bx + x < w; ++x) {
            const uint32_t n = count[y * bs + x];
            out[(size_t)(by + y) * w + bx + x] = (uint8_t)VP8HOST_ARF_DIVIDE(acc[y * bs + x] + n / 2, VP8HOST_ARF_RECIPROCAL(n));
        }
}

}  // namespace

extern "C" void vp8host_arf_round_divide(const uint32_t *acc, const uint32_t *count, size_t n, uint32_t *out) {
    for (size_t i = 0; i < n; ++i) out[i] = VP8HOST_ARF_DIVIDE(acc[i] + count[i] / 2, VP8HOST_ARF_RECIPROCAL(count[i]));
}

extern "C" int vp8host_arf_filter_frame(const uint8_t *const *frames, int n, int centre, int strength, int width, int height, uint8_t *out_y,
                                        uint8_t *out_u, uint8_t *out_v, int32_t weights[3], int8_t *vectors) {
    if (!frames || !out_y || !out_u || !out_v || n < 1 || n > VP8HOST_ARF_MAX_FRAMES || centre < 0 || centre >= n || strength < 0 || strength > 6 ||
        width < 2 || height < 2 || (width & 1) || (height & 1))
        return -1;
    for (int i = 0; i < 3 * n; ++i)
        if (!frames[i]) return -1;
    const int cw = width / 2, ch = height / 2, tw = (width + 15) / 16, th = (height + 15) / 16, We = tw * 16, He = th * 16;
    if (weights) weights[0] = weights[1] = weights[2] = 0;
    const uint8_t *const *C = frames + 3 * centre;
    uint32_t acc[3][256], count[3][256];
    for (int ty = 0; ty < th; ++ty)
        for (int tx = 0; tx < tw; ++tx) {
            const int x0 = tx * 16, y0 = ty * 16;
            memset(acc, 0, sizeof acc);
            memset(count, 0, sizeof count);
            for (int k = 0; k < n; ++k) {
                const uint8_t *const *F = frames + 3 * k;
                int dx = 0, dy = 0, bw = 2;
                if (k != centre) {
                    uint32_t best = 0xFFFFFFFFu;
                    for (int cy = -8; cy <= 7; ++cy)
                        for (int cx = -8; cx <= 7; ++cx) {
                            if (x0 + cx < 0 || x0 + cx + 16 > We || y0 + cy < 0 || y0 + cy + 16 > He) continue;
                            uint32_t sad = 0;
                            for (int y = 0; y < 16; ++y)
                                for (int x = 0; x < 16; ++x) {
                                    const int d = arf_at(C[0], width, height, x0 + x, y0 + y) - arf_at(F[0], width, height, x0 + x + cx, y0 + y + cy);
                                    sad += (uint32_t)(d < 0 ? -d : d);
                                }
                            const uint32_t key = sad << 13 | (uint32_t)((cx < 0 ? -cx : cx) + (cy < 0 ? -cy : cy)) << 8 | (uint32_t)(cy + 8) << 4 | (uint32_t)(cx + 8);
                            if (key < best) best = key;
                        }
                    dx = (int)(best & 15u) - 8;
                    dy = (int)((best >> 4) & 15u) - 8;
                    uint32_t sse = 0;
                    for (int y = 0; y < 16; ++y)
                        for (int x = 0; x < 16; ++x) {
                            const int d = arf_at(C[0], width, height, x0 + x, y0 + y) - arf_at(F[0], width, height, x0 + x + dx, y0 + y + dy);
                            sse += (uint32_t)(d * d);
                        }
                    bw = sse < VP8HOST_ARF_THRESH_LOW ? 2 : (sse < VP8HOST_ARF_THRESH_HIGH ? 1 : 0);
                    if (weights) ++weights[bw];
                }
                if (vectors) {
                    int8_t *v = vectors + ((size_t)(ty * tw + tx) * n + k) * 2;
                    v[0] = (int8_t)dx;
                    v[1] = (int8_t)dy;
                }
                if (!bw) continue;
                arf_accumulate(C[0], F[0], width, height, x0, y0, 16, dx, dy, bw, strength, acc[0], count[0]);
                arf_accumulate(C[1], F[1], cw, ch, x0 / 2, y0 / 2, 8, dx >> 1, dy >> 1, bw, strength, acc[1], count[1]);
                arf_accumulate(C[2], F[2], cw, ch, x0 / 2, y0 / 2, 8, dx >> 1, dy >> 1, bw, strength, acc[2], count[2]);
            }
            arf_put(out_y, width, height, x0, y0, 16, acc[0], count[0]);
            arf_put(out_u, cw, ch, x0 / 2, y0 / 2, 8, acc[1], count[1]);
            arf_put(out_v, cw, ch, x0 / 2, y0 / 2, 8, acc[2], count[2]);
        }
    return 0;
}
