// Stand-alone host program over csrc/gif/d2d_gif_core.h (built with the address and undefined-behaviour
// sanitizers by tests/test_gif.py::test_gif_host_code_sanitized): the palette lookup, the index + delta stage,
// the segmented LZW, the merge and the chunk framing through the CPU twin, decoded again by a plain GIF LZW
// decoder written here.  Chunk rows are exactly d2dg_frame_cap long, so a byte past the bound is a
// sanitizer error; the dictionaries and staging buffers start from garbage, as the device workspace does.
// Exit status 0: every check held and the sanitizers saw nothing.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "gif/d2d_gif_core.h"

#define CHECK(cond)                                                                             \
    do {                                                                                        \
        if (!(cond)) {                                                                          \
            std::fprintf(stderr, "%s:%d: %s failed (%s)\n", __FILE__, __LINE__, #cond, g_case); \
            std::exit(1);                                                                       \
        }                                                                                       \
    } while (0)
static char g_case[128] = "";

static uint32_t g_rng = 12345u;
static uint32_t rnd() {
    g_rng = g_rng * 1664525u + 1013904223u;
    return g_rng >> 8;
}

// GIF89a appendix F: variable-width codes LSB first, Clear at any point, the code-equals-next-entry case
static std::vector<uint8_t> lzw_decode(const std::vector<uint8_t>& data, int m, size_t n_px, bool* saw_end) {
    std::vector<uint8_t> out;
    std::vector<int> prefix(4096, -1);
    std::vector<uint8_t> suffix(4096, 0), stack;
    const int clear = 1 << m, eoi = clear + 1;
    int width = m + 1, avail = clear + 2, prev = -1;
    size_t bit = 0;
    *saw_end = false;
    auto first_of = [&](int c) {
        while (c >= clear) c = prefix[(size_t)c];
        return (uint8_t)c;
    };
    while (bit + (size_t)width <= 8 * data.size()) {
        int code = 0;
        for (int i = 0; i < width; ++i, ++bit) code |= ((data[bit >> 3] >> (bit & 7)) & 1) << i;
        if (code == clear) {
            width = m + 1, avail = clear + 2, prev = -1;
            continue;
        }
        if (code == eoi) {
            *saw_end = true;
            break;
        }
        CHECK(code <= avail && (prev >= 0 || code < clear));
        if (prev >= 0 && avail < 4096) {
            prefix[(size_t)avail] = prev;
            suffix[(size_t)avail] = code == avail ? first_of(prev) : first_of(code);
            ++avail;
            if (avail == (1 << width) && width < 12) ++width;
        } else {
            CHECK(code < avail);
        }
        for (int c = code; c >= clear; c = prefix[(size_t)c]) stack.push_back(suffix[(size_t)c]);
        stack.push_back(first_of(code));
        while (!stack.empty()) out.push_back(stack.back()), stack.pop_back();
        prev = code;
    }
    CHECK(out.size() == n_px);
    return out;
}

struct Stream {
    int W, H, n;
    std::vector<uint8_t> pal, canvas, shown;  // shown: the decoder's canvas of indices
    uint8_t has = 0;
    int32_t inexact = 0, mid_clears = 0;
};

// encode one frame through the twin, decode the chunk, compose it, compare with the wanted indices
static void frame(Stream& s, const std::vector<uint8_t>& rgb, const std::vector<uint8_t>& want_idx) {
    using namespace d2dg;
    PalTable pal;
    build_pal(s.pal.data(), s.n, &pal);
    const int64_t cap = frame_cap(s.W, s.H);
    std::vector<uint8_t> chunk((size_t)cap);
    HostWork wk;
    wk.slot.resize(SLOTS), wk.ent.resize(D2DG_DICT_CAP);
    for (auto& v : wk.slot) v = (uint16_t)rnd();
    for (auto& v : wk.ent) v = rnd() | (rnd() << 16);
    const bool had = s.has != 0;
    const uint32_t len = encode_stream_host(pal, s.W, s.H, rgb.data(), 3, s.canvas.data(), had, chunk.data(), &s.inexact,
                                            &s.mid_clears, wk);
    s.has = 1;
    CHECK((int64_t)len <= cap);
    CHECK(chunk[0] == 0x21 && chunk[1] == 0xF9 && chunk[3] == (had ? 5 : 4) && chunk[4] == 3 && chunk[6] == s.n);
    CHECK(chunk[8] == 0x2C && chunk[18] == pal.m && chunk[len - 1] == 0);
    const int left = chunk[9] | chunk[10] << 8, top = chunk[11] | chunk[12] << 8;
    const int w = chunk[13] | chunk[14] << 8, h = chunk[15] | chunk[16] << 8;
    CHECK(w >= 1 && h >= 1 && left + w <= s.W && top + h <= s.H);
    std::vector<uint8_t> data;
    size_t o = 19;
    while (chunk[o] != 0) {
        CHECK(o + 1 + chunk[o] < len);
        data.insert(data.end(), chunk.begin() + (long)o + 1, chunk.begin() + (long)o + 1 + chunk[o]);
        o += 1u + chunk[o];
    }
    CHECK(o == len - 1);
    bool end = false;
    const std::vector<uint8_t> px = lzw_decode(data, pal.m, (size_t)w * (size_t)h, &end);
    CHECK(end);
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            const uint8_t v = px[(size_t)y * (size_t)w + (size_t)x];
            CHECK(v <= s.n && (had || v < s.n));
            if (v != s.n) s.shown[(size_t)(top + y) * (size_t)s.W + (size_t)(left + x)] = v;
        }
    CHECK(s.shown == want_idx);
    CHECK(s.canvas == want_idx);
}

static Stream make_stream(int W, int H, int n) {
    Stream s;
    s.W = W, s.H = H, s.n = n;
    s.pal.resize((size_t)n * 3);
    for (int i = 0; i < n; ++i) {  // distinct colours
        s.pal[3 * (size_t)i] = (uint8_t)i, s.pal[3 * (size_t)i + 1] = (uint8_t)(255 - i), s.pal[3 * (size_t)i + 2] = (uint8_t)(i * 7);
    }
    s.canvas.assign((size_t)W * (size_t)H, 0);
    s.shown.assign((size_t)W * (size_t)H, 0);
    return s;
}

static std::vector<uint8_t> to_rgb(const Stream& s, const std::vector<uint8_t>& idx) {
    std::vector<uint8_t> rgb(idx.size() * 3);
    for (size_t p = 0; p < idx.size(); ++p) memcpy(&rgb[3 * p], &s.pal[3 * (size_t)idx[p]], 3);
    return rgb;
}

int main() {
    using namespace d2dg;
    // every minimum code size, odd sizes, noise / runs / a frame equal to its predecessor / small boxes
    const int sizes[][2] = {{8, 8}, {53, 37}, {130, 129}};
    const int colours[] = {1, 2, 3, 4, 5, 16, 17, 128, 129, 255};
    for (auto& sz : sizes)
        for (int n : colours) {
            std::snprintf(g_case, sizeof g_case, "%d x %d, %d colours", sz[0], sz[1], n);
            Stream s = make_stream(sz[0], sz[1], n);
            const size_t px = (size_t)sz[0] * (size_t)sz[1];
            std::vector<uint8_t> idx(px);
            for (auto& v : idx) v = (uint8_t)(rnd() % (uint32_t)n);
            frame(s, to_rgb(s, idx), idx);  // noise, first frame
            frame(s, to_rgb(s, idx), idx);  // unchanged: 1 x 1 transparent
            for (int boxw : {1, 63, 64, 65}) {  // a box of 1 x boxw changed pixels (clipped to the row)
                const int bw = boxw < sz[0] ? boxw : sz[0];
                for (int x = 0; x < bw; ++x) idx[(size_t)x + (size_t)sz[0]] = (uint8_t)((idx[(size_t)x + (size_t)sz[0]] + 1) % n);
                if (n > 1) frame(s, to_rgb(s, idx), idx);
            }
            idx.assign(px, (uint8_t)(n - 1));  // one colour: the longest runs
            frame(s, to_rgb(s, idx), idx);
            idx[0] = 0, idx[px - 1] = 0;  // first and last pixel: the box is the whole picture
            frame(s, to_rgb(s, idx), idx);
            for (auto& v : idx) v = (uint8_t)(rnd() % (uint32_t)n);
            frame(s, to_rgb(s, idx), idx);  // noise as a delta (transparent pixels among it)
            CHECK(s.inexact == 0);
        }
    // 255-colour noise whose segments outgrow the dictionary: Clears inside segments
    {
        std::snprintf(g_case, sizeof g_case, "noise 520 x 512");
        Stream s = make_stream(520, 512, 255);
        std::vector<uint8_t> idx((size_t)520 * 512);
        for (auto& v : idx) v = (uint8_t)(rnd() % 255u);
        frame(s, to_rgb(s, idx), idx);
        CHECK(s.mid_clears >= (D2DG_DICT_CAP == 4096 ? 64 : 1));
    }
    // off-palette colours: the nearest entry, the lowest index on ties, counted
    {
        std::snprintf(g_case, sizeof g_case, "nearest");
        Stream s = make_stream(8, 8, 3);
        const uint8_t pal[9] = {0, 0, 0, 10, 0, 0, 0, 10, 0};
        s.pal.assign(pal, pal + 9);
        std::vector<uint8_t> rgb(8 * 8 * 3, 0), want(64, 0);
        rgb[0] = 5, want[0] = 0;               // (5, 0, 0): tie between 0 and 1 -> 0
        rgb[3] = 6, want[1] = 1;               // (6, 0, 0) -> 1
        rgb[6] = 5, rgb[7] = 5, want[2] = 0;   // (5, 5, 0): three-way tie -> 0
        rgb[10] = 200, want[3] = 2;            // (0, 200, 0) -> 2
        frame(s, rgb, want);
        CHECK(s.inexact == 4);
    }
    // the file header and the bound
    {
        PalTable pal;
        const uint8_t c[12] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12};
        build_pal(c, 4, &pal);
        CHECK(pal.bits == 3 && pal.m == 3);
        uint8_t out[D2DG_FILE_HEADER_MAX];
        CHECK(file_header(64, 48, pal, 0, out) == 13 + 24 + 19 && out[10] == (0xF0 | 2) && out[13] == 1 && out[13 + 24] == 0x21);
        CHECK(file_header(64, 48, pal, -1, out) == 13 + 24);
        build_pal(c, 1, &pal);
        CHECK(pal.bits == 1 && pal.m == 2);
        CHECK(frame_cap(8, 8) == 20 + 194 + 1);  // 64 + 64 + 0 + 1 = 129 codes, 194 bytes, one block
    }
    std::puts("gif host code: ok");
    return 0;
}
