// Stand-alone host program over csrc/hud/d2d_hud_core.h (built with the address and undefined-behaviour
// sanitizers by tests/test_hud.py::test_hud_host_code_sanitized): the extended list, the number formatting,
// the text lookup, the shade recorder and the CPU twins on the edge cases -- smallest and odd picture sizes,
// every new layer bit alone and with the base layers, NULL info / shades / obs / trail, shade counts of 0, the
// capacity and beyond, NaN / +-inf / 1e300 in every state field, in the poses and in the info row, and the
// layers-off identity with d2d_raster.h's own twin.  Exit status 0: every check held and the sanitizers saw
// nothing.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "hud/d2d_hud_core.h"

#define CHECK(cond)                                                                             \
    do {                                                                                        \
        if (!(cond)) {                                                                          \
            std::fprintf(stderr, "%s:%d: %s failed (%s)\n", __FILE__, __LINE__, #cond, g_case); \
            std::exit(1);                                                                       \
        }                                                                                       \
    } while (0)
static char g_case[128] = "";

static const double SW = 1300.0, SH = 1300.0;

// a 3-waypoint path (one quadratic) from (100, 200) over (600, 700) to (1100, 400), n circles on a grid
static d2d_scn make_scn(int n_circles) {
    d2d_scn s;
    std::memset(&s, 0, sizeof s);
    s.n_wps = 3;
    s.n_circles = n_circles;
    const double wx[3] = {100, 600, 1100}, wy[3] = {200, 700, 400};
    s.us[0] = 0.0;
    for (int i = 1; i < 3; ++i) s.us[i] = s.us[i - 1] + std::hypot(wx[i] - wx[i - 1], wy[i] - wy[i - 1]);
    auto fit = [&](const double* w, double* a, double* b, double* c) {
        const double u0 = s.us[0], u1 = s.us[1], u2 = s.us[2];
        const double d0 = (u0 - u1) * (u0 - u2), d1 = (u1 - u0) * (u1 - u2), d2 = (u2 - u0) * (u2 - u1);
        *a = w[0] / d0 + w[1] / d1 + w[2] / d2;
        *b = -(w[0] * (u1 + u2) / d0 + w[1] * (u0 + u2) / d1 + w[2] * (u0 + u1) / d2);
        *c = w[0] * u1 * u2 / d0 + w[1] * u0 * u2 / d1 + w[2] * u0 * u1 / d2;
    };
    fit(wx, &s.xa[0], &s.xb[0], &s.xc[0]);
    fit(wy, &s.ya[0], &s.yb[0], &s.yc[0]);
    for (int i = 0; i < n_circles; ++i) s.cx[i] = 150.0 + 140.0 * (i % 8), s.cy[i] = 150.0 + 140.0 * (i / 8), s.cr[i] = 10.0 + i;
    s.wp_last_x = wx[2], s.wp_last_y = wy[2];
    s.spawn_xmin = 50, s.spawn_xmax = 300, s.spawn_ymin = 150, s.spawn_ymax = 1000;
    s.spawn_amin = -0.785, s.spawn_amax = 0.785;
    return s;
}

static void set_pose(std::vector<double>& st, int n, int f, double x, double y, double a, double vx, double vy) {
    const double c = std::cos(a), s = std::sin(a);
    const double v[18] = {x, y, a, vx, vy, 0.1, x - 40 * c, y - 40 * s, a, vx, vy, 0, x + 40 * c, y + 40 * s, a, vx, vy, 0};
    for (int k = 0; k < 18; ++k) st[(size_t)k * (size_t)n + (size_t)f] = v[k];
}

struct Inputs {
    const float *obs, *act, *trail;
    const int32_t* tl;
    int max_trail;
    const float* info;
    const double* shade;
    const int32_t* count;
    int max_shades;
};

static std::vector<uint8_t> render(int W, int H, int n, const std::vector<d2d_scn>& scn, const std::vector<double>& st,
                                   const Inputs& in, uint32_t layers) {
    d2dr_view v = {W, H, SW, SH, layers, 0};
    std::vector<uint8_t> out((size_t)n * (size_t)W * (size_t)H * 3 + 64, 0x5a);  // 64 canary bytes behind
    d2dh::render_host(&v, n, scn.data(), st.data(), in.obs, in.act, in.trail, in.tl, in.max_trail, in.info, in.shade,
                      in.count, in.max_shades, out.data());
    for (size_t k = out.size() - 64; k < out.size(); ++k) CHECK(out[k] == 0x5a);
    out.resize(out.size() - 64);
    return out;
}

static std::string fmt(float v) {
    char buf[16];
    std::memset(buf, 0x7f, sizeof buf);
    const int32_t n = d2dh::format_value(v, buf);
    CHECK(n >= 1 && n <= 13 && buf[n] == 0);
    return std::string(buf);
}

int main() {
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    // ---- formatting: known answers, the longest outputs, every exponent of float32
    std::snprintf(g_case, sizeof g_case, "format");
    CHECK(fmt(2.675f) == "2.67" && fmt(0.125f) == "0.12" && fmt(12.5f) == "12.5" && fmt(-0.0f) == "-0.0");
    CHECK(fmt(0.0f) == "0.0" && fmt(-0.001f) == "-0.0" && fmt(0.005f) == "0.0" && fmt(0.995f) == "1.0");
    CHECK(fmt((float)inf) == "inf" && fmt((float)-inf) == "-inf" && fmt((float)nan) == "nan");
    CHECK(fmt(3e10f) == "999999999.99" && fmt(-3.4e38f) == "-999999999.99" && fmt(999999936.0f) == "999999936.0");
    CHECK(fmt(-99999992.0f) == "-99999992.0" && fmt(1e-45f) == "0.0");
    for (int e = -149; e <= 127; ++e) {
        fmt(std::ldexp(1.0f, e));
        fmt(-std::ldexp(1.999f, e));
    }
    // ---- glyphs: any byte, any row
    for (int ch = -5; ch < 300; ++ch)
        for (int r = 0; r < 7; ++r) CHECK(d2dh_glyph_row(ch, r) < 32u);
    // ---- text lookup beyond the block and beyond the line
    {
        std::vector<uint8_t> lines((size_t)D2DH_TEXT_LINES * D2DH_LINE_CHARS, (uint8_t)'8');
        for (int s : {1, 2, 4})
            for (int r = 0; r < 2048; r += 3)
                for (int c = 0; c < 2048; c += 5) d2dh::text_colour(lines.data(), s, r, c);
        CHECK(d2dh::text_colour(nullptr, 1, 0, 0) == d2dr::C_BG);
        CHECK(d2dh::text_colour(lines.data(), 1, 1, 6 * D2DH_LINE_CHARS) == d2dr::C_BG);
    }
    // ---- frames
    const int sizes[2][2] = {{8, 8}, {97, 61}};
    for (const auto& wh : sizes) {
        const int W = wh[0], H = wh[1];
        for (int nc : {0, 64}) {
            std::snprintf(g_case, sizeof g_case, "%dx%d circles=%d", W, H, nc);
            const int n = 3, T = 12, S = 5;
            std::vector<d2d_scn> scn((size_t)n, make_scn(nc));
            std::vector<double> st((size_t)D2D_NSTATE * n, 0.0);
            set_pose(st, n, 0, 400, 600, 0.3, 60, -30);
            set_pose(st, n, 1, 5000, -4000, -1.2, 10, 10);  // wholly outside the screen
            set_pose(st, n, 2, 700, 300, 0.0, 0, 0);        // zero-length velocity
            std::vector<float> obs((size_t)n * D2D_OBS_DIM, 0.1f), act((size_t)n * 2, 0.25f);
            std::vector<float> trail((size_t)n * T * 2);
            for (size_t k = 0; k < trail.size(); ++k) trail[k] = 100.0f + 37.0f * (float)(k % 29);
            const int32_t tl[3] = {T, 5, 0};
            std::vector<float> info((size_t)n * D2D_INFO_DIM);
            for (size_t k = 0; k < info.size(); ++k) info[k] = -3.0f + 0.37f * (float)k;
            std::vector<double> shade((size_t)n * S * 3);
            for (size_t k = 0; k < shade.size(); k += 3) shade[k] = 100.0 + 31.0 * (double)k, shade[k + 1] = 1200.0 - 29.0 * (double)k, shade[k + 2] = 0.01 * (double)k;
            const Inputs full = {obs.data(), act.data(), trail.data(), tl, T, info.data(), shade.data(), nullptr, S};
            // layers off: d2d_raster.h's own twin, byte for byte, whatever else is given
            for (uint32_t l : {0u, 1u, 2u, 4u, 8u, 16u, 32u, 63u}) {
                d2dr_view v = {W, H, SW, SH, l, 0};
                std::vector<uint8_t> base((size_t)n * W * H * 3);
                d2dr::render_host(&v, n, scn.data(), st.data(), obs.data(), act.data(), trail.data(), tl, T, base.data());
                for (int32_t cnt : {0, 2, S, S + 7, -4}) {
                    const int32_t count[3] = {cnt, cnt, cnt};
                    Inputs in = full;
                    in.count = count;
                    CHECK(render(W, H, n, scn, st, in, l) == base);
                }
                const Inputs bare = {obs.data(), act.data(), trail.data(), tl, T, nullptr, nullptr, nullptr, 0};
                CHECK(render(W, H, n, scn, st, bare, l) == base);
            }
            // every new bit alone, with the base layers, and all; NULL inputs each alone
            const int32_t count[3] = {S + 7, 2, 0};
            Inputs in = full;
            in.count = count;
            for (uint32_t l : {64u, 128u, 256u, 63u | 64u, 63u | 128u, 63u | 256u, 511u}) render(W, H, n, scn, st, in, l);
            for (int m = 0; m < 16; ++m) {
                Inputs q = in;
                if (m & 1) q.obs = nullptr;
                if (m & 2) q.trail = nullptr, q.tl = nullptr;
                if (m & 4) q.info = nullptr;
                if (m & 8) q.shade = nullptr, q.count = nullptr, q.max_shades = 0;
                render(W, H, n, scn, st, q, 511u);
            }
            // NaN, +-inf and 1e300 everywhere: no loop, no write out of range, nothing drawn by a bad shade
            const auto no_shades = render(W, H, n, scn, st, {obs.data(), act.data(), trail.data(), tl, T, nullptr, nullptr, nullptr, 0}, 63u | 128u | 256u);
            for (double bad : {nan, inf, -inf, 1e300, -1e300}) {
                for (int f = 0; f < 18; ++f) {
                    std::snprintf(g_case, sizeof g_case, "%dx%d circles=%d field %d = %g", W, H, nc, f, bad);
                    std::vector<double> s2 = st;
                    for (int e = 0; e < n; ++e) s2[(size_t)f * n + (size_t)e] = bad;
                    render(W, H, n, scn, s2, in, 511u);
                }
                std::vector<float> o2(obs.size(), (float)bad), i2(info.size(), (float)bad);
                std::vector<double> h2(shade.size(), bad);
                Inputs q = in;
                q.obs = o2.data(), q.info = i2.data(), q.shade = h2.data();
                render(W, H, n, scn, st, q, 511u);
                Inputs r = {obs.data(), act.data(), trail.data(), tl, T, nullptr, h2.data(), count, S};
                CHECK(render(W, H, n, scn, st, r, 63u | 128u | 256u) == no_shades);
            }
            std::snprintf(g_case, sizeof g_case, "%dx%d n_frames=0", W, H);
            CHECK(render(W, H, 0, scn, st, in, 511u).empty());
        }
    }
    // ---- the recorder: restart, append, overflow, an id at each end of the batch
    {
        std::snprintf(g_case, sizeof g_case, "recorder");
        const int N = 5, K = 2, S = 3;
        const int32_t ids[K] = {0, N - 1};
        std::vector<double> st((size_t)D2D_NSTATE * N, 0.0), shade((size_t)K * S * 3, -1.0), last((size_t)K * 2, -1.0);
        std::vector<int32_t> count(K, 99);
        std::vector<uint8_t> term(N, 0), trunc(N, 0);
        d2dh::shade_step(0, ids, N, st.data(), nullptr, nullptr, 75.0, S, shade.data(), count.data(), last.data());
        d2dh::shade_step(1, ids, N, st.data(), nullptr, nullptr, 75.0, S, shade.data(), count.data(), last.data());
        CHECK(count[0] == 1 && count[1] == 1 && shade[0] == 0.0 && shade[3] == -1.0);
        for (int step = 1; step <= 6; ++step) {
            st[0] = 80.0 * step, st[(size_t)N + (N - 1)] = -80.0 * step;  // env 0 moves in x, env N-1 in y
            for (int k = 0; k < K; ++k)
                d2dh::shade_step(k, ids, N, st.data(), term.data(), trunc.data(), 75.0, S, shade.data(), count.data(), last.data());
        }
        CHECK(count[0] == 7 && count[1] == 7 && shade[6] == 160.0 && last[0] == 480.0 && last[3] == -480.0);
        trunc[N - 1] = 1;
        for (int k = 0; k < K; ++k)
            d2dh::shade_step(k, ids, N, st.data(), term.data(), trunc.data(), 75.0, S, shade.data(), count.data(), last.data());
        CHECK(count[0] == 7 && count[1] == 1 && shade[(size_t)S * 3 + 1] == -480.0);
        const int32_t outside[1] = {N};
        d2dh::shade_step(0, outside, N, st.data(), nullptr, nullptr, 75.0, S, shade.data(), count.data(), last.data());
        CHECK(count[0] == 7);
    }
    std::puts("hud host code: ok");
    return 0;
}
