// Stand-alone host program over csrc/render/d2d_raster.h (built with the address and undefined-behaviour
// sanitizers by tests/test_render.py::test_render_host_code_sanitized): the renderer's primitive
// construction, coverage predicate and CPU twins on the edge cases -- smallest and odd picture sizes,
// 0 and 64 circles, trails of 0, 1, 2 and max_trail points, NaN / +-inf / 1e300 in every state field,
// a drone wholly outside the screen, a zero-length velocity, n_frames = 0, the plot with paths of every
// short length.  Exit status 0: every check held and the sanitizers saw nothing.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "render/d2d_raster.h"

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
    // Lagrange form of the parabola through the three (u, w) pairs
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

// the state column of a drone at (x, y, angle) with velocity (vx, vy), motors at +-40 along the frame
static void set_pose(std::vector<double>& st, int n, int f, double x, double y, double a, double vx, double vy) {
    const double c = std::cos(a), s = std::sin(a);
    const double v[18] = {x, y, a, vx, vy, 0.1, x - 40 * c, y - 40 * s, a, vx, vy, 0, x + 40 * c, y + 40 * s, a, vx, vy, 0};
    for (int k = 0; k < 18; ++k) st[(size_t)k * (size_t)n + (size_t)f] = v[k];
}

static std::vector<uint8_t> render(int W, int H, int n, const std::vector<d2d_scn>& scn, const std::vector<double>& st,
                                   const float* obs, const float* act, const float* trail, const int32_t* tl,
                                   int max_trail, uint32_t layers = D2DR_L_ALL) {
    d2dr_view v = {W, H, SW, SH, layers, 0};
    std::vector<uint8_t> out((size_t)n * (size_t)W * (size_t)H * 3 + 64, 0x5a);  // 64 canary bytes behind
    d2dr::render_host(&v, n, scn.data(), st.data(), obs, act, trail, tl, max_trail, out.data());
    for (size_t k = out.size() - 64; k < out.size(); ++k) CHECK(out[k] == 0x5a);
    out.resize(out.size() - 64);
    return out;
}

static bool all_background(const std::vector<uint8_t>& img) {
    for (uint8_t b : img)
        if (b != 243) return false;
    return true;
}

int main() {
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    const int sizes[2][2] = {{8, 8}, {50, 70}};
    for (const auto& wh : sizes) {
        const int W = wh[0], H = wh[1];
        for (int nc : {0, 64}) {
            std::snprintf(g_case, sizeof g_case, "%dx%d circles=%d", W, H, nc);
            const int n = 3, T = 12;
            std::vector<d2d_scn> scn((size_t)n, make_scn(nc));
            std::vector<double> st((size_t)D2D_NSTATE * n, 0.0);
            set_pose(st, n, 0, 400, 600, 0.3, 60, -30);
            set_pose(st, n, 1, 5000, -4000, -1.2, 10, 10);  // wholly outside the screen
            set_pose(st, n, 2, 700, 300, 0.0, 0, 0);        // zero-length velocity
            std::vector<float> obs((size_t)n * D2D_OBS_DIM, 0.1f), act((size_t)n * 2, 0.25f);
            std::vector<float> trail((size_t)n * T * 2);
            for (size_t k = 0; k < trail.size(); ++k) trail[k] = 100.0f + 37.0f * (float)(k % 29);
            for (int len : {0, 1, 2, T, T + 5, -3}) {  // beyond max_trail counts as max_trail, below 0 as 0
                const int32_t tl[3] = {len, len, len};
                const auto img = render(W, H, n, scn, st, obs.data(), act.data(), trail.data(), tl, T);
                const auto no_trail = render(W, H, n, scn, st, obs.data(), act.data(), trail.data(), tl, T,
                                             D2DR_L_ALL & ~D2DR_L_TRAIL);
                if (len < 2) CHECK(img == no_trail);  // fewer than 2 points draw nothing
            }
            // NULL obs / act / trail, each alone and together; every layer alone
            const int32_t tl[3] = {T, T, T};
            for (int m = 0; m < 8; ++m)
                render(W, H, n, scn, st, (m & 1) ? nullptr : obs.data(), (m & 2) ? nullptr : act.data(),
                       (m & 4) ? nullptr : trail.data(), (m & 4) ? nullptr : tl, T);
            for (uint32_t l = 1; l <= D2DR_L_TRAIL; l <<= 1)
                render(W, H, n, scn, st, obs.data(), act.data(), trail.data(), tl, T, l);
            CHECK(all_background(render(W, H, n, scn, st, obs.data(), act.data(), trail.data(), tl, T, 0u)));
            // NaN, +-inf and 1e300 in every state field (and in obs / act / trail): no loop, no write out of range
            for (double bad : {nan, inf, -inf, 1e300, -1e300}) {
                for (int f = 0; f < 18; ++f) {
                    std::snprintf(g_case, sizeof g_case, "%dx%d circles=%d field %d = %g", W, H, nc, f, bad);
                    std::vector<double> s2 = st;
                    for (int e = 0; e < n; ++e) s2[(size_t)f * n + (size_t)e] = bad;
                    render(W, H, n, scn, s2, obs.data(), act.data(), trail.data(), tl, T);
                }
                std::vector<float> o2(obs.size(), (float)bad), a2(act.size(), (float)bad), t2(trail.size(), (float)bad);
                render(W, H, n, scn, st, o2.data(), a2.data(), t2.data(), tl, T);
                std::vector<double> s3(st.size(), bad);  // every field at once: only the scenario is left
                const auto only_scn = render(W, H, n, scn, s3, nullptr, nullptr, nullptr, nullptr, 0);
                CHECK(only_scn == render(W, H, n, scn, st, nullptr, nullptr, nullptr, nullptr, 0,
                                         D2DR_L_PATH | D2DR_L_OBSTACLES | D2DR_L_FORCES));  // + the target dot
                d2d_scn bs = make_scn(nc);  // and a scenario of nothing but `bad`
                const std::vector<double> fill((sizeof bs - 8) / sizeof(double), bad);  // all but n_wps, n_circles
                std::memcpy(reinterpret_cast<char*>(&bs) + 8, fill.data(), sizeof bs - 8);
                std::vector<d2d_scn> bscn((size_t)n, bs);
                render(W, H, n, bscn, st, obs.data(), act.data(), trail.data(), tl, T);
            }
            // n_frames = 0 touches nothing
            std::snprintf(g_case, sizeof g_case, "%dx%d n_frames=0", W, H);
            CHECK(render(W, H, 0, scn, st, nullptr, nullptr, nullptr, nullptr, 0).empty());
            // the plot: paths of 0, 1, 2 points draw nothing; 3 and max_len points do; NaN points cover nothing
            const int P = 6, L = 9;
            std::vector<float> xy((size_t)L * P * 2);
            for (int j = 0; j < L; ++j)
                for (int m = 0; m < P; ++m) xy[2 * ((size_t)j * P + m)] = 100.0f + 130.0f * j, xy[2 * ((size_t)j * P + m) + 1] = 650.0f;
            std::vector<uint8_t> rgb((size_t)P * 3, 7);
            d2dr_view v = {W, H, SW, SH, D2DR_L_ALL, 0};
            std::vector<uint8_t> blank((size_t)W * H * 3), shorts(blank.size()), full(blank.size());
            const int32_t none[P] = {0, 0, 0, 0, 0, 0}, shrt[P] = {0, 1, 2, 2, 1, 0}, lens[P] = {0, 1, 2, 3, L, L + 4};
            d2dr::plot_paths_host(&v, scn.data(), xy.data(), none, rgb.data(), P, L, blank.data());
            d2dr::plot_paths_host(&v, scn.data(), xy.data(), shrt, rgb.data(), P, L, shorts.data());
            d2dr::plot_paths_host(&v, scn.data(), xy.data(), lens, rgb.data(), P, L, full.data());
            CHECK(blank == shorts && blank != full);
            for (float& f : xy) f = (float)nan;
            d2dr::plot_paths_host(&v, nullptr, xy.data(), lens, rgb.data(), P, L, full.data());
            d2dr::plot_paths_host(&v, nullptr, xy.data(), none, rgb.data(), P, L, shorts.data());
            CHECK(full == shorts);
        }
    }
    std::puts("render host code: ok");
    return 0;
}
