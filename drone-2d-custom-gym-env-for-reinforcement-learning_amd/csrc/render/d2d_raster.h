/* d2d_raster.h -- the renderer's shared host/device code (include/d2d_render.h has the picture model).
 *
 * Three things live here, each compiled once for the device (csrc/render/d2d_render.hip's kernels)
 * and once for the host (the d2dr_*_host twins and tests/render_host_main.cpp):
 *   build_prim      one primitive of a frame's list from its slot number, in fp64, rounded once to fp32
 *   covers          the fp32 coverage predicate (add, mul, div, compare only)
 *   render_host ... the CPU twins: the same list, the same predicate, the same last-wins resolve
 * Compile with -ffp-contract=off on both sides: host and device then round identically.
 * A fourth, for the device alone (at the end, under __HIPCC__): the 64 x 4 tile walk over a primitive
 * list, which d2d_render.hip and csrc/hud/d2d_hud.hip both instantiate.
 */
#ifndef D2D_RASTER_H
#define D2D_RASTER_H

#include <math.h>
#include <stdint.h>

#include <vector>

#include "../../../include/d2d_render.h"
#include "../../../include/drone2d.h"
#include "../d2d_pmath.h"

#if defined(__HIPCC__)
#define D2DR_FN __host__ __device__ static inline
#else
#define D2DR_FN static inline
#endif

namespace d2dr {

enum { K_NONE = 0, K_CIRCLE = 1, K_CAPSULE = 2, K_BOX = 3 };

/* One primitive, 48 bytes.  p: circle (cx, cy, r^2); capsule (ax, ay, dx, dy, len^2, hw^2); box
 * (cx, cy, cos, sin, hx, hy).  rgbk = r | g << 8 | b << 16 | kind << 24.  [c0, c1] x [r0, r1]: the
 * pixels (inclusive, inside the picture) outside which the primitive covers nothing -- part of the
 * predicate, so culling by it never changes a picture.  The raster kernel moves a primitive as three
 * 16-byte words and reads kind and pixel box out of them: keep the layout. */
struct alignas(16) Prim {
    float p[6];
    uint32_t rgbk;
    int32_t c0, c1, r0, r1;
    uint32_t pad;
};
static_assert(sizeof(Prim) == 48, "Prim is three 16-byte words");

/* slot numbers of a frame's list = painter's order */
enum {
    S_PATH = 0,                               /* 99 capsules */
    S_DOT0 = D2DR_PATH_SAMPLES - 1, S_DOT1,   /* path(us[0]), wp_last */
    S_SPAWN,                                  /* 4 capsules */
    S_CLOSE = S_SPAWN + 4, S_LA_LINE, S_LA_DOT, S_VEL, S_NEAR,
    S_CIRC,                                   /* D2D_MAX_CIRCLES circles */
    S_FRAME = S_CIRC + D2D_MAX_CIRCLES, S_ML, S_MR,
    S_FORCE,                                  /* grey L, red L, grey R, red R */
    S_TARGET = S_FORCE + 4,
    S_TRAIL,                                  /* trail_len - 1 capsules; the plot: D2DR_BAR_ROWS bar rows */
    N_FIXED = S_TRAIL
};

#define D2DR_RGB(r, g, b) ((uint32_t)(r) | ((uint32_t)(g) << 8) | ((uint32_t)(b) << 16))
static constexpr uint32_t C_BG = D2DR_RGB(243, 243, 243), C_BLACK = D2DR_RGB(0, 0, 0), C_BLUE = D2DR_RGB(0, 0, 255),
                          C_LA = D2DR_RGB(0, 150, 150), C_RED = D2DR_RGB(255, 0, 0), C_GREEN = D2DR_RGB(0, 255, 0),
                          C_OBST = D2DR_RGB(188, 72, 72), C_BODY = D2DR_RGB(66, 135, 245),
                          C_MOTOR = D2DR_RGB(33, 93, 191), C_GREY = D2DR_RGB(179, 179, 179),
                          C_TRAIL = D2DR_RGB(16, 19, 97);

/* The view in the forms the two stages use (fp64 for the list, fp32 for the pixels). */
struct View {
    int32_t W, H;
    uint32_t layers;
    int32_t plot;      /* 1: the plot's background list (no spawn rectangle; bar rows in the trail slots) */
    double sw, sh;     /* world extent */
    double px, py;     /* one pixel in world units, x and y */
    float pxf, pyf, shf;
};

D2DR_FN View make_view(const d2dr_view* v, int plot) {
    View o;
    o.W = v->width, o.H = v->height;
    o.layers = plot ? (D2DR_L_PATH | D2DR_L_OBSTACLES) : v->layers;
    o.plot = plot;
    o.sw = v->screen_w, o.sh = v->screen_h;
    o.px = v->screen_w / (double)v->width;
    o.py = v->screen_h / (double)v->height;
    o.pxf = (float)o.px, o.pyf = (float)o.py, o.shf = (float)o.sh;
    return o;
}

/* What one frame's list is built from (device or host pointers alike). */
struct FrameIn {
    const d2d_scn* scn;   /* this frame's record, or NULL (blank plot) */
    const double* state;  /* SoA base; field f of this frame at state[f * stride + frame] */
    int32_t stride, frame;
    const float* obs;     /* this frame's 27 floats or NULL */
    const float* act;     /* this frame's 2 floats or NULL */
    const float* trail;   /* this frame's points or NULL */
    int32_t trail_len;    /* clamped to [0, max_trail] */
};

D2DR_FN bool finite_d(double x) { return x - x == 0.0; }
D2DR_FN bool finite_f(float x) { return x - x == 0.0f; }
D2DR_FN double clamp_d(double x, double lo, double hi) {  /* NaN -> lo */
    double v = (x > lo) ? x : lo;
    return (v < hi) ? v : hi;
}
D2DR_FN double abs_d(double x) { return (x < 0.0) ? -x : x; }
/* floor of v in [-4, 2^30) as an int (v already clamped: out-of-range conversions are undefined on the
 * host and saturate on the device) */
D2DR_FN int32_t floor_i(double v) { return (int32_t)(v + 4.0) - 4; }

D2DR_FN Prim none_prim() {
    Prim q;
    q.p[0] = q.p[1] = q.p[2] = q.p[3] = q.p[4] = q.p[5] = 0.0f;
    q.rgbk = 0u;
    q.c0 = q.r0 = 1;
    q.c1 = q.r1 = 0;
    q.pad = 0u;
    return q;
}

/* Finish a primitive: the pixel box of the world box [x0, x1] x [y0, y1] (two pixels of slack for the
 * fp32 pixel centres), NONE if a parameter is not finite or the box misses the picture. */
D2DR_FN Prim finish(Prim q, uint32_t rgb, int kind, double x0, double x1, double y0, double y1, const View& v) {
    bool ok = finite_d(x0) && finite_d(x1) && finite_d(y0) && finite_d(y1);
    for (int k = 0; k < 6; ++k) ok = ok && finite_f(q.p[k]);
    if (!ok) return none_prim();
    const double W = (double)v.W, H = (double)v.H;
    q.c0 = floor_i(clamp_d(x0 / v.px - 0.5, -2.0, W + 2.0)) - 1;
    q.c1 = floor_i(clamp_d(x1 / v.px - 0.5, -2.0, W + 2.0)) + 2;
    q.r0 = floor_i(clamp_d((v.sh - y1) / v.py - 0.5, -2.0, H + 2.0)) - 1;
    q.r1 = floor_i(clamp_d((v.sh - y0) / v.py - 0.5, -2.0, H + 2.0)) + 2;
    if (q.c0 < 0) q.c0 = 0;
    if (q.r0 < 0) q.r0 = 0;
    if (q.c1 > v.W - 1) q.c1 = v.W - 1;
    if (q.r1 > v.H - 1) q.r1 = v.H - 1;
    if (q.c1 < q.c0 || q.r1 < q.r0) return none_prim();
    q.rgbk = rgb | ((uint32_t)kind << 24);
    q.pad = 0u;
    return q;
}

D2DR_FN Prim make_circle(double cx, double cy, double r_ref, uint32_t rgb, const View& v, bool dot) {
    const double r = (dot && !(r_ref > v.px)) ? v.px : r_ref;  /* a dot's r = max(r_ref, px) */
    Prim q = none_prim();
    q.p[0] = (float)cx, q.p[1] = (float)cy, q.p[2] = (float)(r * r);
    return finish(q, rgb, K_CIRCLE, cx - r, cx + r, cy - r, cy + r, v);
}

D2DR_FN Prim make_capsule(double ax, double ay, double bx, double by, double w_ref, uint32_t rgb, const View& v) {
    const double fl = 0.75 * v.px, h0 = 0.5 * w_ref;
    const double hw = (h0 > fl) ? h0 : fl;  /* hw = max(w_ref / 2, 0.75 px) */
    const double dx = bx - ax, dy = by - ay;
    Prim q = none_prim();
    q.p[0] = (float)ax, q.p[1] = (float)ay, q.p[2] = (float)dx, q.p[3] = (float)dy;
    q.p[4] = (float)(dx * dx + dy * dy), q.p[5] = (float)(hw * hw);
    const double x0 = (ax < bx) ? ax : bx, x1 = (ax < bx) ? bx : ax;
    const double y0 = (ay < by) ? ay : by, y1 = (ay < by) ? by : ay;
    return finish(q, rgb, K_CAPSULE, x0 - hw, x1 + hw, y0 - hw, y1 + hw, v);
}

D2DR_FN Prim make_box(double cx, double cy, double angle, double hx, double hy, uint32_t rgb, const View& v) {
    if (!(abs_d(angle) <= 8.0)) return none_prim();  /* d2d_pm_sincos' range; NaN lands here too */
    double s, c;
    d2d_pm_sincos(angle, &s, &c);
    Prim q = none_prim();
    q.p[0] = (float)cx, q.p[1] = (float)cy, q.p[2] = (float)c, q.p[3] = (float)s, q.p[4] = (float)hx, q.p[5] = (float)hy;
    const double ex = abs_d(c) * hx + abs_d(s) * hy, ey = abs_d(s) * hx + abs_d(c) * hy;
    return finish(q, rgb, K_BOX, cx - ex, cx + ex, cy - ey, cy + ey, v);
}

/* The coverage predicate: does primitive q cover the centre (x, y) of pixel (row, col)? */
D2DR_FN bool covers(const Prim& q, int32_t row, int32_t col, float x, float y) {
    if (col < q.c0 || col > q.c1 || row < q.r0 || row > q.r1) return false;
    const int kind = (int)(q.rgbk >> 24);
    const float wx = x - q.p[0], wy = y - q.p[1];
    if (kind == K_CIRCLE) return wx * wx + wy * wy <= q.p[2];
    if (kind == K_CAPSULE) {
        const float dx = q.p[2], dy = q.p[3], l2 = q.p[4];
        float t = 0.0f;
        if (l2 > 0.0f) {
            t = (wx * dx + wy * dy) / l2;
            t = (t > 0.0f) ? t : 0.0f;
            t = (t < 1.0f) ? t : 1.0f;
        }
        const float ex = wx - t * dx, ey = wy - t * dy;
        return ex * ex + ey * ey <= q.p[5];
    }
    if (kind == K_BOX) {
        const float c = q.p[2], s = q.p[3];
        const float u = wx * c + wy * s, w = wy * c - wx * s;
        return u <= q.p[4] && -u <= q.p[4] && w <= q.p[5] && -w <= q.p[5];
    }
    return false;
}
D2DR_FN float pixel_x(const View& v, int32_t col) { return ((float)col + 0.5f) * v.pxf; }
D2DR_FN float pixel_y(const View& v, int32_t row) { return v.shf - ((float)row + 0.5f) * v.pyf; }

/* ---- QPMI2D from the ABI record (predef_path.py:88-142) ------------------------------ */
D2DR_FN int32_t path_nw(const d2d_scn* s) {
    const int32_t n = s->n_wps;
    return n < 3 ? 3 : (n > D2D_MAX_WPS ? D2D_MAX_WPS : n);
}
D2DR_FN int32_t u_index(const d2d_scn* s, int32_t nw, double u) {
    int32_t n = 0;
    while (n < nw - 1) {
        if (u <= s->us[n + 1]) break;
        ++n;
    }
    return n;
}
D2DR_FN void seg_eval(const d2d_scn* s, int32_t k, double u, double* x, double* y) {
    const double u2 = u * u;
    *x = s->xa[k] * u2 + s->xb[k] * u + s->xc[k];
    *y = s->ya[k] * u2 + s->yb[k] * u + s->yc[k];
}
D2DR_FN void path_eval(const d2d_scn* s, double u, double* x, double* y) {
    const int32_t nw = path_nw(s), last = nw - 3;
    if (u >= s->us[0] && u <= s->us[1]) {
        seg_eval(s, 0, u, x, y);
        return;
    }
    const int32_t n = u_index(s, nw, u);
    if ((u >= s->us[nw - 2] - 0.001 && u <= s->us[nw - 1]) || n == nw - 1) {
        seg_eval(s, last, u, x, y);
        return;
    }
    const double den = s->us[n + 1] - s->us[n];
    const double mu_r = (u - s->us[n]) / den, mu_f = (s->us[n + 1] - u) / den;
    double x1, y1, x2, y2;
    seg_eval(s, n >= 1 ? n - 1 : last, u, &x1, &y1);  /* n = 0 (u < us[0]) blends the last stretch, as a[-1] does */
    seg_eval(s, n <= last ? n : last, u, &x2, &y2);
    *x = mu_r * x2 + mu_f * x1;
    *y = mu_r * y2 + mu_f * y1;
}
/* sample k of np.linspace(us[0], us[-1], 100) (get_path_coord, predef_path.py:297-304) */
D2DR_FN void path_sample(const d2d_scn* s, int32_t k, double* x, double* y) {
    const int32_t nw = path_nw(s);
    const double u0 = s->us[0], u1 = s->us[nw - 1];
    const double step = (u1 - u0) / (double)(D2DR_PATH_SAMPLES - 1);
    path_eval(s, k == D2DR_PATH_SAMPLES - 1 ? u1 : u0 + (double)k * step, x, y);
}

/* the obstacle with the least min over the unrotated vertices of |v + p - c| - r; lowest
 * index on ties; -1 without obstacles (or when nothing compares) */
D2DR_FN int32_t nearest_circle(const d2d_scn* s, double px, double py) {
    int32_t nc = s->n_circles;
    nc = nc < 0 ? 0 : (nc > D2D_MAX_CIRCLES ? D2D_MAX_CIRCLES : nc);
    int32_t best = -1;
    double bd = 0.0;
    for (int32_t i = 0; i < nc; ++i) {
        double m2 = 0.0;
        for (int k = 0; k < 4; ++k) {
            const double ex = px + ((k & 1) ? 50.0 : -50.0) - s->cx[i], ey = py + ((k & 2) ? 5.0 : -5.0) - s->cy[i];
            const double d2 = ex * ex + ey * ey;
            if (k == 0 || d2 < m2) m2 = d2;
        }
        const double d = sqrt(m2) - s->cr[i];
        if (finite_d(d) && (best < 0 || d < bd)) best = i, bd = d;
    }
    return best;
}

D2DR_FN double st(const FrameIn& in, int f) { return in.state[(size_t)f * (size_t)in.stride + (size_t)in.frame]; }

/* red_blue_grad of main.py:18-31 as bytes: (255, 0, 510 f) below one half, (510 (1 - f), 0, 255) from it */
D2DR_FN uint32_t red_blue_grad(double f) {
    if (f < 0.5) return D2DR_RGB(255, 0, (uint32_t)clamp_d(255.0 * f * 2.0, 0.0, 255.0));
    return D2DR_RGB((uint32_t)clamp_d(255.0 * (1.0 - f) * 2.0, 0.0, 255.0), 0, 255);
}

/* Primitive `slot` of a frame's list. */
D2DR_FN Prim build_prim(const FrameIn& in, const View& v, int32_t slot) {
    const d2d_scn* s = in.scn;
    const uint32_t L = v.layers;
    if (slot >= S_TRAIL) {
        const int32_t j = slot - S_TRAIL;
        if (v.plot) {  /* colour bar, main.py:387-388: row i from (sw - 100, 900 + i) to (sw - 50, 900 + i) */
            if (j >= D2DR_BAR_ROWS) return none_prim();
            const double y = 900.0 + (double)j;
            return make_capsule(v.sw - 100.0, y, v.sw - 50.0, y, 1.0, red_blue_grad((double)j / 100.0), v);
        }
        if (!(L & D2DR_L_TRAIL) || in.trail == nullptr || j + 1 >= in.trail_len) return none_prim();
        const float* t = in.trail + 2 * (size_t)j;
        return make_capsule((double)t[0], (double)t[1], (double)t[2], (double)t[3], 1.0, C_TRAIL, v);
    }
    if (s == nullptr) return none_prim();
    if (slot < S_SPAWN) {
        if (!(L & D2DR_L_PATH)) return none_prim();
        double x0, y0, x1, y1;
        if (slot < S_DOT0) {
            path_sample(s, slot, &x0, &y0);
            path_sample(s, slot + 1, &x1, &y1);
            return make_capsule(x0, y0, x1, y1, 1.0, C_BLACK, v);
        }
        if (slot == S_DOT0) {
            path_sample(s, 0, &x0, &y0);
            return make_circle(x0, y0, 5.0, C_BLACK, v, true);
        }
        return make_circle(s->wp_last_x, s->wp_last_y, 5.0, C_BLACK, v, true);
    }
    if (slot < S_CLOSE) {
        if (!(L & D2DR_L_PATH) || v.plot) return none_prim();
        const double xa = s->spawn_xmin, xb = s->spawn_xmax, ya = s->spawn_ymin, yb = s->spawn_ymax;
        const int k = slot - S_SPAWN;
        if (k == 0) return make_capsule(xa, ya, xb, ya, 2.0, C_BLACK, v);
        if (k == 1) return make_capsule(xb, ya, xb, yb, 2.0, C_BLACK, v);
        if (k == 2) return make_capsule(xb, yb, xa, yb, 2.0, C_BLACK, v);
        return make_capsule(xa, yb, xa, ya, 2.0, C_BLACK, v);
    }
    if (slot >= S_CIRC && slot < S_FRAME) {
        const int32_t i = slot - S_CIRC;
        if (!(L & D2DR_L_OBSTACLES) || i >= s->n_circles) return none_prim();
        return make_circle(s->cx[i], s->cy[i], s->cr[i], C_OBST, v, false);
    }
    if (in.state == nullptr) return none_prim();
    const double x = st(in, D2D_S_F), y = st(in, D2D_S_F + 1);
    if (slot < S_CIRC) {
        if (!(L & D2DR_L_GUIDES)) return none_prim();
        if (slot == S_VEL) return make_capsule(x, y, x + st(in, D2D_S_F + 3), y + st(in, D2D_S_F + 4), 4.0, C_RED, v);
        if (slot == S_NEAR) {
            const int32_t i = nearest_circle(s, x, y);
            if (i < 0) return none_prim();
            return make_capsule(x, y, s->cx[i], s->cy[i], 4.0, C_GREEN, v);
        }
        if (in.obs == nullptr) return none_prim();
        if (slot == S_CLOSE)
            return make_circle(((double)in.obs[19] + 1.0) * v.sw * 0.5, ((double)in.obs[20] + 1.0) * v.sh * 0.5, 5.0,
                               C_BLUE, v, true);
        const double lx = ((double)in.obs[21] + 1.0) * v.sw * 0.5, ly = ((double)in.obs[22] + 1.0) * v.sh * 0.5;
        if (slot == S_LA_LINE) return make_capsule(x, y, lx, ly, 4.0, C_LA, v);
        return make_circle(lx, ly, 5.0, C_LA, v, true);
    }
    if (slot == S_FRAME || slot == S_ML || slot == S_MR) {
        if (!(L & D2DR_L_DRONE)) return none_prim();
        if (slot == S_FRAME) return make_box(x, y, st(in, D2D_S_F + 2), 50.0, 5.0, C_BODY, v);
        const int b = (slot == S_ML) ? D2D_S_L : D2D_S_R;
        return make_box(st(in, b), st(in, b + 1), st(in, b + 2), 10.0, 10.0, C_MOTOR, v);
    }
    if (!(L & D2DR_L_FORCES)) return none_prim();
    if (slot == S_TARGET) return make_circle(s->wp_last_x, s->wp_last_y, 5.0, C_RED, v, true);
    /* force vectors at frame-local (-+40, 0): grey to (-+40, 50), red to (-+40, F 0.05) */
    if (in.act == nullptr) return none_prim();
    const double ang = st(in, D2D_S_F + 2);
    if (!(abs_d(ang) <= 8.0)) return none_prim();
    double sn, cs;
    d2d_pm_sincos(ang, &sn, &cs);
    const int k = slot - S_FORCE;
    const double lx = (k < 2) ? -40.0 : 40.0;
    const double F = ((double)in.act[k >> 1] / 2.0 + 0.5) * 1000.0;
    const double ly = (k & 1) ? F * 0.05 : 50.0;
    const double ax = x + cs * lx, ay = y + sn * lx;
    return make_capsule(ax, ay, x + (cs * lx - sn * ly), y + (sn * lx + cs * ly), 4.0, (k & 1) ? C_RED : C_GREY, v);
}

D2DR_FN int32_t clamp_len(int32_t n, int32_t cap) { return n < 0 ? 0 : (n > cap ? cap : n); }
/* segment j of plot path m (points j, j + 1 of xy [max_len][n_paths][2]); NONE past the path's end or
 * when the path has no more than 2 points (main.py:378) */
D2DR_FN Prim plot_segment(const float* xy, int32_t len, int32_t n_paths, int32_t m, int32_t j, const View& v) {
    if (len <= 2 || j + 1 >= len) return none_prim();
    const float* a = xy + 2 * ((size_t)j * (size_t)n_paths + (size_t)m);
    const float* b = a + 2 * (size_t)n_paths;
    return make_capsule((double)a[0], (double)a[1], (double)b[0], (double)b[1], 1.0, 0u, v);
}

/* ---- CPU twins ---------------------------------------------------------------------------------- */
/* Resolve one picture from its list: per pixel the last covering primitive of prims[lo, hi), top
 * first; ids (the plot) sit between the list's fixed part and its bar rows. */
inline void resolve_host(const std::vector<Prim>& prims, const View& v, const uint32_t* ids, const uint8_t* rgb,
                         uint8_t* out) {
    std::vector<int32_t> live;
    for (int32_t r = 0; r < v.H; ++r) {
        live.clear();
        for (int32_t k = (int32_t)prims.size() - 1; k >= 0; --k)
            if ((prims[(size_t)k].rgbk >> 24) != K_NONE && r >= prims[(size_t)k].r0 && r <= prims[(size_t)k].r1)
                live.push_back(k);
        const float y = pixel_y(v, r);
        for (int32_t c = 0; c < v.W; ++c) {
            const float x = pixel_x(v, c);
            uint32_t col = C_BG;
            bool hit = false;
            size_t i = 0;
            for (; i < live.size() && live[i] >= N_FIXED; ++i)
                if (covers(prims[(size_t)live[i]], r, c, x, y)) {
                    col = prims[(size_t)live[i]].rgbk, hit = true;
                    break;
                }
            if (!hit && ids != nullptr) {
                const uint32_t id = ids[(size_t)r * (size_t)v.W + (size_t)c];
                if (id > 0u) {
                    const uint8_t* q = rgb + 3 * (size_t)(id - 1u);
                    col = D2DR_RGB(q[0], q[1], q[2]), hit = true;
                }
            }
            if (!hit) {
                while (i < live.size() && live[i] >= N_FIXED) ++i;
                for (; i < live.size(); ++i)
                    if (covers(prims[(size_t)live[i]], r, c, x, y)) {
                        col = prims[(size_t)live[i]].rgbk;
                        break;
                    }
            }
            uint8_t* o = out + 3 * ((size_t)r * (size_t)v.W + (size_t)c);
            o[0] = (uint8_t)(col & 255u), o[1] = (uint8_t)((col >> 8) & 255u), o[2] = (uint8_t)((col >> 16) & 255u);
        }
    }
}

inline void render_host(const d2dr_view* view, int32_t n_frames, const d2d_scn* scn, const double* state,
                        const float* obs, const float* act, const float* trail, const int32_t* trail_len,
                        int32_t max_trail, uint8_t* out) {
    const View v = make_view(view, 0);
    const bool tr = trail != nullptr && trail_len != nullptr;
    std::vector<Prim> prims;
    for (int32_t f = 0; f < n_frames; ++f) {
        FrameIn in;
        in.scn = scn + f, in.state = state, in.stride = n_frames, in.frame = f;
        in.obs = obs ? obs + (size_t)D2D_OBS_DIM * (size_t)f : nullptr;
        in.act = act ? act + (size_t)D2D_ACT_DIM * (size_t)f : nullptr;
        in.trail = tr ? trail + 2 * (size_t)max_trail * (size_t)f : nullptr;
        in.trail_len = tr ? clamp_len(trail_len[f], max_trail) : 0;
        const int32_t np = N_FIXED + (in.trail_len > 1 ? in.trail_len - 1 : 0);
        prims.resize((size_t)np);
        for (int32_t k = 0; k < np; ++k) prims[(size_t)k] = build_prim(in, v, k);
        resolve_host(prims, v, nullptr, nullptr, out + 3 * (size_t)v.W * (size_t)v.H * (size_t)f);
    }
}

inline void plot_paths_host(const d2dr_view* view, const d2d_scn* scn, const float* xy, const int32_t* len,
                            const uint8_t* rgb, int32_t n_paths, int32_t max_len, uint8_t* out) {
    const View v = make_view(view, 1);
    FrameIn in;
    in.scn = scn, in.state = nullptr, in.stride = 1, in.frame = 0;
    in.obs = in.act = in.trail = nullptr;
    in.trail_len = 0;
    std::vector<Prim> prims((size_t)(N_FIXED + D2DR_BAR_ROWS));
    for (size_t k = 0; k < prims.size(); ++k) prims[k] = build_prim(in, v, (int32_t)k);
    std::vector<uint32_t> ids((size_t)v.W * (size_t)v.H, 0u);
    for (int32_t m = 0; m < n_paths; ++m) {
        const int32_t n = clamp_len(len[m], max_len);
        for (int32_t j = 0; j + 1 < n; ++j) {
            const Prim q = plot_segment(xy, n, n_paths, m, j, v);
            if ((q.rgbk >> 24) == K_NONE) continue;
            for (int32_t r = q.r0; r <= q.r1; ++r)
                for (int32_t c = q.c0; c <= q.c1; ++c)
                    if (covers(q, r, c, pixel_x(v, c), pixel_y(v, r))) {
                        uint32_t& id = ids[(size_t)r * (size_t)v.W + (size_t)c];
                        if ((uint32_t)m + 1u > id) id = (uint32_t)m + 1u;
                    }
        }
    }
    resolve_host(prims, v, ids.data(), rgb, out);
}

#if defined(__HIPCC__)
/* ---- the tile walk (device only) ------------------------------------------------------------------
 * One workgroup of NT lanes resolves one 64 x 4 pixel tile of one frame: one wave per pixel row.  Shared
 * by every library that rasterises a primitive list (libd2d_render.so, libd2d_hud.so): a kernel declares
 * one TileLds, takes its Tile from tile_of(), and either calls walk_tile() -- templated on what differs
 * between the lists: the list's length and the colour of a pixel no primitive covers -- or strings
 * scan_range() calls together itself (the plot) and ends with store_tile(). */
constexpr int TW = 64, TH = 4, NT = TW * TH;

struct TileLds {
    Prim prim[NT];
    int32_t wcnt[NT / 64];
    uint8_t rgb[TH][TW * 3];
};

struct Tile {
    int32_t tx0, ty0, tc1, tr1;  /* first column / row; last column / row inside the picture */
    int32_t row, col;            /* this lane's pixel */
    float x, y;                  /* its centre */
    bool inside;
};

__device__ __forceinline__ Tile tile_of(const View& v) {
    const int32_t t = (int32_t)threadIdx.x, lane = t & 63, w = t >> 6;
    const int32_t tiles_x = (v.W + TW - 1) / TW;
    Tile q;
    q.tx0 = ((int32_t)blockIdx.x % tiles_x) * TW, q.ty0 = ((int32_t)blockIdx.x / tiles_x) * TH;
    q.col = q.tx0 + lane, q.row = q.ty0 + w;
    q.tc1 = (q.tx0 + TW - 1 < v.W - 1) ? q.tx0 + TW - 1 : v.W - 1;
    q.tr1 = (q.ty0 + TH - 1 < v.H - 1) ? q.ty0 + TH - 1 : v.H - 1;
    q.inside = q.col <= q.tc1 && q.row <= q.tr1;
    q.x = pixel_x(v, q.col), q.y = pixel_y(v, q.row);
    return q;
}

/* Primitives [lo, hi) of the list, top first, 256 at a time: cull against the tile, compact the
 * survivors into LDS in list order, then every unresolved pixel scans them. */
__device__ __forceinline__ void scan_range(const Prim* __restrict__ fp, int32_t lo, int32_t hi, const Tile& q, bool& hit,
                                           uint32_t& colour, TileLds& lds) {
    const int32_t t = (int32_t)threadIdx.x, lane = t & 63, w = t >> 6;
    for (int32_t base = hi; base > lo; base -= NT) {
        if (!__syncthreads_or(hit ? 0 : 1)) break;  /* every pixel of the tile has its colour (uniform) */
        const int32_t idx = base - 1 - t;
        /* the primitive as three 16-byte words (a.xyzw, b.xy = p[0..5]; b.z = rgbk; b.w, c.xyz = c0, c1, r0, r1) */
        const uint4* src = reinterpret_cast<const uint4*>(fp + (idx >= lo ? idx : lo));
        const uint4 qa = src[0], qb = src[1], qc = src[2];
        const bool keep = idx >= lo && (qb.z >> 24) != K_NONE && (int32_t)qb.w <= q.tc1 && (int32_t)qc.x >= q.tx0 &&
                          (int32_t)qc.y <= q.tr1 && (int32_t)qc.z >= q.ty0;
        const unsigned long long b = __ballot(keep);
        if (lane == 0) lds.wcnt[w] = __popcll(b);
        __syncthreads();
        int32_t off = 0, total = 0;
#pragma unroll
        for (int k = 0; k < NT / 64; ++k) {
            const int32_t c = lds.wcnt[k];
            off += (k < w) ? c : 0;
            total += c;
        }
        if (keep) {
            uint4* dst = reinterpret_cast<uint4*>(lds.prim + off + __popcll(b & ((1ull << lane) - 1ull)));
            dst[0] = qa, dst[1] = qb, dst[2] = qc;
        }
        __syncthreads();
        if (!hit)
            for (int32_t k = 0; k < total; ++k)
                if (covers(lds.prim[k], q.row, q.col, q.x, q.y)) {
                    colour = lds.prim[k].rgbk;
                    hit = true;
                    break;
                }
    }
}

/* The tile's RGB bytes, staged in LDS, leave as dwords (bytes only at a row's unaligned ends). */
__device__ __forceinline__ void store_tile(const View& v, const Tile& q, int32_t f, uint32_t colour, TileLds& lds,
                                           uint8_t* __restrict__ out) {
    const int32_t t = (int32_t)threadIdx.x, lane = t & 63, w = t >> 6;
    if (q.inside) {
        lds.rgb[w][3 * lane] = (uint8_t)(colour & 255u);
        lds.rgb[w][3 * lane + 1] = (uint8_t)((colour >> 8) & 255u);
        lds.rgb[w][3 * lane + 2] = (uint8_t)((colour >> 16) & 255u);
    }
    __syncthreads();
    if (q.row > q.tr1) return;
    /* wave w stores pixel row `row`: bytes up to the first 4-byte boundary, dwords, bytes after the last */
    const int32_t nbytes = 3 * (q.tc1 - q.tx0 + 1);
    uint8_t* g = out + (((size_t)f * (size_t)v.H + (size_t)q.row) * (size_t)v.W + (size_t)q.tx0) * 3;
    int32_t head = (int32_t)((4u - (uint32_t)((uintptr_t)g & 3u)) & 3u);
    head = head < nbytes ? head : nbytes;
    const int32_t ndw = (nbytes - head) >> 2, tail0 = head + 4 * ndw;
    if (lane < head) g[lane] = lds.rgb[w][lane];
    if (lane < ndw) {
        const uint8_t* s = &lds.rgb[w][head + 4 * lane];
        *reinterpret_cast<uint32_t*>(g + head + 4 * lane) =
            (uint32_t)s[0] | ((uint32_t)s[1] << 8) | ((uint32_t)s[2] << 16) | ((uint32_t)s[3] << 24);
    }
    if (lane < nbytes - tail0) g[tail0 + lane] = lds.rgb[w][tail0 + lane];
}

/* A frame whose picture is its list and nothing else: `len(f)` primitives at fp, and `uncovered(row,
 * col)` for a pixel that none of them covers (evaluated for such pixels only). */
template <class Len, class Uncovered>
__device__ __forceinline__ void walk_tile(const Prim* __restrict__ fp, const View& v, int32_t f, Len len,
                                          Uncovered uncovered, TileLds& lds, uint8_t* __restrict__ out) {
    const Tile q = tile_of(v);
    uint32_t colour = C_BG;
    bool hit = !q.inside;  /* pixels past the picture's edge have nothing to find */
    scan_range(fp, 0, len(f), q, hit, colour, lds);
    if (!hit) colour = uncovered(q.row, q.col);
    store_tile(v, q, f, colour, lds, out);
}
#endif /* __HIPCC__ */
}  // namespace d2dr
#endif /* D2D_RASTER_H */
