/* d2d_hud_core.h -- libd2d_hud.so's shared host/device code (include/d2d_hud.h has the picture model).
 *
 *   ext_prim        one primitive of a frame's EXTENDED list: a slot map sends each extended slot either
 *                   to a slot of csrc/render/d2d_raster.h's build_prim, handed over as is, or to a new
 *                   primitive (arc capsule, shade box)
 *   format_value    str(round(float(v), 2)) without libc;  format_line: label + value
 *   text_colour     the colour of a pixel that no primitive covers
 *   shade_step      one tracked env of the shade recorder
 *   render_host ... the CPU twins
 * Compile with -ffp-contract=off on both sides, as d2d_raster.h.
 */
#ifndef D2D_HUD_CORE_H
#define D2D_HUD_CORE_H

#include <math.h>
#include <stdint.h>

#include <vector>

#include "../../../include/d2d_hud.h"
#include "../render/d2d_raster.h"
#include "d2d_font.h"

namespace d2dh {
using namespace d2dr;

/* extended slot numbers: d2d_raster.h's up to S_LA_DOT keep theirs */
enum {
    X_LA_ARC = S_LA_DOT + 1,                  /* D2DH_ARC_SEGS capsules */
    X_VEL = X_LA_ARC + D2DH_ARC_SEGS,         /* base S_VEL */
    X_VEL_ARC,
    X_NEAR = X_VEL_ARC + D2DH_ARC_SEGS,       /* base S_NEAR */
    X_NEAR_ARC,
    X_SHADE = X_NEAR_ARC + D2DH_ARC_SEGS,     /* 3 max_shades boxes, then base S_CIRC ... */
    N_ARC_SLOTS = 3 * D2DH_ARC_SEGS
};
static_assert(S_VEL == S_LA_DOT + 1 && S_NEAR == S_VEL + 1 && S_CIRC == S_NEAR + 1, "the slot map follows d2d_raster.h");

static constexpr uint32_t C_SHADE_FRAME = D2DR_RGB(205, 222, 250), C_SHADE_MOTOR = D2DR_RGB(170, 195, 235),
                          C_TEXT_RED = D2DR_RGB(150, 0, 0);

/* What the extended list adds to a frame's inputs. */
struct HudIn {
    const double* shade;  /* this frame's [max_shades][3] or NULL */
    int32_t n_shades;     /* min(count, max_shades), 0 without */
    int32_t max_shades;   /* the slots reserved: 3 per shade */
};

D2DR_FN int32_t ext_extra(int32_t max_shades) { return N_ARC_SLOTS + 3 * max_shades; }

/* Capsule j of the arc `which` (0 lookahead, 1 velocity, 2 nearest obstacle). */
D2DR_FN Prim arc_prim(const FrameIn& in, const View& v, int which, int32_t j) {
    if (!(v.layers & D2DH_L_ARCS) || in.scn == nullptr || in.state == nullptr) return none_prim();
    const double x = st(in, D2D_S_F), y = st(in, D2D_S_F + 1), alpha = st(in, D2D_S_F + 2);
    if (!(abs_d(alpha) <= 8.0)) return none_prim();
    double gx, gy, R;
    uint32_t rgb;
    if (which == 0) {
        if (in.obs == nullptr) return none_prim();
        gx = ((double)in.obs[21] + 1.0) * v.sw * 0.5 - x, gy = ((double)in.obs[22] + 1.0) * v.sh * 0.5 - y;
        R = 100.0, rgb = C_LA;
    } else if (which == 1) {
        gx = st(in, D2D_S_F + 3), gy = st(in, D2D_S_F + 4);
        R = 50.0, rgb = C_RED;
    } else {
        const int32_t i = nearest_circle(in.scn, x, y);
        if (i < 0) return none_prim();
        gx = in.scn->cx[i] - x, gy = in.scn->cy[i] - y;
        R = 25.0, rgb = C_GREEN;
    }
    if (!finite_d(gx) || !finite_d(gy) || (gx == 0.0 && gy == 0.0)) return none_prim();
    double sa, ca;
    d2d_pm_sincos(alpha, &sa, &ca);
    const double cross = ca * gy - sa * gx, dot = ca * gx + sa * gy;
    if (!finite_d(cross) || !finite_d(dot)) return none_prim();
    const double two_pi = 6.283185307179586;
    double sweep = d2d_pm_atan2(cross, dot);
    if (sweep < 0.0) sweep += two_pi;
    if (!(sweep >= 0.0 && sweep <= two_pi)) return none_prim();
    /* the segment's two angles, each rotated from alpha by the addition theorems: both sincos
     * arguments stay inside d2d_pmath.h's |angle| <= 8 */
    const double t0 = sweep * (double)j / (double)D2DH_ARC_SEGS, t1 = sweep * (double)(j + 1) / (double)D2DH_ARC_SEGS;
    double s0, c0, s1, c1;
    d2d_pm_sincos(t0, &s0, &c0);
    d2d_pm_sincos(t1, &s1, &c1);
    const double r = R - 1.5;
    return make_capsule(x + r * (ca * c0 - sa * s0), y + r * (sa * c0 + ca * s0), x + r * (ca * c1 - sa * s1),
                        y + r * (sa * c1 + ca * s1), 3.0, rgb, v);
}

/* Box b (0 frame, 1 left motor, 2 right motor) of shade k. */
D2DR_FN Prim shade_prim(const HudIn& h, const View& v, int32_t k, int b) {
    if (!(v.layers & D2DH_L_SHADE) || h.shade == nullptr || k >= h.n_shades) return none_prim();
    const double* p = h.shade + 3 * (size_t)k;
    const double x = p[0], y = p[1], a = p[2];
    if (b == 0) return make_box(x, y, a, 50.0, 5.0, C_SHADE_FRAME, v);
    if (!(abs_d(a) <= 8.0)) return none_prim();
    double sn, cs;
    d2d_pm_sincos(a, &sn, &cs);
    const double lx = (b == 1) ? -40.0 : 40.0;
    return make_box(x + cs * lx, y + sn * lx, a, 10.0, 10.0, C_SHADE_MOTOR, v);
}

/* Primitive `slot` of a frame's extended list. */
D2DR_FN Prim ext_prim(const FrameIn& in, const HudIn& h, const View& v, int32_t slot) {
    if (slot < X_LA_ARC) return build_prim(in, v, slot);
    if (slot < X_VEL) return arc_prim(in, v, 0, slot - X_LA_ARC);
    if (slot == X_VEL) return build_prim(in, v, S_VEL);
    if (slot < X_NEAR) return arc_prim(in, v, 1, slot - X_VEL_ARC);
    if (slot == X_NEAR) return build_prim(in, v, S_NEAR);
    if (slot < X_SHADE) return arc_prim(in, v, 2, slot - X_NEAR_ARC);
    const int32_t k = slot - X_SHADE;
    if (k < 3 * h.max_shades) return shade_prim(h, v, k / 3, k % 3);
    return build_prim(in, v, slot - ext_extra(h.max_shades));
}

/* length of the extended list of a frame with a (clamped) trail of tl points */
D2DR_FN int32_t ext_len(int32_t tl, int32_t max_shades) { return N_FIXED + (tl > 1 ? tl - 1 : 0) + ext_extra(max_shades); }

/* ---- the text ------------------------------------------------------------------------------------ */
/* str(round(float(v), 2)).  a = |v| as a double, p = 100 a rounded, e = the exact error of p (fma):
 * k = floor(p) goes up when the exact fraction is above one half, or is one half and k is odd. */
D2DR_FN int32_t format_value(float value, char* out) {
    int32_t n = 0;
    const double v = (double)value;
    if (v != v) {
        out[0] = 'n', out[1] = 'a', out[2] = 'n', out[3] = 0;
        return 3;
    }
    uint32_t bits;
    memcpy(&bits, &value, sizeof bits);
    if (bits >> 31) out[n++] = '-';
    const double a = (v < 0.0) ? -v : v;
    if (!finite_d(a)) {
        out[n++] = 'i', out[n++] = 'n', out[n++] = 'f', out[n] = 0;
        return n;
    }
    int64_t k;
    if (a >= 1.0e9) {
        k = 99999999999ll;  /* saturated: 999999999.99 */
    } else {
        const double p = a * 100.0, e = fma(a, 100.0, -p);
        k = (int64_t)p;  /* p >= 0: truncation is floor */
        const double f = p - (double)k;
        if (f > 0.5 || (f == 0.5 && (e > 0.0 || (e == 0.0 && (k & 1))))) ++k;
    }
    const int64_t ip = k / 100;
    const int32_t fp = (int32_t)(k % 100);
    char dig[12];
    int32_t nd = 0;
    int64_t q = ip;
    do {
        dig[nd++] = (char)('0' + (int32_t)(q % 10));
        q /= 10;
    } while (q > 0);
    while (nd > 0) out[n++] = dig[--nd];
    out[n++] = '.';
    out[n++] = (char)('0' + fp / 10);
    if (fp % 10) out[n++] = (char)('0' + fp % 10);
    out[n] = 0;
    return n;
}

D2DR_FN const char* line_label(int line) {
    switch (line) {
        case 0: return "Total reward: ";
        case 1: return "Collision avoidance: ";
        case 2: return "Path adherence: ";
        case 3: return "Path progression: ";
        case 4: return "Aggressive alpha: ";
        default: return "Closest obs dist: ";
    }
}
D2DR_FN int line_field(int line) {
    switch (line) {
        case 0: return D2D_INFO_REWARD;
        case 1: return D2D_INFO_CA;
        case 2: return D2D_INFO_PA;
        case 3: return D2D_INFO_PP;
        case 4: return D2D_INFO_AA;
        default: return D2D_INFO_DCLOSE;
    }
}

/* line `line` of a frame's text into D2DH_LINE_CHARS bytes, zero-filled behind the value */
D2DR_FN void format_line(const float* info_row, int line, uint8_t* out) {
    const char* lab = line_label(line);
    int32_t n = 0;
    while (lab[n] != 0) {
        out[n] = (uint8_t)lab[n];
        ++n;
    }
    char num[16];
    const int32_t m = format_value(info_row[line_field(line)], num);
    for (int32_t k = 0; k < m && n < D2DH_LINE_CHARS; ++k) out[n++] = (uint8_t)num[k];
    while (n < D2DH_LINE_CHARS) out[n++] = 0;
}

D2DR_FN int32_t text_scale(int32_t height) { return height / 512 > 1 ? height / 512 : 1; }

/* The colour of pixel (row, col) where no primitive covers it: `text` is the frame's
 * [D2DH_TEXT_LINES][D2DH_LINE_CHARS] bytes, or NULL for plain background. */
D2DR_FN uint32_t text_colour(const uint8_t* text, int32_t s, int32_t row, int32_t col) {
    if (text == nullptr || row >= 53 * s || col >= 6 * D2DH_LINE_CHARS * s) return C_BG;  /* beyond the block */
    const int32_t gr = row / s, gc = col / s;  /* in glyph pixels */
    int32_t line, r;
    if (gr < 40) {
        line = gr >> 3, r = gr & 7;
    } else if (gr >= 45) {
        line = 5, r = gr - 45;
    } else {
        return C_BG;
    }
    const int32_t j = gc / 6, c = gc - 6 * j;
    if (r >= 7 || c >= 5) return C_BG;
    const uint32_t bits = d2dh_glyph_row((int)text[line * D2DH_LINE_CHARS + j], r);
    if (!((bits >> (4 - c)) & 1u)) return C_BG;
    return line == 5 ? C_TEXT_RED : C_BLACK;
}

/* ---- the shade recorder: tracked env k ------------------------------------------------------------ */
D2DR_FN void shade_step(int32_t k, const int32_t* env_ids, int32_t n_envs, const double* state, const uint8_t* term,
                        const uint8_t* trunc, double distance, int32_t max_shades, double* shade, int32_t* count,
                        double* last) {
    const int32_t e = env_ids[k];
    if (e < 0 || e >= n_envs) return;
    const double x = state[(size_t)D2D_S_F * (size_t)n_envs + (size_t)e];
    const double y = state[(size_t)(D2D_S_F + 1) * (size_t)n_envs + (size_t)e];
    const double a = state[(size_t)(D2D_S_F + 2) * (size_t)n_envs + (size_t)e];
    double* row = shade + 3 * (size_t)max_shades * (size_t)k;
    const bool restart = term == nullptr || term[e] != 0 || trunc[e] != 0;
    int32_t n = restart ? 0 : count[k];
    if (!restart && !(abs_d(x - last[2 * k]) > distance || abs_d(y - last[2 * k + 1]) > distance)) return;
    if (n >= 0 && n < max_shades) row[3 * (size_t)n] = x, row[3 * (size_t)n + 1] = y, row[3 * (size_t)n + 2] = a;
    last[2 * k] = x, last[2 * k + 1] = y;
    if (n < 0x7fffffff) count[k] = n + 1;
}

/* ---- CPU twins ------------------------------------------------------------------------------------ */
inline void resolve_host(const std::vector<Prim>& prims, const View& v, const uint8_t* text, uint8_t* out) {
    const int32_t s = text_scale(v.H);
    std::vector<int32_t> live;
    for (int32_t r = 0; r < v.H; ++r) {
        live.clear();
        for (int32_t k = (int32_t)prims.size() - 1; k >= 0; --k)
            if ((prims[(size_t)k].rgbk >> 24) != K_NONE && r >= prims[(size_t)k].r0 && r <= prims[(size_t)k].r1)
                live.push_back(k);
        const float y = pixel_y(v, r);
        for (int32_t c = 0; c < v.W; ++c) {
            const float x = pixel_x(v, c);
            uint32_t col = 0u;
            bool hit = false;
            for (size_t i = 0; i < live.size() && !hit; ++i)
                if (covers(prims[(size_t)live[i]], r, c, x, y)) col = prims[(size_t)live[i]].rgbk, hit = true;
            if (!hit) col = text_colour(text, s, r, c);
            uint8_t* o = out + 3 * ((size_t)r * (size_t)v.W + (size_t)c);
            o[0] = (uint8_t)(col & 255u), o[1] = (uint8_t)((col >> 8) & 255u), o[2] = (uint8_t)((col >> 16) & 255u);
        }
    }
}

inline void render_host(const d2dr_view* view, int32_t n_frames, const d2d_scn* scn, const double* state,
                        const float* obs, const float* act, const float* trail, const int32_t* trail_len,
                        int32_t max_trail, const float* info, const double* shade, const int32_t* shade_count,
                        int32_t max_shades, uint8_t* out) {
    const View v = make_view(view, 0);
    const bool tr = trail != nullptr && trail_len != nullptr;
    const bool text = info != nullptr && (v.layers & D2DH_L_TEXT);
    std::vector<Prim> prims;
    std::vector<uint8_t> lines((size_t)D2DH_TEXT_LINES * D2DH_LINE_CHARS);
    for (int32_t f = 0; f < n_frames; ++f) {
        FrameIn in;
        in.scn = scn + f, in.state = state, in.stride = n_frames, in.frame = f;
        in.obs = obs ? obs + (size_t)D2D_OBS_DIM * (size_t)f : nullptr;
        in.act = act ? act + (size_t)D2D_ACT_DIM * (size_t)f : nullptr;
        in.trail = tr ? trail + 2 * (size_t)max_trail * (size_t)f : nullptr;
        in.trail_len = tr ? clamp_len(trail_len[f], max_trail) : 0;
        HudIn h;
        h.max_shades = shade ? max_shades : 0;
        h.shade = shade ? shade + 3 * (size_t)max_shades * (size_t)f : nullptr;
        h.n_shades = shade ? clamp_len(shade_count[f], max_shades) : 0;
        const int32_t np = ext_len(in.trail_len, h.max_shades);
        prims.resize((size_t)np);
        for (int32_t k = 0; k < np; ++k) prims[(size_t)k] = ext_prim(in, h, v, k);
        if (text)
            for (int l = 0; l < D2DH_TEXT_LINES; ++l)
                format_line(info + (size_t)D2D_INFO_DIM * (size_t)f, l, lines.data() + (size_t)l * D2DH_LINE_CHARS);
        resolve_host(prims, v, text ? lines.data() : nullptr, out + 3 * (size_t)v.W * (size_t)v.H * (size_t)f);
    }
}
}  // namespace d2dh
#endif /* D2D_HUD_CORE_H */
