/* d2d_heat_core.h -- the arithmetic of the arena maps (include/d2d_heat.h), plain C for host and device
 * alike: the cell function, the outcome class, the density and rate levels, the ramp and the blend.
 * heatmap.py restates every function here operation for operation; tests compile this header for the
 * host and compare.  Integer arithmetic throughout, except the cell function, whose three float32
 * operations (an add, two multiplies) are single IEEE operations that no contraction can fuse.
 */
#ifndef D2D_HEAT_CORE_H
#define D2D_HEAT_CORE_H

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define D2D_HEAT_FN static __host__ __device__ __forceinline__
#else
#define D2D_HEAT_FN static inline
#endif

/* outcome classes of a finished episode (cause: the D2D_END_* bitmask of its info row) */
#define D2D_HEAT_SUCCESS 0   /* cause & REACH (2) */
#define D2D_HEAT_COLLIDED 1  /* COLLISION (1) and none of REACH, TIMEUP (4), AA (8): D2D_MON_COLLISION */
#define D2D_HEAT_OTHER 2

/* The cell of one float32 observation value on an axis of G cells, or -1 when it is outside.
 * Inside iff -1 <= o < 1 (NaN and +-inf fail the comparison).  The min matters: o = 1 - 2^-24 rounds
 * o + 1 to 2.0, which would land on G. */
D2D_HEAT_FN int d2d_heat_cell(float o, int G) {
    if (!(-1.0f <= o && o < 1.0f)) return -1;
    const float u = (o + 1.0f) * 0.5f;
    const int c = (int)(u * (float)G);
    return c < G - 1 ? c : G - 1;
}

/* The plane index row * Gx + column of an observed position, or -1 when either axis is outside.
 * Row 0 is the top of the picture: row = Gy - 1 - c_y. */
D2D_HEAT_FN int d2d_heat_cell2(float ox, float oy, int Gx, int Gy) {
    const int cx = d2d_heat_cell(ox, Gx), cy = d2d_heat_cell(oy, Gy);
    if (cx < 0 || cy < 0) return -1;
    return (Gy - 1 - cy) * Gx + cx;
}

D2D_HEAT_FN int d2d_heat_class(int cause) {
    if (cause & 2) return D2D_HEAT_SUCCESS;
    if ((cause & 1) && !(cause & (4 | 8))) return D2D_HEAT_COLLIDED;
    return D2D_HEAT_OTHER;
}

/* floor(sqrt(v)), bit by bit */
D2D_HEAT_FN uint32_t d2d_heat_isqrt(uint64_t v) {
    uint64_t r = 0, bit = (uint64_t)1 << 62;
    while (bit > v) bit >>= 2;
    while (bit != 0) {
        if (v >= r + bit) {
            v -= r + bit;
            r = (r >> 1) + bit;
        } else {
            r >>= 1;
        }
        bit >>= 2;
    }
    return (uint32_t)r;
}

/* density: 0 for an empty cell, else max(1, isqrt(c * 65025 / peak)) in 1 .. 255 (peak >= c > 0) */
D2D_HEAT_FN int d2d_heat_level(uint32_t c, uint32_t peak) {
    if (c == 0 || peak == 0) return 0;
    const uint32_t l = d2d_heat_isqrt((uint64_t)c * 65025u / peak);
    return l < 1 ? 1 : (l > 255 ? 255 : (int)l);
}

/* rate: round(255 num / den) for den > 0 (num <= den gives 0 .. 255; clamped otherwise) */
D2D_HEAT_FN int d2d_heat_rate_level(uint32_t num, uint32_t den) {
    const uint64_t l = ((uint64_t)510 * num + den) / ((uint64_t)2 * den);
    return l > 255 ? 255 : (int)l;
}

D2D_HEAT_FN int d2d_heat_mix(int a, int b, int f) { return (a * (255 - f) + b * f + 127) / 255; }

/* The sequential ramp of the density picture: entry L of the 256-entry table is the integer
 * interpolation between the five anchors below, which stand at levels 0, 63.75, 127.5, 191.25 and 255:
 *   p = 4 L, s = min(p / 255, 3), f = p - 255 s, channel = (A[s] (255 - f) + A[s+1] f + 127) / 255.
 * Dark blue through purple, red and orange to pale yellow. */
#define D2D_HEAT_ANCHORS 5
D2D_HEAT_FN void d2d_heat_ramp(int level, int* r, int* g, int* b) {
    const int A[D2D_HEAT_ANCHORS][3] = {{13, 8, 135}, {126, 3, 168}, {204, 71, 120}, {248, 149, 64}, {240, 249, 33}};
    const int p = 4 * level;
    const int s = p / 255 < D2D_HEAT_ANCHORS - 2 ? p / 255 : D2D_HEAT_ANCHORS - 2;
    const int f = p - 255 * s;
    *r = d2d_heat_mix(A[s][0], A[s + 1][0], f);
    *g = d2d_heat_mix(A[s][1], A[s + 1][1], f);
    *b = d2d_heat_mix(A[s][2], A[s + 1][2], f);
}

/* render.red_blue_grad at f = level / 255: red (low) to blue (high) through magenta */
D2D_HEAT_FN void d2d_heat_rate_colour(int level, int* r, int* g, int* b) {
    *g = 0;
    if (2 * level < 255) {
        *r = 255;
        *b = 2 * level;
    } else {
        *r = 2 * (255 - level);
        *b = 255;
    }
}

/* (bg (255 - a) + colour a + 127) / 255 */
D2D_HEAT_FN int d2d_heat_blend(int bg, int colour, int a) { return d2d_heat_mix(bg, colour, a); }

#endif /* D2D_HEAT_CORE_H */
