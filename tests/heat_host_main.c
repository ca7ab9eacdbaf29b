/* csrc/heat/d2d_heat_core.h compiled for the host as plain C: reads one case per line from stdin and
 * prints the header's answer, for tests/test_heatmap.py to compare with heatmap.py's NumPy restatement.
 *   c BITS G        d2d_heat_cell of the float32 whose bits are BITS (hex)
 *   p BITSX BITSY GX GY   d2d_heat_cell2
 *   k CAUSE         d2d_heat_class
 *   q V             d2d_heat_isqrt
 *   l C PEAK        d2d_heat_level
 *   r NUM DEN       d2d_heat_rate_level
 *   m LEVEL         d2d_heat_ramp
 *   t LEVEL         d2d_heat_rate_colour
 *   b BG COLOUR A   d2d_heat_blend
 */
#include <inttypes.h>
#include <stdio.h>
#include <string.h>

#include "heat/d2d_heat_core.h"

static float from_bits(uint32_t b) {
    float f;
    memcpy(&f, &b, sizeof f);
    return f;
}

int main(void) {
    char line[256];
    while (fgets(line, sizeof line, stdin)) {
        uint32_t a, b;
        uint64_t v, w;
        int i, j, k, r, g, bl;
        if (sscanf(line, "c %" SCNx32 " %d", &a, &i) == 2) {
            printf("%d\n", d2d_heat_cell(from_bits(a), i));
        } else if (sscanf(line, "p %" SCNx32 " %" SCNx32 " %d %d", &a, &b, &i, &j) == 4) {
            printf("%d\n", d2d_heat_cell2(from_bits(a), from_bits(b), i, j));
        } else if (sscanf(line, "k %d", &i) == 1) {
            printf("%d\n", d2d_heat_class(i));
        } else if (sscanf(line, "q %" SCNu64, &v) == 1) {
            printf("%" PRIu32 "\n", d2d_heat_isqrt(v));
        } else if (sscanf(line, "l %" SCNu64 " %" SCNu64, &v, &w) == 2) {
            printf("%d\n", d2d_heat_level((uint32_t)v, (uint32_t)w));
        } else if (sscanf(line, "r %" SCNu64 " %" SCNu64, &v, &w) == 2) {
            printf("%d\n", d2d_heat_rate_level((uint32_t)v, (uint32_t)w));
        } else if (sscanf(line, "m %d", &i) == 1) {
            d2d_heat_ramp(i, &r, &g, &bl);
            printf("%d %d %d\n", r, g, bl);
        } else if (sscanf(line, "t %d", &i) == 1) {
            d2d_heat_rate_colour(i, &r, &g, &bl);
            printf("%d %d %d\n", r, g, bl);
        } else if (sscanf(line, "b %d %d %d", &i, &j, &k) == 3) {
            printf("%d\n", d2d_heat_blend(i, j, k));
        } else {
            fprintf(stderr, "bad case: %s", line);
            return 2;
        }
    }
    return 0;
}
