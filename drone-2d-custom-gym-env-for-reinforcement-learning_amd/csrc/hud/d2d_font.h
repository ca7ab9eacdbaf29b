/* d2d_font.h -- the text overlay's 5 x 7 bitmap font, drawn by hand for this project.
 *
 * glyph_bits(ch) packs a glyph's seven rows, five bits each, into one word: row r (0 = top) is
 * (bits >> 5 r) & 31, and bit 4 of a row is its leftmost pixel.  The set is what the overlay prints:
 * the six labels of include/d2d_hud.h, the digits, '-', '.', ':', the space, and "inf" / "nan"; a few
 * more letters are there so that the lower-case alphabet has no holes in the middle of a word.  Any
 * other byte is an empty cell.  A switch, not a table: the same function compiles for host and device
 * without a device-side global.
 */
#ifndef D2D_FONT_H
#define D2D_FONT_H

#include <stdint.h>

#if defined(__HIPCC__)
#define D2DH_FONT_FN __host__ __device__ static inline
#else
#define D2DH_FONT_FN static inline
#endif

#define D2DH_G(a, b, c, d, e, f, g)                                                                             \
    ((uint64_t)(a) | ((uint64_t)(b) << 5) | ((uint64_t)(c) << 10) | ((uint64_t)(d) << 15) | ((uint64_t)(e) << 20) | \
     ((uint64_t)(f) << 25) | ((uint64_t)(g) << 30))

D2DH_FONT_FN uint64_t d2dh_glyph_bits(int ch) {
    switch (ch) {
        /* digits */
        case '0': return D2DH_G(0b01110, 0b10001, 0b10011, 0b10101, 0b11001, 0b10001, 0b01110);
        case '1': return D2DH_G(0b00100, 0b01100, 0b00100, 0b00100, 0b00100, 0b00100, 0b01110);
        case '2': return D2DH_G(0b01110, 0b10001, 0b00001, 0b00010, 0b00100, 0b01000, 0b11111);
        case '3': return D2DH_G(0b11110, 0b00001, 0b00001, 0b01110, 0b00001, 0b00001, 0b11110);
        case '4': return D2DH_G(0b00010, 0b00110, 0b01010, 0b10010, 0b11111, 0b00010, 0b00010);
        case '5': return D2DH_G(0b11111, 0b10000, 0b11110, 0b00001, 0b00001, 0b10001, 0b01110);
        case '6': return D2DH_G(0b00110, 0b01000, 0b10000, 0b11110, 0b10001, 0b10001, 0b01110);
        case '7': return D2DH_G(0b11111, 0b00001, 0b00010, 0b00100, 0b01000, 0b01000, 0b01000);
        case '8': return D2DH_G(0b01110, 0b10001, 0b10001, 0b01110, 0b10001, 0b10001, 0b01110);
        case '9': return D2DH_G(0b01110, 0b10001, 0b10001, 0b01111, 0b00001, 0b00010, 0b01100);
        /* punctuation */
        case '-': return D2DH_G(0b00000, 0b00000, 0b00000, 0b11111, 0b00000, 0b00000, 0b00000);
        case '.': return D2DH_G(0b00000, 0b00000, 0b00000, 0b00000, 0b00000, 0b01100, 0b01100);
        case ':': return D2DH_G(0b00000, 0b01100, 0b01100, 0b00000, 0b01100, 0b01100, 0b00000);
        /* the labels' capitals */
        case 'A': return D2DH_G(0b00100, 0b01010, 0b10001, 0b10001, 0b11111, 0b10001, 0b10001);
        case 'C': return D2DH_G(0b01110, 0b10001, 0b10000, 0b10000, 0b10000, 0b10001, 0b01110);
        case 'P': return D2DH_G(0b11110, 0b10001, 0b10001, 0b11110, 0b10000, 0b10000, 0b10000);
        case 'T': return D2DH_G(0b11111, 0b00100, 0b00100, 0b00100, 0b00100, 0b00100, 0b00100);
        /* lower case */
        case 'a': return D2DH_G(0b00000, 0b00000, 0b01110, 0b00001, 0b01111, 0b10001, 0b01111);
        case 'b': return D2DH_G(0b10000, 0b10000, 0b11110, 0b10001, 0b10001, 0b10001, 0b11110);
        case 'c': return D2DH_G(0b00000, 0b00000, 0b01110, 0b10001, 0b10000, 0b10001, 0b01110);
        case 'd': return D2DH_G(0b00001, 0b00001, 0b01111, 0b10001, 0b10001, 0b10001, 0b01111);
        case 'e': return D2DH_G(0b00000, 0b00000, 0b01110, 0b10001, 0b11111, 0b10000, 0b01110);
        case 'f': return D2DH_G(0b00110, 0b01001, 0b01000, 0b11100, 0b01000, 0b01000, 0b01000);
        case 'g': return D2DH_G(0b00000, 0b01111, 0b10001, 0b10001, 0b01111, 0b00001, 0b01110);
        case 'h': return D2DH_G(0b10000, 0b10000, 0b10110, 0b11001, 0b10001, 0b10001, 0b10001);
        case 'i': return D2DH_G(0b00100, 0b00000, 0b01100, 0b00100, 0b00100, 0b00100, 0b01110);
        case 'l': return D2DH_G(0b01100, 0b00100, 0b00100, 0b00100, 0b00100, 0b00100, 0b01110);
        case 'm': return D2DH_G(0b00000, 0b00000, 0b11010, 0b10101, 0b10101, 0b10101, 0b10101);
        case 'n': return D2DH_G(0b00000, 0b00000, 0b10110, 0b11001, 0b10001, 0b10001, 0b10001);
        case 'o': return D2DH_G(0b00000, 0b00000, 0b01110, 0b10001, 0b10001, 0b10001, 0b01110);
        case 'p': return D2DH_G(0b00000, 0b11110, 0b10001, 0b10001, 0b11110, 0b10000, 0b10000);
        case 'r': return D2DH_G(0b00000, 0b00000, 0b10110, 0b11001, 0b10000, 0b10000, 0b10000);
        case 's': return D2DH_G(0b00000, 0b00000, 0b01111, 0b10000, 0b01110, 0b00001, 0b11110);
        case 't': return D2DH_G(0b01000, 0b01000, 0b11100, 0b01000, 0b01000, 0b01001, 0b00110);
        case 'u': return D2DH_G(0b00000, 0b00000, 0b10001, 0b10001, 0b10001, 0b10011, 0b01101);
        case 'v': return D2DH_G(0b00000, 0b00000, 0b10001, 0b10001, 0b10001, 0b01010, 0b00100);
        case 'w': return D2DH_G(0b00000, 0b00000, 0b10001, 0b10001, 0b10101, 0b10101, 0b01010);
        default: return 0u;
    }
}

/* row r (0..6) of the glyph of ch: 5 bits, bit 4 leftmost */
D2DH_FONT_FN uint32_t d2dh_glyph_row(int ch, int r) { return (uint32_t)(d2dh_glyph_bits(ch) >> (5 * r)) & 31u; }

#endif /* D2D_FONT_H */
