/* d2d_gif_core.h -- libd2d_gif.so's shared host/device code (include/d2d_gif.h has the format).
 *
 *   PalTable, pal_index   the palette with its exact-match hash and the nearest-colour rule
 *   index_pixel           one pixel of the index + delta stage
 *   lzw_segment           one segment's codes into its staging words; the code widths follow a model of
 *                         the DECODER's table, so a Clear or EOI behind a code has the decoder's width
 *   merge_byte            one byte of the merged LSB-first stream from the 64 staging buffers
 *   chunk layout          header bytes, sub-block positions, the chunk's length
 *   encode_host ...       the CPU twin: the same functions, lane by lane
 * Integer code only: host and device give the same bytes whatever the flags.
 */
#ifndef D2D_GIF_CORE_H
#define D2D_GIF_CORE_H

#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../../include/d2d_gif.h"
#include "../hud/d2d_hud_core.h" /* the colour constants of d2d_raster.h and d2d_hud_core.h only */

#if defined(__HIPCC__)
#define D2DG_FN __host__ __device__ static inline
#else
#define D2DG_FN static inline
#endif

namespace d2dg {

static_assert(D2DG_DICT_CAP >= 1024 && D2DG_DICT_CAP <= 4096, "the dictionary cap is 1024..4096");
static_assert(D2DG_SEGMENTS == 64, "one segment per lane of a wave");

enum {
    HDR = 19,          /* extension 8 + descriptor 10 + code size 1 */
    PAL_HASH = 512,    /* slots of the palette's exact-match hash (<= 255 entries) */
    HALF = 4096,       /* a dictionary's hash: two halves of HALF slots, the half a bit of the key's hash */
    SLOTS = 2 * HALF
};

static constexpr uint32_t MODEL_PALETTE[D2DG_MODEL_COLOURS] = {
    d2dr::C_BG,   d2dr::C_BLACK, d2dr::C_BLUE,  d2dr::C_LA,   d2dr::C_RED,         d2dr::C_GREEN,       d2dr::C_OBST,
    d2dr::C_BODY, d2dr::C_MOTOR, d2dr::C_GREY,  d2dr::C_TRAIL, d2dh::C_SHADE_FRAME, d2dh::C_SHADE_MOTOR, d2dh::C_TEXT_RED};

/* ------------------------------------------------------------------------------------------ the palette */
struct PalTable {
    uint32_t rgb[256];        /* r | g << 8 | b << 16; entries past n are 0 */
    uint16_t hash[PAL_HASH];  /* index + 1, 0: free */
    int32_t n, bits, m, pad;
};

D2DG_FN uint32_t pal_hash(uint32_t c) { return (c * 2654435761u) >> 23; }

D2DG_FN int32_t table_bits(int32_t n) {
    int32_t b = 1;
    while ((1 << b) < n + 1) ++b;
    return b;
}

inline void build_pal(const uint8_t* rgb, int32_t n, PalTable* t) {
    memset(t, 0, sizeof *t);
    t->n = n, t->bits = table_bits(n), t->m = t->bits < 2 ? 2 : t->bits;
    for (int32_t i = 0; i < n; ++i) {
        const uint32_t c = (uint32_t)rgb[3 * i] | ((uint32_t)rgb[3 * i + 1] << 8) | ((uint32_t)rgb[3 * i + 2] << 16);
        t->rgb[i] = c;
        uint32_t h = pal_hash(c);
        bool dup = false;
        while (t->hash[h] != 0) { /* ascending insertion: an equal colour keeps its lowest index */
            if (t->rgb[t->hash[h] - 1] == c) {
                dup = true;
                break;
            }
            h = (h + 1) & (PAL_HASH - 1);
        }
        if (!dup) t->hash[h] = (uint16_t)(i + 1);
    }
}

/* The palette index of colour c; *inexact set when c is not in the palette. */
D2DG_FN int32_t pal_index(const uint32_t* rgb, const uint16_t* hash, int32_t n, uint32_t c, bool* inexact) {
    uint32_t h = pal_hash(c);
    for (;;) {
        const uint32_t e = hash[h];
        if (e == 0) break;
        if (rgb[e - 1] == c) {
            *inexact = false;
            return (int32_t)e - 1;
        }
        h = (h + 1) & (PAL_HASH - 1);
    }
    *inexact = true;
    const int32_t r = (int32_t)(c & 255u), g = (int32_t)((c >> 8) & 255u), b = (int32_t)((c >> 16) & 255u);
    int32_t best = 0, bd = 0x7fffffff;
    for (int32_t i = 0; i < n; ++i) {
        const uint32_t q = rgb[i];
        const int32_t dr = r - (int32_t)(q & 255u), dg = g - (int32_t)((q >> 8) & 255u), db = b - (int32_t)((q >> 16) & 255u);
        const int32_t d = dr * dr + dg * dg + db * db;
        if (d < bd) bd = d, best = i;
    }
    return best;
}

/* One pixel of the index + delta stage: the delta image's byte; the canvas is updated.  *changed: the
 * pixel belongs to the frame's bounding box (only asked for on a later frame). */
D2DG_FN uint8_t index_pixel(const uint32_t* rgb, const uint16_t* hash, int32_t n, const uint8_t* px, bool has_frame,
                            uint8_t* canvas, bool* inexact, bool* changed) {
    const uint32_t c = (uint32_t)px[0] | ((uint32_t)px[1] << 8) | ((uint32_t)px[2] << 16);
    const uint8_t idx = (uint8_t)pal_index(rgb, hash, n, c, inexact);
    if (has_frame && *canvas == idx) {
        *changed = false;
        return (uint8_t)n; /* transparent */
    }
    *canvas = idx;
    *changed = true;
    return idx;
}

/* The frame's image rectangle from the reduced bounding box (x0 > x1: nothing changed). */
struct Rect {
    int32_t left, top, w, h;
};
D2DG_FN Rect frame_rect(bool has_frame, int32_t W, int32_t H, int32_t x0, int32_t y0, int32_t x1, int32_t y1) {
    Rect r;
    if (!has_frame) {
        r.left = 0, r.top = 0, r.w = W, r.h = H;
    } else if (x0 > x1 || y0 > y1) {
        r.left = 0, r.top = 0, r.w = 1, r.h = 1;
    } else {
        r.left = x0, r.top = y0, r.w = x1 - x0 + 1, r.h = y1 - y0 + 1;
    }
    return r;
}

/* ------------------------------------------------------------------------------------------ LZW */
/* staging words of one segment of at most seg_px pixels: its pixel codes, the Clears inside it, a leading
 * Clear and a trailing Clear / EOI, 12 bits each, and two words of slack for the merge's two-word reads */
D2DG_FN int64_t stage_words(int64_t seg_px) {
    return (12 * (seg_px + seg_px / (D2DG_DICT_CAP - 258) + 3) + 31) / 32 + 2;
}
D2DG_FN int64_t seg_pixels(int64_t n_px) { return (n_px + D2DG_SEGMENTS - 1) / D2DG_SEGMENTS; }

struct BitWriter {
    uint32_t* out;
    uint64_t acc;
    int32_t nacc;
    uint32_t bits;
};
D2DG_FN void put(BitWriter& w, uint32_t code, int32_t width) {
    w.acc |= (uint64_t)code << w.nacc;
    w.nacc += width;
    w.bits += (uint32_t)width;
    if (w.nacc >= 32) {
        *w.out++ = (uint32_t)w.acc;
        w.acc >>= 32;
        w.nacc -= 32;
    }
}

/* the dictionary of one lane: slot[SLOTS] holds codes, ent[code] = key | (slot & (HALF - 1)) << 20 with
 * key = prefix << 8 | byte.  A slot is occupied iff its code is one of this generation's ([first, top))
 * AND that code's entry points back at the slot: whatever an earlier generation, frame or call left behind
 * fails one of the two, so a Clear costs nothing and the memory needs no initial value. */
D2DG_FN uint32_t key_hash(uint32_t key) { return key * 2654435761u; }
D2DG_FN uint32_t key_half(uint32_t key) { return (key_hash(key) >> 31) * (uint32_t)HALF; }

/* Compress pixels [p0, p1) (p0 < p1) of the rectangle's row-major order into `stage`; returns the bits.
 * first / last: the stream's first / last non-empty segment. */
D2DG_FN uint32_t lzw_segment(const uint8_t* img, int32_t stride, const Rect& rc, int64_t p0, int64_t p1, int32_t m,
                             bool first, bool last, uint16_t* slot, uint32_t* ent, uint32_t* stage, int32_t* mid_clears) {
    const uint32_t clear = 1u << m, eoi = clear + 1u, base = clear + 2u;
    BitWriter w{stage, 0u, 0, 0u};
    /* the decoder's state: its code width and the number of its next table entry; `fresh`: it has read
     * no code since the last Clear (the first code adds no entry) */
    int32_t width = m + 1;
    uint32_t avail = base;
    bool fresh = true;
    uint32_t top = base; /* this generation's codes are [base, top) */
    if (first) put(w, clear, width);

    int32_t row = (int32_t)(p0 / rc.w), col = (int32_t)(p0 % rc.w);
    const uint8_t* line = img + (size_t)(rc.top + row) * (size_t)stride + (size_t)rc.left;
    uint32_t cur = line[col];
    for (int64_t p = p0 + 1; p < p1; ++p) {
        if (++col == rc.w) col = 0, line += stride;
        const uint32_t ch = line[col];
        const uint32_t key = (cur << 8) | ch;
        const uint32_t half = key_half(key);
        uint32_t h = (key_hash(key) >> 19) & (uint32_t)(HALF - 1);
        uint32_t found = 0u;
        for (;;) {
            const uint32_t c = slot[half + h];
            if (c < base || c >= top) break;
            const uint32_t e = ent[c];
            const uint32_t ekey = e & 0xFFFFFu;
            if ((e >> 20) != h || key_half(ekey) != half) break; /* a stale code: the slot is free */
            if (ekey == key) {
                found = c;
                break;
            }
            h = (h + 1) & (uint32_t)(HALF - 1);
        }
        if (found) {
            cur = found;
            continue;
        }
        /* emit the string so far; the decoder then adds an entry (not for the first code after a Clear) */
        put(w, cur, width);
        if (fresh) {
            fresh = false;
        } else if (avail < 4096u) {
            ++avail;
            if (avail == (1u << width) && width < 12) ++width;
        }
        if (avail < (uint32_t)D2DG_DICT_CAP) { /* our new string takes the number the decoder gives it next */
            slot[half + h] = (uint16_t)avail;
            ent[avail] = key | (h << 20);
            top = avail + 1u;
        } else { /* no number left: Clear, at the width the decoder has after that code's entry */
            put(w, clear, width);
            if (mid_clears) ++*mid_clears;
            width = m + 1, avail = base, fresh = true, top = base;
        }
        cur = ch;
    }
    put(w, cur, width);
    if (!fresh && avail < 4096u) {
        ++avail;
        if (avail == (1u << width) && width < 12) ++width;
    }
    put(w, last ? eoi : clear, width); /* the next segment's Clear, or the EOI */
    if (w.nacc > 0) *w.out = (uint32_t)w.acc;
    return w.bits;
}

/* Byte j of the merged stream.  off[s] is the bit at which segment s begins (off[64]: the total); stage
 * buffers are `stride` words apart.  Bits past the total are 0. */
D2DG_FN uint8_t merge_byte(const uint32_t* stage, int64_t stride, const uint32_t* off, uint32_t j) {
    uint32_t b = 8u * j;
    const uint32_t total = off[D2DG_SEGMENTS];
    int32_t lo = 0, hi = D2DG_SEGMENTS; /* the last s with off[s] <= b */
    while (hi - lo > 1) {
        const int32_t mid = (lo + hi) >> 1;
        if (off[mid] <= b) lo = mid; else hi = mid;
    }
    int32_t s = lo;
    uint32_t val = 0u;
    int32_t got = 0;
    while (got < 8 && b < total) {
        while (off[s + 1] <= b) ++s; /* skips empty segments; b < total keeps s < 64 */
        const uint32_t pos = b - off[s];
        uint32_t take = off[s + 1] - b;
        if (take > (uint32_t)(8 - got)) take = (uint32_t)(8 - got);
        const uint32_t* q = stage + (int64_t)s * stride + (pos >> 5);
        const uint32_t sh = pos & 31u;
        uint32_t bits = q[0] >> sh;
        if (sh + take > 32u) bits |= q[1] << (32u - sh);
        val |= (bits & ((1u << take) - 1u)) << got;
        got += (int32_t)take;
        b += take;
    }
    return (uint8_t)val;
}

/* ------------------------------------------------------------------------------------------ the chunk */
D2DG_FN uint32_t data_bytes(uint32_t total_bits) { return (total_bits + 7u) / 8u; }
D2DG_FN uint32_t n_blocks(uint32_t data) { return (data + 254u) / 255u; }
D2DG_FN uint32_t chunk_len(uint32_t data) { return (uint32_t)HDR + data + n_blocks(data) + 1u; }
D2DG_FN uint32_t data_pos(uint32_t j) { return (uint32_t)HDR + j + j / 255u + 1u; }

/* byte i < HDR of the chunk's fixed head */
D2DG_FN uint8_t header_byte(int32_t i, const Rect& rc, bool has_frame, int32_t delay_cs, int32_t transparent, int32_t m) {
    switch (i) {
        case 0: return 0x21;
        case 1: return 0xF9;
        case 2: return 4;
        case 3: return (uint8_t)(0x04 | (has_frame ? 1 : 0)); /* disposal 1; the transparent flag */
        case 4: return (uint8_t)(delay_cs & 255);
        case 5: return (uint8_t)((delay_cs >> 8) & 255);
        case 6: return (uint8_t)transparent;
        case 7: return 0;
        case 8: return 0x2C;
        case 9: return (uint8_t)(rc.left & 255);
        case 10: return (uint8_t)(rc.left >> 8);
        case 11: return (uint8_t)(rc.top & 255);
        case 12: return (uint8_t)(rc.top >> 8);
        case 13: return (uint8_t)(rc.w & 255);
        case 14: return (uint8_t)(rc.w >> 8);
        case 15: return (uint8_t)(rc.h & 255);
        case 16: return (uint8_t)(rc.h >> 8);
        case 17: return 0;
        default: return (uint8_t)m;
    }
}

D2DG_FN int64_t frame_cap(int64_t w, int64_t h) {
    const int64_t n = w * h;
    const int64_t codes = n + D2DG_SEGMENTS + n / (D2DG_DICT_CAP - 258) + 1;
    const int64_t data = (12 * codes + 7) / 8;
    return D2DG_CHUNK_FIXED + data + (data + 254) / 255;
}

/* ------------------------------------------------------------------------------------------ the CPU twin */
struct HostWork {
    std::vector<uint8_t> delta;
    std::vector<uint16_t> slot;
    std::vector<uint32_t> ent, stage;
};

/* One stream's frame (has_frame as it was before it): returns the chunk's length. */
inline uint32_t encode_stream_host(const PalTable& pal, int32_t W, int32_t H, const uint8_t* frame, int32_t delay_cs,
                                   uint8_t* canvas, bool has_frame, uint8_t* chunk, int32_t* inexact, int32_t* mid_clears,
                                   HostWork& wk) {
    const int64_t n_all = (int64_t)W * H;
    wk.delta.resize((size_t)n_all);
    int32_t x0 = W, y0 = H, x1 = -1, y1 = -1;
    for (int32_t y = 0; y < H; ++y)
        for (int32_t x = 0; x < W; ++x) {
            const int64_t p = (int64_t)y * W + x;
            bool inex = false, ch = false;
            wk.delta[(size_t)p] = index_pixel(pal.rgb, pal.hash, pal.n, frame + 3 * p, has_frame, canvas + p, &inex, &ch);
            if (inex && inexact) ++*inexact;
            if (ch && has_frame) {
                x0 = x < x0 ? x : x0, x1 = x > x1 ? x : x1;
                y0 = y < y0 ? y : y0, y1 = y > y1 ? y : y1;
            }
        }
    const Rect rc = frame_rect(has_frame, W, H, x0, y0, x1, y1);
    const int64_t n = (int64_t)rc.w * rc.h, seg = seg_pixels(n), sw = stage_words(seg);
    const int32_t live = (int32_t)((n + seg - 1) / seg);
    wk.slot.resize(SLOTS);
    wk.ent.resize(D2DG_DICT_CAP);
    wk.stage.assign((size_t)(sw * D2DG_SEGMENTS), 0u);
    uint32_t off[D2DG_SEGMENTS + 1];
    off[0] = 0u;
    for (int32_t s = 0; s < D2DG_SEGMENTS; ++s) {
        uint32_t bits = 0u;
        const int64_t p0 = s * seg, p1 = (p0 + seg < n) ? p0 + seg : n;
        if (p0 < n)
            bits = lzw_segment(wk.delta.data(), W, rc, p0, p1, pal.m, s == 0, s == live - 1, wk.slot.data(), wk.ent.data(),
                               wk.stage.data() + s * sw, mid_clears);
        off[s + 1] = off[s] + bits;
    }
    const uint32_t data = data_bytes(off[D2DG_SEGMENTS]);
    for (int32_t i = 0; i < HDR; ++i) chunk[i] = header_byte(i, rc, has_frame, delay_cs, pal.n, pal.m);
    for (uint32_t j = 0; j < data; ++j) chunk[data_pos(j)] = merge_byte(wk.stage.data(), sw, off, j);
    for (uint32_t t = 0; t < n_blocks(data); ++t)
        chunk[(uint32_t)HDR + 256u * t] = (uint8_t)(data - 255u * t < 255u ? data - 255u * t : 255u);
    chunk[chunk_len(data) - 1u] = 0;
    return chunk_len(data);
}

inline void encode_host(int32_t K, int32_t W, int32_t H, const PalTable& pal, const uint8_t* frames, const uint8_t* active,
                        int32_t delay_cs, uint8_t* canvas, uint8_t* has_frame, uint8_t* chunk, int64_t cap, int32_t* len,
                        int32_t* inexact, int32_t* mid_clears) {
    HostWork wk;
    const int64_t n_all = (int64_t)W * H;
    for (int32_t k = 0; k < K; ++k) {
        if (active && !active[k]) {
            len[k] = 0;
            continue;
        }
        len[k] = (int32_t)encode_stream_host(pal, W, H, frames + 3 * n_all * k, delay_cs, canvas + n_all * k,
                                             has_frame[k] != 0, chunk + cap * k, inexact ? inexact + k : nullptr,
                                             mid_clears ? mid_clears + k : nullptr, wk);
        has_frame[k] = 1;
    }
}

/* the file header; returns its length */
inline int32_t file_header(int32_t W, int32_t H, const PalTable& pal, int32_t loop, uint8_t* out) {
    int32_t o = 0;
    memcpy(out, "GIF89a", 6), o = 6;
    out[o++] = (uint8_t)(W & 255), out[o++] = (uint8_t)(W >> 8);
    out[o++] = (uint8_t)(H & 255), out[o++] = (uint8_t)(H >> 8);
    out[o++] = (uint8_t)(0x80 | 0x70 | (pal.bits - 1)); /* global table, 8 bits of colour resolution, its size */
    out[o++] = 0;                                       /* background index */
    out[o++] = 0;                                       /* no aspect ratio */
    for (int32_t i = 0; i < (1 << pal.bits); ++i) {
        const uint32_t c = i < pal.n ? pal.rgb[i] : 0u;
        out[o++] = (uint8_t)(c & 255u), out[o++] = (uint8_t)((c >> 8) & 255u), out[o++] = (uint8_t)((c >> 16) & 255u);
    }
    if (loop >= 0) {
        static const uint8_t app[14] = {0x21, 0xFF, 0x0B, 'N', 'E', 'T', 'S', 'C', 'A', 'P', 'E', '2', '.', '0'};
        memcpy(out + o, app, 14), o += 14;
        out[o++] = 3, out[o++] = 1, out[o++] = (uint8_t)(loop & 255), out[o++] = (uint8_t)((loop >> 8) & 255), out[o++] = 0;
    }
    return o;
}

}  // namespace d2dg
#endif /* D2D_GIF_CORE_H */
