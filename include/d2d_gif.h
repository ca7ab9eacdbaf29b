/* d2d_gif.h -- C ABI of libd2d_gif.so: device frames into finished GIF89a bytes, on the device.
 *
 * K streams (one GIF each) are encoded side by side.  One encode call takes one RGB frame per stream and
 * appends one FRAME CHUNK per active stream: Graphic Control Extension, Image Descriptor, the LZW data as
 * sub-blocks, the terminator.  A file is d2dg_file_header_host's bytes, the stream's chunks in call order,
 * and the trailer byte 0x3B.
 *
 * Format.
 *  - The palette holds n = 1..255 colours; index n is the TRANSPARENT index.  The global colour table has
 *    2^bits entries, bits = the smallest of 1..8 with 2^bits >= n + 1 (entries past n are black); the
 *    minimum code size is m = max(2, bits).
 *  - A pixel takes the palette index of its exact colour (the lowest index of equal entries).  A colour
 *    that is not in the palette takes the nearest entry -- squared RGB distance, the lowest index on ties
 *    -- and is counted in the stream's `inexact` counter.
 *  - A stream keeps a canvas of indices, uint8 [H][W].  Its first frame after create / restart is the whole
 *    picture with no transparency.  Every later frame is a delta: a pixel whose index equals the canvas's
 *    becomes the transparent index, the others are written to the canvas, and the image is the bounding
 *    box of the changed pixels (disposal 1: a decoder keeps its canvas).  A frame with no changed pixel is
 *    a 1 x 1 transparent image at (0, 0), so that its delay still counts.
 *  - LZW.  The image's n_px indices, row-major, are cut into D2DG_SEGMENTS segments of ceil(n_px / 64)
 *    pixels; the non-empty ones are the first ceil(n_px / that).  Each is compressed with a dictionary of
 *    its own: a non-empty segment begins with a Clear code, an empty one emits nothing, and one
 *    End-of-Information code closes the last.  Inside a segment the dictionary holds codes below
 *    D2DG_DICT_CAP; when the entry that a code would add has no number left, a Clear follows that code.
 *    Code widths are the decoder's: a Clear (or the EOI) that follows a code is written at the width the
 *    decoder has AFTER the table entry that code makes it add.  Segment bit strings are concatenated
 *    LSB-first without padding.  The bytes are a function of the input alone.
 *  - Chunk: 21 F9 04 <04 | transparent flag> <delay lo hi> <transparent index> 00,
 *           2C <left> <top> <width> <height> 00 (little-endian 16-bit; no local table), <m>,
 *           the data as sub-blocks of 255 bytes (the last shorter), 00.
 *    The transparent flag is off on a stream's first frame.
 *
 * d2dg_frame_cap(w, h), the most bytes one chunk of a w x h stream can take.  With n = w h pixels, every
 * pixel a code of its own at the widest code, 12 bits:
 *      codes <= n                                     pixel codes
 *             + D2DG_SEGMENTS                         one Clear per non-empty segment
 *             + n / (D2DG_DICT_CAP - 258)             Clears inside segments: between two of them a
 *                                                     segment emits at least D2DG_DICT_CAP - 257 codes
 *                                                     (the dictionary starts at 2^m + 2 <= 258)
 *             + 1                                     the EOI
 *      data  = ceil(12 codes / 8) bytes,   sub-blocks add ceil(data / 255) length bytes,
 *      cap   = 19 (extension 8, descriptor 10, code size 1) + data + ceil(data / 255) + 1 (terminator).
 *
 * Conventions: d2d_render.h's.  `*_dev` are device pointers; all workspace is allocated at create (the
 * canvases, the delta images, 64 dictionaries and 64 staging buffers per stream); encode calls neither
 * allocate nor synchronise and are ordered on `stream`; exceeding a capacity is D2DG_E_ARG, never a
 * truncated file; 0 on success, else a D2DG_E_* code with the message in the thread-local
 * d2dg_last_error().  A ctx is not re-entrant.
 */
#ifndef D2D_GIF_H
#define D2D_GIF_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define D2DG_ABI_VERSION 1

#define D2DG_MAX_COLOURS 255
#define D2DG_SEGMENTS 64
#define D2DG_DICT_CAP 4096      /* codes per dictionary; [1024, 4096] */
#define D2DG_MIN_SIZE 8         /* D2DR_MIN_SIZE */
#define D2DG_MAX_SIZE 2048      /* D2DR_MAX_SIZE */
#define D2DG_MAX_STREAMS 4096
#define D2DG_CHUNK_FIXED 20     /* bytes of a chunk that are not data or sub-block lengths */
#define D2DG_FILE_HEADER_MAX 800
#define D2DG_MODEL_COLOURS 14

typedef struct d2dg_ctx d2dg_t;

int32_t d2dg_abi_version(void);
const char* d2dg_last_error(void);
int32_t d2dg_dict_cap(void);

/* The bound above; 0 for a size outside D2DG_MIN_SIZE..D2DG_MAX_SIZE. */
int64_t d2dg_frame_cap(int32_t width, int32_t height);

/* All device workspace for max_streams streams of up to max_width x max_height pixels, and the palette
 * (host pointer, uint8 [n_colours][3]) with its lookup table.  Every stream starts without a frame. */
int32_t d2dg_create(int32_t device, int32_t max_streams, int32_t max_width, int32_t max_height,
                    const uint8_t* palette_rgb, int32_t n_colours, d2dg_t** out);
void d2dg_destroy(d2dg_t* ctx);

/* Every stream begins a new GIF: its next frame is a first frame, of any size the ctx holds.  Ordered on
 * `stream`; no synchronisation. */
int32_t d2dg_restart(d2dg_t* ctx, void* stream);

/* One frame per stream, two launches (index + delta; LZW + pack):
 *   frames_dev   uint8 [n_streams][height][width][3]
 *   active_dev   uint8 [n_streams] or NULL (all active).  An inactive stream gets length 0; its canvas,
 *                its chunk row and its counter are left alone.
 *   delay_cs     0..65535, the frame's delay in 1/100 s
 *   chunk_dev    uint8 [n_streams][cap]; cap >= d2dg_frame_cap(width, height), else D2DG_E_ARG
 *   len_dev      int32 [n_streams]: the chunk's length
 *   inexact_dev  int32 [n_streams] or NULL: pixels of this frame that took a nearest colour are ADDED
 * width and height must not change between a restart (or create) and the next.  n_streams = 0 returns
 * D2DG_OK and launches nothing. */
int32_t d2dg_encode(d2dg_t* ctx, int32_t n_streams, int32_t width, int32_t height, const uint8_t* frames_dev,
                    const uint8_t* active_dev, int32_t delay_cs, uint8_t* chunk_dev, int64_t cap, int32_t* len_dev,
                    int32_t* inexact_dev, void* stream);

/* The CPU twin: host pointers, the same bytes.  What the ctx keeps is passed in and out:
 *   canvas       uint8 [n_streams][height][width]
 *   has_frame    uint8 [n_streams]: 0 before a stream's first frame (set to 1 by it)
 *   mid_clears   int32 [n_streams] or NULL: Clear codes written inside segments are ADDED (for tests) */
int32_t d2dg_encode_host(int32_t n_streams, int32_t width, int32_t height, const uint8_t* palette_rgb,
                         int32_t n_colours, const uint8_t* frames, const uint8_t* active, int32_t delay_cs,
                         uint8_t* canvas, uint8_t* has_frame, uint8_t* chunk, int64_t cap, int32_t* len,
                         int32_t* inexact, int32_t* mid_clears);

/* "GIF89a", the logical screen (global table of 2^bits entries, background 0), the table, and the
 * NETSCAPE2.0 block with `loop` repetitions (0: for ever; negative: no block).  out holds out_cap bytes
 * (D2DG_FILE_HEADER_MAX always suffices); *out_len receives the length.  The trailer is the byte 0x3B. */
int32_t d2dg_file_header_host(int32_t width, int32_t height, const uint8_t* palette_rgb, int32_t n_colours,
                              int32_t loop, uint8_t* out, int32_t out_cap, int32_t* out_len);

/* The colours libd2d_render.so and libd2d_hud.so draw with, uint8 [D2DG_MODEL_COLOURS][3], in this order:
 * d2d_raster.h's background, black, blue, lookahead, red, green, obstacle, body, motor, grey, trail; then
 * d2d_hud_core.h's shade frame, shade motor, text red. */
int32_t d2dg_model_palette(uint8_t* out);

#define D2DG_OK 0
#define D2DG_E_ARG 1
#define D2DG_E_HIP 2
#define D2DG_E_NOMEM 4

#ifdef __cplusplus
}
#endif
#endif /* D2D_GIF_H */
