/* d2d_render.h -- C ABI of libd2d_render.so: batched pictures of Drone2dEnv episodes.
 *
 * The reference draws one env in a pygame window (drone_2d_env.py:775-906) and, in test mode, an
 * overview plot of all flight paths of a scenario (main.py:329-389).  This library draws frames of
 * many envs at once into a device tensor, and the overview plot, with its own picture model:
 * deterministic, not anti-aliased, not a pygame clone.
 *
 * Picture model
 *  - Pixel (row r, column c) has its centre at world x = (c + 0.5) screen_w / width,
 *    y = screen_h - (r + 0.5) screen_h / height (world y points up; row 0 is the top).
 *    px = screen_w / width is one output pixel in world units.
 *  - A frame is an ordered list of primitives, each with one colour:
 *      filled circle   covered when dx^2 + dy^2 <= r^2
 *      capsule A->B    covered when the squared distance to the segment <= hw^2, with
 *                      t = clamp(dot / len^2, 0, 1) and t = 0 when len^2 = 0
 *      oriented box    covered when |u| <= hx and |v| <= hy in box coordinates
 *    A pixel takes the colour of the LAST primitive of the list that covers its centre, else the
 *    background (243, 243, 243).
 *  - Widths and radii are the reference's, in world units, with a floor so that small frames stay
 *    legible: a capsule's hw = max(w_ref / 2, 0.75 px), a dot's r = max(r_ref, px).
 *  - Painter's order, bottom to top (colours in d2d_raster.h):
 *      1 path (99 capsules through 100 samples of the QPMI2D path)   2 dots at path(us[0]), wp_last
 *      3 spawn rectangle (where the drones really spawn, y flipped like everything else; the
 *        reference hands pygame the unflipped rectangle -- not reproduced)
 *      4 closest-point dot (obs[19:21])    5 lookahead line + dot (obs[21:23])
 *      6 velocity line    7 line to the nearest obstacle's centre
 *      8 obstacles        9 frame box, then both motor boxes (the bodies' own poses)
 *      10 force vectors   11 target dot at wp_last     12 trail
 *    Not drawn by this library: the text overlay, the three arcs, the shade sprites (libd2d_hud.so draws
 *    them around this list: d2d_hud.h), the mouse target.
 *  - Arithmetic: the primitive list of a frame is built in fp64 (d2d_pmath.h's sincos for the body
 *    angles, defined for |angle| <= 8) and rounded once to fp32; the per-pixel tests are fp32 add,
 *    mul, div and compare only.  The CPU twins below run the same functions (csrc/render/
 *    d2d_raster.h), so device and host pictures are byte-identical.
 *  - A NaN or infinite input covers nothing.
 *
 * Conventions: as drone2d.h -- `*_dev` are device pointers, every render call is ordered on
 * `stream` and neither allocates nor synchronises; 0 on success, else a D2DR_E_* code with the
 * message in the thread-local d2dr_last_error().  A ctx is not re-entrant: its workspace belongs to one
 * call at a time, so use one ctx per stream.
 */
#ifndef D2D_RENDER_H
#define D2D_RENDER_H

#include <stdint.h>

#include "drone2d.h"

#ifdef __cplusplus
extern "C" {
#endif

#define D2DR_ABI_VERSION 1

#define D2DR_MIN_SIZE 8
#define D2DR_MAX_SIZE 2048
#define D2DR_PATH_SAMPLES 100 /* predef_path.py get_path_coord */
#define D2DR_BAR_ROWS 100     /* main.py:387 */

/* layer groups of the `layers` mask (painter's-order items above) */
#define D2DR_L_PATH 1u      /* 1-3   */
#define D2DR_L_GUIDES 2u    /* 4-7   */
#define D2DR_L_OBSTACLES 4u /* 8     */
#define D2DR_L_DRONE 8u     /* 9     */
#define D2DR_L_FORCES 16u   /* 10-11 */
#define D2DR_L_TRAIL 32u    /* 12    */
#define D2DR_L_ALL 63u

typedef struct d2dr_view {
    int32_t width, height;     /* output size, each D2DR_MIN_SIZE..D2DR_MAX_SIZE  */
    double screen_w, screen_h; /* world extent (screensize_x, screensize_y)      */
    uint32_t layers;           /* D2DR_L_* mask                                  */
    uint32_t pad;
} d2dr_view;

typedef struct d2dr_ctx d2dr_t;

int32_t d2dr_abi_version(void);
const char* d2dr_last_error(void);

/* All device workspace is allocated here: the primitive lists of max_frames frames with trails of up
 * to max_trail points, and the plot's id buffer of max_width x max_height pixels.  Exceeding a
 * capacity in a later call is D2DR_E_ARG, never a truncated picture. */
int32_t d2dr_create(int32_t device, int32_t max_frames, int32_t max_trail, int32_t max_width, int32_t max_height,
                    d2dr_t** out);
void d2dr_destroy(d2dr_t* ctx);

/* n_frames frames.
 *   scn_dev    d2d_scn [n_frames]                 one ABI record per frame
 *   state_dev  float64 [D2D_NSTATE][n_frames]     d2d_get_state's layout; fields 0..17 are read
 *   obs_dev    float32 [n_frames][27] or NULL     NULL: no closest-point / lookahead markers
 *   act_dev    float32 [n_frames][2]  or NULL     NULL: no force vectors
 *   trail_dev  float32 [n_frames][max_trail][2] world positions, trail_len_dev int32 [n_frames]
 *              (values above max_trail count as max_trail); both NULL: no trail
 *   out_dev    uint8   [n_frames][height][width][3]  RGB, row 0 at the top
 * n_frames = 0 returns D2DR_OK and launches nothing. */
int32_t d2dr_render(d2dr_t* ctx, const d2dr_view* view, int32_t n_frames, const d2d_scn* scn_dev,
                    const double* state_dev, const float* obs_dev, const float* act_dev, const float* trail_dev,
                    const int32_t* trail_len_dev, uint8_t* out_dev, void* stream);

/* The overview plot of main.py:329-389: layers 1, 2 and 8 of the scenario (scn_dev NULL: a blank
 * background, as the reference has for 'stage_k'), then every path with more than 2 points as width-1
 * capsules in rgb[m] (where paths overlap the highest m wins), then the colour bar of main.py:387-388
 * without its text.
 *   xy_dev   float32 [max_len][n_paths][2]  world positions
 *   len_dev  int32   [n_paths]              (values above max_len count as max_len)
 *   rgb_dev  uint8   [n_paths][3]
 *   out_dev  uint8   [height][width][3]
 * view->layers is ignored.  n_paths = 0 returns D2DR_OK and launches nothing (out_dev is untouched). */
int32_t d2dr_plot_paths(d2dr_t* ctx, const d2dr_view* view, const d2d_scn* scn_dev, const float* xy_dev,
                        const int32_t* len_dev, const uint8_t* rgb_dev, int32_t n_paths, int32_t max_len,
                        uint8_t* out_dev, void* stream);

/* CPU twins: the same arguments with host pointers (max_trail is the ctx capacity the device call
 * takes from its ctx); they run the same primitive construction, coverage predicate and colour
 * resolve, need no GPU, and return byte-identical pictures. */
int32_t d2dr_render_host(const d2dr_view* view, int32_t n_frames, const d2d_scn* scn, const double* state,
                         const float* obs, const float* act, const float* trail, const int32_t* trail_len,
                         int32_t max_trail, uint8_t* out);
int32_t d2dr_plot_paths_host(const d2dr_view* view, const d2d_scn* scn, const float* xy, const int32_t* len,
                             const uint8_t* rgb, int32_t n_paths, int32_t max_len, uint8_t* out);
/* The 100 path samples of layer 1 (fp64 world x, y pairs), for tests. */
int32_t d2dr_path_samples_host(const d2d_scn* scn, double* xy);

#define D2DR_OK 0
#define D2DR_E_ARG 1
#define D2DR_E_HIP 2
#define D2DR_E_NOMEM 4

#ifdef __cplusplus
}
#endif
#endif /* D2D_RENDER_H */
