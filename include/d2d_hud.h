/* d2d_hud.h -- C ABI of libd2d_hud.so: frames with the reference's "watch the agent fly" extras.
 *
 * libd2d_render.so (d2d_render.h) draws everything of the reference's render() (drone_2d_env.py:775-906)
 * except what ENV_TEST_CONFIG's render_text / render_shade switch on and the three angle arcs.  This
 * library draws those too.  It changes nothing of d2d_render.h: it builds an EXTENDED primitive list
 * around that library's own (csrc/render/d2d_raster.h's build_prim, called slot by slot), and rasterises
 * it with the same tile walk and the same coverage predicate.  With none of the three new layer bits set
 * d2dh_render returns exactly d2dr_render's bytes.
 *
 * Picture model: d2d_render.h's, with these additions.
 *  - Painter's order, bottom to top (numbers are d2d_render.h's items):
 *      text   1-4   5 + lookahead arc   6 + velocity arc   7 + obstacle arc   shades   8-12
 *  - Arcs.  An arc shows which angle a guide line stands for: it runs on a circle around the frame body's
 *    position from the frame's angle alpha counter-clockwise (world axes, y up) by
 *        sweep = atan2(cross, dot) mod 2 pi
 *    with cross and dot between the frame's axis (cos alpha, sin alpha) and the guide line's direction
 *    (to the lookahead point of obs[21:23]; the velocity; to the nearest obstacle's centre -- the end
 *    points items 5-7 use).  It is a polyline of D2DH_ARC_SEGS capsules; capsule j joins the angles
 *    alpha + sweep j / 32 and alpha + sweep (j + 1) / 32 on the circle of radius R - 1.5 with half-width
 *    max(1.5, 0.75 px): the reference's arcs are 3 wide, drawn inward from R.  Radii and colours are the
 *    reference's (:849-868): lookahead 100, (0, 150, 150); velocity 50, red; obstacle 25, green.  A
 *    zero-length or non-finite guide, no obstacle, obs_dev NULL (lookahead) or |alpha| > 8 draws no arc.
 *    Built in fp64 with d2d_pmath.h's sincos / atan2 and rounded once, like the rest of the list.
 *    This is the project's own arc, NOT pygame's: the reference hands pygame.draw.arc a mix of world and
 *    body-relative angles (:390-392, :445, :486), so its arcs do not in general span the angle they are
 *    named after.  Not reproduced (compare the spawn rectangle in d2d_render.h).
 *  - Shades.  Shade k of a frame is the drone's silhouette at a recorded pose (x, y, angle): three
 *    oriented boxes, 100 x 10 in (205, 222, 250) and two 20 x 20 at frame-local (-+40, 0) in
 *    (170, 195, 235), all at the pose's angle.  min(count, max_shades) of them are drawn, oldest first.
 *    A non-finite pose or |angle| > 8 draws nothing.
 *  - Text.  Six lines, "<label><value>", from the frame's info row (:787-819):
 *        Total reward: D2D_INFO_REWARD        Collision avoidance: D2D_INFO_CA
 *        Path adherence: D2D_INFO_PA          Path progression: D2D_INFO_PP
 *        Aggressive alpha: D2D_INFO_AA        Closest obs dist: D2D_INFO_DCLOSE   (this one in (150, 0, 0),
 *    the others black).  <value> is what Python prints for str(round(float(v), 2)): correctly rounded to
 *    two decimals (half to even on the exact binary value), shortest form ("-0.0", "2.67", "12.5"),
 *    "inf", "-inf", "nan"; |v| >= 1e9 saturates to +-999999999.99.  Formatting runs on the device.
 *    The font is the project's own 5 x 7 bitmap (csrc/hud/d2d_font.h).  Text is sized in OUTPUT pixels:
 *    a cell is 6 s x 8 s pixels with s = max(1, height / 512) (integer division); line k starts at row
 *    8 s k, line 5 a further 5 s down; character j starts at column 6 s j; a glyph bit is an s x s block;
 *    what falls outside the picture is clipped.  Text is not a primitive: it is the colour of a pixel
 *    that NO primitive covers -- the glyph colour where a bit is set, else the background -- as the
 *    reference blits its text first, on background-coloured boxes.
 *
 * The shade recorder (d2dh_shade_update) keeps the shade lists of K tracked envs of a batch as the
 * reference does (:397, :416-419, :988-999): a shade at spawn, another after a step whenever |x - last_x|
 * or |y - last_y| exceeds `distance`.
 *
 * Conventions: d2d_render.h's.  `*_dev` are device pointers; all workspace is allocated at create; render
 * and update calls neither allocate nor synchronise and are ordered on `stream`; exceeding a capacity is
 * D2DH_E_ARG, never a truncated picture; 0 on success, else a D2DH_E_* code with the message in the
 * thread-local d2dh_last_error().  A ctx is not re-entrant.
 */
#ifndef D2D_HUD_H
#define D2D_HUD_H

#include <stdint.h>

#include "d2d_render.h"
#include "drone2d.h"

#ifdef __cplusplus
extern "C" {
#endif

#define D2DH_ABI_VERSION 1

/* layer bits of view->layers in this library only (D2DR_L_* pass through unchanged; D2DR_L_ALL stays 63) */
#define D2DH_L_TEXT 64u
#define D2DH_L_ARCS 128u
#define D2DH_L_SHADE 256u
#define D2DH_L_ALL 511u

#define D2DH_ARC_SEGS 32
#define D2DH_TEXT_LINES 6
#define D2DH_LINE_CHARS 40   /* bytes of one formatted line (longest: 21 label + 13 value characters) */
#define D2DH_MAX_SHADES 4096

typedef struct d2dh_ctx d2dh_t;

int32_t d2dh_abi_version(void);
const char* d2dh_last_error(void);

/* All device workspace: the extended lists of max_frames frames (trails of up to max_trail points, up to
 * max_shades shades) and their formatted text lines. */
int32_t d2dh_create(int32_t device, int32_t max_frames, int32_t max_trail, int32_t max_shades, int32_t max_width,
                    int32_t max_height, d2dh_t** out);
void d2dh_destroy(d2dh_t* ctx);

/* n_frames frames.  The arguments up to trail_len_dev are d2dr_render's own; then
 *   info_dev         float32 [n_frames][D2D_INFO_DIM] or NULL      NULL: no text
 *   shade_dev        float64 [n_frames][max_shades][3]             (x, y, frame angle), world units
 *   shade_count_dev  int32   [n_frames]   (values above max_shades count as max_shades)
 *                    both shade arguments or neither; NULL: no shades
 *   out_dev          uint8   [n_frames][height][width][3]
 * n_frames = 0 returns D2DH_OK and launches nothing. */
int32_t d2dh_render(d2dh_t* ctx, const d2dr_view* view, int32_t n_frames, const d2d_scn* scn_dev,
                    const double* state_dev, const float* obs_dev, const float* act_dev, const float* trail_dev,
                    const int32_t* trail_len_dev, const float* info_dev, const double* shade_dev,
                    const int32_t* shade_count_dev, uint8_t* out_dev, void* stream);

/* One launch, one lane per tracked env k (env env_ids_dev[k] of a batch of n_envs):
 *   state_dev        float64 [D2D_NSTATE][n_envs]  d2d_get_state's layout, read after the step
 *   term_dev, trunc_dev  uint8 [n_envs], the step's flags; both NULL: "after reset"
 *   shade_dev        float64 [n_tracked][max_shades][3], shade_count_dev int32 [n_tracked]
 *   last_dev         float64 [n_tracked][2]: the position of the last shade counted (equal to the last
 *                    stored pose until the list overflows)
 * Where the env finished this step (or after reset) the auto-reset has already put the new episode's
 * spawn pose into the state: the list restarts, count = 1, with that pose.  Otherwise, when |x - last_x|
 * or |y - last_y| exceeds `distance`, the pose is appended.  count keeps counting past max_shades and
 * poses beyond the capacity are not stored (trail_len's convention).  env_ids_dev is not read on the
 * host: check the ids where they are given (an id outside the batch makes its lane do nothing).
 * n_tracked = 0 returns D2DH_OK and launches nothing. */
int32_t d2dh_shade_update(int32_t device, int32_t n_tracked, const int32_t* env_ids_dev, int32_t n_envs,
                          const double* state_dev, const uint8_t* term_dev, const uint8_t* trunc_dev, double distance,
                          int32_t max_shades, double* shade_dev, int32_t* shade_count_dev, double* last_dev,
                          void* stream);

/* CPU twins: host pointers, the ctx capacities as arguments; byte-identical pictures and buffers.  The
 * update twin reads the ids and returns D2DH_E_ARG for one outside the batch. */
int32_t d2dh_render_host(const d2dr_view* view, int32_t n_frames, const d2d_scn* scn, const double* state,
                         const float* obs, const float* act, const float* trail, const int32_t* trail_len,
                         int32_t max_trail, const float* info, const double* shade, const int32_t* shade_count,
                         int32_t max_shades, uint8_t* out);
int32_t d2dh_shade_update_host(int32_t n_tracked, const int32_t* env_ids, int32_t n_envs, const double* state,
                               const uint8_t* term, const uint8_t* trunc, double distance, int32_t max_shades,
                               double* shade, int32_t* shade_count, double* last);

/* For tests: the text of a value (NUL-terminated, at most 13 characters), and the 7 rows of a glyph
 * (5 bits each, bit 4 leftmost; an unknown byte gives seven zeros). */
int32_t d2dh_format_host(float value, char out[16]);
int32_t d2dh_glyph_host(int32_t ch, uint8_t rows[7]);

#define D2DH_OK 0
#define D2DH_E_ARG 1
#define D2DH_E_HIP 2
#define D2DH_E_NOMEM 4

#ifdef __cplusplus
}
#endif
#endif /* D2D_HUD_H */
