/* d2d_heat.h -- C ABI of libd2d_heat.so: arena maps, histograms over the arena of where the first
 * episodes of a batch fly, where they end and which spawn positions they fail from, accumulated while
 * the episodes fly.
 *
 * d2d_heat_step is ONE launch per env step, after the env's own step, on that step's outputs.  Every
 * call is stream-ordered on `stream` (a hipStream_t; NULL = the default stream), neither allocates nor
 * synchronises, and so captures into a HIP graph.  All pointers are device pointers owned by the caller.
 * Return value: 0, or a hipError_t code (hipErrorInvalidValue = 1 for arguments that contradict each
 * other; nothing is launched then).
 *
 * The library reads drone2d.h for D2D_OBS_DIM, D2D_INFO_* and D2D_END_* only and calls nothing in the
 * other libraries.  Its arithmetic is csrc/heat/d2d_heat_core.h.
 *
 * Position and cell.  The position of env i is obs[i][6:8] (2 p / (W, H) - 1), taken from
 * terminal_obs on the step where term | trunc is set, exactly as the flight recorder of d2d_eval.h takes
 * it.  d2d_heat_cell2 maps it to a cell of the Gy x Gx grid (row 0 on top) or to "outside".
 *
 * Planes.  Per group g there are D2D_HEAT_PLANES uint32 planes [Gy][Gx] and one `outside` counter per
 * plane: planes [n_groups][6][Gy][Gx], outside [n_groups][6].  A count whose position is outside the
 * arena (or not finite) goes to the plane's outside counter of its group instead of a cell.
 *
 * Per-env state: alive u8 [n] (the env is still in its first episode), spawn_cell i32 [n] (the cell of
 * its reset observation, -1 outside), env_group i32 [n] or NULL (all 0); the host has checked every
 * group id against n_groups.
 *
 * Only integer atomics touch the planes, so the result does not depend on the order of the adds and is
 * identical from run to run.  No plane can wrap while n x steps < 2^32, which the host checks.
 *
 * Aggregation.  A key is (group, plane, cell or outside).  Within a wave, lanes that hold the same key
 * are found by ballot and their leader adds the count of all of them.  Path D2D_HEAT_PATH_LDS: the
 * leaders add into a hash table in LDS (D2D_HEAT_TABLE slots, keyed by the key itself), which a
 * workgroup keeps across the 256-env chunks it walks and empties into the planes with one global atomic
 * per distinct key, at its end or when the next chunk might not fit.  Path D2D_HEAT_PATH_GLOBAL: the
 * leaders add to the planes directly.  D2D_HEAT_PATH_AUTO takes the table for grids of up to
 * D2D_HEAT_LDS_MAX_CELLS cells: beyond that the envs of one workgroup rarely share a cell and the table
 * would only add its own cost.
 */
#ifndef D2D_HEAT_H
#define D2D_HEAT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define D2D_HEAT_ABI_VERSION 1
#define D2D_HEAT_PLANES 6
#define D2D_HEAT_MAX_GRID 256       /* Gx and Gy are each 1 .. 256 */
#define D2D_HEAT_MAX_GROUPS 4096    /* keeps a key (group, plane, cell) inside 31 bits */
#define D2D_HEAT_CHUNK 256          /* envs per workgroup pass */
#define D2D_HEAT_MAX_BLOCKS 256
#define D2D_HEAT_TABLE 4096         /* LDS hash slots per workgroup */
#define D2D_HEAT_LDS_MAX_CELLS 16384

enum {
    D2D_HEAT_VISIT = 0,           /* one per env step of an episode still in its first run */
    D2D_HEAT_SPAWN = 1,           /* one per finished episode, at the cell of its reset observation */
    D2D_HEAT_SPAWN_SUCCESS = 2,   /* ... where cause & D2D_END_REACH */
    D2D_HEAT_SPAWN_COLLISION = 3, /* ... where the episode is a collision (D2D_MON_COLLISION) */
    D2D_HEAT_END_COLLISION = 4,   /* collision episode, at its terminal position */
    D2D_HEAT_END_OTHER = 5        /* neither success nor collision, at its terminal position */
};

enum { D2D_HEAT_PATH_AUTO = 0, D2D_HEAT_PATH_LDS = 1, D2D_HEAT_PATH_GLOBAL = 2 };
enum { D2D_HEAT_DENSITY = 0, D2D_HEAT_RATE = 1 };

int32_t d2d_heat_abi_version(void);

typedef struct d2d_heat_args {
    int32_t n;         /* envs */
    int32_t n_groups;  /* 1 .. D2D_HEAT_MAX_GROUPS */
    int32_t gx, gy;    /* 1 .. D2D_HEAT_MAX_GRID each */
    int32_t obs_dim;   /* must be D2D_OBS_DIM (27) */
    int32_t info_dim;  /* must be D2D_INFO_DIM (12) */
    int32_t path;      /* D2D_HEAT_PATH_* */
    int32_t pad;
    const float* obs;          /* [n][27] this step's observations */
    const float* terminal_obs; /* [n][27] */
    const uint8_t* term;       /* [n] 0 / 1 */
    const uint8_t* trunc;      /* [n] */
    const float* info;         /* [n][12] */
    const int32_t* env_group;  /* [n] or NULL */
    uint8_t* alive;            /* [n] */
    int32_t* spawn_cell;       /* [n] */
    uint32_t* planes;          /* [n_groups][6][gy][gx] */
    uint32_t* outside;         /* [n_groups][6] */
} d2d_heat_args;

/* alive = 1, spawn_cell = the cell of obs0[i][6:8] (args' obs, term, trunc, info, terminal_obs unused) */
int32_t d2d_heat_begin(const d2d_heat_args* args, const float* obs0, void* stream);

/* Alive envs deposit VISIT at their position; those with term | trunc set also deposit SPAWN and, by
 * their outcome class, SPAWN_SUCCESS / SPAWN_COLLISION at spawn_cell and END_COLLISION / END_OTHER at the
 * terminal position, and clear alive. */
int32_t d2d_heat_step(const d2d_heat_args* args, void* stream);

/* planes = 0, outside = 0 (alive and spawn_cell are d2d_heat_begin's) */
int32_t d2d_heat_clear(const d2d_heat_args* args, void* stream);

typedef struct d2d_heat_colour_args {
    int32_t n_groups;  /* frames painted: frame k shows group k */
    int32_t gx, gy;
    int32_t h, w;      /* frame size, 1 .. 16384 each */
    int32_t mode;      /* D2D_HEAT_DENSITY: plane_a; D2D_HEAT_RATE: plane_a over plane_b */
    int32_t plane_a, plane_b;
    int32_t alpha;     /* 0 .. 255, one for every painted cell */
    int32_t bg_shared; /* 1: bg is one frame [h][w][3]; 0: one per group [n_groups][h][w][3] */
    uint32_t min_count; /* rate: cells whose denominator is below it (or 0) stay transparent */
    int32_t pad;
    const uint32_t* planes; /* [n_groups][6][gy][gx] */
    const uint8_t* bg;
    uint8_t* out;           /* [n_groups][h][w][3], not overlapping bg */
    uint32_t* peak;         /* [n_groups] scratch: the maximum of plane_a per group (density) */
} d2d_heat_colour_args;

/* Pixel (x, y) of frame k reads cell (x gx / w, y gy / h) of group k, by integer division.  Density:
 * level = d2d_heat_level(count, peak of the plane), colour = d2d_heat_ramp; cells of level 0 (and every
 * cell of a plane whose peak is 0) keep the background.  Rate: level = d2d_heat_rate_level(num, den),
 * colour = d2d_heat_rate_colour; cells with den < max(min_count, 1) keep the background.  Painted
 * pixels are d2d_heat_blend(bg, colour, alpha) per channel. */
int32_t d2d_heat_colour(const d2d_heat_colour_args* args, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* D2D_HEAT_H */
