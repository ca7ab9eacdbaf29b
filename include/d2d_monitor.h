/* d2d_monitor.h -- C ABI of libd2d_monitor.so: the episode monitor of a training run (what the
 * reference's TensorboardLogger callback collects, tensorboardlogger.py:49-110, plus the per-term
 * breakdown of every finished episode's return).
 *
 * d2d_monitor_step is ONE launch per env step: it digests that step's term / trunc / info outputs into
 * per-env running state and, for the envs whose episode ended, into a small table of partial sums;
 * d2d_monitor_flush folds the table into one vector of D2D_MON_K doubles and clears it.  Every call is
 * stream-ordered on `stream` (a hipStream_t; NULL = the default stream), neither allocates nor
 * synchronises, and so captures into a HIP graph.  All pointers are device pointers owned by the
 * caller.  Return value: 0, or a hipError_t code (hipErrorInvalidValue = 1 for arguments that contradict
 * each other; nothing is launched then).
 *
 * The library reads drone2d.h for the D2D_INFO_* and D2D_END_* constants only and calls nothing in the
 * other libraries.
 *
 * Per-env state (one lane per env)
 *   run     f64 [6][n], field-major: the running sums of this episode's six reward terms,
 *           D2D_INFO_CA .. D2D_INFO_AA (each f32 info value widened to f64, then added)
 *   minclr  f32 [n]: the episode's minimum D2D_INFO_DCLOSE; m = d < m ? d : m (a NaN d is ignored)
 *   live    u8 [n]: the monitor saw this episode start
 * Per env and step: run += the row's terms; minclr = min; at done = term | trunc the episode is an
 * EVENT: live -> its deposit vector is the columns below, not live -> SKIPPED = 1 and 0 elsewhere;
 * after it run = 0, minclr = +inf, live = 1.
 *
 * Summation order (part of the contract: no float atomics anywhere, results are bit-identical from run
 * to run, and a host program that follows this order reproduces them bit for bit)
 *   - env i is lane i % 64 of wave (i / 64) % 4 of chunk i / 256; workgroup b of n_blocks takes chunks
 *     b, b + n_blocks, b + 2 n_blocks, ... in that order;
 *   - a wave without an event adds nothing (a wave-uniform branch on a ballot).  A wave with events
 *     starts from +0.0 and adds its events' vectors in ascending lane order;
 *   - the chunk's sum starts from +0.0 and adds the sums of its waves that had events, in wave order;
 *   - a chunk with an event is added to row b of `part` (part[b] = part[b] + chunk sum), chunk after
 *     chunk in walk order;
 *   - d2d_monitor_flush starts from +0.0 and adds rows 0, 1, ... n_blocks - 1 in that order.
 * IEEE specials pass through (D2D_INFO_DCLOSE is +inf without obstacles; the collision-avoidance term
 * can be inf or NaN, as in the reference).  The sign and payload of a NaN are not portable between
 * adders, so d2d_monitor_flush writes every NaN as the quiet NaN 0x7FF8000000000000.
 */
#ifndef D2D_MONITOR_H
#define D2D_MONITOR_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define D2D_MON_ABI_VERSION 1
#define D2D_MON_TERMS 6        /* D2D_INFO_CA .. D2D_INFO_AA */
#define D2D_MON_CHUNK 256      /* envs per workgroup pass */
#define D2D_MON_MAX_BLOCKS 1024

/* columns of a `part` row and of the flushed vector (float64) */
enum {
    D2D_MON_EPISODES = 0,    /* deposited episodes                                              */
    D2D_MON_SUCCESS = 1,     /* info['n_successful_runs'] == 1: cause & REACH                   */
    D2D_MON_FAIL = 2,        /* info['n_failed_runs'] == 1: cause & (COLLISION | TIMEUP | AA)   */
    D2D_MON_COLLISION = 3,   /* info['n_collisions'] == 1: COLLISION and none of the other three
                                (the overwrite order of drone_2d_env.py:595-610): D2D_ST_COLLISION */
    D2D_MON_TIMEUP = 4,      /* cause & D2D_END_TIMEUP                                          */
    D2D_MON_AA = 5,          /* cause & D2D_END_AA                                              */
    D2D_MON_LEN = 6,         /* sum of D2D_INFO_STEPS                                           */
    D2D_MON_TOTREW = 7,      /* sum of D2D_INFO_TOTREW                                          */
    D2D_MON_APE = 8,         /* sum of D2D_INFO_APE                                             */
    D2D_MON_RUN = 9,         /* 6 columns: sum over episodes of the episode's term sums (`run`)  */
    D2D_MON_LAST = 15,       /* 6 columns: sum of the terminal step's term values               */
    D2D_MON_LAST_REWARD = 21, /* sum of the terminal step's D2D_INFO_REWARD                     */
    D2D_MON_MINCLR = 22,     /* sum of the episode's minimum clearance where it is finite       */
    D2D_MON_MINCLR_N = 23,   /* ... and the number of those episodes                            */
    D2D_MON_SKIPPED = 24,    /* episodes that ended without the monitor having seen them start  */
    D2D_MON_K = 25
};

int32_t d2d_monitor_abi_version(void);

typedef struct d2d_monitor_step_args {
    int32_t n;         /* envs */
    int32_t info_dim;  /* must be D2D_INFO_DIM (12): a row is three 16-byte words */
    int32_t n_blocks;  /* 1 .. D2D_MON_MAX_BLOCKS: workgroups, and rows of part */
    int32_t pad;
    const uint8_t* term;  /* [n] 0 / 1 */
    const uint8_t* trunc; /* [n] */
    const float* info;    /* [n][12], 16-byte aligned */
    double* run;          /* [6][n] */
    float* minclr;        /* [n] */
    uint8_t* live;        /* [n] */
    double* part;         /* [n_blocks][D2D_MON_K] */
} d2d_monitor_step_args;

int32_t d2d_monitor_step(const d2d_monitor_step_args* args, void* stream);

/* out[k] = sum over rows of part[.][k] (ascending), NaN canonicalised; part = 0.  out: f64 [D2D_MON_K]. */
int32_t d2d_monitor_flush(double* part, int32_t n_blocks, double* out, void* stream);

/* run = 0, minclr = +inf, live = live_value (1 after a reset of every env; 0 when attaching to a batch
 * in mid-flight: the episodes under way are then counted as skipped, not deposited with partial sums). */
int32_t d2d_monitor_reset(int32_t n, double* run, float* minclr, uint8_t* live, int32_t live_value, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* D2D_MONITOR_H */
