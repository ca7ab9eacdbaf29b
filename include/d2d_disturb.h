/* d2d_disturb.h -- C ABI of libd2d_disturb.so: what stands between the env and the policy in a disturbed
 * evaluation (drone2d_amd.disturb): sensor noise and obstacle-sensor dropout on the observations the
 * policy sees, actuator noise, lag and motor loss on the actions the env gets.
 *
 * The disturbance is a LEVEL AXIS of the batch: env i flies under row env_level[i] of a table
 * params [L][D2D_DISTURB_PARAMS], the way it acts under policy env_policy[i] of a policy bank.  An env
 * whose level is outside [0, L) is skipped: the id never indexes the table, d2d_disturb_obs copies its row
 * unchanged and d2d_disturb_act leaves its action and its history alone.
 *
 * Both calls are ONE launch, stream-ordered on `stream` (a hipStream_t; NULL = the default stream), do
 * not synchronise and do not allocate, so they capture into a HIP graph.  All pointers are device
 * pointers.  Return value: 0, or a hipError_t code (hipErrorInvalidValue = 1 for arguments that
 * contradict each other; nothing is launched then).
 *
 * Arithmetic.  Every float32 operation below is a single IEEE operation rounded to nearest (the library is
 * built with -ffp-contract=off and spells the noise as __fmul_rn then __fadd_rn), in the order written, so a
 * float32 restatement (drone2d_amd.disturb.HostDisturber) gives the same bits from the same draws.
 * clip(x, -1, 1) = fminf(fmaxf(x, -1), 1).
 *
 * Neutral means skipped.  A stage whose parameter has its neutral value (sigma 0, p 0, delay 0, gain 1)
 * does not run for that env: the value passes through bit for bit (the sign of zero, infinities and NaN
 * payloads included); it is not computed as x + 0 z.  No Philox block is generated for a skipped stage,
 * for a channel block outside the mask, or for a pair of normals nothing uses.
 *
 * Row invariance: env i's outputs are a function of its own row, its level's parameters and
 * (seed, env_id_base + i, t) alone, so shards of a batch give the rows of the whole batch.
 */
#ifndef D2D_DISTURB_H
#define D2D_DISTURB_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define D2D_DISTURB_ABI_VERSION 1
#define D2D_DISTURB_OBS_DIM 27
#define D2D_DISTURB_ACT_DIM 2
#define D2D_DISTURB_PARAMS 8      /* float32 words per level */
#define D2D_DISTURB_MAX_DELAY 8   /* env steps: 133 ms at the env's 60 Hz */
#define D2D_DISTURB_HIST_ROWS (D2D_DISTURB_MAX_DELAY + 1)
#define D2D_DISTURB_SLOTS 3       /* obstacle-sensor slots: channels 8 + 3 j .. 10 + 3 j */
#define D2D_DISTURB_SLOT0 8
#define D2D_DISTURB_OBS_BLOCKS 7  /* Philox blocks of four normals that cover 27 channels */

/* Philox counter word 2 of the three streams ("DS"); they differ from D2D_EVAL_NOISE_TAG (0x45560000) and
 * from the env's spawn words 0, 1, 2 */
#define D2D_DISTURB_TAG_OBS  0x44530000u
#define D2D_DISTURB_TAG_DROP 0x44530001u
#define D2D_DISTURB_TAG_ACT  0x44530002u

/* a level's row of params */
enum {
    D2D_DISTURB_P_OBS_SIGMA = 0, /* >= 0; neutral 0 */
    D2D_DISTURB_P_ACT_SIGMA = 1, /* >= 0; neutral 0 */
    D2D_DISTURB_P_DROPOUT = 2,   /* 0 <= p <= 1; neutral 0 */
    D2D_DISTURB_P_GAIN_L = 3,    /* >= 0; neutral 1: the fraction of its thrust the left motor delivers */
    D2D_DISTURB_P_GAIN_R = 4,
    D2D_DISTURB_P_DELAY = 5      /* an integer 0 .. D2D_DISTURB_MAX_DELAY stored as float; neutral 0.  The kernel
                                    clamps it to that range, so no value can index outside hist. */
    /* words 6 and 7 are reserved and must be 0 */
};

enum {
    D2D_DISTURB_NOISE_NONE = 0,  /* no draw is made: sensor noise, dropout and actuator noise are off; lag and
                                    motor loss, which draw nothing, still run */
    D2D_DISTURB_NOISE_GIVEN = 1, /* the draws are z_obs, u_drop, z_act */
    D2D_DISTURB_NOISE_PHILOX = 2 /* the draws come from Philox4x32-10, see below */
};

int32_t d2d_disturb_abi_version(void);

typedef struct d2d_disturb_args {
    int32_t n;           /* envs in this batch (this rank's shard) */
    int32_t t;           /* the env step the observations / actions are for, >= 0 */
    int32_t n_levels;    /* L >= 1 */
    int32_t noise_mode;  /* D2D_DISTURB_NOISE_* */
    uint32_t obs_mask;   /* bit c set: channel c takes sensor noise (bits 27 .. 31 must be 0); batch-wide */
    int32_t pad;
    int64_t env_id_base; /* global id of env 0: env i is g = env_id_base + i */
    uint64_t seed;       /* Philox key (lo, hi) */
    const float* params;      /* [L][D2D_DISTURB_PARAMS] */
    const int32_t* env_level; /* [n] */

    /* d2d_disturb_obs */
    const float* obs_in; /* [n][27]: the env's observations; never written */
    float* obs_out;      /* [n][27]: what the policy sees; a buffer of its own (obs_out == obs_in is refused) */
    const float* z_obs;  /* [n][27], mode 1 */
    const float* u_drop; /* [n][3], mode 1 */
    float* z_obs_out;    /* [n][27] or NULL: the normals used; 0 where none was (stage skipped, channel unmasked) */
    float* u_drop_out;   /* [n][3] or NULL: the uniforms used; 0 where the stage was skipped */

    /* d2d_disturb_act */
    float* act;          /* [n][2], in place: the tensor d2d_step will read */
    float* hist;         /* [D2D_DISTURB_HIST_ROWS][n][2], the caller's; needs no clearing when t starts at 0 */
    const float* z_act;  /* [n][2], mode 1 */
    float* z_act_out;    /* [n][2] or NULL: the normals used; 0 where the stage was skipped */
} d2d_disturb_args;

/* Draws (mode 2).  (w0, w1, w2, w3) = Philox4x32-10(counter (g, t, TAG, b), key (seed lo, seed hi)), the
 * function of the env library's spawn stream and of d2d_eval.h's policy noise, and the uniform and
 * Box-Muller formulas are d2d_eval.h's: u_k = ((w_k >> 8) + 0.5) * 2^-24 in float32 (so 0 < u <= 1);
 * words (0, 1) give normals 0 and 1 of the block, r = sqrtf(-2 logf(u0)), (r cosf(2 pi u1), r sinf(2 pi u1)),
 * words (2, 3) give normals 2 and 3 in the same way.
 *   sensor noise    TAG_OBS,  b = c >> 2: channel c takes normal c & 3 of block c >> 2
 *   dropout         TAG_DROP, b = 0: slot j takes the uniform of word j
 *   actuator noise  TAG_ACT,  b = 0: the left motor takes normal 0, the right one normal 1
 *
 * d2d_disturb_obs: obs_out[i] = the stages below applied to obs_in[i], for an env with a level in [0, L):
 *   1. sensor noise (obs_sigma != 0, mode != 0): for every channel c of obs_mask,
 *        x[c] = __fadd_rn(x[c], __fmul_rn(obs_sigma, z_c)).  No clip.
 *   2. dropout (dropout_p != 0, mode != 0): for slot j = 0, 1, 2 with u_j < dropout_p, channels
 *        8 + 3 j .. 10 + 3 j become (1, 0, 0), the env's "nothing seen" triple.  After the noise: a dropped
 *        slot is clean.
 * hipErrorInvalidValue: args NULL, n < 1, t < 0, L < 1, a mode outside 0 .. 2, mask bits above 26,
 * env_id_base < 0 or env_id_base + n > 2^32, params, env_level, obs_in or obs_out NULL, obs_out == obs_in,
 * mode 1 without z_obs or u_drop. */
int32_t d2d_disturb_obs(const d2d_disturb_args* args, void* stream);

/* d2d_disturb_act: act[i] in place, for an env with a level in [0, L):
 *   1. actuator noise (act_sigma != 0, mode != 0): a1 = clip(__fadd_rn(a, __fmul_rn(act_sigma, z)), -1, 1)
 *   2. lag: hist[t % 9][i] = a1 (always, so levels of different delay share a history);
 *        delay != 0: a2 = hist[max(t - delay, 0) % 9][i] -- the first `delay` steps apply the first action
 *   3. motor loss, per motor with its gain g != 1: the env maps an action to the thrust (a / 2 + 0.5) * 1000, so a
 *        motor that delivers the fraction g of it is a3 = clip((a2 + 1) * g - 1, -1, 1), three operations
 * The history is read back from rows written at steps max(t - 8, 0) .. t of the same flight: call it for
 * t = 0, 1, 2, ... of one flight and nothing has to be cleared between flights.
 * hipErrorInvalidValue: as above for the common fields, act or hist NULL or not 8-byte aligned (rows are
 * moved as one 8-byte word), mode 1 without z_act. */
int32_t d2d_disturb_act(const d2d_disturb_args* args, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* D2D_DISTURB_H */
