/* d2d_eval.h -- C ABI of libd2d_eval.so: one fused evaluation step of the test loop
 * (drone2d_amd.evaluate.evaluate_policy; the reference's mode == "test", main.py:220-288).
 *
 * d2d_eval_step is ONE launch per env step and does two things:
 *   record half  digests the outputs of env step t-1 into the first-episode records (what
 *                harness.run_first_episodes does with where / mask ops after every step);
 *   act half     SB3's MlpPolicy actor (27-64-64-2, tanh) on the current observations, the policy
 *                noise, the clip to the action space: act_env, ready for d2d_step.
 * The call is stream-ordered on `stream` (a hipStream_t; NULL = the default stream), does not
 * synchronise and does not allocate, so a loop of (d2d_eval_step, d2d_step) captures into a HIP graph.
 * All pointers are device pointers.  Return value: 0, or a hipError_t code (hipErrorInvalidValue = 1
 * for arguments that contradict each other; nothing is launched then).
 *
 * Row invariance: env i's action is a function of its observation row, the weights and
 * (seed, env_id_base + i, t) alone -- bit for bit independent of n, of the row's place in the batch
 * and of the other rows.  Every output element is one k-ordered fmaf chain (the 32x32x2 fp32
 * matrix-core tile for the hidden layers, a 64-term loop for the output layer).
 */
#ifndef D2D_EVAL_H
#define D2D_EVAL_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define D2D_EVAL_ABI_VERSION 1
#define D2D_EVAL_OBS_DIM 27
#define D2D_EVAL_ACT_DIM 2
#define D2D_EVAL_HIDDEN 64
#define D2D_EVAL_NOISE_TAG 0x45560000u /* Philox counter word 2 of the policy-noise stream ("EV") */

enum {
    D2D_EVAL_NOISE_NONE = 0,   /* a = clip(mean): deterministic */
    D2D_EVAL_NOISE_GIVEN = 1,  /* z = noise[i] */
    D2D_EVAL_NOISE_PHILOX = 2  /* z from Philox4x32-10, see below */
};

int32_t d2d_eval_abi_version(void);

typedef struct d2d_eval_step_args {
    int32_t n;          /* envs in this batch (this rank's shard) */
    int32_t t;          /* call index: the env step the actions are for; the record half digests step t-1 */
    int32_t info_dim;   /* row length of prev_info and rows (D2D_INFO_DIM) */
    int32_t act;        /* 0: record only (the call after the last env step) */
    int32_t noise_mode; /* D2D_EVAL_NOISE_* */
    int32_t flight_cap; /* rows of flight (record half with flight: 1 <= t <= flight_cap) */
    int64_t env_id_base; /* global id of env 0: env i is g = env_id_base + i */
    uint64_t seed;      /* Philox key (lo, hi) */

    const float* obs;   /* [n][27]: the observations step t-1 returned (reset observations at t = 0) */

    /* act half */
    const float* w1;      /* [64][27]  mlp_extractor.policy_net.0.weight */
    const float* b1;      /* [64] */
    const float* w2;      /* [64][64]  mlp_extractor.policy_net.2.weight */
    const float* b2;      /* [64] */
    const float* w3;      /* [2][64]   action_net.weight */
    const float* b3;      /* [2] */
    const float* log_std; /* [2] (unused in mode 0) */
    const float* noise;   /* [n][2], mode 1 */
    float* noise_out;     /* [n][2] or NULL: the z that was used (modes 1, 2) */
    float* act_env;       /* [n][2]: clip(mean + exp(log_std) z, -1, 1) */

    /* record half: all NULL = skipped (t = 0).  done = term | trunc; new = done & !finished;
     * new: rows[i] = prev_info[i]; flight and !finished[i]: flight[t-1][i] = done ? prev_term_obs[i][6:8]
     * : obs[i][6:8]; finished[i] |= done; *remaining -= number of new (integer atomics). */
    const uint8_t* prev_term;   /* [n] 0 / 1 */
    const uint8_t* prev_trunc;  /* [n] */
    const float* prev_info;     /* [n][info_dim] */
    const float* prev_term_obs; /* [n][27] (needed with flight only) */
    uint8_t* finished;          /* [n] */
    float* rows;                /* [n][info_dim] */
    float* flight;              /* [flight_cap][n][2] or NULL; the caller pre-fills it with NaN */
    int32_t* remaining;         /* one int32: envs that have not finished their first episode */
} d2d_eval_step_args;

/* Mode 2: (w0, w1, ., .) = Philox4x32-10(counter (g, t, D2D_EVAL_NOISE_TAG, 0), key (seed lo, seed hi)),
 * the function of the env library's spawn stream (counter word 2 = 0, 1, 2 there);
 * u_k = ((w_k >> 8) + 0.5) * 2^-24 in float32; r = sqrtf(-2 logf(u0)); z = (r cosf(2 pi u1), r sinf(2 pi u1)). */
int32_t d2d_eval_step(const d2d_eval_step_args* args, void* stream);

/* The policy bank: one launch acts for envs that belong to different agents (a sweep of P agents x
 * S scenarios x R runs as one batch; drone2d_amd.evaluate.evaluate_policies).  Additive: the functions
 * above and D2D_EVAL_ABI_VERSION are unchanged; the bank carries a version of its own. */
#define D2D_EVAL_BANK_VERSION 1
#define D2D_EVAL_BANK_STRIDE  6084   /* floats per policy, in this order: W1 [64][27], b1 [64], W2 [64][64],
                                        b2 [64], W3 [2][64], b3 [2], log_std [2] */
typedef struct d2d_eval_bank {
    int32_t n_policies;          /* P >= 1 */
    int32_t pad;
    const float* params;         /* [P][D2D_EVAL_BANK_STRIDE] */
    const int32_t* env_policy;   /* [n]: the policy of env i */
} d2d_eval_bank;
int32_t d2d_eval_bank_version(void);

/* d2d_eval_step with one difference: env i's actor and log_std are those of policy env_policy[i].
 * args->w1 ... args->log_std must all be NULL; the record half, the noise modes, noise_out, env_id_base
 * and t are d2d_eval_step's.  One launch, stream-ordered, no synchronisation, no allocation.
 *
 * Row invariance extends to the bank: env i's action is, bit for bit, the action d2d_eval_step gives
 * the same observation row under policy env_policy[i] alone, whatever policies its neighbours have.
 * The map is arbitrary: a workgroup handles a 64-env chunk once per distinct policy present, in
 * ascending policy order, with that policy's weights staged, and keeps only that policy's rows.
 * An env whose id is outside [0, P) is skipped: the id never indexes the bank and act_env[i] is not
 * written.  hipErrorInvalidValue (nothing launched): bank NULL, P < 1, any of w1 ... log_std non-NULL,
 * with act != 0 a NULL params or env_policy (act == 0 reads neither), or what d2d_eval_step rejects. */
int32_t d2d_eval_step_bank(const d2d_eval_step_args* args, const d2d_eval_bank* bank, void* stream);

/* The sequenced step: d2d_eval_step (bank == NULL) or d2d_eval_step_bank with one difference: the call
 * index is *t_dev (a device int32), read when the kernel runs, so a captured segment of (d2d_eval_step_seq,
 * d2d_step) iterations replays with the index moving on.  Additive: the functions above, the argument
 * struct, D2D_EVAL_ABI_VERSION and D2D_EVAL_BANK_VERSION are unchanged, and so are the bits they produce.
 *
 * The index.  args->t must be 0; t = *t_dev feeds exactly what args->t feeds above: the Philox counter
 *   word of noise mode 2 and the flight[t-1] row.
 * Checks.  What the host checks of a by-value t the kernel decides: the record half runs when the prev_*
 *   pointers are non-NULL and t >= 1 (t = 0 with them given is a skipped record half, not an error);
 *   flight is written only for 1 <= t <= flight_cap, beyond that nothing of flight is touched and the
 *   rest of the step is done.  Every check that does not involve t stays on the host:
 *   hipErrorInvalidValue (nothing launched) for t_dev NULL, args->t != 0, flight_cap < 0 with flight
 *   given, or what d2d_eval_step / d2d_eval_step_bank reject.
 * The increment.  The call issues TWO launches: the step, every workgroup of which reads *t_dev and none
 *   of which writes it, then a one-thread launch that stores t + 1 (a plain store), ordered after the
 *   whole step by the stream, so no late-starting workgroup can see the moved index.  After the call
 *   *t_dev is t + 1; the caller rewinds it with an ordinary stream-ordered write.
 * Invariance.  Row invariance and bank invariance carry over word for word: for the same t every output
 *   (act_env, noise_out, rows, finished, flight, remaining) is the by-value call's, bit for bit.
 * Capture.  Stream-ordered, no synchronisation, no allocation: the call captures into a HIP graph. */
#define D2D_EVAL_SEQ_VERSION 1
int32_t d2d_eval_seq_version(void);
int32_t d2d_eval_step_seq(const d2d_eval_step_args* args, const d2d_eval_bank* bank /* NULL: one actor */,
                          int32_t* t_dev, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* D2D_EVAL_H */
