/* d2d_norm.h -- C ABI of libd2d_norm.so: reward normalisation in the rollout, the reward half of
 * Stable-Baselines3 2.1's VecNormalize(norm_obs=False, norm_reward=True, gamma=...): a discounted return
 * per env, a RunningMeanStd of those returns, and every reward divided by the running standard
 * deviation and clipped.
 *
 * d2d_norm_step is ONE call per env step (two small launches, see "Launch structure").  Every call is
 * stream-ordered on `stream` (a hipStream_t; NULL = the default stream), neither allocates nor
 * synchronises, and so captures into a HIP graph.  All pointers are device pointers owned by the
 * caller.  Return value: 0, or a hipError_t code (hipErrorInvalidValue = 1 for arguments that contradict
 * each other; nothing is launched then).  The library calls nothing in the other libraries.
 *
 * State (caller-owned)
 *   ret     f64 [n]: SB3's self.returns, the discounted return of each env's running episode
 *   rms     f64 [3] = (mean, var, count): SB3's RunningMeanStd of the returns; starts at (0, 1, 1e-4)
 *   part    f64 [n_blocks][2]: the step's partial sums (S1, S2) per workgroup; rewritten by every step
 *   ticket  i32 [1]: an arrival counter, 0 between calls (allocate it zeroed; the library leaves it 0)
 *
 * One step with training = 1, in float64, with add, mul, div and sqrt only, each expression evaluated
 * left to right exactly as written (the library is built with -ffp-contract=off):
 *   1. ret[i] = ret[i] * gamma + (double)rew[i]
 *   2. c = rms.mean as it was before this step;  d_i = ret[i] - c
 *      S1 = sum d_i,  S2 = sum d_i * d_i                     (in the summation order below)
 *      bm = S1 / n
 *      bv = S2 / n - bm * bm;  if (bv < 0) bv = 0            (a NaN stays a NaN)
 *   3. SB3's update_from_moments (batch mean - running mean is bm):
 *      tot    = count + n
 *      mean'  = mean + bm * n / tot
 *      M2     = var * count + bv * n + bm * bm * count * n / tot
 *      var'   = M2 / tot
 *      count' = tot
 *   4. x = (double)rew[i] / sqrt(var' + epsilon);  if (x < -clip) x = -clip;  if (x > clip) x = clip
 *      rew_out[i] = (float)x                                  (rounded once, to nearest even)
 *      The UPDATED variance: SB3's step_wait updates the statistics, then normalises.
 *   5. ret[i] = 0 where term[i] | trunc[i]                    (after step 4, as in SB3)
 * With training = 0 only step 4 runs, with the stored var; ret, rms, part and ticket are not touched
 * (and may be NULL, as may term and trunc).
 *
 * Summation order (part of the contract: no float atomics anywhere, results are bit-identical from run
 * to run, and a host program that follows this order reproduces them bit for bit).  S1 and S2 are summed
 * alike:
 *   - env i is lane i % 64 of wave (i / 64) % 4 of chunk i / 256; a lane at or past n contributes +0.0;
 *   - inside a wave the shuffle-down tree: v[l] = v[l] + v[l + s] for l < s, with s = 32, 16, 8, 4, 2, 1;
 *     the wave's sum is v[0];
 *   - the chunk's sum starts at wave 0's sum and adds the sums of waves 1, 2, 3 in that order;
 *   - workgroup b of n_blocks walks chunks b, b + n_blocks, b + 2 n_blocks, ... and adds each chunk's sum
 *     to part[b] in walk order, starting from +0.0 at every step;
 *   - the fold starts from +0.0 and adds rows 0, 1, ... n_blocks - 1 in that order.
 *
 * Launch structure: the scale of a step depends on every env's return at that step, so step 4 needs
 * the fold of the whole grid.  Two launches of n_blocks workgroups of 256 lanes: the first does steps 1
 * and 2 up to part[b]; in the second, every workgroup fetches the <= 1024 rows into LDS, its lane 0
 * folds them and does step 3 (every workgroup computes the same bits), then all lanes do steps 4 and 5
 * for the workgroup's chunks.  Every workgroup reads the old rms, so no workgroup may overwrite it while another has yet to
 * read it: each draws an integer ticket after its read, and the one that draws the last ticket writes
 * (mean', var', count') and sets the ticket back to 0.
 *
 * IEEE specials: the env's collision-avoidance term can be inf or NaN, as in the reference.  Such a
 * reward is not guarded: it passes through the formulas above and leaves rms non-finite for good,
 * exactly as it does in SB3.  Bit identity between this library and a host program holds for finite
 * inputs; for non-finite ones only the isnan / isinf pattern of rms and rew_out is the same (the sign
 * and payload of a NaN are the adder's own).
 */
#ifndef D2D_NORM_H
#define D2D_NORM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define D2D_NORM_ABI_VERSION 1
#define D2D_NORM_CHUNK 256       /* envs per workgroup pass */
#define D2D_NORM_MAX_BLOCKS 1024

int32_t d2d_norm_abi_version(void);

typedef struct d2d_norm_step_args {
    int32_t n;         /* envs, >= 1 */
    int32_t n_blocks;  /* 1 .. D2D_NORM_MAX_BLOCKS: workgroups, and rows of part */
    int32_t training;  /* 1: steps 1-5; 0: step 4 alone */
    int32_t pad;
    double gamma;
    double clip;
    double epsilon;
    const float* rew;     /* [n] the env's rewards */
    const uint8_t* term;  /* [n] 0 / 1 (training) */
    const uint8_t* trunc; /* [n] (training) */
    float* rew_out;       /* [n]; may be rew itself */
    double* ret;          /* [n] (training) */
    double* rms;          /* [3] */
    double* part;         /* [n_blocks][2] (training) */
    int32_t* ticket;      /* [1] (training) */
} d2d_norm_step_args;

int32_t d2d_norm_step(const d2d_norm_step_args* args, void* stream);

/* ret = 0 (the envs were reset) and, when rms is not NULL, rms = (0, 1, 1e-4). */
int32_t d2d_norm_reset(int32_t n, double* ret, double* rms, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* D2D_NORM_H */
