/* d2d_ppo.h -- C ABI of libd2d_ppo.so: one PPO minibatch update in five launches
 * (drone2d_amd.ppo.ManualStep).  The reference trains with
 * Stable-Baselines3 2.1's PPO.train (main.py:181-210); these kernels restate its loss head, the
 * backward pass through the two MLPs and clip_grad_norm_ + torch.optim.Adam over one flat
 * parameter buffer.
 *
 * All pointers are device pointers (float32 unless stated), every call is stream-ordered on
 * `stream` (a hipStream_t; NULL = the default stream) and launches without synchronising, so a
 * sequence of calls captures into a HIP graph.  Return value: 0, or a hipError_t code.
 */
#ifndef D2D_PPO_H
#define D2D_PPO_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define D2D_PPO_ABI_VERSION 6  /* v6 (round 4): d2d_ppo_adam_spread / d2d_ppo_wgrad_head_adam removed.  The control
                                  entry points below (d2d_ppo_ctl_*, *_ctl) are additive: every v6 function keeps
                                  its signature and behaviour, so the version stays; the control block has a
                                  version of its own (D2D_PPO_CTL_VERSION) */
#define D2D_PPO_HEAD_BLOCK 64  /* v1: 256 */

int32_t d2d_ppo_abi_version(void);

/* Advantage statistics of the minibatch (SB3 normalize_advantage: mean and unbiased std of
 * adv[idx[0..m)]): per-workgroup double partial sums ws[2 b] = sum, ws[2 b + 1] = sum of squares,
 * b < ceil(m / D2D_PPO_HEAD_BLOCK); d2d_ppo_mlp_backward finishes them. */
int32_t d2d_ppo_adv_stats(int32_t m, const int64_t* idx, const float* adv, double* ws, void* stream);

/* Reduces the head's partials: log_std_grad[d] = sum_b partial[b][3 + d] - ent_coef, and adds the
 * minibatch statistics to acc[0..3] (policy loss, value loss, entropy, clip fraction).  One
 * workgroup. */
int32_t d2d_ppo_head_finish(int32_t m, int32_t n_blocks, const float* partial, const float* log_std, float ent_coef,
                            float* log_std_grad, float* acc_pl, float* acc_vl, float* acc_ent, float* acc_clip,
                            void* stream);

/* clip_grad_norm_(max_norm) then one torch.optim.Adam step (betas b1, b2, eps; bias corrections
 * from the step counter *t, which is incremented) over n parameters p with gradients g and
 * moments m1, m2; g is clipped in place, as torch clips .grad.  One workgroup, n <= 16 384 (the
 * policy has ~10 k parameters).  The moments are scaled as torch scales them, by the float nearest to
 * 1 - beta of the decimal beta that b1 / b2 round (0.9, 0.999), not by 1 - (float)beta; the bias
 * corrections are float32 (powf of the float beta). */
int32_t d2d_ppo_adam(int32_t n, float* p, float* g, float* m1, float* m2, float* t, float lr, float b1, float b2,
                     float eps, float max_norm, void* stream);

/* Weight and bias gradients of up to D2D_PPO_WGRAD_MAX linear layers in one launch (+ one reduce):
 * for problem k, g[w_off[k] + i q + j] = sum_r a_k[r][i] b_k[r][j] (i < p[k], j < q[k]; rows r < m;
 * a_k row stride lda[k], b_k ldb[k]; p, q <= 64) and g[b_off[k] + i] = sum_r a_k[r][i].  `a` and `b`
 * are host arrays of device pointers.  partial: device scratch of
 * d2d_ppo_wgrad_chunks(m) x row_len floats; g[0 .. row_len) is overwritten (entries no problem
 * covers become 0). */
#define D2D_PPO_WGRAD_MAX 8
int32_t d2d_ppo_wgrad(int32_t m, int32_t n_problems, const float* const* a, const int32_t* lda, const float* const* b,
                      const int32_t* ldb, const int32_t* p, const int32_t* q, const int32_t* w_off,
                      const int32_t* b_off, int32_t row_len, float* partial, float* g, void* stream);
/* d2d_ppo_wgrad and d2d_ppo_head_finish in two launches instead of three (the reduce's last
 * workgroup finishes the head; log_std_grad must point at two slots inside g[0 .. row_len), which
 * the reduce leaves to the head).  Added in ABI v2. */
int32_t d2d_ppo_wgrad_head(int32_t m, int32_t n_problems, const float* const* a, const int32_t* lda,
                           const float* const* b, const int32_t* ldb, const int32_t* p, const int32_t* q,
                           const int32_t* w_off, const int32_t* b_off, int32_t row_len, float* partial, float* g,
                           int32_t n_blocks, const float* head_partial, const float* log_std, float ent_coef,
                           float* log_std_grad, float* acc_pl, float* acc_vl, float* acc_ent, float* acc_clip,
                           void* stream);
int32_t d2d_ppo_wgrad_chunks(int32_t m);

/* The two MLPs (policy 27-64-64-2, value 27-64-64-1, tanh) per minibatch sample, four threads per
 * (sample, net) each owning a quarter of every layer's units.  weights: 12 device pointers, per net (policy, then value): W1 [64][27], b1 [64],
 * W2 [64][64], b2 [64], W3 [od][64], b3 [od].  bufs: 10 device pointers, per net: h1 [m][64],
 * h2 [m][64], out [m][od] (the action mean / the value), g1 [m][64], g2 [m][64].
 * mlp_forward: the rollout rows idx[0..m) of obs [.][27] through both nets (h1, h2, out) and the
 * gathered observations into xg [m][27].  mlp_backward: the loss head below (gout[0] =
 * d loss / d mean [m][2], gout[1] = d loss / d value [m]; partial[d2d_ppo_mlp_partial_rows(m)][5],
 * finished by d2d_ppo_head_finish with n_blocks = d2d_ppo_mlp_partial_rows(m)) and the hidden layers' output gradients g2, g1.
 * The head: Gaussian log-density of act under (mean, exp(log_std)), ratio = exp(logp - old_logp),
 * clipped surrogate with advantages normalised by d2d_ppo_adv_stats' partials (normalize != 0),
 * squared value error scaled by vf_coef.  The head takes the action mean as a double sum over h2
 * (mlp_backward sums it again instead of reading `out`), z = (a - mean) / sigma, logp - old_logp and
 * the normalised advantage in double and rounds each to float once (at a small sigma their float32
 * roundings, times 1 / sigma and z, were the gradient's largest error). */
int32_t d2d_ppo_mlp_forward(int32_t m, const int64_t* idx, const float* obs, const float* const* weights,
                            float* const* bufs, float* xg, void* stream);
/* mlp_forward plus d2d_ppo_adv_stats' partials into ws from the same launch (adv != NULL; the
 * matrix-core forward's workgroups each take D2D_PPO_HEAD_BLOCK rows).  Added in ABI v2. */
int32_t d2d_ppo_mlp_forward_adv(int32_t m, const int64_t* idx, const float* obs, const float* adv,
                                const float* const* weights, float* const* bufs, float* xg, double* ws, void* stream);
int32_t d2d_ppo_mlp_partial_rows(int32_t m);
int32_t d2d_ppo_mlp_backward(int32_t m, const int64_t* idx, const float* act, const float* old_logp, const float* adv,
                             const float* ret, const float* log_std, const double* ws, int32_t normalize, float clip,
                             float vf_coef, const float* const* weights, float* const* bufs, float* const* gout,
                             float* partial, void* stream);

/* The per-epoch minibatch shuffles of one update (SB3 PPO.train: RolloutBuffer.get draws
 * np.random.permutation(buffer_size) every epoch): out[e n + i] = pi_e(i) for e < n_perm, i < n, each
 * pi_e a bijection of [0, n) -- an 8-round keyed Feistel network on the next power of two >= n, walked
 * back into [0, n) -- keyed by (seed, *counter + e).  A one-thread launch after it advances *counter
 * (one uint64 in device memory) by n_perm, so a captured graph draws new shuffles on every replay.
 * Two launches, replacing torch.randperm's sort (~0.24 ms per 1 M-sample epoch).  Added in ABI v4. */
int32_t d2d_ppo_permute(int64_t n, int32_t n_perm, uint64_t seed, uint64_t* counter, int64_t* out, void* stream);

/* One step of SB3 OnPolicyAlgorithm.collect_rollouts over n envs in one launch (ABI v4): both MLPs
 * on the observations of step t, the Gaussian action a = mean + exp(log_std) noise (stored
 * unclipped, clipped to [-1, 1] into act_env for the env), its log-density and the value into row t of
 * the rollout buffers ([T][n] rows, row t = samples t n .. t n + n - 1); for t >= 1 also step t-1's
 * env outputs (reward, done = terminated | truncated) into row t-1 and per-workgroup episode
 * statistics of step t-1.  t == T: the bootstrap value of obs, step T-1's env outputs, then
 * RolloutBuffer.compute_returns_and_advantage (GAE(gamma, gae_lambda) with the episode starts, same
 * operation order as the torch restatement) into adv_buf / ret_buf.  Time-limit bootstrapping of
 * truncated episodes is d2d_ppo_rollout_step_tb's (declared with the step, below); this entry point
 * records the env's reward as it is (the reference never truncates). */
/* The minibatch gradient in one launch (ABI v5): what d2d_ppo_mlp_forward_adv + d2d_ppo_mlp_backward +
 * d2d_ppo_wgrad compute, with every per-sample activation and gradient kept on chip.  Workgroup
 * (x, net) handles the 64-sample chunks x, x + R, ... (R = d2d_ppo_fused_rows(m)) of rows idx[0..m) and
 * writes its net's weight / bias gradient sums into row x of wpart ([R][row_len], at offsets[6 net
 * + k] for W1, b1, W2, b2, W3, b3 of net 0 = policy, 1 = value) and its loss-head sums into row x
 * (policy) / R + x (value) of hpart ([2 R][5], d2d_ppo_mlp_backward's partial-row meaning).  ws: the
 * minibatch's d2d_ppo_adv_stats partials (normalize != 0).  d2d_ppo_grad_reduce then adds the rows
 * into g and finishes the head (log_std gradient, statistics) as d2d_ppo_wgrad_head does. */
int32_t d2d_ppo_fused_rows(int32_t m);
int32_t d2d_ppo_fused_grad(int32_t m, const int64_t* idx, const float* obs, const float* act, const float* old_logp,
                           const float* adv, const float* ret, const float* log_std, const double* ws, int32_t normalize,
                           float clip, float vf_coef, const float* const* weights, const int32_t* offsets,
                           int32_t row_len, float* wpart, float* hpart, void* stream);
int32_t d2d_ppo_grad_reduce(int32_t n_rows, int32_t row_len, const float* partial, float* g, int32_t n_blocks,
                            const float* head_partial, int32_t m, const float* log_std, float ent_coef,
                            float* log_std_grad, float* acc_pl, float* acc_vl, float* acc_ent, float* acc_clip,
                            void* stream);

/* ---------------------------------------------------------------------------------------------------
 * PPO control: schedules, value clipping, approx_kl and SB3's target_kl stop inside a captured update.
 *
 * The by-value coefficients of the entry points above are frozen when an update is captured into a
 * HIP graph, and nothing in a replayed update can wait for the host.  The *_ctl entry points read
 * their coefficients from, and leave their decisions in, one small block of device memory instead:
 * the host writes the first four words before each update (one stream-ordered copy outside the
 * graph) and reads the block back with the update's statistics.  Layout (8 x 4 bytes; mirrored by
 * drone2d_amd.ppo.D2DPPOCtl):
 *
 *   word 0  float   lr        learning rate of this update
 *   word 1  float   clip      clip_range of this update
 *   word 2  float   clip_vf   clip_range_vf; negative: value clipping off
 *   word 3  float   kl_limit  1.5 * target_kl, or +inf (never stop)
 *   word 4  int32   stop      set by d2d_ppo_adam_ctl when a minibatch's KL exceeds kl_limit
 *   word 5  int32   count     minibatches whose statistics were recorded (the stopping one included)
 *   word 6  float   kl_sum    sum of the recorded minibatches' approx_kl, in launch order
 *   word 7  float   kl_last   approx_kl of the last recorded minibatch
 *
 * One update is: d2d_ppo_ctl_reset, then per minibatch d2d_ppo_fused_grad_ctl, d2d_ppo_grad_reduce_ctl,
 * (multi-rank: the collective over g and kl_last,) d2d_ppo_adam_ctl.  SB3's order (PPO.train): the
 * minibatch's statistics are recorded, approx_kl = mean((ratio - 1) - log_ratio) is computed, and if
 * it exceeds kl_limit that minibatch's optimiser step is not taken and the rest of the update is
 * skipped.  Once `stop` is set, every later *_ctl launch of the update returns at once (the fused
 * gradient before its first barrier: the flag is uniform over the grid), so a stopped update still
 * executes its launches, as near-empty ones.  The shuffles (d2d_ppo_permute) and the up-front
 * advantage statistics are not part of the control path: a stopped update has drawn all its n_epochs
 * shuffles and advanced the shuffle counter by n_epochs, so a run is reproducible whether or not an
 * update stopped.
 *
 * The decision sits in d2d_ppo_adam_ctl, not in the reduce, so that a multi-rank run can replace
 * kl_last by its rank mean between the two (every rank must take the same decision).
 *
 * Only the fused path (d2d_ppo_fused_grad) has control variants.  The separate kernels
 * (d2d_ppo_mlp_forward_adv / d2d_ppo_mlp_backward / d2d_ppo_wgrad_head, D2D_PPO_FUSED=0) are a
 * diagnostic A/B path; drone2d_amd.ppo.ManualStep refuses the control path there with an error. */
#define D2D_PPO_CTL_VERSION 1
typedef struct d2d_ppo_ctl {
    float lr;
    float clip;
    float clip_vf;
    float kl_limit;
    int32_t stop;
    int32_t count;
    float kl_sum;
    float kl_last;
} d2d_ppo_ctl;
int32_t d2d_ppo_ctl_version(void);

/* The first launch of an update: stop = 0, count = 0, kl_sum = 0, kl_last = 0 (the coefficients stay). */
int32_t d2d_ppo_ctl_reset(d2d_ppo_ctl* ctl, void* stream);

/* d2d_ppo_fused_grad (the same kernel, instantiated a second time) with clip and clip_vf read from
 * ctl.  old_values [rollout rows]: the rollout's stored value predictions (SB3 rollout_data.old_values,
 * not returns - advantages, which rounds differently); with clip_vf >= 0 the value head uses
 * values_pred = old + clamp(value - old, -clip_vf, clip_vf), value loss mean((ret - values_pred)^2),
 * whose gradient passes where |value - old| <= clip_vf (bounds included) and is zero elsewhere.  The
 * policy head's row of hpart has a sixth sum, sum((ratio - 1) - log_ratio): hpart is [2 R][6] here.
 * Returns without writing anything when ctl->stop is set. */
int32_t d2d_ppo_fused_grad_ctl(int32_t m, const int64_t* idx, const float* obs, const float* act,
                               const float* old_logp, const float* adv, const float* ret, const float* old_values,
                               const float* log_std, const double* ws, int32_t normalize, float vf_coef,
                               const float* const* weights, const int32_t* offsets, int32_t row_len, float* wpart,
                               float* hpart, const d2d_ppo_ctl* ctl, void* stream);

/* d2d_ppo_grad_reduce over the [n_blocks][6] head rows.  Nothing when ctl->stop is set; otherwise g,
 * log_std's gradient and the four statistics as d2d_ppo_grad_reduce, then (one thread, plain stores,
 * fixed order) count += 1, kl_last = the minibatch's approx_kl, kl_sum += kl_last. */
int32_t d2d_ppo_grad_reduce_ctl(int32_t n_rows, int32_t row_len, const float* partial, float* g, int32_t n_blocks,
                                const float* head_partial, int32_t m, const float* log_std, float ent_coef,
                                float* log_std_grad, float* acc_pl, float* acc_vl, float* acc_ent, float* acc_clip,
                                d2d_ppo_ctl* ctl, void* stream);

/* d2d_ppo_adam with lr read from ctl.  Nothing when ctl->stop is set; when kl_last > kl_limit one
 * thread sets stop and no thread steps (p, g, m1, m2 and *t stay as they are); otherwise
 * d2d_ppo_adam's step. */
int32_t d2d_ppo_adam_ctl(int32_t n, float* p, float* g, float* m1, float* m2, float* t, float b1, float b2, float eps,
                         float max_norm, d2d_ppo_ctl* ctl, void* stream);

typedef struct d2d_ppo_rollout {
    int32_t n;            /* envs */
    int32_t t;            /* rollout step of obs: 0 .. T */
    int32_t T;            /* rollout length */
    int32_t info_dim;     /* row length of prev_info (D2D_INFO_DIM) */
    int32_t info_totrew;  /* column of the episode return in prev_info (D2D_INFO_TOTREW) */
    float gamma;
    float gae_lambda_gamma; /* gamma * gae_lambda, rounded to float as torch rounds the scalar */
    int32_t pad;
    const float* obs;        /* [n][27] observations of step t (the env's output tensor) */
    const float* noise;      /* [n][2] N(0, 1) draws of step t (t < T) */
    const float* log_std;    /* [2] */
    const float* prev_rew;   /* step t-1's env outputs (t >= 1): reward [n] */
    const uint8_t* prev_term;   /* [n] 0 / 1 */
    const uint8_t* prev_trunc;  /* [n] 0 / 1 */
    const float* prev_info;  /* [n][info_dim], or NULL (episode returns not summed) */
    float* obs_buf;          /* [T][n][27] */
    float* act_buf;          /* [T][n][2] unclipped actions */
    float* logp_buf;         /* [T][n] */
    float* val_buf;          /* [T][n] */
    float* rew_buf;          /* [T][n] */
    uint8_t* done_buf;       /* [T][n] */
    uint8_t* start0;         /* [n] episode starts of step 0; t == T: replaced by done of step T-1 */
    float* act_env;          /* [n][2] */
    float* adv_buf;          /* [T][n] (t == T) */
    float* ret_buf;          /* [T][n] (t == T) */
    double* stats;           /* [T][ceil(n / 64)][2]: per workgroup, (episodes ended, sum of their returns) at
                                step t-1 */
} d2d_ppo_rollout;
int32_t d2d_ppo_rollout_step(const d2d_ppo_rollout* r, const float* const* weights, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Time-limit bootstrap inside the rollout step (additive to ABI v6; a version of its own).
 *
 * d2d_ppo_rollout_step with one difference: for t >= 1, env i with prev_trunc[i] != 0 records
 * rew = prev_rew[i] + gamma * V(prev_term_obs[i]) instead of prev_rew[i] -- in rew_buf row t-1 and, at
 * t == T, in the GAE recursion's step T-1 (SB3 2.1 collect_rollouts: rewards[idx] += gamma *
 * predict_values(terminal_observation) where TimeLimit.truncated).  prev_term_obs [n][27] is the env's
 * terminal-observation tensor of step t-1 (d2d_step's term_obs).
 *
 *  - One launch, ordered on the stream, no allocation and no synchronisation: the bootstrap is a second
 *    pass through the tile loop inside the same workgroup (a second instantiation of the step's kernel).
 *  - V(prev_term_obs[i]) is bit for bit the value this kernel's value head writes to val_buf when the
 *    same 27 floats arrive as an ordinary obs row: the same matrix-core tiles, tanh and 64-term output
 *    loop.  It does not depend on n, on the row's place or on its neighbours.
 *  - rew = prev_rew + (gamma * V): two float32 roundings, no contraction (torch's rew + gamma * tv).
 *  - Selected, never blended: rows with prev_trunc == 0 record prev_rew unchanged, bit for bit.  Their
 *    prev_term_obs rows are stale (the env writes finished envs' rows only) and may hold anything, NaN
 *    included; they are not loaded, and nothing of them reaches an output.
 *  - A workgroup none of whose 64 envs truncated at step t-1 does no second pass (the decision is
 *    uniform over the workgroup); within one that does, a 32-env tile without a truncated env is skipped.
 *  - The condition is prev_trunc != 0, whatever prev_term holds (the env never sets both).
 *  - done_buf, stats (episode counts and the raw info returns), start0, act_*, logp_buf, val_buf and
 *    obs_buf are what d2d_ppo_rollout_step writes.
 *  - prev_term_obs == NULL or t == 0: exactly d2d_ppo_rollout_step (the same kernel instantiation, the
 *    same bits).  hipErrorInvalidValue, with nothing launched, for whatever d2d_ppo_rollout_step rejects. */
#define D2D_PPO_TB_VERSION 1
int32_t d2d_ppo_tb_version(void);
int32_t d2d_ppo_rollout_step_tb(const d2d_ppo_rollout* r, const float* prev_term_obs /* [n][27] */,
                                const float* const* weights, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* D2D_PPO_H */
