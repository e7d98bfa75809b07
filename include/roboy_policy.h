/* roboy_policy.h - C ABI of the fused MLP policy step for the PPO consumer.
 *
 * NOT part of the drop-in boundary of the simulation path (that is roboy_sim.h): the reference's consumer is
 * stable_baselines' PPO2("MlpPolicy", env) (/root/reference/gym_roboy/train_parallel.py:28-35), whose policy is two
 * tanh layers of 64 units for the action mean and two for the value, with a state-independent log-std
 * (gym_roboy_amd/ppo.py: MlpPolicy restates it on torch).  With the env step at ~12 us for 262 144 envs, the torch
 * forward pass + sampling of that policy (about 30 small kernels, 370 us) is what a rollout step costs; this
 * library evaluates  obs -> (action sample, log-probability, value)  in ONE kernel on the matrix cores
 * (v_mfma_f32_32x32x2_f32: exact f32, a k-ordered fmaf chain), gym_roboy_amd/csrc/mlp_policy.hip.
 *
 * Plain C, pointers and sizes only; device pointers are HIP device memory of the current device; `stream` is a
 * hipStream_t (0 = the default stream).  Every function returns 0 on success, a negative code otherwise
 * (rp_last_error() has the message).
 */
#ifndef ROBOY_POLICY_H
#define ROBOY_POLICY_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define RP_ABI_VERSION 5
#define RP_HIDDEN 64          /* units per hidden layer (stable_baselines' MlpPolicy) */
#define RP_MAX_OBS 95         /* obs_dim + 1 (bias column) <= 96 */
#define RP_MAX_ACT 64

enum { RP_OK = 0, RP_EINVAL = -1, RP_EHIP = -2, RP_EUNSUPPORTED = -3 };

/* parameters of one MlpPolicy in torch's layout: Linear.weight is [out][in] row-major, bias [out] */
typedef struct rp_mlp_params {
    const float *pi_w1, *pi_b1, *pi_w2, *pi_b2, *pi_w3, *pi_b3;   /* [64][obs], [64], [64][64], [64], [act][64], [act] */
    const float *vf_w1, *vf_b1, *vf_w2, *vf_b2, *vf_w3, *vf_b3;   /* [64][obs], [64], [64][64], [64], [1][64],   [1]   */
    const float *log_std;                                          /* [act] */
} rp_mlp_params;

int rp_abi_version(void);
const char *rp_last_error(void);

/* Number of floats of the packed parameter blob for these dimensions (the matrix-core operand order: each weight
 * sits where the lane that feeds it to the MFMA reads it), or a negative code if the dimensions are not supported. */
int64_t rp_packed_floats(int obs_dim, int act_dim);

/* Host: reorder the parameters (host pointers) into the packed blob (host, rp_packed_floats() floats).  The order
 * depends on the dimensions only, so a caller may pack an index-valued parameter set once and use the result as a
 * gather map on the device. */
int rp_pack(const rp_mlp_params *host_params, int obs_dim, int act_dim, float *packed_host);

/* One policy step for n observations (device pointers): obs [n][obs_dim] -> act [n][act_dim] = mean + std * eps,
 * logp [n] = log N(act; mean, std), value [n]; mean [n][act_dim] is written too unless NULL.  eps: standard normal
 * from Philox4x32-10 keyed (seed; sample index + sample_offset, step) by Box-Muller - the same draw whatever the
 * batch is sharded into; d_step_base (device, may be NULL): added to `step` when the kernel runs, so that a
 * captured launch (hipGraph replay) draws fresh noise on every replay; deterministic != 0: act = mean.
 * Asynchronous on `stream`. */
int rp_act_dev(const float *d_packed, const float *d_obs, float *d_act, float *d_logp, float *d_value, float *d_mean,
               int64_t n, int obs_dim, int act_dim, uint64_t seed, uint64_t sample_offset, uint32_t step,
               const uint32_t *d_step_base, int deterministic, void *stream);

/* ---- the PPO minibatch gradient (gym_roboy_amd/ppo.py: _minibatch_loss is the torch statement) ----
 * Loss = mean_i max(-A_i r_i, -A_i clip(r_i, 1 -+ c)) + vf_coef * mean_i 1/2 max((v_i - R_i)^2, (vclip_i - R_i)^2),
 * r_i = exp(logp(act_i | obs_i) - logp_old_i), vclip_i = v_old_i + clip(v_i - v_old_i, -+c); A_i is the caller's
 * (already normalised) advantage.  The entropy bonus of a state-independent log-std has the constant gradient
 * -ent_coef per log-std component and is left to the caller. */

/* Generalised advantage estimation over a rollout (device pointers, [n_steps][n_envs] row-major; done[t] = step t
 * ended an episode, as 0 / 1 floats; last_val [n_envs] = value of the observation after the last step):
 * delta_t = rew_t + gamma * V_{t+1} * (1 - done_t) - V_t,  adv_t = delta_t + gamma * lam * (1 - done_t) * adv_{t+1},
 * ret_t = adv_t + V_t.  One launch, one env per thread. */
int rp_gae_dev(const float *d_rew, const float *d_val, const float *d_done, const float *d_last_val, float gamma, float lam,
               float *d_adv, float *d_ret, int n_steps, int64_t n_envs, void *stream);

/* floats of the blob rp_pack_train() writes: the rp_pack() blob followed by the transposed weights; negative if the
 * gradient kernels do not support the dimensions: obs_dim <= 63, and the operands of the action net plus the per-wave
 * scratch must fit the 160 KB of LDS (60 -> 38 does, 63 -> 64 does not) */
int64_t rp_train_packed_floats(int obs_dim, int act_dim);
int rp_pack_train(const rp_mlp_params *host_params, int obs_dim, int act_dim, float *packed_host);

/* The gradient vector d_grad: two blocks of rp_grad_floats() / 2 floats, action net then value net, each in torch
 * layout  [w1 (64 x obs), b1 (64), w2 (64 x 64), b2 (64), w3 (out x 64), b3 (out), log_std (out; zero for the value
 * net), loss term, 3 spare]  padded to a multiple of 4 (out = act_dim / 1).  The action net's first two spare slots carry approx_kl
 * and clip_frac after rp_ppo_grad_diag_dev (below), and only after it. */
int64_t rp_grad_floats(int obs_dim, int act_dim);
int64_t rp_ppo_workspace_floats(int obs_dim, int act_dim, int64_t batch);

/* Device pointers.  d_index == NULL: obs [batch][obs_dim], act [batch][act_dim], adv / logp_old / val_old / ret
 * [batch].  d_index != NULL (int64 [batch]): sample i of the minibatch is ROW d_index[i] of obs, act, logp_old,
 * val_old, ret (the whole rollout's tensors - no gathered copies).  The advantage: with d_adv_stats == NULL, adv
 * [batch] is in minibatch order and already normalised by the caller; with d_adv_stats = the {mean, 1 / (std + 1e-8)}
 * pair rp_adv_stats_dev wrote, adv is the rollout's raw advantage, indexed like the rest and normalised per sample
 * in the kernel.  d_grad: rp_grad_floats() floats (overwritten), d_workspace: rp_ppo_workspace_floats() floats.
 * Four launches on `stream` (one per net, two reductions); asynchronous.  Like every rp_*_dev entry point it runs
 * on the device its first device pointer lives on (made current for the call). */
int rp_ppo_grad_dev(const float *d_packed_train, const float *d_obs, const float *d_act, const float *d_adv,
                    const float *d_adv_stats, const float *d_logp_old, const float *d_val_old, const float *d_ret,
                    const int64_t *d_index, int64_t batch, int obs_dim, int act_dim, float cliprange, float vf_coef,
                    float *d_grad, float *d_workspace, void *stream);

/* ---- the rest of a PPO update (gym_roboy_amd/ppo.py: update) ---- */
/* The sample order of an epoch: out[j] = P(first + j), j < count, for a bijection P of [0, n) keyed by `key` (a
 * four-round Feistel network on the next even power of two, cycle-walked into [0, n)): what torch.randperm(n) is to
 * the torch path, evaluated per element instead of sorting n keys.  _host: the same function on the CPU. */
int rp_perm_dev(uint64_t key, int64_t n, int64_t first, int64_t count, int64_t *d_out, void *stream);
int rp_perm_host(uint64_t key, int64_t n, int64_t first, int64_t count, int64_t *out);
/* d_stats2 = {mean, 1 / (std + 1e-8)} (std: the unbiased estimate, as torch.Tensor.std) of adv[d_index[i]], i < batch
 * (d_index == NULL: adv[i]).  d_scratch: rp_adv_stats_scratch_doubles() doubles, zeroed ONCE by the caller (the kernel
 * leaves it ready for the next call).  One launch; sums in fp64 in a fixed order. */
int64_t rp_adv_stats_scratch_doubles(void);
int rp_adv_stats_dev(const float *d_adv, const int64_t *d_index, int64_t batch, float *d_stats2, double *d_scratch, void *stream);
/* clip_grad_norm_(max_grad_norm) followed by Adam.step() as one launch: d_params, d_m, d_v are rp_grad_floats()
 * floats in the layout of the gradient vector d_grad (a policy whose parameters are views of d_params sees the
 * update in place); the gradient is first scaled by grad_scale (1 / world size after an all-reduce) and the entropy
 * bonus of the state-independent log-std (-ent_coef per component) is added; the loss slots are left alone.  step =
 * the number of this update, from 1 (bias corrections); eps enters as in torch.optim.Adam. */
int rp_clip_adam_dev(float *d_params, const float *d_grad, float *d_m, float *d_v, int obs_dim, int act_dim, float lr,
                     float beta1, float beta2, float eps, int64_t step, float max_grad_norm, float grad_scale, float ent_coef,
                     void *stream);
/* ---- running observation normalisation (gym_roboy_amd/ppo.py: ObsNorm) ----
 * State per observation column: mean, var and a shared count, float64 (d_state: double[2 * obs_dim + 1] = mean, var, count).
 * The form the kernels read is d_norm = float[2][obs_dim]: row 0 mean, row 1 rstd = 1 / sqrt(var + eps); while count == 0 it is
 * the identity (mean 0, rstd 1).  A column value enters the network as
 *     x' = min(max((x - mean) * rstd, -clip), clip)
 * with the difference and the product each rounded once to float32 (never contracted) and the clamp last, so that a numpy / torch
 * float32 restatement reproduces the operand bit for bit; the bias column stays the constant 1; the statistics carry no gradient.
 * The statistics take no LDS: every limit of the unnormalised entry points (rp_train_packed_floats, rp_grad_form) holds unchanged. */

/* rp_act_dev with the observation normalised as it is fetched (the layer-1 operands: the kernel's only read of it).  d_norm == NULL
 * launches rp_act_dev's kernel itself; clip > 0 (INFINITY: no clamp). */
int rp_act_norm_dev(const float *d_packed, const float *d_obs, float *d_act, float *d_logp, float *d_value, float *d_mean,
                    int64_t n, int obs_dim, int act_dim, uint64_t seed, uint64_t sample_offset, uint32_t step,
                    const uint32_t *d_step_base, int deterministic, const float *d_norm, float clip, void *stream);
/* rp_ppo_grad_dev on normalised observations, in all three forms rp_grad_form reports: the layer-1 forward operands AND the operands
 * of dW1 += delta1 [obs | 1]^T are x'.  d_norm == NULL launches rp_ppo_grad_dev's kernels themselves. */
int rp_ppo_grad_norm_dev(const float *d_packed_train, const float *d_obs, const float *d_act, const float *d_adv,
                         const float *d_adv_stats, const float *d_logp_old, const float *d_val_old, const float *d_ret,
                         const int64_t *d_index, int64_t batch, int obs_dim, int act_dim, float cliprange, float vf_coef,
                         const float *d_norm, float clip, float *d_grad, float *d_workspace, void *stream);
/* Shifted moments of obs [rows][obs_dim] (float32, contiguous): d_sums = double[1 + 2 * obs_dim] = {rows, sum_c (x - shift_c),
 * sum_c (x - shift_c)^2}; d_shift: double[obs_dim] or NULL (= 0).  The shift is the current running mean (d_state's first obs_dim
 * doubles), which is what rp_obs_norm_merge_dev assumes; sums of different ranks taken with the same shift add.  One launch, fp64
 * accumulation in a fixed order (bit-reproducible run to run), no floating-point atomics.  d_scratch:
 * rp_obs_moments_scratch_doubles() doubles, zeroed ONCE by the caller (the kernel leaves it ready for the next call).
 * rp_obs_moments_blocks(): the grid of that launch - a workgroup takes 256 / obs_dim rows per pass of its grid-stride loop. */
int64_t rp_obs_moments_scratch_doubles(void);
int64_t rp_obs_moments_blocks(int64_t rows, int obs_dim);
int rp_obs_moments_dev(const float *d_obs, int64_t rows, int obs_dim, const double *d_shift, double *d_sums, double *d_scratch,
                       void *stream);
/* Chan's parallel merge of d_sums (taken with shift = d_state's mean) into d_state = {mean, var (population), count}, and the float
 * form d_norm = {mean, 1 / sqrt(var + eps)}.  rows == 0 (d_sums[0]) leaves everything unchanged.  One small launch. */
int rp_obs_norm_merge_dev(double *d_state, const double *d_sums, int obs_dim, double eps, float *d_norm, void *stream);
/* ---- running return normalisation of the reward (gym_roboy_amd/ppo.py: RewardNorm) ----
 * The tail of a rollout as ONE launch: reward scaling, the discounted-return scan with its moments, the done conversion and GAE.
 * Device pointers, [n_steps][n_envs] row-major.  Per env, forwards in time from R = d_ret_carry[i] (double, read and written back):
 *     r_s = fl32(rew_raw_t * reward_scale);  R = gamma * R + r_s (float64);  d = R - shift joins S += d, SS += d * d;
 *     then R = 0 where done_i_t != 0
 * and backwards rp_gae_dev's recurrence (gamma, lam rounded to float32) over
 *     r~_t = min(max(fl32(r_s * rstd), -clip), clip)
 * - both products rounded once to float32, the clamp last, the mean NOT subtracted - writing d_rew = r~, d_done = done_i as 0 / 1
 * floats, d_adv, d_ret.  d_norm2: float[2] = {mean, rstd} of the discounted return, NULL = the identity (rstd 1); clip > 0
 * (INFINITY: no clamp); d_shift: one double, the statistics' running mean, NULL = 0; d_sums3 = double[3] = {n_steps * n_envs, S, SS},
 * the layout rp_obs_norm_merge_dev merges with obs_dim = 1.  fp64 sums in one fixed order (bit-reproducible run to run), no
 * floating-point atomics.  d_scratch: rp_rollout_tail_scratch_doubles() doubles, zeroed ONCE by the caller (the kernel leaves it
 * ready for the next call).  rp_rollout_tail_blocks(): the grid of that launch - one env per lane, 256 per workgroup, at most
 * 4 096 workgroups striding over the envs (n_envs < 2^26).  Null pointers, n_steps < 1, n_envs < 1, clip not > 0, gamma outside
 * [0, 1]: RP_EINVAL. */
int64_t rp_rollout_tail_scratch_doubles(void);
int64_t rp_rollout_tail_blocks(int n_steps, int64_t n_envs);
int rp_rollout_tail_dev(const float *d_rew_raw, const int32_t *d_done_i, const float *d_val, const float *d_last_val, float reward_scale,
                        const float *d_norm2, float clip, const double *d_shift, double gamma, double lam, double *d_ret_carry,
                        float *d_rew, float *d_done, float *d_adv, float *d_ret, double *d_sums3, double *d_scratch, int n_steps,
                        int64_t n_envs, void *stream);
/* ---- the same tail with value bootstrapping of truncated episodes (ABI 5; PPO(bootstrap_timeouts=True)) ----
 * rp_rollout_tail_dev's argument list and launch; d_done_i carries episode-end codes (roboy_sim.h: RB_DONE_*): 0 none, 1 terminated
 * (the goal was reached), 2 truncated (the time limit ended the episode).  Any non-zero code ends the episode exactly as above: the
 * return scan's reset, GAE's mask, d_done written as 0 / 1 floats.  Where the code is 2 the backward recurrence takes
 *     r^_t = fl32(r~_t + fl32(gamma32 * val_t))
 * in place of r~_t - two roundings, no contraction - and is otherwise rp_rollout_tail_dev's: the return the critic is trained on
 * no longer collapses at a moment the observation does not show.  val_t is the value of the last observation before the limit
 * (the terminal observation itself is overwritten by the auto-reset row: the rl_games / Isaac Gym form).  d_rew still receives r~
 * without the bootstrap, and the return scan with its fp64 moments does not see it.  With no code 2 anywhere every output is
 * bit-equal to rp_rollout_tail_dev's.  A second instance of the same kernel text: rp_rollout_tail_dev's instruction stream is
 * unchanged.  Same scratch, same grid, same argument errors. */
int rp_rollout_tail_boot_dev(const float *d_rew_raw, const int32_t *d_done_i, const float *d_val, const float *d_last_val, float reward_scale,
                             const float *d_norm2, float clip, const double *d_shift, double gamma, double lam, double *d_ret_carry,
                             float *d_rew, float *d_done, float *d_adv, float *d_ret, double *d_sums3, double *d_scratch, int n_steps,
                             int64_t n_envs, void *stream);
/* ---- update diagnostics and the KL-adaptive learning rate (PPO(diagnostics=True / lr_schedule="adaptive")) ----
 * For a minibatch of B samples with x_i = logp(act_i | obs_i) - logp_old_i, ratio_i = exp(x_i) and cliprange c:
 *     approx_kl = (1 / B) sum_i 0.5 x_i^2                     (stable-baselines PPO2's `approxkl`)
 *     clip_frac = (1 / B) #{i: ratio_i < 1 - c or ratio_i > 1 + c}   (a sample counts when the kernel's own clamp changed its ratio)
 * rp_ppo_grad_diag_dev is rp_ppo_grad_norm_dev - the same argument list, d_norm == NULL selecting the unnormalised kernels, the same
 * four launches, workspace, limits and errors - whose action-net launch is a diagnostics instance of the same kernel text: it
 * additionally leaves approx_kl at d_grad[L + 1] and clip_frac at d_grad[L + 2], L = the action net's loss slot (the first two of
 * its three spare slots).  approx_kl is a per-lane fp32 sum under the same guard and 1 / B factor as the loss term; clip_frac is
 * counted per wave (an integer) and scaled by 1 / B once per wave; both then take the loss term's road - one partial per wave, folded
 * per workgroup in wave order, summed by the reduction launch - so they are bit-reproducible from call to call.  The gradient and
 * the two loss terms are what rp_ppo_grad_norm_dev computes.  The value net's block is untouched.  The spare slots are DEFINED ONLY
 * after this entry point: rp_ppo_grad_dev / rp_ppo_grad_norm_dev leave whatever their partial sums held there, and nothing reads it. */
int rp_ppo_grad_diag_dev(const float *d_packed_train, const float *d_obs, const float *d_act, const float *d_adv,
                         const float *d_adv_stats, const float *d_logp_old, const float *d_val_old, const float *d_ret,
                         const int64_t *d_index, int64_t batch, int obs_dim, int act_dim, float cliprange, float vf_coef,
                         const float *d_norm, float clip, float *d_grad, float *d_workspace, void *stream);
/* rp_clip_adam_dev with the learning rate on the device (d_lr: one float, read and rewritten) and rsl_rl's "adaptive" schedule in front
 * of the step of the same minibatch, in fp32, every thread computing it redundantly:
 *     kl = d_grad[L + 1] * grad_scale                          (after an all-reduce: the mean over the ranks)
 *     if      kl > 2 desired_kl               lr = max(lr_min, lr / lr_factor)      (IEEE division, one rounding)
 *     else if kl < desired_kl / 2 and kl > 0  lr = min(lr_max, lr * lr_factor)
 *     else                                    lr unchanged     (every comparison is false on a NaN)
 * Adam then steps with the new lr, which one thread stores to d_lr[0] once every thread has read the old one; clip_grad_norm_ and
 * the moments are exactly rp_clip_adam_dev's, and like it the kernel reads no other non-parameter slot and writes none.  One launch,
 * no host read-back.  RP_EINVAL: null pointers, desired_kl not > 0, lr_factor not > 1, lr_min not > 0, lr_min > lr_max, step < 1. */
int rp_clip_adam_kl_dev(float *d_params, const float *d_grad, float *d_m, float *d_v, int obs_dim, int act_dim, float *d_lr,
                        float desired_kl, float lr_factor, float lr_min, float lr_max, float beta1, float beta2, float eps, int64_t step,
                        float max_grad_norm, float grad_scale, float ent_coef, void *stream);
/* ---- an asymmetric critic: the value net on privileged rows of its own (PPO(asymmetric_critic=True)) ----
 * The action net reads obs [n][obs_dim] through a blob packed for (obs_dim, act_dim); the value net reads cobs [n][cobs_dim] (the
 * env's critic rows: roboy_sim.h, rb_env_critic_obs_*) through a blob packed for (cobs_dim, act_dim).  A blob holds both nets'
 * operands; each net is read from its own blob only, so the value weights of the first blob and the action weights of the second are
 * never used (a caller may pack the same rp_mlp_params twice with the first-layer matrix of the net that does not apply left at any
 * width-correct filler).  RP_ABI_VERSION is still 5: nothing that existed changed.
 *
 * rp_act_asym_dev / rp_act_asym_norm_dev: the policy step.  Two further instances of the policy-step kernel's text with ONE NET PER
 * WORKGROUP - a workgroup stages only its net's operands in LDS, half of the symmetric step's - otherwise rp_act_dev's work items,
 * network arithmetic and epilogue: actions, log-probabilities, means and the Philox keys are those of rp_act_dev(obs) for the same
 * (seed, sample_offset, step), and the values those of rp_act_dev(cobs) on a policy of input width cobs_dim with the same value
 * weights.  The norm form takes statistics and a clip per net (both or neither: both NULL launches the plain instance). */
int rp_act_asym_dev(const float *d_packed_pi, const float *d_packed_vf, const float *d_obs, const float *d_cobs, float *d_act, float *d_logp,
                    float *d_value, float *d_mean, int64_t n, int obs_dim, int cobs_dim, int act_dim, uint64_t seed, uint64_t sample_offset,
                    uint32_t step, const uint32_t *d_step_base, int deterministic, void *stream);
int rp_act_asym_norm_dev(const float *d_packed_pi, const float *d_packed_vf, const float *d_obs, const float *d_cobs, float *d_act, float *d_logp,
                         float *d_value, float *d_mean, int64_t n, int obs_dim, int cobs_dim, int act_dim, uint64_t seed,
                         uint64_t sample_offset, uint32_t step, const uint32_t *d_step_base, int deterministic, const float *d_norm_pi,
                         const float *d_norm_vf, float clip_pi, float clip_vf, void *stream);
/* The gradient: NO new kernel.  The existing instances are launched with per-net arguments - the action net with (d_packed_pi, d_obs,
 * obs_dim, d_norm_pi, clip_pi), the value net with (d_packed_vf, d_cobs, cobs_dim, d_norm_vf, clip_vf) - and each net's form
 * (rp_grad_form) is chosen from its own width.  d_packed_*: rp_pack_train blobs.  The gradient vector: the action net's block of
 * rp_grad_floats(obs_dim, act_dim) / 2 floats, then the value net's of rp_grad_floats(cobs_dim, act_dim) / 2, each in the layout
 * above (w1 is 64 x obs_dim / 64 x cobs_dim): rp_grad_asym_floats() in all.  Each block is bit-equal to the same block of
 * rp_ppo_grad_norm_dev / rp_ppo_grad_diag_dev on a symmetric policy of that width and those weights.  Statistics for both nets or for
 * neither; diag != 0: the action net's launch is its diagnostics instance (rp_ppo_grad_diag_dev).  d_workspace:
 * rp_ppo_asym_workspace_floats() floats.  Every other argument, limit and error is rp_ppo_grad_dev's. */
int64_t rp_grad_asym_floats(int obs_dim, int cobs_dim, int act_dim);
int64_t rp_ppo_asym_workspace_floats(int obs_dim, int cobs_dim, int act_dim, int64_t batch);
int rp_ppo_grad_asym_dev(const float *d_packed_pi, const float *d_packed_vf, const float *d_obs, const float *d_cobs, const float *d_act,
                         const float *d_adv, const float *d_adv_stats, const float *d_logp_old, const float *d_val_old, const float *d_ret,
                         const int64_t *d_index, int64_t batch, int obs_dim, int cobs_dim, int act_dim, float cliprange, float vf_coef,
                         const float *d_norm_pi, const float *d_norm_vf, float clip_pi, float clip_vf, int diag, float *d_grad,
                         float *d_workspace, void *stream);
/* The optimiser: NO new kernel.  rp_clip_adam_dev / rp_clip_adam_kl_dev over a vector of rp_grad_asym_floats() floats in the layout
 * of rp_ppo_grad_asym_dev's gradient; every other argument, rule and error is theirs. */
int rp_clip_adam_asym_dev(float *d_params, const float *d_grad, float *d_m, float *d_v, int obs_dim, int cobs_dim, int act_dim, float lr,
                          float beta1, float beta2, float eps, int64_t step, float max_grad_norm, float grad_scale, float ent_coef,
                          void *stream);
int rp_clip_adam_kl_asym_dev(float *d_params, const float *d_grad, float *d_m, float *d_v, int obs_dim, int cobs_dim, int act_dim, float *d_lr,
                             float desired_kl, float lr_factor, float lr_min, float lr_max, float beta1, float beta2, float eps, int64_t step,
                             float max_grad_norm, float grad_scale, float ent_coef, void *stream);
/* ---- mirror-symmetry augmentation (gym_roboy_amd/ppo.py: PPO(symmetry="augment")) ----
 * A robot with a mirror plane gives every transition (s, a, r, s') a twin (M s, P a, r, M s') that costs no simulation: M flips the
 * sign of some observation columns and swaps others with their partner's, P permutes the action's tendons.  The update then runs on
 * the rollout's n samples AND their images, 2 n rows, through the unchanged gradient, statistics, sample-order and optimiser entry
 * points above.  This is the one new launch: it materialises the second half.
 *     d_mirror[r][c] = d_col_sign[c] * d_src[r][d_col_src[c]]      one IEEE multiply: a flipped 0 is -0
 *     d_plain [r][c] = d_src[r][c]                                 where d_plain is given
 * for rows x width floats; d_col_src (int32, entries in [0, width)) and d_col_sign are device arrays of `width` entries.  d_plain:
 * NULL - not written; == d_src - allowed, and then skipped; otherwise a copy.  1 <= width <= 128.  The arrays of rows x width floats
 * must not overlap - d_mirror with d_src, d_plain with d_mirror, d_plain with d_src unless it IS d_src: any overlap, partial ones
 * included, is refused with RP_EINVAL (the address ranges are compared).
 * No output needs more than the 4-byte alignment of a float: the halves of one [2 n, width] allocation are served as they lie
 * (n = 321, width = 9: the second half starts 4-byte aligned), with 16-byte accesses wherever the run in question allows them.
 * One entry point serves the observation rows (the env's map), the action rows (the tendon permutation) and - width 1, the identity
 * map, sign +1 - the per-sample scalars.  rows == 0: nothing is launched.  Added by name: the ABI version stays 5. */
int rp_mirror_rows_dev(const float *d_src, float *d_plain /* NULL: not written */, float *d_mirror, int64_t rows, int width,
                       const int32_t *d_col_src, const float *d_col_sign, void *stream);
/* ---- the mirror-symmetry loss on the action mean (gym_roboy_amd/ppo.py: PPO(symmetry="loss")) ----
 * For a minibatch of B rows s_i, A = act_dim, M / P the env's observation / action mirror maps:
 *     e_i[j] = mu(M s_i)[j] - mu(s_i)[P j]        L_sym = coef / (B A) sum_i sum_j e_i[j]^2
 * mu is the action net's mean; the gradient flows through BOTH branches; log_std and the value net get none (the log_std entries of
 * the block are exact zeros).  It touches the action net and the actor's rows only: no critic-row map is needed.
 * One launch of a further instance family of the gradient kernel's text (mlp_sym_kernel / mlp_sym_norm_kernel) + a reduction.  A
 * wave tile is 32 PAIRS: column tile 0 reads row d_index[p] (or p) of d_obs, column tile 1 the same row of d_obs_image (the rows
 * M s, e.g. from rp_mirror_rows_dev); after the forward pass lane l holds mu(s_l) and lane l ^ 32 holds mu(M s_l), and with
 * c' = 2 coef / (B A) the loss derivative of both branches is the one expression d3[j] = c' (out[j] - partner[P j]) - no second
 * forward pass, no target buffer, no stop-gradient.  Everything behind d3 is the PPO kernel's text on the matrix cores in exact f32.
 *   d_packed_train: the action net's rp_pack_train blob (the asymmetric layout: d_packed_pi).
 *   act_src: HOST array of act_dim int32, P as envs.symmetry's act_src; it must be an involution of [0, act_dim) (fixed points are
 *     legal; act_dim = 1 with {0} works), otherwise RP_EINVAL.  It travels in the kernel arguments.
 *   coef: finite and >= 0.  coef = 0 gives an all-zero block.
 *   d_grad_pi: the action net's block of rp_ppo_grad_dev's / rp_ppo_grad_asym_dev's gradient vector (rp_grad_floats() / 2 floats; the
 *     action block comes first in both layouts, so the vector itself may be handed in).  Written: the parameter entries [0, L) and
 *     L_sym at d_grad_pi[L + 3], L = the action net's loss slot - its third spare slot, a slot of L_sym's own.  d_grad_pi[L], [L + 1],
 *     [L + 2] (the surrogate loss, approx_kl, clip_frac) are neither read nor written.  rp_ppo_grad_*_dev leave 0 at [L + 3].
 *   accumulate: 0 overwrites those entries, 1 adds to what is there: the sum over the partials is formed first and added LAST, so
 *     accumulate = 1 onto g0 is exactly g0 + (the accumulate = 0 result), element by element.  Behind rp_ppo_grad_*_dev on the same
 *     stream this puts L_sym's gradient into the PPO gradient in front of clip + Adam with no add launch.
 *   d_workspace: rp_sym_workspace_floats() floats.  Sums in a fixed order: bit-reproducible, and the same minibatch addressed through
 *     d_index into longer tensors gives the same bits.
 * rp_sym_grad_norm_dev: both branches' observation operands normalised (d_norm, clip as rp_ppo_grad_norm_dev; d_norm == NULL launches
 * rp_sym_grad_dev's kernels).  Limits: rp_train_packed_floats()'s (obs_dim <= 63, up to 64 actions, the same LDS budget rule).
 * rp_sym_grad_form: 2 = the small instance (obs_dim <= 31, up to 8 actions) with its rows prefetched by LDS-DMA - every small policy:
 * the two input buffers hold obs_dim + 2 rows each and always fit - 1 = the small instance staging its rows at the start of each tile
 * (ROBOY_POLICY_PREFETCH=0 only), 0 = the general instance; < 0: unsupported.  Added by name: the ABI version stays 5. */
int rp_sym_grad_dev(const float *d_packed_train, const float *d_obs, const float *d_obs_image, const int64_t *d_index /* or NULL */,
                    int64_t batch, int obs_dim, int act_dim, const int32_t *act_src /* host, [act_dim] */, float coef,
                    float *d_grad_pi, int accumulate /* 0: overwrite, 1: add to what is there */, float *d_workspace, void *stream);
int rp_sym_grad_norm_dev(const float *d_packed_train, const float *d_obs, const float *d_obs_image, const int64_t *d_index, int64_t batch,
                         int obs_dim, int act_dim, const int32_t *act_src, float coef, const float *d_norm, float clip, float *d_grad_pi,
                         int accumulate, float *d_workspace, void *stream);
int64_t rp_sym_workspace_floats(int obs_dim, int act_dim, int64_t batch);
int rp_sym_grad_form(int obs_dim, int act_dim);
/* test hook: would a grant of lds_bytes of dynamic LDS be issued for (kernel id, device) now?  Records it. */
int rp_debug_lds_grant_needed(int kernel_id, int dev, int64_t lds_bytes);
/* which form of the gradient kernels rp_ppo_grad_dev launches for this policy: 2 = the small instance (obs_dim <= 31, up to 8
 * actions) with its inputs prefetched by LDS-DMA, 1 = the small instance loading at the start of each tile (the two input
 * buffers per wave do not fit beside the operands, or ROBOY_POLICY_PREFETCH=0), 0 = the general instance; < 0: unsupported */
int rp_grad_form(int obs_dim, int act_dim);

#ifdef __cplusplus
}
#endif
#endif
