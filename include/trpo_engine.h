/*
 * trpo_engine.h — C-ABI of the MI355X-native TRPO policy-update engine.
 *
 * The reference (inksci/TRPO) runs its update through a TF-1.3 session and
 * numpy; every entry point below replaces one reference interface, cited as
 * file:line into the reference tree.  Conventions:
 *
 *   - return 0 on success, a negative code on failure; trpo_last_error()
 *     returns the message of the calling thread's last failure;
 *   - `mem` selects where a caller pointer lives: TRPO_MEM_HOST or
 *     TRPO_MEM_DEVICE (a device pointer on the engine's GPU, e.g. a torch-ROCm
 *     tensor's data_ptr()).  Inputs are copied; caller buffers are never
 *     retained (reference: caller-owned numpy in, fresh numpy out);
 *   - one engine is driven from one host thread; calls are ordered on the
 *     engine's HIP stream and synchronise only when they return host data;
 *   - flat parameter vectors use the reference's layout
 *     [W1, b1, W2, b2, ..., WL, bL], W_l row-major [fan_in][fan_out]
 *     (tf.trainable_variables() order, trpo_inksci.py:49; var_shape/numel,
 *     utils.py:108-116).
 *
 * All arithmetic that the reference does in float32 is float32 here; the
 * scalars its NumPy-1.x promotion keeps in float64 (shs, lm, the
 * expected-improve rate, the line-search ratio) are float64.
 */
#ifndef TRPO_ENGINE_H
#define TRPO_ENGINE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TRPO_MEM_HOST 0
#define TRPO_MEM_DEVICE 1

#define TRPO_OK 0
#define TRPO_ERR_ARG (-1)
#define TRPO_ERR_HIP (-2)
#define TRPO_ERR_RCCL (-3)
#define TRPO_ERR_STATE (-4)

typedef struct trpo_engine trpo_engine;

/* Hyper-parameters of one update; defaults are config/eps of trpo_inksci.py:16-17
 * and the CG/line-search defaults of utils.py:171-172,185. */
typedef struct trpo_update_params {
  int cg_iters;            /* 10          utils.py:185 */
  float residual_tol;      /* 1e-10       utils.py:185 (absolute, on r.r) */
  float cg_damping;        /* 0.1         trpo_inksci.py:17,126 */
  double max_kl;           /* 0.01        trpo_inksci.py:17,149,157 */
  int compute_advantages;  /* 1: discount + standardise the rewards given to trpo_set_rewards first */
  double gamma;            /* 0.95        trpo_inksci.py:17,104 */
} trpo_update_params;

typedef struct trpo_update_stats {
  int cg_iters;            /* CG iterations run (early exit on r.r < residual_tol) */
  int k;                   /* accepted backtrack index (step fraction 0.5^k), -1 if none */
  int reverted;            /* 1 if kl > 2 max_kl restored theta_prev (trpo_inksci.py:157-158) */
  int pad;
  double shs, lm, rate;    /* trpo_inksci.py:148-153 */
  float surr_before, kl_before, ent_before;   /* losses at theta_prev */
  float surr_after, kl_after, ent_after;      /* losses at the line-search result (:156) */
  float rdotr;             /* final CG residual r.r */
  float gdotstepdir;       /* g . stepdir */
} trpo_update_stats;

/* Vectors of the last update, for trpo_get_vector(). */
#define TRPO_VEC_THETA 0       /* current parameters (GetFlat) */
#define TRPO_VEC_THETA_PREV 1  /* thprev, trpo_inksci.py:144 */
#define TRPO_VEC_G 2           /* policy gradient, :146 */
#define TRPO_VEC_STEPDIR 3     /* CG solution, :147 */
#define TRPO_VEC_FULLSTEP 4    /* :150 */
#define TRPO_VEC_THETA_LS 5    /* linesearch result before the revert check, :153 */

/* ---- lifecycle --------------------------------------------------------- */

/* Build an engine for the categorical tanh-MLP policy of trpo_inksci.py:38-40
 * (hidden widths as a list; the reference is the depth-1 case {64}) with room
 * for `max_rows` states on GPU `device`.  n_actions <= 128 for the update (trpo_act: <= 64; the reference's softmax_classifier has
 * no bound; a softmax row spans up to 4 x 32 lanes here). */
int trpo_create(trpo_engine** out, int obs_dim, const int* hidden, int n_hidden, int n_actions,
                int64_t max_rows, int device);

/* ---- the policy's distribution family -----------------------------------------------------
 * TRPO_DIST_CATEGORICAL is the reference's softmax policy (trpo_create).  TRPO_DIST_GAUSSIAN is the
 * diagonal-Gaussian policy of continuous control, which the reference does not have: the equations
 * below are its definition.
 *
 * Policy.  The same tanh-MLP; its last layer is linear and gives the mean mu(s) in R^A.  The parameters
 * gain a state-independent log-std vector s in R^A, sigma = exp(s), stored last in the flat layout:
 * [W1, b1, ..., WL, bL, logstd], so P = sum(fan_in*fan_out + fan_out) + A, and every P-long vector
 * (theta, g, v, Hv, stepdir, fullstep) carries that tail.
 *
 * Feed.  states [n][obs] f32, actions [n][A] f32, advant [n] f32, old_mean [n][A] f32 (mu0) and
 * old_logstd [A] f32 (s0).  With z = (a - mu)/sigma and z0 = (a - mu0)/sigma0 per dimension d and
 * N = n_global:
 *   log r_n = sum_d [(s0_d - s_d) + (z0_d^2 - z_d^2)/2]
 *   surr    = -(1/N) sum_n adv_n exp(log r_n)
 *   kl      = (1/N) sum_n sum_d [s_d - s0_d + (sigma0_d^2 + (mu0_nd - mu_nd)^2)/(2 sigma_d^2) - 1/2]   (KL(old || new))
 *   ent     = (1/N) sum_n sum_d [s_d + ln(2 pi e)/2]
 * The mean is float32; the per-row log-ratio, KL and entropy terms are formed from it in float64 (the KL and
 * the log-ratio are differences of near-equal terms) and summed over rows in float64.
 *
 * Policy gradient.  g = grad_theta surr: the head delta DS_L[n,d] = -(adv_n r_n / N) z_nd / sigma_d followed by
 * the usual backprop, and on the tail g_s[d] = -(1/N) sum_n adv_n r_n (z_nd^2 - 1).
 *
 * FVP.  Hv is the Hessian-vector product of KL_ff(theta) = kl with (mu0, s0) := stop_grad(mu(theta), s) at the
 * same theta (the construction of trpo_inksci.py:56-70).  In closed form: the R-forward R{mu} = J_mu v;
 * RD_L = R{mu} / (sigma^2 N); backprop of RD_L like a policy gradient (at theta = theta_old the plain KL
 * backward is exactly zero, so no other term survives); Hv_s = 2 v_s (n/N) on the tail, each rank's partial,
 * which sums to 2 v_s over ranks.
 *
 * Sampling.  a = mu + sigma xi with xi [n][A] f64 standard normals given by the caller, evaluated in float64
 * and rounded to float32; train = 0 gives a = mu.
 *
 * On a Gaussian engine trpo_losses, trpo_eval_losses, trpo_policy_grad, trpo_fvp, trpo_cg, trpo_linesearch,
 * trpo_update, trpo_get/set_flat, trpo_get_vector, trpo_set_rewards, trpo_compute_advantages, the
 * estimator, tail-value and baseline calls, trpo_explained_variance, trpo_get_feed_view (whose old_dist
 * then points at old_mean and n_actions is act_dim), the comm calls and profiling work unchanged.  The
 * categorical-only calls (trpo_set_batch, trpo_action_dist, trpo_act, trpo_rollout_env, trpo_rollout_cartpole,
 * trpo_rollout_fetch*, and trpo_rollout_to_batch) on a Gaussian engine, and the Gaussian calls
 * (trpo_set_batch_gaussian, trpo_action_mean, trpo_act_gaussian and the four trpo_rollout_gaussian* calls) on a
 * categorical engine, return TRPO_ERR_STATE with a message that names the engine's distribution; nothing is
 * launched.  A Gaussian engine rolls out the continuous-action environments (trpo_rollout_gaussian, below). */
#define TRPO_DIST_CATEGORICAL 0
#define TRPO_DIST_GAUSSIAN 1
/* trpo_create for either family; act_dim <= 128 (trpo_act_gaussian: <= 64) */
int trpo_create_dist(trpo_engine** out, int dist, int obs_dim, const int* hidden, int n_hidden, int act_dim,
                     int64_t max_rows, int device);
int trpo_get_dist(trpo_engine* e, int* dist);
void trpo_destroy(trpo_engine* e);
const char* trpo_last_error(void);
int64_t trpo_num_params(const trpo_engine* e);
int trpo_synchronize(trpo_engine* e);
/* the engine's HIP stream (hipStream_t) as an opaque pointer */
void* trpo_stream(trpo_engine* e);

/* ---- multi-GPU (one process per GPU, RCCL over xGMI) ---------------------
 * The reference is single-process (trpo_inksci.py:23).  Rank 0 creates an id,
 * the launcher broadcasts it, every rank calls trpo_comm_init.  After that the
 * FVP / gradient / loss sums of each rank's shard are all-reduced. */
int trpo_comm_unique_id(uint8_t out_id[128]);
int trpo_comm_init(trpo_engine* e, const uint8_t id[128], int rank, int world);
/* Test transport: instead of RCCL, every all-reduce is stream-ordered and capturable: an async copy of
 * the buffer into a pinned host slot, a hipLaunchHostFunc callback that calls cb(host_buf, count,
 * dtype = TRPO_F32 / TRPO_F64, ctx), which must sum it across ranks in place (e.g. torch.distributed
 * over gloo), and an async copy back.  Lets several ranks share one GPU in tests. */
typedef int (*trpo_allreduce_cb)(void* host_buf, int64_t count, int dtype, void* ctx);
int trpo_comm_set_host_allreduce(trpo_engine* e, trpo_allreduce_cb cb, void* ctx, int rank, int world);
/* What carries this engine's all-reduces, for a launcher to verify (e.g. that N ranks of an RCCL
 * communicator sit on N distinct devices).  transport: 0 none (one process), 1 RCCL, 2 host callback.
 * comm_count / comm_rank / comm_device: ncclCommCount / ncclCommUserRank / ncclCommCuDevice of the RCCL
 * communicator (-1 without one); device: the engine's HIP device; pci_bus_id: hipDeviceGetPCIBusId. */
typedef struct trpo_comm_info_t {
  int transport;
  int rank, world;
  int comm_count, comm_rank, comm_device;
  int device;
  char pci_bus_id[64];
} trpo_comm_info_t;
int trpo_comm_info(trpo_engine* e, trpo_comm_info_t* out);

/* ---- parameters: SetFromFlat / GetFlat (utils.py:125-158) ---------------- */
int trpo_set_flat(trpo_engine* e, const float* theta, int mem);
int trpo_get_flat(trpo_engine* e, float* theta_out, int mem);
int trpo_get_vector(trpo_engine* e, int which, float* out, int mem);

/* ---- the feed (trpo_inksci.py:119-122) ------------------------------------
 * states [n][obs_dim] f32, actions [n] int64 in [0, n_actions), advant [n] f32
 * (may be NULL when trpo_set_rewards + compute_advantages provide it),
 * old_dist [n][n_actions] f32.  n_global = rows over all ranks (the 1/N of
 * reduce_mean, trpo_inksci.py:48-51,56). */
int trpo_set_batch(trpo_engine* e, int64_t n, int64_t n_global, const float* states,
                   const int64_t* actions, const float* advant, const float* old_dist, int mem);
/* the Gaussian engine's feed (TRPO_DIST_GAUSSIAN above): states [n][obs_dim], actions [n][act_dim], advant [n]
 * (may be NULL, as above), old_mean [n][act_dim], old_logstd [act_dim], all f32 */
int trpo_set_batch_gaussian(trpo_engine* e, int64_t n, int64_t n_global, const float* states, const float* actions,
                            const float* advant, const float* old_mean, const float* old_logstd, int mem);
/* rewards [n] f64, episode_starts [n] u8 (1 = first step of a path), baseline [n] f64 or NULL.
 * The paths of trpo_inksci.py:102-112, concatenated; this rank's shard must begin at a path start. */
int trpo_set_rewards(trpo_engine* e, const double* rewards, const uint8_t* episode_starts,
                     const double* baseline, int mem);
/* returns = discount(rewards, gamma) per path; advant = returns - baseline,
 * standardised (trpo_inksci.py:102-117).  Optional host copies (f64). */
int trpo_compute_advantages(trpo_engine* e, double gamma, double* returns_out, double* advant_out,
                            int mem);

/* adv = (adv - adv.mean()) / (adv.std() + 1e-8) in place, float64, population std
 * (trpo_inksci.py:115-117; SURVEY.md §8(b) `standardize(adv, n)`).  adv32_out (may be NULL) receives
 * float32(adv), what the advant placeholder is fed (:121).  With an engine the two sums run over all
 * ranks of its communicator (n = this rank's rows, n_global = all ranks') on its stream; e = NULL
 * runs on the current device for one process (n_global must equal n). */
int trpo_standardize(trpo_engine* e, double* adv, int64_t n, int64_t n_global, float* adv32_out, int mem);

/* ---- advantage estimator ---------------------------------------------------
 * What trpo_compute_advantages (and trpo_update with compute_advantages = 1) standardises.
 * TRPO_ADV_RETURNS, the default, is the reference's returns - baseline (trpo_inksci.py:102-105).
 * TRPO_ADV_GAE is generalised advantage estimation, which the reference does not have; per path, float64,
 * with end_t true on a path's last row, v = the baseline (0 when the feed has none):
 *   vnext_t = end_t ? (tail_values ? tail_values[t] : 0) : v_{t+1}
 *   delta_t = (r_t + gamma vnext_t) - v_t
 *   A_t     = end_t ? delta_t : delta_t + gamma lambda A_{t+1}
 *   R_t     = end_t ? r_t + gamma vnext_t : r_t + gamma R_{t+1}
 * R stays the feed's returns (the VF's target, explained variance); A replaces returns - baseline. */
#define TRPO_ADV_RETURNS 0
#define TRPO_ADV_GAE 1
/* kind = TRPO_ADV_RETURNS (lambda ignored) or TRPO_ADV_GAE with 0 <= lambda <= 1; engine state, kept
 * across feeds.  kind and lambda are checked first, before the engine is touched. */
int trpo_set_advantage_estimator(trpo_engine* e, int kind, double lambda);
/* the estimator in force; either output may be NULL */
int trpo_get_advantage_estimator(trpo_engine* e, int* kind, double* lambda);
/* tail_values [n] f64 of the current feed: V(s_T) of paths that were cut off rather than terminated, read
 * only at path-end rows; NULL clears them.  trpo_set_batch, trpo_set_rewards and trpo_rollout_to_batch
 * clear them too.  Only TRPO_ADV_GAE uses them: computing advantages under TRPO_ADV_RETURNS while they
 * are set fails with TRPO_ERR_STATE.  Called with the engine's own buffer (trpo_get_tail_view's tail,
 * TRPO_MEM_DEVICE) it marks the values written there as set, without a copy. */
int trpo_set_tail_values(trpo_engine* e, const double* tail_values, int mem);
/* the feed's tail values [n] f64 as the scan will read them: zeros when none are set */
int trpo_get_tail_values(trpo_engine* e, double* out, int mem);

/* ---- the graph outputs ---------------------------------------------------- */
/* session.run(self.losses) -> [surr, kl, ent] at the current parameters (trpo_inksci.py:53,156) */
int trpo_losses(trpo_engine* e, float out3[3]);
/* loss(th): SetFromFlat(th) then session.run(surr) (trpo_inksci.py:127-129); out3 = [surr, kl, ent] */
int trpo_eval_losses(trpo_engine* e, const float* theta, float out3[3], int mem);
/* session.run(self.action_dist) -> [n][n_actions] f32 at the current parameters
 * (trpo_inksci.py:38-40,78; the policy forward) */
int trpo_action_dist(trpo_engine* e, float* out, int mem);
/* the Gaussian policy forward at the current parameters over the feed: mean_out [n][act_dim] f32 and
 * logstd_out [act_dim] f32 (either may be NULL) */
int trpo_action_mean(trpo_engine* e, float* mean_out, float* logstd_out, int mem);
/* session.run(self.pg) = flatgrad(surr, var_list) (trpo_inksci.py:54,146) */
int trpo_policy_grad(trpo_engine* e, float* g_out, int mem);
/* fisher_vector_product(p) = session.run(self.fvp) + cg_damping * p (trpo_inksci.py:56-70,124-126) */
int trpo_fvp(trpo_engine* e, const float* v, float* out, float damping, int mem);

/* ---- Fisher-vector products on a subsample of the batch ----------------------------------
 * The estimator of Schulman's modular_rl and OpenAI baselines' trpo_mpi (fvpargs = [arr[::5] for arr in args]),
 * which the reference does not have.  With stride k >= 1 the Fisher rows are the feed's rows i with i % k == 0,
 * n_sub = ceil(n / k) of them, and every Fisher-vector product the engine evaluates is
 *   F_sub v + damping v,   F_sub = (1 / n_sub) sum_{i % k == 0} J_i^T M_i J_i
 * (J_i the Jacobian of row i's head outputs, M_i the head's Fisher metric: the FVP above, over those rows with
 * N = n_sub).  That is trpo_fvp, trpo_cg and, inside trpo_update, the CG products and the shs product.  Everything
 * else still runs on all n rows: the advantages, g, the losses, every line-search trial and the kl > 2 max_kl
 * revert.  The engine keeps the sampled rows in a child engine of ceil(max_rows / k) rows, gathered on the device
 * whenever the feed or its advantages change; products and CG solves are bit-identical to those of a plain engine
 * with max_rows = ceil(max_rows / k) that was fed states[::k], actions[::k], advant[::k], old[::k].
 * k = 1 (the default) is the engine without any of this: no child, no launch, no allocation.
 * This entry point (the local mode) is single-process only: with k > 1 a feed whose n_global != n, trpo_comm_init and
 * trpo_comm_set_host_allreduce fail with TRPO_ERR_STATE, and so does trpo_set_fvp_subsample(k > 1) on an engine that
 * has a communicator or a host transport; k < 1 fails with TRPO_ERR_STATE; nothing is launched in either case.
 * Changing k, or the mode (below), drops the captured update graph. */
int trpo_set_fvp_subsample(trpo_engine* e, int stride);
/* The same child engine with the stride taken over GLOBAL row indices, for a batch sharded over ranks.  Rank r holds
 * rows [o_r, o_r + n_r) of a global batch of n_global rows (o_r: trpo_set_row_offset).  Its Fisher rows are the local
 * rows i with (o_r + i) % k == 0:
 *   phase_r = (k - o_r % k) % k                          the first local Fisher row
 *   n_sub_r = ceil((n_r - phase_r) / k) if n_r > phase_r, else 0
 *   N_sub   = ceil(n_global / k)                          known to every rank without a collective
 * and the rank's partial of every Fisher-vector product is scaled by 1 / N_sub and all-reduced like the full one.
 * When the ranks' shards tile [0, n_global), sum_r n_sub_r = N_sub and the product is the single-process
 * trpo_set_fvp_subsample(k) product on the concatenated batch, up to summation order.  Offsets that tile the batch
 * are the caller's responsibility: the engine checks only its own shard against n_global.  With offset 0 and
 * n_global == n this is the local mode's rows 0, k, 2k, ...
 * Allowed with a communicator or a host transport, set before or after it; the child's all-reduces go through its
 * owner's transport.  An engine needs n > 0, the child included, so a rank without a Fisher row is refused, not
 * supported.  A feed with row0 + n > n_global or n <= phase fails with TRPO_ERR_STATE, nothing launched and the
 * previous feed left in place; so does this call when the current feed is such a feed.  k = 1 is the plain engine. */
int trpo_set_fvp_subsample_global(trpo_engine* e, int stride);
/* row0 >= 0: the global index of the first row of the feeds that follow (trpo_set_batch, trpo_set_batch_gaussian,
 * trpo_rollout_to_batch, trpo_rollout_gaussian_to_batch); the default is 0.  The current feed keeps the offset it was
 * loaded with.  Outside the global mode it is recorded and has no effect: no launch, no byte.  row0 < 0 fails with
 * TRPO_ERR_STATE. */
int trpo_set_row_offset(trpo_engine* e, int64_t row0);
/* the stride in force and this engine's Fisher rows of the current feed, n_sub = ceil(n / stride) or in the global
 * mode n_sub_r (0 without a feed); either may be NULL */
int trpo_get_fvp_subsample(trpo_engine* e, int* stride, int64_t* n_sub);
/* the mode (1 = global rows), N_sub = ceil(n_global / stride) (local mode: n_sub), the current feed's phase (local
 * mode: 0) and the row offset set for the next feeds; any may be NULL */
int trpo_get_fvp_subsample_global(trpo_engine* e, int* global, int64_t* n_sub_global, int64_t* phase, int64_t* row0);
/* The Fisher feed's rows, unpadded, for tests of the gather: states [n_sub][obs_dim] f32, actions [n_sub] int32
 * (categorical, as the engine keeps them) or [n_sub][act_dim] f32 (Gaussian), old [n_sub][A] f32 (old_dist or
 * old_mean), advant [n_sub] f32; any may be NULL.  TRPO_ERR_STATE when the stride is 1 or there is no feed. */
int trpo_fvp_subsample_fetch(trpo_engine* e, float* states, void* actions, float* old, float* advant, int mem);

/* ---- the numpy half --------------------------------------------------------- */
/* conjugate_gradient(fisher_vector_product, b, cg_iters, residual_tol) (utils.py:185-201),
 * device-resident: every FVP, dot and axpy stays on the GPU. */
int trpo_cg(trpo_engine* e, const float* b, float* x_out, int cg_iters, float residual_tol,
            float damping, int* iters_out, int mem);
/* conjugate_gradient(f_Ax, b, cg_iters, residual_tol) for an arbitrary host f_Ax
 * (utils.py:185-201, the reference's generic signature).  The CG vectors, dots and axpys run
 * on the current GPU in `dtype` (TRPO_F32 / TRPO_F64, the dtype of the caller's b); for each
 * iteration p is copied out and f_Ax(p, z, ctx) must write z = A p (n elements of dtype) and
 * return 0.  Engine-free. */
#define TRPO_F32 0
#define TRPO_F64 1
typedef int (*trpo_fax_cb)(const void* p, void* z, void* ctx);
int trpo_cg_callback(trpo_fax_cb f_Ax, void* ctx, const void* b, void* x_out, int64_t n, int dtype,
                     int cg_iters, double residual_tol, int* iters_out);
/* linesearch(loss, x, fullstep, expected_improve_rate) (utils.py:170-182) with f = the policy
 * surrogate (trpo_inksci.py:127-129).  theta_out = accepted xnew or x; k_out = accepted index or -1.
 * Leaves the engine's parameters at the last evaluated point, as loss() does. */
int trpo_linesearch(trpo_engine* e, const float* x, const float* fullstep, double expected_improve_rate,
                    float* theta_out, int* k_out, int mem);

/* ---- the update block (trpo_inksci.py:101-158) ---------------------------------- */
void trpo_default_params(trpo_update_params* p);
int trpo_update(trpo_engine* e, const trpo_update_params* p, trpo_update_stats* stats);

/* ---- engine-free helpers ------------------------------------------------------------ */
/* number of visible GPUs (0 when none); never fails on a host without GPUs */
int trpo_device_count(int* out);
/* discount(x, gamma) (utils.py:14-16) over a concatenation of paths on the current device.
 * episode_starts may be NULL (one path). */
int trpo_discount(const double* x, const uint8_t* episode_starts, int64_t n, double gamma,
                  double* out, int mem);
/* GAE(lambda) (see TRPO_ADV_GAE) over a concatenation of paths on the current device: adv_out = A,
 * returns_out = R.  values (V = 0), episode_starts (one path), tail_values (0) and either output may be
 * NULL; n = 0 succeeds and writes nothing. */
int trpo_gae(const double* rewards, const double* values, const uint8_t* episode_starts,
             const double* tail_values, int64_t n, double gamma, double lambda, double* adv_out,
             double* returns_out, int mem);

/* ---- kernel-variant switches (for A/B measurements and variant parity tests) ----------
 * "split_mfma" (0 = f32 MFMA row GEMMs; 5 = the 256 x 256 split row-GEMM tile for outputs wider than
 * 128, at BK 32 on f16 planes, the default; 6 = the same tile at BK 16; any other value = 128 x 256),
 * "split_wg" (0 = f32 weight gradients; 1 = split tile for fan_out > 128), "chain" (fused FVP chain: 0 off, 1 auto, 2..4 forced variants),
 * "split_f16" (split GEMMs on scaled f16 hi+lo planes), "split_min_k" (few-k row GEMMs stay on f32
 * MFMA), "graphs" (1 = trpo_update replays its sync-free prefix as a captured hipGraph, all-reduces
 * included; results are bit-identical to eager launches), "tail" (1 = the fused last-layer FVP tail
 * of tail.hip where eligible: f16 split, last hidden width in (128, 256], 17..32 actions), "fused"
 * (whole FVP incl. weight gradients in one launch of fused.hip for one or two hidden layers of
 * width <= 64, obs <= 128, <= 32 actions: 0 off, 1 = 8-wave workgroups, 2 = 4-wave workgroups, 3 = the
 * default: two hidden layers of width 49..64 on the scaled f16 hi+lo split (fused16.hip, needs "split_f16"),
 * other eligible shapes as 2),
 * "low_seg" (f16 split GEMMs with two K-segments: a segment whose running-max product scale lies at
 * least this many binades below the other's -- the O(eps) KL_ff plain-delta terms -- runs on one
 * f16 product instead of three; 4 more binades when the dominant segment has an operand without a
 * running max; 0 = off; default 14), "planes" (1 = row GEMMs whose operands the engine keeps as
 * pre-split k-blocked f16 hi/lo planes run the LDS-DMA plane kernel of plane.hip; bit-identical to
 * the register-staged split; default 1),
 * "rbwd0" (1 = layer 1's R-backward and layer 0's weight gradient run as one launch of rbwd0.hip:
 * RD_0 stays in registers and X^T RD_0 is reduced from the engine's X planes; eligible on the f16
 * split with planes on, obs <= 128, hidden widths <= 256 and multiples of 32; also serves the policy
 * gradient's layer-1 backward; default 1),
 * "hbwd2" (1 = the prepare pass's and the policy gradient's backward through the softmax head's layer
 * run as one launch of hbwd.hip over one read of H_{L-1}, which also writes D_{L-2}'s f16 hi plane for
 * rbwd0 (or E_{L-2} where the FVP path reads it) and the policy gradient's head-layer weight gradient;
 * <= 32 actions, last hidden width 129..256; 2 = on f32 MFMA, the default; 1 = on VALU f32 FMA chains),
 * "head_fwd" (softmax head forwards with one state per lane on f32 FMAs,
 * hbwd.hip: 1 = the prepare and the line-search heads, the default; 2 = the line-search heads, and the
 * prepare head when the head has <= 8 actions; 0 = off), "splits" (split-K slabs of the FVP's weight
 * gradients; 0 = auto: by tile count, at least one per 16k rows; 512 at C4, 245 at C5) and "pg_splits" (the
 * policy gradient's; 0 = auto: 4 x splits or one per 4k rows, up to 2048): both are read when an engine
 * is created; "ls_fused" (where the FVP runs on fused16.hip, the policy forward as one launch from f16 weight
 * images, fwd_loss16: 1 = the prepare pass's and the line search's, the default; 2 = the line search's only;
 * 0 = the per-layer forwards); "cg_fuse_reduce" (single rank with the one-launch FVP: each CG iteration's slab
 * reduction fused with its z = Hv + damping p step; 1 = on, the default; 2 = on, and the rest of the iteration
 * (x, r, p, the next FVP's f16 V image) runs in the same launch, in the workgroup that finishes last,
 * bit-identical to 1 but slower (one CU's serial tail); 0 = off: 0 and 1 group the p.z partials differently, so
 * each is deterministic but their CG scalars are not bit-identical to each other).
 * "cg_p_img" (the fused16 path: each CG iteration's p update and the next FVP's f16 V images in one launch,
 * bit-identical: 1 = on, the default; 0 = two launches).
 * "rfwd01" (the FVP's R-forward through layers 0 and 1 as one launch, rfwd.hip, where two hidden layers of 256
 * with obs <= 128 run the fused tail: 1 = on, the default; 0 = the plane and row GEMM launches).
 * "fwd01" (the prepare and line-search forwards through layers 0 and 1 as one launch, rfwd.hip, at the same
 * shapes: 1 = on, the default; 0 = the plane and row GEMM launches).
 * "rh1_planes" (where "rfwd01" and "rbwd0" both run on the f16 split: rfwd01 writes RH_1 as two row-paired f16
 * planes, hi and lo, in the bytes of the f32 matrix, and its readers, rbwd0's epilogue and the layer-1 weight
 * gradient, fetch the hi plane alone where their "low_seg" test fires and both planes where it does not:
 * 1 = on, the default; 0 = RH_1 in f32, every launch and every bit as without the option).
 * "rbwd0_bdma" (rbwd0.hip's k-loop: the pre-split weight planes reach LDS by LDS-DMA, a ring of three 32-KB
 * slots, instead of through registers; the same planes, products and order, so bit-identical: 1 = on, the
 * default; 0 = register-staged).
 * "ls_fused" = 2 mixes two forwards inside one line search (loss_before from the per-layer forward, the
 * trials' losses from fwd_loss16); it exists for A/B timing and is held to the same parity tests.
 * Rejected variants (other tiles, last-layer fusions, 16-bit E planes, a second stream) were removed
 * from the build in round 4; tools/patches/pruned_variants.patch restores them.
 * Process-wide. */
int trpo_set_option(const char* name, int value);
/* Host-only: whether a batch whose X planes have x_mpad rows (n rounded up to 256) is within the row limit of the
 * one-launch forwards ("rfwd01" / "fwd01") and of the row-paired planes ("rh1_planes").  The engine's gates and the
 * launchers read the same two predicates, so a default-on path cannot throw on a row count the fallback takes. */
int trpo_plane_rows_ok(int64_t x_mpad, int* rfwd01_ok, int* pair_planes_ok);
int trpo_get_option(const char* name, int* value);

/* ---- profiling: per-launch HIP events on the engine stream ------------------------- */
int trpo_profile_enable(trpo_engine* e, int enable);
/* JSON {"tag": [count, total_ms], ...}; returns bytes needed (excluding NUL) or < 0 */
int trpo_profile_query(trpo_engine* e, char* buf, int cap);
int trpo_profile_reset(trpo_engine* e);

/* ==== sampling and rollouts (trpo_inksci.py:76-87, utils.py:18-45,95-105) ======================
 * The reference steps one gym CartPole-v0 env and calls agent.act once per step (a 1-row
 * session.run + cat_sample).  Here n_envs CartPole-v0 instances (gym's classic_control/cartpole.py
 * restated in float64; gym is not vendored) run on the GPU, one wave each, under the engine's
 * current policy.  Every environment collects whole episodes until its own step count reaches
 * ceil(n_timesteps / n_envs) -- utils.py:23-44's stopping rule per environment (n_envs = 1 is the
 * reference's loop) -- and the episodes are concatenated in environment order.
 * The reference does not tell a path the environment terminated from one that time_limit or
 * max_pathlength cut off.  The rollout records it per path, with the state s_T after the last step and
 * the policy's distribution there (trpo_rollout_fetch_ends), so that GAE can bootstrap cut-off paths
 * from V(s_T) (trpo_get_tail_view, trpo_vf_predict_tails).  The per-step outputs and the random
 * draws do not depend on it.
 *
 * Two more of gym's discrete-action classic_control tasks, which the reference does not run, roll out the same way
 * (trpo_rollout_env).  gym is not vendored: the equations below are the definition.  All arithmetic is float64
 * in the operation order written (x^2 is x*x), pi = 3.141592653589793, min/max as Python's.
 *
 * MountainCar-v0: state = obs = (p, v); actions 0, 1, 2; time limit 200.
 *   reset: p = -0.6 + (-0.4 - -0.6)*u0, v = 0 (one draw)
 *   step:  v = v + (action-1)*0.001 + cos(3*p)*(-0.0025);  v = min(max(v,-0.07),0.07)
 *          p = p + v;  p = min(max(p,-1.2),0.6);  if (p == -1.2 && v < 0) v = 0
 *          done = p >= 0.5 && v >= 0;  reward -1 on every step, the terminating one included
 * Acrobot-v1 ("book" dynamics): state (t1, t2, w1, w2); obs (cos t1, sin t1, cos t2, sin t2, w1, w2); actions
 * 0, 1, 2; time limit 500.
 *   reset: s_i = -0.1 + (0.1 - -0.1)*u_i (four draws)
 *   step:  torque a = action - 1; m1 = m2 = l1 = 1, lc1 = lc2 = 0.5, I1 = I2 = 1, g = 9.8, dt = 0.2;
 *          f(t1,t2,w1,w2) = (w1, w2, dd1, dd2) with
 *            d1   = m1*lc1^2 + m2*(l1^2 + lc2^2 + 2*l1*lc2*cos(t2)) + I1 + I2
 *            d2   = m2*(lc2^2 + l1*lc2*cos(t2)) + I2
 *            phi2 = m2*lc2*g*cos(t1 + t2 - pi/2)
 *            phi1 = -m2*l1*lc2*w2^2*sin(t2) - 2*m2*l1*lc2*w2*w1*sin(t2) + (m1*lc1 + m2*l1)*g*cos(t1 - pi/2) + phi2
 *            dd2  = (a + d2/d1*phi1 - m2*l1*lc2*w1^2*sin(t2) - phi2) / (m2*lc2^2 + I2 - d2^2/d1)
 *            dd1  = -(d2*dd2 + phi1)/d1
 *          one classical RK4 step: k1 = f(y), k2 = f(y + dt/2*k1), k3 = f(y + dt/2*k2), k4 = f(y + dt*k3),
 *            y' = y + dt/6*(k1 + 2*k2 + 2*k3 + k4)
 *          then t1, t2 wrapped into [-pi, pi] (while x > pi: x -= 2*pi; while x < -pi: x += 2*pi), w1 clamped to
 *          +-4 pi and w2 to +-9 pi with min(max()); done = -cos(t1) - cos(t2 + t1) > 1.0 on the new state;
 *          reward = done ? 0 : -1
 * Reset draws are Philox (seed, env index, stream 1, episode*reset_draws + i), action draws (seed, env index,
 * stream 0, step count), for every environment. */
#define TRPO_ENV_CARTPOLE_V0 0
#define TRPO_ENV_MOUNTAINCAR_V0 1
#define TRPO_ENV_ACROBOT_V1 2
typedef struct trpo_env_info_t {
  int obs_dim, state_dim, n_actions;
  int reset_draws;           /* uniforms one env.reset() consumes */
  int time_limit;            /* the task's TimeLimit */
  char name[32];
} trpo_env_info_t;
/* Host-only (works with no GPU): the table of a built-in environment; an unknown id is TRPO_ERR_ARG. */
int trpo_env_info(int env, trpo_env_info_t* out);
typedef struct trpo_rollout_params {
  int n_envs;                /* parallel environments (1) */
  int max_pathlength;        /* config["max_steps"] = 1000 (trpo_inksci.py:17; utils.py:28) */
  int64_t n_timesteps;       /* config["episodes_per_roll"] = 1000 (trpo_inksci.py:17; utils.py:23) */
  int train;                 /* 1: cat_sample; 0: argmax (trpo_inksci.py:79-83) */
  int time_limit;            /* the TimeLimit: CartPole-v0's 200 steps by default */
  uint64_t seed;             /* Philox stream: action uniforms and env.reset draws */
  /* optional injected uniforms (tests): reset [n_envs][max_episodes_per_env][reset_draws] in [0,1) and
   * cat_sample [n_envs][ceil(n_timesteps/n_envs) + min(max_pathlength, time_limit) - 1] */
  const double* reset_uniforms;
  const double* action_uniforms;
  int max_episodes_per_env;
  int mem;                   /* where the injected arrays live */
} trpo_rollout_params;
void trpo_default_rollout_params(trpo_rollout_params* p);
/* run the rollout; returns the total steps N and the number of paths */
int trpo_rollout_cartpole(trpo_engine* e, const trpo_rollout_params* p, int64_t* n_steps_out, int64_t* n_paths_out);
/* trpo_default_rollout_params with the environment's own time_limit */
int trpo_default_rollout_params_env(int env, trpo_rollout_params* p);
/* The same rollout of environment `env` (TRPO_ENV_*); trpo_rollout_cartpole is env = TRPO_ENV_CARTPOLE_V0.  The
 * engine's obs_dim and n_actions must be the environment's: TRPO_ERR_ARG otherwise, with both in the message. */
int trpo_rollout_env(trpo_engine* e, int env, const trpo_rollout_params* p, int64_t* n_steps_out,
                     int64_t* n_paths_out);
/* the environment state every observation was made from, concatenated like obs: [N][state_dim] f64 (for
 * CartPole-v0 and MountainCar-v0 the observation itself).  TRPO_ERR_STATE when there is no rollout. */
int trpo_rollout_fetch_states(trpo_engine* e, double* env_states, int mem);
/* the concatenated paths (utils.py:36-39): obs [N][obs_dim] f64 (and/or as the float32 the placeholders
 * receive), actions [N] i64, action_dists [N][A] f32, rewards [N] f64, episode_starts [N] u8, and the
 * cat_sample uniform of every step; any may be NULL */
int trpo_rollout_fetch(trpo_engine* e, double* obs, float* obs32, int64_t* actions, float* action_dists,
                       double* rewards, uint8_t* episode_starts, double* uniforms, int mem);
/* How each of the rollout's n_paths paths ended, in the order of the concatenated rollout: truncated
 * [n_paths] u8 (1 = the path's last step did not terminate the environment: time_limit or
 * max_pathlength cut it off; a step that terminates and reaches the limit counts as terminated),
 * final_obs [n_paths][obs_dim] f64 (the observation of s_T, the state after the last step), final_dists [n_paths][A] f32
 * (the policy at float32(s_T) for cut-off paths, zeros for terminated ones), lengths [n_paths] i64 (T)
 * and end_rows [n_paths] i64 (the row of the path's last step); any may be NULL.  TRPO_ERR_STATE
 * when there is no rollout. */
int trpo_rollout_fetch_ends(trpo_engine* e, uint8_t* truncated, double* final_obs, float* final_dists,
                            int64_t* lengths, int64_t* end_rows, int mem);
/* the rollout becomes the feed on the device (trpo_inksci.py:108-112,119-122): states, actions,
 * oldaction_dist, rewards and path starts, with no host round trip; baseline cleared */
int trpo_rollout_to_batch(trpo_engine* e, int64_t n_global);
/* Device pointers into the current feed, for other device-side consumers (the VF) to read in place;
 * synchronises the engine stream first. */
typedef struct trpo_feed_view {
  int64_t n, n_global;
  int obs_dim, n_actions;
  const float* states;       /* [n][ld_states] f32 */
  int ld_states;
  const float* old_dist;     /* [n][ld_old] f32; on a Gaussian engine the old mean */
  int ld_old;
  const uint8_t* episode_starts;   /* [n] */
  const double* returns;     /* [n] f64 after the advantages of this feed were computed, else NULL */
  double* baseline;          /* [n] f64; trpo_set_baseline(e, view.baseline, TRPO_MEM_DEVICE) marks it set */
  const int64_t* step_index; /* [n] each row's step index in its episode when the feed is a segment rollout's
                              * (trpo_rollout_env_segment), else NULL: a path then starts at step 0 */
} trpo_feed_view;
int trpo_get_feed_view(trpo_engine* e, trpo_feed_view* out);
/* The companion view of the feed's path ends, for the consumer that computes V(s_T) on the device (the
 * VF: trpo_vf_predict_tails).  Valid only while the feed is the one trpo_rollout_to_batch loaded:
 * after trpo_set_batch, trpo_set_rewards or a new rollout it fails with TRPO_ERR_STATE.  Zero-fills the
 * engine's tail buffer, leaves the feed without tail values and synchronises the engine stream;
 * trpo_set_tail_values(e, view.tail, TRPO_MEM_DEVICE) then marks the buffer set without a copy. */
typedef struct trpo_tail_view {
  int64_t n, n_paths;
  int obs_dim, n_actions;
  const float* final_obs32;  /* [n_paths][obs_dim] float32(s_T) */
  const float* final_dist;   /* [n_paths][n_actions] f32 */
  const int64_t* lengths;    /* [n_paths] T, the episode's step count at s_T (of a segment rollout's path, which
                              * may continue an episode: t0 + its rows, not the rows trpo_rollout_fetch_ends reports) */
  const uint8_t* truncated;  /* [n_paths] */
  const int64_t* end_rows;   /* [n_paths] */
  double* tail;              /* [n] f64, the engine's tail values */
} trpo_tail_view;
int trpo_get_tail_view(trpo_engine* e, trpo_tail_view* out);
/* set only the baseline [n] f64 of the current feed (VF.predict output, trpo_inksci.py:103) */
int trpo_set_baseline(trpo_engine* e, const double* baseline, int mem);
/* explained_variance(baseline, returns) (utils.py:208-211, trpo_inksci.py:167) over the current
 * feed (all ranks), after the returns were computed; NaN when var(returns) == 0 */
int trpo_explained_variance(trpo_engine* e, double* out);
/* agent.act on n states [n][obs_dim] f32 (trpo_inksci.py:76-87): action_dist at the current
 * parameters and cat_sample against `uniforms` [n] (train = 1) or argmax (train = 0).
 * n_actions <= 64 here (one wave per state): an engine created with 65..128 actions updates, but
 * trpo_act returns an error for it (and trpo_rollout_cartpole needs exactly 2 actions). */
int trpo_act(trpo_engine* e, const float* states, int64_t n, const double* uniforms, int train, int64_t* actions_out,
             float* dists_out, int mem);
/* the Gaussian policy's act on n states [n][obs_dim] f32: mean_out [n][act_dim] at the current parameters,
 * logstd_out [act_dim], and actions_out [n][act_dim] = float32(mean + exp(logstd) * normals) with normals
 * [n][act_dim] f64 (train = 1; the sum and product in float64) or the mean (train = 0, normals may be NULL).
 * Any output may be NULL.  act_dim <= 64 here (one wave per state), as trpo_act. */
int trpo_act_gaussian(trpo_engine* e, const float* states, int64_t n, const double* normals, int train,
                      float* actions_out, float* mean_out, float* logstd_out, int mem);
/* cat_sample(prob_nk) (utils.py:95-105) with the uniforms given: engine-free, current device */
int trpo_cat_sample(const float* prob, int64_t n, int k, const double* uniforms, int64_t* out, int mem);
/* one CartPole-v0 step per row (state [n][4] f64, action [n] i64); done = termination (not the TimeLimit) */
int trpo_cartpole_step(const double* state, const int64_t* action, int64_t n, double* state_out, double* reward,
                       uint8_t* done, int mem);
/* one step per row of environment `env`: state [n][state_dim] f64, action [n] i64 -> state_out [n][state_dim],
 * obs_out [n][obs_dim] (the observation of state_out), reward [n], done [n] (termination, not the TimeLimit);
 * any output may be NULL.  Engine-free, current device. */
int trpo_env_step(int env, const double* state, const int64_t* action, int64_t n, double* state_out, double* obs_out,
                  double* reward, uint8_t* done, int mem);

/* ==== continuous-action rollouts under the Gaussian policy ======================================
 * Two of gym's continuous-action classic_control tasks roll out on a TRPO_DIST_GAUSSIAN engine the way the
 * discrete ones do on a categorical engine: one wave per environment, whole episodes until the environment's own
 * step count reaches ceil(n_timesteps / n_envs), the path-end records, the concatenation in environment order.
 * They have a table and entry points of their own, next to the discrete ones.  gym is not vendored: the equations
 * below are the definition.  All arithmetic is float64 in the operation order written (x^2 is x*x),
 * pi = 3.141592653589793, clamp(x, lo, hi) = min(max(x, lo), hi) as Python's; an action component is the float32
 * the policy produced, widened to float64.
 *
 * Pendulum-v1: state (th, thd); obs (cos th, sin th, thd); act_dim 1; time limit 200; it never terminates.
 *   reset: th = -pi + (pi - -pi)*u0, thd = -1 + (1 - -1)*u1 (two draws)
 *   step:  u = clamp(a, -2, 2);  y = th + pi;  m = fmod(y, 2*pi);  if (m < 0) m = m + 2*pi;  an = m - pi
 *          cost = an*an + 0.1*(thd*thd) + 0.001*(u*u)
 *          thd' = thd + (3*10.0/(2*1.0)*sin(th) + 3.0/(1.0*(1.0*1.0))*u)*0.05;  thd' = clamp(thd', -8, 8)
 *          th' = th + thd'*0.05;  reward = -cost;  done = false
 * MountainCarContinuous-v0: state = obs = (p, v); act_dim 1; time limit 999.
 *   reset: p = -0.6 + (-0.4 - -0.6)*u0, v = 0 (one draw)
 *   step:  f = clamp(a, -1, 1);  v = v + f*0.0015 + cos(3*p)*(-0.0025);  v = clamp(v, -0.07, 0.07)
 *          p = p + v;  p = clamp(p, -1.2, 0.6);  if (p == -1.2 && v < 0) v = 0
 *          done = p >= 0.45 && v >= 0;  reward = (done ? 100 : 0) - (a*a)*0.1, with the unclamped a, as gym's
 *
 * Per step the rollout runs the policy's mean forward on float32(obs) and forms, for d < act_dim,
 * a_d = float32(double(mu_d) + exp(double(logstd_d)) * xi_d) when train (trpo_act_gaussian's arithmetic), else
 * a_d = mu_d with a recorded xi of 0.  The normals are a Box-Muller pair off one Philox call: counter (env index,
 * stream 0, k) with k = step_count*act_dim + d, step_count the environment's steps so far over all its episodes
 * (it advances whether or not train); u1 from words (c0, c1) and u2 from (c2, c3) by the 53-bit recipe
 * ((c>>5)*2^26 + (c'>>6)) / 2^53; xi = sqrt(-2*log(1 - u1)) * cos(2*pi*u2).  Reset draws are as for the discrete
 * environments: stream 1, index episode*reset_draws + i.  The rollout samples with a snapshot of the log-std
 * vector taken when it starts. */
#define TRPO_CENV_PENDULUM_V1 0
#define TRPO_CENV_MOUNTAINCAR_CONTINUOUS_V0 1
typedef struct trpo_cont_env_info_t {
  int obs_dim, state_dim, act_dim;
  int reset_draws;           /* uniforms one env.reset() consumes */
  int time_limit;            /* the task's TimeLimit */
  char name[32];
} trpo_cont_env_info_t;
/* Host-only (works with no GPU): the table of a continuous-action environment; an unknown id is TRPO_ERR_ARG. */
int trpo_cont_env_info(int cenv, trpo_cont_env_info_t* out);
/* trpo_default_rollout_params with the environment's own time_limit */
int trpo_default_rollout_params_cont(int cenv, trpo_rollout_params* p);
/* The rollout of environment `cenv` (TRPO_CENV_*) on a Gaussian engine whose obs_dim and act_dim are the
 * environment's: TRPO_ERR_ARG otherwise, with both in the message.  In `p`, train = 1 samples and train = 0 acts
 * with the mean; the injected action_uniforms are standard normals [n_envs][ceil(n_timesteps/n_envs) +
 * min(max_pathlength, time_limit) - 1][act_dim].  Returns the total steps N and the number of paths. */
int trpo_rollout_gaussian(trpo_engine* e, int cenv, const trpo_rollout_params* p, int64_t* n_steps_out,
                          int64_t* n_paths_out);
/* the concatenated paths: obs [N][obs_dim] f64 (and/or f32), actions and means [N][act_dim] f32, logstd [act_dim]
 * f32 (the rollout's snapshot), rewards [N] f64, episode_starts [N] u8, the normal of every action component
 * [N][act_dim] f64 (zeros when train = 0) and the state every observation was made from [N][state_dim] f64; any
 * may be NULL */
int trpo_rollout_gaussian_fetch(trpo_engine* e, double* obs, float* obs32, float* actions, float* means,
                                float* logstd, double* rewards, uint8_t* episode_starts, double* normals,
                                double* env_states, int mem);
/* trpo_rollout_fetch_ends of a Gaussian rollout: final_means [n_paths][act_dim] f32 is the policy's mean at
 * float32(s_T) for cut-off paths, zeros for terminated ones */
int trpo_rollout_gaussian_fetch_ends(trpo_engine* e, uint8_t* truncated, double* final_obs, float* final_means,
                                     int64_t* lengths, int64_t* end_rows, int mem);
/* the rollout becomes the feed on the device: states, actions, old mean, the old log-std from the rollout's
 * snapshot, rewards, path starts and the path-end records; baseline and tail values cleared.  trpo_get_feed_view,
 * trpo_get_tail_view (final_dist = the mean at s_T, n_actions = act_dim), trpo_vf_predict_tails,
 * trpo_compute_advantages and trpo_update then work as on a categorical rollout feed. */
int trpo_rollout_gaussian_to_batch(trpo_engine* e, int64_t n_global);
/* one step per row of environment `cenv`: state [n][state_dim] f64, action [n][act_dim] f32 -> state_out, obs_out
 * [n][obs_dim] (the observation of state_out), reward [n], done [n] (termination, not the TimeLimit); any output
 * may be NULL.  Engine-free, current device. */
int trpo_cont_env_step(int cenv, const double* state, const float* action, int64_t n, double* state_out,
                       double* obs_out, double* reward, uint8_t* done, int mem);

/* ==== fixed-horizon rollout segments: environments that persist across calls ====================
 * The rollouts above reset every environment at the start of every call and collect whole episodes.  A segment
 * rollout collects as baselines' traj_segment_generator does: every environment takes exactly
 * H = ceil(n_timesteps / n_envs) steps per call and continues where the previous call left it, so a rollout has
 * exactly n_envs * H rows.  It runs on both heads and all five environments; observe, forward, sample and step are
 * those of the whole-episode rollout, operation for operation.
 *
 * Per environment the engine keeps a carry, which outlives every rollout and trpo_set_flat: the state s
 * [state_dim] f64, t (the steps taken in the current episode) and ret (the f64 sum of the current episode's rewards
 * so far, added in step order).  With ep_max = min(max_pathlength, time_limit) one call runs, per environment:
 *
 *   resume ? load the carry : (reset with reset index 0; t = 0; ret = 0)
 *   for k in 0 .. H-1:
 *     row = env*H + k
 *     observe, forward, sample, step, and record what the whole-episode rollout records per step, plus
 *       step_index[row] = t              the step's index in its episode
 *       starts[row] = (k == 0 || the previous step ended an episode)
 *     t += 1; ret += reward
 *     if done or t >= ep_max:
 *       end record of kind 0 (terminated) or 1 (cut by the limit; a step that does both is a termination)
 *       reset with the next reset index; t = 0; ret = 0
 *   if the last step did not end an episode:
 *     end record of kind 2 (cut by the segment); the environment is not reset
 *   store the carry
 *
 * A path of a segment rollout is the fragment of an episode that lies in the call, so the paths tile the rows.
 * An end record holds what the whole-episode rollout's does -- truncated (1 for kinds 1 and 2, so that both are
 * bootstrapped from V(s_T)), the observation of s_T, the head row at float32(s_T) of a cut-off path from one more
 * forward that draws nothing, the fragment's rows as `lengths` and its last row -- and four more fields: end_kind,
 * t0 (the episode step index of the fragment's first row), the fragment's row count, and episode_return (ret at
 * the path's end, earlier segments included).  For kind 2, s_T is the carried state: its observation is bitwise
 * the next call's row-0 observation of that environment.
 *
 * Random draws are indexed per call: the action draw of the environment's step k is Philox (seed, env index,
 * stream 0, k), or (Gaussian) the normal of component d at k*act_dim + d; reset draws are stream 1 at
 * reset_index*reset_draws + i, reset_index counting this environment's resets within this call (resume = 0: the
 * initial reset is index 0).  Injected action draws are [n_envs][H]([act_dim]); injected reset_uniforms are
 * [n_envs][max_episodes_per_env][reset_draws] with max_episodes_per_env >= H + (resume ? 0 : 1).
 *
 * trpo_rollout_fetch*, trpo_rollout_gaussian_fetch*, *_fetch_ends, *_fetch_states and *_to_batch work on a segment
 * rollout unchanged.  The feed loaded from one also carries step_index (trpo_feed_view.step_index), which the VF's
 * time feature then uses in place of the distance to the path's start, and its trpo_tail_view.lengths are the
 * episodes' step counts at s_T, t0 + rows.
 *
 * Refused with TRPO_ERR_STATE or TRPO_ERR_ARG, nothing launched, the previous rollout and the carry left as they
 * were: resume = 1 without a carry, or with a carry of another environment, head or n_envs, or with a carried
 * t >= ep_max (or < 0); the wrong head for the call; an engine whose obs_dim or head width is not the
 * environment's; max_episodes_per_env too small for the injected resets.  n_envs * H rows beyond the engine's
 * max_rows are refused by *_to_batch. */
/* exactly H = ceil(p->n_timesteps / p->n_envs) steps per environment; resume = 0 resets every environment
 * first, resume = 1 continues from the carry */
int trpo_rollout_env_segment(trpo_engine* e, int env, const trpo_rollout_params* p, int resume, int64_t* n_steps_out,
                             int64_t* n_paths_out);
int trpo_rollout_gaussian_segment(trpo_engine* e, int cenv, const trpo_rollout_params* p, int resume,
                                  int64_t* n_steps_out, int64_t* n_paths_out);
/* of the last rollout when it was a segment rollout (TRPO_ERR_STATE otherwise); any may be NULL:
 * end_kind [P] u8, t0 [P] i64, episode_returns [P] f64, step_index [N] i64 */
int trpo_rollout_segment_fetch(trpo_engine* e, uint8_t* end_kind, int64_t* t0, double* episode_returns,
                               int64_t* step_index, int mem);
/* the carry: states [n_envs][state_dim] f64, t [n_envs] i64, returns [n_envs] f64; any output may be NULL.
 * TRPO_ERR_STATE when there is none. */
int trpo_rollout_carry_get(trpo_engine* e, int* env_out, int* n_envs_out, double* states, int64_t* t,
                           double* returns, int mem);
/* env: TRPO_ENV_* or TRPO_CENV_* by the engine's dist; the engine's obs_dim and head width must be the
 * environment's (TRPO_ERR_ARG) */
int trpo_rollout_carry_set(trpo_engine* e, int env, int n_envs, const double* states, const int64_t* t,
                           const double* returns, int mem);
int trpo_rollout_carry_clear(trpo_engine* e);

/* ==== value-function baseline: class VF (utils.py:48-92) ==================================
 * Features [obs | action_dist | t/10] (VF._features, utils.py:70-77) -> fully_connected(64, relu)
 * -> fully_connected(64, relu) -> fully_connected(1) (create_net, utils.py:56-62); fit = 50 steps
 * of tf.train.AdamOptimizer() on sum((net - y)^2) over the whole batch (utils.py:64-66,79-85);
 * predict = the net on one path's features (utils.py:87-92).  Parameters are flat in creation
 * order [W1, b1, W2, b2, W3, b3], W row-major [fan_in][fan_out]. */
typedef struct trpo_vf trpo_vf;
/* feat_dim = obs_dim + n_actions + 1; hidden = two widths, each in [1, TRPO_VF_MAX_HIDDEN], or NULL/0 for the
 * reference's {64, 64} (utils.py:60-61); a width outside the range is refused.  Any width in the range works, a
 * multiple of 4 or not: the two ReLU layers and the backward run on the f32 MFMA row tiles at every width (128- or
 * 256-column tiles past 128), the weight gradients on the f32 tiles up to fan_out 128 and on the bf16 x 3 split
 * tiles beyond. */
#define TRPO_VF_MAX_HIDDEN 512
int trpo_vf_create(trpo_vf** out, int feat_dim, const int* hidden, int n_hidden, int64_t max_rows, int device);
void trpo_vf_destroy(trpo_vf* vf);
int64_t trpo_vf_num_params(const trpo_vf* vf);
int trpo_vf_set_params(trpo_vf* vf, const float* flat, int mem);
int trpo_vf_get_params(trpo_vf* vf, float* flat_out, int mem);
/* AdamOptimizer(learning_rate, beta1, beta2, epsilon) (defaults 1e-3, 0.9, 0.999, 1e-8); resets the slots */
int trpo_vf_set_adam(trpo_vf* vf, float lr, float beta1, float beta2, float epsilon);
/* m = v = 0, beta powers = (beta1, beta2): the state tf.initialize_all_variables() gives (utils.py:66) */
int trpo_vf_reset_optimizer(trpo_vf* vf);
/* Adam slots m, v [P] (either may be NULL), beta powers, steps taken */
int trpo_vf_get_optimizer(trpo_vf* vf, float* m_out, float* v_out, float powers_out[2], int64_t* steps_out,
                          int mem);
/* Build the features on the device from a concatenation of paths: obs [n][obs_dim], action_dists
 * [n][n_actions] f32, episode_starts [n] u8 (1 = first step of a path; NULL = one path).  t counts
 * steps from each path start.  n_global = rows over all ranks. */
int trpo_vf_set_features(trpo_vf* vf, int64_t n, int64_t n_global, const float* obs, int obs_dim,
                         const float* action_dists, int n_actions, const uint8_t* episode_starts, int mem);
/* ... or from an engine's feed in place (trpo_get_feed_view), targets = its returns when with_targets */
int trpo_vf_set_features_view(trpo_vf* vf, const trpo_feed_view* view, int with_targets);
/* ... or take a ready feature matrix [n][feat_dim] f32 */
int trpo_vf_set_feature_matrix(trpo_vf* vf, int64_t n, int64_t n_global, const float* feat, int mem);
int trpo_vf_get_feature_matrix(trpo_vf* vf, float* feat_out, int mem);
/* regression targets = the paths' returns [n] (TRPO_F64 as the reference feeds them, or TRPO_F32) */
int trpo_vf_set_targets(trpo_vf* vf, const void* returns, int dtype, int mem);
/* VF.fit's loop body `steps` times (utils.py:84-85; the reference runs 50) */
int trpo_vf_fit(trpo_vf* vf, int steps);
/* gradient of sum((net - y)^2) at the current parameters (all ranks) and, if loss_out, that sum */
int trpo_vf_gradient(trpo_vf* vf, float* grad_out, double* loss_out, int mem);
/* VF.predict: net on the current features -> out [n] (TRPO_F32 / TRPO_F64) */
int trpo_vf_predict(trpo_vf* vf, void* out, int dtype, int mem);
/* V(s_T) of an engine feed's cut-off paths (trpo_get_tail_view): the features of s_T,
 * [final_obs32 | final_dist | float32(T/10.0)] (row t = T of VF._features), one row per path, through
 * the net; then view.tail[end_rows[p]] = truncated[p] ? (double)net[p] : 0.  Afterwards the VF's features
 * are these n_paths rows.  Synchronises the VF's stream; n_paths = 0 succeeds. */
int trpo_vf_predict_tails(trpo_vf* vf, const trpo_tail_view* view);
/* multi-GPU: shard rows, all-reduce the [P] gradient (RCCL), or the host test transport */
int trpo_vf_comm_init(trpo_vf* vf, const uint8_t id[128], int rank, int world);
int trpo_vf_comm_set_host_allreduce(trpo_vf* vf, trpo_allreduce_cb cb, void* ctx, int rank, int world);

#ifdef __cplusplus
}
#endif
#endif /* TRPO_ENGINE_H */
