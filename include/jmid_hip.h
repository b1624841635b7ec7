/*
 * jmid_hip.h  --  C ABI of libjmid_hip.so: the MI355X (gfx950) implementation of the
 * SICNav-Diffusion trajectory predictor hot path (iMID / JMID).
 *
 * The reference (sepsamavi/safe-interactive-crowdnav) has no FFI: its boundary is the
 * Python class HumanTrajectoryForecasterSim (sicnav_diffusion/JMID/mid_sim_wrapper.py:207).
 * The Python host layer in safe-interactive-crowdnav_amd/ keeps that class surface and
 * binds the entry points below with ctypes.  Every entry point names
 * the reference code it replaces (paths relative to sicnav_diffusion/JMID/).
 *
 * Conventions
 *   - plain C types only: pointers, sizes, ints, floats.  No torch / HIP types.
 *   - every function returns 0 on success, a negative JMID_E* code otherwise; the message
 *     is available from jmid_last_error().
 *   - buffers are caller-owned.  `mem` says where they live: JMID_MEM_HOST (the library
 *     copies through its stream) or JMID_MEM_DEVICE (device pointers on the handle's GPU,
 *     e.g. torch.Tensor.data_ptr(); no copies are made).
 *   - one HIP stream per handle, created hipStreamNonBlocking (no implicit ordering against the legacy null stream: other work of
 *     the process on the default stream neither waits for nor delays the predictor); a handle is not re-entrant (the reference is a
 *     single-threaded caller; mid_sim_wrapper.py:174 only locks its history buffer).
 *   - JMID_MEM_DEVICE calls are stream-ordered against the CALLER's stream (jmid_set_caller_stream, default the
 *     legacy null stream): on entry the handle's stream waits for everything the caller enqueued on that stream,
 *     on exit that stream waits for the call's last kernel.  The call may return before the outputs are complete
 *     (exact-fp32 mode; the split modes read a range flag back and therefore block): consume them on the caller's
 *     stream, or call jmid_synchronize first.  Buffers produced or consumed on any OTHER stream need the caller's
 *     own events.  JMID_MEM_HOST calls return with the outputs complete.
 *   - all floating point buffers are fp32, row-major, densely packed.
 *
 * Row / token order used throughout (matches the reference's `context.repeat(sample, 1)`,
 * MID/models/diffusion.py:496, extended with a leading episode axis):
 *     row r = (e * K + s) * A + a          e: episode, s: sample, a: agent
 *     x[r, t, c]                           t: horizon step, c in {x, y}
 */
#ifndef JMID_HIP_H
#define JMID_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
typedef struct jmid_ctx* jmid_handle_t;      /* opaque */

/* The library is built with -fvisibility=hidden: the entry points below are all the C++ host code it exports (next to the
 * kernel handles the HIP runtime needs). */
#pragma GCC visibility push(default)

enum { JMID_NET_IMID = 0, JMID_NET_JMID = 1 };
enum { JMID_MEM_HOST = 0, JMID_MEM_DEVICE = 1 };
/* arithmetic used for the GEMM / attention contractions (softmax, LayerNorm, gates, DDIM are
 * always fp32):
 *   JMID_PREC_F32     exact fp32 MFMA (v_mfma_f32_32x32x2_f32)
 *   JMID_PREC_F16X3   fp32 emulated by three fp16 MFMAs per product on hi/lo-split operands
 *                     (~22 significand bits, fp32 accumulate)
 *   JMID_PREC_F16X2   same operand planes, but the linear contractions take the activation as its fp16 hi plane only:
 *                     A_hi x (W_hi + W_lo) in the GEMMs, two MFMAs per product, and P_hi x V_hi in attention (P rounded to nearest);
 *                     the softmax logits Q.K keep all three terms (their error is exponentiated) and the residual
 *                     stream, LayerNorm and DDIM state keep hi + lo.  Mean ADE vs the reference 7e-6 m on the cfg3
 *                     shape (F16X3: 1e-6 m; gate 1e-4 m), ~35 % more trajectories per second on batches; the lo planes this mode never reads are not written
 *   JMID_PREC_F16MX   F16X2 with the weight-lo correction term of every GEMM on the fp8 matrix path: A_hi x W_hi as fp16 MFMAs
 *                     plus ONE v_mfma_f32_32x32x64_f8f6f4 per 64-deep block on bf8(A_hi) x bf8(W_lo) (bf8 = e5m2 = the top byte
 *                     of the fp16 value, rounded to nearest; unscaled) - 1.5 instead of 2 MFMA passes per product.  The term is
 *                     2^-11 of the product, so its 2-bit significand costs nothing measurable: same GEMM error (2^-12.7) and
 *                     same ADE as F16X2 on every fixture.  In attention (head_dim 128) the two correction terms of the logits
 *                     take the same path (bf8 images of K from the QKV GEMM, of Q made in the kernel), and P.V is one MFMA per
 *                     product: P_hi . V_hi with P rounded to nearest - the one rounding every other activation of the mode gets.
 *                     ~20 % more trajectories per second than F16X2.
 *                     Bit-identical across chunk plans like the other modes.  What bench.py quotes, and since round 6 the default of
 *                     the Python class (together with its first-call self check against JMID_PREC_F16X3).
 *   JMID_PREC_F16     single fp16 MFMA (11 bits; does NOT meet the 1e-4 ADE gate, reported only; not built) */
enum { JMID_PREC_F32 = 0, JMID_PREC_F16X3 = 1, JMID_PREC_F16 = 2, JMID_PREC_F16X2 = 3, JMID_PREC_F16MX = 4 };

enum {
    JMID_OK = 0,
    JMID_EINVAL = -1,     /* bad argument / unsupported dimension */
    JMID_ENOWEIGHT = -2,  /* a required weight has not been loaded */
    JMID_EHIP = -3,       /* HIP runtime error */
    JMID_ENOMEM = -4,
    JMID_ERANGE = -5,     /* F16X3/F16X2/F16MX: an operand left the fp16 range; rerun with JMID_PREC_F32 */
    JMID_ETIMEOUT = -6,   /* a workgroup of a one-launch GEMM + LayerNorm (small F16MX calls) gave up waiting for its partner workgroups -
                             not all of the launch was resident on the GPU (another process or stream held compute units).  Nothing to do
                             with the arithmetic: the outputs are undefined, the handle runs the unfused kernels from now on (same bits,
                             ~0.6 ms more per 50-step one-scene call); repeat the call in the SAME precision.  Counted: jmid_timeout_count */
    JMID_EHISTORY = -7    /* jmid_build_scene_stamped: an episode has fewer than hist_len frames on the time_step grid - where the reference
                             fails with TypeError (get_timesteps_data returns None, MID/mid.py:326); scene.HistoryTooShortError in Python */
};

/* Library / build identification (also the cheap "does it load" probe). */
const char* jmid_version(void);
/* Number of visible HIP devices (0 when there is no GPU); never fails. */
int jmid_device_count(void);

/* Construct a predictor engine on `device_id`.
 * Replaces the module construction of MID._build_model (MID/mid.py:1270-1297):
 *   net_kind  JMID_NET_JMID -> JointPredictionTransformerConcatLinear (MID/models/diffusion.py:153)
 *             JMID_NET_IMID -> TransformerConcatLinear               (MID/models/diffusion.py:112)
 *   ctx_dim   the yaml key `encoder_dim` (d_model = 2*ctx_dim, ff = 4*ctx_dim, LSTM hidden = ctx_dim/2)
 *   tf_layer  the yaml key `tf_layer`;  nhead is 4 in the reference (diffusion.py:121,162)
 *   hist_len  history frames fed to the context encoder (`past_num_frames`, 6 in env.config:11) */
int jmid_create(jmid_handle_t* out, int device_id, int net_kind, int ctx_dim, int tf_layer, int nhead,
                int hist_len);
int jmid_destroy(jmid_handle_t h);
const char* jmid_last_error(jmid_handle_t h);

/* Upload one named fp32 parameter from HOST memory.  Names are the reference's state-dict keys
 * (net: "concat1._layer.weight", "transformer_encoder.layers.0.self_attn.in_proj_weight", ...;
 * encoder: "PEDESTRIAN/node_history_encoder.weight_ih_l0", ...), i.e. what
 * model.load_state_dict(ckpt["ddpm"]) / registrar.load_models(ckpt["encoder"]) consume
 * (MID/mid.py:1231-1232, 1291).  Unknown names are rejected. */
int jmid_load_weight(jmid_handle_t h, const char* name, const float* host_data, size_t n_elems);
/* Check that every parameter is present and build the device-side derived forms
 * (fp16 hi/lo planes, positional-encoding table).  Must be called once after loading. */
int jmid_finalize_weights(jmid_handle_t h);

/* Install the DDIM step table: n_steps entries, one per reverse step, in execution order.
 * Replaces VarianceSchedule + the scalar bookkeeping of sample_sicnav_inference
 * (MID/models/diffusion.py:12-64, 507-528):
 *   beta[i]                       betas[t_i]
 *   c_e[i] = sqrt(1 - abar_t)     c_x[i] = sqrt(abar_t)
 *   n_x[i] = sqrt(abar_{t-s})     n_e[i] = sqrt(1 - abar_{t-s})
 * so that  x0 = (x - e*c_e)/c_x ;  x <- n_x*x0 + n_e*e . */
int jmid_set_ddim_table(jmid_handle_t h, int n_steps, const float* beta, const float* c_e, const float* c_x,
                        const float* n_x, const float* n_e);

/* DDPM variant of the step table (sampling="ddpm", MID/models/diffusion.py:509-522, flexibility 0):
 *   c0[i] = 1/sqrt(alpha_t)   c1[i] = (1-alpha_t)/sqrt(1-abar_t)   sigma[i] = sigmas_inflex[t]
 *   use_noise[i] = (t > 1)    so that  x <- c0*(x - c1*e) + sigma*z   (z = 0 where use_noise is 0).
 * Installing it switches the handle to DDPM until jmid_set_ddim_table is called again. */
int jmid_set_ddpm_table(jmid_handle_t h, int n_steps, const float* beta, const float* c0, const float* c1,
                        const float* sigma, const int* use_noise);

/* Context encoder: Trajectron.get_latent in PREDICT mode
 * (MID/models/trajectron.py:416-454 -> MID/models/encoders/mgcvae.py:505-880).
 *   n_agents   total rows (episodes * agents), any order
 *   x_st       [n_agents, hist_len, 6]     standardized own history
 *   nbr_sum    [n_agents, 2, hist_len, 6]  per edge type (PED->PED, PED->ROBOT) the summed neighbour
 *                                          histories (zeros when there is none; mgcvae.py:726-757)
 *   edge_mask  [n_agents, 2]               clamp(sum(edge values), max=1)  (mgcvae.py:758-768, 821-822)
 *   ctx_out    [n_agents, ctx_dim] */
int jmid_encode(jmid_handle_t h, int n_agents, const float* x_st, const float* nbr_sum, const float* edge_mask,
                float* ctx_out, int mem);

/* jmid_encode for rows seen for fewer than hist_len frames (the reference's first_history_index, MID/dataset/preprocessing.py:468,
 * MID/models/encoders/model_utils.py:77-105): the history LSTM and both edge LSTMs of row r run over frames first_index[r] .. hist_len-1
 * from a zero state and the last output is the encoding.  Frames in front of first_index[r] are not read - x_st AND nbr_sum may hold NaN
 * there.  Row r equals row r of a handle created with hist_len - first_index[r] fed the slice, bit for bit; all zero: jmid_encode's bits.
 *   first_index  [n_agents] int32, a HOST array in both memory modes (like the episode ids of the seeded entries)
 * JMID_EINVAL, before anything is enqueued, for a value outside 0..hist_len-2 (a row needs two frames) or a NULL first_index. */
int jmid_encode_var(jmid_handle_t h, int n_agents, const float* x_st, const float* nbr_sum, const float* edge_mask,
                    const int32_t* first_index, float* ctx_out, int mem);

/* The batched reverse-denoising loop + integrator:
 * DiffusionTraj.sample_sicnav_inference with sampling="ddim" (MID/models/diffusion.py:478-541),
 * the net forward (diffusion.py:133-150 / 173-209) and SingleIntegrator.integrate_samples
 * (MID/models/encoders/dynamics/single_integrator.py:290-321).
 *   E, A, K, T  episodes, agents per episode, samples, horizon
 *   x_T       [E, K*A, T, 2]  initial noise (drawn by the host with torch's CPU generator so that the
 *                             reference's RNG contract is kept, diffusion.py:499)
 *   ctx       [E, A, ctx_dim]
 *   p0        [E, A, 2]       current positions (initial condition of the integrator); may be NULL
 *                             when pos_out is NULL
 *   dt        env time_step
 *   vel_out   [E, K, A, T, 2] predicted velocities            (may be NULL)
 *   pos_out   [E, K, A, T, 2] cumsum(vel)*dt + p0             (may be NULL)
 * JMID attention spans all (t, s, a) tokens of ONE episode (block-diagonal over episodes). */
int jmid_denoise(jmid_handle_t h, int E, int A, int K, int T, const float* x_T, const float* ctx,
                 const float* p0, float dt, int precision, float* vel_out, float* pos_out, int mem);

/* DDPM sampling loop: as jmid_denoise, plus the per-step normal draws the reference takes from the torch generator
 * after x_T (diffusion.py:509): z [n_steps, E, K*A, T, 2] (the host draws them so the RNG contract is kept). */
int jmid_denoise_ddpm(jmid_handle_t h, int E, int A, int K, int T, const float* x_T, const float* z, const float* ctx,
                      const float* p0, float dt, int precision, float* vel_out, float* pos_out, int mem);

/* One evaluation of the denoising net e_theta([x, ctx], beta) for step-table entry `step_idx`
 * (diffusion.py:520); used by the parity tests.  x [E, K*A, T, 2] -> e_out same shape. */
int jmid_net_eval(jmid_handle_t h, int E, int A, int K, int T, int step_idx, const float* x, const float* ctx,
                  int precision, float* e_out, int mem);

/* Per-episode displacement metrics of the sampled futures for the multi-episode evaluation sweep (ADE / FDE as
 * defined in MID/evaluation/evaluation.py:11-28; minimum taken jointly over the scene's agents):
 *   pos [E, K, A, T, 2], gt [E, A, T, 2] -> out [E, 4] = {mean ADE, min-over-samples ADE, mean FDE, min FDE}. */
int jmid_episode_metrics(jmid_handle_t h, int E, int A, int K, int T, const float* pos, const float* gt,
                         float* out, int mem);

/* The statistics the reference's evaluation reports per agent and per scene, for a batch of episodes:
 * compute_batch_statistics (MID/evaluation/evaluation.py:456-739, the branch without is_eval_hst; summarised at MID/mid.py:965-1003
 * and logged as "Best Of 20: ADE / FDE / KDE", "SADE / SFDE").
 *   pos        [E, K, A, T, 2]  sampled futures (jmid_denoise's pos_out layout), or NULL: the positions of the most recent
 *                               jmid_denoise on this handle, under exactly the rules of jmid_topk's pos = NULL below
 *   gt         [E, A, T, 2]     ground-truth futures
 *   agent_out  [E, A, 10] = {ade_min, ade_mean, ade_std, ade_ml, fde_min, fde_mean, fde_std, fde_ml, kde_nll, ml_idx}
 *                - ade[s] = mean_t ||pos - gt||, fde[s] = the last step's distance (compute_ade / compute_fde, :11-36); min, mean and
 *                  np.std (population) over the K samples (:590-602)
 *                - kde_nll (compute_kde_nll, :191-232): per horizon step a 2-D scipy.stats.gaussian_kde of the K points with its defaults
 *                  (covariance with divisor K - 1, Scott's factor K^(-1/6)), its log-pdf at the ground truth clipped below at -20,
 *                  averaged over the steps, negated
 *                - ml_idx (get_most_likely_trajectory_idx -> _calc_kde_nll_for_each_traj, :259-285, 445-453): the sample with the highest
 *                  step-mean clipped log-pdf under the same KDEs (the lowest index on an exact tie), stored as a float;
 *                  ade_ml / fde_ml are that sample's ade / fde (:573-582)
 *                - a step whose covariance has no Cholesky factor (scipy raises LinAlgError, which compute_kde_nll turns into nan,
 *                  :229-230; e.g. K identical samples): kde_nll = NaN, ml_idx = -1, ade_ml = fde_ml = NaN, the other columns as usual
 *   scene_out  [E, 6] = {sade_min, sade_mean, sade_std, sfde_min, sfde_mean, sfde_std}, sade[s] = mean_a ade[s, a], sfde[s] =
 *                mean_a fde[s, a] (:717-737); may be NULL
 * fp64 inside on the fp32 inputs, so the outputs are the fp32 roundings of the reference's float64 values; every reduction runs in
 * a fixed order without atomics: an episode's rows are bit-identical whatever batch it is part of and in both memory modes.
 * 2 <= K <= 1024, T <= 24, any A (JMID_EINVAL beyond).  jmid_episode_metrics above is unchanged by this entry point. */
int jmid_eval_statistics(jmid_handle_t h, int E, int A, int K, int T, const float* pos, const float* gt, float* agent_out,
                         float* scene_out, int mem);

/* The masked form of jmid_eval_statistics: the is_eval_hst branch of compute_batch_statistics (MID/evaluation/evaluation.py:540-545,
 * 556-558, 566-568, 573-577, 624-715; its fixed-horizon columns are printed at MID/mid.py:978-1000, 1051-1075), for episodes whose
 * ground-truth future is only partly real (an episode that ended, a human that arrived).
 *   pos, gt        as jmid_eval_statistics (pos = NULL under the same rules)
 *   interp_future  [E, A, T] bytes, 1 = the step's ground truth is interpolated or absent: not scored (interpolated_future)
 *   skip           [E, A] bytes or NULL, 1 = the agent is left out (the reference: its history is all interpolated, :542-545); an agent
 *                  without any scored step is left out as well
 *   n_cut, cutoffs host ints: the fixed-horizon steps, each in [0, T), n_cut <= 4, may be 0 (the reference hard-codes 2, 5, 8 for
 *                  T = 12: "one / two / three fourth")
 *   agent_out  [E, A, 12] = the ten columns of jmid_eval_statistics, n_valid, fde_valid
 *                - ade[s] = the mean of the distances over the scored steps (compute_ade, :20-22); fde[s] = the last step's distance,
 *                  absent when that step is not scored (compute_fde, :32-34): fde_valid = 0 and fde_min / fde_mean / fde_std / fde_ml NaN
 *                - kde_nll and ml_idx over the scored steps only (np.compress, :212-214, :262-266); one scored step is enough
 *                - n_valid = the number of scored steps; 0 = the agent is left out: every float column NaN, ml_idx = -1
 *   cut_out    [E, A, n_cut, 5] = {ade_min, ade_mean, ade_ml, kde, valid} per cut-off step c; may be NULL when n_cut = 0
 *                - the distance at step c alone per sample (compute_ade with cutoff_idx, :13-18): its min and mean over the samples
 *                  (:634-646) and its value at the most likely sample of the whole masked horizon (:647-653)
 *                - kde: QUIRK OF THE REFERENCE, reproduced.  compute_kde_nll(cutoff_idx = c) slices the ground truth to shape [2] and
 *                  then loops "time steps" over its two entries (:209-222), so it returns the mean of two 1-D gaussian_kde negative
 *                  log-pdfs, each floored at -20 - the K x-coordinates at the ground truth's x and the K y-coordinates at its y, with
 *                  scipy's 1-D defaults (variance with divisor K - 1, Scott's factor K^(-1/5)) - not a 2-D single-step density
 *                - step c not scored (or the agent left out): the four values NaN, valid = 0
 *   scene_out  [E, 6] as jmid_eval_statistics over the agents that are kept (:717-737); may be NULL
 * A factorisation that fails follows jmid_eval_statistics: a scored step without a 2 x 2 Cholesky factor makes kde_nll NaN, ml_idx -1
 * and every *_ml column (the cut-offs' too) NaN; a cut-off step whose x or y coordinates have no variance makes that cut-off's kde NaN.
 * n_valid, fde_valid and valid tell "absent" from "NaN because scipy would have raised".
 * THIS PROJECT'S CONVENTIONS, where the reference raises instead of computing: its scene block fails with TypeError when a kept
 * agent has no fde and with IndexError when no agent is kept (and appends a stale min_fde_errors for an agent without fde, :592-612).
 * Here sfde runs over the kept agents whose last step is scored, sade over all kept agents, and a block without any qualifying agent
 * is NaN (three columns).
 * fp64 inside, fixed-order reductions, no atomics, as jmid_eval_statistics; with nothing masked and skip = NULL the first ten agent
 * columns and the scene row are bit-identical to that entry point's.  2 <= K <= 1024, T <= 24, any A (JMID_EINVAL beyond). */
int jmid_eval_statistics_masked(jmid_handle_t h, int E, int A, int K, int T, const float* pos, const float* gt,
                                const uint8_t* interp_future, const uint8_t* skip, int n_cut, const int* cutoffs, float* agent_out,
                                float* cut_out, float* scene_out, int mem);

/* Collision statistics of joint samples: how close the agents of one sampled future come to each other and which of them collide -
 * sicnav_diffusion/JMID/MID/models/collision_check_utils.py, whose counts DiffusionTraj.sample still returns as placeholders
 * (MID/models/diffusion.py:606-613).
 *   pos         [E, K, A, T, 2]  sampled futures (jmid_denoise's pos_out layout), or NULL: the positions of the most recent
 *                                jmid_denoise on this handle, under exactly the rules of jmid_topk's pos = NULL below.  Ground-truth
 *                                futures [E, A, T, 2] go through the same call as K = 1
 *   threshold   metres; a pair collides when its distance is < threshold in fp64 (the reference hard-codes 0.2, :88).  NaN never
 *               collides
 *   pair_out    [E, K, P], P = A (A - 1) / 2; may be NULL.  calc_min_dists (:58-80): every agent's path between consecutive horizon
 *               steps is a line segment, and a pair's value is the minimum over the T - 1 segments of the distance from the origin to
 *               the segment of the relative position pos_i - pos_j (lineseg_dist, :20-55: |a| when the relative position stands still,
 *               hypot(max(a.d, -b.d, 0), |(-a) x d|) with d the unit tangent otherwise).  Pairs in pdist order (get_diffs_pred, :5-17):
 *               p(i, j) = i A - i (i + 1) / 2 + (j - i - 1), i < j
 *   agent_out   [E, K, A] bytes; may be NULL.  1 = the agent belongs to a colliding pair (get_agents_in_collision, :83-97)
 *   sample_out  [E, K, 4] = {min_dist, closest_pair, n_pairs_colliding, n_agents_colliding}; may be NULL.  min_dist = the smallest pair
 *               value, closest_pair = its pair index as a float (the lowest index on an exact tie).  n_agents_colliding > 0 is
 *               check_collision_velocity (:100-108) of the sample
 *   scene_out   [E, 5] = {collision_rate, agent_collision_rate, min_dist_min, min_dist_mean, min_dist_std}; may be NULL.
 *               collision_rate = the share of the K samples with a collision, agent_collision_rate = the mean of the K A flags; min,
 *               mean and np.std (population) of min_dist over the samples
 * A = 1 has no pairs: min_dist = +inf, closest_pair = -1, counts and rates 0, min_dist_min = min_dist_mean = +inf, min_dist_std = NaN
 * (inf - inf, as np.std).  A non-finite position makes the pairs it belongs to NaN (torch.min / torch.max propagate it) and with them
 * the sample's min_dist (closest_pair = -1) and the episode's three min_dist columns; the counts and rates leave NaN pairs out.
 * T = 1 IS REFUSED: with a single step the reference collapses to one scalar over all pairs instead of one value per pair (:69-79),
 * which is not a per-pair quantity; duplicate the step (T = 2) for the static distance.
 * fp64 inside on the fp32 inputs, so the fp32 outputs are the roundings of the fp64 values; fixed-order reductions, no atomics: a row
 * is bit-identical whatever batch it is part of and in both memory modes.  1 <= K <= 1024, 2 <= T <= 24, 1 <= A <= 64, threshold
 * finite and >= 0, at least one output (JMID_EINVAL otherwise). */
int jmid_collision_statistics(jmid_handle_t h, int E, int A, int K, int T, const float* pos, double threshold,
                              float* pair_out, uint8_t* agent_out, float* sample_out, float* scene_out, int mem);

/* Wall statistics of joint samples: how close each agent's forecast path comes to every wall segment and which agents walk into one.
 * The predicate is the reference simulator's own: constrain_agent_action_exact (crowd_sim_plus/envs/crowd_sim_plus.py:885-893) takes an
 * agent's step as a line segment, and the step hits a wall when closest_distance_between_line_segments(wall, step) - radius < 0
 * (crowd_sim_plus/envs/utils/utils_plus.py:205-338).
 *   Walls     walls [L, 4] float64 {x1, y1, x2, y2}, 0 <= L <= 64: a HOST array in both memory modes, like episode_ids (the library
 *             keeps a device copy for the call).  crowd_env.static_obstacles(rule)[0].reshape(-1, 4) as it is.  A non-finite
 *             coordinate is JMID_EINVAL.  A zero-length wall is a point, handled as the reference handles it (:222-224: it goes through
 *             the parallel branch and yields the distance to the END of the step)
 *   Paths     agent a of sample (e, k) walks the segments pos[t-1] -> pos[t], t = 1 .. T-1.  With p0 [E, A, 2] (may be NULL) it walks
 *             p0 -> pos[0] first: T segments, in step order.  The step from the present position into the forecast is where a wall
 *             right next to a pedestrian is crossed
 *   Distance  d(a, l) = the minimum over the agent's segments of the reference's closest distance between wall l and the segment, in
 *             fp64 on the fp32 positions, with the reference's branches (segments shorter than 1e-8 are points; exactly parallel
 *             segments with the three sub-cases of :242-291; crossing lines with both clamps) - no other formula, so the conditioning
 *             near parallel segments is the reference's.  A segment with a non-finite end makes the agent's d(a, .) NaN (the minimum
 *             keeps a NaN)
 *   Hit       agent a hits wall l iff d(a, l) - radius < 0 in fp64; NaN never hits.  radius: a finite double >= 0
 *   pos         [E, K, A, T, 2], or NULL: the resident positions, under exactly the rules of jmid_collision_statistics
 *   dist_out    [E, K, A, L] d(a, l); may be NULL
 *   agent_out   [E, K, A] bytes, 1 = the agent hits some wall; may be NULL
 *   sample_out  [E, K, 3] = {min_clear, n_agents_hitting, n_hits}; may be NULL.  min_clear = the smallest d of the sample (a NaN decides
 *               it), n_hits = the number of (agent, wall) pairs that hit
 *   scene_out   [E, 5] = {wall_hit_rate, agent_wall_hit_rate, min_clear_min, min_clear_mean, min_clear_std}; may be NULL.  The
 *               definitions of jmid_collision_statistics' scene row with "hits a wall" for "collides"
 * L = 0: min_clear = +inf, counts and rates 0, min_clear_std NaN (what jmid_collision_statistics gives for A = 1).
 * There is no "nearest wall" index: walls share corner points and a path may cross two walls (a crossing's distance is a cancellation of
 * about 1e-17), so the index would be decided by rounding; take the argmin of dist_out where it is wanted.
 * fp64 inside, fixed-order reductions, no atomics: a row is bit-identical whatever batch it is part of and in both memory modes.
 * 1 <= K <= 1024, 2 <= T <= 24, 1 <= A <= 64, 0 <= L <= 64, at least one output (JMID_EINVAL otherwise). */
int jmid_wall_statistics(jmid_handle_t h, int E, int A, int K, int T, const float* pos, const float* p0, int L, const double* walls,
                         double radius, float* dist_out, uint8_t* agent_out, float* sample_out, float* scene_out, int mem);

/* Joint-KDE ranking of the K sampled futures of every episode and selection of the k most likely ones:
 * get_most_likely_samples (sicnav_diffusion/JMID/mid_sim_wrapper.py:14-169, the joint branch :20-21 the predictor always takes;
 * called from predict_ret_best when num_ret_samples < K, :487-492), which the reference runs on its GPU when it has one (:26-30).
 *   pos   [E, K, A, T, 2]  integrated sample trajectories (jmid_denoise's pos_out layout), or NULL: the positions of the most
 *                          recent jmid_denoise on this handle (same E, A, K, T, called with p0) - the samples then never leave
 *                          the GPU.  They are forgotten (JMID_EINVAL here) when that call returned JMID_ERANGE and by any later
 *                          host-mode jmid_encode / jmid_episode_metrics or denoise call on the handle, which reuse the workspace
 *   bw    [T] KDE bandwidth per horizon step, exp(linspace(ln .01, ln .1, T)) as the reference computes it (:26-30), or NULL
 *                          (computed in the library)
 *   sel   [E, A, k, T, 2]  the kept samples in ascending likelihood (the reference's argsort(...)[-k:], :117-121)
 *   logw  [E, A, k]        their renormalised log-weights, the same row for every agent (:139-151)
 * fp64 inside (A <= 32, K <= 1024, T <= 24: JMID_EINVAL beyond); exact ties are broken by sample index (torch.argsort's tie
 * order is not reproduced); non-finite totals rank lowest. */
int jmid_topk(jmid_handle_t h, int E, int A, int K, int T, int k, const float* pos, const float* bw, float* sel, float* logw,
              int mem);

/* One predictor call end to end, host buffers in, host buffers out: what HumanTrajectoryForecasterSim.predict_ret_best issues per
 * MPC step (sicnav_diffusion/JMID/mid_sim_wrapper.py:482-510 -> MID.eval_sicnav, MID/mid.py:298-349) - jmid_encode, jmid_denoise
 * and, when k < K, jmid_topk chained on the handle's stream with ONE upload (a pinned staging buffer), no host round trip between
 * the stages (the context and the K sampled futures never leave the GPU) and ONE download + synchronisation at the end.
 *   x_st [E*A, hist_len, 6], nbr_sum [E*A, 2, hist_len, 6], edge_mask [E*A, 2]   as jmid_encode
 *   x_T [E, K*A, T, 2], p0 [E, A, 2], dt, precision                              as jmid_denoise
 *   k < K:  bw [T] as jmid_topk (or NULL); sel [E, A, k, T, 2] and logw [E, A, k] receive the k most likely futures; pos_out may
 *           be NULL
 *   k == K: no ranking (the reference skips it, mid_sim_wrapper.py:487-492); pos_out [E, K, A, T, 2] receives all futures, sel /
 *           logw / bw are ignored
 * Returns JMID_ERANGE like jmid_denoise (the outputs are then undefined: repeat the stages in JMID_PREC_F32). */
int jmid_predict(jmid_handle_t h, int E, int A, int K, int T, int k, const float* x_st, const float* nbr_sum, const float* edge_mask,
                 const float* x_T, const float* p0, float dt, int precision, const float* bw, float* sel, float* logw, float* pos_out);

/* Padded scene batches: ONE call for episodes of different agent counts.  Every array keeps the uniform layout of the plain entry with
 * A - the largest count of the batch - as the row stride, plus
 *   n_agents  [E] int32, HOST array in both memory modes, 1 <= n_agents[e] <= A: episode e has n_agents[e] real agents, a < n_agents[e]
 * Row s*A + a of an episode is real iff a < n_agents[e]; the other rows are padding.  The semantics are the reference's attn_mask
 * (JointPredictionTransformerConcatLinear.forward(..., mask), MID/models/diffusion.py:186-195, built in
 * MID/dataset/preprocessing.py:36-89): joint attention is block-diagonal over episodes and the tokens of padded agents are excluded as
 * keys, so the real rows of episode e are what the plain entry computes for that episode alone at A = n_agents[e] (up to the rounding
 * of a sum taken in another order; an episode with n_agents[e] == A keeps the plain call's bits under the rule of
 * jmid_set_chunk_episodes).  Attention is the only operation that couples rows: an iMID handle accepts the same calls and needs no mask.
 *   - what the caller leaves in the padded rows of x / x_T, ctx and p0 is never read (the library works on zeroed copies), NaN included,
 *     and cannot raise JMID_ERANGE;
 *   - the padded rows of every returned array are quiet NaN - e_out, vel_out, pos_out, sel, logw, and the positions left resident for
 *     pos = NULL: a consumer that forgets n_agents sees it at once;
 *   - jmid_topk_padded ranks episode e in 2 * n_agents[e] dimensions over its real agents (pos = NULL: as jmid_topk, after
 *     jmid_denoise_padded of the same shape);
 *   - chunking, chunk lanes and the split-KV factor follow E, A, K, T exactly as for the plain call; the padded share of the rows
 *     is computed and thrown away.
 * DDIM only: there is no padded form of jmid_denoise_ddpm.  The entries above take the caller's x_T; the seeded forms
 * (jmid_noise_fill_padded, jmid_denoise_padded_seeded) and the padded chains on the resident scene (jmid_predict_scene_padded,
 * jmid_forecast_scene_padded and their seeded forms) stand with "Seeded noise" and "Padded chains on the resident scene" below;
 * jmid_predict_scene / jmid_forecast_scene themselves keep JMID_EINVAL on mixed counts.  JMID_EINVAL for NULL n_agents, a count outside 1..A,
 * a DDPM table on the handle, and (diagnostics flavour) for the attention A/B knobs that have no masked kernel: "attn_sm" = 2 in every
 * split mode, "attn_mx" = 1 and "attn_pf" = 2 in JMID_PREC_F16X2 / F16MX.  Everything else as the plain entry of the same name. */
int jmid_net_eval_padded(jmid_handle_t h, int E, int A, int K, int T, const int32_t* n_agents, int step_idx, const float* x, const float* ctx,
                         int precision, float* e_out, int mem);
int jmid_denoise_padded(jmid_handle_t h, int E, int A, int K, int T, const int32_t* n_agents, const float* x_T, const float* ctx, const float* p0,
                        float dt, int precision, float* vel_out, float* pos_out, int mem);
int jmid_topk_padded(jmid_handle_t h, int E, int A, int K, int T, int k, const int32_t* n_agents, const float* pos, const float* bw, float* sel,
                     float* logw, int mem);
int jmid_predict_padded(jmid_handle_t h, int E, int A, int K, int T, int k, const int32_t* n_agents, const float* x_st, const float* nbr_sum,
                        const float* edge_mask, const float* x_T, const float* p0, float dt, int precision, const float* bw, float* sel,
                        float* logw, float* pos_out);

/* Collision and wall statistics of a padded batch: jmid_collision_statistics / jmid_wall_statistics that know which agents are real.
 * (The plain entries have no such notion: fed a padded call's positions, the NaN rows make every sample's min_dist / min_clear NaN.)
 * n_agents as above; every output keeps the plain entry's shape at A.
 *   pair_out    [E, K, P_A] in pdist order at A.  A pair with a padded agent is quiet NaN and takes part in NOTHING - not in min_dist,
 *               closest_pair or the counts (in the plain entry a NaN pair decides the minimum).  A non-finite position of a REAL agent
 *               propagates exactly as in the plain entry
 *   dist_out    [E, K, A, L]: quiet NaN in a padded agent's row; that agent is left out of min_clear, n_agents_hitting and n_hits
 *   agent_out   a padded agent's byte is 0 (a byte has no NaN: read it with n_agents at hand)
 *   sample_out  closest_pair is the pair's index at A.  n_agents[e] = 1 behaves as A = 1 does in the plain entry: min_dist +inf,
 *               closest_pair -1, counts 0
 *   scene_out   agent_collision_rate / agent_wall_hit_rate divide by K * n_agents[e]; everything else as the plain row
 *   pos, p0     padded rows are never read (NaN, 1e30, anything).  pos = NULL: the resident positions after a padded denoise call of
 *               the same shape (jmid_denoise_padded, jmid_denoise_padded_seeded, jmid_denoise_reject_padded_seeded), under the rule of
 *               jmid_topk_padded
 * THE EQUALITY that defines them: every value of episode e is bit for bit what the plain entry gives for that episode's compacted
 * [1, K, n_e, T, 2] block (and [1, n_e, 2] p0), with pair (i, j) at p_A(i, j) instead of p_{n_e}(i, j).  The index map is monotone, so
 * "the lowest index on an exact tie" carries over.  It holds by construction, not by measurement: a workgroup is one (episode, sample)
 * and walks the real pairs / (agent, wall) couples of the compacted episode in the plain kernel's order; the minimum is a total order;
 * the counts are exact integer sums in fp64; the sums over the K samples keep their order.
 * JMID_EINVAL: NULL n_agents, a count outside 1..A, and the plain entry's refusals. */
int jmid_collision_statistics_padded(jmid_handle_t h, int E, int A, int K, int T, const int32_t* n_agents, const float* pos, double threshold,
                                     float* pair_out, uint8_t* agent_out, float* sample_out, float* scene_out, int mem);
int jmid_wall_statistics_padded(jmid_handle_t h, int E, int A, int K, int T, const int32_t* n_agents, const float* pos, const float* p0, int L,
                                const double* walls, double radius, float* dist_out, uint8_t* agent_out, float* sample_out, float* scene_out,
                                int mem);

/* The scene batch on the device: track positions on the time_step grid in, the encoder's inputs left resident on the handle - what the
 * reference does between update_state_hists and Trajectron.get_latent (mid_sim_wrapper.py:313-437, MID/dataset/preprocessing.py:428-620,
 * MID/environment/scene_graph.py:111-250, the neighbour reductions of MID/models/encoders/mgcvae.py:726-768) for E independent episodes.
 * With this entry a C caller goes from positions to forecasts: build -> draw x_T [E, K * n_in, T, 2] -> jmid_predict_scene, or without a
 * generator of its own: build -> jmid_predict_scene_seeded (the library draws x_T from its counter generator, "Seeded noise" below).
 *   human_xy  [E, F, N, 2] doubles  pedestrian positions, oldest frame first; F = the handle's hist_len (>= 3), 1 <= N <= 63
 *   robot_xy  [E, F, 2] doubles     robot positions on the same frames
 *   time_step the grid spacing in seconds (velocities and accelerations are first differences divided by it)
 *   force_all_in_cluster  0: the reference's choice - the pedestrians within 3 m (at the last frame) of the pedestrian whose cluster mean
 *             lies nearest the robot go through the network; non-zero: every pedestrian (and the robot) does
 *   in_cluster_out        [E, N] bytes, 1 = the pedestrian is in the chosen cluster
 *   robot_in_cluster_out  [E] bytes
 *   n_in_out  [E] ints    pedestrians in the cluster: the A of the jmid_predict_scene call, and what sizes its x_T
 *   cv_out    [E, N, horizon, 2] doubles or NULL: the constant-velocity forecasts of EVERY pedestrian - what the reference returns for the
 *             ones outside the cluster (mid_sim_wrapper.py:413-429); 1 <= horizon <= 24 (horizon is ignored when cv_out is NULL)
 * Left on the handle, in the padded layout that gives every pedestrian a row (jmid_scene_get copies them out): x and x_st [E, N, F, 6],
 * nbr_sum [E, N, 2, F, 6], edge_mask [E, N, 2], p0 [E, N, 2], all fp32.  A row outside the cluster is computed as a node without neighbours.
 * The edge mask of a row is min(sum of its edge scaling values, 1) for BOTH edge types: the reference does not filter the edge values by
 * type (scene_graph.py:293-299), reproduced.
 * fp64 wherever the reference computes in float64, fp32 exactly where it casts, the neighbour sums in node order, no FMA contraction: the
 * rows are bit-identical to the reference's batch tensors.  The one freedom is the cluster means: the members are summed in ascending
 * track id here and by a BLAS product there, so a scene whose two best clusters of DIFFERENT membership lie within rounding of the same
 * distance from the robot may choose the other one.
 * The call synchronises (the caller needs n_in to draw x_T).  The scene stays resident until the next jmid_build_scene on the handle; no
 * other entry point touches it.  JMID_EINVAL (the resident scene, if any, is kept): F != hist_len, F < 3, N < 1, N > 63, horizon outside
 * 1..24 with cv_out, time_step not finite and positive. */
int jmid_build_scene(jmid_handle_t h, int E, int N, int F, const double* human_xy, const double* robot_xy, double time_step, int horizon,
                     int force_all_in_cluster, uint8_t* in_cluster_out, uint8_t* robot_in_cluster_out, int* n_in_out, double* cv_out, int mem);

/* Copies of the arrays jmid_build_scene left on the handle, in its padded layout: x, x_st [E, N, F, 6], nbr_sum [E, N, 2, F, 6],
 * edge_mask [E, N, 2], p0 [E, N, 2].  NULL arguments are skipped.  JMID_EINVAL without a preceding jmid_build_scene. */
int jmid_scene_get(jmid_handle_t h, float* x, float* x_st, float* nbr_sum, float* edge_mask, float* p0, int mem);

/* jmid_build_scene for tracks seen for fewer than F frames (an episode's first control steps, a pedestrian entering sensor range):
 *   first_frame  [E, N + 1] int32, robot first then the pedestrians by id; a HOST array in both memory modes; NULL: all zero, and then
 *                every resident array has the bits jmid_build_scene leaves
 * Node j is present on frames first_frame[j] .. F-1, without gaps; its positions in front of that are never read and may be NaN.
 *   - velocity and acceleration are first differences over the node's own span (MID/environment/data_utils.py:24-37; one frame: zero);
 *     x and x_st are NaN in front of it
 *   - the scene graph has no adjacency on a frame where either node is absent (MID/environment/scene.py:84-106)
 *   - a connected neighbour is taken with padding 0.0 and THEN standardised relative to the ego (preprocessing.py:531-550): on a frame
 *     where it is absent it adds (0 - ego_now) / std in all six columns, so nbr_sum is finite on all F frames.  The reference's quirk.
 *   - a pedestrian with ONE frame is never an ego row: in_cluster_out 0 and not counted in n_in_out, its cv_out row its position repeated;
 *     it still counts in the cluster choice and as a neighbour
 * Additionally resident: first_index [E, N] int32 (jmid_scene_get_first_index); jmid_predict_scene, jmid_forecast_scene and their seeded
 * forms gather it with the rows and run the encoder as jmid_encode_var does.  A scene built by jmid_build_scene or
 * jmid_build_scene_stamped has none and runs the launches it always ran.
 * JMID_EINVAL (the resident scene is kept): a first_frame outside 0..F-1, a robot with fewer than 2 frames while force_all_in_cluster is
 * 0, and every refusal of jmid_build_scene.
 * Raw-stamp input, with gaps inside a track's span interpolated: jmid_build_scene_stamped_var (jmid_build_scene_stamped still ends in
 * JMID_EHISTORY below hist_len grid frames).  A track that ends before the last frame: jmid_build_scene_absent (left out), or coasted
 * from raw frames by jmid_build_scene_stamped_coast.  This entry keeps refusing a negative first_frame. */
int jmid_build_scene_var(jmid_handle_t h, int E, int N, int F, const double* human_xy, const double* robot_xy, const int32_t* first_frame,
                         double time_step, int horizon, int force_all_in_cluster, uint8_t* in_cluster_out, uint8_t* robot_in_cluster_out,
                         int* n_in_out, double* cv_out, int mem);

/* jmid_build_scene_var for episodes in which some pedestrians are NOT IN THE SCENE: the same arguments, and first_frame[e, 1 + j] may be -1
 * (never the robot's entry).  "Not there" is the reference's own treatment of a node without data at the current frame (edge scaling is
 * zero where not adjacent now, a NaN distance is not <= radius, present_nodes does not list it), so pedestrian j of episode e
 *   - is never read (his positions may be anything), is no candidate of the cluster choice and no member of a cluster mean,
 *   - is no graph node, nobody's neighbour and no ego row: in_cluster_out 0, not counted in n_in_out,
 *   - has NaN in every float row of his: x, x_st, nbr_sum, edge_mask, p0 (jmid_scene_get), cv_out; first_index -1,
 *   - gets NaN forecast rows (the prepended pose included) and a NaN log-weight row from jmid_forecast_scene and its forms,
 * and every output of every other track is bit for bit what jmid_build_scene_var leaves for the episode with his column removed - so a
 * batch whose episodes see different pedestrians keeps ONE N.  Every chained entry works on the scene unchanged.  Without a -1 every
 * byte is jmid_build_scene_var's.  JMID_EINVAL (the resident scene is kept): an episode in which every pedestrian is -1
 * (jmid_last_error names it), a NULL first_frame, and every refusal of jmid_build_scene_var. */
int jmid_build_scene_absent(jmid_handle_t h, int E, int N, int F, const double* human_xy, const double* robot_xy, const int32_t* first_frame,
                            double time_step, int horizon, int force_all_in_cluster, uint8_t* in_cluster_out, uint8_t* robot_in_cluster_out,
                            int* n_in_out, double* cv_out, int mem);

/* first_index [E, N] int32 of the resident scene, in its padded layout (all zero after a build without first_frame; -1: a pedestrian
 * who is not in the scene, jmid_build_scene_absent).  JMID_EINVAL without a resident scene. */
int jmid_scene_get_first_index(jmid_handle_t h, int32_t* out, int mem);

/* jmid_predict on the resident scene: the in-cluster rows are gathered on the device in ascending track id, then encoder -> denoise loop ->
 * integrator -> top-k run chained on the stream exactly as in jmid_predict (the same kernels on the same values: the outputs are
 * bit-identical to jmid_predict fed those rows).  Host buffers: x_T [E, K*A, T, 2], bw / sel / logw / pos_out as jmid_predict.
 * JMID_EINVAL when no scene is resident, when E differs from the build's, or when any episode's in-cluster count is not A (group the
 * episodes of a batch by their count, one jmid_build_scene + jmid_predict_scene per group); otherwise the limits and status codes of
 * jmid_predict, JMID_ERANGE and JMID_ETIMEOUT included (the scene stays resident: jmid_scene_get feeds the staged repeat). */
int jmid_predict_scene(jmid_handle_t h, int E, int A, int K, int T, int k, const float* x_T, float dt, int precision, const float* bw,
                       float* sel, float* logw, float* pos_out);

/* jmid_build_scene from raw stamped frames: the history frame table of predict_ret_best (mid_sim_wrapper.py:244-298: dropna, the stable sort
 * by stamp, subsample_df's trunc(stamp * 100) bins of round(time_step * 100) anchored at the LAST stamp, the last row per bin, linear
 * interpolation of empty bins, the cut to past_num_frames) on the device, then exactly what jmid_build_scene does with the resulting grid.
 * For histories in which every human and the robot share the stamps of a frame - what update_state_hists (:198-204) produces.
 *   stamps    [E, R] doubles          the stamp of each raw frame, oldest-PUSHED first (they need not be sorted); 1 <= R <= 64
 *   human_xy  [E, R, N, 2] doubles    pedestrian positions per raw frame, 1 <= N <= 63
 *   robot_xy  [E, R, 2] doubles
 *   n_frames  [E] ints or NULL        the first n_frames[e] (1..R) raw frames of episode e are valid; NULL: all R of every episode
 *   n_grid_out [E] ints               frames on the grid per episode, min(hist_len, bins between the oldest kept and the newest stamp)
 *   everything else as jmid_build_scene (F is the handle's hist_len)
 * A frame with a NaN stamp or coordinate is dropped; equal stamps keep push order and the later one wins its bin; an empty bin is
 * interpolated in fp64 as np.interp does (slope = (y1 - y0) / (x1 - x0); y = slope * (x - x0) + y0, no FMA) between the last frames of the
 * nearest filled bins on either side - the older one may lie any number of bins back: only the hist_len newest bins are ever produced.
 * pose_now (what predict_ret_best prepends, :444-454) is the LAST PUSHED valid frame, before anything is dropped (agent_df.tail(1)).
 * The grid is bit-identical to the reference's frame table, so the resident arrays are jmid_build_scene's on that grid.
 * Synchronises like jmid_build_scene.  JMID_EHISTORY when an episode has fewer than hist_len grid frames: n_grid_out is filled and the
 * previously resident scene, if any, is kept.  JMID_EINVAL (the resident scene is kept): R outside 1..64, an n_frames[e] outside 1..R,
 * time_step not finite or round(time_step * 100) < 1, and every refusal of jmid_build_scene. */
int jmid_build_scene_stamped(jmid_handle_t h, int E, int N, int R, const double* stamps, const double* human_xy, const double* robot_xy,
                             const int* n_frames, double time_step, int horizon, int force_all_in_cluster, uint8_t* in_cluster_out,
                             uint8_t* robot_in_cluster_out, int* n_in_out, int* n_grid_out, double* cv_out, int mem);

/* jmid_build_scene_stamped with a history window PER TRACK: a NaN coordinate of pedestrian j in a raw frame means "track j was not seen in
 * this frame" and drops nothing, and a window shorter than hist_len is built, not refused.  The arguments of jmid_build_scene_stamped and
 *   first_frame_out [E, N + 1] int32 or NULL   robot first, the first_frame of jmid_build_scene_var as derived from the raw frames
 * One definition, shared with scene.py::frame_table_tracks (fp64, no FMA, the association of jmid_build_scene_stamped):
 *   1. pose_now = the human positions of the last PUSHED valid frame (NaN for a track not seen there)
 *   2. a frame is dropped iff its stamp or a robot coordinate is NaN
 *   3. the kept frames, in stable sort order by stamp, share one grid: ns = trunc(stamp * 100), w = round(time_step * 100), bin
 *      b = floor((ns_last - ns) / w) counted back from the newest kept frame (the ANCHOR), nb = max(b) + 1, n_grid = min(hist_len, nb).
 *      The robot's column is jmid_build_scene_stamped's.
 *   4. pedestrian j's frames are the kept ones where both its coordinates are non-NaN.  A bin holds the last sorted of them; an empty bin
 *      between filled ones is interpolated between the nearest filled older and newer bin OF THAT TRACK in index space x = nb-1-b;
 *      nothing is extrapolated in front of its oldest filled bin b_old(j), which may lie beyond the window.
 *   5. the grid is right-aligned in hist_len rows, NaN in front, the newest frame in row hist_len-1 (jmid_scene_get_frames returns it so);
 *      first_frame = hist_len - n_grid for the robot and hist_len-1 - min(b_old(j), n_grid-1) for pedestrian j - a pedestrian seen only in
 *      the anchor frame is a graph node and no ego row, as jmid_build_scene_var has it.
 * Then exactly jmid_build_scene_var on that grid and first_frame: first_index is resident, and jmid_predict_scene, jmid_forecast_scene, their
 * _seeded and _padded forms, jmid_scene_get* and jmid_scene_get_frames work on the scene unchanged.  Without a human NaN and with
 * n_grid = hist_len every resident array has the bits jmid_build_scene_stamped leaves.
 * n_grid_out and first_frame_out are filled before either refusal below, and the previously resident scene, if any, is kept:
 *   JMID_EHISTORY  an episode has n_grid < 2
 *   JMID_EINVAL    a pedestrian is not seen in the anchor frame (first_frame_out -1; jmid_last_error names the episode and the track): the
 *                  resident scene cannot hold a node that is absent now - leave the track out of the call, as for an empty cluster;
 *                  and every refusal of jmid_build_scene_stamped.
 * A pedestrian who is not seen now, left out or coasted instead of refused: jmid_build_scene_stamped_coast. */
int jmid_build_scene_stamped_var(jmid_handle_t h, int E, int N, int R, const double* stamps, const double* human_xy, const double* robot_xy,
                                 const int* n_frames, double time_step, int horizon, int force_all_in_cluster, uint8_t* in_cluster_out,
                                 uint8_t* robot_in_cluster_out, int* n_in_out, int* n_grid_out, double* cv_out, int32_t* first_frame_out,
                                 int mem);

/* jmid_build_scene_stamped_var that never refuses a pedestrian who is not seen in the anchor frame: he is COASTED to it or LEFT OUT of the
 * scene (jmid_build_scene_absent's -1).  The arguments of jmid_build_scene_stamped_var and
 *   max_coast  0 .. hist_len-2   the bins a track may be extrapolated over; 0: leave out whoever is not seen in the anchor's bin
 *   coast_out  [E, N] int32 or NULL   0: seen in the anchor frame; b_new > 0: coasted over b_new bins; -1: left out
 * One definition, shared with scene.py::frame_table_tracks(max_coast=) (fp64, no FMA).  b_new(j) is pedestrian j's newest filled bin:
 *   - seen in the anchor frame: everything as jmid_build_scene_stamped_var has it, coast 0
 *   - no filled bin, b_new > max_coast or b_new > n_grid-1: left out - first_frame -1, his column and pose_now NaN, coast -1
 *   - otherwise coasted: the bins b >= b_new of his column by rule 4 of jmid_build_scene_stamped_var; the bins b < b_new are
 *     y(b) = y(b_new) + (double)(b_new - b) * step with step = y(b_new) - y(b_new + 1) when the grid row b_new + 1 exists in his window
 *     (b_new + 1 <= min(b_old, n_grid-1); real or interpolated) and 0 otherwise (one observation: the position repeated);
 *     first_frame by the formula of rule 5, pose_now = y(0), coast = b_new (0: seen in the anchor's bin, not in the anchor frame)
 * Then exactly jmid_build_scene_absent on that grid and first_frame.  A coasted pedestrian is an ordinary node: a network forecast when
 * he is in the cluster with two grid rows, his constant-velocity row otherwise, his coasted pose prepended.  When the anchor frame
 * sees everybody every byte is jmid_build_scene_stamped_var's.
 * n_grid_out, first_frame_out and coast_out are filled before the refusals that follow the kernel; the resident scene is kept by all:
 *   JMID_EHISTORY  an episode has n_grid < 2
 *   JMID_EINVAL    max_coast outside 0..hist_len-2 (nothing is filled); an episode with nobody left (jmid_last_error names it); and every
 *                  refusal of jmid_build_scene_stamped. */
int jmid_build_scene_stamped_coast(jmid_handle_t h, int E, int N, int R, const double* stamps, const double* human_xy, const double* robot_xy,
                                   const int* n_frames, double time_step, int horizon, int force_all_in_cluster, uint8_t* in_cluster_out,
                                   uint8_t* robot_in_cluster_out, int* n_in_out, int* n_grid_out, double* cv_out, int32_t* first_frame_out,
                                   int max_coast, int32_t* coast_out, int mem);

/* The grid the resident scene was built from and its pose_now, as doubles: human_xy [E, F, N, 2], robot_xy [E, F, 2] (the frame table of
 * mid_sim_wrapper.py:244-298 after jmid_build_scene_stamped; the caller's own input after a plain jmid_build_scene) and pose_now [E, N, 2]
 * (:444-454; after a plain jmid_build_scene the last frame of the grid).  NULL arguments are skipped.  JMID_EINVAL without a resident scene. */
int jmid_scene_get_frames(jmid_handle_t h, double* human_xy_out, double* robot_xy_out, double* pose_now_out, int mem);

/* jmid_predict_scene followed by the result assembly of predict_ret_best (mid_sim_wrapper.py:493-510, :444-454) on the stream, with one
 * download: exactly the two arrays HumanTrajectoryForecasterSim.predict_ret_best returns, for E episodes.
 *   forecasts_out [E, N, k, T+1, 2] doubles   step 0 = pose_now; an in-cluster pedestrian (rank by ascending track id) gets its k kept
 *                 futures (k == K: all K samples in sample order), fp32 widened exactly; a pedestrian outside the cluster its
 *                 constant-velocity row (:413-429) for every sample
 *   logw_out      [E, N, k] doubles           k < K: the renormalised log-weights of the kept samples (the same row for everybody, :139-151);
 *                 k == K: log(1 / K) (:498)
 * Host buffers.  All limits and status codes of jmid_predict_scene (one A per call: group the episodes by their count); JMID_EINVAL also
 * when the resident scene was built without cv_out, or with a horizon other than T. */
int jmid_forecast_scene(jmid_handle_t h, int E, int A, int K, int T, int k, const float* x_T, float dt, int precision, const float* bw,
                        double* forecasts_out, double* logw_out);

/* ---- Seeded noise: x_T and the DDPM z from a counter generator on the device ----------------------------------------------------
 * OPT-IN, and statistically - NOT seed- - compatible with the reference: the reference draws x_T from torch's CPU generator and its
 * per-step z from the generator of the device it runs on (MID/models/diffusion.py:499, 509), and the explicit-noise entries above keep
 * that contract (the host draws, the library consumes).  The ADE gate of this project stays defined on identical x_T through those
 * entries.  The entries below draw from the library's own generator instead, so that a C caller needs no Gaussian generator, a DDPM
 * call uploads no [n_steps, ...] tensor, and an episode's noise is a pure function of its address - identical for every batch size,
 * count group, chunk plan, lane and rank.  No generator state lives on the handle.
 *
 * Generator: Philox4x32-10 (Salmon, Moraes, Dror, Shaw, SC'11): multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 /
 * 0xBB67AE85, ten rounds.  Known answer: counter (0, 0, 0, 0), key (0, 0) -> 6627e8d5 e169c58d bc57ac4c 9b00dbd8.
 * Addressing:
 *   key     = (seed & 0xffffffff, seed >> 32)
 *   counter = (q, episode_id, draw, 0)
 *     episode_id  the caller's GLOBAL episode number (uint32): in a sharded sweep the number of the episode in the whole sweep, not
 *                 its position in the call
 *     draw        0 = x_T; i + 1 = the z of step-table entry i (entries whose use_noise is 0 keep their number: nothing is drawn
 *                 for them, and the numbers of the others do not move)
 *     q           idx / 4, idx = (r * T + t) * 2 + c the row-major element index inside the episode's [rows, T, 2] tensor (rows = K * A
 *                 in the row order of this header); q must fit 32 bits
 *     the fourth counter word is reserved and always 0
 *   The four output words of block q belong to the elements 4q .. 4q + 3; the last block of an episode may be partly used.
 * Normals: Box-Muller per word pair - (w0, w1) gives the elements 4q and 4q + 1, (w2, w3) the elements 4q + 2 and 4q + 3 - evaluated
 * in fp64 and rounded once to fp32: for a pair (a, b)
 *   u1 = (a + 1) * 2^-32,  u2 = b * 2^-32,  r = sqrt(-2 ln u1),  values (r cos(2 pi u2), r sin(2 pi u2))
 * with 2 pi the fp64 constant 6.283185307179586 multiplied in one rounding, no fast-math and no FMA contraction.  |z| <= 6.67 by
 * construction.  noise.py restates all of it in NumPy; the two agree to the bit except where the fp64 value lies within the math
 * libraries' last-place difference of an fp32 rounding boundary (about 1e-8 of the values, one fp32 ulp there).
 * episode_ids [E] is a HOST array in both memory modes (like the cut-offs of jmid_eval_statistics_masked); the library keeps a
 * device copy for the duration of the call.
 *
 * jmid_noise_fill: one draw for E episodes, out [E, rows, T, 2] (where `mem` says).  JMID_EINVAL: E < 1, rows < 1, T < 1, draw < 0,
 * NULL episode_ids, NULL out. */
int jmid_noise_fill(jmid_handle_t h, uint64_t seed, int E, int rows, int T, const uint32_t* episode_ids, int draw, float* out, int mem);

/* jmid_denoise or jmid_denoise_ddpm - whichever step table is installed - with the noise drawn by the library: x_T is draw 0, filled
 * straight into the workspace; under DDPM the z of step-table entry i is draw i + 1, filled on the chunk's own stream just before that
 * step's update into a one-step buffer per lane - no [n_steps, ...] buffer exists anywhere.  The update kernels are the ones of the
 * explicit entries (they receive a pointer): the outputs are bit-identical to jmid_denoise / jmid_denoise_ddpm fed the same draws from
 * jmid_noise_fill.  Same limits and status codes as those entries, JMID_ERANGE and JMID_ETIMEOUT included; the positions stay in the
 * workspace for jmid_topk(pos = NULL) and the statistics entries exactly as after jmid_denoise.  JMID_EINVAL for NULL episode_ids.
 * Captured loop ("graph" knob): the x_T fill is an input stage and lies outside the captured loop like the copies of the explicit
 * entry, and a DDPM loop is never captured - a seeded call gives the same bits with and without capture, and a replay needs no
 * re-instantiation for a new seed or new ids. */
int jmid_denoise_seeded(jmid_handle_t h, int E, int A, int K, int T, uint64_t seed, const uint32_t* episode_ids, const float* ctx,
                        const float* p0, float dt, int precision, float* vel_out, float* pos_out, int mem);

/* Collision-free sampling: jmid_denoise_seeded that redraws joint samples in which two agents collide.  OFF unless this entry is called.
 * DiffusionTraj.sample (MID/models/diffusion.py:544-613) takes with_constraints / constraint_type / dynamics and returns (samples,
 * number_of_steps, num_iter, total_num_samples_with_collisions, total_num_samples_with_collisions_fixed); MID/mid.py:404-407, 492-498,
 * 908-954, 1048 accumulate and print the counts ("Rejection sampling fixed X samples out of Y samples with collisions").  The reference's
 * loop body is gone and its counts are hard-coded zeros; its predicate is check_collision_velocity (MID/models/collision_check_utils.py:
 * 100-108).  THE RULE, decided here:
 *   In JMID the K samples of an episode are ONE attention sequence (diffusion.py:196-204; jmid_denoise above), so a single sample cannot be
 *   redrawn alone without changing what it attends to: a redraw is a whole episode, all K samples afresh.  With K = 1 this is the
 *   reference's offline per-sample loop.
 *   Predicate: a candidate joint sample [A, T, 2] is ACCEPTABLE iff its n_agents_colliding column of jmid_collision_statistics is 0 at
 *   `threshold` AND its min_dist column is not NaN (A = 1: +inf, acceptable).  fp64, that entry's own kernel.  The reference's 0.2 is the
 *   Python default.
 *   Round 0: the candidates c_0[s] are the K samples of draw number draw0; slot s holds c_0[s]; bad = the slots whose candidate is not
 *   acceptable.
 *   Round j = 1 .. max_rounds: only the episodes with a non-empty bad set are rerun - their K samples are denoised again from the x_T of
 *   draw number draw0 + j (episode id, seed and element addressing of "Seeded noise" above); good_j = the ascending list of the acceptable
 *   candidate indices; the i-th smallest slot of bad receives the i-th smallest candidate of good_j, i < min(|bad|, |good_j|), positions
 *   and velocities both; filled slots leave bad; unused candidates are discarded.
 *   End: a slot that never got an acceptable candidate keeps its round-0 sample and stays flagged.  Slots acceptable at round 0 and slots
 *   never fixed are bit for bit the plain seeded call's samples; max_rounds = 0 is the plain call plus the flags.
 * Every output of an episode is a function of (weights, ctx, p0, seed, episode id, draw0, threshold, max_rounds) only - not of its batch
 * mates, its shard or the chunk plan - on top of the rule for calls of different episode counts at jmid_set_chunk_episodes (bit-identical
 * at head_dim 16, equal to rounding at head_dim 128).  Two equalities:
 *   - draw0 = 0, max_rounds = 0 is bit-identical to jmid_denoise_seeded;
 *   - round j's candidates are bit-identical to jmid_noise_fill(draw = draw0 + j) + jmid_denoise on the gathered ctx / p0 rows of exactly
 *     the rerun episodes, in ascending order, as ONE call.
 *   ctx [E, A, ctx_dim], p0 [E, A, 2] (required: the predicate is defined on positions), episode_ids [E] a HOST array
 *   vel_out, pos_out  [E, K, A, T, 2]; may be NULL
 *   slot_out    [E, K, 3] int32 = {round whose draw the slot holds (0 .. max_rounds), candidate index within that round, 1 if the slot's
 *               sample is not acceptable}; may be NULL
 *   episode_out [E, 3] int32 = {slots not acceptable at round 0, slots fixed, last round in which the episode was rerun (0 = never)};
 *               may be NULL
 * Every kernel of the loop runs in a fixed order without atomics.  The host reads ONE small download per round (how many episodes the next
 * round reruns, which, and the round's range flag): the loop's inherent synchronisation, the rerun's launch dimensions depend on it.  A
 * rerun is a seeded denoise call of E' episodes through the same planner, the denoise kernels are untouched, and the captured loop ("graph")
 * gives the same bits on and off.
 * After the call the ACCEPTED set is what pos = NULL means for jmid_topk, jmid_eval_statistics, jmid_eval_statistics_masked and
 * jmid_collision_statistics, at (E, A, K, T), forgotten exactly as after jmid_denoise.
 * DDIM only (JMID_EINVAL under a DDPM table: its draws 1.. are the steps' z); uniform agent count only (mixed counts:
 * jmid_denoise_reject_padded_seeded below).  JMID_EINVAL:
 * E < 1, K outside 1..1024, T outside 2..24, A outside 1..64, threshold not finite or < 0, max_rounds outside 0..64, draw0 < 0, NULL
 * episode_ids / ctx / p0.  JMID_ERANGE or JMID_ETIMEOUT of any round is the status of the whole call and the outputs are then undefined. */
int jmid_denoise_reject_seeded(jmid_handle_t h, int E, int A, int K, int T, uint64_t seed, const uint32_t* episode_ids, int draw0,
                               const float* ctx, const float* p0, float dt, int precision, double threshold, int max_rounds,
                               float* vel_out, float* pos_out, int32_t* slot_out, int32_t* episode_out, int mem);

/* jmid_denoise_reject_seeded with walls: a joint sample is ACCEPTABLE iff it is acceptable there AND jmid_wall_statistics at (walls,
 * radius, the call's p0: T segments per agent) gives it n_agents_hitting == 0 AND a min_clear that is not NaN.  Everything else of the rule
 * is that entry's: the rounds, the ascending fill, the slots that stay flagged, slot_out / episode_out (whose counts now speak of slots
 * that are not acceptable for either cause), what pos = NULL means afterwards, the refusals, DDIM and a uniform agent count only.
 *   walls [L, 4] float64, a HOST array, 0 <= L <= 64, finite; radius finite and >= 0 (JMID_EINVAL otherwise)
 *   cause_out [E, 2] int32 = {slots whose round-0 sample fails the pedestrian predicate, slots whose round-0 sample fails the wall
 *             predicate}; a slot may count in both; may be NULL
 * The wall kernel runs next to the collision kernel on each round's candidates, and the one small download per round stays the only one.
 * L = 0 is bit-identical to jmid_denoise_reject_seeded in every output, with cause_out[:, 1] = 0: that entry IS this one at L = 0. */
int jmid_denoise_reject_walls_seeded(jmid_handle_t h, int E, int A, int K, int T, uint64_t seed, const uint32_t* episode_ids, int draw0,
                                     const float* ctx, const float* p0, float dt, int precision, double threshold, int max_rounds, int L,
                                     const double* walls, double radius, float* vel_out, float* pos_out, int32_t* slot_out,
                                     int32_t* episode_out, int32_t* cause_out, int mem);

/* jmid_predict_scene and jmid_forecast_scene with (seed, episode_ids [E]) in place of x_T: x_T is draw 0 with rows = K * A, filled on the
 * device (nothing but bw is uploaded).  Everything else as their namesakes, whose chain they share: bit-identical to them fed
 * jmid_noise_fill's draw 0. */
int jmid_predict_scene_seeded(jmid_handle_t h, int E, int A, int K, int T, int k, uint64_t seed, const uint32_t* episode_ids, float dt,
                              int precision, const float* bw, float* sel, float* logw, float* pos_out);
int jmid_forecast_scene_seeded(jmid_handle_t h, int E, int A, int K, int T, int k, uint64_t seed, const uint32_t* episode_ids, float dt,
                               int precision, const float* bw, double* forecasts_out, double* logw_out);

/* Seeded noise of a padded batch.  THE DECISION: episode e draws exactly what it draws alone, at ITS count - its tensor is the compact
 * [K * n_e, T, 2], n_e = n_agents[e]:
 *     idx = ((s * n_e + a) * T + t) * 2 + c,  counter = (idx / 4, episode_id, draw, 0),  the value lands in padded row s * A + a
 * so an episode's noise stays a pure function of (seed, episode id, draw, element): the same bits in a padded batch, in its count group
 * (jmid_*_seeded at A = n_e) and alone.  Drawing at the batch's A instead would make an episode's futures depend on its batch mates.
 * One Philox block serves four consecutive COMPACT elements, which may lie in two padded rows.
 *
 * jmid_noise_fill_padded: out [E, K*A, T, 2] (where `mem` says); the real rows of episode e are bit-identical to
 * jmid_noise_fill(E = 1, rows = K * n_agents[e]) of that episode, the padded rows quiet NaN.  n_agents and episode_ids are HOST arrays.
 * JMID_EINVAL: a dimension < 1, draw < 0, a NULL argument, a count outside 1..A.
 *
 * jmid_denoise_padded_seeded: jmid_denoise_padded with (seed, episode_ids) in place of x_T - draw 0 of the rule above, filled straight
 * into the workspace (whose padded rows are zeroed as jmid_denoise_padded zeroes them): bit-identical to jmid_denoise_padded fed
 * jmid_noise_fill_padded's draw 0.  DDIM only: JMID_EINVAL with a DDPM table on the handle, exactly like jmid_denoise_padded. */
int jmid_noise_fill_padded(jmid_handle_t h, uint64_t seed, int E, int A, int K, int T, const int32_t* n_agents, const uint32_t* episode_ids,
                           int draw, float* out, int mem);
int jmid_denoise_padded_seeded(jmid_handle_t h, int E, int A, int K, int T, const int32_t* n_agents, uint64_t seed, const uint32_t* episode_ids,
                               const float* ctx, const float* p0, float dt, int precision, float* vel_out, float* pos_out, int mem);

/* Collision-free sampling of a padded batch: ONE rejection loop for episodes of different agent counts, in the layout of "Padded scene
 * batches".  The rule is jmid_denoise_reject_walls_seeded's, word for word (L = 0: no walls, as jmid_denoise_reject_seeded is that entry at
 * L = 0), and three things change:
 *   Predicate  a candidate is ACCEPTABLE iff jmid_collision_statistics_padded (and, with walls, jmid_wall_statistics_padded at the call's
 *              p0) gives it no colliding / hitting agent and a clearance that is not NaN - those entries' own kernels on the round's
 *              counts.  An episode with n_agents[e] = 1 can only fail on walls
 *   Noise      round j draws by the padded rule above at draw number draw0 + j: episode e draws what it draws alone at its own count
 *   Reruns     a rerun is ONE padded seeded denoise call with the listed episodes' rows and THEIR counts, gathered in ascending order, at
 *              the CALL's A: the row stride does not shrink when the episodes left over are all smaller.  The padded share of the rows is
 *              computed and thrown away, as in every padded call
 * The candidates' padded rows are quiet NaN and are copied as they are: the accepted block is NaN in its padded rows in every round.
 * Equalities:
 *   - every count equal to A: bit-identical to jmid_denoise_reject_walls_seeded in all five outputs;
 *   - max_rounds = 0, draw0 = 0: vel_out and pos_out are bit-identical to jmid_denoise_padded_seeded;
 *   - round j's candidates are bit-identical to jmid_noise_fill_padded(draw = draw0 + j) + jmid_denoise_padded on the gathered rows and
 *     counts of exactly the rerun episodes, ascending, as ONE call at the call's A;
 *   - an episode's outputs are a function of (weights, its ctx, p0, n_agents[e], A, seed, id, draw0, threshold, walls, radius, max_rounds)
 *     only, under the chunk rule of jmid_set_chunk_episodes - not of its batch mates.
 * The host still reads ONE small download per round; the gathered counts of a rerun go up with the rerun's episode ids.
 * Afterwards the accepted set is what pos = NULL means for jmid_topk_padded, jmid_collision_statistics_padded and
 * jmid_wall_statistics_padded at (E, A, K, T), forgotten exactly as after jmid_denoise_padded.
 * JMID_EINVAL: the refusals of jmid_denoise_reject_walls_seeded and of jmid_denoise_padded_seeded (NULL n_agents, a count outside 1..A, a
 * DDPM table, the attention A/B knobs that have no masked kernel). */
int jmid_denoise_reject_padded_seeded(jmid_handle_t h, int E, int A, int K, int T, const int32_t* n_agents, uint64_t seed,
                                      const uint32_t* episode_ids, int draw0, const float* ctx, const float* p0, float dt, int precision,
                                      double threshold, int max_rounds, int L, const double* walls, double radius, float* vel_out,
                                      float* pos_out, int32_t* slot_out, int32_t* episode_out, int32_t* cause_out, int mem);

/* Collision repair: the second mechanism DiffusionTraj.sample names - constraint_type, next to with_constraints (MID/models/diffusion.py:
 * 544-613); every shipped config sets constraint_type: opt_softplus (test_time_configs/mid_jp.yaml:34).  The reference's stripped sampler
 * has no body for it and nothing in the reference mentions softplus, so THE RULE is decided here, as the rejection rule was.  OFF unless
 * this entry is called.  A small fp64 optimisation on FINISHED samples: only colliding samples are touched, no net evaluation, no redraw,
 * no noise (it works behind every entry that leaves positions, whatever drew them), no download.
 * Per joint sample x[a][t], a < n agents, t < T; inputs fp32, everything inside fp64, every sample independent of every other:
 *   Candidates  a sample is repaired iff jmid_collision_statistics' own kernel gives it n_agents_colliding > 0 at `threshold`.  A sample
 *               whose min_dist is NaN is untouched and reported as such (state 3); a sample with A = 1 or n_agents[e] = 1 is untouched.
 *               Every untouched sample comes back bit for bit.
 *   Objective   J(x) = sum over the pairs i < j (pdist order) and the segments s = 0 .. T - 2 of tau * softplus((m - d_ijs) / tau),
 *               m = threshold + margin, d_ijs the distance from the origin to the segment of the relative position in closest-point form:
 *                 a = x_i[s] - x_j[s], b = x_i[s+1] - x_j[s+1], ab = b - a, den = ab . ab,
 *                 u = den > 0 ? clamp(-(a . ab) / den, 0, 1) : 0,  c = a + u ab,  d = sqrt(c . c),  n = d > 0 ? c / d : (1, 0)
 *               The step from the present position is not part of it, as in the pedestrian predicate.
 *   Iteration   at most max_iter times:
 *                 1. dmin = the minimum of d over all pairs and segments; stop when dmin >= threshold + margin / 2;
 *                 2. sigma = sigmoid(z), z = (m - d) / tau, in the overflow-free form: e = exp(-|z|), sigma = 1 / (1 + e) for z >= 0 and
 *                    e / (1 + e) otherwise.  Pair (i, j, s) subtracts (sigma (1 - u)) n from g_i[s] and (sigma u) n from g_i[s+1] and
 *                    adds the same amounts to g_j;
 *                 3. x <- x - step g (Jacobi: every gradient comes from the same iterate).
 *               The summation order of g[a][t] is fixed: partners b ascending, per partner the segment t - 1 first, then the segment t.
 *               No atomics.
 *   End         x is rounded to fp32 and the predicate is evaluated on the rounded values with the predicate's own device function.
 *               Acceptable: state 1 (repaired).  Otherwise the sample reverts to its input bits, state 2: an output is always either the
 *               model's sample or an acceptable one.  The velocities of a repaired sample are
 *               float((double(x32[t]) - double(x32[t-1])) / dt), x32[-1] = p0.
 * Defaults of the Python layer (arguments here, not constants): margin 0.02 m, tau 0.005 m, step 0.02 m, max_iter 32.
 *   n_agents    int32 [E] HOST, or NULL: every agent is real.  Otherwise the layout and NaN conventions of "Padded scene batches": the
 *               padded agents take part in nothing and their rows are copied as they are
 *   pos         [E, K, A, T, 2], or NULL: the resident set (what jmid_denoise*, or the rejection entries, left; the rules of jmid_topk), which
 *               is repaired IN PLACE - a following jmid_topk(pos = NULL) or statistics entry sees the repaired set; the accepted block's
 *               velocities are rewritten too where the block holds them and p0 is given.  The forgetting rules are unchanged
 *   p0          [E, A, 2] or NULL (no velocities); dt must then be finite and > 0
 *   pos_out     [E, K, A, T, 2] or NULL; may be pos itself in JMID_MEM_DEVICE.  With pos = NULL: a copy of the repaired resident set
 *   vel_out     [E, K, A, T, 2] or NULL, IN and OUT: the caller's velocities, of which only the real rows of REPAIRED samples are rewritten
 *   sample_out  [E, K, 4] float = {min_dist before, min_dist after (of the sample that comes back), iterations used, state: 0 untouched,
 *               1 repaired, 2 reverted, 3 NaN}; may be NULL
 *   episode_out [E, 3] int32 = {samples colliding on entry (states 1 and 2), samples repaired, the largest iteration count}; may be NULL
 * max_iter = 0 is the identity plus the flags (every colliding sample is state 2).  Three launches on the handle's stream - the collision
 * kernel's lean form, one workgroup per (episode, sample) that holds the sample in LDS and does the iteration, the final predicate, the
 * revert and the velocities, one workgroup per episode for episode_out - and nothing comes back to the host in between.
 * Limits: those of jmid_collision_statistics.  JMID_EINVAL: those, a threshold or margin that is not finite or < 0, tau <= 0, step <= 0,
 * max_iter outside 0..1024, a NULL p0 with a non-NULL vel_out, a count outside 1..A, pos with every output NULL, pos = NULL without a
 * resident set of this shape. */
int jmid_repair_collisions(jmid_handle_t h, int E, int A, int K, int T, const int32_t* n_agents, const float* pos, const float* p0, float dt,
                           double threshold, double margin, double tau, double step, int max_iter, float* pos_out, float* vel_out,
                           float* sample_out, int32_t* episode_out, int mem);

/* Collision repair with walls: jmid_repair_collisions whose objective and whose two gates know the wall segments of
 * jmid_wall_statistics.  The reference has no body for this either, so THE RULE is decided here; it is that entry's rule plus a second
 * family of terms.  fp64 on the fp32 inputs, every sample independent of every other.  OFF unless this entry is called.
 *   Paths       agent a walks q[0 .. NP-1]: its T forecast points, with p0[a] in front when p0 is given (NP = T + 1) - the segments
 *               jmid_wall_statistics walks.  p0 is fixed: it takes no gradient and is never written.
 *   Candidates  a sample is a candidate iff the pedestrian predicate flags it (n_agents_colliding > 0 at `threshold`) OR the wall predicate
 *               flags it (jmid_wall_statistics' own kernel at (walls, wall_radius, p0) gives n_agents_hitting > 0).  A NaN in either
 *               minimum is state 3, untouched.  A single real agent (A = 1 or n_agents[e] = 1) IS a candidate when it hits a wall.
 *   Wall term   per (agent, step s = q[s] -> q[s+1], wall l) the objective gains tau * softplus((m_w - d) / tau), m_w = wall_radius + margin.
 *               d, the unit normal n and the weights of the step's two ends come from a closest-point form of their own (NOT the
 *               predicate's branchy function, which judges the result).  With b0 = q[s], b1 = q[s+1], the wall w0 -> w1 and the four
 *               difference vectors p00 = b0 - w0, p01 = b0 - w1, p10 = b1 - w0, p11 = b1 - w1, four candidates in fixed order, each the
 *               origin against a segment a -> b in jmid_repair_collisions' closed form (ab = b - a, den = ab . ab,
 *               u = den > 0 ? clamp(-(a . ab) / den, 0, 1) : 0, c = a + u ab, s = c . c; c points from the wall to the path):
 *                 0. b0 onto the wall:           (a, b) = (p00, p01), weights (1, 0) on (b0, b1)
 *                 1. b1 onto the wall:           (a, b) = (p10, p11), weights (0, 1)
 *                 2. the wall's start onto the step: (a, b) = (p00, p10), weights (1 - u, u)
 *                 3. the wall's end onto the step:   (a, b) = (p01, p11), weights (1 - u, u)
 *               The candidate with the smallest s wins, the first one on a tie; d = sqrt(s), n = d > 0 ? c / d : (1, 0).
 *               A step that PROPERLY CROSSES the wall - with W = w1 - w0, B = b1 - b0, o1 = W x p00, o2 = W x p10, o3 = By p00x - Bx p00y,
 *               o4 = By p01x - Bx p01y: o1 and o2 of strictly opposite signs AND o3 and o4 of strictly opposite signs - takes candidate 1
 *               with d negated and the normal reversed, so the far end is pulled back to the near end's side.
 *               sigma = sigmoid((m_w - d) / tau) in the overflow-free form; the step subtracts (sigma w_b0) n from g[b0] and
 *               (sigma w_b1) n from g[b1].
 *   Order       the summation order of g[a][t]: the pedestrian partners first, exactly as in jmid_repair_collisions; then the walls l
 *               ascending, per wall the step that ENDS in the point first, then the step that STARTS there.  No atomics.
 *   Stop        when the pedestrian minimum is >= threshold + margin / 2 AND the minimum of d over all (agent, step, wall) is
 *               >= wall_radius + margin / 2.  With fewer than two real agents only the wall minimum counts.
 *   End         x is rounded to fp32 and BOTH predicates' own device functions run on the rounded values (the p0 step included for the
 *               walls; a NaN is kept).  Acceptable to both (no pair closer than threshold, no d(a, l) - wall_radius < 0): state 1.
 *               Otherwise the sample reverts bit for bit, state 2.  The velocity rule is jmid_repair_collisions'.
 * A step that crosses a wall is repaired only by walking its far point back, point after point: a path that stays behind a wall for many
 * steps reverts within max_iter = 32.  That is a stated limit of the form.
 *   walls       [L, 4] float64 {x1, y1, x2, y2}, a HOST array, 0 <= L <= 64, finite; wall_radius finite and >= 0
 *   p0          [E, A, 2] or NULL: the first point of every path (and x32[-1] of the velocities).  NULL: T - 1 steps per agent
 *   sample_out, episode_out   as jmid_repair_collisions ("colliding on entry" reads "a candidate for either cause"): the old entry's rows
 *               are a prefix of this entry's outputs
 *   wall_out    [E, K, 2] float = {min_clear before, min_clear after (of the sample that comes back)}; may be NULL.  L = 0: +inf twice
 * Everything else - n_agents (with jmid_wall_statistics_padded's rules), pos = NULL and the resident set, pos_out, vel_out, the defaults -
 * as jmid_repair_collisions.  L = 0 IS jmid_repair_collisions, bit for bit in the four outputs they share.  Four launches on the handle's
 * stream: the collision kernel's lean form, the wall kernel's lean form, the repair kernel (the walls [L, 4] and the p0 rows staged in LDS
 * next to the sample: 53.0 KB at A = 64, T = 24, L = 64 with p0, inside the 64 KB a workgroup gets by default), the episode rows.
 * Limits: those of jmid_repair_collisions and jmid_wall_statistics.  JMID_EINVAL: those of jmid_repair_collisions, L outside 0..64, a
 * wall_radius that is not finite or < 0, L > 0 with walls NULL, a non-finite wall coordinate. */
int jmid_repair_collisions_walls(jmid_handle_t h, int E, int A, int K, int T, const int32_t* n_agents, const float* pos, const float* p0, float dt,
                                 double threshold, double margin, double tau, double step, int max_iter, int L, const double* walls,
                                 double wall_radius, float* pos_out, float* vel_out, float* sample_out, int32_t* episode_out, float* wall_out,
                                 int mem);

/* Guided sampling: a guidance term INSIDE the denoise loop.  The repair above moves a finished sample - the net never sees the correction -
 * and a redraw costs a whole denoise call; guidance nudges the intermediate sample after every denoise step, so the remaining steps of the
 * net run on the corrected state.  Like the rejection rule and the repair rule, the reference names the mechanism
 * (DiffusionTraj.sample(with_constraints, constraint_type)) and has no body for it, so THE RULE is decided here.  OFF unless these entries
 * are called; no existing entry changes.
 * State x [E, K*A, T, 2] fp32 is the loop's velocity state, row r = (e*K + s)*A + a: the A*T*2 floats of one joint sample (e, s) are
 * contiguous.  After the sampler update of step-table entry i (every entry, the last included), when weights[i] > 0, each sample goes
 * through three stages independently of every other sample; everything inside is fp64, without contraction into FMA:
 *   Integrate   acc[a][t] = acc[a][t-1] + double(x[a][t]) (acc[a][-1] = 0), q[a][t] = double(p0[e][a]) + double(dt) * acc[a][t], ascending
 *               t.  Only the a < n real agents take part (n = n_agents[e], or A).  A sample with a q that is not finite is untouched.
 *   Iterate     at most n_inner times exactly the Iteration of jmid_repair_collisions on q with step := weights[i] (metres): the minimum,
 *               the stop at threshold + margin / 2, the Jacobi step, the summation order.  With L > 0 the iteration of
 *               jmid_repair_collisions_walls: p0 is the fixed first point of every path, the wall terms come behind the partners, and
 *               the order and the stop rule (both minima clear) are that entry's.  The kernel calls the repair's own device functions.
 *               There is NO "End" stage: no rounding of positions, no predicate, no revert.  A sample that stops before its first
 *               iteration is NOT WRITTEN at all.  T = 1 has no pedestrian segment: untouched without walls, wall terms only (the step
 *               from p0) with them.  With one real agent only the wall terms exist.
 *   Write back  with D[a][t] = q_final[a][t] - q_initial[a][t], D[a][-1] = 0:
 *                 x[a][t] <- float(double(x[a][t]) + (D[a][t] - D[a][t-1]) / double(dt))
 *               for all real rows of a sample that took at least one iteration: one rounding per point, no cumsum / difference round
 *               trip - a point whose difference is exactly 0 keeps its value.  Padded agents' rows are never read or written.
 * weights[i] = 0: no launch behind entry i; an all-zero table makes the whole call the unguided call, bit for bit.  Because the samples of
 * one JMID episode attend to each other, "unchanged" is a statement per episode: an episode none of whose samples ever took an iteration
 * equals the unguided call in every bit.
 *
 * jmid_guide_step: ONE application of the rule to a given block x [E, K*A, T, 2] at `weight` -> x_out (may be x itself in
 * JMID_MEM_DEVICE); weight = 0 copies.  guide_out [E, K, 2] float = {1 if the sample iterated, iterations used}; may be NULL.
 *
 * jmid_denoise_guided: jmid_denoise (n_agents NULL) or jmid_denoise_padded (a HOST array [E]) under the rule, DDIM.  Every step embeds at
 * its head (the unfused seam, bit-identical to the fused one), the guide kernel runs behind each entry with weights[i] > 0 on the stream of
 * the chunk it belongs to, and the integrator and everything behind the loop are unchanged: vel_out, pos_out and the resident positions
 * are the guided ones.  The call equals, bit for bit, the chain of one-entry calls with jmid_guide_step between them.  Never captured
 * into a graph.  Nothing of the guidance stays on the handle.
 *   weights     double [n_steps], a HOST array (n_steps: the installed DDIM table), metres, finite and >= 0
 *   walls       [L, 4] float64 {x1, y1, x2, y2}, a HOST array, 0 <= L <= 64 (L = 0: no walls), finite; wall_radius finite and >= 0
 *   p0          [E, A, 2], required; dt finite and > 0
 *   guide_out   [E, K, 2] float = {steps at which the sample iterated, iterations in total}; may be NULL
 * jmid_denoise_guided_seeded: the same with (seed, episode_ids) in place of x_T - draw 0, by the padded rule when counts are given.
 * The kernel holds a sample in LDS as the repair with walls does (53.0 KB at A = 64, T = 24, L = 64).
 * Limits: 1 <= K <= 1024, 1 <= T <= 24, 1 <= A <= 64.  JMID_EINVAL: those; a threshold or margin that is not finite or < 0; tau <= 0;
 * L outside 0..64, L > 0 with walls NULL, a non-finite wall coordinate, a wall_radius that is not finite or < 0; p0 NULL; dt not finite or
 * <= 0; a weight that is negative or not finite; n_inner outside 1..64; a count outside 1..A; a handle with the DDPM table set (the
 * denoise entries); and whatever jmid_denoise / jmid_denoise_padded refuse. */
int jmid_guide_step(jmid_handle_t h, int E, int A, int K, int T, const int32_t* n_agents, const float* x, const float* p0, float dt,
                    double threshold, double margin, double tau, double weight, int n_inner, int L, const double* walls, double wall_radius,
                    float* x_out, float* guide_out, int mem);
int jmid_denoise_guided(jmid_handle_t h, int E, int A, int K, int T, const int32_t* n_agents, const float* x_T, const float* ctx, const float* p0,
                        float dt, int precision, double threshold, double margin, double tau, const double* weights, int n_inner, int L,
                        const double* walls, double wall_radius, float* vel_out, float* pos_out, float* guide_out, int mem);
int jmid_denoise_guided_seeded(jmid_handle_t h, int E, int A, int K, int T, const int32_t* n_agents, uint64_t seed, const uint32_t* episode_ids,
                               const float* ctx, const float* p0, float dt, int precision, double threshold, double margin, double tau,
                               const double* weights, int n_inner, int L, const double* walls, double wall_radius, float* vel_out,
                               float* pos_out, float* guide_out, int mem);

/* Padded chains on the resident scene: jmid_predict_scene / jmid_forecast_scene (and their seeded forms) for a scene whose episodes have
 * DIFFERENT in-cluster counts - what jmid_build_scene leaves whenever it chooses the clusters itself - in one call, in the layout and
 * under the rules of "Padded scene batches" above.  The caller passes no n_agents: the counts are the resident scene's n_in, read on the
 * device where the build kernel wrote them (the chain uploads nothing but x_T and bw; the seeded forms nothing but bw).
 *   A     must equal the LARGEST in-cluster count of the resident scene, and every count must be >= 1: JMID_EINVAL otherwise (the scene
 *         stays resident; an episode with an empty cluster has nothing to forecast - leave it out of the build)
 *   x_T   [E, K*A, T, 2] in the padded layout, row s*A + a real iff a < n_in[e]; padded rows are never read, NaN included.  The seeded
 *         forms draw by the padded rule above: episode e gets the bits jmid_predict_scene_seeded gives it in a batch of its own count
 *   the gather writes zeros into the padded rows of the encoder's inputs (x_st, nbr_sum, edge_mask, p0, first_index), never what an earlier
 *   call left there; the encoder runs on all E * A rows, and a padded row can neither raise JMID_ERANGE nor reach a real row
 *   a scene from jmid_build_scene_var works (first_index is gathered and the encoder runs as jmid_encode_var): the padded form of short
 *   histories, which jmid_predict_padded - it takes no first_index - does not have
 *   sel, logw, pos_out and the resident positions: quiet NaN in the padded rows; the ranking is jmid_topk_padded's, in 2 * n_in[e] dimensions
 *   forecasts_out / logw_out: as jmid_forecast_scene - an in-cluster pedestrian reads its own (real) row, everybody else the
 *   constant-velocity row: no NaN in either array
 * The real rows are bit-identical to jmid_predict_padded fed the gathered rows of jmid_scene_get and the same x_T; a scene whose counts
 * are all equal gives the bits of jmid_predict_scene / jmid_forecast_scene.  Everything else - limits, JMID_ERANGE, JMID_ETIMEOUT, the
 * forecast entries' refusals, DDIM only - as their namesakes. */
int jmid_predict_scene_padded(jmid_handle_t h, int E, int A, int K, int T, int k, const float* x_T, float dt, int precision, const float* bw,
                              float* sel, float* logw, float* pos_out);
int jmid_forecast_scene_padded(jmid_handle_t h, int E, int A, int K, int T, int k, const float* x_T, float dt, int precision, const float* bw,
                               double* forecasts_out, double* logw_out);
int jmid_predict_scene_padded_seeded(jmid_handle_t h, int E, int A, int K, int T, int k, uint64_t seed, const uint32_t* episode_ids, float dt,
                                     int precision, const float* bw, float* sel, float* logw, float* pos_out);
int jmid_forecast_scene_padded_seeded(jmid_handle_t h, int E, int A, int K, int T, int k, uint64_t seed, const uint32_t* episode_ids, float dt,
                                      int precision, const float* bw, double* forecasts_out, double* logw_out);

/* Constrained chains: guidance and repair INSIDE the one-entry chains - one upload, the phases on the stream, one download that brings the
 * reports with it.  OFF unless these entries are called; no existing entry, layout or refusal changes.
 *   jmid_predict_constrained          n_agents NULL: jmid_predict; a HOST array [E]: jmid_predict_padded
 *   jmid_predict_scene_constrained    x_T NULL: the seeded form from (seed, episode_ids) (draw 0, by the padded rule when `padded`), else x_T
 *                                     and (seed, episode_ids) unread; `padded` != 0: the rules of jmid_predict_scene_padded
 *   jmid_forecast_scene_constrained   the same for jmid_forecast_scene / _seeded / _padded / _padded_seeded
 * THE RULE is a composition, not a restatement.  A constrained chain equals, bit for bit in every output and every report row, the staged
 * calls: the gathered rows of the scene (jmid_scene_get; or the caller's arrays) -> jmid_encode / jmid_encode_var -> jmid_denoise_guided
 * [_seeded] when guide_weights is given, else jmid_denoise[_padded][_seeded] -> when `repair`, jmid_repair_collisions (repair_walls = 0)
 * or jmid_repair_collisions_walls on the resident set (pos = NULL, with p0 and dt) -> jmid_topk[_padded](pos = NULL) -> the assembly of
 * jmid_forecast_scene.  The ranking and the assembly read the repaired set, and with pos_out so does the caller.
 *   threshold      of both mechanisms (metres between two pedestrians' centres)
 *   guide_weights  double [n_steps], a HOST array (the installed DDIM table), or NULL: no guidance.  n_inner, guide_margin, guide_tau: the
 *                  n_inner, margin and tau of jmid_denoise_guided.  guide_walls != 0: the guidance takes the wall terms too
 *   repair         0: no repair.  margin, tau, step, max_iter: those of jmid_repair_collisions.  repair_walls != 0: the repair with walls
 *   L, walls, wall_radius   [L, 4] float64 {x1, y1, x2, y2}, a HOST array; sent once per call, for both mechanisms.  Read only when
 *                  guide_walls or repair_walls asks for them
 *   guide_out [E, K, 2], sample_out [E, K, 4], episode_out [E, 3] int32, wall_out [E, K, 2]: HOST arrays, each may be NULL - the rows of
 *                  jmid_denoise_guided, jmid_repair_collisions and jmid_repair_collisions_walls, unchanged.  A mechanism that is off leaves
 *                  zeros in its rows (no guided step; state 0); a repair without repair_walls leaves +inf in wall_out (that entry's L = 0)
 * With guidance the denoise loop is never captured into a graph (as jmid_denoise_guided); a repair-only chain keeps whatever capture the
 * unconstrained chain of its shape has.  The repair phase is the staged entries' launches on the handle's stream between the denoise stage
 * and the ranking; the reports lie inside the chain's download block: still one device-to-host copy and one synchronisation per call.
 * Not here: the redraw loop (jmid_denoise_reject_*), DDPM.
 * JMID_EINVAL, before anything is enqueued: whatever the namesake chain refuses; whatever jmid_denoise_guided and
 * jmid_repair_collisions_walls refuse for the same arguments (so T >= 2 with repair); guide_walls or repair_walls with L = 0; a DDPM table.
 * JMID_ERANGE and JMID_ETIMEOUT as in the chains (the reports are then undefined too). */
int jmid_predict_constrained(jmid_handle_t h, int E, int A, int K, int T, int k, const int32_t* n_agents, const float* x_st, const float* nbr_sum,
                             const float* edge_mask, const float* x_T, const float* p0, float dt, int precision, const float* bw, double threshold,
                             const double* guide_weights, int n_inner, double guide_margin, double guide_tau, int guide_walls, int repair,
                             double margin, double tau, double step, int max_iter, int repair_walls, int L, const double* walls,
                             double wall_radius, float* sel, float* logw, float* pos_out, float* guide_out, float* sample_out,
                             int32_t* episode_out, float* wall_out);
int jmid_predict_scene_constrained(jmid_handle_t h, int E, int A, int K, int T, int k, int padded, const float* x_T, uint64_t seed,
                                   const uint32_t* episode_ids, float dt, int precision, const float* bw, double threshold,
                                   const double* guide_weights, int n_inner, double guide_margin, double guide_tau, int guide_walls, int repair,
                                   double margin, double tau, double step, int max_iter, int repair_walls, int L, const double* walls,
                                   double wall_radius, float* sel, float* logw, float* pos_out, float* guide_out, float* sample_out,
                                   int32_t* episode_out, float* wall_out);
int jmid_forecast_scene_constrained(jmid_handle_t h, int E, int A, int K, int T, int k, int padded, const float* x_T, uint64_t seed,
                                    const uint32_t* episode_ids, float dt, int precision, const float* bw, double threshold,
                                    const double* guide_weights, int n_inner, double guide_margin, double guide_tau, int guide_walls, int repair,
                                    double margin, double tau, double step, int max_iter, int repair_walls, int L, const double* walls,
                                    double wall_radius, double* forecasts_out, double* logw_out, float* guide_out, float* sample_out,
                                    int32_t* episode_out, float* wall_out);

/* ---- the denoising loss on data with known futures: DiffusionTraj.get_loss (MID/models/diffusion.py:448-476), reached through
 * AutoEncoder.get_loss (MID/models/autoencoder.py:105-122) from MID.validation() (MID/mid.py:252-296, its "Avg. Val Loss") - the
 * noise-prediction MSE of ONE net evaluation per scene, every agent row at a timestep of its own.
 *
 * jmid_set_loss_schedule: the forward process per TIMESTEP: beta, c0 = sqrt(alpha_bar), c1 = sqrt(1 - alpha_bar) [n_t], index = timestep,
 * entry 0 the reference's padding entry (n_t = num_steps + 1 = 101), c0 / c1 computed by the host in fp32 as diffusion.py:456-457 does.
 * Builds the device time table [n_t, hyper width] with the expression of the sampler's step table: a timestep that is also a step of the
 * installed DDIM table has identical bits.  Independent of jmid_set_ddim_table / jmid_set_ddpm_table (either order, any number of times);
 * captured loops stay.
 *
 * jmid_loss: x0, e [E, A, T, 2] and ctx [E, A, ctx_dim] where `mem` says; t int32 [E, A] is always a HOST array, like n_agents, values
 * 1 .. n_t - 1.  x_t = c0[t_r] x0 + c1[t_r] e (two rounded products, one rounded sum), e_theta = net(x_t, beta[t_r], ctx) with K = 1 - the
 * row's timestep is folded into its hyper-net row once, the net's kernels are those of jmid_net_eval -, then per element (e_theta - e)^2
 * in fp32 (F.mse_loss(reduction="none")) and fp64 sums in a fixed order (no atomics: the same bits for every chunk plan).
 *   n_agents    int32 [E] HOST, or NULL when every row is real: a padded batch as jmid_net_eval_padded (generate_mask,
 *               MID/dataset/preprocessing.py:35-89: padded agents are no attention keys and are dropped from the loss)
 *   loss_out    double [2]: the mean squared error over the real rows' T * 2 components, the number of components
 *   row_out     double [E, A] sum of squared errors per row, or NULL; NaN for padded rows
 *   e_theta_out [E, A, T, 2] or NULL; NaN for padded rows
 * (the three outputs where `mem` says).  JMID_NET_JMID and JMID_NET_IMID, every precision.  JMID_EINVAL before anything is enqueued: no
 * loss schedule, a t outside 1 .. n_t - 1 (the message names the row), a count outside 1..A, a padded call on a non-default attention
 * variant, T > 24, NULL t / x0 / e / ctx / loss_out.  JMID_ERANGE and JMID_ETIMEOUT as from jmid_net_eval.  Leaves no state on the handle
 * (but, like jmid_net_eval, reuses the workspace of the resident positions).
 *
 * jmid_loss_seeded: the same with e drawn by the library - draw 0 of the counter generator with rows = A, the bits
 * jmid_noise_fill(seed, E, A, T, episode_ids, 0) returns; t stays the caller's. */
int jmid_set_loss_schedule(jmid_handle_t h, int n_t, const float* beta, const float* c0, const float* c1);
int jmid_loss(jmid_handle_t h, int E, int A, int T, const int32_t* n_agents, const int32_t* t, const float* x0, const float* e, const float* ctx,
              int precision, double* loss_out, double* row_out, float* e_theta_out, int mem);
int jmid_loss_seeded(jmid_handle_t h, int E, int A, int T, const int32_t* n_agents, const int32_t* t, const float* x0, uint64_t seed,
                     const uint32_t* episode_ids, const float* ctx, int precision, double* loss_out, double* row_out, float* e_theta_out, int mem);

/* The stream (a hipStream_t passed as void*, e.g. torch.cuda.current_stream().cuda_stream; NULL = the legacy default
 * stream) that produces the inputs and consumes the outputs of this handle's JMID_MEM_DEVICE calls - see Conventions. */
int jmid_set_caller_stream(jmid_handle_t h, void* stream);

/* Number of calls on this handle whose denoise loop ran as a replayed hipGraph (see "graph" below); -1 for a null handle. */
int64_t jmid_graph_replays(jmid_handle_t h);

/* Number of calls on this handle that ended with JMID_ERANGE (an fp16 operand left the fp16 range in a split-fp16 mode and the
 * caller had to repeat the call in JMID_PREC_F32 - the Python predictor does, forecaster.py: what the reference computes in fp32
 * throughout, MID/models/diffusion.py:478-541, so the result is unchanged and only the latency differs); -1 for a null handle.
 * A deployment with trained weights reads this to see how often the slow path fires. */
int64_t jmid_erange_count(jmid_handle_t h);
/* Number of calls on this handle that ended with JMID_ETIMEOUT (at most one per handle in practice: the first one switches the handle
 * to the unfused kernels for good); -1 for a null handle. */
int64_t jmid_timeout_count(jmid_handle_t h);

/* ---- tuning / measurement ------------------------------------------------------------------ */
/* Episodes processed together per pass of the 50-step loop (0 = automatic: a whole number of rounds of the attention
 * launch, a short ragged tail spread over the full chunks).  Results are bit-identical for every chunking of the same
 * call; the split-KV factor of the attention launches is a function of (E, A, K, T) and the precision only, so calls with different
 * episode counts agree to rounding (ADE ~1e-7 m), not bit for bit, when head_dim is 128. */
int jmid_set_chunk_episodes(jmid_handle_t h, int episodes);
/* Run-time switches of a handle.  The production library knows ONE key:
 *   "lanes"           chunks of the denoise loop in flight at once on separate HIP streams, 1..4 (default 2; the results do
 *                     not depend on it)
 * The diagnostics flavour of the library (built with -DJMID_DIAGNOSTICS as csrc/libjmid_hip_diag.so; what tests/ and tools/
 * load) additionally takes the implementation knobs the experiments of docs/NOTEBOOK.md are made with - kernel-variant
 * selectors such as "gemm_h_variant", "ln_fuse", "ln_rows", "mx_ln", "attn_mx", "attn_nsplit", "vt_stage", "graph",
 * "out_traj", "csl_swap", "attn_pf" (listed with their value ranges in csrc/jmid_abi.hip::jmid_set_tuning and
 * csrc/common.hpp::Tuning; every variant of a key computes the same values, most of them bit-identically) - and, with
 * -DJMID_ABLATIONS on top, the timing ablations "gemm_abl" / "attn_abl" (WRONG results).  Every switch belongs to the handle it
 * is set on.  Unknown keys return JMID_EINVAL. */
int jmid_set_tuning(jmid_handle_t h, const char* key, int value);
/* Per-kernel-class timing with HIP events recorded on the handle's stream.
 * mask: bit i enables class i (see jmid_kernel_class_name); 0 disables.  Timers accumulate until reset. */
int jmid_profile_enable(jmid_handle_t h, uint32_t class_mask);
int jmid_profile_reset(jmid_handle_t h);
/* Synchronizes the stream and returns, for kernel class `cls`, the number of launches and the summed
 * duration in milliseconds since the last reset. */
int jmid_profile_get(jmid_handle_t h, int cls, int64_t* n_launches, double* total_ms);
int jmid_kernel_class_count(void);
const char* jmid_kernel_class_name(int cls);
/* Block until all work queued on the handle's stream has finished. */
int jmid_synchronize(jmid_handle_t h);

/* ---- diagnostics: single-kernel entry points for the unit tests (HOST buffers only) ----------- */
/* Exported by the diagnostics flavour only (-DJMID_DIAGNOSTICS, csrc/libjmid_hip_diag.so). */
#ifdef JMID_DIAGNOSTICS
/* C[M,N] = A[M,K] . Wt[N,K]^T + bias (optional ReLU): the nn.Linear contraction of every layer. */
int jmid_dbg_gemm(jmid_handle_t h, int M, int N, int K, const float* A, const float* Wt, const float* bias, int relu,
                  int precision, float* C);
/* Multi-head self-attention over `nseq` sequences of length S from a packed QKV buffer
 * [nseq*S, 3*d_model] -> OUT [nseq*S, d_model] (heads/dims of the handle). */
int jmid_dbg_attention(jmid_handle_t h, int nseq, int S, const float* QKV, int precision, float* OUT);
/* X <- LayerNorm(X + A . Wt^T + bias) * gamma + beta in JMID_PREC_F16MX at d_model 512 (A [M, K], Wt [512, K], X [M, 512]), with the
 * second-generation kernels: fused = 1 the row-complete GEMM + residual + LayerNorm, 0 the GEMM + add_ln2 pair, 3 the small-launch
 * GEMM whose workgroups exchange the row statistics and normalise their own columns (all bit-identical). */
int jmid_dbg_gemm_ln_mx(jmid_handle_t h, int M, int K, const float* A, const float* Wt, const float* bias, const float* gamma,
                        const float* beta, float* X, int fused);
/* X <- LayerNorm(X + Y) * gamma + beta, eps = 1e-5 (post-norm residual of nn.TransformerEncoderLayer). */
int jmid_dbg_add_layernorm(jmid_handle_t h, int M, int d, float* X, const float* Y, const float* gamma,
                           const float* beta);
/* The chunk plan run_network would use for a call of E episodes of `tokens_per_episode` tokens (host logic only, no device):
 * writes at most `cap` chunk sizes to `sizes`, returns the number of chunks (or a negative JMID_E* code). */
int jmid_dbg_plan_chunks(int net_kind, int nhead, int lanes, int chunk_episodes, int E, int tokens_per_episode, int* sizes, int cap);
/* ... of a call in arithmetic mode `precision` (a JMID_PREC_F16MX batch of at most 2 560 tokens stays ONE chunk: its out-projection /
 * linear2 launches then carry the LayerNorm and the split-KV merge; every other mode runs such a batch as two halves side by side). */
int jmid_dbg_plan_chunks_mode(int net_kind, int nhead, int lanes, int chunk_episodes, int E, int tokens_per_episode, int precision, int* sizes, int cap);
/* The launch plan of ONE split-fp16 GEMM (csrc/launch_plan.hpp::plan_gemm; host logic only, no device): what the planner decides
 * for a launch of mode (0 F16X3, 1 F16X2, 2 F16MX), epilogue class epi (0 bias, 1 bias + ReLU, 2 ConcatSquash) and out (0 fp32,
 * 1 split planes, 2 Q / K / V^T, 4 + residual + LayerNorm in one small launch) on [M, K] x [N, K], with `small_now` / `one_chunk` as the
 * call's facts and knobs[JMID_DBG_GEMM_PLAN_KNOBS] = the jmid_set_tuning values of "gemm_h_variant", "gemm_small", "ln_rows",
 * "small_lnx", "small_lnx2", "cus", "vt_stage", "csl_swap", "h1_stage", "gemm_pn", "small_qk", "small_pn", "gemm_ng" in that order.
 * plan[8] <- kernel family (a mode), tile shape (GemmShape; 0 = the launch does not fit, out = 4 only), flag word, N-tiles per column
 * group, the shape's tile rows and columns, and the row tile of the first- / second-generation GEMM + LayerNorm kernel for M rows. */
#define JMID_DBG_GEMM_PLAN_KNOBS 13
int jmid_dbg_gemm_plan(int mode, int epi, int out, int M, int N, int K, int small_now, int one_chunk, const int* knobs, int* plan);
/* The layouts of a chained call's I/O block and of the scene workspace (csrc/jmid_abi.hip::chain_io, scene_arrays; host logic only, no
 * device): where every array of jmid_predict* / jmid_predict_scene* / jmid_forecast_scene* lies for a handle of this hist_len and ctx_dim, a
 * call of E, A, K, T, k and a resident scene of N pedestrians.  flags: JMID_DBG_LAYOUT_SCENE the scene entries (clear: host arrays),
 * _FORECAST jmid_forecast_scene*, _SEEDED the seeded entries, _PADDED the padded ones, _FIRST_INDEX a scene built with first_frame, _BW a
 * bw is given, _POS pos_out is given, _CV the scene was built with cv_out (at horizon T).  JMID_EINVAL for a call no entry makes: forecast,
 * seeded or first_index without scene; a forecast without cv or with pos_out; k == K without pos_out (outside a forecast).
 * Every array is a pair (byte offset from the block's base, bytes); an array the call does not have is (-1, 0).
 * chain_dev, chain_pin [JMID_DBG_CHAIN_WORDS]: the device block and the pinned block - 14 arrays, then the upload block's (offset, bytes),
 * the download block's (offset, bytes) and the block's size.  With Th = hist_len and fp32 unless said:
 *    0 x_st [E A, Th, 6]   1 nbr_sum [E A, 2, Th, 6]   2 edge_mask [E A, 2]   3 x_T [E, K A, T, 2]   4 p0 [E, A, 2]   5 bw [T] (k < K and _BW)
 *    6 ctx [E A, ctx_dim] (device only)   7 the range flag, one int32   8 forecasts [E, N, k, T+1, 2] fp64   9 their logw [E, N, k] fp64 (8, 9: _FORECAST)
 *   10 sel [E, A, k, T, 2]   11 logw [E, A, k] (10, 11: k < K)   12 pos [E, K, A, T, 2] (_POS)   13 first_index [E A] int32 (_FIRST_INDEX, device only)
 * The upload block is arrays 0-5 (a scene call's copy starts at x_T), the download block 7-12, ending behind 9 in a forecast - whose pinned
 * block has no 10-12.
 * scene [JMID_DBG_SCENE_WORDS]: 13 arrays, then the grid block's bytes, the download block's (offset, bytes) and the workspace's size:
 *    0 human_xy [E, Th, N, 2] fp64   1 robot_xy [E, Th, 2] fp64   2 pose_now [E, N, 2] fp64 (0-2: the grid block, the workspace's first bytes)
 *    3 x [E, N, Th, 6]   4 x_st [E, N, Th, 6]   5 nbr_sum [E, N, 2, Th, 6]   6 edge_mask [E, N, 2]   7 p0 [E, N, 2]
 *    8 n_in [E] int32   9 in_cluster [E, N] bytes   10 robot_in [E] bytes   11 cv [E, N, T, 2] fp64 (_CV)   (8-11: the download block)
 *   12 first_index [E, N] int32 (_FIRST_INDEX) */
#define JMID_DBG_LAYOUT_SCENE 1
#define JMID_DBG_LAYOUT_FORECAST 2
#define JMID_DBG_LAYOUT_SEEDED 4
#define JMID_DBG_LAYOUT_PADDED 8
#define JMID_DBG_LAYOUT_FIRST_INDEX 16
#define JMID_DBG_LAYOUT_BW 32
#define JMID_DBG_LAYOUT_POS 64
#define JMID_DBG_LAYOUT_CV 128
#define JMID_DBG_CHAIN_WORDS (2 * 14 + 5)
#define JMID_DBG_SCENE_WORDS (2 * 13 + 4)
int jmid_dbg_chain_layout(int hist_len, int ctx_dim, int E, int A, int K, int T, int k, int N, int flags, int64_t* chain_dev, int64_t* chain_pin,
                          int64_t* scene);
/* Layer 0's Q, K, V of one denoise step of a JMID net in a split-fp16 mode, as the step's kernels leave them for the attention
 * kernel: x [M, 2] (M = E K A T tokens) is embedded at step-table entry `step` with the hyper rows hyp [E A, hyper width] (the ctx
 * part of the hyper nets: gate1 | bias1 | ... as the handle lays them out), layer 0's operand planes are made - expanded from the
 * per-(row, step) coefficient tables, or by the in_proj GEMM with jmid_set_tuning "qkv0" = 1 - and read back as fp32
 * qkv [M, 3 d_model] (hi + lo plane, or the bf8 image where it replaces a lo plane; Q without its softmax scale).  thyp_row (or
 * NULL) receives the time part of the hyper nets at that step, [hyper width].  hyp_width is the caller's row length: a value other
 * than the handle's hyper width (2 d_model + 2 d_mid + 2 d_low + 4) is JMID_EINVAL.  "qkv0" = 2 (A/B): expanded, with the table's
 * GEMM as one running fp32 sum instead of per-tile sums. */
int jmid_dbg_qkv0(jmid_handle_t h, int E, int A, int K, int T, const float* x, const float* hyp, int hyp_width, int step, int precision,
                  float* qkv, float* thyp_row);
/* The tail of one denoise step alone (concat3 -> concat4 -> output layer) in a split-fp16 mode: X [M, d_model] fp32 stands for the
 * last LayerNorm's output and is split into the planes the mode's concat3 reads (X_hi; X_hi + X_lo in JMID_PREC_F16X3), hyp and step
 * as for jmid_dbg_qkv0; e [M, 2] receives e_theta.  The tail runs as a step of a one-chunk call runs it: as one 2 x d_model map per
 * (episode, agent) row from a one-step table, or as the two GEMMs + the output kernel with jmid_set_tuning "tail_fold" = 1.
 * JMID_PREC_F32: the two fp32 GEMMs + the output kernel on X itself. */
int jmid_dbg_tail(jmid_handle_t h, int E, int A, int K, int T, const float* X, const float* hyp, int hyp_width, int step, int precision,
                  float* e, float* thyp_row);
/* The seam between e_theta of step-table entry `step` and the residual stream of entry `next_step`, as a step of a one-chunk call of
 * that shape on an idle handle runs it after its last layer (all four precisions, JMID and iMID; the launches are that plan's: the
 * folded tail or the two tail GEMMs + the output kernel by jmid_set_tuning "tail_fold", one wave per token or per trajectory piece by
 * "out_traj"; DDIM or DDPM as the handle's step table is): the tail on X [M, d_model] fp32 (split as jmid_dbg_tail splits it), the
 * sampler update of x [M, 2] with z [M, 2] (or NULL: no draw; a DDPM entry that takes none ignores it) and - next_step >= 0 - the
 * embedding of the updated x with the time row of `next_step`; next_step = -1: the loop's last step, no embedding.  The hyper rows:
 * exactly one of ctx [E A, ctx_dim] (the call's own hyper GEMM makes them) and hyp [E A, hyp_width] (given, as for jmid_dbg_qkv0).
 * embed_only != 0: the embedding kernel of a call's first step alone on x at entry `step` (X, z and next_step are not read).
 *   x_next [M, 2]     x after the update (embed_only: x)
 *   hi, lo [M, d_model] each: the embedding's buffers after the launch as the mode stores them, as fp32 - blocked planes un-blocked,
 *                     the bf8 byte plane decoded; JMID_PREC_F32: hi = X, lo = 0.  Before the launch every one of those buffers that is
 *                     not an input of the tail is filled with the byte JMID_DBG_SEAM_FILL, the others hold X as split: with
 *                     next_step = -1 they come back as that (fp16 planes of that byte: 0x3c3c = 1.05859375, a bf8 byte: 1.0)
 *   hyp_out (or NULL) [E A, hyper width]: the hyper rows the kernels read
 *   thyp_rows (or NULL) [2, hyper width]: the time rows of `step` and of `next_step` (next_step = -1: of `step` again)
 *   coef (or NULL) [JMID_DBG_SEAM_COEF_WORDS]: the handle's coefficients of `step`: c_e, c_x, n_x, n_e (DDIM), c0, c1, sigma, and 1.0
 *                     where the DDPM entry takes a draw
 *   plan [JMID_DBG_SEAM_PLAN_WORDS]: the kernel that ran (JMID_DBG_SEAM_*), its tokens per wave (out_tpw; 0 = one wave per token), the
 *                     representation (0 fp32, 1 fp16 hi + lo, 2 fp16 hi + bf8 lo), DDPM, embedded for next_step, folded tail, range flag.
 * Returns as a denoise call does when the flag is set. */
#define JMID_DBG_SEAM_FILL 0x3c
#define JMID_DBG_SEAM_OUT 0        /* out_ddim_kernel */
#define JMID_DBG_SEAM_OUT_TRAJ 1   /* out_ddim_traj_kernel */
#define JMID_DBG_SEAM_FOLD 2       /* tail_fold_kernel */
#define JMID_DBG_SEAM_FOLD_TRAJ 3  /* tail_fold_traj_kernel */
#define JMID_DBG_SEAM_EMBED 4      /* embed_kernel */
#define JMID_DBG_SEAM_COEF_WORDS 8
#define JMID_DBG_SEAM_PLAN_WORDS 7
int jmid_dbg_seam(jmid_handle_t h, int E, int A, int K, int T, const float* X, const float* x, const float* z, const float* ctx, const float* hyp,
                  int hyp_width, int step, int next_step, int precision, int embed_only, float* x_next, float* hi, float* lo, float* hyp_out,
                  float* thyp_rows, float* coef, int* plan);
/* Encoder layer `layer` of one net evaluation, launch for launch as a step of a one-chunk call of that shape on an idle handle runs it
 * (all four precisions, JMID and iMID; the split-KV factor and the launch plans are that call's), with every stage copied out in
 * between.  X [M, d_model] fp32 (M = E K A T tokens) is split into the operand planes the mode's layer reads (fp16 hi + lo; hi + the
 * bf8 image of lo where the residual stream's lo plane is the byte plane); n_agents [E] (or NULL: an unpadded call) makes it a padded
 * call, its key-mask words made on the device as a denoise call makes them; last != 0: the layer is the encoder's last (norm2 does
 * not write the lo plane where nothing reads it).  Layer 0 runs its in_proj GEMM here (its coefficient expansion: jmid_dbg_qkv0).
 * hi and lo, each [M x JMID_DBG_LAYER_WIDTH(d_model, d_ff)] floats, receive the two planes of every stage as fp32 (one array and a zero
 * lo plane in JMID_PREC_F32, and wherever a mode does not write a lo plane); stage s is the row-major [M, width] block at
 * M x (the widths of the stages before it):
 *   0  X as split                                        [M, d_model]
 *   1  Q, K, V as the attention kernel reads them        [M, 3 d_model]  (Q's pre-scale undone, bf8 images decoded, V^T read back)
 *   2  the attention output                              [M, d_model]
 *   3  X after out_proj + residual + LayerNorm 1         [M, d_model]
 *   4  linear1 + ReLU                                    [M, d_ff]
 *   5  X after linear2 + residual + LayerNorm 2          [M, d_model]
 * plan [JMID_DBG_LAYER_PLAN_WORDS] receives: bit mask of the stages present (stage 2 is absent when the out-projection's launch merges
 * the split-KV partials itself); in_proj's GEMM family, tile shape (GemmShape) and flag word; linear1's; the path of the out_proj
 * block (0 row-tile GEMM + LayerNorm second generation, 1 first generation, 2 one small launch with the statistics exchange, 3 GEMM +
 * add_ln), its row tile and the tile shape of its GEMM; the same three for the linear2 block; V^T written by in_proj's epilogue;
 * bf8 images of K; of Q_lo; the split-KV factor; masked; the out-projection merges the partials; byte lo plane; LDS-DMA attention
 * kernel; the range flag; the GEMM family of the out_proj block's and of the linear2 block's arithmetic (-1 where a split-fp16 plan does
 * not apply); the exact-fp32 attention kernel packs several short sequences into a wave ("attn_pack").  Returns as a denoise call does when the flag is set. */
#define JMID_DBG_LAYER_WIDTH(d_model, d_ff) (7 * (d_model) + (d_ff))
#define JMID_DBG_LAYER_PLAN_WORDS 25
int jmid_dbg_layer(jmid_handle_t h, int E, int A, int K, int T, int layer, int precision, const float* X, const int32_t* n_agents, int last,
                   float* hi, float* lo, int* plan);
/* The raw Philox words behind jmid_noise_fill, same addressing: out [E, rows, T, 2] uint32 (where `mem` says). */
int jmid_dbg_noise_words(jmid_handle_t h, uint64_t seed, int E, int rows, int T, const uint32_t* episode_ids, int draw, uint32_t* out, int mem);
#endif /* JMID_DIAGNOSTICS */

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* JMID_HIP_H */
