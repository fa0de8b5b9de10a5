/*
 * svgd_capi.h -- C-ABI boundary of the MI355X-native SVGD inner step.
 *
 * This is the drop-in boundary for the reference's hot path
 * (khaiyichin/SVGDCpp, paths relative to the reference root):
 *
 *   SVGD::Step            include/SVGDCpp/SVGD.hpp:373-400   -> svgd_step / svgd_begin_step+svgd_finish_step
 *   SVGD::ComputePhi      include/SVGDCpp/SVGD.hpp:407-454   -> svgd_phi
 *   GaussianRBFKernel::Step/ComputeScale/ComputeMedian
 *                         include/SVGDCpp/Kernel/GaussianRBFKernel.hpp:141-156,164-188,222-254
 *                                                            -> svgd_median_scale
 *   Kernel::EvaluateKernel/EvaluateKernelGrad (RBF lambda :75-81)
 *                         include/SVGDCpp/Kernel/Kernel.hpp:279-297 -> fused inside svgd_phi
 *   Optimizer::Initialize/Step  Adam.hpp:61-83, AdaGrad.hpp:49-65, RMSProp.hpp:58-74
 *                                                            -> svgd_set_optimizer / svgd_reset_optimizer
 *   bounds setup/clamp    include/SVGDCpp/SVGD.hpp:184-216,396-399 -> svgd_set_bounds
 *   coordinate matrix     std::shared_ptr<Eigen::MatrixXd> (SVGD.hpp:494) -> svgd_set_particles / svgd_get_particles
 *
 * Conventions
 *  - Plain C types only.  Host buffers are caller-owned and only touched
 *    during the call.  Particle matrices use the reference's layout: a
 *    d x n column-major Eigen matrix, i.e. particle i occupies
 *    X[i*d .. i*d+d-1] (doubles).
 *  - A context owns all device memory and one HIP stream; it is driven by a
 *    single host thread.
 *  - Multi-GPU: one process (context) per GPU.  Particles are sharded by
 *    contiguous rows (svgd_shard); per step the context all-gathers the
 *    coordinates and log-gradients over RCCL and all-reduces the median
 *    counts.  Every rank must make the same sequence of calls.
 *  - Errors: every int-returning function returns SVGD_OK (0) or a negative
 *    SVGD_ERR_* code; svgd_last_error() gives the message, already prefixed
 *    "SVGDCpp: " like the reference's exceptions (Exceptions.hpp:16-56).
 */
#ifndef SVGDCPP_AMD_SVGD_CAPI_H
#define SVGDCPP_AMD_SVGD_CAPI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ----- return codes (mapped onto the reference's exception types by the
 *       C++ shim include/SVGDCpp/SVGD.hpp) ------------------------------ */
#define SVGD_OK 0
#define SVGD_ERR_DIM -1     /* DimensionMismatchException (SVGD.hpp:172,195,207) */
#define SVGD_ERR_UNSET -2   /* UnsetException (GaussianRBFKernel.hpp:57) */
#define SVGD_ERR_ARG -3     /* std::invalid_argument (SVGD.hpp:225-235, Adam.hpp:47) */
#define SVGD_ERR_HIP -4     /* HIP runtime failure -> std::runtime_error */
#define SVGD_ERR_RCCL -5    /* RCCL failure        -> std::runtime_error */
#define SVGD_ERR_RUNTIME -6 /* other runtime error -> std::runtime_error */

/* compute dtype of the device path (host I/O is always double).  F32 runs the
 * O(N^2) work -- median distances, kernel values, phi contraction -- on the
 * fp32 MFMA tile kernels (v_mfma_f32_16x16x4f32, v_exp_f32) for every d; the
 * O(N d) work (centring, phi epilogue, optimizer, clamp) stays fp64.  The
 * median is the exact order statistic of the fp32 distances. */
#define SVGD_F64 0
#define SVGD_F32 1

/* optimizer kinds (Optimizer/Adam.hpp, AdaGrad.hpp, RMSProp.hpp) */
#define SVGD_OPT_ADAM 0
#define SVGD_OPT_ADAGRAD 1
#define SVGD_OPT_RMSPROP 2

/* kernel scale methods (GaussianRBFKernel::ScaleMethod, GaussianRBFKernel.hpp:25-30).
 * SVGD_SCALE_FIXED is an extension: M = a*I with a user-set a (the
 * reference's "TODO: constant scale"; used by the test_svgd scenario). */
#define SVGD_SCALE_MEDIAN 0
#define SVGD_SCALE_HESSIAN 1 /* M = sum_i -hess log p(x_i) / (2 d N), GaussianRBFKernel.hpp:189-210 */
#define SVGD_SCALE_FIXED 2
#define SVGD_SCALE_MATRIX 3  /* extension: a fixed full (SPD) scale matrix M */

/* median path taken by the last svgd_median_scale / step (diagnostics) */
#define SVGD_MEDIAN_DIRECT 0   /* all pair keys stored and selected exactly */
#define SVGD_MEDIAN_BRACKET 1  /* sampled bracket + candidate selection (exact) */
#define SVGD_MEDIAN_FALLBACK 2 /* bracket missed: streamed radix select (exact) */
#define SVGD_MEDIAN_REBRACKET 3 /* bracket missed: wider bracket, collect again (exact) */

typedef struct svgd_ctx svgd_ctx;

/* ---- lifetime ---------------------------------------------------------- */

/* Single-GPU context for `dim`-dimensional particles, n of them, on HIP
 * device `device`.  Replaces SVGD's constructor allocations (SVGD.hpp:151-250). */
int svgd_create(svgd_ctx **out, int dim, int64_t n, int dtype, int device);

/* Multi-GPU context: rank `rank` of `world`, all ranks passing the same
 * 128-byte RCCL unique id (from svgd_get_unique_id on one rank, broadcast by
 * the caller by any means). */
int svgd_create_dist(svgd_ctx **out, int dim, int64_t n, int dtype, int device,
                     int world, int rank, const void *unique_id128);
int svgd_get_unique_id(void *unique_id128);
/* Measurement only (not a drop-in call): a one-GPU context that runs rank 0's
 * share of a `sim_world`-rank step -- its rows of phi and the update, its
 * share of the median's pair tiles (order statistics re-anchored inside its
 * own candidates), the host gradient on the threads one rank of sim_world
 * would get -- with no collectives, to time the per-rank work of a P-GPU run
 * on one GPU.  Its results are not the step's: svgd_get_particles,
 * svgd_get_shard, svgd_median_scale and svgd_phi return SVGD_ERR_RUNTIME, and
 * svgd_get_diagnostics reports SIM_WORLD. */
int svgd_create_sim(svgd_ctx **out, int dim, int64_t n, int dtype, int device, int sim_world);
int svgd_destroy(svgd_ctx *ctx);
const char *svgd_last_error(const svgd_ctx *ctx);

/* Rows [*row0, *row1) of the particle matrix owned by this context. */
int svgd_shard(const svgd_ctx *ctx, int64_t *row0, int64_t *row1);

/* ---- plugins ------------------------------------------------------------ */

/* Adam(lr, beta1, beta2, eps) | AdaGrad(lr, eps) | RMSProp(lr, beta=beta1, eps).
 * Argument checks and messages follow Adam.hpp:45-48, RMSProp.hpp:42-45. */
int svgd_set_optimizer(svgd_ctx *ctx, int kind, double lr, double beta1, double beta2,
                       double eps);
/* Optimizer::Initialize (zero moments, counter = 0). */
int svgd_reset_optimizer(svgd_ctx *ctx);
/* d-vector bounds; both NULL = unbounded (SVGD.hpp:184-190). */
int svgd_set_bounds(svgd_ctx *ctx, const double *lower_d, const double *upper_d);
/* SVGD_SCALE_MEDIAN (default) or SVGD_SCALE_FIXED with M = fixed_a * I. */
int svgd_set_scale(svgd_ctx *ctx, int method, double fixed_a);

/* Full-matrix kernel scale k(x, x') = exp(-(x-x')^T M (x-x')) (the
 * reference's M = kernel_parameters_[0], GaussianRBFKernel.hpp:75-81):
 *  - svgd_set_scale_matrix: a fixed symmetric positive-definite M (d x d,
 *    row-major); selects SVGD_SCALE_MATRIX.
 *  - SVGD_SCALE_HESSIAN (svgd_set_scale): every step, between
 *    svgd_begin_step and svgd_finish_step, the caller passes
 *    sum_{i in its shard} -hess log p(x_i) (d x d); the context sums it over
 *    ranks and uses M = sum / (2 d N) for that step (:189-210).
 *  The phi kernels run on z = L^T x (M = L L^T) with V_j = G_j - 2 M x_j.
 *  svgd_get_scale_matrix returns the M of the last step (a I for the
 *  isotropic methods); SVGD_ERR_RUNTIME if M was not positive definite. */
int svgd_set_scale_matrix(svgd_ctx *ctx, const double *M);
int svgd_set_step_hessian_sum(svgd_ctx *ctx, const double *H_shard_sum);
int svgd_get_scale_matrix(svgd_ctx *ctx, double *M_out);

/* ---- particles ---------------------------------------------------------- */

/* Full n x d matrix (every rank passes the full matrix). */
int svgd_set_particles(svgd_ctx *ctx, const double *X);
/* Full n x d matrix (collective in multi-GPU mode). */
int svgd_get_particles(svgd_ctx *ctx, double *X);
/* This rank's rows only ((row1-row0) x d). */
int svgd_get_shard(svgd_ctx *ctx, double *X_shard);

/* ---- the hot path ------------------------------------------------------- */

/* a = ln(n)/med^2 of the current particles (GaussianRBFKernel.hpp:168-188).
 * Either output may be NULL.  Collective in multi-GPU mode. */
int svgd_median_scale(svgd_ctx *ctx, double *a_out, double *med_out);

/* phi_hat for this rank's rows given this rank's rows of G = grad log p and
 * the scale a (SVGD.hpp:407-454).  phi_shard_out may be NULL (device only). */
int svgd_phi(svgd_ctx *ctx, const double *G_shard, double a, double *phi_shard_out);

/* One SVGD::Step (SVGD.hpp:373-400): scale from X_t, phi_hat from G_shard
 * (= grad log p at this rank's rows of X_t), optimizer increment, clamp.
 * X stays device-resident. */
int svgd_step(svgd_ctx *ctx, const double *G_shard);

/* Split step for overlapping the host log-gradient with the device median:
 * begin launches the scale computation and copies this rank's rows of X_t
 * into X_shard_out (returns once that copy is done; may be NULL); the caller
 * evaluates G there and passes it to finish. */
int svgd_begin_step(svgd_ctx *ctx, double *X_shard_out);
int svgd_finish_step(svgd_ctx *ctx, const double *G_shard);

/* Context-owned page-locked host buffers of (row1-row0) x d doubles.
 * Passing them to svgd_begin_step / svgd_finish_step avoids a staging copy. */
int svgd_host_buffers(svgd_ctx *ctx, double **x_shard, double **g_shard);

/* Block until all work queued by the context is complete. */
int svgd_sync(svgd_ctx *ctx);

/* ---- diagnostics / measurement ----------------------------------------- */

/* Scale a and median of the last step (host copies). */
int svgd_last_scale(const svgd_ctx *ctx, double *a_out, double *med_out, int *median_path);
/* The two upper-list order statistics (squared distances) the last median
 * averaged, and their ranks among the n(n-1)/2 upper-triangle distances
 * (svgd_plan_median_ranks; rank -1 = a diagonal zero, value 0).  For
 * size-independent rank checks of the selection at full size. */
int svgd_last_median_keys(svgd_ctx *ctx, double *sq_lo, double *sq_hi, int64_t *rank_lo,
                          int64_t *rank_hi);
/* HIP-event timing on the context stream.  level 1: the phi phase (median
 * end -> record prep .. reduce + update) and the median phase (previous phi
 * end -> scale final), with events only at phase boundaries; get returns the
 * accumulated milliseconds and the phi-phase count (and resets them).
 * level 2 adds the diagnostic events read by svgd_get_diagnostics -- the phi
 * kernel alone, the device's wait between the median's end and the phi chain,
 * every collective -- each one a ~5 us dispatch gap (a diagnostic pass, not
 * the timed one).  0 disables. */
int svgd_set_timing(svgd_ctx *ctx, int level);
int svgd_get_timing(svgd_ctx *ctx, double *phi_ms, double *median_ms, int64_t *count);
/* Accumulated diagnostics since the last call (then reset); writes
 * min(cap, SVGD_DIAG_LEN) doubles, returns that count or an error:
 *   STEPS            svgd_step_host_model calls
 *   PHI_KERNEL_MS/N  phi kernel alone (k_phi_rows without its reduce, or the
 *                    tile kernel), HIP events (level 2)
 *   PHI_WAIT_MS/N    device idle between the median's end and the phi chain:
 *                    waiting for the host gradient / G copies / G all-gather (level 2)
 *   COLL_MS/N        collectives on the compute stream (level 2, P > 1)
 *   GATHER_G_MS/N    the G all-gather on its own stream (level 2, P > 1)
 *   HOST_GRAD_MS     host grad log p wall time (worker thread, all chunks)
 *   HOST_XWAIT_MS    worker waiting for X_t chunk copies
 *   HOST_JOB_MS      worker job: post -> last G chunk landed
 *   HOST_WAIT_MS     calling thread waiting for the worker after queuing the median
 *   RANKS            ranks in the communicator (1 without one)
 *   HOST_THREADS     OpenMP threads of the host gradient
 *   TRK_STEPS        speculative steps whose median bracket was predicted from
 *                    the previous steps' medians (no sample, no bracket passes)
 *   TRK_MISS         of those, steps redone because the bracket missed
 *   SIM_WORLD        simulated world of a measurement context (svgd_create_sim), else 1
 *   CPU_QUOTA        CPUs of the cgroup quota (0: none); a rank's gradient
 *                    threads are at most CPU_QUOTA / world (or / SIM_WORLD)
 *   SPLIT_STEPS      steps whose phi + update ran in two row parts (the first
 *                    part's X_{t+1} feeding the next host gradient early)
 *   MIRROR_STEPS     host-model steps whose gradient read X_t from the
 *                    update's pinned mirror instead of a copy
 *   SPEC_STEPS       steps whose median took the speculative device plan
 *   G_COMM           1 if the G all-gather has its own communicator and stream */
#define SVGD_DIAG_STEPS 0
#define SVGD_DIAG_PHI_KERNEL_MS 1
#define SVGD_DIAG_PHI_KERNEL_N 2
#define SVGD_DIAG_PHI_WAIT_MS 3
#define SVGD_DIAG_PHI_WAIT_N 4
#define SVGD_DIAG_COLL_MS 5
#define SVGD_DIAG_COLL_N 6
#define SVGD_DIAG_GATHER_G_MS 7
#define SVGD_DIAG_GATHER_G_N 8
#define SVGD_DIAG_HOST_GRAD_MS 9
#define SVGD_DIAG_HOST_XWAIT_MS 10
#define SVGD_DIAG_HOST_JOB_MS 11
#define SVGD_DIAG_HOST_WAIT_MS 12
#define SVGD_DIAG_RANKS 13
#define SVGD_DIAG_HOST_THREADS 14
#define SVGD_DIAG_TRK_STEPS 15
#define SVGD_DIAG_TRK_MISS 16
#define SVGD_DIAG_SIM_WORLD 17
#define SVGD_DIAG_CPU_QUOTA 18
#define SVGD_DIAG_SPLIT_STEPS 19
#define SVGD_DIAG_MIRROR_STEPS 20
#define SVGD_DIAG_SPEC_STEPS 21
#define SVGD_DIAG_G_COMM 22
#define SVGD_DIAG_TRK_BAND 23 /* sum over tracked steps of the predicted bracket's share of the pairs */
#define SVGD_DIAG_LEN 24
int svgd_get_diagnostics(svgd_ctx *ctx, double *out, int cap);
/* Name and template arguments of the phi kernel this context launches, as
 * rocprofv3 prints them (e.g. "k_phi_rows<8, 4, 8, 8192, 8>"): the key under
 * which committed PMC profiles of that kernel are matched (bench.py).  The
 * kernel is planned at creation (svgd_plan_phi_name gives the same answer
 * without a context); a full-matrix scale set afterwards does not change the
 * name, which stays the isotropic-scale kernel's. */
int svgd_phi_kernel_name(const svgd_ctx *ctx, char *buf, int cap);
/* Median tuning knobs (tests force each path): pair count at or below which
 * all keys are stored (direct path), sample size, candidate capacity.
 * Values <= 0 keep the current setting. */
int svgd_set_median_tuning(svgd_ctx *ctx, int64_t direct_max_pairs, int64_t sample_size,
                           int64_t candidate_capacity);
/* Upper-triangle squared-distance keys exactly as the device median sees
 * them, in (i<j) row-major order; n(n-1)/2 doubles (small n only). */
int svgd_debug_pair_keys(svgd_ctx *ctx, double *out, int64_t capacity);

/* ---- host-side built-in models (no GPU needed) ---------------------------
 * The target density's log-gradient stays on the host, as in the reference
 * (Model::EvaluateLogModelGrad, include/SVGDCpp/Model/Model.hpp:335-338).
 * A model here is the sum of `ncomp` unnormalised Gaussians
 * exp(-1/2 (x-mu_c)^T cov_c^-1 (x-mu_c)): ncomp = 1 is MultivariateNormal
 * (MultivariateNormal.hpp:56-61), ncomp > 1 the reference's operator+
 * composition (Model.hpp:55-92).  mus: ncomp x dim, covs: ncomp x dim x dim. */
int svgd_model_create(void **model, int dim, int ncomp, const double *mus, const double *covs);
int svgd_model_destroy(void *model);
/* G[i] = grad log p(X[i]) for nrows particles (OpenMP over rows). */
int svgd_model_logp_grad(void *model, const double *X, int64_t nrows, double *G);
/* H = sum_i -hess log p(x_i) over nrows particles (d x d, row-major): the sum
 * of the Hessian scale (GaussianRBFKernel.hpp:197-205, Model.hpp:366-370). */
int svgd_model_neg_hess_sum(void *model, const double *X, int64_t nrows, double *H);

/* One SVGD::Step (SVGD.hpp:373-400) with grad log p from a host model
 * (svgd_model_create; Model::EvaluateLogModelGrad, Model.hpp:335-338,
 * evaluated per particle as SVGD.hpp:412-416 does): svgd_begin_step +
 * svgd_model_logp_grad + svgd_finish_step with the X_t copy, the host
 * gradient and the G upload pipelined in row chunks (chunk i's gradient
 * overlaps chunk i+1's copy down and chunk i-1's copy up), so the whole host
 * round trip hides behind the device median.  Same result as the split
 * calls.  Not for SVGD_SCALE_HESSIAN (that step also needs the caller's
 * Hessian sum).  On a shard of <= 1 MiB the previous update's epilogue
 * leaves X_t in a context-private pinned buffer instead of a copy
 * (SVGD_X_MIRROR=0 disables it): the buffers of svgd_host_buffers are then
 * not guaranteed to hold X_t afterwards. */
int svgd_step_host_model(svgd_ctx *ctx, const void *model);

/* Mirror a built-in Gaussian-sum model (svgd_model_create) on the device
 * (MultivariateNormal.hpp:56-61, Model.hpp:55-92):
 * afterwards svgd_step(ctx, NULL) evaluates grad log p on the device and the
 * whole step stays in HBM.  NULL removes it.  d <= 64. */
int svgd_set_device_model(svgd_ctx *ctx, const void *model);
/* grad log p of the device model at the current particles, this rank's rows
 * (shard layout like svgd_get_shard). */
int svgd_device_logp_grad(svgd_ctx *ctx, double *G_shard_out);

/* ---- generalized linear model posterior (extension) ----------------------
 * Bayesian logistic / linear regression on data A (m x dim, row-major) and
 * y (m), prior N(0, I / prior_prec), for theta = one particle:
 *   z_j   = a_j . theta
 *   log p = s (m/B) sum_j l(y_j, z_j) - (prior_prec / 2) |theta|^2
 *   grad  = s (m/B) sum_j r(y_j, z_j) a_j - prior_prec theta
 *   SVGD_GLM_LOGISTIC  l = y z - log(1 + e^z),  r = y - sigma(z),  y in [0, 1]
 *   SVGD_GLM_GAUSSIAN  l = -(y - z)^2 / 2,      r = y - z
 * s = lik_scale > 0 (the 1/sigma^2 of the Gaussian link, or a tempering
 * factor); the sums run over the batch window [m0, m0 + B) of the data rows
 * (all m rows until svgd_glm_set_batch), scaled by m / B.  The data are
 * copied.  Refused: NULL pointers, an unknown link, non-finite data,
 * logistic labels outside [0, 1], s <= 0, prior_prec < 0 (SVGD_ERR_ARG);
 * dim < 1 or m < 1 (SVGD_ERR_DIM). */
#define SVGD_GLM_LOGISTIC 0
#define SVGD_GLM_GAUSSIAN 1
int svgd_glm_create(void **model, int dim, int64_t m, const double *A, const double *y, int link,
                    double lik_scale, double prior_prec);
int svgd_glm_destroy(void *model);
/* The batch window [m0, m0 + count) of the data rows; SVGD_ERR_ARG unless
 * m0 >= 0, count >= 1 and m0 + count <= m.  (The caller shuffles its data
 * once and moves the window: there is no random selection here.) */
int svgd_glm_set_batch(void *model, int64_t m0, int64_t count);
/* out[i] = log p(X[i]) for nrows particles (OpenMP over rows). */
int svgd_glm_logp(void *model, const double *X, int64_t nrows, double *out);
/* G[i] = grad log p(X[i]) for nrows particles (OpenMP over rows; each row's
 * sum in data order, so the result does not depend on the thread count). */
int svgd_glm_logp_grad(void *model, const double *X, int64_t nrows, double *G);
/* H = sum_i -hess log p(x_i) over nrows particles (d x d, row-major), the
 * sum of the Hessian scale: sum_i [ s (m/B) sum_j w_ij a_j a_j^T +
 * prior_prec I ], w = sigma (1 - sigma) (logistic) or 1 (Gaussian). */
int svgd_glm_neg_hess_sum(void *model, const double *X, int64_t nrows, double *H);
/* Mirror a GLM (svgd_glm_create) on the device: the data are uploaded once
 * (every rank holds all m rows; only particles are sharded) and the model's
 * current batch window is taken over.  Afterwards svgd_step(ctx, NULL),
 * svgd_device_logp_grad and svgd_ksd(ctx, NULL, ...) evaluate grad log p on
 * the device, in fp64 whatever the context's dtype; two calls on the same
 * state return the same bits.  A context holds one device model: this call
 * removes a Gaussian-sum mirror and svgd_set_device_model removes this one.
 * NULL removes it.  d <= 64. */
int svgd_set_device_glm(svgd_ctx *ctx, const void *glm);
/* Move the device GLM's batch window (no data is copied); SVGD_ERR_UNSET
 * without a device GLM, SVGD_ERR_ARG for a window outside the data. */
int svgd_set_device_glm_batch(svgd_ctx *ctx, int64_t m0, int64_t count);
/* H_shard_out (dim x dim, row-major) = sum_i -hess log p(x_i) of the device
 * model (either kind) over this rank's rows of the current particles: what
 * svgd_glm_neg_hess_sum / svgd_model_neg_hess_sum return for those rows,
 * computed on the device in fp64 whatever the context's dtype.  An empty
 * shard gives zeros; a GLM's result is exactly symmetric; two calls on the
 * same state return the same bits.  An observer like svgd_device_logp_grad.
 * SVGD_ERR_UNSET without a device model, SVGD_ERR_ARG for NULL. */
int svgd_device_neg_hess_sum(svgd_ctx *ctx, double *H_shard_out);
/* on != 0: under SVGD_SCALE_HESSIAN, svgd_step(ctx, NULL) takes the step's
 * Hessian sum from the device model -- the sum above, computed straight into
 * the scale's source and summed over the ranks where
 * svgd_set_step_hessian_sum would do it, with no host copy; every rank must
 * set the switch alike.  A sum supplied for the step with
 * svgd_set_step_hessian_sum wins (a kernel whose target model is not the
 * stepped one).  Off (the default): that step fails with the Unset Error, as
 * before.  Harmless under the other scale methods; svgd_set_device_model and
 * svgd_set_device_glm leave the switch alone. */
int svgd_set_device_hessian(svgd_ctx *ctx, int on);

/* Posterior prediction of a GLM on held-out rows a_j (A: m x dim, row-major)
 * and optional labels y_j, over all N particles theta_i (z_ij = a_j . theta_i,
 * mu = sigma for SVGD_GLM_LOGISTIC and the identity for SVGD_GLM_GAUSSIAN):
 *   mean_j = (1/N) sum_i mu(z_ij)
 *   var_j  = (1/N) sum_i (mu(z_ij) - mean_j)^2     (>= 0: the spread over the particles)
 *   lpd_j  = log (1/N) sum_i p(y_j | z_ij)          (only with y)
 *     logistic  p = exp(y z - log(1 + e^z))         (y in [0, 1]; lik_scale is not used)
 *     Gaussian  p = sqrt(s / 2 pi) exp(-s (y - z)^2 / 2),  s = lik_scale
 * The sums are centred on mu(a_j . theta_bar), theta_bar the particles' mean,
 * so var does not cancel.  The likelihood sum is not shifted: a record whose
 * likelihood underflows at every particle gives lpd = -inf.  y may be NULL
 * and any output may be NULL; lpd_out without y is SVGD_ERR_ARG.  Refused:
 * NULL A, an unknown link, non-finite data, logistic labels outside [0, 1],
 * lik_scale <= 0 (SVGD_ERR_ARG); m < 1, dim < 1 or nrows < 1 (SVGD_ERR_DIM).
 *
 * host, no GPU: particles X (nrows x dim), OpenMP over records, each record's
 * sums in particle order (independent of the thread count) */
int svgd_glm_predict_host(int link, double lik_scale, int dim, const double *A, const double *y,
                          int64_t m, const double *X, int64_t nrows,
                          double *mean_out, double *var_out, double *lpd_out);
/* device: the context's current particles; collective in multi-GPU mode, every
 * rank passes the same test data and gets the same m-vectors.  Needs no
 * device model; fp64 whatever the context's dtype; two calls on the same
 * state return the same bits.  A pure observer like svgd_ksd.  d <= 64. */
int svgd_glm_predict(svgd_ctx *ctx, int link, double lik_scale, const double *A, const double *y,
                     int64_t m, double *mean_out, double *var_out, double *lpd_out);

/* Kernelized Stein discrepancy of the current particles with the isotropic
 * RBF kernel k = exp(-a |x - y|^2), whatever scale method the context steps
 * with.  For s_i = grad log p(x_i), r = x_i - x_j:
 *   u_ij   = k_ij [ s_i.s_j + 2a (s_i - s_j).r + 2ad - 4a^2 |r|^2 ]
 *   row_i  = (1/N) sum_j u_ij
 *   KSD2_V = (1/N) sum_i row_i                     (V-statistic, >= 0)
 *   KSD2_U = (1/(N(N-1))) sum_{i != j} u_ij        (U-statistic; NaN for N < 2)
 * G_shard: this rank's rows of grad log p at the current particles, as for
 * svgd_phi; NULL evaluates the device model (svgd_set_device_model).  Any
 * output may be NULL; rows_shard_out takes this rank's row_i.  fp64 for
 * SVGD_F32 contexts too; two calls on the same state return the same bits.
 * A pure observer: particles, optimizer state, the last scale and the
 * median's history are left as they were.  Collective in multi-GPU mode
 * (every rank gets the same two scalars). */
int svgd_ksd(svgd_ctx *ctx, const double *G_shard, double a, double *ksd2_v, double *ksd2_u,
             double *rows_shard_out);

/* ---- inverse multiquadric kernel (extension) ------------------------------
 *   k(x, x')  = (1 + a |x - x'|^2)^(-1/2)              a >= 0 (a = 0: k = 1)
 *   grad_x' k = -a (x' - x) k^3
 *   phi_i     = (1/N) sum_j [ k_ij G_j + a k_ij^3 (x_i - x_j) ]   (SVGD.hpp:407-454 with this kernel)
 * The exponent -1/2 and the offset 1 are fixed.  a comes from the scale
 * methods above: SVGD_SCALE_MEDIAN (a = ln N / med^2, the same median) or
 * SVGD_SCALE_FIXED.  SVGD_SCALE_HESSIAN and SVGD_SCALE_MATRIX with the IMQ
 * kernel are refused with SVGD_ERR_ARG, whichever of the two calls comes
 * second.
 *
 * svgd_set_kernel chooses the kernel of svgd_phi and of every step call of
 * this context (every rank alike); the default is SVGD_KERNEL_RBF.  With
 * SVGD_KERNEL_IMQ, phi_hat is computed in fp64 whatever the context's dtype
 * (the median stays the dtype's), the optimizer update is a launch of its
 * own, and two calls on the same state return the same bits.
 * svgd_phi_kernel_name reports the IMQ pass while it is set.  svgd_ksd stays
 * the RBF statistic whatever kernel is set; svgd_ksd_kernel (below) gives the
 * IMQ one.  d <= 64. */
#define SVGD_KERNEL_RBF 0
#define SVGD_KERNEL_IMQ 1
int svgd_set_kernel(svgd_ctx *ctx, int kind);
int svgd_get_kernel(const svgd_ctx *ctx, int *kind);

/* Kernelized Stein discrepancy with the kernel named in the call, whatever
 * kernel the context steps with (svgd_set_kernel neither reads nor is read
 * by it).  SVGD_KERNEL_RBF is svgd_ksd itself: the same code, the same bits.
 * SVGD_KERNEL_IMQ: with q = 1 + a |r|^2, k = q^(-1/2), r = x_i - x_j,
 *   u_ij   = k s_i.s_j + a k^3 (s_i - s_j).r + a d k^3 - 3 a^2 k^5 |r|^2
 *   u_ii   = |s_i|^2 + a d
 * and row_i, KSD2_V, KSD2_U as for svgd_ksd (Gorham & Mackey 2017 with
 * beta = -1/2, c = 1).  The contract is svgd_ksd's: G_shard == NULL evaluates
 * the device model, any output may be NULL, fp64 whatever the dtype, equal
 * bits on equal state, a pure observer with work arrays of its own
 * (allocated by the first IMQ call), collective in multi-GPU mode.  a must be
 * finite and > 0 and the kernel one of the two (SVGD_ERR_ARG).  d <= 64. */
int svgd_ksd_kernel(svgd_ctx *ctx, int kernel, const double *G_shard, double a, double *ksd2_v,
                    double *ksd2_u, double *rows_shard_out);
/* host, no GPU: the same two statistics of X (n x dim) with scores G
 * (n x dim) by direct differences (no centring, no Gram form); rows_out
 * (n, may be NULL) takes row_i.  OpenMP over rows, each row's sum in particle
 * order and the sums over rows in row order (independent of the thread
 * count).  Refused: NULL X or G, an unknown kernel, a not finite or <= 0
 * (SVGD_ERR_ARG); dim < 1 or n < 1 (SVGD_ERR_DIM). */
int svgd_ksd_host(int kernel, int dim, int64_t n, const double *X, const double *G, double a,
                  double *ksd2_v, double *ksd2_u, double *rows_out);
/* Maximum mean discrepancy (Gretton et al. 2012) between the particles X
 * (N x dim, all ranks) and the caller's sample Y (m x dim, row-major like the
 * particle rows), with the kernel named in the call and the scale a > 0:
 *   SVGD_KERNEL_RBF  k = exp(-a |x - y|^2)
 *   SVGD_KERNEL_IMQ  k = (1 + a |x - y|^2)^(-1/2)
 *   Sxx = sum_{i,j<N} k(x_i, x_j),  Syy = sum_{i,j<m} k(y_i, y_j)   (the diagonal counts 1 each)
 *   Sxy = sum_{i<N} sum_{j<m} k(x_i, y_j)
 *   mean_xx = Sxx / N^2,  mean_yy = Syy / m^2,  mean_xy = Sxy / (N m)
 *   MMD2_V  = mean_xx + mean_yy - 2 mean_xy                      (biased, >= 0 up to rounding)
 *   MMD2_U  = (Sxx - N) / (N (N - 1)) + (Syy - m) / (m (m - 1)) - 2 mean_xy   (NaN if N < 2 or m < 2)
 *   wit_i   = (1/N) sum_j k(x_i, x_j) - (1/m) sum_j k(x_i, y_j)
 * means3_out = [mean_xx, mean_yy, mean_xy]; witness_shard_out (this rank's
 * rows, shard layout like svgd_get_shard) takes wit_i, the witness function
 * at particle i: positive where the particles are over-dense relative to Y.
 * Any output may be NULL.  The contract is svgd_ksd_kernel's: fp64 whatever
 * the dtype, blind to svgd_set_kernel, equal bits on equal state, a pure
 * observer with work arrays of its own (allocated by the first call, grown
 * when a later m needs it).  Collective in multi-GPU mode: every rank passes
 * the same Y and gets the same scalars and means.  SVGD_ERR_ARG: NULL Y, an
 * unknown kernel, a not finite or <= 0, a non-finite value in Y;
 * SVGD_ERR_DIM: m < 1.  d <= 64. */
int svgd_mmd(svgd_ctx *ctx, int kernel, const double *Y, int64_t m, double a, double *mmd2_v, double *mmd2_u,
             double *means3_out, double *witness_shard_out);
/* host, no GPU: the same quantities of X (n x dim) and Y (m x dim) by direct
 * differences (no centring, no Gram form); witness_out (n, may be NULL) takes
 * wit_i.  OpenMP over rows, each row's sum in column order and the sums over
 * rows in row order (independent of the thread count).  Refused: NULL X or Y,
 * an unknown kernel, a not finite or <= 0, a non-finite value in Y
 * (SVGD_ERR_ARG); dim < 1, n < 1 or m < 1 (SVGD_ERR_DIM). */
int svgd_mmd_host(int kernel, int dim, int64_t n, const double *X, int64_t m, const double *Y, double a,
                  double *mmd2_v, double *mmd2_u, double *means3_out, double *witness_out);
/* Stein thinning (Riabiz et al. 2022): the greedy choice of m of the current
 * particles whose empirical measure has the smallest KSD under the kernel
 * named in the call, with u_ij and u_ii as above for svgd_ksd /
 * svgd_ksd_kernel (u_ii = |s_i|^2 + 2ad for the RBF kernel):
 *   acc_0[j] = 0
 *   for t = 1..m:
 *     obj_t[j] = u_jj / 2 + acc_{t-1}[j]              j = 0..N-1
 *     pi_t     = the smallest j that attains min_j obj_t[j]
 *     S_t      = S_{t-1} + 2 acc_{t-1}[pi_t] + u_{pi_t pi_t}      (S_0 = 0)
 *     ksd2_t   = S_t / t^2        (= KSD2_V of the multiset {pi_1..pi_t})
 *     acc_t[j] = acc_{t-1}[j] + u(pi_t, j)            (u(pi_t, pi_t) by index)
 * Picks may repeat, so m may exceed N.  idx_out (m, may be NULL) takes the
 * global row indices in pick order, ksd2_out (m, may be NULL) the ksd2_t.
 * The contract is svgd_ksd_kernel's: G_shard == NULL evaluates the device
 * model, fp64 whatever the dtype, blind to svgd_set_kernel, equal bits on
 * equal state, a pure observer with work arrays of its own (allocated by the
 * first call, grown when a later m needs it).  Collective in multi-GPU mode:
 * each rank passes its rows of G, the selection runs on every rank on the
 * all-gathered X and G, and every rank gets the same m indices and values.
 * SVGD_ERR_ARG: an unknown kernel, a not finite or <= 0, m < 1, NULL G_shard
 * without a device model, d > 64.  SVGD_ERR_RUNTIME: a ksd2_t that is not
 * finite (the outputs are written). */
int svgd_stein_thin(svgd_ctx *ctx, int kernel, const double *G_shard, double a, int64_t m,
                    int64_t *idx_out, double *ksd2_out);
/* host, no GPU: the same selection of X (n x dim) with scores G (n x dim) by
 * direct differences, OpenMP over j inside a pick, the minimum compared in
 * index order (independent of the thread count).  Refused: NULL X or G, an
 * unknown kernel, a not finite or <= 0, m < 1 (SVGD_ERR_ARG); dim < 1 or
 * n < 1 (SVGD_ERR_DIM); SVGD_ERR_RUNTIME as above. */
int svgd_stein_thin_host(int kernel, int dim, int64_t n, const double *X, const double *G, double a,
                         int64_t m, int64_t *idx_out, double *ksd2_out);
/* host, no GPU: phi_out (nrows x dim) = phi_i of the definition above for the
 * rows [row0, row0 + nrows) of X (n x dim) with G (n x dim), by direct
 * differences; OpenMP over rows, each row's sums in particle order
 * (independent of the thread count).  Refused: NULL pointers, a < 0 or not
 * finite, a row window outside [0, n] (SVGD_ERR_ARG); dim < 1 or n < 1
 * (SVGD_ERR_DIM). */
int svgd_imq_phi_host(int dim, int64_t n, const double *X, const double *G, double a, int64_t row0,
                      int64_t nrows, double *phi_out);

/* ---- host-only planning helpers (no GPU needed) ------------------------ */

/* Row shard of rank r among `world` for n particles: equal chunks of
 * ceil(n/world) rows (trailing ranks may be short or empty). */
void svgd_plan_rows(int64_t n, int world, int rank, int64_t *row0, int64_t *row1);
/* The name svgd_phi_kernel_name reports for a context of `rank` among
 * `world` created with these arguments under the current environment (the
 * SVGD_PHI_* knobs): the same plan, made without a context or a GPU.
 * SVGD_ERR_DIM above dimension 64. */
int svgd_plan_phi_name(int dim, int64_t n, int dtype, int world, int rank, char *buf, int cap);
/* Full-list ranks of the median (GaussianRBFKernel.hpp:222-254 over the n^2
 * distance list incl. n diagonal zeros) mapped onto the ascending list of
 * the n(n-1)/2 upper-triangle distances.  Writes up to two upper-list ranks
 * (-1 = a diagonal zero) and returns how many order statistics are averaged
 * (2 for even n^2, 1 for odd). */
int svgd_plan_median_ranks(int64_t n, int64_t *rank_lo, int64_t *rank_hi);
/* Number of block-level tiles of the median pair sweep owned by rank r
 * (row blocks of `block` particles; each unordered pair of particles is
 * visited by exactly one rank), and the (row block, column block) of tile t
 * of that rank.  The device uses block = SVGD_PAIR_BLOCK(dim) for F64 and
 * SVGD_PAIR_BLOCK_DT(dim, dtype) in general (F32: always the 64 tile). */
#define SVGD_PAIR_BLOCK(dim) ((dim) <= 16 ? 256 : 64)
#define SVGD_PAIR_BLOCK_DT(dim, dtype) ((dtype) == SVGD_F32 ? 64 : SVGD_PAIR_BLOCK(dim))
int64_t svgd_plan_pair_tiles(int64_t n, int block, int world, int rank);
void svgd_plan_pair_tile(int64_t n, int block, int world, int rank, int64_t t,
                         int64_t *row_block, int64_t *col_block);
/* Symmetric phi pass units: the (tile, sub-tile) pairs of the tile plan
 * above (blocks of `block` rows, `nsub` sub-tiles of block / nsub columns
 * per tile) in order, without the last column block's sub-tiles that hold
 * padding columns only.  svgd_plan_sym_total: their number;
 * svgd_plan_sym_unit: tile and sub-tile of unit u (returns -1 past the end). */
int64_t svgd_plan_sym_total(int64_t n, int block, int nsub);
int svgd_plan_sym_unit(int64_t n, int block, int nsub, int64_t u, int64_t *tile, int64_t *q);
/* Symmetric phi pass (k_phi_sym) plan of rank r among `world`: its
 * units [*u0, *u1) (equal pair counts per rank),
 * run by `grid` work-groups in contiguous runs; per row block P (of
 * nb = ceil(n/block)) blkg[2P] .. blkg[2P+1] = the work-groups visiting it
 * (blkg[2P+1] < blkg[2P]: none) and rbase[P] = its first row-sum record;
 * *Ia .. *Ib = the row blocks the rank's units span.  blkg holds 2 nb ints,
 * rbase nb.  Returns the number of row-sum records.  (The pass replaces the
 * reference's ComputePhi, SVGD.hpp:407-454, for d <= 8.) */
int64_t svgd_plan_sym_units(int64_t n, int block, int nsub, int world, int rank, int grid,
                            int64_t *u0, int64_t *u1, int *blkg, int *rbase, int64_t *Ia, int64_t *Ib);
/* The sharded symmetric pass's exchange (replaces the parallel branch of
 * SVGD.hpp:410-432): the rows [*r0, *r1) of rank dst's shard (svgd_plan_rows)
 * that rank src's units can add to -- the row blocks its units span and the
 * column blocks they pair with (at most (nb - 1) / 2 + 1 ahead, cyclic),
 * intersected with dst's rows (the hull of at most two pieces; *r0 == *r1:
 * none).  src sends exactly this range of its per-particle sums to dst, dst
 * receives it from src; the two sides compute the same range.  src == dst:
 * the rank's own rows it contributes to. */
void svgd_plan_sym_exchange(int64_t n, int block, int nsub, int world, int src, int dst, int64_t *r0,
                            int64_t *r1);
/* Median bucket select: from the all-reduced histogram of candidate keys in
 * `nb` ascending key-range buckets, the bucket holding each of the `nsel`
 * (1 or 2) candidate ranks, the rank inside it, and the total count of the
 * distinct selected buckets (the keys a rank compacts and all-gathers).
 * Returns 0, or -1 if a rank lies past the counted candidates. */
int svgd_plan_bucket_select(const unsigned long long *counts, int nb, int nsel,
                            const int64_t *ranks, int *bsel, int64_t *rank_in, int64_t *total);
/* The median's host policy as the library runs it, without a context or a GPU.
 *
 * Tracked bracket: the next median of D^2 predicted from the last selected
 * ones.  A tracker (new: the half-width's multiple of the recent prediction
 * errors and its relative floor; NULL if out of memory) per trajectory;
 * restart forgets the history (new particles).  Per step: begin_step, then
 * predict -- 1 and the bracket [*lo_key, *hi_key) as key bit patterns, its
 * expected share *band of `pairs` pairs, the predicted D^2 *pred and the
 * relative half-width *width, or 0: sample the bracket (band_samp: the
 * sampled bracket's share, which the predicted one must not exceed) -- then
 * record with the step's selected keys (lower and upper order statistic; error
 * != 0: the selection failed or went another way, the history restarts), the
 * bracket they were selected from and its candidate count over all ranks. */
void *svgd_plan_tracker_new(double err_mult, double min_width);
void svgd_plan_tracker_free(void *tracker);
void svgd_plan_tracker_restart(void *tracker);
void svgd_plan_tracker_begin_step(void *tracker);
int svgd_plan_tracker_predict(void *tracker, double pairs, double band_samp, uint64_t *lo_key,
                              uint64_t *hi_key, double *band, double *pred, double *width);
void svgd_plan_tracker_record(void *tracker, uint64_t key_lo, uint64_t key_hi, int error,
                              uint64_t bracket_lo_key, uint64_t bracket_hi_key, uint64_t cand);
/* The bracket sample of a step over n particles: its size (the return value)
 * and *band_samp, its bracket's expected share of the pairs.  tile_kernels:
 * the median runs on the tile kernels (d > 16 or F32: whole 64 x 64 tiles are
 * drawn), else scattered pairs; forced: a set sample size (0: automatic);
 * multi: more than one rank shares the step; shard_sample: ranks draw
 * disjoint parts (SVGD_SAMPLE_SHARD); sim_world: svgd_create_sim's (else 1);
 * bracket_sigma: sample-quantile standard deviations either side. */
int64_t svgd_plan_median_sample(int64_t n, int tile_kernels, int64_t forced, int multi, int shard_sample,
                                int sim_world, double bracket_sigma, double *band_samp);
/* The sample ranks [*slo, *shi] bracketing the quantiles qlo <= qhi of a
 * sample of S keys, sigma standard deviations either side, and *band_est
 * (optional), the bracket's expected share of the pairs. */
void svgd_plan_sample_ranks(int64_t S, double qlo, double qhi, double sigma, int64_t *slo, int64_t *shi,
                            double *band_est);
/* Per-rank key capacity of a speculative step's segment after a selection
 * whose selected buckets held last_tot keys over all ranks. */
int64_t svgd_plan_spec_cap(int64_t last_tot);

#ifdef __cplusplus
}
#endif

#endif /* SVGDCPP_AMD_SVGD_CAPI_H */
