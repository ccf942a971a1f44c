/* bayesfilt.h -- C-ABI of the MI355X-native batched Bayesian-filtering engine.
 *
 * The reference (kostastsa/BayesianFiltering, package `gaussfiltax`) has no FFI/plugin
 * interface; its boundary for the filtering hot path is the Python call surface
 *
 *   gaussian_sum_filter(params, emissions, num_components, num_iter, inputs)
 *                                               gaussfiltax/inference.py:303-309
 *   bootstrap_particle_filter(params, emissions, num_particles, key, inputs, ess_threshold)
 *                                               gaussfiltax/inference.py:1302-1309
 *
 * Each entry point below replaces the `lax.scan` body of one of those drivers
 * (inference.py:333-371 and :1330-1377) for a whole batch of independent trajectories.
 * Conventions: extern "C", plain pointers and sizes, no exceptions; every function returns an
 * int status (0 = BF_OK, negative = BF_E*; text via bf_last_error()).  All array arguments
 * named `d_*` or carried in bf_stream/bf_cstream/bf_carry are DEVICE pointers owned by the
 * caller; the engine never allocates outputs.  Model parameter structs hold HOST pointers to
 * small row-major fp32 arrays which are copied into kernel arguments at launch.  `stream` is a
 * hipStream_t passed as void* (NULL = the default stream).  Launches are asynchronous: no entry point synchronises
 * the host with the stream (constant blocks are uploaded stream-ordered through a content-keyed cache and found
 * again on later calls, so a warmed-up call is also capturable into a hipGraph).
 *
 * Arithmetic is fp32 like the reference's JAX path (no jax_enable_x64 anywhere); the
 * reference's quirks are reproduced: update -> reweight -> predict order,
 * psd_solve = LU solve of (S + 1e-6 on every entry) (gaussfiltax/utils.py:256-259),
 * P+ = P - K S K^T with the un-jittered S, log-likelihood by Cholesky of the un-jittered S,
 * linear-domain weights.
 */
#ifndef BAYESFILT_H_
#define BAYESFILT_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BF_VERSION 210 /* 0.2.0: major = ABI revision (struct layouts), see bf_abi_check */

#define BF_OK 0
#define BF_EINVAL (-1)       /* bad argument (NULL pointer, non-positive size, misaligned) */
#define BF_EUNSUPPORTED (-2) /* dimension / model / option not compiled into this build  */
#define BF_EHIP (-3)         /* HIP runtime error (text in bf_last_error)                */
#define BF_ENOGPU (-4)       /* no gfx950 device visible                                 */

/* Strided view of an fp32 output stream.  Element (b, k, t, e) lives at
 *   ptr[b*sB + k*sK + t*sT + e*sE]      (strides in ELEMENTS)
 * where e indexes the row-major flattened event (vector entry i, or matrix entry i*n+j).
 * ptr == NULL: the stream is not emitted.  Two layouts have tuned kernels:
 *   "reference" [B][K][T][E] contiguous (sE = 1, sT = E, sK = T*E, sB = K*T*E): what the
 *       reference returns per trajectory after swap_axes_on_values (inference.py:372), with
 *       a leading batch axis;
 *   "batch-inner" [K][T][E][B] (sB = 1): the scan-native order, perfectly coalesced.
 * Any other stride set runs on the generic strided path. */
typedef struct bf_stream {
  float* ptr;
  int64_t sB, sK, sT, sE;
} bf_stream;

typedef struct bf_cstream {
  const float* ptr;
  int64_t sB, sK, sT, sE; /* sK unused for observations / inputs */
} bf_cstream;

/* The five arrays of PosteriorGaussianSumFiltered (inference.py:29-39, emitted at
 * :357-363) plus the per-step component log-likelihoods (the `lls` of :345, which the
 * reference computes but does not return). */
typedef struct bf_out_desc {
  bf_stream weights;    /* E = 1    */
  bf_stream means;      /* E = n    */
  bf_stream covs;       /* E = n*n  */
  bf_stream pred_means; /* E = n    */
  bf_stream pred_covs;  /* E = n*n  */
  bf_stream loglik;     /* E = 1    */
  /* COLLAPSED mode (bf_gsf_ekf_f32 only; sK unused): the moment-matched single Gaussian of the
   * filtered mixture at every step -- utils.collapse (utils.py:10-18) and the point estimate
   * sum_k w_k m_k of BOT_Experiment_script.py:101 -- formed inside the scan, so a K-component run
   * can return 4(n + n*n) bytes per step instead of the K-fold streams above. */
  bf_stream coll_mean;  /* E = n    */
  bf_stream coll_cov;   /* E = n*n  */
} bf_out_desc;

/* Scan carry (weights, pred_means, pred_covs) of inference.py:334,356: the state the filter
 * starts from and (optionally) the state it ends with, so that T can be processed in chunks
 * when the full posterior history exceeds HBM.  Contiguous [B][K], [B][K][n], [B][K][n][n].
 * *_out may alias *_in; NULL *_out = not written.  w_in == NULL means 1/K (inference.py:369). */
typedef struct bf_carry {
  const float* w_in;
  const float* m_in; /* required: initial (predicted) means, inference.py:367 */
  const float* P_in; /* required: initial (predicted) covariances, inference.py:368 */
  float* w_out;
  float* m_out;
  float* P_out;
} bf_carry;

/* Linear-Gaussian SSM   f(x,q,u) = A x + G q,  h(x,r,u) = H x + D r   (the "Kalman" model:
 * gaussian_sum_filter with num_components = 1 and linear f, h; e.g.
 * docs/experiments/adaptive_experiment.py:59-64, BOT_Experiment_script.py:31-41).
 * HOST pointers, row-major fp32.  G == NULL: identity (dq = n); D == NULL: identity (dr = m);
 * q0 / r0 == NULL: zeros.  Q_steps / R_steps: 1 = time-invariant [d,d]; T = one matrix per
 * step [T,d,d] (the `_get_params(x, 2, t)` rule of inference.py:21,337-340). */
typedef struct bf_lgssm {
  int32_t n, dq, m, dr;
  const float *A, *G, *H, *D;
  const float *q0, *r0;
  const float *Q, *R;
  int32_t Q_steps, R_steps;
} bf_lgssm;

int bf_version(void);
/* ABI guard.  A binding that mirrors the structs of this header by hand (ctypes, cgo, JNI ...) calls this once after
 * loading the library, with the BF_VERSION it was written against and ITS sizes of the structs it fills; a mismatch
 * (e.g. a bf_out_desc with six streams against the library's eight) returns BF_EINVAL with the offending struct in
 * bf_last_error() instead of an out-of-bounds read later.  A size of 0 means "this binding does not mirror that struct". */
int bf_abi_check(int32_t header_version, size_t sizeof_out_desc, size_t sizeof_lgssm, size_t sizeof_model,
                 size_t sizeof_bpf_model, size_t sizeof_bpf_out);
const char* bf_last_error(void);
/* Number of visible gfx950 devices (0 if none / HIP unavailable). */
int bf_device_count(void);

/* Tuning / test hooks.
 *   "kf_emit_mode": -1 = choose the store path from the layout (default), 0 = strided dword
 *                   stores, 2 = LDS time-transpose (contiguous reference layout only).
 *   "kf_lanes":     lanes that cooperate on one trajectory (0 = default for the dimensions;
 *                   otherwise one of the compiled powers of two, e.g. 1, 2 or 4 at n = 4).
 *   "kf_small_mode": 1 (default) = Kalman models with 9 <= n <= 32, m <= 32 run on the one-wave-per-trajectory matrix-core
 *                   kernel (single 32 x 32 tiles, bf16 three-term products); 0 = off (n >= 24 then rides padded in the
 *                   (64, 32) kernel, smaller n on the run-time-dimension kernel).  Models with 33 <= n <= 64, m <= 32 always
 *                   run on the (64, 32) matrix-core kernel (gain-free update P+ = P - W^T W + c c^T with W = L^-1 H P, the
 *                   same three-term bf16 products); it has no option.
 *   "force_generic": 1 = bf_kalman_filter_f32 / bf_gsf_ekf_f32 run the run-time-dimension kernel (any n, m, K; state in
 *                   LDS) even where a compile-time-dimension instance exists (test hook; default 0).  The smoothers
 *                   (bf_rts_smoother_f32, bf_eks_smoother_f32) honour it the same way, bf_eks_smoother_f32 / bf_effbs_sample_f32
 *                   also for dynamics given as source (the run-time-dimension kernel built around them).
 *   "agsf_force_generic": 1 = bf_agsf_ekf_f32 / bf_agsf_ukf_f32 run the run-time-dimension kernel (the node in turn in LDS, up
 *                   to 256 leaves per trajectory, registry functions) even where every dimension is <= 8 (default 0): the two
 *                   kernels on one model, or more than 64 leaves at 5 <= n <= 8.
 *   "rts_load_mode": the smoothers' data path: -1 = choose from the layout (default), 0 = strided per-lane loads and
 *                   stores, 2 = LDS-staged time chunks (contiguous reference layout, n <= 4 only); dynamics given as
 *                   source follow the same rule.
 *   "ffbs_spl":     samples per lane of the posterior samplers' register kernel (n <= 8): 0 = the smallest compiled count that holds all S
 *                   samples of a trajectory in one lane, 8 for S > 8 (default),
 *                   otherwise one of the compiled counts 1, 2, 4, 8 (the arithmetic of a sample does not depend on it);
 *                   the kernels built around dynamics given as source have the same four counts.
 *   "pkf_block":    block length L of bf_kalman_filter_pscan_f32: 0 (default) = from (B, T), otherwise 4 ... 4096 (the arithmetic of
 *                   a trajectory depends on T and L alone).
 *   "prs_block":    block length L of bf_rts_smoother_pscan_f32: 0 (default) = from (B, T) by the rule of "pkf_block", otherwise
 *                   4 ... 4096.
 *   "pfs_block":    block length L of bf_ffbs_sample_pscan_f32: 0 (default) = from (B, S, T), otherwise 4 ... 4096.
 *   "gsf_structured": 1 (default) lets bf_gsf_ekf_f32 use the structure-aware kernel instances
 *                   (banded Lorenz-96 Jacobian, selection emission) when the model qualifies;
 *                   0 forces the dense generic instances.
 *   "bpf_variant":  workgroup geometry of the 4096-particle instance: 0 (default) = 1024 threads x 4 particles, 1 = 512 x 8.
 *   "bpf_hbm_mode": particle counts beyond the in-register capacities: 0 (default) = choose by batch
 *                   size, 1 = one workgroup per trajectory, 2 = one workgroup per 1024-particle chunk
 *                   (six launches per step; same results bit for bit).
 *   "bpf_spec":     1 (default) = models whose structure has a compile-time instance (Lorenz-96 dynamics with identity noise
 *                   input, diagonal chol(Q), selection emission, diagonal chol(R)) run on it; 0 = the run-time instance
 *                   (same results bit for bit).
 *   "bpf_arith":    arithmetic of the particle filter's weight path (the normal draws' erf_inv, the exp of the weights): 0
 *                   (default) = the engine's DEFINED fp32 arithmetic (IEEE operations in a fixed order; resampling indices
 *                   reproducible bit for bit); 1 = the hardware's v_log_f32 / v_exp_f32 (1 ulp, not
 *                   reproducible across architectures; results agree with mode 0 to rounding until a uniform draw lands within
 *                   that rounding of a CDF step).  Mode 1 compiles the kernel at run time (needs hiprtc, like bf_user_model_create)
 *                   and serves particle counts up to 4 096 with registry functions.
 * bf_set_option changes the PROCESS-WIDE default.  A library or a thread that must not disturb -- or be disturbed by -- other
 * callers uses bf_set_call_option instead: it arms the same option on the CALLING THREAD for the NEXT filter entry point
 * called on that thread (bf_kalman_filter_f32, bf_kalman_filter_missing_f32, bf_kalman_filter_pscan_f32, bf_kalman_filter_pscan_missing_f32, bf_gsf_ekf_f32, bf_ugsf_ukf_f32, bf_gsf_ekf_missing_f32, bf_ugsf_ukf_missing_f32, bf_agsf_*, bf_bpf_f32, bf_bpf_missing_f32, bf_sample_ssm_f32,
 * bf_resample_f32, bf_optimal_resample_f32, bf_collapse_f32, bf_rts_smoother_f32, bf_rts_smoother_pscan_f32, bf_eks_smoother_f32,
 * bf_ffbs_sample_f32, bf_ffbs_sample_pscan_f32, bf_effbs_sample_f32, bf_uks_smoother_f32, bf_gs_smoother_f32, bf_gs_sample_f32, bf_uffbs_sample_f32, bf_pf_backward_sample_f32, bf_pf_trace_sample_f32) and for that call only; every armed override is dropped when
 * that call returns, whatever its status. */
int bf_set_option(const char* name, int value);
int bf_set_call_option(const char* name, int value);

/* Batched Kalman filter: B independent trajectories, one component each (K = 1), T steps.
 * Replaces the lax.scan of gaussian_sum_filter (inference.py:333-371) with
 * _condition_on (:72-105) and _predict (:51-70) specialised to linear f, h.
 * y: observations, element (b, t, e) at y->ptr[b*sB + t*sT + e*sE], E = m. */
int bf_kalman_filter_f32(const bf_lgssm* model, const bf_cstream* y, int64_t B, int64_t T,
                         const bf_carry* carry, const bf_out_desc* out, void* stream);

/* bf_kalman_filter_f32 for series with gaps: the same arguments and streams, and a NaN entry of y means "component a of
 * trajectory b was not observed at step t" (the convention of statsmodels / pykalman; no second input stream).  With o the
 * components of a step that are not NaN, the update is _condition_on on the sub-model of those rows -- H[o,:], (D r0)[o],
 * (D R D^T)[o,o], the reference's 1e-6 on every entry of the reduced S_oo in the gain solve -- and the step's log-likelihood
 * is log N(v_o; 0, S_oo) with |o| in the log 2 pi term.  o empty: m+ = m-, P+ = P- exactly, log-likelihood 0, weight
 * reweight(0, w); the predict step runs as always, so trailing unobserved steps are a forecast.  +-Inf is NOT missing: a
 * non-finite innovation of an observed component poisons the trajectory as in bf_kalman_filter_f32 (which keeps treating NaN
 * that way: this entry point is opt-in).  The step is the reduced model's arithmetic embedded in the m x m system (missing
 * rows and columns of S replaced by those of the identity, exact zeros elsewhere), so lanes with different patterns stay
 * convergent and a trajectory's bits do not depend on its neighbours' gaps.  The smoothers and samplers read no observations:
 * they run on these streams as they are.
 * Register kernels only, each (n, m) pair at its default lanes per trajectory; honours "kf_emit_mode" ("force_generic" and
 * "kf_small_mode" do not apply: there is no other kernel to fall back to).
 * BF_EUNSUPPORTED: n > 8 or m > 4 (the message names the limit), m > n, a "kf_lanes" other than 0 or the pair's default,
 * collapsed streams.  BF_EINVAL: NULL arguments, B or T <= 0, what bf_kalman_filter_f32 refuses of the model and the carry.
 * Every check precedes the first HIP call.  With this one, this header declares 46 entry points. */
int bf_kalman_filter_missing_f32(const bf_lgssm* model, const bf_cstream* y, int64_t B, int64_t T,
                                 const bf_carry* carry, const bf_out_desc* out, void* stream);

/* Parallel-in-time Kalman filter for few long trajectories: the model, streams, carry and log-likelihood of
 * bf_kalman_filter_f32, with time cut into blocks of L steps that run on separate lanes (the associative filtering elements
 * of Sarkka & Garcia-Fernandez 2021; the scheme is stated at the head of csrc/kf_pscan.hpp).  Three launches on `stream`,
 * no waiting between workgroups: fold (one lane per (trajectory, block) builds the block's aggregate), scan (one workgroup per
 * trajectory turns the aggregates into every block's start state), emit (one lane per (trajectory, block) runs the ordinary
 * update -> predict step of bf_kalman_filter_f32 from its block's start state and stores the streams, any strides).
 * Inside a block the outputs are the ordinary filter's from that block's start state; the start states come from a jitter-free
 * recursion, so the result agrees with bf_kalman_filter_f32 to fp32 tolerance (1e-5 relative), not bit for bit.  A trajectory's
 * bits depend on (T, L) alone.  A NaN / Inf observation at step t gives NaN in every stream and in the carry from t on, in that
 * trajectory only -- the covariances included, which bf_kalman_filter_f32 leaves finite: a step whose innovation is not finite has no posterior.
 * L: option "pkf_block" (4..4096; 0 = default: the largest of ceil(B T / 65 536) -- one (trajectory, block) lane per lane of the
 * device --, the smallest s with 50 s^2 >= T -- the balance between the per-trajectory scan and the per-lane work -- and 16,
 * at most 4096).
 * workspace: a caller-owned DEVICE buffer of at least bf_kalman_pscan_workspace_bytes(n, m, B, T, L) =
 *   4 B ceil(T / L) (4 n^2 + 3 n) bytes, 4-byte aligned; its contents before and after the call mean nothing.
 * bf_kalman_pscan_workspace_bytes: `block` = 0 reads "pkf_block" as the filter call would and else uses the default; a negative
 * result is a BF_E* code (B or T <= 0, a block length outside 4..4096, dimensions that are not built, B ceil(T / L) >= 2^31).
 * BF_EUNSUPPORTED: n > 6 or m > 4 (register kernels: the scan needs scratch from n = 7; the message names the limit), per-step covariances (Q_steps or
 * R_steps > 1: "constant Q and R"), collapsed streams, a singular S = H G Q G^T H^T + D R D^T.  BF_EINVAL: NULL arguments,
 * B or T <= 0, a workspace that is too small (the message names the bytes needed).  Every check precedes the first HIP call.
 * With these two, this header declares 41 entry points (43 with the two of the parallel-in-time smoother below). */
int64_t bf_kalman_pscan_workspace_bytes(int32_t n, int32_t m, int64_t B, int64_t T, int32_t block); /* < 0: BF_E* */
int bf_kalman_filter_pscan_f32(const bf_lgssm* model, const bf_cstream* y, int64_t B, int64_t T,
                               const bf_carry* carry, const bf_out_desc* out,
                               void* workspace, int64_t workspace_bytes, void* stream);

/* bf_kalman_filter_pscan_f32 for series with gaps: the same arguments, workspace (bf_kalman_pscan_workspace_bytes) and three
 * launches, with the contract of bf_kalman_filter_missing_f32 -- a NaN entry of y is a component that was not observed at
 * that step; the update conditions on the observed rows only; a step with none leaves mean and covariance as they are and has
 * log-likelihood 0 (on an already poisoned trajectory too: its weight stays NaN); the predict step always runs, so trailing
 * gaps are a forecast; +-Inf in an observed entry still poisons from that step on.  Opt-in: bf_kalman_filter_pscan_f32 keeps
 * treating NaN as poison.
 * A step's filtering element depends on its observation pattern, so the host forms the constant parts (A_e, C_e, J_e and the
 * maps K, W; float64, as for the complete step) once per call for each of the 2^m patterns -- 3 n^2 + 2 n m floats each, at
 * most 9 984 bytes at (6, 4) --, keeps the table as a cached device constant block and the fold stages it into LDS; a lane
 * selects its step's entry by the pattern's bit mask.  The entry of the complete pattern equals the constants of
 * bf_kalman_filter_pscan_f32 bit for bit, and block 0 and the emit launch run the masked step of
 * bf_kalman_filter_missing_f32; inside a block the outputs are that filter's from the block's start state, the start states
 * are jitter-free, and the whole agrees with it to fp32 tolerance.  Scan, workspace layout and "pkf_block" are unchanged.
 * Refusals: those of bf_kalman_filter_pscan_f32, in the same order and words, before the first HIP call; every S_o is a
 * principal submatrix of S and is checked like S.  With this one, this header declares 50 entry points. */
int bf_kalman_filter_pscan_missing_f32(const bf_lgssm* model, const bf_cstream* y, int64_t B, int64_t T,
                                       const bf_carry* carry, const bf_out_desc* out,
                                       void* workspace, int64_t workspace_bytes, void* stream);

/* A state-space model built from the function registry (the device-side replacement of the
 * Python callables f(x,q,u), h(x,r,u) of gaussfiltax/models.py:46-49; ids and theta layouts:
 * bayesianfiltering_amd/nonlinearities.py, formulas: csrc/models.hpp).  HOST pointers. */
typedef struct bf_model {
  int32_t dyn_id, emi_id;
  int32_t n, dq, m, dr;
  const float* dyn_theta;
  int32_t n_dyn_theta;
  const float* emi_theta;
  int32_t n_emi_theta;
  const float *q0, *r0; /* noise biases, NULL = zeros                */
  const float *Q, *R;   /* noise covariances [dq,dq], [dr,dr]; [steps,d,d] when Q_steps / R_steps > 1 */
  int32_t flags;        /* 0 = the JAX path's semantics; BF_MODEL_* bits for the legacy NumPy classes */
  int32_t Q_steps, R_steps; /* 0 or 1 = constant; T = one covariance per step, the (T,d,d) arrays that
                               _get_params(..., 2, t) selects from (inference.py:21, :337-340).  Honoured by
                               bf_gsf_ekf_f32 (emissions with a constant H_r); the sampling kernels need 0 / 1. */
  const struct bf_user_model* user; /* functions compiled from source (dyn_id / emi_id = BF_FN_USER), else NULL */
} bf_model;

/* ---- user-defined f / h ------------------------------------------------------------------------
 * The reference accepts arbitrary Python callables f(x, q, u), h(x, r, u) (gaussfiltax/models.py:46-49) and takes their
 * Jacobians with jacfwd (gaussfiltax/inference.py:328-329).  Here a function outside the registry is given as HIP C++
 * SOURCE TEXT, written once for any scalar type:
 *
 *     template <class T> __device__ void dynamics(const T* x, const T* q, T u, const float* theta, T* out);   // out[BF_N]
 *     template <class T> __device__ void emission(const T* x, const T* r, T u, const float* theta, T* out);   // out[BF_M]
 *
 * (BF_N, BF_DQ, BF_M, BF_DR are compile-time constants; sin cos tan exp log sqrt tanh atan atan2 pow abs are available
 * for T; theta = bf_model.dyn_theta / emi_theta).  bf_user_model_create compiles it with hiprtc into the
 * run-time-dimension scan kernel; values come from T = float, Jacobians w.r.t. state AND noise from forward-mode dual
 * numbers (what jacfwd computes), F_q Q F_q^T / H_r R H_r^T are formed on the device every step.  Either source may be
 * NULL (that side stays a registry function).  Compiled models are cached by source (memory + $BAYESFILT_CACHE_DIR,
 * default .jit_cache next to the library); a source that does not compile returns BF_EINVAL with the compiler's first error in
 * bf_last_error().  Use: set bf_model.user and dyn_id / emi_id = BF_FN_USER, then call bf_gsf_ekf_f32.  For n, dq, m, dr <= 8 (both
 * functions from source, or the other one the registry's linear function; no legacy flags, no collapsed streams) the handle also
 * builds, on first use, the Gaussian-sum scan with the state in REGISTERS (one lane per (trajectory, component), the same dual-number
 * Jacobians): two orders of magnitude faster than the run-time-dimension kernel and the default there ("force_generic" = 1 keeps
 * the LDS kernel). */
#define BF_FN_USER 100
typedef struct bf_user_model bf_user_model;
int bf_user_model_create(const char* dynamics_src, const char* emission_src, int32_t n, int32_t dq, int32_t m, int32_t dr,
                         bf_user_model** model);
/* ... and for the bootstrap particle filter (bf_bpf_f32), whose model is f, the emission log-density and nothing else
 * (gaussfiltax/inference.py:1344-1349: x' = f(x, q, u), lls = emission_distribution_log_prob(x', y, u), any callables):
 * the same handle also compiles the particle-filter kernel with the caller's functions, on first use and per particle
 * capacity (particles in registers up to 4096 for state_dim <= 16 / 1024 beyond; above that the particles-in-HBM kernel, up to
 * 2^20 per trajectory) -- and, likewise on first use, the unscented (bf_ugsf_ukf_f32) and augmented (bf_agsf_ekf_f32 /
 * bf_agsf_ukf_f32) scans and the data generator (bf_sample_ssm_f32) around the same functions (augmented scans around functions from source: dimensions up to 8 -- registry functions run at any dimension, see bf_agsf_ekf_f32; sampler 32).  The density is either Gaussian around the (registry or
 * source) emission function, MVN(h(x, r_eval, u), lp_cov) as for registry models, or -- log_prob_src -- the caller's own
 *
 *     template <class T> __device__ T log_prob(const T* x, const float* y, T u, const float* theta);   // theta = bf_bpf_model.lp_theta
 *
 * In these kernels sin cos sincos atan atan2 exp log sqrt abs fma are the CANONICAL fp32 arithmetic of the weight path
 * (bf_canon_eval_f32), so a function written like a registry function gives that function's bits.  Any of the three
 * sources may be NULL (at least one is given). */
int bf_user_model_create_lp(const char* dynamics_src, const char* emission_src, const char* log_prob_src, int32_t n, int32_t dq,
                            int32_t m, int32_t dr, bf_user_model** model);
void bf_user_model_destroy(bf_user_model* model);

/* Hyper-parameters of the unscented transform -- ParamsUKF (inference.py:41-49): lambda =
 * alpha^2 (L + kappa) - L with L = state_dim + noise_dim of the augmented state. */
typedef struct bf_ukf_params {
  float alpha, beta, kappa;
} bf_ukf_params;

/* Legacy-class semantics (gaussfiltax/gaussfilt.py, gausssumfilt.py), honoured by bf_gsf_ekf_f32: */
#define BF_MODEL_PREDICT_FIRST 1  /* step order predict -> update (gaussfilt.py:113-121); carry = filtered state   */
#define BF_MODEL_NO_JITTER 2      /* gain from S itself, no 1e-6 (gaussfilt.py:118 `Cxy @ inv(Sy)`)                 */
#define BF_MODEL_LEGACY_GSF_COV 4 /* predicted covariance P + J P J^T, Q never added (gausssumfilt.py:59)           */

/* Batched Gaussian-sum filter (bank of K extended Kalman filters + weight update): replaces the
 * lax.scan of gaussian_sum_filter (inference.py:333-371) for K >= 1 and nonlinear f, h.
 * u: optional inputs, element (b, t) at u->ptr[b*sB + t*sT] (only u[0] is used by the registry
 * functions); NULL or u->ptr == NULL means zeros((T,1)) (inference.py:23).  The carry holds
 * the K initial component means / covariances per trajectory ([B][K][n], [B][K][n][n]) and,
 * optionally, weights [B][K] (NULL = 1/K, inference.py:369).  K rounded up to a power of two
 * times the lanes per chain must not exceed 256. */
int bf_gsf_ekf_f32(const bf_model* model, const bf_cstream* y, const bf_cstream* u, int64_t B, int64_t T, int32_t K,
                   const bf_carry* carry, const bf_out_desc* out, void* stream);

/* Batched unscented Gaussian-sum filter: K unscented Kalman filters with non-additive noise
 * (augmented sigma points) per trajectory plus the weight update.  Replaces the lax.scan of
 * unscented_gaussian_sum_filter (inference.py:379-456) with _ukf_condition_on_nonadditive
 * (:198-224), the reweight (:424-427) and _ukf_predict_nonadditive (:146-174); sigma points as
 * utils._get_sigma_points (utils.py:247-254) with the symmetric matrix square root computed on the
 * device.  Arguments as bf_gsf_ekf_f32; constant or per-step (T, d, d) covariances; out->coll_* unsupported.  Every dimension
 * <= 8: state in registers, K <= 256.  Any of n, dq, m, dr above 8 (or option "ugsf_force_generic" = 1): state in LDS, any K,
 * registry functions linear / Lorenz-96 / sine and linear / quadratic / stochastic volatility or functions from source;
 * BF_EUNSUPPORTED with the byte count when a workgroup's 160 KiB of LDS do not hold the model (n = 68 with n / 2 observations fits). */
int bf_ugsf_ukf_f32(const bf_model* model, const bf_ukf_params* uparams, const bf_cstream* y, const bf_cstream* u,
                    int64_t B, int64_t T, int32_t K, const bf_carry* carry, const bf_out_desc* out, void* stream);

/* The two Gaussian-sum filters on series with gaps: a NaN y(b, t, a) means "component a was not observed at step t" (the
 * convention of bf_kalman_filter_missing_f32, per component of the bank).  Arguments of their plain twins.  With o the
 * components of the step that are not NaN, every component k conditions on the rows o only -- extended nodes: H_x[o, :],
 * h(x)[o], (H_r R H_r^T)[o, o], state-dependent H_r included, the jitter on every entry of the reduced S_oo; unscented nodes:
 * the sigma points of the full augmented state with mu, S and C restricted to the rows o -- and ll_k = log N(v_o; 0, S_oo)
 * with |o| in the log 2 pi term.  The weights go through the unchanged reweight with those ll_k.  o empty: every ll_k is 0,
 * means and covariances are untouched exactly, the weights are renormalised only (K = 1: exactly 1); the predict always runs,
 * so trailing unobserved steps are a forecast.  Only a NaN in y means missing: what the model computes for a missing row is
 * discarded by selects, so a NaN or Inf produced there does not leak; +-Inf in y, or a non-finite innovation of an observed
 * component, poisons as in the plain entry points (which keep reading a NaN as poison: these two are opt-in).  Collapsed
 * streams and per-step Q / R tables work as on the plain route where its register kernels produce them.
 * Register kernels only, and no fallback.  BF_EUNSUPPORTED, with a message that names the limit: flags != 0 (legacy classes);
 * registry models with n > 8 or m > 4 (bf_gsf_ekf_missing_f32: the matrix-core and run-time-dimension kernels take no gaps) or
 * m > n; models from source that the register kernel does not take (a log-density, a dimension above 8, K > 256, collapsed
 * streams); unscented models with a dimension above 8 or K > 256; "force_generic" / "ugsf_force_generic" set; a "kf_lanes"
 * other than 0 or the compiled default for n.  BF_EINVAL: NULL arguments, non-positive sizes, what the plain twins refuse of
 * the model and the carry.  "kf_emit_mode" and "gsf_structured" are honoured.  Every check precedes the first HIP call.
 * With these two, this header declares 48 entry points. */
int bf_gsf_ekf_missing_f32(const bf_model* model, const bf_cstream* y, const bf_cstream* u, int64_t B, int64_t T, int32_t K,
                           const bf_carry* carry, const bf_out_desc* out, void* stream);
int bf_ugsf_ukf_missing_f32(const bf_model* model, const bf_ukf_params* uparams, const bf_cstream* y, const bf_cstream* u,
                            int64_t B, int64_t T, int32_t K, const bf_carry* carry, const bf_out_desc* out, void* stream);

/* Batched "speedy" augmented Gaussian-sum filter: replaces the lax.scan of
 * speedy_augmented_gaussian_sum_filter (inference.py:621-812).  num_components = (N0, N1, N2): every
 * step branches the N0 carried components into N1 z-samples each (predicted with covariance
 * opt_args[0] * P), every prediction into N2 s-samples (updated with covariance opt_args[1] * P-), and
 * draws N0 of the N0*N1*N2 leaves with jr.choice under PRNGKey(0).  key: the reference's rng_key (it is
 * never advanced: the same normals at every step).  The carry holds N0 components per trajectory;
 * out: weights / means / covs with K = N0 (the other streams must be unset).  leaf_idx: optional
 * DEVICE int32 [B][T][N0], the leaf each carried component was drawn from.  N0*N1*N2 <= 64 in general,
 * <= 1024 for state_dim <= 4 (one workgroup per trajectory; every variant) while every dimension is <= 8: a leaf per lane,
 * in registers.  Any of n, dq, m, dr above 8 (or option "agsf_force_generic" = 1): the node in turn in LDS, N0*N1*N2 <= 256,
 * registry functions, bounded by the 160 KiB of LDS of a workgroup (BF_EUNSUPPORTED names the bytes needed).
 * variant: 0 = the speedy filter's two shared normal arrays (:672-688, :716-726); 1 = the branches of
 * augmented_gaussian_sum_filter (inference.py:458-620) through containers._branches_from_tree1/2
 * (containers.py:63-140): one key per node, jr.multivariate_normal per node, NaN samples replaced by the mean;
 * 2 = augmented_gaussian_sum_filter_optimal (:1157-1300): the branches of 1 and utils.optimal_resampling
 * (utils.py:216-244) instead of jr.choice, so the carried components keep unequal weights. */
int bf_agsf_ekf_f32(const bf_model* model, const bf_cstream* y, const bf_cstream* u, int64_t B, int64_t T,
                    const int32_t num_components[3], const uint32_t key[2], const float opt_args[2], const bf_carry* carry,
                    const bf_out_desc* out, int32_t* leaf_idx, int32_t variant, void* stream);

/* The augmented filter with unscented nodes: replaces the lax.scan of speedy_unscented_agsf
 * (inference.py:966-1156; variant 0) and unscented_agsf (:813-965; variant 1) -- the tree, sampling and
 * resampling of bf_agsf_ekf_f32 with _ukf_predict_nonadditive / _ukf_condition_on_nonadditive at the nodes. */
int bf_agsf_ukf_f32(const bf_model* model, const bf_ukf_params* uparams, const bf_cstream* y, const bf_cstream* u, int64_t B,
                    int64_t T, const int32_t num_components[3], const uint32_t key[2], const float opt_args[2],
                    const bf_carry* carry, const bf_out_desc* out, int32_t* leaf_idx, int32_t variant, void* stream);

/* utils.optimal_resampling(weights, N, key) (utils.py:216-244, Fearnhead & Clifford) for B weight vectors of
 * length M <= 1024 (one wave segment per vector up to 64, one workgroup beyond): d_weights [B][M] -> d_idx [B][N] (indices into the M particles), d_weights_out [B][N]. */
int bf_optimal_resample_f32(const float* d_weights, const uint32_t key[2], int64_t B, int32_t M, int32_t N, int32_t* d_idx,
                            float* d_weights_out, void* stream);

/* Moment-matching collapse of the mixture posterior per (trajectory, step): gaussfiltax/utils.py:10-18
 * and the point estimate sum_k w_k m_k (docs/experiments/BOT_Experiment_script.py:101).  weights /
 * means / covs are the strided streams a filter emitted (covs may be NULL when cov_out is NULL);
 * mean_out [B][T][n], cov_out [B][T][n][n] contiguous DEVICE buffers (either may be NULL). */
int bf_collapse_f32(const bf_stream* weights, const bf_stream* means, const bf_stream* covs, int64_t B, int64_t T,
                    int32_t K, int32_t n, float* mean_out, float* cov_out, void* stream);

/* ---- bootstrap particle filter ------------------------------------------------------- */
/* ParamsBPF (gaussfiltax/models.py:55-84): the state-space model plus the Gaussian emission
 * log-density  MVN(h(x, r_eval, u), lp_cov).log_prob(y)  (the form of every `*lp` function of the
 * reference's scripts, e.g. gaussfiltax/nonlinearities.py:51-52) and the initial law N(m0, P0).
 * HOST pointers. */
typedef struct bf_bpf_model {
  bf_model ssm;
  const float* m0;     /* [n]      */
  const float* P0;     /* [n,n]    */
  const float* lp_cov; /* [m,m] covariance R of the emission log-density (the stochastic-volatility
                        * emission uses M(x,u) R M(x,u)^T, adaptive_experiment.py:55-57)          */
  const float* r_eval; /* [dr] noise value h is evaluated at (NULL = zeros)     */
  const float* lp_theta; /* parameters of a log-density given as source (bf_user_model_create_lp), else NULL */
  int32_t n_lp_theta;
} bf_bpf_model;

/* Scan carry (weights, particles, key) of inference.py:1364 for chunked runs; DEVICE pointers,
 * contiguous [B][N][n], [B][N], [B][2].  x_in == NULL: draw the initial particles (:1369-1373). */
typedef struct bf_bpf_carry {
  const float* x_in;
  const float* w_in;
  const uint32_t* key_in;
  float* x_out;
  float* w_out;
  uint32_t* key_out;
} bf_bpf_carry;

/* Outputs (DEVICE pointers, NULL = not emitted).  weights / particles are what the reference
 * returns (inference.py:1359-1362): element (b,i,t) at weights[b*w_sB + i*w_sN + t*w_sT],
 * (b,i,t,d) at particles[b*x_sB + i*x_sN + t*x_sT + d]; ancestors share the weights' strides.
 * The per-step summaries are contiguous [B][T][n] / [B][T]. */
typedef struct bf_bpf_out {
  float* weights;
  int64_t w_sB, w_sN, w_sT;
  float* particles;
  int64_t x_sB, x_sN, x_sT;
  int32_t* ancestors;
  float* mean;      /* sum_i w_i x_i of the emitted weights / particles */
  float* ess;       /* 1 / sum w^2 before the resampling decision       */
  float* logz;      /* log sum_i w_{t-1,i} p(y_t | x_i)                 */
  float* resampled; /* 1.0 where the step resampled                     */
} bf_bpf_out;

/* Batched bootstrap particle filter: replaces the lax.scan of bootstrap_particle_filter
 * (inference.py:1330-1377) with _resample (utils.py:207-214).  One workgroup per
 * trajectory: N <= 4096 particles (16 384 for state / noise dimensions <= 4) stay in the workgroup's
 * registers; larger N up to 2^20 keep the particles in HBM scratch (stream-ordered allocation) and run
 * the same tree orders chunk by chunk (a workgroup per trajectory, or per chunk when B < 128).  key = {hi, lo} of jr.PRNGKey (used for every
 * trajectory unless carry->key_in is given).  resampler: 0 = multinomial inverse-CDF (the
 * reference's jr.choice), 1 = systematic. */
int bf_bpf_f32(const bf_bpf_model* model, const bf_cstream* y, const bf_cstream* u, int64_t B, int64_t T, int32_t N,
               const uint32_t key[2], float ess_threshold, int32_t resampler, const bf_bpf_carry* carry,
               const bf_bpf_out* out, void* stream);

/* The bootstrap particle filter on observations with GAPS: bf_bpf_f32's arguments, dispatch (compiled instances, particles in
 * HBM per trajectory or per chunk, kernels built at run time) and pre-launch refusals, on the MISSING = true kernels.  A NaN entry
 * y[b, t, a] means "component a was not observed at step t"; o = the components of the step that are not NaN.
 *   - Propagation never changes: every step consumes the keys it consumes in bf_bpf_f32.  With nothing missing the weights,
 *     particles, ancestors, ESS, logz and carry are bf_bpf_f32's bit for bit.
 *   - Gaussian densities (registry, source or recorded emission function), |o| > 0: the log-weight is
 *     log N(y_o; h(x, r_eval, u)_o, (R_lp)_oo), factored per step; the stochastic-volatility scale enters for observed rows only.
 *     What the model computes for a missing row is discarded.
 *   - Nothing observed: every log-weight is 0 and the step runs the unchanged reweight -- the weights are the previous ones
 *     renormalised, logz is log(sum w), within an ulp of 0 and not exactly 0; trailing gaps are a forecast, and sum_t logz is the
 *     log-evidence of the observed entries.
 *   - A density from the caller's source (bf_user_model_create_lp): a wholly missing step as above, the function is not called;
 *     a PARTLY observed y is handed to it as it is, NaN entries included -- the library cannot marginalise a density it does not
 *     know.  A function that treats NaN itself (per component `y[a] != y[a] ? 0 : ...`) takes gapped series, another one is
 *     poisoned as under bf_bpf_f32.
 *   - +-Inf is never "missing": a non-finite innovation of an observed component poisons that trajectory, and only it.
 *   - Chunks through bf_bpf_carry cut anywhere, inside a gap included, equal the single call bit for bit.
 * With this one, this header declares 49 entry points. */
int bf_bpf_missing_f32(const bf_bpf_model* model, const bf_cstream* y, const bf_cstream* u, int64_t B, int64_t T, int32_t N,
                       const uint32_t key[2], float ess_threshold, int32_t resampler, const bf_bpf_carry* carry,
                       const bf_bpf_out* out, void* stream);

/* Synthetic data: NonlinearSSM.sample (gaussfiltax/models.py:240-289) for B trajectories, one key
 * per trajectory (d_keys [B][2], DEVICE).  model->ssm carries f, h, q0, Q, r0, R; model->m0 / P0 the
 * initial law (lp_cov / r_eval unused).  d_states [B][T][n], d_emissions [B][T][m] contiguous
 * DEVICE buffers (either may be NULL). */
int bf_sample_ssm_f32(const bf_bpf_model* model, const uint32_t* d_keys, const bf_cstream* u, int64_t B, int64_t T,
                      float* d_states, float* d_emissions, void* stream);

/* Index draw of utils.py:210 alone: d_idx[b][i] = choice(d_keys[b], N, (N,), p = d_w[b]). */
int bf_resample_f32(const float* d_w, const uint32_t* d_keys, int64_t B, int32_t N, int32_t resampler,
                    int32_t* d_idx, void* stream);

/* The canonical fp32 arithmetic of the particle filter's weight path (csrc/bf_canon_math.hpp: IEEE add / mul / div /
 * sqrt / fma and integer operations in a fixed order, identical on host and device, restated by the oracle so that
 * in-filter resampling indices are bit-exact), evaluated elementwise: op 0 = log, 1 = exp, 2 = jax.random.normal's
 * bits -> N(0,1) map (the input words are the raw uint32 bits), 3 = sin, 4 = cos, 5 = atan2(in[i], in[n + i]) (the input
 * holds 2 n values).  on_device = 0: HOST buffers, evaluated by the host
 * build of the same functions; 1: DEVICE buffers, one lane per element.  A test / audit hook. */
int bf_canon_eval_f32(int32_t op, const float* in, int64_t n, float* out, int32_t on_device, void* stream);

/* jax.random.normal(key, (count,)) for the default threefry PRNG, written to a HOST buffer
 * (used for the reference's fixed `MVN(m0, P0).sample(K, PRNGKey(0))` draw of the initial
 * component means, inference.py:367: m0 + chol(P0) z).  key = {hi, lo} as jr.PRNGKey. */
int bf_random_normal_f32(const uint32_t key[2], int64_t count, float* host_out);
/* jax.random.split(key, num) -> num keys (2 words each) in a HOST buffer. */
int bf_random_split(const uint32_t key[2], int64_t num, uint32_t* host_out);

/* ---- multi-GPU: the path's one exchange step --------------------------------
 * Trajectories are independent: the batch axis is sharded contiguously over the ranks (one process per GPU), every
 * rank calls the bf_* entry points above on its own shard with no traffic during the scan, and the per-trajectory
 * posterior summaries are exchanged once: d_send (this rank's `bytes` bytes, DEVICE) -> d_recv (world_size * bytes,
 * rank-major, DEVICE) with one ncclAllGather on `stream` over the caller's communicator (`nccl_comm` = ncclComm_t as
 * void*; RCCL over xGMI).  RCCL is loaded on first use.  The Python layer does the same through torch.distributed
 * (bayesianfiltering_amd/distributed.py: backend "nccl" is RCCL). */
int bf_allgather_summaries(const void* d_send, void* d_recv, size_t bytes, void* nccl_comm, void* stream);

/* ---- Rauch-Tung-Striebel smoothing (the reference's SSM.smoother, gaussfiltax/ssm.py:55-61, 282-300) --------------
 * Input: the streams a filter above emitted (update -> predict order): filtered m_t, P_t (out->means / covs) and the
 * one-step predictions m-_{t+1}, P-_{t+1} (out->pred_means / pred_covs at index t).  With F_t the dynamics Jacobian the
 * filter's predict used at step t (A for bf_lgssm; the registry Jacobian at (m_t, q0, u_t) for bf_model):
 *   t = T-1:            m^s = m, P^s = P (copied bit for bit; unless carry->m_in gives the smoothed state at T)
 *   t = T-2 ... 0:      X_t = (P-_{t+1})^-1 (F_t P_t) by Cholesky of P-_{t+1} (lower triangle read, no jitter), G_t = X_t^T
 *                       m^s_t = m_t + G_t (m^s_{t+1} - m-_{t+1})
 *                       P^s_t = P_t + G_t (P^s_{t+1} - P-_{t+1}) G_t^T
 *                       C_t  = Cov(x_t, x_{t+1} | y_{1:T}) = G_t P^s_{t+1}   (optional: what EM's E-step needs)
 * A P- that is not positive definite gives NaN for that trajectory from that step backwards (as a non-PD S does in the
 * filters).  Element (b, t, e) of every stream at ptr[b*sB + t*sT + e*sE] (sK unused: one component). */
typedef struct bf_smooth_desc {
  bf_stream means;      /* E = n,   required */
  bf_stream covs;       /* E = n*n, required */
  bf_stream cross_covs; /* E = n*n, optional: entry t for t < T-1 (entry T-1 too when carry->m_in is given) */
} bf_smooth_desc;

/* Backward chunking when the history does not fit in HBM: process the LAST chunk of steps first, then feed its m_out /
 * P_out as the next (earlier) chunk's m_in / P_in.  DEVICE pointers, contiguous [B][n] and [B][n][n].
 * m_in / P_in: the smoothed state at the first step AFTER this chunk (both NULL: the chunk ends at T-1).
 * m_out / P_out: receive the smoothed state at the chunk's first step (NULL = not written). */
typedef struct bf_smooth_carry {
  const float* m_in;
  const float* P_in;
  float* m_out;
  float* P_out;
} bf_smooth_carry;

/* ABI guard of the two smoother structs (bf_abi_check covers the rest); a size of 0 = not mirrored. */
int bf_smoother_abi_check(size_t sizeof_smooth_desc, size_t sizeof_smooth_carry);

/* RTS smoother of the linear model (bf_kalman_filter_f32's).  filtered->means / covs are required, the other fields
 * other than pred_means / pred_covs are ignored.  pred_means / pred_covs both NULL: they are RECOMPUTED from the filtered
 * streams, m- = A m + G q0 and P- = A P A^T + G Q_t G^T (Q_steps honoured; Q_steps = T of THIS call), so that the filter
 * may emit the filtered fields only.  carry may be NULL.  Asynchronous on `stream`, no allocation.  n <= 8: registers,
 * one lane per trajectory; larger n: the run-time-dimension kernel (one workgroup per trajectory, state in LDS). */
int bf_rts_smoother_f32(const bf_lgssm* model, const bf_out_desc* filtered, int64_t B, int64_t T,
                        const bf_smooth_carry* carry, const bf_smooth_desc* out, void* stream);

/* Parallel-in-time RTS smoother for few long trajectories: the model, streams, carry and outputs of bf_rts_smoother_f32 (both
 * of its routes: predictions given, or both NULL and recomputed), with time cut into blocks of L steps that run on separate
 * lanes (the associative smoothing elements of Sarkka & Garcia-Fernandez 2021; the scheme is stated at the head of
 * csrc/rts_pscan.hpp).  Three launches on `stream`, no waiting between workgroups: fold (one lane per (trajectory, block) builds
 * the block's aggregate; the last block's is its smoothed first-step state), scan (one workgroup per trajectory turns the
 * aggregates into the smoothed state at every block's first step), emit (one lane per (trajectory, block) runs the ordinary
 * backward step of bf_rts_smoother_f32 from the state after its block and stores the streams, any strides).
 * Inside a block the outputs are the ordinary smoother's from that block's carry: the last block, and with T <= L the whole
 * call, equals bf_rts_smoother_f32 bit for bit; elsewhere the two agree to fp32 tolerance (1e-5 relative).  A trajectory's bits
 * depend on (T, L) and the route alone.  NaN handling is bf_rts_smoother_f32's (from a step backwards, in that trajectory only).
 * L: option "prs_block" (4..4096; 0 = default: the rule of "pkf_block").
 * workspace: a caller-owned DEVICE buffer of at least bf_rts_pscan_workspace_bytes(n, B, T, L) =
 *   4 B ceil(T / L) (3 n^2 + 2 n) bytes, 4-byte aligned; its contents before and after the call mean nothing.
 * bf_rts_pscan_workspace_bytes: `block` = 0 reads "prs_block" as the call would and else uses the default; a negative result is
 * a BF_E* code (B or T <= 0, a block length outside 4..4096, n that is not built, B ceil(T / L) >= 2^31).
 * BF_EUNSUPPORTED: n > 6 (the parallel filter's limit; the message names it), a per-step Q (Q_steps > 1: "constant Q").
 * BF_EINVAL: NULL arguments (carry may be NULL), missing streams or outputs, one predicted stream without the other, B or
 * T <= 0, a workspace that is too small (the message names the bytes needed) or misaligned.  Every check precedes the first HIP
 * call.  With these two, this header declares 43 entry points (45 with the two of the parallel-in-time sampler below). */
int64_t bf_rts_pscan_workspace_bytes(int32_t n, int64_t B, int64_t T, int32_t block); /* < 0: BF_E* */
int bf_rts_smoother_pscan_f32(const bf_lgssm* model, const bf_out_desc* filtered, int64_t B, int64_t T,
                              const bf_smooth_carry* carry, const bf_smooth_desc* out,
                              void* workspace, int64_t workspace_bytes, void* stream);

/* Extended RTS smoother (K = 1; the streams of bf_gsf_ekf_f32 with one component) for registry dynamics and for dynamics
 * given as source.  pred_means / pred_covs are required.  u: the filter's inputs (NULL or u->ptr == NULL = zeros).
 * Dynamics from source (model->user with dyn_id = BF_FN_USER): F_t is the Jacobian of the caller's dynamics with respect to
 * the state at (m_t, q0, u_t) by forward-mode dual numbers, the one the filter's predict used; the kernels are compiled by
 * hiprtc on first use through the handle -- n <= 8: registers, one lane per trajectory, both data paths ("rts_load_mode"),
 * at most 64 parameters; larger n and "force_generic": one workgroup per trajectory, state in LDS.  BF_EINVAL for a handle
 * made for other dimensions or another device.  A handle that holds only the emission (or a log-density) runs the registry
 * instances: a backward pass never reads the emission.  BF_EUNSUPPORTED for BF_FN_USER without a handle and for
 * model->flags != 0.  (The unscented smoother below and bf_pf_backward_sample_f32 do not serve dynamics from source.) */
int bf_eks_smoother_f32(const bf_model* model, const bf_cstream* u, const bf_out_desc* filtered, int64_t B, int64_t T,
                        const bf_smooth_carry* carry, const bf_smooth_desc* out, void* stream);

/* Unscented RTS smoother for registry dynamics (K = 1; the streams of bf_ugsf_ukf_f32 with one component, update -> predict
 * order: filtered m_t, P_t and the predictions m-_{t+1}, P-_{t+1} at index t, all required).  u: the filter's inputs.
 * With L = n + dq, lambda = alpha^2 (L + kappa) - L, c = sqrt(L + lambda), w = 1 / (2 (L + lambda)) (the prediction's constants):
 *   R_t = symmetric square root of P_t (eigenvalues clamped at 0, lower triangle read: the root the filter's predict formed at t)
 *   s_j = c R_t[j, :],  j = 0 ... n-1
 *   X_t = w sum_j ( f(m_t + s_j, q0, u_t) - f(m_t - s_j, q0, u_t) ) s_j^T      (X[k][i] = Cov(x_{t+1,k}, x_{t,i} | y_{1:t}))
 * takes the place of F_t P_t above; everything after it is unchanged: Cholesky of P-_{t+1} without jitter, G_t = (P-^-1 X_t)^T,
 * m^s, P^s, C_t = G_t P^s_{t+1}; the last step without a carry is copied; a P- that is not positive definite gives NaN from
 * that step backwards.  The sigma points that perturb only the noise have zero state deviation: neither Q nor its root is
 * read, and the centre term and the predicted mean cancel by symmetry.  For f = A x + G q, X_t = A P_t exactly (2 w c^2 = 1).
 * X_t is a difference of images 2 c |R_t| apart: its fp32 relative error is about 2^-24 |f(m_t)| / (c |P_t|^1/2), large for
 * alpha << 1 (1e-4 ... 2e-4 at alpha = 1e-3).
 * n on the register kernel as far as every instance builds without scratch, other n and "force_generic": one workgroup per
 * trajectory, state in LDS.  BF_EUNSUPPORTED for functions given as source (BF_FN_USER), for model->flags != 0 and for an n
 * beyond the LDS capacity (the message names the limit); BF_EINVAL for missing predicted streams and for ParamsUKF values
 * the filter refuses (alpha <= 0, L + lambda <= 0). */
int bf_uks_smoother_f32(const bf_model* model, const bf_ukf_params* uparams, const bf_cstream* u, const bf_out_desc* filtered,
                        int64_t B, int64_t T, const bf_smooth_carry* carry, const bf_smooth_desc* out, void* stream);

/* ---- Gaussian-sum smoothing: the backward pass of bf_gsf_ekf_f32 / bf_ugsf_ukf_f32 with K >= 1 components ---------------
 * In those filters the components never interact: each is an extended (unscented) Kalman chain started from its own
 * initial mean, coupled only through the weight recursion w_{t,k} ~ w_{t-1,k} p(y_t | y_{<t}, k).  The model is a mixture over
 * the index k of the initial component, so
 *   p(x_{0:T-1} | y_{0:T-1}) = sum_k w_{T-1,k} p(x_{0:T-1} | y_{0:T-1}, k):
 * the smoothed weights are the filter's weights at the LAST step of the whole series, constant in t, and smoothed component k
 * is the RTS pass of chain k -- the recursion of bf_eks_smoother_f32 (uparams == NULL; registry dynamics or dynamics from
 * source) or of bf_uks_smoother_f32 (uparams given) on chain (b, k), bit for bit.
 * Inputs: the K-component streams means / covs / pred_means / pred_covs, all required, element (b, k, t, e) at
 * ptr[b*sB + k*sK + t*sT + e*sE]; u is read at b; the carry is bf_smooth_carry with contiguous [B][K][n] / [B][K][n][n].
 * Outputs, at least one: the per-component streams (means and covs together, cross_covs optional, sK honoured) and the
 * collapsed moments (either or both; element (b, t, e) at ptr[b*sB + t*sT + e*sE], sK unused) with w = weights[b][.]:
 *   mu_t = sum_k w_k m^s_{k,t},   Sigma_t = sum_k w_k (P^s_{k,t} + (m^s_{k,t} - mu_t)(m^s_{k,t} - mu_t)^T)
 * (utils.collapse / bf_collapse_f32 with time-constant weights).  n <= 8 and K <= 64: formed inside the smoother, the chains of
 * a trajectory in adjacent lanes, the sum over k an adjacent-pair tree over the power of two >= K whose order depends on K
 * alone; with only collapsed outputs nothing per component is stored.  NaN weights or a NaN chain give NaN collapsed values
 * for that trajectory only.  K > 64, n > 8 and "force_generic": with the per-component streams present bf_collapse_f32's
 * kernel runs over them on the same stream (coll_mean / coll_cov must then be contiguous [B][T][E]); collapsed outputs alone
 * are BF_EUNSUPPORTED there and the message names the limit.
 * weights: DEVICE [B][K], required with a collapsed output.  Errors otherwise as the two smoothers above; BF_EINVAL for K < 1.
 * Asynchronous on `stream`, no allocation; "force_generic" and "rts_load_mode" honoured (the staged data path serves
 * per-component output on the contiguous reference layout, where the chains are B K one-component trajectories). */
typedef struct bf_gs_smooth_desc {
  bf_stream means;      /* E = n,   per component */
  bf_stream covs;       /* E = n*n, per component; given together with means */
  bf_stream cross_covs; /* E = n*n, optional, needs means / covs: entries as bf_smooth_desc's */
  bf_stream coll_mean;  /* E = n,   collapsed, optional */
  bf_stream coll_cov;   /* E = n*n, collapsed, optional */
  const float* weights; /* DEVICE [B][K] */
} bf_gs_smooth_desc;

/* ABI guard of bf_gs_smooth_desc and bf_gs_sample_desc (below); a size of 0 = not mirrored. */
int bf_gs_abi_check(size_t sizeof_gs_smooth_desc, size_t sizeof_gs_sample_desc);

int bf_gs_smoother_f32(const bf_model* model, const bf_ukf_params* uparams /* NULL = extended route */, const bf_cstream* u,
                       const bf_out_desc* filtered, int64_t B, int64_t T, int64_t K, const bf_smooth_carry* carry,
                       const bf_gs_smooth_desc* out, void* stream);

/* Joint draws from the smoothed mixture: sample (b, s) picks a component z ~ Cat(weights[b][.]) ONCE and is then the backward
 * sampling recursion of bf_effbs_sample_f32 (uparams == NULL) / bf_uffbs_sample_f32 on chain (b, z) with noise row (b, s); its
 * bits do not depend on S, on the other samples' components or on the launch shape.  (bf_sample_desc / bf_sample_carry and
 * the recursion are declared below.)
 *   c_j = the inclusive cumulative sum of weights[b][0..j] in index order, by sequential fp32 adds;
 *   z   = the smallest j with c_j > v c_{K-1}, clamped to K-1, v = the sample's uniform in [0, 1);
 *   c_{K-1} not finite or not > 0: the draw is invalid, z = -1, and that sample is NaN at every step and in the carry; other
 *   samples are untouched.
 * Noise: a stream, or keys[b] exactly as the samplers below (random.normal(keys[b], (S, T, n))).  Uniforms: comp_noise[B][S], or
 * comp_keys[b] -> the S values bf_random_uniform_f32(comp_keys[b], S) writes.  comp_in[B][S] (a later chunk's components, or
 * the caller's; values outside [0, K) count as invalid draws) replaces the draw; comp_out[B][S] receives the components.
 * BF_EINVAL for K < 1, for weights missing where a draw is needed, and for both or neither of comp_noise and comp_keys
 * without comp_in.  n <= 8: registers, one lane per (trajectory, sample); other n and "force_generic": one workgroup per
 * (trajectory, component) serving the samples of its component ("ffbs_spl" is not read).  Asynchronous, no allocation. */
struct bf_sample_carry;
typedef struct bf_gs_sample_desc {
  bf_stream samples;         /* E = n; the K axis is the sample s; required */
  bf_cstream noise;          /* standard normals, same indexing; ptr == NULL: drawn from keys */
  const uint32_t* keys;      /* DEVICE [B][2], required when noise.ptr == NULL */
  const float* weights;      /* DEVICE [B][K], required unless comp_in is given */
  const float* comp_noise;   /* DEVICE [B][S] uniforms in [0, 1) */
  const uint32_t* comp_keys; /* DEVICE [B][2] */
  const int32_t* comp_in;    /* DEVICE [B][S] */
  int32_t* comp_out;         /* DEVICE [B][S] */
} bf_gs_sample_desc;

int bf_gs_sample_f32(const bf_model* model, const bf_ukf_params* uparams /* NULL = extended route */, const bf_cstream* u,
                     const bf_out_desc* filtered, int64_t B, int64_t T, int64_t K, int32_t S, const struct bf_sample_carry* carry,
                     const bf_gs_sample_desc* out, void* stream);

/* ---- Posterior sampling: the backward half of forward-filter backward-sampling (dynamax's lgssm_posterior_sample) ----
 * Draws S joint trajectories x_{0:T-1} ~ p(x_{0:T-1} | y_{0:T-1}) per filtered trajectory from the streams the smoothers
 * read (same order, same F_t).  With xi_{s,t} in R^n standard normals:
 *   t = T-1 (no carry):  x_{T-1} = m_{T-1} + psdchol(P_{T-1}; diag P_{T-1}) xi_{T-1}
 *   t = T-2 ... 0:       Lp = chol(P-_{t+1})             (as the smoothers: lower triangle, no jitter, NaN if not PD)
 *   (with a carry:       W  = Lp^-1 (F_t P_t),  X = Lp^-T W,  G_t = X^T
 *    from t = T-1)       Sigma_t = P_t - W^T W           (symmetric by construction)
 *                        L_t = psdchol(Sigma_t; diag P_t)
 *                        x_t = m_t + G_t (x_{t+1} - m-_{t+1}) + L_t xi_t
 * psdchol(S; d): left-looking Cholesky without pivoting; when the pivot p_j = S_jj - sum_k L_jk^2 is not greater than
 * tau d_j, tau = 2^-17, column j of L is zero, diagonal included (a zero pivot of a PSD matrix implies a zero column:
 * singular G Q G^T, e.g. the constant-velocity model, is part of the definition and not an error).  xi = 0 gives the RTS
 * smoothed means.  One component (K = 1), flags == 0.
 * With bf_sampler_abi_check, the three samplers below, the unscented smoother above and the four entry points of the particle
 * smoother, and the three of the Gaussian-sum smoother and sampler above, this header declares 39 entry points (41 with the two of the
 * parallel-in-time Kalman filter above). */
typedef struct bf_sample_desc {
  bf_stream samples;    /* E = n; the K axis is the sample s: ptr[b*sB + s*sK + t*sT + e*sE]; required */
  bf_cstream noise;     /* standard normals, same indexing; ptr == NULL: drawn from keys */
  const uint32_t* keys; /* DEVICE [B][2], required when noise.ptr == NULL: trajectory b uses the S*T*n values
                           bf_random_normal_f32(keys[b], S*T*n, ...) writes, element (s, t, i) at (s*T + t)*n + i */
} bf_sample_desc;

/* Backward chunking (as bf_smooth_carry).  DEVICE pointers, contiguous [B][S][n].
 * x_in: the samples at the first step AFTER this chunk (NULL: the chunk ends at T-1).
 * x_out: receives the samples at the chunk's first step (NULL = not written).
 * The two fields are independent, unlike the m / P pairs of bf_smooth_carry: x_in without x_out (a chunk that takes a carry
 * and hands none on) and x_out without x_in are both valid calls, so there is no "half a carry" to reject. */
typedef struct bf_sample_carry {
  const float* x_in;
  float* x_out;
} bf_sample_carry;

/* ABI guard of the two sampler structs; a size of 0 = not mirrored. */
int bf_sampler_abi_check(size_t sizeof_sample_desc, size_t sizeof_sample_carry);

/* Posterior samples of the linear model.  filtered as in bf_rts_smoother_f32 (pred_* both NULL: recomputed, Q_steps
 * honoured).  carry may be NULL.  Asynchronous on `stream`, no allocation.  n <= 8: registers, one lane per (trajectory,
 * block of samples); other n and "force_generic": one workgroup per trajectory, matrices and samples in LDS
 * (BF_EUNSUPPORTED when n exceeds its capacity). */
int bf_ffbs_sample_f32(const bf_lgssm* model, const bf_out_desc* filtered, int64_t B, int64_t T, int32_t S,
                       const bf_sample_carry* carry, const bf_sample_desc* out, void* stream);

/* Parallel-in-time posterior sampler for few long trajectories: the model, streams, noise, carry and output of bf_ffbs_sample_f32
 * (both of its routes: predictions given, or both NULL and recomputed), with time cut into blocks of L steps that run on separate
 * lanes.  The backward-sampling step is an affine map x_t = G_t x_{t+1} + c_{s,t} of the sample at t+1, so a span of steps is
 * (E, g_s) with E shared by a trajectory's samples; spans combine without a solve (E = E_i E_j, g = E_i g_j + g_i; the scheme is
 * stated at the head of csrc/ffbs_pscan.hpp).  Three launches on `stream`, no waiting between workgroups: fold (one lane per
 * (trajectory, block, block of samples) builds the block's aggregate; the last block's is its first-step sample), scan (one
 * workgroup per (trajectory, sample) turns the aggregates into the sample at every block's first step), emit (one lane per
 * (trajectory, block, block of samples) runs the ordinary backward-sampling step of bf_ffbs_sample_f32 from the sample after
 * its block and stores through the strided view).
 * Inside a block the samples are the serial sampler's from that block's start: the last block, and with T <= L the whole call,
 * equals bf_ffbs_sample_f32 on the same streams and noise bit for bit; elsewhere the two agree to fp32 tolerance (1e-5
 * relative).  A sample's bits depend on (T, L), the route, its trajectory's streams and its own noise row (with keys: also on
 * (S, T), through element (s, t, i) = value (s T + t) n + i of S T n), not on B, the other samples, "ffbs_spl", the layout
 * or the workspace's contents.  With keys each normal is generated twice (fold and emit).  NaN and zero pivots are
 * bf_ffbs_sample_f32's (NaN from a step backwards, in that trajectory's samples only).
 * L: option "pfs_block" (4..4096; 0 = default: the largest of ceil(B ceil(S / 4) T / 65 536), the smallest s with
 * 250 s^2 >= T, and 16; at most 4096).  Samples per lane: option
 * "ffbs_spl" 0, 1, 2 or 4 (0: the smallest of 1, 2, 4 that holds S, 4 for S > 4).
 * workspace: a caller-owned DEVICE buffer of at least bf_ffbs_pscan_workspace_bytes(n, B, T, S, L) =
 *   4 B ceil(T / L) (n^2 + 2 S n) bytes, 4-byte aligned; its contents before and after the call mean nothing.
 * bf_ffbs_pscan_workspace_bytes: `block` = 0 reads "pfs_block" as the call would and else uses the default; a negative result is
 * a BF_E* code (B, T or S <= 0, a block length outside 4..4096, n that is not built, B S ceil(T / L) >= 2^31).
 * BF_EUNSUPPORTED: n > 6 (the parallel filter's limit; the message names it), a per-step Q (Q_steps > 1: "constant Q").
 * BF_EINVAL: NULL arguments (carry may be NULL), missing streams or output, one predicted stream without the other, B, T or
 * S <= 0, neither or both of noise and keys, "ffbs_spl" = 8, a workspace that is too small (the message names the bytes needed)
 * or misaligned.  Every check precedes the first HIP call.  With these two, this header declares 45 entry points. */
int64_t bf_ffbs_pscan_workspace_bytes(int32_t n, int64_t B, int64_t T, int32_t S, int32_t block); /* < 0: BF_E* */
int bf_ffbs_sample_pscan_f32(const bf_lgssm* model, const bf_out_desc* filtered, int64_t B, int64_t T, int32_t S,
                             const bf_sample_carry* carry, const bf_sample_desc* out,
                             void* workspace, int64_t workspace_bytes, void* stream);

/* Posterior samples over extended Kalman streams (pred_* required) for registry dynamics and for dynamics given as source
 * (model->user with dyn_id = BF_FN_USER: F_t by dual numbers as in bf_eks_smoother_f32, kernels compiled on first use; n <= 8:
 * registers at every "ffbs_spl" count, larger n and "force_generic": state in LDS; BF_EINVAL for a handle made for other
 * dimensions or another device; a handle holding only the emission runs the registry instances).  BF_EUNSUPPORTED for
 * BF_FN_USER without a handle and for model->flags != 0.  (bf_uffbs_sample_f32 does not serve dynamics from source.) */
int bf_effbs_sample_f32(const bf_model* model, const bf_cstream* u, const bf_out_desc* filtered, int64_t B, int64_t T,
                        int32_t S, const bf_sample_carry* carry, const bf_sample_desc* out, void* stream);

/* Posterior samples for registry dynamics over unscented streams (bf_ugsf_ukf_f32 with K = 1, pred_* required): the recursion
 * above with X_t of bf_uks_smoother_f32 in place of F_t P_t (W = Lp^-1 X_t, Sigma_t = P_t - W^T W, psdchol with tau = 2^-17,
 * x_t = m_t + G_t (x_{t+1} - m-_{t+1}) + L_t xi_t).  Errors as bf_uks_smoother_f32. */
int bf_uffbs_sample_f32(const bf_model* model, const bf_ukf_params* uparams, const bf_cstream* u, const bf_out_desc* filtered,
                        int64_t B, int64_t T, int32_t S, const bf_sample_carry* carry, const bf_sample_desc* out, void* stream);

/* ---- Particle smoothing: joint draws from a bootstrap particle filter's stored history -------------------------------
 * S joint trajectories x_{0:T-1} ~ p(x_{0:T-1} | y_{0:T-1}) per filtered trajectory from what bf_bpf_f32 wrote: weights
 * w[i,t], particles x[i,t,:] and (genealogy only) ancestors a[i,t] (identity on steps that did not resample).  Per sample s
 * and step t a uniform v[s,t] in [0,1) is given.
 *   draw(l, v):  M = max_i l_i;  e_i = exp(l_i - M);  c = inclusive cumulative sum of e in index order; the result is the
 *                smallest j with c_j > v c_{N-1}, clamped to N-1 ("greater than": in exact arithmetic a drawn particle never has e_j = 0).
 *                M not finite: the draw is INVALID.
 *   Backward simulation (bf_pf_backward_sample_f32):
 *     t = T-1 without a carry:   l_i = log w[i,T-1]
 *     every other step, and T-1 with a carry:
 *                                l_i = log w[i,t] - 1/2 |L^-1 (x~_{t+1} - mu_i)|^2,  mu_i = f(x[i,t], q0, u_{t+1}),
 *                                L = lower Cholesky factor of F_q Q F_q^T (the common normalising constant is dropped)
 *     j_t = draw(l, v[s,t]),  x~_t = x[j_t,t,:]: an exact copy of a stored particle.
 *   Genealogy (bf_pf_trace_sample_f32): j_{T-1} = draw(log w[:,T-1], v[s,T-1]) (only that uniform is used),
 *     j_{t-1} = a[j_t,t], x~_t = x[j_t,t,:].  With the same uniforms both methods return the same x~_{T-1}.
 *   An invalid draw (the filter went NaN, or every logit overflowed) writes NaN and index -1 at that step and at every earlier
 *   step of that sample, and into the carry; other samples and trajectories are untouched.
 *   The arithmetic is fp32 with the hardware's log / exp; the order of the maximum and of the cumulative sum depends on N
 *   alone (csrc/pf_sampler.hpp), so a sample's bits do not depend on S, on B or on which samples share a launch. */
typedef struct bf_pf_history {
  const float* weights;   /* element (b,i,t) at weights[b*w_sB + i*w_sN + t*w_sT]: the strides of bf_bpf_out */
  int64_t w_sB, w_sN, w_sT;
  const float* particles; /* element (b,i,t,d) at particles[b*x_sB + i*x_sN + t*x_sT + d] */
  int64_t x_sB, x_sN, x_sT;
  const int32_t* ancestors; /* the weights' strides; required by bf_pf_trace_sample_f32 only */
} bf_pf_history;

typedef struct bf_pf_sample_desc {
  bf_stream samples;    /* E = n; the K axis is the sample s: ptr[b*sB + s*sK + t*sT + e*sE]; required */
  int32_t* indices;     /* optional: the drawn particle indices j, contiguous [B][S][T] */
  const float* noise;   /* uniforms in [0,1), element (b,s,t) at noise[b*z_sB + s*z_sS + t*z_sT]; or NULL and keys given */
  int64_t z_sB, z_sS, z_sT;
  const uint32_t* keys; /* DEVICE [B][2]: trajectory b uses the S*T values bf_random_uniform_f32(keys[b], S*T, ...) writes,
                           element (s,t) at s*T + t.  Exactly one of noise and keys. */
} bf_pf_sample_desc;

/* Backward chunking: the LAST chunk of steps first; its outputs are the next (earlier) chunk's inputs.  DEVICE pointers.
 * x_in [B][S][n]: the samples at the first step AFTER this chunk (NULL: the chunk ends at T-1); u_in [B]: the input u of that
 * step (NULL = zeros); a_in [B][S] (genealogy): the slot a[j,t] of that step, i.e. this chunk's j at its last step.
 * x_out / a_out: receive x~ at this chunk's first step and the slot a[j_{t0},t0] (NULL = not written).  Backward simulation reads
 * x_in / u_in and writes x_out; the genealogy reads a_in and writes x_out / a_out. */
typedef struct bf_pf_sample_carry {
  const float* x_in;
  const float* u_in;
  const int32_t* a_in;
  float* x_out;
  int32_t* a_out;
} bf_pf_sample_carry;

/* ABI guard of the three particle-smoother structs; a size of 0 = not mirrored. */
int bf_pf_sampler_abi_check(size_t sizeof_history, size_t sizeof_sample_desc, size_t sizeof_sample_carry);

/* Backward simulation.  model->ssm carries the registry dynamics, q0 and a constant Q (m0 / P0 / lp_cov and the emission are
 * not read); u: the filter's inputs (NULL or u->ptr == NULL = zeros).  State dimensions 1 ... 16, N <= 4096.
 * BF_EUNSUPPORTED, each naming the genealogy method: F_q Q F_q^T not positive definite (float64 Cholesky, pivot <= 2^-17 of
 * the diagonal: e.g. the constant-velocity and manoeuvring-target models, dq < n), dynamics given as source, N > 4096; also
 * for model->ssm.flags != 0 and Q_steps > 1.  Asynchronous on `stream`, no allocation. */
int bf_pf_backward_sample_f32(const bf_bpf_model* model, const bf_cstream* u, const bf_pf_history* history, int64_t B, int64_t T,
                              int32_t N, int32_t S, const bf_pf_sample_carry* carry, const bf_pf_sample_desc* out, void* stream);

/* Genealogy tracing: needs no model (any f, any Q, any N); n = the state dimension.  An ancestor entry outside [0, N) ends
 * the path as an invalid draw does. */
int bf_pf_trace_sample_f32(const bf_pf_history* history, int64_t B, int64_t T, int32_t N, int32_t n, int32_t S,
                           const bf_pf_sample_carry* carry, const bf_pf_sample_desc* out, void* stream);

/* jax.random.uniform(key, (count,)) in [0, 1), written to a HOST buffer (beside bf_random_normal_f32). */
int bf_random_uniform_f32(const uint32_t key[2], int64_t count, float* host_out);

/* Bytes one (trajectory, timestep) moves for the streams enabled in `out`: the algorithmic
 * traffic figure of SURVEY.md 8(d)  (4m + 4K(1 + 2n + 2n^2) for all five streams). */
int64_t bf_bytes_per_step(int32_t n, int32_t m, int32_t K, const bf_out_desc* out);

#ifdef __cplusplus
}
#endif
#endif /* BAYESFILT_H_ */
