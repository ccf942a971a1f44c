/*
 * bayesfilt_ext.h -- entry points of libbayesfilt_hip.so added after include/bayesfilt.h was frozen.
 *
 * Why a second header: bayesfilt.h counts its own declarations (its comments and the tests that pin them say "this header
 * declares 50 entry points"), and bindings generated from it rely on that list.  Functions that extend the library without
 * touching any struct are therefore declared here.  This header includes bayesfilt.h, follows every convention stated there
 * (extern "C", int status with the text in bf_last_error(), DEVICE pointers in the stream descriptors, the last argument a
 * hipStream_t passed as void*), uses its structs unchanged and keeps BF_VERSION at 210: bf_abi_check covers both.
 */
#ifndef BAYESFILT_EXT_H_
#define BAYESFILT_EXT_H_

#include "bayesfilt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Missing observations at ANY dimension: the run-time-dimension kernel (one workgroup per trajectory, state in LDS).
 *
 * The contract is that of bf_kalman_filter_missing_f32 / bf_gsf_ekf_missing_f32, unchanged: a NaN y(b, t, a) means "component a
 * was not observed at step t".  With o the components of the step that are not NaN, every component of the bank conditions on
 * the rows o only -- H_x[o, :], h(x)[o], (H_r R H_r^T)[o, o], state-dependent H_r included, the jitter on every entry of the
 * reduced S_oo -- and its log-likelihood is log N(v_o; 0, S_oo) with |o| in the log 2 pi term.  o empty: means and covariances
 * pass bit for bit, every log-likelihood is exactly 0 and the weights are renormalised only (K = 1: they stay 1).  The predict
 * step always runs, so trailing unobserved steps are a forecast.  Here the observed rows are really compacted (copies): what the
 * model computes for a missing row is never read again, so a NaN or Inf produced there does not leak.  +-Inf in y is not
 * "missing" and poisons its trajectory, and only it.  Complete data gives the plain run-time-dimension kernel's streams and carry
 * bit for bit; chunks through bf_carry cut anywhere, inside a gap included, equal the single call bit for bit.
 *
 * Both functions take the argument lists of their plain twins and ALWAYS run the run-time-dimension kernel, for every
 * (n, m, K) its LDS holds, small models included (the register kernels of the two *_missing_f32 entry points are faster where
 * they apply: n <= 8 and m <= 4).  Linear models with n >= 16 leave the matrix-core route here.  Registry models, models from
 * source (bf_user_model_create: the twin kernel is built on first use) and per-step Q_t / R_t tables are served.
 * Before the first HIP call they refuse, in this order: NULL arguments and non-positive sizes, and what the plain twins refuse
 * of the model and the carry (BF_EINVAL); collapsed streams (BF_EUNSUPPORTED); the legacy classes, flags != 0
 * (BF_EUNSUPPORTED); a handle that carries only a log-density (BF_EINVAL); a model whose tiles exceed the 160 KiB of LDS of a
 * workgroup (BF_EUNSUPPORTED, the message names the bytes).  "force_generic" is accepted and changes nothing.
 * With these two, the library exports 52 entry points: the 50 of bayesfilt.h and these. */
int bf_kalman_filter_missing_anydim_f32(const bf_lgssm* model, const bf_cstream* y, int64_t B, int64_t T,
                                        const bf_carry* carry, const bf_out_desc* out, void* stream);
int bf_gsf_ekf_missing_anydim_f32(const bf_model* model, const bf_cstream* y, const bf_cstream* u, int64_t B, int64_t T,
                                  int32_t K, const bf_carry* carry, const bf_out_desc* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* BAYESFILT_EXT_H_ */
