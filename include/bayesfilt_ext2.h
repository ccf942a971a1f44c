/*
 * bayesfilt_ext2.h -- entry points of libbayesfilt_hip.so added after include/bayesfilt_ext.h was frozen in its turn.
 *
 * Why a third header: bayesfilt.h and bayesfilt_ext.h both count their own declarations, and tests and generated bindings pin
 * those lists.  This header includes bayesfilt_ext.h (and through it bayesfilt.h), follows every convention stated there, uses
 * the structs unchanged and keeps BF_VERSION at 210: bf_abi_check covers all three.
 */
#ifndef BAYESFILT_EXT2_H_
#define BAYESFILT_EXT2_H_

#include "bayesfilt_ext.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Missing observations on the one-wave matrix-core Kalman kernel (one wave per chain, every matrix a single 32 x 32 tile).
 *
 * The contract is that of bf_kalman_filter_missing_anydim_f32 / bf_gsf_ekf_missing_anydim_f32, unchanged: a NaN y(b, t, a)
 * means "component a was not observed at step t"; the update conditions on the observed rows only, a step with none passes
 * means and covariances bit for bit with log-likelihood exactly 0 (the weights are renormalised only; K = 1: they stay 1), the
 * predict step always runs, +-Inf is not "missing" and poisons its trajectory, and only it.  Here a missing row stays in the
 * tile as a padded row for that step (zero row of H, unit noise, zero innovation; its log N(0; 0, 1) is taken off the
 * log-likelihood), which equals the reduced model to rounding: the psd_solve jitter of the embedded system differs from the
 * jitter on the reduced S_oo by a relative 1e-5 of 1e-6.  Complete data gives the plain matrix-core call's streams, carry and
 * log-likelihood bit for bit; chunks through bf_carry cut anywhere, inside a gap included, equal the single call bit for bit.
 *
 * Both functions take the argument lists of their plain twins.  Where the plain twin (bf_kalman_filter_f32 / bf_gsf_ekf_f32)
 * would run the one-wave matrix-core kernel -- 9 <= n <= 32, m <= 32 and (n >= 16 or m > 8), "kf_small_mode" not 0,
 * "force_generic" not set; for the Gaussian sum also a linear emission, flags == 0, K <= 64, linear or Lorenz-96 / sine
 * registry dynamics with identity noise input, and no function from source; per-step Q_t / R_t tables included -- they run its
 * MISSING instance.  Everywhere else, and when that launch answers BF_EUNSUPPORTED, they ARE the *_missing_anydim_f32 entry
 * points: the same refusals in the same order before the first HIP call (collapsed streams among them), the same kernel, the
 * same bits.  Models with 33 <= n <= 64 are not served by a matrix-core kernel here (the four-wave kernel takes no gaps).
 * With these two, the library exports 54 entry points: the 50 of bayesfilt.h, the 2 of bayesfilt_ext.h and these. */
int bf_kalman_filter_missing_tiles_f32(const bf_lgssm* model, const bf_cstream* y, int64_t B, int64_t T,
                                       const bf_carry* carry, const bf_out_desc* out, void* stream);
int bf_gsf_ekf_missing_tiles_f32(const bf_model* model, const bf_cstream* y, const bf_cstream* u, int64_t B, int64_t T,
                                 int32_t K, const bf_carry* carry, const bf_out_desc* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* BAYESFILT_EXT2_H_ */
