// Host side of the forward family -- the six five-stream entry points (bf_kalman_filter_f32, bf_kalman_filter_pscan_f32,
// bf_gsf_ekf_f32, bf_ugsf_ukf_f32, bf_agsf_ekf_f32, bf_agsf_ukf_f32) and their launchers.  Host only: no kernel compiled at
// run time reads it (the headers jit_embed.py embeds keep their own copies of the view lines below).
//
// The refusals several entry points make in the same words are written here once; an entry point calls them in its own order,
// around the checks that are its own (which message wins when two things are wrong is part of what it promises:
// tests/test_forward_refusals_cpu.py).  A new five-stream filter writes its own entry point -- NULL arguments, sizes, whatever
// only it refuses -- and its kernel; the model and stream checks and the kernel-argument views come from here.
#pragma once
#include "bf_common.hpp"

namespace bf {

// Every check sets the error text and returns its code, BF_OK (= 0) when there is nothing to refuse.
inline int check_dimensions(int n, int dq, int m, int dr) {
  if (n <= 0 || m <= 0 || dq <= 0 || dr <= 0) return set_error(BF_EINVAL, "non-positive model dimension");
  return BF_OK;
}

inline int check_noise_steps(int Q_steps, int R_steps) {
  if (Q_steps < 1 || R_steps < 1) return set_error(BF_EINVAL, "Q_steps / R_steps must be >= 1");
  return BF_OK;
}
// bf_lgssm: dimensions; A, H, Q, R; G; D; Q_steps / R_steps
inline int check_lgssm(const bf_lgssm* p) {
  if (const int rc = check_dimensions(p->n, p->dq, p->m, p->dr)) return rc;
  if (!p->A || !p->H || !p->Q || !p->R) return set_error(BF_EINVAL, "A, H, Q, R are required");
  if (!p->G && p->dq != p->n) return set_error(BF_EINVAL, "G == NULL requires dq == n");
  if (!p->D && p->dr != p->m) return set_error(BF_EINVAL, "D == NULL requires dr == m");
  return check_noise_steps(p->Q_steps, p->R_steps);
}
// bf_model: dimensions; Q and R
inline int check_model(const bf_model* p) {
  if (const int rc = check_dimensions(p->n, p->dq, p->m, p->dr)) return rc;
  if (!p->Q || !p->R) return set_error(BF_EINVAL, "Q and R are required");
  return BF_OK;
}
// the observations and the carry-in every filter reads
inline int check_streams(const bf_cstream* y, const bf_carry* carry) {
  if (!y->ptr) return set_error(BF_EINVAL, "observations pointer is NULL");
  if (!carry->m_in || !carry->P_in) return set_error(BF_EINVAL, "carry.m_in and carry.P_in are required");
  return BF_OK;
}
inline int check_alpha(const bf_ukf_params* up) {
  if (!(up->alpha > 0.f)) return set_error(BF_EINVAL, "ParamsUKF.alpha must be positive");
  return BF_OK;
}

// The kernel arguments every forward kernel takes by value, from the caller's descriptors.  All eight output streams are
// filled, the collapsed pair included.  Only the Gaussian-sum register kernel (gsf_scan.hpp) writes that pair; every other
// launcher is reached with both pointers NULL -- the Kalman entry points and the run-time-dimension launchers refuse collapsed
// streams, bf_gsf_ekf_f32 takes the matrix-core route only without them -- so cm / cP are the zeros those launchers used to
// leave there, and their kernels get the same bytes.
struct ForwardViews {
  CView y;
  CarryView carry;
  OutViews out;
};
inline ForwardViews forward_views(const bf_cstream* y, const bf_carry* carry, const bf_out_desc* out) {
  const CView yv{y->ptr, y->sB, y->sT, y->sE};
  const CarryView cv{carry->w_in, carry->m_in, carry->P_in, carry->w_out, carry->m_out, carry->P_out};
  const OutViews ov{make_sview(out->weights), make_sview(out->means), make_sview(out->covs), make_sview(out->pred_means),
                    make_sview(out->pred_covs), make_sview(out->loglik), make_sview(out->coll_mean), make_sview(out->coll_cov)};
  return ForwardViews{yv, cv, ov};
}
// The inputs (U = UView or UViewG); `u` NULL or u->ptr NULL: zeros((T, 1)).
template <class U>
inline U input_view(const bf_cstream* u) {
  return U{u && u->ptr ? u->ptr : nullptr, u ? u->sB : 0, u ? u->sT : 0};
}

}  // namespace bf
