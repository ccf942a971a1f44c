// Host side of the backward family that neither product owns (backward_host.hpp): the model validation, the route
// resolution with the routes' constant fills, and the constant blocks of the run-time-dimension kernels.  No kernel.
#include <cmath>
#include "backward_host.hpp"
#include "lgssm_pack.hpp"

namespace bf {

// ---- model validation ----------------------------------------------------------------------------------------------
int backward_check_lgssm(const bf_lgssm* p) {
  if (p->n <= 0 || p->dq <= 0) return set_error(BF_EINVAL, "non-positive model dimension");
  if (!p->A) return set_error(BF_EINVAL, "A is required");
  if (!p->G && p->dq != p->n) return set_error(BF_EINVAL, "G == NULL requires dq == n");
  return BF_OK;
}

int backward_check_recompute(const bf_lgssm* p, long long T) {
  if (!p->Q) return set_error(BF_EINVAL, "recomputing the predictions needs Q");
  if (p->Q_steps < 1 || (p->Q_steps > 1 && p->Q_steps != T)) return set_error(BF_EINVAL, "Q_steps must be 1 or T = %lld", T);
  return BF_OK;
}

int backward_check_source(const bf_model* p, const char* noun, bool unscented) {
  if (unscented) {
    if (p->user || p->dyn_id == BF_FN_USER || p->emi_id == BF_FN_USER)
      return set_error(BF_EUNSUPPORTED, "the %s serves registry dynamics; functions given as source are not supported", noun);
  } else if (!p->user && (p->dyn_id == BF_FN_USER || p->emi_id == BF_FN_USER)) {
    return set_error(BF_EUNSUPPORTED, "the %s serves functions given as source through bf_model.user (bf_user_model_create); it is NULL", noun);
  }
  if (p->flags != 0) return set_error(BF_EUNSUPPORTED, "the %s needs the JAX path's update -> predict streams (flags = 0)", noun);
  if (p->user) {  // dynamics from source: the kernels built around them; an emission from source is never read
    int rc = check_user_model(p->user, p);
    if (rc == BF_OK && p->dyn_id == BF_FN_USER) rc = check_user_device(p->user);
    if (rc != BF_OK) return rc;
  }
  return BF_OK;
}

int backward_check_dims(const bf_model* p) {
  if (p->n <= 0 || p->m <= 0 || p->dq <= 0 || p->dr <= 0) return set_error(BF_EINVAL, "non-positive model dimension");
  if (!p->Q || !p->R) return set_error(BF_EINVAL, "Q and R are required");
  return BF_OK;
}

// ---- route resolution ----------------------------------------------------------------------------------------------
// (lgssm_pack.hpp: the bits the filters upload)
int backward_route(const bf_lgssm* p, bool recompute, BackwardRoute& r) {
  const int n = p->n, dq = p->dq, qs = p->Q_steps;
  r.kind = recompute ? RTS_LIN_RECOMPUTE : RTS_LIN;
  r.n = n;
  r.lin = p;
  r.A.assign(p->A, p->A + (size_t)n * n);
  r.GQG.assign((size_t)qs * n * n, 0.f);
  if (p->Q) for (int s = 0; s < qs; ++s) noise_cov(p->G, p->Q + (size_t)s * dq * dq, n, dq, &r.GQG[(size_t)s * n * n], n);
  r.Gq0.assign(n, 0.f);
  noise_mean(p->G, p->q0, n, dq, r.Gq0.data());
  return BF_OK;
}

int backward_route(const bf_model* p, long long T, BackwardRoute& r) {
  r.n = p->n;
  r.model = p;
  if (p->user && p->dyn_id == BF_FN_USER) {  // the source route: nothing of the registry
    r.kind = RTS_EXT_USER;
    return BF_OK;
  }
  r.kind = RTS_EXT;
  return gen_fill(p, T, r.g, r.blk);
}

int backward_route(const bf_model* p, const bf_ukf_params* up, BackwardRoute& r) {
  RtsUnscHost& h = r.unsc;
  const int n = p->n, dq = p->dq;
  r.kind = RTS_UNSC;
  r.n = n;
  r.model = p;
  if (!(up->alpha > 0.f)) return set_error(BF_EINVAL, "ParamsUKF.alpha must be positive");
  bf_model q = *p;
  q.Q_steps = q.R_steps = 1;  // the noise covariances never enter X_t; the fill reads their first matrices only
  std::vector<uint32_t> words(ukf_model_words(n, dq, p->m, p->dr), 0u);
  const UkfModelView e = ukf_model_view_flat(words.data(), n, dq, p->m, p->dr);
  const int rc = fill_ukf_model_view(&q, up, e, 0);
  if (rc != BF_OK) return rc;
  h.cu = e.cp[0];
  h.wu = e.cp[1];
  if (!(h.cu > 0.f) || !std::isfinite(h.cu) || !std::isfinite(h.wu))
    return set_error(BF_EINVAL, "ParamsUKF: L + lambda = alpha^2 (n + dq + kappa) must be positive and finite (alpha = %g, kappa = %g, n + dq = %d)",
                     (double)up->alpha, (double)up->kappa, n + dq);
  h.dyn_id = p->dyn_id;
  for (int i = 0; i < 8; ++i) h.dth[i] = e.dth[i];
  h.A.assign(e.A, e.A + (size_t)n * n);
  h.Gq0.assign(n, 0.f);
  for (int i = 0; i < n; ++i) {  // F_q q0 as ukf_dyn adds it
    if (*e.g_identity) {
      h.Gq0[i] = e.q0[i];
    } else {
      float s = 0.f;
      for (int k = 0; k < dq; ++k) s = std::fmaf(e.Gm[i * dq + k], e.q0[k], s);
      h.Gq0[i] = s;
    }
  }
  return BF_OK;
}

int rts_user_fill(const bf_model* p, RtsUserHost& h) {
  std::memset(&h, 0, sizeof(h));
  if (p->n_dyn_theta > 64)
    return set_error(BF_EUNSUPPORTED, "smoother / sampler: a dynamics function from source takes at most 64 parameters (got %d)", p->n_dyn_theta);
  for (int i = 0; i < p->n_dyn_theta; ++i) h.theta[i] = p->dyn_theta[i];
  for (int i = 0; i < p->dq; ++i) h.q0[i] = p->q0 ? p->q0[i] : 0.f;
  return BF_OK;
}

// ---- the run-time-dimension kernels' constants ---------------------------------------------------------------------
void rts_gen_lin_block(const BackwardRoute& r, RtsGen& c, std::vector<float>& blk) {
  const int n = r.n;
  blk.clear();
  blk.insert(blk.end(), r.A.begin(), r.A.end());
  blk.insert(blk.end(), r.Gq0.begin(), r.Gq0.end());
  blk.insert(blk.end(), r.GQG.begin(), r.GQG.end());
  c.n = n;
  c.kind = r.kind;
  c.A = reinterpret_cast<const float*>((size_t)0);
  c.Gq0 = reinterpret_cast<const float*>((size_t)n * n);
  c.GQG = reinterpret_cast<const float*>((size_t)n * n + n);
  c.q_tv = r.lin->Q_steps > 1;
  c.dyn_id = 0;
  for (int i = 0; i < 8; ++i) c.dth[i] = 0.f;
  c.cu = c.wu = 0.f;
}

void rts_gen_unsc_block(const RtsUnscHost& h, int n, RtsGen& c, std::vector<float>& blk) {
  std::memset(&c, 0, sizeof(c));
  blk.clear();
  blk.insert(blk.end(), h.A.begin(), h.A.end());
  blk.insert(blk.end(), h.Gq0.begin(), h.Gq0.end());
  c.n = n;
  c.kind = RTS_UNSC;
  c.A = reinterpret_cast<const float*>((size_t)0);
  c.Gq0 = reinterpret_cast<const float*>((size_t)n * n);
  c.GQG = reinterpret_cast<const float*>((size_t)0);
  c.dyn_id = h.dyn_id;
  for (int i = 0; i < 8; ++i) c.dth[i] = h.dth[i];
  c.cu = h.cu;
  c.wu = h.wu;
}

int rts_gen_upload(RtsGen& c, GenModel& gg, const std::vector<float>& blk, hipStream_t stream) {
  const void* dv = nullptr;
  const int rc = device_constants(blk.data(), sizeof(float) * blk.size(), stream, &dv);
  if (rc != BF_OK) return rc;
  const float* base = static_cast<const float*>(dv);
  auto fix = [&](const float*& q) { q = base + reinterpret_cast<size_t>(q); };
  if (c.kind == RTS_EXT) {
    fix(gg.A); fix(gg.Hm); fix(gg.Gq0); fix(gg.Dr0); fix(gg.R); fix(gg.r0); fix(gg.GQG); fix(gg.DRD);
    fix(gg.q0); fix(gg.Q); fix(gg.dyn_theta); fix(gg.emi_theta);
  } else {
    fix(c.A); fix(c.GQG); fix(c.Gq0);
  }
  return BF_OK;
}

int backward_launch_user_generic(const bf_model* p, int jit_kind, const char* noun, void* c, void* views, long long B, long long T,
                                 size_t lds, hipStream_t stream, int K, void* last) {
  if (B * (K > 0 ? K : 1) > 0x7fffffffLL) return set_error(BF_EINVAL, "%s: B too large for the run-time-dimension kernel", noun);
  // the kernels' constants of the source route: q0 | theta on the device, g.q0 / g.dyn_theta pointing into it
  GenModel g;
  std::memset(&g, 0, sizeof(g));
  g.dyn_id = DYN_USER; g.emi_id = p->emi_id; g.n = p->n; g.dq = p->dq; g.m = p->m; g.dr = p->dr;
  const int nth = p->n_dyn_theta > 0 ? p->n_dyn_theta : 0;
  std::vector<float> blk((size_t)p->dq + nth + 1, 0.f);
  for (int i = 0; i < p->dq; ++i) blk[i] = p->q0 ? p->q0[i] : 0.f;
  for (int i = 0; i < nth; ++i) blk[(size_t)p->dq + i] = p->dyn_theta[i];
  const void* dv = nullptr;
  int rc = device_constants(blk.data(), sizeof(float) * blk.size(), stream, &dv);
  if (rc != BF_OK) return rc;
  g.q0 = static_cast<const float*>(dv);
  g.dyn_theta = g.q0 + p->dq;
  hipFunction_t fn = nullptr;
  if ((rc = user_kernel(p->user, jit_kind, 0, 0, JIT_SPEC_USER, &fn)) != BF_OK) return rc;
  void* args[] = {c, &g, views, &T, last ? last : &K};  // (the fifth: read by the Gaussian-sum kernels only, whose signatures end with it)
  return launch_user_kernel(p->user, 64, (unsigned)(B * (K > 0 ? K : 1)), lds, stream, args, fn);
}

}  // namespace bf
