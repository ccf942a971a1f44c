// Host side of the RTS smoother (rts_smoother.hpp): validation of the layouts, the register instances for n <= 8 and the
// run-time-dimension kernel for every other n (one wave per trajectory, the smoother's matrices in LDS).
//
// Register instances (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): every instance, n = 1 ... 8, both data paths,
// all three dynamics kinds, builds without scratch.  Strided path, VGPRs (arch + acc) / waves per SIMD: n = 1: 24-48 / 8,
// n = 2: 44-67 / 7-8, n = 3: 79-104 / 4-6, n = 4: 131-168 / 3, n = 5: 189-206 / 2, n = 6 ... 8: 266-481 / 1 (the five
// n x n matrices of a step plus the carry spill into the accumulation registers, not to memory).  Staged path (n <= 4,
// plus the chunk's prefetch registers): n = 1: 76-114 / 4-6, n = 2: 125-180 / 2-4, n = 3: 261-357 / 1, n = 4: 255-343 / 1-2.
// The run-time-dimension kernel serves n > 8 and "force_generic" = 1.
//
// Unscented route (RTS_UNSC: sym_sqrt<N> and the 2 n sigma-point images before the step; strided path only -- the route is
// bound by the root's arithmetic, not by its loads).  The predictions are loaded after the root, when its 2 n^2 registers
// are free again; with that every instance n = 1 ... 8 builds without scratch, so the register limit is 8 (RTS_UNSC_REG_MAX).
// VGPRs (arch + acc) / waves per SIMD: n = 1: 35 / 8, n = 2: 62 / 8, n = 3: 105 / 4, n = 4: 170 / 2, n = 5: 235 / 2,
// n = 6: 346 / 1, n = 7: 447 / 1, n = 8: 496 / 1.  Run-time-dimension kernel: rts_generic_kernel<true> 130 VGPRs, 3 waves per
// SIMD; rts_generic_kernel<false> (every other kind) 112 VGPRs, 4 waves, as before the route existed.
//
// Source route (RTS_EXT_USER: F_t from n dual-number evaluations of the caller's dynamics; kernels compiled at run time,
// jit_source.hip JIT_RTS_REGS / JIT_RTS_GENERIC).  Measured on a Lorenz-96 twin written as source (a loop over BF_N, dq = n),
// hipcc -Rpass-analysis=kernel-resource-usage, gfx950, -ffp-contract=off: every instance n = 1 ... 8 builds without scratch,
// so the register limit of the route is 8 (RTS_USER_REG_MAX) for that function; a caller's function with more live values
// may spill where this one does not.  VGPRs (arch + acc) / waves per SIMD, strided path: n = 1: 25 / 8, n = 2: 58 / 8,
// n = 3: 82 / 5, n = 4: 135 / 3, n = 5: 207 / 2, n = 6: 280 / 1, n = 7: 438 / 1, n = 8: 420 / 1; staged path: n = 1: 94 / 5,
// n = 2: 166 / 3, n = 3: 341 / 1, n = 4: 330 / 1.  Run-time-dimension kernel (lane d evaluates the function with the seed
// in state direction d; the per-lane arrays are BF_N long): n = 3: 87 VGPRs / 5 waves, n = 10: 101 / 4, n = 64: 281 / 1, no
// scratch.
#include "rts_generic.hpp"
#include "lgssm_pack.hpp"

namespace bf {

// ---- run-time-dimension kernel -----------------------------------------------------------------------------------
// One 64-lane workgroup per trajectory.  LDS: five n x ld matrices (P, P^s, P-, X, W) and four vectors; RTS_UNSC: two more
// matrices (V, Rt) and the root's vectors -- the root's iterate and its Newton scratch alias W and X, dead until the solve --
// which bounds the route at n <= 75 in 160 KiB (the host computes it from rts_gen_lds_floats).  Per step, with
// the helpers of rts_generic.hpp: W <- F_t, X = F P, [recompute: P-, m-], W <- chol(P-), X <- L^-T L^-1 X,
// C = X^T P^s (straight to HBM), m^s <- m + X^T (m^s - m-), P^s <- P^s - P-, P- <- X^T (P^s), P <- P + P- X, swap P / P^s.
// RTS_UNSC: two more matrices (the root's eigenvectors and the root) and the root's vectors (rts_generic.hpp: RtsUnscLds)
template <bool UNSC>
__global__ void __launch_bounds__(64) rts_generic_kernel(RtsGen c, GenModel g, RtsViews v, long long T) {
  rts_generic_body<UNSC, false>(c, g, v, T);
}

// ---- host helpers --------------------------------------------------------------------------------------------------
// host helpers shared with the sampler (rts_generic.hpp)
void rts_lin_fill(const bf_lgssm* p, std::vector<float>& A, std::vector<float>& GQG, std::vector<float>& Gq0) {
  const int n = p->n, dq = p->dq, qs = p->Q_steps;
  A.assign(p->A, p->A + (size_t)n * n);
  GQG.assign((size_t)qs * n * n, 0.f);
  if (p->Q) for (int s = 0; s < qs; ++s) noise_cov(p->G, p->Q + (size_t)s * dq * dq, n, dq, &GQG[(size_t)s * n * n], n);
  Gq0.assign(n, 0.f);
  noise_mean(p->G, p->q0, n, dq, Gq0.data());
}

void rts_gen_lin_block(const bf_lgssm* p, bool recompute, const std::vector<float>& A, const std::vector<float>& GQG,
                       const std::vector<float>& Gq0, RtsGen& c, std::vector<float>& blk) {
  const int n = p->n;
  blk.clear();
  blk.insert(blk.end(), A.begin(), A.end());
  blk.insert(blk.end(), Gq0.begin(), Gq0.end());
  blk.insert(blk.end(), GQG.begin(), GQG.end());
  c.n = n;
  c.kind = recompute ? RTS_LIN_RECOMPUTE : RTS_LIN;
  c.A = reinterpret_cast<const float*>((size_t)0);
  c.Gq0 = reinterpret_cast<const float*>((size_t)n * n);
  c.GQG = reinterpret_cast<const float*>((size_t)n * n + n);
  c.q_tv = p->Q_steps > 1;
  c.dyn_id = 0;
  for (int i = 0; i < 8; ++i) c.dth[i] = 0.f;
  c.cu = c.wu = 0.f;
}

int rts_unsc_fill(const bf_model* p, const bf_ukf_params* up, RtsUnscHost& h) {
  const int n = p->n, dq = p->dq;
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

int rts_gen_unsc_block(const RtsUnscHost& h, int n, RtsGen& c, std::vector<float>& blk) {
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
  return BF_OK;
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

// contiguous reference rows of `rows` steps, every row 16-byte aligned
static inline bool rts_ref_stream(const SView& s, long long E, long long rows) {
  return s.p == nullptr || (s.sE == 1 && s.sT == E && s.sB == rows * E && (reinterpret_cast<uintptr_t>(s.p) % 16 == 0) &&
                            (rows * E) % 4 == 0);
}

static Option g_rts_load_mode{-1, OPT_RTS_LOAD_MODE};
Option& rts_load_mode_option() { return g_rts_load_mode; }

// The data path of a register launch: staged for whole waves of contiguous reference rows (stage_ok: RtsStage<N>::OK), strided
// otherwise.  Without a carry the cross-covariances have T-1 entries: their rows may be T-1 steps long as well as T (the kernel
// takes the row pitch from the view and never touches entry T-1; rts_ref_stream's ((T-1) E) % 4 test keeps every row on 16 bytes)
static int rts_pick_path(int n, bool stage_ok, bool load_pred, const RtsViews& v, long long B, long long T, int load_mode, bool* staged) {
  const bool cs_ok = rts_ref_stream(v.Cs, n * n, T) || (v.m_in == nullptr && T > 1 && rts_ref_stream(v.Cs, n * n, T - 1));
  bool staged_ok = stage_ok && rts_ref_stream(v.m, n, T) && rts_ref_stream(v.P, n * n, T) && rts_ref_stream(v.ms, n, T) &&
                   rts_ref_stream(v.Ps, n * n, T) && cs_ok;
  if (load_pred) staged_ok = staged_ok && rts_ref_stream(v.pm, n, T) && rts_ref_stream(v.pP, n * n, T);
  if (load_mode == RTS_STAGED && !staged_ok)
    return set_error(BF_EINVAL, "rts_load_mode = 2 needs n <= 4 and the contiguous reference layout with 16-byte aligned rows");
  *staged = staged_ok && load_mode != RTS_STRIDED && B >= 64;
  return BF_OK;
}

// the views of the trajectories from b_begin on
static RtsViews rts_shifted(const RtsViews& v, long long b_begin, int n) {
  RtsViews w = v;
  for (SView* s : {&w.m, &w.P, &w.pm, &w.pP, &w.ms, &w.Ps, &w.Cs}) if (s->p) s->p += b_begin * s->sB;
  if (w.m_in) w.m_in += b_begin * n;
  if (w.P_in) w.P_in += b_begin * n * n;
  if (w.m_out) w.m_out += b_begin * n;
  if (w.P_out) w.P_out += b_begin * n * n;
  if (w.u) w.u += b_begin * w.u_sB;
  return w;
}

template <int N, int KIND, class Arg>
static int launch_rts_n(const Arg& c, const float* d_gqg, const RtsViews& v, long long B, long long T, int load_mode,
                        hipStream_t stream) {
  using S = RtsStage<N>;
  bool staged = false;
  const int rc = rts_pick_path(N, S::OK, KIND != RTS_LIN_RECOMPUTE, v, B, T, load_mode, &staged);
  if (rc != BF_OK) return rc;
  long long b_main = 0;
  if constexpr (S::OK && KIND != RTS_UNSC) {  // (the unscented route is compute-bound: strided loads only)
    if (staged) {
      // the staged kernel takes whole waves; a ragged remainder goes through the strided one
      b_main = (B / 64) * 64;
      hipLaunchKernelGGL((rts_reg_kernel<N, RTS_STAGED, KIND, Arg>), dim3((unsigned)(b_main / 64)), dim3(64),
                         sizeof(float) * S::FLOATS, stream, c, d_gqg, v, b_main, T);
    }
  }
  if (b_main < B) {
    const long long nb = B - b_main;
    hipLaunchKernelGGL((rts_reg_kernel<N, RTS_STRIDED, KIND, Arg>), dim3((unsigned)((nb + 63) / 64)), dim3(64), 0, stream, c,
                       d_gqg, rts_shifted(v, b_main, N), nb, T);
  }
  BF_HIP_CHECK(hipGetLastError());
  return BF_OK;
}

static int launch_rts_generic(const RtsGen& c0, const GenModel& g, const std::vector<float>& blk, const RtsViews& v,
                              long long B, long long T, hipStream_t stream) {
  const size_t lds = sizeof(float) * rts_gen_lds_floats(c0.n, c0.kind);
  if (lds > 160 * 1024) {
    if (c0.kind == RTS_UNSC) {
      int nmax = 1;
      while (sizeof(float) * rts_gen_lds_floats(nmax + 1, RTS_UNSC) <= 160 * 1024) ++nmax;
      return set_error(BF_EUNSUPPORTED, "unscented smoother: n = %d needs %zu bytes of LDS (160 KiB per workgroup: n <= %d)", c0.n, lds, nmax);
    }
    return set_error(BF_EUNSUPPORTED, "smoother: n = %d needs %zu bytes of LDS (160 KiB per workgroup)", c0.n, lds);
  }
  RtsGen c = c0;
  GenModel gg = g;
  const int rc = rts_gen_upload(c, gg, blk, stream);
  if (rc != BF_OK) return rc;
  if (B > 0x7fffffffLL) return set_error(BF_EINVAL, "smoother: B too large for the run-time-dimension kernel");
  auto kern = c.kind == RTS_UNSC ? rts_generic_kernel<true> : rts_generic_kernel<false>;
  if (lds > 64 * 1024) BF_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(kern, dim3((unsigned)B), dim3(64), lds, stream, c, gg, v, T);
  BF_HIP_CHECK(hipGetLastError());
  return BF_OK;
}

int launch_rts_linear(const bf_lgssm* p, const RtsViews& v, long long B, long long T, bool recompute, bool force_generic,
                      int load_mode, hipStream_t stream) {
  const int n = p->n;
  std::vector<float> A, GQG, Gq0;
  rts_lin_fill(p, A, GQG, Gq0);
  const bool tv = recompute && p->Q_steps > 1;
  if (!force_generic && n <= 8) {
    const float* d_gqg = nullptr;
    if (tv) {
      const void* dv = nullptr;
      const int rc = device_constants(GQG.data(), sizeof(float) * GQG.size(), stream, &dv);
      if (rc != BF_OK) return rc;
      d_gqg = static_cast<const float*>(dv);
    }
    auto go = [&](auto NC) -> int {
      constexpr int N = decltype(NC)::value;
      const RtsLin<N> c = rts_lin_arg<N>(A, GQG, Gq0);
      if (recompute) return launch_rts_n<N, RTS_LIN_RECOMPUTE>(c, d_gqg, v, B, T, load_mode, stream);
      return launch_rts_n<N, RTS_LIN>(c, nullptr, v, B, T, load_mode, stream);
    };
    BF_RTS_DIMS(n, go)
  }
  if (load_mode == RTS_STAGED) return set_error(BF_EINVAL, "rts_load_mode = 2 needs n <= 4 on the register kernel");
  std::vector<float> blk;
  RtsGen c;
  rts_gen_lin_block(p, recompute, A, GQG, Gq0, c, blk);
  GenModel g;
  std::memset(&g, 0, sizeof(g));
  return launch_rts_generic(c, g, blk, v, B, T, stream);
}

int launch_rts_user(const bf_model* p, const RtsViews& v, long long B, long long T, bool force_generic, int load_mode,
                    hipStream_t stream);

int launch_rts_ext(const bf_model* p, const RtsViews& v, long long B, long long T, bool force_generic, int load_mode,
                   hipStream_t stream) {
  if (p->user && p->dyn_id == BF_FN_USER) return launch_rts_user(p, v, B, T, force_generic, load_mode, stream);
  GenModel g;
  std::vector<float> blk;
  int rc = gen_fill(p, T, g, blk);  // validates the registry ids and theta layouts
  if (rc != BF_OK) return rc;
  const int n = p->n;
  if (!force_generic && n <= 8) {
    auto go = [&](auto NC) -> int {
      constexpr int N = decltype(NC)::value;
      return launch_rts_n<N, RTS_EXT>(rts_ekf_arg<N>(p, g), nullptr, v, B, T, load_mode, stream);
    };
    BF_RTS_DIMS(n, go)
  }
  if (load_mode == RTS_STAGED) return set_error(BF_EINVAL, "rts_load_mode = 2 needs n <= 4 on the register kernel");
  RtsGen c;
  std::memset(&c, 0, sizeof(c));
  c.n = n;
  c.kind = RTS_EXT;
  return launch_rts_generic(c, g, blk, v, B, T, stream);
}

// ---- source route (RTS_EXT_USER): the register kernels compiled at run time around the caller's dynamics ------------------
// (RTS_USER_REG_MAX, rts_generic.hpp: the largest n of the route on the register kernels -- every instance up to it, both
// data paths of the smoother and the four samples-per-lane counts of the sampler, builds without scratch for the Lorenz-96
// twin written as source; header comment)
int rts_user_fill(const bf_model* p, RtsUserHost& h) {
  std::memset(&h, 0, sizeof(h));
  if (p->n_dyn_theta > 64)
    return set_error(BF_EUNSUPPORTED, "smoother / sampler: a dynamics function from source takes at most 64 parameters (got %d)", p->n_dyn_theta);
  for (int i = 0; i < p->n_dyn_theta; ++i) h.theta[i] = p->dyn_theta[i];
  for (int i = 0; i < p->dq; ++i) h.q0[i] = p->q0 ? p->q0[i] : 0.f;
  return BF_OK;
}

// the run-time-dimension kernels' constants of the source route: q0 | theta on the device, g.q0 / g.dyn_theta pointing into it
int rts_user_gen_model(const bf_model* p, GenModel& g, hipStream_t stream) {
  std::memset(&g, 0, sizeof(g));
  g.dyn_id = DYN_USER; g.emi_id = p->emi_id; g.n = p->n; g.dq = p->dq; g.m = p->m; g.dr = p->dr;
  const int nth = p->n_dyn_theta > 0 ? p->n_dyn_theta : 0;
  std::vector<float> blk((size_t)p->dq + nth + 1, 0.f);
  for (int i = 0; i < p->dq; ++i) blk[i] = p->q0 ? p->q0[i] : 0.f;
  for (int i = 0; i < nth; ++i) blk[(size_t)p->dq + i] = p->dyn_theta[i];
  const void* dv = nullptr;
  const int rc = device_constants(blk.data(), sizeof(float) * blk.size(), stream, &dv);
  if (rc != BF_OK) return rc;
  g.q0 = static_cast<const float*>(dv);
  g.dyn_theta = g.q0 + p->dq;
  return BF_OK;
}

static int launch_rts_user_generic(const bf_model* p, const RtsViews& v, long long B, long long T, hipStream_t stream) {
  const int n = p->n;
  const size_t lds = sizeof(float) * rts_gen_lds_floats(n, RTS_EXT_USER);
  if (lds > 160 * 1024) return set_error(BF_EUNSUPPORTED, "smoother: n = %d needs %zu bytes of LDS (160 KiB per workgroup)", n, lds);
  if (B > 0x7fffffffLL) return set_error(BF_EINVAL, "smoother: B too large for the run-time-dimension kernel");
  RtsGen c;
  std::memset(&c, 0, sizeof(c));
  c.n = n;
  c.kind = RTS_EXT_USER;
  GenModel g;
  int rc = rts_user_gen_model(p, g, stream);
  if (rc != BF_OK) return rc;
  hipFunction_t fn = nullptr;
  if ((rc = user_kernel(p->user, JIT_RTS_GENERIC, 0, 0, JIT_SPEC_USER, &fn)) != BF_OK) return rc;
  RtsViews w = v;
  long long T_ = T;
  void* args[] = {&c, &g, &w, &T_};
  return launch_user_kernel(p->user, 64, (unsigned)B, lds, stream, args, fn);
}

int launch_rts_user(const bf_model* p, const RtsViews& v, long long B, long long T, bool force_generic, int load_mode,
                    hipStream_t stream) {
  const int n = p->n;
  if (force_generic || n > RTS_USER_REG_MAX) {
    if (load_mode == RTS_STAGED) return set_error(BF_EINVAL, "rts_load_mode = 2 needs n <= 4 on the register kernel");
    return launch_rts_user_generic(p, v, B, T, stream);
  }
  RtsUserHost h;
  int rc = rts_user_fill(p, h);
  if (rc != BF_OK) return rc;
  bool staged = false;
  size_t stage_bytes = 0;
  auto dims = [&](auto NC) -> int {
    using S = RtsStage<decltype(NC)::value>;
    stage_bytes = sizeof(float) * S::FLOATS;
    return rts_pick_path(decltype(NC)::value, S::OK, true, v, B, T, load_mode, &staged);
  };
  auto pick = [&]() -> int { BF_RTS_DIMS(n, dims) };
  if ((rc = pick()) != BF_OK) return rc;
  long long b_main = 0, T_ = T;
  if (staged) {  // whole waves; a ragged remainder goes through the strided kernel, as in launch_rts_n
    hipFunction_t fn = nullptr;
    if ((rc = user_kernel(p->user, JIT_RTS_REGS, RTS_STAGED, 0, JIT_SPEC_USER, &fn)) != BF_OK) return rc;
    b_main = (B / 64) * 64;
    RtsViews w = v;
    void* args[] = {&h, &w, &b_main, &T_};
    BF_HIP_CHECK(hipModuleLaunchKernel(fn, (unsigned)(b_main / 64), 1, 1, 64, 1, 1, (unsigned)stage_bytes, stream, args, nullptr));
  }
  if (b_main < B) {
    hipFunction_t fn = nullptr;
    if ((rc = user_kernel(p->user, JIT_RTS_REGS, RTS_STRIDED, 0, JIT_SPEC_USER, &fn)) != BF_OK) return rc;
    long long nb = B - b_main;
    RtsViews w = rts_shifted(v, b_main, n);
    void* args[] = {&h, &w, &nb, &T_};
    BF_HIP_CHECK(hipModuleLaunchKernel(fn, (unsigned)((nb + 63) / 64), 1, 1, 64, 1, 1, 0, stream, args, nullptr));
  }
  return BF_OK;
}

// Largest n of the unscented route on the register kernel: every instance up to it builds without scratch (header comment)
enum { RTS_UNSC_REG_MAX = 8 };

int launch_rts_unsc(const bf_model* p, const bf_ukf_params* up, const RtsViews& v, long long B, long long T, bool force_generic,
                    int load_mode, hipStream_t stream) {
  RtsUnscHost h;
  int rc = rts_unsc_fill(p, up, h);
  if (rc != BF_OK) return rc;
  const int n = p->n;
  if (load_mode == RTS_STAGED) return set_error(BF_EINVAL, "rts_load_mode = 2 is not offered on the unscented route");
  if (!force_generic && n <= RTS_UNSC_REG_MAX) {
    auto go = [&](auto NC) -> int {
      constexpr int N = decltype(NC)::value;
      if constexpr (N <= RTS_UNSC_REG_MAX) return launch_rts_n<N, RTS_UNSC>(rts_unsc_arg<N>(h), nullptr, v, B, T, RTS_STRIDED, stream);
      else return set_error(BF_EUNSUPPORTED, "no register instance");
    };
    BF_RTS_DIMS(n, go)
  }
  RtsGen c;
  std::vector<float> blk;
  if ((rc = rts_gen_unsc_block(h, n, c, blk)) != BF_OK) return rc;
  GenModel g;
  std::memset(&g, 0, sizeof(g));
  return launch_rts_generic(c, g, blk, v, B, T, stream);
}

}  // namespace bf

namespace bf {

// bf_out_desc / bf_smooth_carry / bf_smooth_desc -> RtsViews, with the checks both entry points share
int rts_views(const bf_out_desc* f, const bf_smooth_carry* carry, const bf_smooth_desc* out, const bf_cstream* u, long long B,
              long long T, int n, bool need_pred, int (*launch)(const RtsViews&, void*), void* ctx) {
  if (!f->means.ptr || !f->covs.ptr) return set_error(BF_EINVAL, "filtered means and covariances are required");
  if (need_pred && (!f->pred_means.ptr || !f->pred_covs.ptr))
    return set_error(BF_EINVAL, "the extended and the unscented smoother need the predicted means and covariances");
  if (!out->means.ptr || !out->covs.ptr) return set_error(BF_EINVAL, "smoothed means and covariances are required outputs");
  if (carry && ((carry->m_in == nullptr) != (carry->P_in == nullptr)))
    return set_error(BF_EINVAL, "carry.m_in and carry.P_in are given together or not at all");
  if (carry && ((carry->m_out == nullptr) != (carry->P_out == nullptr)))
    return set_error(BF_EINVAL, "carry.m_out and carry.P_out are given together or not at all");
  (void)n;
  RtsViews v;
  std::memset(&v, 0, sizeof(v));
  v.m = make_sview(f->means);
  v.P = make_sview(f->covs);
  v.pm = make_sview(f->pred_means);
  v.pP = make_sview(f->pred_covs);
  v.ms = make_sview(out->means);
  v.Ps = make_sview(out->covs);
  v.Cs = make_sview(out->cross_covs);
  if (carry) {
    v.m_in = carry->m_in;
    v.P_in = carry->P_in;
    v.m_out = carry->m_out;
    v.P_out = carry->P_out;
  }
  if (u && u->ptr) {
    v.u = u->ptr;
    v.u_sB = u->sB;
    v.u_sT = u->sT;
  }
  (void)B;
  (void)T;
  return launch(v, ctx);
}

}  // namespace bf
