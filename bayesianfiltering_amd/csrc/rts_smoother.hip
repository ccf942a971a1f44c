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
static inline size_t rts_gen_lds_floats(int n, int kind) {
  const size_t base = 5 * (size_t)n * rts_gen_ld(n) + 4 * (size_t)n;
  return kind == RTS_UNSC ? base + 2 * (size_t)n * rts_gen_ld(n) + (size_t)rts_unsc_vec_floats(n) : base;
}

template <bool UNSC>
__global__ void __launch_bounds__(64) rts_generic_kernel(RtsGen c, GenModel g, RtsViews v, long long T) {
  const int tid = threadIdx.x;
  const long long b = blockIdx.x;
  const int n = c.n, ld = rts_gen_ld(n), nn = n * n;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* P = lds;
  float* Ps = P + n * ld;
  float* Pp = Ps + n * ld;
  float* X = Pp + n * ld;
  float* W = X + n * ld;
  float* m = W + n * ld;
  float* ms = m + n;
  float* mp = ms + n;
  float* tv = mp + n;
  const RtsUnscLds ul = rts_unsc_carve(tv + n, tv + n + n * ld, tv + n + 2 * n * ld, n);  // carved for RTS_UNSC only
  const bool want_c = v.Cs.p != nullptr;
  auto at = [&](const SView& s, long long t, int e) { return b * s.sB + t * s.sT + e * s.sE; };

  long long t = T - 1;
  if (v.m_in) {
    for (int e = tid; e < n; e += 64) ms[e] = v.m_in[b * n + e];
    for (int e = tid; e < nn; e += 64) Ps[(e / n) * ld + e % n] = v.P_in[b * nn + e];
  } else {
    for (int e = tid; e < n; e += 64) { const float x = v.m.p[at(v.m, t, e)]; ms[e] = x; v.ms.p[at(v.ms, t, e)] = x; }
    for (int e = tid; e < nn; e += 64) { const float x = v.P.p[at(v.P, t, e)]; Ps[(e / n) * ld + e % n] = x; v.Ps.p[at(v.Ps, t, e)] = x; }
    --t;
  }
  wave_lds_sync();
  for (; t >= 0; --t) {
    for (int e = tid; e < n; e += 64) m[e] = v.m.p[at(v.m, t, e)];
    for (int e = tid; e < nn; e += 64) P[(e / n) * ld + e % n] = v.P.p[at(v.P, t, e)];
    if (c.kind != RTS_LIN_RECOMPUTE) {
      for (int e = tid; e < n; e += 64) mp[e] = v.pm.p[at(v.pm, t, e)];
      for (int e = tid; e < nn; e += 64) Pp[(e / n) * ld + e % n] = v.pP.p[at(v.pP, t, e)];
    }
    wave_lds_sync();
    const float u0 = ((UNSC || c.kind == RTS_EXT) && v.u) ? v.u[b * v.u_sB + t * v.u_sT] : 0.f;
    rts_gen_linearize<UNSC>(c, g, u0, t, m, P, mp, Pp, X, W, tv, tid, ul);
    rts_gen_chol(n, Pp, W, tid);
    rts_gen_solve_lower(n, W, X, tid);  // X <- L^-T L^-1 X
    rts_gen_solve_upper(n, W, X, tid);
    wave_lds_sync();
    if (want_c) {
      for (int e = tid; e < nn; e += 64) {  // C = G P^s = X^T P^s
        const int i = e / n, j = e - i * n;
        float s = X[i] * Ps[j];
        for (int k = 1; k < n; ++k) s = fmaf(X[k * ld + i], Ps[k * ld + j], s);
        v.Cs.p[at(v.Cs, t, e)] = s;
      }
    }
    for (int i = tid; i < n; i += 64) tv[i] = ms[i] - mp[i];
    wave_lds_sync();
    for (int i = tid; i < n; i += 64) {
      float s = X[i] * tv[0];
      for (int k = 1; k < n; ++k) s = fmaf(X[k * ld + i], tv[k], s);
      ms[i] = m[i] + s;
    }
    for (int e = tid; e < nn; e += 64) {
      const int i = e / n, j = e - i * n;
      Ps[i * ld + j] = Ps[i * ld + j] - Pp[i * ld + j];
    }
    wave_lds_sync();
    for (int e = tid; e < nn; e += 64) {  // G D -> P-
      const int i = e / n, j = e - i * n;
      float s = X[i] * Ps[j];
      for (int k = 1; k < n; ++k) s = fmaf(X[k * ld + i], Ps[k * ld + j], s);
      Pp[i * ld + j] = s;
    }
    wave_lds_sync();
    for (int e = tid; e < nn; e += 64) {  // P + (G D) G^T -> P, which becomes P^s
      const int i = e / n, j = e - i * n;
      float s = Pp[i * ld] * X[j];
      for (int k = 1; k < n; ++k) s = fmaf(Pp[i * ld + k], X[k * ld + j], s);
      P[i * ld + j] = P[i * ld + j] + s;
    }
    wave_lds_sync();
    float* sw = P;
    P = Ps;
    Ps = sw;
    for (int e = tid; e < n; e += 64) v.ms.p[at(v.ms, t, e)] = ms[e];
    for (int e = tid; e < nn; e += 64) v.Ps.p[at(v.Ps, t, e)] = Ps[(e / n) * ld + e % n];
    wave_lds_sync();
  }
  if (v.m_out) for (int e = tid; e < n; e += 64) v.m_out[b * n + e] = ms[e];
  if (v.P_out) for (int e = tid; e < nn; e += 64) v.P_out[b * nn + e] = Ps[(e / n) * ld + e % n];
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

template <int N, int KIND, class Arg>
static int launch_rts_n(const Arg& c, const float* d_gqg, const RtsViews& v, long long B, long long T, int load_mode,
                        hipStream_t stream) {
  using S = RtsStage<N>;
  // without a carry the cross-covariances have T-1 entries: their rows may be T-1 steps long as well as T (the kernel
  // takes the row pitch from the view and never touches entry T-1; rts_ref_stream's ((T-1) E) % 4 test keeps every row on 16 bytes)
  const bool cs_ok = rts_ref_stream(v.Cs, N * N, T) || (v.m_in == nullptr && T > 1 && rts_ref_stream(v.Cs, N * N, T - 1));
  bool staged_ok = S::OK && rts_ref_stream(v.m, N, T) && rts_ref_stream(v.P, N * N, T) && rts_ref_stream(v.ms, N, T) &&
                   rts_ref_stream(v.Ps, N * N, T) && cs_ok;
  if (KIND != RTS_LIN_RECOMPUTE) staged_ok = staged_ok && rts_ref_stream(v.pm, N, T) && rts_ref_stream(v.pP, N * N, T);
  if (load_mode == RTS_STAGED && !staged_ok)
    return set_error(BF_EINVAL, "rts_load_mode = 2 needs n <= 4 and the contiguous reference layout with 16-byte aligned rows");
  const bool staged = staged_ok && load_mode != RTS_STRIDED && B >= 64;
  auto shifted = [&](long long b_begin) {
    RtsViews w = v;
    for (SView* s : {&w.m, &w.P, &w.pm, &w.pP, &w.ms, &w.Ps, &w.Cs}) if (s->p) s->p += b_begin * s->sB;
    if (w.m_in) w.m_in += b_begin * N;
    if (w.P_in) w.P_in += b_begin * N * N;
    if (w.m_out) w.m_out += b_begin * N;
    if (w.P_out) w.P_out += b_begin * N * N;
    if (w.u) w.u += b_begin * w.u_sB;
    return w;
  };
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
                       d_gqg, shifted(b_main), nb, T);
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

int launch_rts_ext(const bf_model* p, const RtsViews& v, long long B, long long T, bool force_generic, int load_mode,
                   hipStream_t stream) {
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
