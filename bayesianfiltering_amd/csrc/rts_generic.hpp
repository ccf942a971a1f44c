// What the run-time-dimension kernels of the smoother (rts_smoother.hip) and of the posterior sampler (ffbs_sampler.hip)
// share: the per-step gain work on n x (n + 1) matrices in LDS (F_t, X = F P, the recomputed prediction, the Cholesky of
// P- and the two triangular solves), the constant block behind it and the model structs of the register kernels.
//
// The kernel bodies live here as device functions: the ahead-of-time kernels (rts_smoother.hip, ffbs_sampler.hip) and the
// entry points hiprtc compiles around a caller's dynamics (jit_source.hip: JIT_RTS_GENERIC / JIT_FFBS_GENERIC, the
// RTS_EXT_USER route for n above the register limit and "force_generic" = 1) are thin kernels around them.  The file is
// embedded for that purpose (jit_embed.py): device code and the structs and LDS sizes both sides read, nothing of the host
// (the family's host side is backward_host.hpp).
#pragma once
#include "rts_smoother.hpp"
#include "ffbs_sampler.hpp"
#include "generic_device.hpp"
#include "ugsf_generic_device.hpp"

namespace bf {

struct RtsGen {
  int n, kind;          // RTS_LIN, RTS_LIN_RECOMPUTE, RTS_EXT, RTS_UNSC, RTS_EXT_USER
  const float* A;       // [n][n]            (linear kinds; RTS_UNSC: linear dynamics)
  const float* GQG;     // [q_steps][n][n]   (recompute)
  const float* Gq0;     // [n]               (recompute; RTS_UNSC: F_q q0)
  int q_tv;
  // RTS_UNSC: the registry dynamics and the prediction's unscented constants c = sqrt(L + lambda), w = 1 / (2 (L + lambda))
  int dyn_id;
  float dth[8];
  float cu, wu;
};

__host__ __device__ inline int rts_gen_ld(int n) { return n + 1; }

// RTS_UNSC on the run-time-dimension kernels: LDS of the symmetric square root (ug_sym_sqrt) beyond what the kernels own.
// Its iterate lives in W, its Newton scratch in X (both are outputs of the step's linearisation, dead until then); the
// eigenvectors V and the root Rt are n x ld matrices of the caller's (the sampler lends Sg as V); the vectors follow.
struct RtsUnscLds {
  float *V, *Rt, *sd, *red, *rot;
};
__host__ __device__ inline int rts_unsc_vec_floats(int n) {
  const int nv = (n + 3) & ~3, h4 = (((n + 1) >> 1) + 3) & ~3;
  return 3 * nv + 4 * h4;  // sd [nv], red [2][nv], rot [ceil(n / 2)][4]
}
__host__ __device__ inline RtsUnscLds rts_unsc_carve(float* V, float* Rt, float* vec, int n) {
  const int nv = (n + 3) & ~3;
  return RtsUnscLds{V, Rt, vec, vec + nv, vec + 3 * nv};
}

// LDS floats of the smoother's run-time-dimension kernel
__host__ __device__ inline size_t rts_gen_lds_floats(int n, int kind) {
  const size_t base = 5 * (size_t)n * rts_gen_ld(n) + 4 * (size_t)n;
  return kind == RTS_UNSC ? base + 2 * (size_t)n * rts_gen_ld(n) + (size_t)rts_unsc_vec_floats(n) : base;
}

// the sampler's run-time-dimension kernel: the smoother's constants and the sample blocking
struct FfbsGen {
  RtsGen r;
  int S, SB;            // samples, samples per LDS block
};

// RTS_UNSC: one more matrix (the root; Sg holds the eigenvectors while it is taken) and the root's vectors
__host__ __device__ inline size_t ffbs_gen_unsc_floats(int n, int kind) {
  return kind == RTS_UNSC ? (size_t)n * rts_gen_ld(n) + (size_t)rts_unsc_vec_floats(n) : 0;
}
__host__ __device__ inline size_t ffbs_gen_mat_floats(int n, int kind) {
  return 5 * (size_t)n * rts_gen_ld(n) + 3 * (size_t)n + ffbs_gen_unsc_floats(n, kind);
}

#if defined(__HIPCC__) || defined(BF_JIT)
// The differences of the images of the n sigma-point pairs, D[j][k] = f_k(m + s_j, q0, u) - f_k(m - s_j, q0, u) with
// s_j = cu Rt[j, :] (pitch ld).  Linear, Lorenz-96 and sine dynamics: one work item per (pair, output row), the formulas and
// the per-entry operation order of ug_eval_dyn, whose points these are.  The registry functions of one fixed dimension
// (Lorenz-63, manoeuvring target, growth): a lane per pair, the point in registers (dyn_base_t).
template <int N>
__device__ __forceinline__ void rts_gen_unsc_pair(const RtsGen& c, float u0, const float* m, const float* row, float* Drow) {
#pragma clang fp contract(off)
  float xp[N], xm[N], fp[N], fm[N];
  BF_UNROLL for (int k = 0; k < N; ++k) {
    xp[k] = m[k] + c.cu * row[k];
    xm[k] = m[k] + (-c.cu) * row[k];
  }
  dyn_base_t<N, N, RtsGen>(c, xp, u0, fp);
  dyn_base_t<N, N, RtsGen>(c, xm, u0, fm);
  BF_UNROLL for (int k = 0; k < N; ++k) Drow[k] = (fp[k] + c.Gq0[k]) - (fm[k] + c.Gq0[k]);
}
__device__ __forceinline__ void rts_gen_unsc_images(const RtsGen& c, float u0, const float* m, const float* Rt, int ld, float* D,
                                                    int tid) {
#pragma clang fp contract(off)
  const int n = c.n;
  if (c.dyn_id == DYN_LORENZ63 || c.dyn_id == DYN_MANEUVER_BOT || c.dyn_id == DYN_GROWTH) {
    if (tid < n) {
      if (c.dyn_id == DYN_LORENZ63) rts_gen_unsc_pair<3>(c, u0, m, Rt + tid * ld, D + tid * ld);
      else if (c.dyn_id == DYN_MANEUVER_BOT) rts_gen_unsc_pair<4>(c, u0, m, Rt + tid * ld, D + tid * ld);
      else rts_gen_unsc_pair<1>(c, u0, m, Rt + tid * ld, D + tid * ld);
    }
    return;
  }
  for (int e = tid; e < n * n; e += 64) {
    const int j = e / n, i = e - j * n;
    const float* row = Rt + j * ld;
    float o[2];
    for (int sg = 0; sg < 2; ++sg) {
      const float cs = sg == 0 ? c.cu : -c.cu;
      auto X = [&](int k) { return m[k] + cs * row[k]; };
      float v;
      if (c.dyn_id == DYN_LINEAR) {
        float s = c.A[i * n] * X(0);
        for (int k = 1; k < n; ++k) s = fmaf(c.A[i * n + k], X(k), s);
        v = s + c.Gq0[i];
      } else if (c.dyn_id == DYN_LORENZ96) {
        const float alpha = c.dth[0], beta = c.dth[1], gamma = c.dth[2], dt = c.dth[3];
        const float xi = X(i), ax = X((i + n - 1) % n);
        const float bx = (c.dth[4] != 0.f) ? (X((i + 1) % n) - X((i + 2 * n - 2) % n)) : 0.f;
        v = xi + dt * (alpha * (ax * bx) - beta * xi + gamma);
        v += c.Gq0[i];
      } else {  // DYN_SINE
        v = sinf(c.dth[0] * X(i));
        v += c.Gq0[i];
      }
      o[sg] = v;
    }
    D[j * ld + i] = o[0] - o[1];
  }
}

// W <- F_t (registry dynamics; linear: A is read from the constant block), X = F P, [recompute: P- = X F^T + GQG_t,
// m- = F m + G q0].  One 64-lane wave; m, P (and, unless recomputed, m-, P-) are in LDS and synchronised on entry; X
// (and P-, m-) are synchronised on return.  RTS_UNSC: X = X_t of rts_smoother.hpp's contract instead -- Rt <- the root of P
// (ug_sym_sqrt, the filter's, Newton step included), W <- the image differences, X = w W^T (c Rt) as an LDS product.
// UNSC is a template parameter: the kernels of the other kinds carry none of the root's code or registers.
#ifdef BF_USER_DYN
// F_t of the source route (RTS_EXT_USER): lane d evaluates the caller's dynamics with the unit seed in state direction d and
// writes column d of F -- the state half of user_dyn_linearize (generic_device.hpp): no F_q, no noise covariance, none of
// its scratch.  g.q0 / g.dyn_theta: the noise bias and the caller's parameters in the constant block.
__device__ __forceinline__ void rts_gen_user_jacobian(const GenModel& g, const float* m, float u0, float* F, int ld, int tid) {
#pragma clang fp contract(off)
  constexpr int N = BF_N, DQ = BF_DQ;
  for (int d = tid; d < N; d += 64) {
    bfu::Dual xs[N], qs[DQ], out[N];
    BF_UNROLL for (int i = 0; i < N; ++i) xs[i] = bfu::Dual(m[i], i == d ? 1.0f : 0.0f);
    BF_UNROLL for (int k = 0; k < DQ; ++k) qs[k] = bfu::Dual(g.q0[k]);
    bfu::dynamics<bfu::Dual>(xs, qs, bfu::Dual(u0), g.dyn_theta, out);
    BF_UNROLL for (int i = 0; i < N; ++i) F[i * ld + d] = out[i].d;
  }
}
#endif

template <bool UNSC, bool USER = false>
__device__ __forceinline__ void rts_gen_linearize(const RtsGen& c, const GenModel& g, float u0, long long t, const float* m,
                                                  const float* P, float* mp, float* Pp, float* X, float* W, float* tv, int tid,
                                                  const RtsUnscLds& ul) {
  const int n = c.n, ld = rts_gen_ld(n), nn = n * n;
  if constexpr (UNSC) {
    ug_sym_sqrt<64>(P, ld, W, ul.V, ul.Rt, X, ld, ul.sd, ul.red, ul.rot, n, tid);
    rts_gen_unsc_images(c, u0, m, ul.Rt, ld, W, tid);
    wave_lds_sync();
    for (int e = tid; e < nn; e += 64) {  // X[k][i] = w sum_j D[j][k] s_j[i]
      const int k = e / n, i = e - k * n;
      float s = W[k] * (c.cu * ul.Rt[i]);
      for (int j = 1; j < n; ++j) s = fmaf(W[j * ld + k], c.cu * ul.Rt[j * ld + i], s);
      X[k * ld + i] = s * c.wu;
    }
    wave_lds_sync();
    return;
  }
  const float* F;
  int ldf;
  if constexpr (USER) {
#ifdef BF_USER_DYN
    rts_gen_user_jacobian(g, m, u0, W, ld, tid);
#endif
    wave_lds_sync();
    F = W;
    ldf = ld;
  } else if (c.kind == RTS_EXT) {
    gen_dyn_linearize<64>(g, m, u0, W, ld, tv, tid);
    wave_lds_sync();
    F = W;
    ldf = ld;
  } else {
    F = c.A;
    ldf = n;
  }
  for (int e = tid; e < nn; e += 64) {  // X = F P
    const int i = e / n, j = e - i * n;
    float s = F[i * ldf] * P[j];
    for (int k = 1; k < n; ++k) s = fmaf(F[i * ldf + k], P[k * ld + j], s);
    X[i * ld + j] = s;
  }
  wave_lds_sync();
  if (c.kind == RTS_LIN_RECOMPUTE) {
    const float* q = c.GQG + (c.q_tv ? t * nn : 0);
    for (int e = tid; e < nn; e += 64) {  // P- = (F P) F^T + G Q_t G^T
      const int i = e / n, j = e - i * n;
      float s = X[i * ld] * F[j * ldf];
      for (int k = 1; k < n; ++k) s = fmaf(X[i * ld + k], F[j * ldf + k], s);
      Pp[i * ld + j] = s + q[e];
    }
    for (int i = tid; i < n; i += 64) {
      float s = F[i * ldf] * m[0];
      for (int k = 1; k < n; ++k) s = fmaf(F[i * ldf + k], m[k], s);
      mp[i] = s + c.Gq0[i];
    }
    wave_lds_sync();
  }
}

// Cholesky of P- into W (lower triangle, the diagonal holds the RECIPROCAL pivot), left-looking, one column per barrier;
// every lane forms the pivot itself.  NaN for a P- that is not positive definite.
__device__ __forceinline__ void rts_gen_chol(int n, const float* Pp, float* W, int tid) {
  const int ld = rts_gen_ld(n);
  for (int j = 0; j < n; ++j) {
    float d = Pp[j * ld + j];
    for (int k = 0; k < j; ++k) d = fmaf(-W[j * ld + k], W[j * ld + k], d);
    d = fast_sqrt(d);
    const float inv = fast_rcp(d);
    for (int i = j + 1 + tid; i < n; i += 64) {
      float s = Pp[i * ld + j];
      for (int k = 0; k < j; ++k) s = fmaf(-W[i * ld + k], W[j * ld + k], s);
      W[i * ld + j] = s * inv;
    }
    if (tid == 0) W[j * ld + j] = inv;
    wave_lds_sync();
  }
}

// X <- L^-1 X and X <- L^-T X with L from rts_gen_chol, a column per lane; no barrier inside (a lane's columns are its own)
__device__ __forceinline__ void rts_gen_solve_lower(int n, const float* W, float* X, int tid) {
  const int ld = rts_gen_ld(n);
  for (int cc = tid; cc < n; cc += 64) {
    for (int i = 0; i < n; ++i) {
      float s = X[i * ld + cc];
      for (int k = 0; k < i; ++k) s = fmaf(-W[i * ld + k], X[k * ld + cc], s);
      X[i * ld + cc] = s * W[i * ld + i];
    }
  }
}
__device__ __forceinline__ void rts_gen_solve_upper(int n, const float* W, float* X, int tid) {
  const int ld = rts_gen_ld(n);
  for (int cc = tid; cc < n; cc += 64) {
    for (int i = n - 1; i >= 0; --i) {
      float s = X[i * ld + cc];
      for (int k = i + 1; k < n; ++k) s = fmaf(-W[k * ld + i], X[k * ld + cc], s);
      X[i * ld + cc] = s * W[i * ld + i];
    }
  }
}

// The smoother's run-time-dimension kernel (rts_smoother.hip states its LDS carve-up): one 64-lane workgroup per trajectory.
// GS (the Gaussian-sum smoother): one workgroup per chain ch = b K + k, streams at b sB + k sK, inputs at b, carries at ch.
template <bool UNSC, bool USER, bool GS = false>
__device__ __forceinline__ void rts_generic_body(const RtsGen& c, const GenModel& g, const RtsViews& v, long long T, int K = 1) {
  const int tid = threadIdx.x;
  const long long ch = blockIdx.x;
  long long b = ch;
  int kc = 0;
  if constexpr (GS) {
    b = ch / K;
    kc = (int)(ch - b * K);
  }
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
  auto at = [&](const SView& s, long long t, int e) {
    if constexpr (GS) return b * s.sB + kc * s.sK + t * s.sT + e * s.sE;
    else return b * s.sB + t * s.sT + e * s.sE;
  };

  long long t = T - 1;
  if (v.m_in) {
    for (int e = tid; e < n; e += 64) ms[e] = v.m_in[ch * n + e];
    for (int e = tid; e < nn; e += 64) Ps[(e / n) * ld + e % n] = v.P_in[ch * nn + e];
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
    const float u0 = ((UNSC || USER || c.kind == RTS_EXT) && v.u) ? v.u[b * v.u_sB + t * v.u_sT] : 0.f;
    rts_gen_linearize<UNSC, USER>(c, g, u0, t, m, P, mp, Pp, X, W, tv, tid, ul);
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
  if (v.m_out) for (int e = tid; e < n; e += 64) v.m_out[ch * n + e] = ms[e];
  if (v.P_out) for (int e = tid; e < nn; e += 64) v.P_out[ch * nn + e] = Ps[(e / n) * ld + e % n];
}


// The sampler's run-time-dimension kernel (ffbs_sampler.hip states its LDS carve-up): one 64-lane workgroup per trajectory.
// GS (the Gaussian-sum sampler): one workgroup per (trajectory, component) that serves the samples whose component is its
// own -- their indices, in order, in `sel` behind the sample buffers -- and exits at once when there is none; the workgroup
// of component 0 also writes the drawn components and the NaN of the invalid draws.
template <bool UNSC, bool USER, bool GS = false>
__device__ __forceinline__ void ffbs_generic_body(const FfbsGen& fc, const GenModel& g, const FfbsViews& v, long long T,
                                                  const GsDraw* gd = nullptr) {
  const RtsGen& c = fc.r;
  const int tid = threadIdx.x;
  long long b = blockIdx.x;
  int kc = 0;
  if constexpr (GS) {
    b = blockIdx.x / gd->K;
    kc = (int)(blockIdx.x - b * gd->K);
  }
  const int n = c.n, ld = rts_gen_ld(n), nn = n * n, S = fc.S, SB = fc.SB;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* P = lds;
  float* Pp = P + n * ld;
  float* X = Pp + n * ld;
  float* W = X + n * ld;
  float* Sg = W + n * ld;
  float* m = Sg + n * ld;
  float* mp = m + n;
  float* tv = mp + n;
  const RtsUnscLds ul = rts_unsc_carve(Sg, tv + n, tv + n + n * ld, n);  // carved for RTS_UNSC only
  float* xs = tv + n + (UNSC ? n * ld + rts_unsc_vec_floats(n) : 0);  // x_{t+1} of the block, then x_{t+1} - m-
  float* xi = xs + SB * n;   // the block's noise
  float* xo = xi + SB * n;   // x_t of the block
  int NS = S;   // samples this workgroup serves
  int* sel = reinterpret_cast<int*>(xo + SB * n);
  if constexpr (GS) {
    int cnt = 0;
    for (int s0 = 0; s0 < S; s0 += 64) {  // uniform trip count: every lane reaches the ballot
      const int s = s0 + tid;
      const int z = s < S ? gs_draw_component(*gd, b, s, S) : -2;
      if (kc == 0 && s < S) {
        if (gd->z_out) gd->z_out[b * S + s] = z;
        if (z < 0) {
          const float nan = __builtin_nanf("");
          for (long long t = 0; t < T; ++t) for (int i = 0; i < n; ++i) v.x.p[b * v.x.sB + s * v.x.sK + t * v.x.sT + i * v.x.sE] = nan;
          if (v.x_out) for (int i = 0; i < n; ++i) v.x_out[((long long)b * S + s) * n + i] = nan;
        }
      }
      const unsigned long long mask = __ballot(z == kc);
      if (z == kc) sel[cnt + __popcll(mask & ((1ull << tid) - 1ull))] = s;
      cnt += __popcll(mask);
    }
    NS = cnt;
    if (NS == 0) return;  // uniform
    wave_lds_sync();
  }
  const bool one_block = SB >= NS;
  const bool keyed = v.xi.p == nullptr;
  uint32_t k0 = 0, k1 = 0;
  if (keyed) {
    k0 = v.keys[2 * b];
    k1 = v.keys[2 * b + 1];
  }
  const uint32_t count = (uint32_t)S * (uint32_t)T * (uint32_t)n;
  auto at = [&](const SView& s, long long t, int e) {
    if constexpr (GS) return b * s.sB + kc * s.sK + t * s.sT + e * s.sE;
    else return b * s.sB + t * s.sT + e * s.sE;
  };
  auto smp_of = [&](int j) {
    if constexpr (GS) return sel[j];
    else return j;
  };
  auto xat = [&](const SView& s, int smp, long long t, int e) { return b * s.sB + smp * s.sK + t * s.sT + e * s.sE; };

  // the samples of step t in blocks: first = the chunk's last step without a carry (x = m + Sg xi)
  auto samples = [&](long long t, bool first) {
    for (int sb0 = 0; sb0 < NS; sb0 += SB) {
      const int ne = ((NS - sb0) < SB ? (NS - sb0) : SB) * n;
      for (int e = tid; e < ne; e += 64) {
        const int sl = e / n, i = e - sl * n, smp = smp_of(sb0 + sl);
        xi[e] = keyed ? bits_to_normal(threefry_bits(k0, k1, ((uint32_t)smp * (uint32_t)T + (uint32_t)t) * (uint32_t)n + i, count))
                      : v.xi.p[xat(v.xi, smp, t, i)];
        if (!first) {
          float xn;
          if (t == T - 1) xn = v.x_in[((long long)b * S + smp) * n + i];
          else if (one_block) xn = xs[e];
          else xn = v.x.p[xat(v.x, smp, t + 1, i)];
          xs[e] = xn - mp[i];
        }
      }
      wave_lds_sync();
      for (int e = tid; e < ne; e += 64) {
        const int sl = e / n, i = e - sl * n;
        const float* z = xi + sl * n;
        float s;
        if (first) {
          s = Sg[i * ld] * z[0];
          for (int k = 1; k <= i; ++k) s = fmaf(Sg[i * ld + k], z[k], s);
        } else {
          const float* dx = xs + sl * n;
          s = X[i] * dx[0];
          for (int k = 1; k < n; ++k) s = fmaf(X[k * ld + i], dx[k], s);
          for (int k = 0; k <= i; ++k) s = fmaf(Sg[i * ld + k], z[k], s);
        }
        const float xv = m[i] + s;
        xo[e] = xv;
        if constexpr (GS) {
          const int smp = sel[sb0 + sl];
          v.x.p[xat(v.x, smp, t, i)] = xv;
          if (t == 0 && v.x_out) v.x_out[((long long)b * S + smp) * n + i] = xv;
        } else {
          v.x.p[xat(v.x, sb0 + sl, t, i)] = xv;
          if (t == 0 && v.x_out) v.x_out[((long long)b * S + sb0 + sl) * n + i] = xv;
        }
      }
      wave_lds_sync();
      if (one_block) {
        float* sw = xs;
        xs = xo;
        xo = sw;
      }
    }
  };
  // Sg (lower triangle) <- psdchol(Sg; diag P); every lane forms the pivot itself
  auto psd_factor = [&]() {
    for (int j = 0; j < n; ++j) {
      float p = Sg[j * ld + j];
      for (int k = 0; k < j; ++k) p = fmaf(-Sg[j * ld + k], Sg[j * ld + k], p);
      const bool keep = p > BF_FFBS_TAU * P[j * ld + j];
      const float r = keep ? fast_sqrt(p) : 0.f;
      const float inv = keep ? fast_rcp(r) : 0.f;
      for (int i = j + 1 + tid; i < n; i += 64) {
        float s = Sg[i * ld + j];
        for (int k = 0; k < j; ++k) s = fmaf(-Sg[i * ld + k], Sg[j * ld + k], s);
        Sg[i * ld + j] = keep ? s * inv : 0.f;
      }
      wave_lds_sync();  // the pivot's reads of row j are done before its diagonal changes
      if (tid == 0) Sg[j * ld + j] = r;
      wave_lds_sync();
    }
  };

  long long t = T - 1;
  if (!v.x_in) {
    for (int e = tid; e < n; e += 64) m[e] = v.m.p[at(v.m, t, e)];
    for (int e = tid; e < nn; e += 64) {
      const float x = v.P.p[at(v.P, t, e)];
      P[(e / n) * ld + e % n] = x;
      Sg[(e / n) * ld + e % n] = x;
    }
    wave_lds_sync();
    psd_factor();
    samples(t, true);
    --t;
  }
  for (; t >= 0; --t) {
    for (int e = tid; e < n; e += 64) m[e] = v.m.p[at(v.m, t, e)];
    for (int e = tid; e < nn; e += 64) P[(e / n) * ld + e % n] = v.P.p[at(v.P, t, e)];
    if (c.kind != RTS_LIN_RECOMPUTE) {
      for (int e = tid; e < n; e += 64) mp[e] = v.pm.p[at(v.pm, t, e)];
      for (int e = tid; e < nn; e += 64) Pp[(e / n) * ld + e % n] = v.pP.p[at(v.pP, t, e)];
    }
    wave_lds_sync();
    const float u0 = ((UNSC || USER || c.kind == RTS_EXT) && v.u) ? v.u[b * v.u_sB + t * v.u_sT] : 0.f;
    rts_gen_linearize<UNSC, USER>(c, g, u0, t, m, P, mp, Pp, X, W, tv, tid, ul);
    rts_gen_chol(n, Pp, W, tid);
    rts_gen_solve_lower(n, W, X, tid);  // X <- L^-1 X
    wave_lds_sync();
    for (int e = tid; e < nn; e += 64) {  // Sg = P - X^T X, lower triangle
      const int i = e / n, j = e - i * n;
      if (j > i) continue;
      float s = P[i * ld + j];
      for (int k = 0; k < n; ++k) s = fmaf(-X[k * ld + i], X[k * ld + j], s);
      Sg[i * ld + j] = s;
    }
    wave_lds_sync();
    rts_gen_solve_upper(n, W, X, tid);  // X <- L^-T X
    wave_lds_sync();
    psd_factor();
    samples(t, false);
  }
}

#endif

}  // namespace bf
