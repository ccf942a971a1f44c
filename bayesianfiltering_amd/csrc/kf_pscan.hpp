// kf_pscan: parallel-in-time Kalman filter for few long trajectories (include/bayesfilt.h, bf_kalman_filter_pscan_f32).
// Same model, streams, carry and log-likelihood as bf_kalman_filter_f32; time is cut into blocks of L steps and the blocks
// run on separate lanes (Sarkka & Garcia-Fernandez, "Temporal parallelization of Bayesian smoothers", IEEE TAC 2021).
//
// Math (the contract).  x_t = A x_{t-1} + G q, q ~ N(q0, Q);  y_t = H x_t + D r, r ~ N(r0, R);  Qb = G Q G^T, Rb = D R D^T,
// u = G q0, d = D r0; constant Q and R.  Order update -> predict: the carry (m_in, P_in) is the prediction for step 0.
//
// Element of one step t (the filtering element of a step whose predecessor state is unknown).  With S = H Qb H^T + Rb,
// K = Qb H^T S^-1, W = A^T H^T S^-1 and v = y_t - H u - d:
//   A_e = (I - K H) A     b_e = u + K v     C_e = (I - K H) Qb     eta_e = W v     J_e = W H A
// A_e, C_e, J_e, K and W are constants of the call: the host forms them once in float64 (Gauss-Jordan with partial pivoting on
// the m x m matrix S, no jitter; a singular S is refused) and rounds them to fp32.  Only b_e and eta_e read the data.
//
// Combination of an earlier span i with a later span j (associative):
//   A   = A_j (I + C_i J_j)^-1 A_i
//   b   = A_j (I + C_i J_j)^-1 (b_i + C_i eta_j) + b_j
//   C   = A_j (I + C_i J_j)^-1 C_i A_j^T + C_j
//   eta = A_i^T (I + J_j C_i)^-1 (eta_j - J_j b_i) + eta_i
//   J   = A_i^T (I + J_j C_i)^-1 J_j A_i + J_i
// C and J are symmetrised after every combination.  I + C J is similar to the symmetric I + C^1/2 J C^1/2: its eigenvalues are
// real and >= 1, so it is never near-singular, but it is not symmetric -- both solves are the pivoted LU of psd_solve
// (kf_math.hpp) with jitter = 0.
//
// Applying a span (A, b, C, eta, J) to a filtered state (m, P):
//   m' = A (I + P J)^-1 (m + P eta) + b        P' = A (I + P J)^-1 P A^T + C      (P' symmetrised)
// A filtered state is itself the span (0, m, P, 0, 0); combining it with a later span is exactly this rule.
//
// Three launches, fold, scan and emit; the scheme and the scan are pscan_common.hpp's, here as a PREFIX scan over NB = ceil(T / L):
//   fold   blocks 1 ... NB-2 build their L elements from y and fold them left to right into the block aggregate; block 0 is
//          filtered from the carry with the ordinary step and its filtered end state is stored as the span (0, m, P, 0, 0); the
//          last block needs no aggregate.  Workspace: agg[e][b NB + k].
//   scan   one workgroup per trajectory over the spans k = 0 ... NB-2.  Every prefix starts at step 0, so it is a plain
//          Gaussian: per block the scan writes only the prediction A m + u, A P A^T + Qb for the next block's first step,
//          start[e][b NB + k + 1], n + n^2 floats.
//   emit   the ordinary step from the block's start state -- condition_on<N, M> with the reference's 1e-6 jitter,
//          mvn_logpdf_chol, predict_cov<N>, in the association of kf_scan_group.hpp at one lane per trajectory -- and stores the
//          requested streams through the strided views; the last block writes the carry-out.
//
// Consequences.  Inside a block the outputs are, for finite data, the ordinary filter's from that block's start state; the only new arithmetic
// is in the block-start states, which are jitter-free: the product agrees with bf_kalman_filter_f32 to a tolerance, not bit for
// bit.  The arithmetic of a trajectory depends on (T, L) and on nothing else (not on B, the layout or the enabled streams).
// A NaN or Inf observation at step t gives NaN in every stream (weights, means, covariances, predictions, log-likelihood) and in
// the carry from t on, in that trajectory only; the steps before t inside its block stay finite because emit is sequential.
// For the weights, means and log-likelihoods this is the arithmetic of bf_kalman_filter_f32.  The covariance recursion reads no
// observation (there, and in the combination's C and J), so bf_kalman_filter_f32 keeps finite covariances beside NaN means;
// here the update sets mean, covariance and log-likelihood to NaN whenever the innovation is not finite (ps_update): a step without a posterior
// mean has no posterior.  The block-start means are NaN from the NaN's block on, so every later innovation is NaN too.
//
// Registers: every per-lane array is indexed by compile-time constants only (fully unrolled loops).  A combination holds two
// spans of 3 n^2 + 2 n floats plus the solve's right-hand sides: no scratch up to n = 6 (table in DESIGN.md, section 6h).
#pragma once
#include <cstring>
#include "kf_scan_group.hpp"
#include "pscan_common.hpp"
#include "pscan_host.hpp"

namespace bf {

template <int N, int M>
struct PsConst {
  KFConst<N, M> kf;   // the ordinary step's constants (block 0, emit)
  float Ae[N * N], Ce[N * N], Je[N * N];
  float K[N * M];     // b_e = u + K v
  float W[N * M];     // eta_e = W v
  float hud[M];       // H u + d
};
// what the scan's prediction reads of KFConst
template <int N>
struct PsPredict {
  float A[N * N], GQG[N * N], Gq0[N];
};

// A | b | C | eta | J, the workspace's entry order
template <int N>
struct PsSpan {
  static constexpr int F = 3 * N * N + 2 * N;
  float v[F];
  __device__ float* A() { return v; }                         __device__ const float* A() const { return v; }
  __device__ float* b() { return v + N * N; }                 __device__ const float* b() const { return v + N * N; }
  __device__ float* C() { return v + N * N + N; }             __device__ const float* C() const { return v + N * N + N; }
  __device__ float* eta() { return v + 2 * N * N + N; }       __device__ const float* eta() const { return v + 2 * N * N + N; }
  __device__ float* J() { return v + 2 * N * N + 2 * N; }     __device__ const float* J() const { return v + 2 * N * N + 2 * N; }
};
// a block-start state: m | P
constexpr int ps_state_floats(int n) { return n + n * n; }

// o = i (+) j, i the earlier span.  o may alias i or j: everything is read before the first write.
template <int N>
__device__ __forceinline__ void ps_combine(const PsSpan<N>& i, const PsSpan<N>& j, PsSpan<N>& o) {
  constexpr int C1 = 2 * N + 1, C2 = N + 1;
  // (I + C_i J_j) X = [A_i | C_i | b_i + C_i eta_j]
  float M1[N * N], X[N * C1], t[N];
  mm<N, N, N>(i.C(), j.J(), M1);
  BF_UNROLL for (int r = 0; r < N; ++r) M1[r * N + r] += 1.0f;
  mv<N, N>(i.C(), j.eta(), t);
  BF_UNROLL for (int r = 0; r < N; ++r) {
    BF_UNROLL for (int c = 0; c < N; ++c) {
      X[r * C1 + c] = i.A()[r * N + c];
      X[r * C1 + N + c] = i.C()[r * N + c];
    }
    X[r * C1 + 2 * N] = i.b()[r] + t[r];
  }
  psd_solve<N, C1>(M1, X, 0.0f);
  // (I + J_j C_i) Y = [J_j A_i | eta_j - J_j b_i]
  float M2[N * N], Y[N * C2], JA[N * N];
  mm<N, N, N>(j.J(), i.C(), M2);
  BF_UNROLL for (int r = 0; r < N; ++r) M2[r * N + r] += 1.0f;
  mm<N, N, N>(j.J(), i.A(), JA);
  mv<N, N>(j.J(), i.b(), t);
  BF_UNROLL for (int r = 0; r < N; ++r) {
    BF_UNROLL for (int c = 0; c < N; ++c) Y[r * C2 + c] = JA[r * N + c];
    Y[r * C2 + N] = j.eta()[r] - t[r];
  }
  psd_solve<N, C2>(M2, Y, 0.0f);

  float oA[N * N], ob[N], oC[N * N], oe[N], oJ[N * N], T1[N * N];
  BF_UNROLL for (int r = 0; r < N; ++r) {
    BF_UNROLL for (int c = 0; c < N; ++c) {
      float sa = j.A()[r * N] * X[c], sc = j.A()[r * N] * X[N + c];
      BF_UNROLL for (int k = 1; k < N; ++k) {
        sa = fmaf(j.A()[r * N + k], X[k * C1 + c], sa);
        sc = fmaf(j.A()[r * N + k], X[k * C1 + N + c], sc);
      }
      oA[r * N + c] = sa;
      T1[r * N + c] = sc;   // A_j (I + C_i J_j)^-1 C_i
    }
    float sb = j.A()[r * N] * X[2 * N];
    BF_UNROLL for (int k = 1; k < N; ++k) sb = fmaf(j.A()[r * N + k], X[k * C1 + 2 * N], sb);
    ob[r] = sb + j.b()[r];
  }
  mm_nt<N, N, N>(T1, j.A(), oC);
  BF_UNROLL for (int e = 0; e < N * N; ++e) oC[e] += j.C()[e];
  BF_UNROLL for (int r = 0; r < N; ++r) {   // A_i^T Y
    BF_UNROLL for (int c = 0; c < N; ++c) {
      float s = i.A()[r] * Y[c];
      BF_UNROLL for (int k = 1; k < N; ++k) s = fmaf(i.A()[k * N + r], Y[k * C2 + c], s);
      oJ[r * N + c] = s + i.J()[r * N + c];
    }
    float s = i.A()[r] * Y[N];
    BF_UNROLL for (int k = 1; k < N; ++k) s = fmaf(i.A()[k * N + r], Y[k * C2 + N], s);
    oe[r] = s + i.eta()[r];
  }
  symmetrise<N>(oC);
  symmetrise<N>(oJ);
  BF_UNROLL for (int e = 0; e < N * N; ++e) { o.A()[e] = oA[e]; o.C()[e] = oC[e]; o.J()[e] = oJ[e]; }
  BF_UNROLL for (int e = 0; e < N; ++e) { o.b()[e] = ob[e]; o.eta()[e] = oe[e]; }
}

// x = (m | P) <- the span s applied to the filtered state x
template <int N>
__device__ __forceinline__ void ps_apply(const PsSpan<N>& s, float* x) {
  constexpr int C2 = N + 1;
  float *m = x, *P = x + N;
  float M1[N * N], X[N * C2], t[N];
  mm<N, N, N>(P, s.J(), M1);
  BF_UNROLL for (int r = 0; r < N; ++r) M1[r * N + r] += 1.0f;
  mv<N, N>(P, s.eta(), t);
  BF_UNROLL for (int r = 0; r < N; ++r) {
    BF_UNROLL for (int c = 0; c < N; ++c) X[r * C2 + c] = P[r * N + c];
    X[r * C2 + N] = m[r] + t[r];
  }
  psd_solve<N, C2>(M1, X, 0.0f);
  float T1[N * N];
  BF_UNROLL for (int r = 0; r < N; ++r) {
    BF_UNROLL for (int c = 0; c < N; ++c) {
      float sc = s.A()[r * N] * X[c];
      BF_UNROLL for (int k = 1; k < N; ++k) sc = fmaf(s.A()[r * N + k], X[k * C2 + c], sc);
      T1[r * N + c] = sc;
    }
    float sb = s.A()[r * N] * X[N];
    BF_UNROLL for (int k = 1; k < N; ++k) sb = fmaf(s.A()[r * N + k], X[k * C2 + N], sb);
    m[r] = sb + s.b()[r];
  }
  mm_nt<N, N, N>(T1, s.A(), P);
  BF_UNROLL for (int e = 0; e < N * N; ++e) P[e] += s.C()[e];
  symmetrise<N>(P);
}

// ---- the ordinary step, one lane per trajectory (kf_scan_group.hpp at NL = 1) -------------------------------------------
template <int N, int M>
__device__ __forceinline__ void ps_load_y(const CView& y, long long b, long long t, float* yv) {
  BF_UNROLL for (int a = 0; a < M; ++a) yv[a] = y.p[b * y.sB + t * y.sT + a * y.sE];
}
// update: (m, P) prediction -> filtered; returns the log-likelihood.  An innovation that is not finite (a NaN / Inf
// observation, or a mean that an earlier one made NaN) leaves no posterior: mean, covariance and log-likelihood are set to NaN
// by selects, so that finite data keep the ordinary step's bits.
template <int N, int M>
__device__ __forceinline__ float ps_update(const KFConst<N, M>& c, const float* yv, float* m, float* P) {
  float v[M];
  float z = 0.f;   // 0, or NaN when an entry of v is NaN / Inf
  BF_UNROLL for (int a = 0; a < M; ++a) {
    float s = c.H[a * N] * m[0];
    BF_UNROLL for (int i = 1; i < N; ++i) s = fmaf(c.H[a * N + i], m[i], s);
    v[a] = yv[a] - (s + c.Dr0[a]);
    z += v[a] - v[a];
  }
  const float ll = condition_on<N, M>(c.H, c.DRD, v, m, P);
  const bool finite = (z == 0.f);
  BF_UNROLL for (int i = 0; i < N * N; ++i) P[i] = finite ? P[i] : __builtin_nanf("");
  BF_UNROLL for (int i = 0; i < N; ++i) m[i] = finite ? m[i] : __builtin_nanf("");   // (an Inf observation alone gives +-Inf here)
  return finite ? ll : __builtin_nanf("");
}
// predict: (m, P) filtered -> prediction for the next step; Const: KFConst<N, M> or PsPredict<N>
template <int N, class Const>
__device__ __forceinline__ void ps_predict(const Const& c, float* m, float* P) {
  predict_cov<N>(c.A, c.GQG, P);
  float mp[N];
  mv<N, N>(c.A, m, mp);
  BF_UNROLL for (int i = 0; i < N; ++i) m[i] = mp[i] + c.Gq0[i];
}

// ---- launch 1: fold -----------------------------------------------------------------------------------------------------
template <int N, int M>
__device__ __forceinline__ void ps_fold_body(const PsConst<N, M>& c, const CView& y, const CarryView& carry,
                                             float* __restrict__ agg, long long B, long long NB, int L) {
  long long g, b, k;
  int j;
  if (!pscan_lane(B, 1, NB, g, b, j, k)) return;
  if (k == NB - 1) return;   // the last block is only emitted
  PsSpan<N> s;
  if (k == 0) {
    // block 0: the ordinary filter from the carry; its filtered end state is the span (0, m, P, 0, 0)
    float m[N], P[N * N], yv[M];
    BF_UNROLL for (int i = 0; i < N; ++i) m[i] = carry.m_in[b * N + i];
    BF_UNROLL for (int i = 0; i < N * N; ++i) P[i] = carry.P_in[b * N * N + i];
    for (int t = 0; t < L; ++t) {
      ps_load_y<N, M>(y, b, t, yv);
      ps_update<N, M>(c.kf, yv, m, P);
      if (t + 1 < L) ps_predict<N>(c.kf, m, P);
    }
    BF_UNROLL for (int e = 0; e < N * N; ++e) { s.A()[e] = 0.f; s.C()[e] = P[e]; s.J()[e] = 0.f; }
    BF_UNROLL for (int e = 0; e < N; ++e) { s.b()[e] = m[e]; s.eta()[e] = 0.f; }
  } else {
    PsSpan<N> e;
    BF_UNROLL for (int i = 0; i < N * N; ++i) { e.A()[i] = c.Ae[i]; e.C()[i] = c.Ce[i]; e.J()[i] = c.Je[i]; }
    const long long t0 = k * (long long)L;
    for (int q = 0; q < L; ++q) {
      float yv[M], v[M];
      ps_load_y<N, M>(y, b, t0 + q, yv);
      BF_UNROLL for (int a = 0; a < M; ++a) v[a] = yv[a] - c.hud[a];
      BF_UNROLL for (int i = 0; i < N; ++i) {
        float sb = c.K[i * M] * v[0], se = c.W[i * M] * v[0];
        BF_UNROLL for (int a = 1; a < M; ++a) {
          sb = fmaf(c.K[i * M + a], v[a], sb);
          se = fmaf(c.W[i * M + a], v[a], se);
        }
        e.b()[i] = c.kf.Gq0[i] + sb;
        e.eta()[i] = se;
      }
      if (q == 0) {
        BF_UNROLL for (int i = 0; i < PsSpan<N>::F; ++i) s.v[i] = e.v[i];
      } else {
        ps_combine<N>(s, e, s);
      }
    }
  }
  pscan_col_store<PsSpan<N>::F>(agg, B * NB, g, s.v);
}

// ---- launch 2: scan (pscan_common.hpp) -----------------------------------------------------------------------------------
// Span 0 has A = 0, eta = 0, J = 0 and maps any finite state to (b, C) exactly.  finish: the state is the filtered (m, P) at
// the last step of block k; its prediction starts block k + 1.
template <int N>
struct PsScan {
  using Span = PsSpan<N>;
  static constexpr int STATE = ps_state_floats(N);
  static constexpr int DIM = N;
  static constexpr bool SUFFIX = false;
  struct Args {
    PsPredict<N> c;
    const float* __restrict__ agg;
    float* __restrict__ start;
    long long col0, stride;   // b NB and B NB
  };
  static __device__ __forceinline__ void load(const Args& a, long long k, Span& s) {
    pscan_col_load<Span::F>(a.agg, a.stride, a.col0 + k, s.v);
  }
  static __device__ __forceinline__ void combine(const Span& i, const Span& j, Span& o) { ps_combine<N>(i, j, o); }
  static __device__ __forceinline__ void apply(const Span& s, float* x) { ps_apply<N>(s, x); }
  static __device__ __forceinline__ void finish(const Args& a, long long k, float* x) {
    ps_predict<N>(a.c, x, x + N);
    pscan_col_store<STATE>(a.start, a.stride, a.col0 + k + 1, x);
  }
};

// ---- launch 3: emit -----------------------------------------------------------------------------------------------------
template <int N, int M>
__device__ __forceinline__ void ps_emit_body(const KFConst<N, M>& c, const CView& y, const CarryView& carry, const OutViews& out,
                                             const float* __restrict__ start, long long B, long long T, long long NB, int L) {
  long long g, b, k;
  int j;
  if (!pscan_lane(B, 1, NB, g, b, j, k)) return;
  float x[ps_state_floats(N)], *m = x, *P = x + N;
  float w = carry.w_in ? carry.w_in[b] : 1.0f;
  if (k == 0) {
    BF_UNROLL for (int i = 0; i < N; ++i) m[i] = carry.m_in[b * N + i];
    BF_UNROLL for (int i = 0; i < N * N; ++i) P[i] = carry.P_in[b * N * N + i];
  } else {
    pscan_col_load<ps_state_floats(N)>(start, B * NB, g, x);
    w = reweight_single(0.f, w);   // the weight after any earlier step: 1, or NaN for a carry weight that is not a positive number
  }
  const long long t0 = k * (long long)L;
  const long long t1 = (t0 + L < T) ? t0 + L : T;
  for (long long t = t0; t < t1; ++t) {
    float yv[M];
    ps_load_y<N, M>(y, b, t, yv);
    const float ll = ps_update<N, M>(c, yv, m, P);
    w = reweight_single(ll, w);
    if (out.w.p) out.w.p[b * out.w.sB + t * out.w.sT] = w;
    if (out.ll.p) out.ll.p[b * out.ll.sB + t * out.ll.sT] = ll;
    if (out.m.p) BF_UNROLL for (int i = 0; i < N; ++i) out.m.p[b * out.m.sB + t * out.m.sT + i * out.m.sE] = m[i];
    if (out.P.p) BF_UNROLL for (int i = 0; i < N * N; ++i) out.P.p[b * out.P.sB + t * out.P.sT + i * out.P.sE] = P[i];
    ps_predict<N>(c, m, P);
    if (out.pm.p) BF_UNROLL for (int i = 0; i < N; ++i) out.pm.p[b * out.pm.sB + t * out.pm.sT + i * out.pm.sE] = m[i];
    if (out.pP.p) BF_UNROLL for (int i = 0; i < N * N; ++i) out.pP.p[b * out.pP.sB + t * out.pP.sT + i * out.pP.sE] = P[i];
  }
  if (k == NB - 1) {
    if (carry.m_out) BF_UNROLL for (int i = 0; i < N; ++i) carry.m_out[b * N + i] = m[i];
    if (carry.P_out) BF_UNROLL for (int i = 0; i < N * N; ++i) carry.P_out[b * N * N + i] = P[i];
    if (carry.w_out) carry.w_out[b] = w;
  }
}

template <int N, int M>
__global__ void __launch_bounds__(64) kf_pscan_fold_kernel(PsConst<N, M> c, CView y, CarryView carry, float* agg, long long B,
                                                           long long NB, int L) {
  ps_fold_body<N, M>(c, y, carry, agg, B, NB, L);
}
template <int N>   // one workgroup per trajectory
__global__ void __launch_bounds__(256) kf_pscan_scan_kernel(PsPredict<N> c, const float* agg, float* start, long long B,
                                                            long long NB) {
  __shared__ float lds[pscan_lds_floats<PsScan<N>>()];
  pscan_scan<PsScan<N>>({c, agg, start, blockIdx.x * NB, B * NB}, NB, lds);
}
template <int N, int M>
__global__ void __launch_bounds__(64) kf_pscan_emit_kernel(KFConst<N, M> c, CView y, CarryView carry, OutViews out,
                                                           const float* start, long long B, long long T, long long NB, int L) {
  ps_emit_body<N, M>(c, y, carry, out, start, B, T, NB, L);
}

// ---- host: the call's constants and the three launches ------------------------------------------------------------------
// Element constants in float64 from the fp32 model terms the ordinary step uses.  false: S is singular.
template <int N, int M>
static inline bool ps_fill_const(const bf_lgssm* p, PsConst<N, M>& c) {
  fill_const<N, M>(p, c.kf, p->Q, p->R);
  double A[N * N], H[M * N], Qb[N * N], u[N], S[M * M], Si[M * M], HQ[M * N], hud[M];
  for (int i = 0; i < N * N; ++i) { A[i] = c.kf.A[i]; Qb[i] = c.kf.GQG[i]; }
  for (int i = 0; i < M * N; ++i) H[i] = c.kf.H[i];
  for (int i = 0; i < N; ++i) u[i] = c.kf.Gq0[i];
  for (int a = 0; a < M; ++a) {
    double s = c.kf.Dr0[a];
    for (int i = 0; i < N; ++i) s += H[a * N + i] * u[i];
    hud[a] = s;
    for (int j = 0; j < N; ++j) {
      double q = 0;
      for (int i = 0; i < N; ++i) q += H[a * N + i] * Qb[i * N + j];
      HQ[a * N + j] = q;
    }
  }
  for (int a = 0; a < M; ++a)
    for (int e = 0; e < M; ++e) {
      double s = c.kf.DRD[a * M + e];
      for (int j = 0; j < N; ++j) s += HQ[a * N + j] * H[e * N + j];
      S[a * M + e] = s;
      Si[a * M + e] = (a == e) ? 1.0 : 0.0;
    }
  for (int k = 0; k < M; ++k) {   // Gauss-Jordan with partial pivoting: Si <- S^-1
    int piv = k;
    for (int r = k + 1; r < M; ++r) if (std::fabs(S[r * M + k]) > std::fabs(S[piv * M + k])) piv = r;
    const double d = S[piv * M + k];
    if (!(std::fabs(d) > 1e-300) || !std::isfinite(d)) return false;
    for (int e = 0; e < M; ++e) { std::swap(S[k * M + e], S[piv * M + e]); std::swap(Si[k * M + e], Si[piv * M + e]); }
    for (int e = 0; e < M; ++e) { S[k * M + e] /= d; Si[k * M + e] /= d; }
    for (int r = 0; r < M; ++r) if (r != k) {
      const double f = S[r * M + k];
      for (int e = 0; e < M; ++e) { S[r * M + e] -= f * S[k * M + e]; Si[r * M + e] -= f * Si[k * M + e]; }
    }
  }
  double K[N * M], HA[M * N], W[N * M], IKH[N * N], Ae[N * N], Ce[N * N], Je[N * N];
  for (int i = 0; i < N; ++i)
    for (int a = 0; a < M; ++a) {
      double s = 0;
      for (int e = 0; e < M; ++e) s += HQ[e * N + i] * Si[e * M + a];   // Qb H^T S^-1 (Qb symmetric)
      K[i * M + a] = s;
    }
  for (int a = 0; a < M; ++a)
    for (int j = 0; j < N; ++j) {
      double s = 0;
      for (int i = 0; i < N; ++i) s += H[a * N + i] * A[i * N + j];
      HA[a * N + j] = s;
    }
  for (int i = 0; i < N; ++i)
    for (int a = 0; a < M; ++a) {
      double s = 0;
      for (int e = 0; e < M; ++e) s += HA[e * N + i] * Si[e * M + a];   // A^T H^T S^-1
      W[i * M + a] = s;
    }
  for (int i = 0; i < N; ++i)
    for (int j = 0; j < N; ++j) {
      double s = (i == j) ? 1.0 : 0.0, q = 0;
      for (int a = 0; a < M; ++a) { s -= K[i * M + a] * H[a * N + j]; q += W[i * M + a] * HA[a * N + j]; }
      IKH[i * N + j] = s;
      Je[i * N + j] = q;
    }
  for (int i = 0; i < N; ++i)
    for (int j = 0; j < N; ++j) {
      double s = 0, q = 0;
      for (int k = 0; k < N; ++k) { s += IKH[i * N + k] * A[k * N + j]; q += IKH[i * N + k] * Qb[k * N + j]; }
      Ae[i * N + j] = s;
      Ce[i * N + j] = q;
    }
  for (int i = 0; i < N; ++i)
    for (int j = 0; j < N; ++j) {
      c.Ae[i * N + j] = (float)Ae[i * N + j];
      c.Ce[i * N + j] = (float)(0.5 * (Ce[i * N + j] + Ce[j * N + i]));
      c.Je[i * N + j] = (float)(0.5 * (Je[i * N + j] + Je[j * N + i]));
    }
  for (int i = 0; i < N * M; ++i) { c.K[i] = (float)K[i]; c.W[i] = (float)W[i]; }
  for (int a = 0; a < M; ++a) c.hud[a] = (float)hud[a];
  bool finite = true;
  for (int i = 0; i < N * N; ++i) finite = finite && std::isfinite(c.Ae[i]) && std::isfinite(c.Ce[i]) && std::isfinite(c.Je[i]);
  return finite;
}

template <int N, int M>
static inline int launch_pscan_nm(const bf_lgssm* p, const bf_cstream* y, long long B, long long T, const bf_carry* carry,
                                  const bf_out_desc* out, float* workspace, int L, hipStream_t stream) {
  PsConst<N, M> c;
  if (!ps_fill_const<N, M>(p, c))
    return set_error(BF_EUNSUPPORTED, "parallel kalman filter: S = H G Q G^T H^T + D R D^T is singular, the step element does not exist");
  auto [yv, cv, ov] = forward_views(y, carry, out);
  const PscanGeom g = pscan_geom(B, 1, T, L);
  float* agg = workspace;
  float* start = workspace + g.lanes * PsSpan<N>::F;
  if (g.NB > 1) {
    PsPredict<N> pc;
    std::memcpy(pc.A, c.kf.A, sizeof(pc.A));
    std::memcpy(pc.GQG, c.kf.GQG, sizeof(pc.GQG));
    std::memcpy(pc.Gq0, c.kf.Gq0, sizeof(pc.Gq0));
    hipLaunchKernelGGL((kf_pscan_fold_kernel<N, M>), dim3(g.grid), dim3(64), 0, stream, c, yv, cv, agg, B, g.NB, L);
    hipLaunchKernelGGL((kf_pscan_scan_kernel<N>), dim3((unsigned)B), dim3(g.scan_threads), 0, stream, pc, (const float*)agg, start,
                       B, g.NB);
  }
  hipLaunchKernelGGL((kf_pscan_emit_kernel<N, M>), dim3(g.grid), dim3(64), 0, stream, c.kf, yv, cv, ov, (const float*)start, B, T,
                     g.NB, L);
  BF_HIP_CHECK(hipGetLastError());
  return BF_OK;
}

}  // namespace bf
