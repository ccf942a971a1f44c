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
//
// Missing observations (MISSING = true, bf_kalman_filter_pscan_missing_f32): a NaN entry of y is a component that was not
// observed at that step, with the contract of bf_kalman_filter_missing_f32.  The element of a step with observed rows o uses
// S_o = H_o Qb H_o^T + Rb_oo, K_o = Qb H_o^T S_o^-1, W_o = A^T H_o^T S_o^-1 (o empty: (A, u, Qb, 0, 0)), so A_e, C_e, J_e, K, W
// are constants per observation PATTERN: the host forms all 2^m (kf_pscan_patterns.hpp), the fold stages the table into LDS
// and a lane takes its step's entry by the pattern's bit mask p = sum obs[a] << a, with v[a] = 0 for a missing a.  Entry 2^m - 1
// is the complete step's element.  Block 0 and emit run condition_on_masked; the non-finite check runs over the observed
// components only, and a wholly missing step leaves m and P as they are and has log-likelihood 0 -- on a poisoned trajectory
// too, whose streams stay NaN.  ps_combine, the scan and the workspace are unchanged.
#pragma once
#include <cstring>
#include <type_traits>
#include "kf_scan_group.hpp"
#include "pscan_common.hpp"
#include "pscan_host.hpp"
#include "kf_pscan_patterns.hpp"

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

// One step's element with A, C and J left where they are (the missing route's table in LDS): a combination reads them at
// their uses, which keeps 3 n^2 floats per lane out of the registers.
template <int N>
struct PsElementRef {
  const float *a, *c, *jj;
  float bv[N], ev[N];
  __device__ const float* A() const { return a; }
  __device__ const float* b() const { return bv; }
  __device__ const float* C() const { return c; }
  __device__ const float* eta() const { return ev; }
  __device__ const float* J() const { return jj; }
};

// o = i (+) j, i the earlier span.  o may alias i or j: everything is read before the first write.
template <int N, class SpanJ = PsSpan<N>>
__device__ __forceinline__ void ps_combine(const PsSpan<N>& i, const SpanJ& j, PsSpan<N>& o) {
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
// MISSING: a NaN entry of yv is a component that was not observed (condition_on_masked, kf_math.hpp); the check runs over the
// observed components only, and a step with none leaves m and P as they are -- NaN on a poisoned trajectory -- and returns 0.
template <int N, int M, bool MISSING = false>
__device__ __forceinline__ float ps_update(const KFConst<N, M>& c, const float* yv, float* m, float* P) {
  float v[M];
  float z = 0.f;   // 0, or NaN when an entry of v is NaN / Inf
  BF_UNROLL for (int a = 0; a < M; ++a) {
    float s = c.H[a * N] * m[0];
    BF_UNROLL for (int i = 1; i < N; ++i) s = fmaf(c.H[a * N + i], m[i], s);
    if constexpr (MISSING) {
      v[a] = s + c.Dr0[a];   // the predicted observation
      const float d = yv[a] - v[a];
      z += (yv[a] == yv[a]) ? d - d : 0.f;
    } else {
      v[a] = yv[a] - (s + c.Dr0[a]);
      z += v[a] - v[a];
    }
  }
  float ll;
  if constexpr (MISSING) ll = condition_on_masked<N, M>(c.H, c.DRD, yv, v, m, P);
  else ll = condition_on<N, M>(c.H, c.DRD, v, m, P);
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
// MISSING: `table` is the workgroup's LDS copy of PsPatternTable<N, M>; a middle-block step takes the element of its own
// observation pattern from it, and block 0 runs the masked step.
template <int N, int M, bool MISSING = false>
__device__ __forceinline__ void ps_fold_body(const PsConst<N, M>& c, const CView& y, const CarryView& carry,
                                             float* __restrict__ agg, long long B, long long NB, int L,
                                             [[maybe_unused]] const float* table = nullptr) {
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
      ps_update<N, M, MISSING>(c.kf, yv, m, P);
      if (t + 1 < L) ps_predict<N>(c.kf, m, P);
    }
    BF_UNROLL for (int e = 0; e < N * N; ++e) { s.A()[e] = 0.f; s.C()[e] = P[e]; s.J()[e] = 0.f; }
    BF_UNROLL for (int e = 0; e < N; ++e) { s.b()[e] = m[e]; s.eta()[e] = 0.f; }
  } else {
    std::conditional_t<MISSING, PsElementRef<N>, PsSpan<N>> e;
    if constexpr (!MISSING) BF_UNROLL for (int i = 0; i < N * N; ++i) { e.A()[i] = c.Ae[i]; e.C()[i] = c.Ce[i]; e.J()[i] = c.Je[i]; }
    const long long t0 = k * (long long)L;
    for (int q = 0; q < L; ++q) {
      float yv[M], v[M];
      ps_load_y<N, M>(y, b, t0 + q, yv);
      BF_UNROLL for (int a = 0; a < M; ++a) v[a] = yv[a] - c.hud[a];
      const float *Kp = c.K, *Wp = c.W;
      float *eb, *ee;
      if constexpr (MISSING) {
        unsigned p = 0;
        BF_UNROLL for (int a = 0; a < M; ++a) {
          const bool obs = (yv[a] == yv[a]);
          v[a] = obs ? v[a] : 0.f;   // a select: the NaN never enters an fma
          p |= (obs ? 1u : 0u) << a;
        }
        const float* el = table + p * PsPattern<N, M>::F;   // A_e | C_e | J_e | K | W of this lane's pattern
        e.a = el;
        e.c = el + N * N;
        e.jj = el + 2 * N * N;
        Kp = el + 3 * N * N;
        Wp = Kp + N * M;
        eb = e.bv;
        ee = e.ev;
      } else {
        eb = e.b();
        ee = e.eta();
      }
      BF_UNROLL for (int i = 0; i < N; ++i) {
        float sb = Kp[i * M] * v[0], se = Wp[i * M] * v[0];
        BF_UNROLL for (int a = 1; a < M; ++a) {
          sb = fmaf(Kp[i * M + a], v[a], sb);
          se = fmaf(Wp[i * M + a], v[a], se);
        }
        eb[i] = c.kf.Gq0[i] + sb;
        ee[i] = se;
      }
      if (q == 0) {
        if constexpr (MISSING) {
          BF_UNROLL for (int i = 0; i < N * N; ++i) { s.A()[i] = e.A()[i]; s.C()[i] = e.C()[i]; s.J()[i] = e.J()[i]; }
          BF_UNROLL for (int i = 0; i < N; ++i) { s.b()[i] = e.b()[i]; s.eta()[i] = e.eta()[i]; }
        } else {
          BF_UNROLL for (int i = 0; i < PsSpan<N>::F; ++i) s.v[i] = e.v[i];
        }
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
template <int N, int M, bool MISSING = false>
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
    if constexpr (MISSING) {
      // A wholly missing step checks nothing and reports log-likelihood 0, on a poisoned trajectory too, so the block's
      // first step need not learn of the poison as it does on the plain route.  The scan's covariances read no observation
      // and are finite beside a NaN mean: a start mean that is not finite starts the block with NaN covariance and weight.
      float z = 0.f;
      BF_UNROLL for (int i = 0; i < N; ++i) z += m[i] - m[i];
      const bool finite = (z == 0.f);
      BF_UNROLL for (int i = 0; i < N * N; ++i) P[i] = finite ? P[i] : __builtin_nanf("");
      w = finite ? w : __builtin_nanf("");
    }
  }
  const long long t0 = k * (long long)L;
  const long long t1 = (t0 + L < T) ? t0 + L : T;
  for (long long t = t0; t < t1; ++t) {
    float yv[M];
    ps_load_y<N, M>(y, b, t, yv);
    const float ll = ps_update<N, M, MISSING>(c, yv, m, P);
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

// The fold's constants: PsConst, and on the missing route the device copy of the pattern table behind it.
template <int N, int M>
struct PsConstMissing : PsConst<N, M> {
  const float* table;   // PsPatternTable<N, M> (device_constants)
};
template <int N, int M, bool MISSING>
using PsFoldConst = std::conditional_t<MISSING, PsConstMissing<N, M>, PsConst<N, M>>;

template <int N, int M, bool MISSING = false>
__global__ void __launch_bounds__(64) kf_pscan_fold_kernel(PsFoldConst<N, M, MISSING> c, CView y, CarryView carry, float* agg,
                                                           long long B, long long NB, int L) {
  if constexpr (MISSING) {
    // the table once per workgroup, before any lane leaves: lanes of a wave index it by their own pattern
    constexpr int F = (int)(sizeof(PsPatternTable<N, M>) / sizeof(float));
    __shared__ float table[F];
    for (int i = threadIdx.x; i < F; i += 64) table[i] = c.table[i];
    __syncthreads();
    ps_fold_body<N, M, true>(c, y, carry, agg, B, NB, L, table);
  } else {
    ps_fold_body<N, M>(c, y, carry, agg, B, NB, L);
  }
}
template <int N>   // one workgroup per trajectory
__global__ void __launch_bounds__(256) kf_pscan_scan_kernel(PsPredict<N> c, const float* agg, float* start, long long B,
                                                            long long NB) {
  __shared__ float lds[pscan_lds_floats<PsScan<N>>()];
  pscan_scan<PsScan<N>>({c, agg, start, blockIdx.x * NB, B * NB}, NB, lds);
}
template <int N, int M, bool MISSING = false>
__global__ void __launch_bounds__(64) kf_pscan_emit_kernel(KFConst<N, M> c, CView y, CarryView carry, OutViews out,
                                                           const float* start, long long B, long long T, long long NB, int L) {
  ps_emit_body<N, M, MISSING>(c, y, carry, out, start, B, T, NB, L);
}

// ---- host: the call's constants and the three launches ------------------------------------------------------------------
// Element constants in float64 from the fp32 model terms the ordinary step uses.  false: S is singular.
template <int N, int M>
static inline bool ps_fill_const(const bf_lgssm* p, PsConst<N, M>& c) {
  fill_const<N, M>(p, c.kf, p->Q, p->R);
  for (int a = 0; a < M; ++a) {
    double s = c.kf.Dr0[a];
    for (int i = 0; i < N; ++i) s += (double)c.kf.H[a * N + i] * (double)c.kf.Gq0[i];
    c.hud[a] = (float)s;
  }
  PsPattern<N, M> e;   // every component observed: the element of a complete step
  if (!ps_pattern_element<N, M>(c.kf.A, c.kf.H, c.kf.GQG, c.kf.DRD, (1u << M) - 1u, e)) return false;
  std::memcpy(c.Ae, e.Ae, sizeof(c.Ae));
  std::memcpy(c.Ce, e.Ce, sizeof(c.Ce));
  std::memcpy(c.Je, e.Je, sizeof(c.Je));
  std::memcpy(c.K, e.K, sizeof(c.K));
  std::memcpy(c.W, e.W, sizeof(c.W));
  return true;
}

// MISSING (bf_kalman_filter_pscan_missing_f32): the fold's middle blocks need one element per observation pattern; the host
// forms all 2^M (kf_pscan_patterns.hpp), refuses a singular S_o like a singular S, and hands the table over as a cached
// device constant block in front of the fold launch.  A single-block call (NB = 1) is the emit launch alone and uploads none.
template <int N, int M, bool MISSING = false>
static inline int launch_pscan_nm(const bf_lgssm* p, const bf_cstream* y, long long B, long long T, const bf_carry* carry,
                                  const bf_out_desc* out, float* workspace, int L, hipStream_t stream) {
  static const char singular[] =
      "parallel kalman filter: S = H G Q G^T H^T + D R D^T is singular, the step element does not exist";
  PsFoldConst<N, M, MISSING> c;
  if (!ps_fill_const<N, M>(p, c)) return set_error(BF_EUNSUPPORTED, singular);
  [[maybe_unused]] PsPatternTable<N, M> table;
  if constexpr (MISSING)
    if (!ps_pattern_table<N, M>(c.kf.A, c.kf.H, c.kf.GQG, c.kf.DRD, table)) return set_error(BF_EUNSUPPORTED, singular);
  auto [yv, cv, ov] = forward_views(y, carry, out);
  const PscanGeom g = pscan_geom(B, 1, T, L);
  float* agg = workspace;
  float* start = workspace + g.lanes * PsSpan<N>::F;
  if (g.NB > 1) {
    PsPredict<N> pc;
    std::memcpy(pc.A, c.kf.A, sizeof(pc.A));
    std::memcpy(pc.GQG, c.kf.GQG, sizeof(pc.GQG));
    std::memcpy(pc.Gq0, c.kf.Gq0, sizeof(pc.Gq0));
    if constexpr (MISSING) {
      const void* d_table = nullptr;
      if (const int rc = device_constants(&table, sizeof(table), stream, &d_table)) return rc;
      c.table = static_cast<const float*>(d_table);
    }
    hipLaunchKernelGGL((kf_pscan_fold_kernel<N, M, MISSING>), dim3(g.grid), dim3(64), 0, stream, c, yv, cv, agg, B, g.NB, L);
    hipLaunchKernelGGL((kf_pscan_scan_kernel<N>), dim3((unsigned)B), dim3(g.scan_threads), 0, stream, pc, (const float*)agg, start,
                       B, g.NB);
  }
  hipLaunchKernelGGL((kf_pscan_emit_kernel<N, M, MISSING>), dim3(g.grid), dim3(64), 0, stream, c.kf, yv, cv, ov, (const float*)start, B, T,
                     g.NB, L);
  BF_HIP_CHECK(hipGetLastError());
  return BF_OK;
}

}  // namespace bf
