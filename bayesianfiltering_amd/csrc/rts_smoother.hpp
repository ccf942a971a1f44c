// rts_smoother: batched Rauch-Tung-Striebel backward pass over the streams a filter emitted (include/bayesfilt.h,
// bf_rts_smoother_f32 / bf_eks_smoother_f32; the reference's SSM.smoother, gaussfiltax/ssm.py:55-61, 282-300).
//
// Math (the contract).  The filter's streams at step t (update -> predict order, inference.py:342-363) are the filtered
// m_t, P_t and the one-step prediction m-_{t+1}, P-_{t+1} (pred_means[t], pred_covs[t]).  With F_t the dynamics Jacobian
// the filter's predict used at step t:
//   t = T-1 (no carry):  m^s = m, P^s = P, bit for bit
//   t = T-2 ... 0:       X_t = (P-_{t+1})^-1 (F_t P_t)  (Cholesky of P-_{t+1}, lower triangle read, no jitter), G_t = X_t^T
//                        m^s_t = m_t + G_t (m^s_{t+1} - m-_{t+1})
//                        P^s_t = P_t + G_t (P^s_{t+1} - P-_{t+1}) G_t^T
//                        C_t  = G_t P^s_{t+1}                                   (optional lag-one cross-covariance)
// A P- that is not positive definite gives NaN (sqrt of a negative pivot) from that step backwards.
//
// Unscented route (RTS_UNSC; bf_uks_smoother_f32, bf_uffbs_sample_f32).  Inputs are the streams of bf_ugsf_ukf_f32 with
// K = 1 (update -> predict order): filtered m_t, P_t and the predictions m-_{t+1}, P-_{t+1} at index t, all required.  With
// L = n + dq, lambda = alpha^2 (L + kappa) - L, c = sqrt(L + lambda) and w = 1 / (2 (L + lambda)) (UkfModel's c_p, ws_p):
//   R_t = symmetric square root of P_t (eigenvalues clamped at 0): the root the filter's predict formed at step t --
//         sym_sqrt<N> (ugsf_scan.hpp) here, ug_sym_sqrt with its Newton step on the run-time-dimension kernel (lower triangle read)
//   s_j = c R_t[j, :],  j = 0 ... n-1
//   X_t = w sum_j ( f(m_t + s_j, q0, u_t) - f(m_t - s_j, q0, u_t) ) s_j^T            (X[k][i] = Cov(x_{t+1,k}, x_{t,i} | y_{1:t}))
// replaces F_t P_t; everything after it (the Cholesky of P-_{t+1}, G_t, m^s, P^s, C_t, the sampler's recursion) is unchanged.
// The sigma points that perturb only the noise have zero state deviation, so neither Q nor its root is read; the centre
// term and the predicted mean cancel by symmetry.  For f = A x + G q, X_t = A P_t exactly (2 w c^2 = 1).  X_t is a
// difference of images 2 c |R_t| apart: its fp32 relative error is about 2^-24 |f(m_t)| / (c |P_t|^1/2), the cancellation
// the filter's own moment sums have; alpha << 1 makes it large (1e-4 ... 2e-4 against float64 at alpha = 1e-3).
//
// Gaussian-sum smoother (bf_gs_smoother_f32; K >= 1 components).  In bf_gsf_ekf_f32 and bf_ugsf_ukf_f32 the components never
// interact: each is an extended (unscented) Kalman chain started from its own initial mean, coupled only through the weight
// recursion w_{t,k} ~ w_{t-1,k} p(y_t | y_{<t}, k).  The model is a mixture over the index k of the initial component,
//   p(x_{0:T-1} | y_{0:T-1}) = sum_k w_{T-1,k} p(x_{0:T-1} | y_{0:T-1}, k),
// so the smoothed weights are the filter's weights at the LAST step of the whole series (constant in t, given as weights[B][K] so
// that backward chunks share them) and smoothed component k is the recursion above (extended from the registry or from source,
// or unscented) on chain (b, k): streams at b sB + k sK, inputs u at b, the carry bf_smooth_carry contiguous [B][K][n] /
// [B][K][n][n] at b K + k.  Optional collapsed streams, the moment match of utils.collapse with time-constant weights:
//   mu_t = sum_k w_k m^s_{k,t},   Sigma_t = sum_k w_k (P^s_{k,t} + (m^s_{k,t} - mu_t)(m^s_{k,t} - mu_t)^T),
// the sum over k an adjacent-pair tree over the power of two >= K whose order depends on K alone (never on B or on where a
// trajectory sits in a wave); NaN weights or a NaN chain give NaN collapsed values for that trajectory only.  The kernels are at
// the end of this file (rts_gs_reg_body) and in rts_generic.hpp (rts_generic_body<.., GS>); the host side is gs_smoother.hip.
//
// Register kernel (this file, n <= 8): one lane per trajectory, 64-thread workgroups.  The carry (m^s, P^s) and the
// step's P, P-, X, Cholesky factor live in VGPRs; every loop has compile-time bounds.  Two data paths, same arithmetic
// (so the same bits):
//   RTS_STRIDED  any strides: each lane loads / stores its own elements (the batch-inner layout [T][E][B] is coalesced
//                across lanes as it is);
//   RTS_STAGED   contiguous reference layout [B][T][E], n <= 4: the wave walks time in chunks of TC steps.  A chunk of
//                the 64 trajectories' rows is fetched with 16-byte loads (consecutive lanes on consecutive 16-byte pieces
//                of one row: TC*E*4-byte runs) into per-stream LDS tiles padded by 4 floats per row, the lanes walk
//                their row backwards from LDS, write the smoothed values in place of the inputs they consumed (m^s over
//                m, P^s over P, C over P-) and the tile leaves through 16-byte non-temporal stores.  The next (earlier)
//                chunk's loads are issued into registers before the current chunk is computed (double buffering: the
//                registers are the second buffer) and land in LDS after the flush.
// Run-time-dimension kernel (rts_smoother.hip): one wave per trajectory, state in LDS, for every other n.
//
// Source route (RTS_EXT_USER; bf_eks_smoother_f32 / bf_effbs_sample_f32 with dynamics given as source): F_t is the Jacobian
// of the caller's dynamics(x, q, u, theta, out) with respect to the state at (m_t, q0, u_t) by forward-mode dual numbers,
// the Jacobian the filter's predict used at step t.  This file and ffbs_sampler.hpp are embedded in the library
// (jit_embed.py) and compiled by hiprtc around the caller's source (jit_source.hip: JIT_RTS_REGS / JIT_FFBS_REGS), so they
// stay self-contained under BF_JIT: device code only, after bf_views.hpp, kf_math.hpp, scan_common.hpp, bf_rng.hpp,
// models.hpp and ugsf_scan.hpp.
#pragma once
#ifndef BF_JIT
#include "bf_common.hpp"
#endif
#include "kf_math.hpp"
#include "models.hpp"
#include "scan_common.hpp"
#include "ugsf_scan.hpp"

namespace bf {

enum { RTS_STRIDED = 0, RTS_STAGED = 2 };
enum { RTS_LIN = 0, RTS_LIN_RECOMPUTE = 1, RTS_EXT = 2, RTS_UNSC = 3, RTS_EXT_USER = 4 };

// Linear dynamics: A, G Q G^T (constant part), G q0.
template <int N>
struct RtsLin {
  float A[N * N];
  float GQG[N * N];
  float Gq0[N];
};

// Unscented route: what f(x, q0, u) of the registry dynamics reads (dyn_base_t's fields), F_q q0 and the prediction's
// unscented constants c = sqrt(L + lambda), w = 1 / (2 (L + lambda)).
template <int N>
struct RtsUnsc {
  int dyn_id;
  float dth[8];
  float A[N * N];
  float Gq0[N];
  float c, w;
};

// Source route (RTS_EXT_USER): what the caller's dynamics(x, q, u, theta, out) reads besides the state and the input -- its
// parameters (at most 64, the register filter's limit) and the noise bias q0.  Nothing of the registry.
template <int DQ_>
struct RtsUser {
  static constexpr int DQ = DQ_;
  float theta[64];
  float q0[DQ_];
};

struct RtsViews {
  SView m, P, pm, pP;  // filtered inputs (read only)
  SView ms, Ps, Cs;    // outputs (Cs.p may be NULL)
  const float* m_in;   // smoothed state after the chunk ([B][n], [B][n][n]); NULL = the chunk ends at T-1
  const float* P_in;
  float* m_out;
  float* P_out;
  const float* u;      // inputs, element (b, t) at u[b*u_sB + t*u_sT]; NULL = zeros
  long long u_sB, u_sT;
};

// steps per staged chunk: 128-byte runs for the covariance rows where the prefetch registers allow (TC*E % 4 == 0 for
// E = n and n*n)
template <int N>
struct RtsStage {
  static constexpr int TC = N == 1 ? 8 : (N == 2 ? 4 : (N == 3 ? 4 : 2));
  static constexpr int WM = TC * N, WP = TC * N * N;
  static constexpr int PAD = 4;
  static constexpr int PM = WM + PAD, PP = WP + PAD;  // row pitches (floats); rows stay 16-byte aligned
  static constexpr int CHM = WM / 4, CHP = WP / 4;    // 16-byte pieces per row = loads per lane per tile
  static constexpr int FLOATS = 64 * (2 * PM + 2 * PP);
  static constexpr bool OK = N <= 4 && WM % 4 == 0 && WP % 4 == 0;
};

// One backward step.  In: X = F_t P_t, P_t, m_t, m-_{t+1}, P-_{t+1}; carry ms / Ps = smoothed state at t+1.
// Out: ms / Ps = smoothed state at t; C = G_t P^s_{t+1} when WANT_C.
template <int N>
__device__ __forceinline__ void rts_step(float* X, const float* P, const float* m, const float* mp, const float* Pp,
                                         float* ms, float* Ps, float* C, bool want_c) {
  // Cholesky of P- (lower triangle), reciprocal pivots
  float L[N * N];
  float rd[N];
  BF_UNROLL for (int j = 0; j < N; ++j) {
    float d = Pp[j * N + j];
    BF_UNROLL for (int k = 0; k < j; ++k) d = fmaf(-L[j * N + k], L[j * N + k], d);
    d = fast_sqrt(d);  // NaN for a non-PD P-
    const float inv = fast_rcp(d);
    rd[j] = inv;
    BF_UNROLL for (int i = j + 1; i < N; ++i) {
      float s = Pp[i * N + j];
      BF_UNROLL for (int k = 0; k < j; ++k) s = fmaf(-L[i * N + k], L[j * N + k], s);
      L[i * N + j] = s * inv;
    }
  }
  // X <- L^-T L^-1 X, column by column
  BF_UNROLL for (int c = 0; c < N; ++c) {
    BF_UNROLL for (int i = 0; i < N; ++i) {
      float s = X[i * N + c];
      BF_UNROLL for (int k = 0; k < i; ++k) s = fmaf(-L[i * N + k], X[k * N + c], s);
      X[i * N + c] = s * rd[i];
    }
    BF_UNROLL for (int i = N - 1; i >= 0; --i) {
      float s = X[i * N + c];
      BF_UNROLL for (int k = i + 1; k < N; ++k) s = fmaf(-L[k * N + i], X[k * N + c], s);
      X[i * N + c] = s * rd[i];
    }
  }
  // G[i][k] = X[k][i]
  if (want_c) {
    BF_UNROLL for (int i = 0; i < N; ++i) BF_UNROLL for (int j = 0; j < N; ++j) {
      float s = X[i] * Ps[j];
      BF_UNROLL for (int k = 1; k < N; ++k) s = fmaf(X[k * N + i], Ps[k * N + j], s);
      C[i * N + j] = s;
    }
  }
  float dm[N];
  BF_UNROLL for (int i = 0; i < N; ++i) dm[i] = ms[i] - mp[i];
  BF_UNROLL for (int i = 0; i < N; ++i) {
    float s = X[i] * dm[0];
    BF_UNROLL for (int k = 1; k < N; ++k) s = fmaf(X[k * N + i], dm[k], s);
    ms[i] = m[i] + s;
  }
  BF_UNROLL for (int i = 0; i < N * N; ++i) Ps[i] = Ps[i] - Pp[i];  // D = P^s_{t+1} - P-_{t+1}
  float GD[N * N];
  BF_UNROLL for (int i = 0; i < N; ++i) BF_UNROLL for (int j = 0; j < N; ++j) {
    float s = X[i] * Ps[j];
    BF_UNROLL for (int k = 1; k < N; ++k) s = fmaf(X[k * N + i], Ps[k * N + j], s);
    GD[i * N + j] = s;
  }
  BF_UNROLL for (int i = 0; i < N; ++i) BF_UNROLL for (int j = 0; j < N; ++j) {
    float s = GD[i * N] * X[j];
    BF_UNROLL for (int k = 1; k < N; ++k) s = fmaf(GD[i * N + k], X[k * N + j], s);
    Ps[i * N + j] = P[i * N + j] + s;
  }
}

// X_t of the unscented route (the contract above): the root of P_t, then one pair of sigma points at a time; no point set
// is stored.  The points and their images are formed as the filter's predict forms them (ukf_predict: x = m + cs R[j, :],
// ukf_dyn = dyn_base_t + F_q q0).
template <int N>
__device__ __forceinline__ void rts_unsc_cross(const RtsUnsc<N>& c, float u0, const float* m, const float* P, float* X) {
#pragma clang fp contract(fast)
  float R[N * N];
  BF_UNROLL for (int i = 0; i < N * N; ++i) R[i] = P[i];
  sym_sqrt<N>(R);
  BF_UNROLL for (int i = 0; i < N * N; ++i) X[i] = 0.f;
  BF_UNROLL for (int j = 0; j < N; ++j) {
    float s[N], x[N], fp[N], fm[N];
    BF_UNROLL for (int i = 0; i < N; ++i) s[i] = c.c * R[j * N + i];
    BF_UNROLL for (int i = 0; i < N; ++i) x[i] = m[i] + s[i];
    dyn_base_t<N, N, RtsUnsc<N>>(c, x, u0, fp);
    BF_UNROLL for (int i = 0; i < N; ++i) x[i] = m[i] - s[i];
    dyn_base_t<N, N, RtsUnsc<N>>(c, x, u0, fm);
    BF_UNROLL for (int k = 0; k < N; ++k) {
      const float d = (fp[k] + c.Gq0[k]) - (fm[k] + c.Gq0[k]);
      BF_UNROLL for (int i = 0; i < N; ++i) X[k * N + i] = fmaf(d, s[i], X[k * N + i]);
    }
  }
  BF_UNROLL for (int i = 0; i < N * N; ++i) X[i] *= c.w;
}

#ifdef BF_USER_DYN
// F_t of the source route: the Jacobian of the caller's dynamics with respect to the state at (m_t, q0, u_t), by forward-mode
// dual numbers (jit_source.hip) -- one evaluation per state direction, n in all: F_q and Q never enter the backward pass.
// The seed loop is fully unrolled, so every index into the per-lane arrays is a compile-time constant (no scratch).
template <int N, class Arg>
__device__ __forceinline__ void rts_user_jacobian(const Arg& c, float u0, const float* m, float* F) {
  constexpr int DQ = Arg::DQ;
  bfu::Dual xd[N], qd[DQ], od[N];
  BF_UNROLL for (int i = 0; i < N; ++i) xd[i] = bfu::Dual(m[i]);
  BF_UNROLL for (int i = 0; i < DQ; ++i) qd[i] = bfu::Dual(c.q0[i]);
  BF_UNROLL for (int s = 0; s < N; ++s) {
    xd[s].d = 1.f;
    bfu::dynamics<bfu::Dual>(xd, qd, bfu::Dual(u0), c.theta, od);
    xd[s].d = 0.f;
    BF_UNROLL for (int i = 0; i < N; ++i) F[i * N + s] = od[i].d;
  }
}
#endif

// F_t P_t (RTS_UNSC: X_t from the sigma points) and, for the recompute path, m-_{t+1} = A m + G q0,
// P-_{t+1} = (A P) A^T + G Q_t G^T (kf_math.hpp's predict_cov association).
template <int N, int KIND, class Arg>
__device__ __forceinline__ void rts_linearize(const Arg& c, const float* gqg_t, long long t, float u0, const float* m,
                                              const float* P, float* X, float* mp, float* Pp) {
  if constexpr (KIND == RTS_UNSC) {
    rts_unsc_cross<N>(c, u0, m, P, X);
  } else {
    float F[N * N];
    if constexpr (KIND == RTS_EXT_USER) {
#ifdef BF_USER_DYN
      rts_user_jacobian<N>(c, u0, m, F);
#endif
    } else if constexpr (KIND == RTS_EXT) {
      float fx[N];
      dyn_linearize<N, 1>(c, m, u0, F, fx);
    } else {
      BF_UNROLL for (int i = 0; i < N * N; ++i) F[i] = c.A[i];
    }
    mm<N, N, N>(F, P, X);
    if constexpr (KIND == RTS_LIN_RECOMPUTE) {
      mm_nt<N, N, N>(X, F, Pp);
      const float* q = gqg_t ? gqg_t + t * (N * N) : c.GQG;
      BF_UNROLL for (int i = 0; i < N * N; ++i) Pp[i] = Pp[i] + q[i];
      mv<N, N>(F, m, mp);
      BF_UNROLL for (int i = 0; i < N; ++i) mp[i] += c.Gq0[i];
    }
  }
}

typedef float rts_f4 __attribute__((ext_vector_type(4)));  // native vector: stays in registers across the chunk loop

__device__ __forceinline__ void rts_store16(float* p, const rts_f4& v) {
  __builtin_nontemporal_store(v, reinterpret_cast<rts_f4*>(p));
}

// Rows of one staged tile: CH 16-byte pieces per row, piece q = lane + 64 i of the wave -> row q / CH, piece q % CH.
// Global row r starts at base + r * sB (floats); only floats below `lim` of each row are touched.
template <int CH>
__device__ __forceinline__ void tile_fetch(const float* base, long long sB, int lim, int lane, rts_f4* v) {
  BF_UNROLL for (int i = 0; i < CH; ++i) {
    const int q = lane + 64 * i, r = q / CH, ch = q - r * CH;
    if (ch * 4 < lim) v[i] = *reinterpret_cast<const rts_f4*>(base + (long long)r * sB + ch * 4);
  }
}
template <int CH, int PITCH>
__device__ __forceinline__ void tile_put(float* tile, int lane, const rts_f4* v) {
  BF_UNROLL for (int i = 0; i < CH; ++i) {
    const int q = lane + 64 * i, r = q / CH, ch = q - r * CH;
    *reinterpret_cast<rts_f4*>(tile + r * PITCH + ch * 4) = v[i];
  }
}
// LDS tile -> global; a piece that straddles `lim` is written dword by dword
template <int CH, int PITCH>
__device__ __forceinline__ void tile_flush(const float* tile, float* base, long long sB, int lim, int lane) {
  BF_UNROLL for (int i = 0; i < CH; ++i) {
    const int q = lane + 64 * i, r = q / CH, ch = q - r * CH;
    const rts_f4 v = *reinterpret_cast<const rts_f4*>(tile + r * PITCH + ch * 4);
    float* dst = base + (long long)r * sB + ch * 4;
    if (ch * 4 + 4 <= lim) {
      rts_store16(dst, v);
    } else if (ch * 4 < lim) {
      BF_UNROLL for (int j = 0; j < 4; ++j) if (ch * 4 + j < lim) dst[j] = v[j];
    }
  }
}

// (the body is a device function: the ahead-of-time instances below and the entry points compiled at run time around the
// caller's dynamics, jit_source.hip, are both thin kernels around it)
template <int N, int MODE, int KIND, class Arg>
__device__ __forceinline__ void rts_reg_body(const Arg& c, const float* __restrict__ gqg_t, const RtsViews& v, long long B,
                                             long long T) {
  constexpr int NN = N * N;
  const int lane = threadIdx.x;
  const long long b0 = (long long)blockIdx.x * 64;
  const long long b_raw = b0 + lane;
  if constexpr (MODE == RTS_STRIDED) {
    if (b_raw >= B) return;  // no cross-lane work on this path
  }
  const long long b = b_raw;  // staged launches hold whole waves only
  const bool want_c = v.Cs.p != nullptr;
  const bool carry_in = v.m_in != nullptr;
  float ms[N], Ps[NN];

  if constexpr (MODE == RTS_STRIDED) {
    auto ld = [&](const SView& s, long long t, int e) { return s.p[b * s.sB + t * s.sT + e * s.sE]; };
    auto st = [&](const SView& s, long long t, int e, float x) { s.p[b * s.sB + t * s.sT + e * s.sE] = x; };
    long long t = T - 1;
    if (carry_in) {
      BF_UNROLL for (int i = 0; i < N; ++i) ms[i] = v.m_in[b * N + i];
      BF_UNROLL for (int i = 0; i < NN; ++i) Ps[i] = v.P_in[b * NN + i];
    } else {
      BF_UNROLL for (int i = 0; i < N; ++i) { ms[i] = ld(v.m, t, i); st(v.ms, t, i, ms[i]); }
      BF_UNROLL for (int i = 0; i < NN; ++i) { Ps[i] = ld(v.P, t, i); st(v.Ps, t, i, Ps[i]); }
      --t;
    }
    for (; t >= 0; --t) {
      float m[N], P[NN], mp[N], Pp[NN], X[NN], C[NN];
      BF_UNROLL for (int i = 0; i < N; ++i) m[i] = ld(v.m, t, i);
      BF_UNROLL for (int i = 0; i < NN; ++i) P[i] = ld(v.P, t, i);
      if constexpr (KIND != RTS_LIN_RECOMPUTE && KIND != RTS_UNSC) {
        BF_UNROLL for (int i = 0; i < N; ++i) mp[i] = ld(v.pm, t, i);
        BF_UNROLL for (int i = 0; i < NN; ++i) Pp[i] = ld(v.pP, t, i);
      }
      const float u0 = v.u ? v.u[b * v.u_sB + t * v.u_sT] : 0.f;
      rts_linearize<N, KIND>(c, gqg_t, t, u0, m, P, X, mp, Pp);
      if constexpr (KIND == RTS_UNSC) {  // after the root: its 2 n^2 registers are free again
        BF_UNROLL for (int i = 0; i < N; ++i) mp[i] = ld(v.pm, t, i);
        BF_UNROLL for (int i = 0; i < NN; ++i) Pp[i] = ld(v.pP, t, i);
      }
      rts_step<N>(X, P, m, mp, Pp, ms, Ps, C, want_c);
      BF_UNROLL for (int i = 0; i < N; ++i) st(v.ms, t, i, ms[i]);
      BF_UNROLL for (int i = 0; i < NN; ++i) st(v.Ps, t, i, Ps[i]);
      if (want_c) BF_UNROLL for (int i = 0; i < NN; ++i) st(v.Cs, t, i, C[i]);
    }
  } else if constexpr (RtsStage<N>::OK) {
    using S = RtsStage<N>;
    constexpr int TC = S::TC;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* tm = lds;                 // m    -> m^s
    float* tP = tm + 64 * S::PM;     // P    -> P^s
    float* tpm = tP + 64 * S::PP;    // m-
    float* tpP = tpm + 64 * S::PM;   // P-   -> C
    constexpr bool LOAD_PRED = KIND != RTS_LIN_RECOMPUTE;
    // wave-uniform row bases of this wave's 64 trajectories (reference layout: sE = 1, sT = E, sB = T*E)
    const float* gm = v.m.p + b0 * v.m.sB;
    const float* gP = v.P.p + b0 * v.P.sB;
    const float* gpm = LOAD_PRED ? v.pm.p + b0 * v.pm.sB : nullptr;
    const float* gpP = LOAD_PRED ? v.pP.p + b0 * v.pP.sB : nullptr;
    float* gms = v.ms.p + b0 * v.ms.sB;
    float* gPs = v.Ps.p + b0 * v.Ps.sB;
    float* gCs = want_c ? v.Cs.p + b0 * v.Cs.sB : nullptr;
    rts_f4 fm[S::CHM], fP[S::CHP], fpm[LOAD_PRED ? S::CHM : 1], fpP[LOAD_PRED ? S::CHP : 1];
    const long long NC = (T + TC - 1) / TC;
    auto fetch = [&](long long k) __attribute__((always_inline)) {
      const long long t0 = k * TC;
      const int vs = (int)((T - t0) < TC ? (T - t0) : TC);
      tile_fetch<S::CHM>(gm + t0 * N, v.m.sB, vs * N, lane, fm);
      tile_fetch<S::CHP>(gP + t0 * NN, v.P.sB, vs * NN, lane, fP);
      if constexpr (LOAD_PRED) {
        tile_fetch<S::CHM>(gpm + t0 * N, v.pm.sB, vs * N, lane, fpm);
        tile_fetch<S::CHP>(gpP + t0 * NN, v.pP.sB, vs * NN, lane, fpP);
      }
    };
    auto put = [&]() __attribute__((always_inline)) {
      tile_put<S::CHM, S::PM>(tm, lane, fm);
      tile_put<S::CHP, S::PP>(tP, lane, fP);
      if constexpr (LOAD_PRED) {
        tile_put<S::CHM, S::PM>(tpm, lane, fpm);
        tile_put<S::CHP, S::PP>(tpP, lane, fpP);
      }
    };
    fetch(NC - 1);
    put();
    const float* rm = tm + lane * S::PM;  // this lane's rows
    const float* rP = tP + lane * S::PP;
    const float* rpm = tpm + lane * S::PM;
    const float* rpP = tpP + lane * S::PP;
    float* wm = tm + lane * S::PM;
    float* wP = tP + lane * S::PP;
    float* wC = tpP + lane * S::PP;
    for (long long k = NC - 1; k >= 0; --k) {
      const long long t0 = k * TC;
      const int vs = (int)((T - t0) < TC ? (T - t0) : TC);
      wave_lds_sync();
      if (k > 0) fetch(k - 1);  // in flight while this chunk is computed
      int s = vs - 1;
      if (k == NC - 1) {
        if (carry_in) {
          BF_UNROLL for (int i = 0; i < N; ++i) ms[i] = v.m_in[b * N + i];
          BF_UNROLL for (int i = 0; i < NN; ++i) Ps[i] = v.P_in[b * NN + i];
        } else {  // t = T-1: the filtered state, left in the tile as it is
          BF_UNROLL for (int i = 0; i < N; ++i) ms[i] = rm[s * N + i];
          BF_UNROLL for (int i = 0; i < NN; ++i) Ps[i] = rP[s * NN + i];
          --s;
        }
      }
      for (; s >= 0; --s) {
        const long long t = t0 + s;
        float m[N], P[NN], mp[N], Pp[NN], X[NN], C[NN];
        BF_UNROLL for (int i = 0; i < N; ++i) m[i] = rm[s * N + i];
        BF_UNROLL for (int i = 0; i < NN; ++i) P[i] = rP[s * NN + i];
        if constexpr (LOAD_PRED) {
          BF_UNROLL for (int i = 0; i < N; ++i) mp[i] = rpm[s * N + i];
          BF_UNROLL for (int i = 0; i < NN; ++i) Pp[i] = rpP[s * NN + i];
        }
        const float u0 = v.u ? v.u[b * v.u_sB + t * v.u_sT] : 0.f;
        rts_linearize<N, KIND>(c, gqg_t, t, u0, m, P, X, mp, Pp);
        rts_step<N>(X, P, m, mp, Pp, ms, Ps, C, want_c);
        BF_UNROLL for (int i = 0; i < N; ++i) wm[s * N + i] = ms[i];
        BF_UNROLL for (int i = 0; i < NN; ++i) wP[s * NN + i] = Ps[i];
        if (want_c) BF_UNROLL for (int i = 0; i < NN; ++i) wC[s * NN + i] = C[i];
      }
      wave_lds_sync();
      tile_flush<S::CHM, S::PM>(tm, gms + t0 * N, v.ms.sB, vs * N, lane);
      tile_flush<S::CHP, S::PP>(tP, gPs + t0 * NN, v.Ps.sB, vs * NN, lane);
      // C: entry T-1 exists only with a carry
      if (want_c) tile_flush<S::CHP, S::PP>(tpP, gCs + t0 * NN, v.Cs.sB, (k == NC - 1 && !carry_in ? vs - 1 : vs) * NN, lane);
      if (k > 0) {
        wave_lds_sync();
        put();
      }
    }
  }
  if (v.m_out) BF_UNROLL for (int i = 0; i < N; ++i) v.m_out[b * N + i] = ms[i];
  if (v.P_out) BF_UNROLL for (int i = 0; i < NN; ++i) v.P_out[b * NN + i] = Ps[i];
}

template <int N, int MODE, int KIND, class Arg>
__global__ void __launch_bounds__(64) rts_reg_kernel(Arg c, const float* __restrict__ gqg_t, RtsViews v, long long B,
                                                     long long T) {
  rts_reg_body<N, MODE, KIND, Arg>(c, gqg_t, v, B, T);
}

// ---- Gaussian-sum smoother: K chains per trajectory (the contract at the top of this file) -------------------------------
// Chain (b, k) reads and writes the streams at b sB + k sK, the inputs at b and the carries at b K + k; its arithmetic is
// rts_linearize / rts_step, the one-component kernel's, so its streams carry the same bits.
enum { GS_COMP = 1, GS_COLL = 2 };  // what a launch writes: the per-component streams, the collapsed moments, or both

struct RtsGsViews {
  RtsViews v;       // sK honoured; m_in / P_in / m_out / P_out contiguous [B][K][n] / [B][K][n][n]
  SView cm, cP;     // collapsed mean / covariance, element (b, t, e) at p[b sB + t sT + e sE]; p may be NULL
  const float* w;   // [B][K], read when a collapsed output is written
  int K;
  int KP;           // GS_COLL: lanes per trajectory, the power of two >= K (<= 64); the lanes k >= K idle with weight 0
  int b_inner;      // components only: adjacent lanes are adjacent trajectories (sB < sK), else adjacent components
};

// sum over the KP adjacent lanes of a trajectory as an adjacent-pair tree (lane ^ 1, ^ 2, ...): a + b is commutative, so
// every lane of the group holds the same bits, and the order depends on KP alone
__device__ __forceinline__ float gs_tree_sum(float x, int KP) {
  for (int off = 1; off < KP; off <<= 1) x += __shfl_xor(x, off, 64);
  return x;
}

// Register kernel, strided data path.  OUT == GS_COMP: one lane per chain, densely packed (a single trajectory with many
// components fills its waves).  OUT & GS_COLL: a trajectory's chains sit in KP adjacent lanes; after every step the n + n^2
// weighted moments are summed across them and the lane of component 0 stores mu_t, Sigma_t.  Without GS_COMP the
// per-component stores are not compiled in.
template <int N, int KIND, int OUT, class Arg>
__device__ __forceinline__ void rts_gs_reg_body(const Arg& c, const RtsGsViews& gv, long long B, long long T) {
  constexpr int NN = N * N;
  constexpr bool COMP = (OUT & GS_COMP) != 0, COLL = (OUT & GS_COLL) != 0;
  const RtsViews& v = gv.v;
  const int lane = threadIdx.x;
  const int K = gv.K;
  long long b;
  int k;
  bool act = true;
  if constexpr (COLL) {
    const int KP = gv.KP;
    b = (long long)blockIdx.x * (64 / KP) + lane / KP;
    k = lane & (KP - 1);
    act = b < B && k < K;  // idle lanes stay for the cross-lane sums
  } else {
    const long long g = (long long)blockIdx.x * 64 + lane;
    if (g >= B * K) return;  // no cross-lane work on this path
    if (gv.b_inner) { k = (int)(g / B); b = g - (long long)k * B; }
    else { b = g / K; k = (int)(g - b * K); }
  }
  const long long ch = b * K + k;
  const bool want_c = COMP && v.Cs.p != nullptr;
  const bool carry_in = v.m_in != nullptr;
  float ms[N], Ps[NN];
  float w = 0.f;
  if constexpr (COLL) {
    BF_UNROLL for (int i = 0; i < N; ++i) ms[i] = 0.f;
    BF_UNROLL for (int i = 0; i < NN; ++i) Ps[i] = 0.f;
    if (act) w = gv.w[ch];
  }
  auto ld = [&](const SView& s, long long t, int e) { return s.p[b * s.sB + k * s.sK + t * s.sT + e * s.sE]; };
  auto st = [&](const SView& s, long long t, int e, float x) { s.p[b * s.sB + k * s.sK + t * s.sT + e * s.sE] = x; };
  // mu_t = sum_k w_k m^s_k, Sigma_t = sum_k w_k (P^s_k + (m^s_k - mu_t)(m^s_k - mu_t)^T); every lane of the wave takes part
  auto collapse = [&](long long t) __attribute__((always_inline)) {
    const int KP = gv.KP;
    const bool lead = act && k == 0;
    float d[N];
    BF_UNROLL for (int i = 0; i < N; ++i) {
      const float mu = gs_tree_sum(act ? w * ms[i] : 0.f, KP);
      d[i] = ms[i] - mu;
      if (lead && gv.cm.p) gv.cm.p[b * gv.cm.sB + t * gv.cm.sT + i * gv.cm.sE] = mu;
    }
    if (gv.cP.p) {
      BF_UNROLL for (int i = 0; i < N; ++i) BF_UNROLL for (int j = 0; j < N; ++j) {
        const float s = gs_tree_sum(act ? w * fmaf(d[i], d[j], Ps[i * N + j]) : 0.f, KP);
        if (lead) gv.cP.p[b * gv.cP.sB + t * gv.cP.sT + (i * N + j) * gv.cP.sE] = s;
      }
    }
  };

  long long t = T - 1;
  if (act) {
    if (carry_in) {
      BF_UNROLL for (int i = 0; i < N; ++i) ms[i] = v.m_in[ch * N + i];
      BF_UNROLL for (int i = 0; i < NN; ++i) Ps[i] = v.P_in[ch * NN + i];
    } else {
      BF_UNROLL for (int i = 0; i < N; ++i) { ms[i] = ld(v.m, t, i); if constexpr (COMP) st(v.ms, t, i, ms[i]); }
      BF_UNROLL for (int i = 0; i < NN; ++i) { Ps[i] = ld(v.P, t, i); if constexpr (COMP) st(v.Ps, t, i, Ps[i]); }
    }
  }
  if (!carry_in) {
    if constexpr (COLL) collapse(t);
    --t;
  }
  for (; t >= 0; --t) {
    if (act) {
      float m[N], P[NN], mp[N], Pp[NN], X[NN], C[NN];
      BF_UNROLL for (int i = 0; i < N; ++i) m[i] = ld(v.m, t, i);
      BF_UNROLL for (int i = 0; i < NN; ++i) P[i] = ld(v.P, t, i);
      if constexpr (KIND != RTS_UNSC) {
        BF_UNROLL for (int i = 0; i < N; ++i) mp[i] = ld(v.pm, t, i);
        BF_UNROLL for (int i = 0; i < NN; ++i) Pp[i] = ld(v.pP, t, i);
      }
      const float u0 = v.u ? v.u[b * v.u_sB + t * v.u_sT] : 0.f;
      rts_linearize<N, KIND>(c, nullptr, t, u0, m, P, X, mp, Pp);
      if constexpr (KIND == RTS_UNSC) {  // after the root, as in rts_reg_body
        BF_UNROLL for (int i = 0; i < N; ++i) mp[i] = ld(v.pm, t, i);
        BF_UNROLL for (int i = 0; i < NN; ++i) Pp[i] = ld(v.pP, t, i);
      }
      rts_step<N>(X, P, m, mp, Pp, ms, Ps, C, want_c);
      if constexpr (COMP) {
        BF_UNROLL for (int i = 0; i < N; ++i) st(v.ms, t, i, ms[i]);
        BF_UNROLL for (int i = 0; i < NN; ++i) st(v.Ps, t, i, Ps[i]);
        if (want_c) BF_UNROLL for (int i = 0; i < NN; ++i) st(v.Cs, t, i, C[i]);
      }
    }
    if constexpr (COLL) collapse(t);
  }
  if (act) {
    if (v.m_out) BF_UNROLL for (int i = 0; i < N; ++i) v.m_out[ch * N + i] = ms[i];
    if (v.P_out) BF_UNROLL for (int i = 0; i < NN; ++i) v.P_out[ch * NN + i] = Ps[i];
  }
}

template <int N, int KIND, int OUT, class Arg>
__global__ void __launch_bounds__(64) rts_gs_reg_kernel(Arg c, RtsGsViews gv, long long B, long long T) {
  rts_gs_reg_body<N, KIND, OUT, Arg>(c, gv, B, T);
}

}  // namespace bf
