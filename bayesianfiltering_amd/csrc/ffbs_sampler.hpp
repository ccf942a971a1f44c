// ffbs_sampler: batched posterior sampling, the backward half of forward-filter backward-sampling, over the streams a
// filter emitted (include/bayesfilt.h, bf_ffbs_sample_f32 / bf_effbs_sample_f32; dynamax's lgssm_posterior_sample).
//
// Math (the contract).  Inputs are the filter's streams in update -> predict order: filtered m_t, P_t and the predictions
// m-_{t+1}, P-_{t+1} at index t.  F_t as in the smoother (rts_smoother.hpp): A for the linear model, the registry Jacobian
// at (m_t, q0, u_t) for the extended one.  xi_{s,t} in R^n are standard normals for sample s.
//   t = T-1 (no carry):  x_{T-1} = m_{T-1} + psdchol(P_{T-1}; diag P_{T-1}) xi_{T-1}
//   t = T-2 ... 0:       Lp = chol(P-_{t+1})               (as the smoother: lower triangle, no jitter, NaN if not PD)
//   (with a carry:       W  = Lp^-1 (F_t P_t),  X = Lp^-T W,  G_t = X^T
//    from t = T-1)       Sigma_t = P_t - W^T W             (symmetric by construction: the lower triangle is formed)
//                        L_t = psdchol(Sigma_t; diag P_t)
//                        x_t = m_t + G_t (x_{t+1} - m-_{t+1}) + L_t xi_t
// psdchol(S; d) is a left-looking Cholesky without pivoting.  When the pivot p_j = S_jj - sum_k L_jk^2 is not greater
// than tau d_j, column j of L is zero, its diagonal included.  tau = 2^-17: a true-zero pivot is computed as cancellation
// noise of about (n + 2) 2^-24 d_j, 2^-18 d_j at n = 64, so tau sits a factor 2 above the noise and far below any pivot a
// model with non-degenerate noise produces.  For a PSD matrix a zero pivot implies a zero column, so dropping the column
// is exact and not a regularisation: a singular G Q G^T (the constant-velocity model: Sigma_t has exact rank 2) is part of
// the definition.  With xi = 0 the recursion is the RTS mean recursion.
//
// Noise: either a stream of standard normals indexed like the output, or keys[b] = (k0, k1) per trajectory, element
// (s, t, i) = bits_to_normal(threefry_bits(k0, k1, (s T + t) n + i, S T n)) (bf_rng.hpp): jax.random.normal(keys[b],
// (S, T, n)), the values bf_random_normal_f32(keys[b], S T n) writes on the host.
//
// Gaussian-sum sampler (bf_gs_sample_f32; K >= 1 components; the mixture over the initial component's index of
// rts_smoother.hpp).  Per sample (b, s) a component z: c_j = the inclusive cumulative sum of w[b][0..j] in index order by
// sequential fp32 adds; z = the smallest j with c_j > v c_{K-1}, clamped to K-1, v = comp_noise[b][s] in [0, 1) -- or
// bf_random_uniform_f32(comp_keys[b], S)[s]; c_{K-1} not finite or not > 0: the draw is invalid, z = -1, and that sample is NaN at
// every step and in the carry, other samples untouched.  comp_in[B][S] replaces the draw, comp_out[B][S] returns it.  Sample s is
// then the recursion above on chain (b, z) -- streams at b sB + z sK, inputs and keys at b -- with noise row (b, s): its bits do
// not depend on S, on the other samples' components or on the launch shape.  Noise: a stream, or keys[b] exactly as above.
//
// Register kernel (this file, n <= 8): a lane is one (trajectory, block of SPL samples); adjacent lanes are adjacent sample
// blocks of one trajectory, so the stream loads of a wave are same-address broadcasts and nothing crosses lanes.  Every
// lane repeats the factorization its trajectory shares (ALU time, no HBM traffic) and then serves its SPL samples from it.
// Run-time-dimension kernel (ffbs_sampler.hip): one wave per trajectory, matrices and a block of samples in LDS.
#pragma once
#ifndef BF_JIT
#include "bf_common.hpp"
#endif
#include "bf_rng.hpp"
#include "rts_smoother.hpp"

namespace bf {

#define BF_FFBS_TAU 7.62939453125e-06f  // 2^-17

struct FfbsViews {
  SView m, P, pm, pP;   // filtered inputs (read only)
  SView x;              // samples: element (b, s, t, e) at p[b sB + s sK + t sT + e sE]
  SView xi;             // noise, same indexing (read only); p == NULL: keys
  const uint32_t* keys; // [B][2]
  const float* x_in;    // samples at the first step after the chunk, [B][S][n]; NULL = the chunk ends at T-1
  float* x_out;         // samples at the chunk's first step
  const float* u;       // inputs, element (b, t) at u[b*u_sB + t*u_sT]; NULL = zeros
  long long u_sB, u_sT;
};

// In: S = the lower triangle of a PSD matrix (row-major N x N, the upper part is not read), d = the scale of every pivot.
// Out: S = its factor L (lower triangle, diagonal included); dropped columns are zero.
template <int N>
__device__ __forceinline__ void psdchol(float* S, const float* d) {
  BF_UNROLL for (int j = 0; j < N; ++j) {
    float p = S[j * N + j];
    BF_UNROLL for (int k = 0; k < j; ++k) p = fmaf(-S[j * N + k], S[j * N + k], p);
    const bool keep = p > BF_FFBS_TAU * d[j];
    const float r = keep ? fast_sqrt(p) : 0.f;
    const float inv = keep ? fast_rcp(r) : 0.f;
    S[j * N + j] = r;
    BF_UNROLL for (int i = j + 1; i < N; ++i) {
      float s = S[i * N + j];
      BF_UNROLL for (int k = 0; k < j; ++k) s = fmaf(-S[i * N + k], S[j * N + k], s);
      S[i * N + j] = keep ? s * inv : 0.f;
    }
  }
}

// The part of one backward step every sample of the trajectory shares.  In: X = F_t P_t, P_t, P-_{t+1}.
// Out: X with G_t[i][k] = X[k][i], Ls = L_t (lower triangle).
template <int N>
__device__ __forceinline__ void ffbs_factor(float* X, const float* P, const float* Pp, float* Ls) {
  // Cholesky of P- (lower triangle), reciprocal pivots: the smoother's rts_step
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
  // W = L^-1 X, column by column
  BF_UNROLL for (int c = 0; c < N; ++c) BF_UNROLL for (int i = 0; i < N; ++i) {
    float s = X[i * N + c];
    BF_UNROLL for (int k = 0; k < i; ++k) s = fmaf(-L[i * N + k], X[k * N + c], s);
    X[i * N + c] = s * rd[i];
  }
  // Sigma = P - W^T W, lower triangle
  BF_UNROLL for (int i = 0; i < N; ++i) BF_UNROLL for (int j = 0; j <= i; ++j) {
    float s = P[i * N + j];
    BF_UNROLL for (int k = 0; k < N; ++k) s = fmaf(-X[k * N + i], X[k * N + j], s);
    Ls[i * N + j] = s;
  }
  // X <- L^-T W
  BF_UNROLL for (int c = 0; c < N; ++c) BF_UNROLL for (int i = N - 1; i >= 0; --i) {
    float s = X[i * N + c];
    BF_UNROLL for (int k = i + 1; k < N; ++k) s = fmaf(-L[k * N + i], X[k * N + c], s);
    X[i * N + c] = s * rd[i];
  }
  float d[N];
  BF_UNROLL for (int j = 0; j < N; ++j) d[j] = P[j * N + j];
  psdchol<N>(Ls, d);
}

// ---- Gaussian-sum sampler: the component of a sample (the contract in include/bayesfilt.h, bf_gs_sample_f32) ---------------
// c_j = the inclusive cumulative sum of w[b][0..j] by sequential fp32 adds; z = the smallest j with c_j > v c_{K-1}, clamped
// to K-1; -1 (an invalid draw) when c_{K-1} is not finite or not positive.  v = comp_noise[b][s], or
// bits_to_unit(threefry_bits(comp_keys[b], s, S)): bf_random_uniform_f32(comp_keys[b], S).  z_in replaces the draw (values
// outside [0, K) count as invalid); z_out receives it.
struct GsDraw {
  const float* w;         // [B][K]
  const float* v;         // [B][S] or NULL
  const uint32_t* vkeys;  // [B][2], read when v == NULL
  const int* z_in;        // [B][S] or NULL
  int* z_out;             // [B][S] or NULL
  int K;
};
__device__ __forceinline__ int gs_draw_component(const GsDraw& d, long long b, int s, int S) {
#pragma clang fp contract(off)
  const int K = d.K;
  if (d.z_in) {
    const int z = d.z_in[b * S + s];
    return (z >= 0 && z < K) ? z : -1;
  }
  const float* w = d.w + b * K;
  float tot = w[0];
  for (int j = 1; j < K; ++j) tot = tot + w[j];
  if (!(tot > 0.f) || !(tot <= 3.4028234663852886e38f)) return -1;
  const float v = d.v ? d.v[b * S + s] : bits_to_unit(threefry_bits(d.vkeys[2 * b], d.vkeys[2 * b + 1], (uint32_t)s, (uint32_t)S));
  const float thr = v * tot;
  float c = w[0];
  int j = 0;
  while (!(c > thr) && j < K - 1) {
    ++j;
    c = c + w[j];
  }
  return j;
}

// (a device function, as rts_reg_body: shared by the ahead-of-time instances and the entry points compiled at run time)
// GS (the Gaussian-sum sampler, SPL = 1): a lane is one (trajectory, sample); its component z only changes which chain's
// streams the lane reads (b sB + z sK); an invalid draw writes NaN at every step and into the carry.
template <int N, int SPL, int KIND, class Arg, bool GS = false>
__device__ __forceinline__ void ffbs_reg_body(const Arg& c, const float* __restrict__ gqg_t, const FfbsViews& v, long long B,
                                              long long T, int S, const GsDraw* gd = nullptr) {
  constexpr int NN = N * N;
  const int NB = (S + SPL - 1) / SPL;  // sample blocks (lanes) per trajectory
  const long long g = (long long)blockIdx.x * 64 + threadIdx.x;
  const long long b = g / NB;
  if (b >= B) return;  // no cross-lane work
  const int s0 = (int)(g - b * NB) * SPL;
  int zk = 0;
  if constexpr (GS) {
    zk = gs_draw_component(*gd, b, s0, S);
    if (gd->z_out) gd->z_out[b * S + s0] = zk;
    if (zk < 0) {
      const float nan = __builtin_nanf("");
      for (long long t = 0; t < T; ++t) BF_UNROLL for (int i = 0; i < N; ++i) v.x.p[b * v.x.sB + s0 * v.x.sK + t * v.x.sT + i * v.x.sE] = nan;
      if (v.x_out) BF_UNROLL for (int i = 0; i < N; ++i) v.x_out[(b * S + s0) * N + i] = nan;
      return;
    }
  }
  const bool keyed = v.xi.p == nullptr;
  uint32_t k0 = 0, k1 = 0;
  if (keyed) {
    k0 = v.keys[2 * b];
    k1 = v.keys[2 * b + 1];
  }
  const uint32_t count = (uint32_t)S * (uint32_t)T * (uint32_t)N;
  auto ld = [&](const SView& s, long long t, int e) {
    if constexpr (GS) return s.p[b * s.sB + zk * s.sK + t * s.sT + e * s.sE];
    else return s.p[b * s.sB + t * s.sT + e * s.sE];
  };
  auto noise = [&](int s, long long t, float* z) __attribute__((always_inline)) {
    if (keyed) {
      const uint32_t base = ((uint32_t)s * (uint32_t)T + (uint32_t)t) * (uint32_t)N;
      BF_UNROLL for (int i = 0; i < N; ++i) z[i] = bits_to_normal(threefry_bits(k0, k1, base + i, count));
    } else {
      const float* q = v.xi.p + b * v.xi.sB + s * v.xi.sK + t * v.xi.sT;
      BF_UNROLL for (int i = 0; i < N; ++i) z[i] = q[i * v.xi.sE];
    }
  };
  auto emit = [&](int s, long long t, const float* x) __attribute__((always_inline)) {
    float* q = v.x.p + b * v.x.sB + s * v.x.sK + t * v.x.sT;
    BF_UNROLL for (int i = 0; i < N; ++i) q[i * v.x.sE] = x[i];
  };

  float x[SPL][N];
  long long t = T - 1;
  if (v.x_in) {
    BF_UNROLL for (int j = 0; j < SPL; ++j) if (s0 + j < S)
      BF_UNROLL for (int i = 0; i < N; ++i) x[j][i] = v.x_in[(b * S + s0 + j) * N + i];
  } else {
    float m[N], Ls[NN], d[N];
    BF_UNROLL for (int i = 0; i < N; ++i) m[i] = ld(v.m, t, i);
    BF_UNROLL for (int i = 0; i < N; ++i) BF_UNROLL for (int j = 0; j <= i; ++j) Ls[i * N + j] = ld(v.P, t, i * N + j);
    BF_UNROLL for (int i = 0; i < N; ++i) d[i] = Ls[i * N + i];
    psdchol<N>(Ls, d);
    BF_UNROLL for (int j = 0; j < SPL; ++j) if (s0 + j < S) {
      float z[N];
      noise(s0 + j, t, z);
      BF_UNROLL for (int i = 0; i < N; ++i) {
        float s = Ls[i * N] * z[0];
        BF_UNROLL for (int k = 1; k <= i; ++k) s = fmaf(Ls[i * N + k], z[k], s);
        x[j][i] = m[i] + s;
      }
      emit(s0 + j, t, x[j]);
    }
    --t;
  }
  for (; t >= 0; --t) {
    float m[N], P[NN], mp[N], Pp[NN], X[NN], Ls[NN];
    BF_UNROLL for (int i = 0; i < N; ++i) m[i] = ld(v.m, t, i);
    BF_UNROLL for (int i = 0; i < NN; ++i) P[i] = ld(v.P, t, i);
    if constexpr (KIND != RTS_LIN_RECOMPUTE) {
      BF_UNROLL for (int i = 0; i < N; ++i) mp[i] = ld(v.pm, t, i);
      BF_UNROLL for (int i = 0; i < NN; ++i) Pp[i] = ld(v.pP, t, i);
    }
    const float u0 = v.u ? v.u[b * v.u_sB + t * v.u_sT] : 0.f;
    rts_linearize<N, KIND>(c, gqg_t, t, u0, m, P, X, mp, Pp);
    ffbs_factor<N>(X, P, Pp, Ls);
    BF_UNROLL for (int j = 0; j < SPL; ++j) if (s0 + j < S) {
      float z[N], dx[N];
      noise(s0 + j, t, z);
      BF_UNROLL for (int i = 0; i < N; ++i) dx[i] = x[j][i] - mp[i];
      BF_UNROLL for (int i = 0; i < N; ++i) {
        float s = X[i] * dx[0];
        BF_UNROLL for (int k = 1; k < N; ++k) s = fmaf(X[k * N + i], dx[k], s);
        BF_UNROLL for (int k = 0; k <= i; ++k) s = fmaf(Ls[i * N + k], z[k], s);
        x[j][i] = m[i] + s;
      }
      emit(s0 + j, t, x[j]);
    }
  }
  if (v.x_out) {
    BF_UNROLL for (int j = 0; j < SPL; ++j) if (s0 + j < S)
      BF_UNROLL for (int i = 0; i < N; ++i) v.x_out[(b * S + s0 + j) * N + i] = x[j][i];
  }
}

template <int N, int SPL, int KIND, class Arg>
__global__ void __launch_bounds__(64) ffbs_reg_kernel(Arg c, const float* __restrict__ gqg_t, FfbsViews v, long long B,
                                                      long long T, int S) {
  ffbs_reg_body<N, SPL, KIND, Arg>(c, gqg_t, v, B, T, S);
}

template <int N, int KIND, class Arg>
__global__ void __launch_bounds__(64) ffbs_gs_reg_kernel(Arg c, FfbsViews v, GsDraw gd, long long B, long long T, int S) {
  ffbs_reg_body<N, 1, KIND, Arg, true>(c, nullptr, v, B, T, S, &gd);
}

}  // namespace bf
