// What the run-time-dimension kernels of the smoother (rts_smoother.hip) and of the posterior sampler (ffbs_sampler.hip)
// share: the per-step gain work on n x (n + 1) matrices in LDS (F_t, X = F P, the recomputed prediction, the Cholesky of
// P- and the two triangular solves), the constant block behind it and the model structs of the register kernels.
#pragma once
#include <cstring>
#include <vector>
#include "rts_smoother.hpp"
#include "generic_device.hpp"

namespace bf {

struct RtsGen {
  int n, kind;          // RTS_LIN, RTS_LIN_RECOMPUTE, RTS_EXT
  const float* A;       // [n][n]            (linear kinds)
  const float* GQG;     // [q_steps][n][n]   (recompute)
  const float* Gq0;     // [n]               (recompute)
  int q_tv;
};

__host__ __device__ inline int rts_gen_ld(int n) { return n + 1; }

#ifdef __HIPCC__
// W <- F_t (registry dynamics; linear: A is read from the constant block), X = F P, [recompute: P- = X F^T + GQG_t,
// m- = F m + G q0].  One 64-lane wave; m, P (and, unless recomputed, m-, P-) are in LDS and synchronised on entry; X
// (and P-, m-) are synchronised on return.
__device__ __forceinline__ void rts_gen_linearize(const RtsGen& c, const GenModel& g, float u0, long long t, const float* m,
                                                  const float* P, float* mp, float* Pp, float* X, float* W, float* tv, int tid) {
  const int n = c.n, ld = rts_gen_ld(n), nn = n * n;
  const float* F;
  int ldf;
  if (c.kind == RTS_EXT) {
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
#endif

// ---- host side (defined in rts_smoother.hip) --------------------------------------------------------------------------
int gen_fill(const bf_model* p, long long T, GenModel& g, std::vector<float>& blk);  // generic_scan.hip
// A, G Q_s G^T for every step s of Q (zeros without Q), G q0 (lgssm_pack.hpp: the bits the filters upload)
void rts_lin_fill(const bf_lgssm* p, std::vector<float>& A, std::vector<float>& GQG, std::vector<float>& Gq0);
// the linear kinds' constant block A | Gq0 | GQG[qs], with c's pointers as offsets into it
void rts_gen_lin_block(const bf_lgssm* p, bool recompute, const std::vector<float>& A, const std::vector<float>& GQG,
                       const std::vector<float>& Gq0, RtsGen& c, std::vector<float>& blk);
// uploads blk (content-keyed cache) and turns the offsets of c (linear kinds) or g (RTS_EXT) into device pointers
int rts_gen_upload(RtsGen& c, GenModel& g, const std::vector<float>& blk, hipStream_t stream);

template <int N>
inline RtsLin<N> rts_lin_arg(const std::vector<float>& A, const std::vector<float>& GQG, const std::vector<float>& Gq0) {
  RtsLin<N> c;
  std::memcpy(c.A, A.data(), sizeof(c.A));
  std::memcpy(c.GQG, GQG.data(), sizeof(c.GQG));
  std::memcpy(c.Gq0, Gq0.data(), sizeof(c.Gq0));
  return c;
}
template <int N>
inline EkfModel<N, 1> rts_ekf_arg(const bf_model* p, const GenModel& g) {
  EkfModel<N, 1> e;
  std::memset(&e, 0, sizeof(e));
  e.dyn_id = p->dyn_id;
  for (int i = 0; i < 8; ++i) e.dth[i] = g.dth[i];
  if (p->dyn_id == DYN_LINEAR) for (int i = 0; i < N * N; ++i) e.A[i] = p->dyn_theta[i];
  return e;
}

// return GO_(std::integral_constant<int, n>{}) for n = 1 ... 8
#define BF_RTS_DIMS(N_, GO_)                                     \
  switch (N_) {                                                  \
    case 1: return GO_(std::integral_constant<int, 1>{});        \
    case 2: return GO_(std::integral_constant<int, 2>{});        \
    case 3: return GO_(std::integral_constant<int, 3>{});        \
    case 4: return GO_(std::integral_constant<int, 4>{});        \
    case 5: return GO_(std::integral_constant<int, 5>{});        \
    case 6: return GO_(std::integral_constant<int, 6>{});        \
    case 7: return GO_(std::integral_constant<int, 7>{});        \
    default: return GO_(std::integral_constant<int, 8>{});       \
  }

}  // namespace bf
