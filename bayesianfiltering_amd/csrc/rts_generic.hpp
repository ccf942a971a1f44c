// What the run-time-dimension kernels of the smoother (rts_smoother.hip) and of the posterior sampler (ffbs_sampler.hip)
// share: the per-step gain work on n x (n + 1) matrices in LDS (F_t, X = F P, the recomputed prediction, the Cholesky of
// P- and the two triangular solves), the constant block behind it and the model structs of the register kernels.
#pragma once
#include <cstring>
#include <vector>
#include "rts_smoother.hpp"
#include "generic_device.hpp"
#include "ugsf_generic_device.hpp"

namespace bf {

struct RtsGen {
  int n, kind;          // RTS_LIN, RTS_LIN_RECOMPUTE, RTS_EXT, RTS_UNSC
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

#ifdef __HIPCC__
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
template <bool UNSC>
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
// The unscented route's model on the host: the filter's own model fill (ugsf_scan.hpp: fill_ukf_model_view validates the
// registry ids and forms the constants), reduced to what X_t reads.  BF_EINVAL for ParamsUKF values with L + lambda <= 0.
struct RtsUnscHost {
  int dyn_id;
  float dth[8];
  std::vector<float> A, Gq0;
  float cu, wu;
};
int rts_unsc_fill(const bf_model* p, const bf_ukf_params* up, RtsUnscHost& h);
// the run-time-dimension kernels' constant block A | Gq0 and c for RTS_UNSC; BF_EUNSUPPORTED for dynamics they do not hold
int rts_gen_unsc_block(const RtsUnscHost& h, int n, RtsGen& c, std::vector<float>& blk);
template <int N>
inline RtsUnsc<N> rts_unsc_arg(const RtsUnscHost& h) {
  RtsUnsc<N> c;
  std::memset(&c, 0, sizeof(c));
  c.dyn_id = h.dyn_id;
  for (int i = 0; i < 8; ++i) c.dth[i] = h.dth[i];
  std::memcpy(c.A, h.A.data(), sizeof(c.A));
  std::memcpy(c.Gq0, h.Gq0.data(), sizeof(c.Gq0));
  c.c = h.cu;
  c.w = h.wu;
  return c;
}
// uploads blk (content-keyed cache) and turns the offsets of c (linear kinds, RTS_UNSC) or g (RTS_EXT) into device pointers
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
