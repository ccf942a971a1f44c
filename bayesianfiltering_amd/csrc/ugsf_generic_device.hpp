// ugsf_generic_device.hpp: the device side of the run-time-dimension unscented Gaussian-sum scan (see ugsf_generic.hip for the
// design notes, the LDS budget and the resource table).  Like generic_device.hpp, whose helpers it uses and which precedes it in
// both builds, it is compiled twice: ahead of time into libbayesfilt_hip.so (ugsf_generic.hip) and at RUN time by hiprtc around a
// user's own f / h (jit_source.hip: BF_JIT, BF_USER_DYN / BF_USER_EMI) -- so it must stay self-contained under BF_JIT.
#pragma once
#include "generic_device.hpp"

namespace bf {

struct UgModel {  // pointers are DEVICE pointers into one constant block (the flat words of ugsf_scan.hpp's UkfModel + the parameter vectors)
  int dyn_id, emi_id, n, dq, m, dr;
  float dth[8], eth[8];
  const float *A, *Gm, *Hm, *Dm, *q0, *r0;
  const float *sQ, *sR;       // sqrtm(Q), sqrtm(R) from the host (double-precision Jacobi, ugsf_scan.hpp: host_sym_sqrt) ...
  const float *tvsq, *tvsr;   // ... or one per step when the covariance is (T, d, d); NULL otherwise
  float c_u, ws_u, w0_u, wc_u;  // update, L = n + dr: sqrt(L + lambda), 1 / (2 (L + lambda)), lambda / (L + lambda), w0 + 1 - alpha^2 + beta
  float c_p, ws_p, w0_p, wc_p;  // prediction, L = n + dq
  const float *dyn_theta, *emi_theta;   // parameters of functions compiled from the caller's source
};

enum { UG_MAX_SWEEPS = 24 };   // compile-time bound of the Jacobi sweep loop (observed: DESIGN.md 4c)

// LDS carve-up in floats, shared by the kernel and by the host's size check.  Every block starts on a multiple of 4 floats.
struct UgCarve {
  int ldn, ldm, ldj, nv, mv, KPa;
  int oP, oA, oV, oRt, omean, omu, ov, or_, ord, operm, od, ored, orot, oll, ow, otree, oreg, total;
  int oYu, oX, oXT, oKS, oS, oa, oL;   // update scratch inside the shared region; the predict's point images start at oreg
};
__host__ __device__ inline UgCarve ug_carve(int n, int dq, int m, int dr, int KP) {
  UgCarve c;
  auto r4 = [](int v) { return (v + 3) & ~3; };
  c.ldn = r4(n) + 4; c.ldm = r4(m) + 4; c.ldj = n | 1;   // odd pitch: a rotation walks down two columns, one row per lane
  c.nv = r4(n); c.mv = r4(m); c.KPa = r4(KP);
  const int nj = r4(n * c.ldj), vmax = c.nv > c.mv ? c.nv : c.mv;
  int o = 0;
  auto take = [&](int k) { const int at = o; o += k; return at; };
  c.oP = take(n * c.ldn);
  c.oA = take(nj); c.oV = take(nj); c.oRt = take(nj);
  c.omean = take(c.nv); c.omu = take(vmax); c.ov = take(c.mv); c.or_ = take(c.mv); c.ord = take(c.mv); c.operm = take(c.mv);
  c.od = take(c.nv); c.ored = take(2 * c.nv); c.orot = take(4 * r4((n + 1) / 2));
  c.oll = take(c.KPa); c.ow = take(c.KPa); c.otree = take(c.KPa);
  c.oreg = o;
  const int prd = (2 * (n + dq) + 1) * c.ldn;
  c.oYu = take((2 * (n + dr) + 1) * c.ldm);
  c.oX = take(m * c.ldn); c.oXT = take(n * c.ldm); c.oKS = take(n * c.ldm);
  c.oS = take(m * c.ldm); c.oa = take(m * c.ldm); c.oL = take(m * c.ldm);
  if (o - c.oreg < prd) o = c.oreg + prd;
  c.total = o;
  return c;
}

// pair r of stage s of the round-robin (Brent-Luk) ordering over np1 + 1 indices, np1 odd: index np1 stays, the others rotate
__device__ __forceinline__ void ug_rr_pair(int s, int r, int np1, int& p, int& q) {
  int a = s + r, b = s - r;
  a = a >= np1 ? a - np1 : a;
  b = b < 0 ? b + np1 : b;
  if (r == 0) a = np1;
  p = a < b ? a : b;
  q = a < b ? b : a;
}

// C[i][j] = epi(i, j, sum_k a(i, k) b(k, j)) over n x n LDS matrices of one odd pitch ld (TA / TB: the operand is read transposed),
// k ascending, the first term a plain product; one lane per entry
template <int NT, bool TA, bool TB, class EPI>
__device__ __forceinline__ void ug_mm(const float* A, const float* Bm, int ld, int n, int tid, EPI epi) {
#pragma clang fp contract(off)
  for (int e = tid; e < n * n; e += NT) {
    const int i = e / n, j = e - i * n;
    const float* a = TA ? A + i : A + i * ld;
    const float* b = TB ? Bm + j * ld : Bm + j;
    const int sa = TA ? ld : 1, sb = TB ? 1 : ld;
    float s = a[0] * b[0];
    for (int k = 1; k < n; ++k) s = fmaf(a[k * sa], b[k * sb], s);
    epi(i, j, s);
  }
}

// Rt <- symmetric square root V diag(sqrt(max(lambda, 0))) V^T of the symmetric P (pitch ldp), all in LDS (A, V, Rt: pitch ld).
// Parallel Jacobi: a sweep is np1 stages of ceil(n / 2) disjoint rotations (odd n: one idle index); the first lanes compute
// the angles (formula and arithmetic of ugsf_scan.hpp: sym_sqrt), then the whole workgroup applies them to
// the columns of A and V and, after a barrier, to the rows of A.  Every lane reads the same off-diagonal mass from LDS, so the
// exit is workgroup-uniform; a NaN or infinite matrix leaves at the first test and comes back as NaN.  Like numpy's eigh, P is
// read through its lower triangle (P - K S K^T is symmetric to rounding only).
// Each column of V goes through sweeps x (n - 1) rotations, each leaving a rounding error of its own, so V diag(d) V^T is good to
// ~1e-6 (n = 12) ... 5e-6 (n = 40) only, and the filter amplifies that tenfold within a dozen steps.  One Newton step on
// R^2 = P -- solve R E + E R = P - R^2 in R's own eigenbasis: E = V [(V^T (P - R^2) V)_ij / (d_i + d_j)] V^T -- brings the root
// to float32 resolution (6e-8 / 2e-7) for five n^3 products in LDS (Wk: one more n x ld matrix of scratch).
template <int NT>
__device__ void ug_sym_sqrt(const float* P, int ldp, float* A, float* V, float* Rt, float* Wk, int ld, float* sd, float* red, float* rot,
                            int n, int tid) {
#pragma clang fp contract(off)
  const int nv = (n + 3) & ~3, h = (n + 1) >> 1, np1 = 2 * h - 1;
  for (int e = tid; e < n * n; e += NT) {
    const int i = e / n, j = e - i * n;
    A[i * ld + j] = i >= j ? P[i * ldp + j] : P[j * ldp + i];
    V[i * ld + j] = i == j ? 1.f : 0.f;
  }
  gsync<NT>();
  // work item e = tid + i NT of a stage <-> (rotation r0 + ..., row / column k0 + ...): stepped, not divided, in the hot loops
  const int r0 = tid / n, k0 = tid - r0 * n, rstep = NT / n, kstep = NT - rstep * n;
  auto next = [&](int& r, int& k) {
    const bool wrap = k + kstep >= n;
    r += rstep + (wrap ? 1 : 0);
    k += kstep - (wrap ? n : 0);
  };
  float off = 0.f, diag = 0.f;
  for (int sweep = 0; sweep < UG_MAX_SWEEPS; ++sweep) {
    for (int i = tid; i < n; i += NT) {
      float o = 0.f;
      for (int q = i + 1; q < n; ++q) o = fmaf(A[i * ld + q], A[i * ld + q], o);
      red[i] = o;
      red[nv + i] = A[i * ld + i] * A[i * ld + i];
    }
    gsync<NT>();
    off = 0.f;
    diag = 0.f;
    for (int i = 0; i < n; ++i) {   // broadcast reads, the same order on every lane: one value for the whole workgroup
      off += red[i];
      diag += red[nv + i];
    }
    if (!(off > 1e-14f * diag)) break;   // also leaves on NaN / Inf
    for (int s = 0; s < np1; ++s) {
      for (int r = tid; r < h; r += NT) {
        int p, q;
        ug_rr_pair(s, r, np1, p, q);
        if (q < n) {
          const float apq = A[p * ld + q], app = A[p * ld + p], aqq = A[q * ld + q];
          // tan(2 phi) = 2 a_pq / (a_qq - a_pp), the smaller root t = tan(phi); an entry already negligible (or NaN): identity
          // (single-instruction reciprocal / square roots, 1 ulp, as in the register kernel: a rotation only has to shrink a_pq,
          // and the whole workgroup waits for these few lanes)
          const float theta = (aqq - app) * fast_rcp(2.f * apq);
          float t = fast_rcp(fabsf(theta) + fast_sqrt(fmaf(theta, theta, 1.f)));
          t = theta < 0.f ? -t : t;
          t = !(fabsf(apq) > 1e-30f) ? 0.f : t;
          const float c = __builtin_amdgcn_rsqf(fmaf(t, t, 1.f));
          rot[4 * r] = c;
          rot[4 * r + 1] = t * c;
          rot[4 * r + 2] = app - t * apq;
          rot[4 * r + 3] = aqq + t * apq;
        }
      }
      gsync<NT>();
      for (int e = tid, r = r0, k = k0; e < h * n; e += NT, next(r, k)) {
        int p, q;   // columns p, q of A and V: lane <-> row
        ug_rr_pair(s, r, np1, p, q);
        if (q < n) {
          const float c = rot[4 * r], sn = rot[4 * r + 1];
          const float akp = A[k * ld + p], akq = A[k * ld + q];
          A[k * ld + p] = c * akp - sn * akq;
          A[k * ld + q] = sn * akp + c * akq;
          const float vkp = V[k * ld + p], vkq = V[k * ld + q];
          V[k * ld + p] = c * vkp - sn * vkq;
          V[k * ld + q] = sn * vkp + c * vkq;
        }
      }
      gsync<NT>();
      for (int e = tid, r = r0, k = k0; e < h * n; e += NT, next(r, k)) {
        int p, q;   // rows p, q of A: lane <-> column; the 2 x 2 block takes its closed form
        ug_rr_pair(s, r, np1, p, q);
        if (q < n) {
          const float c = rot[4 * r], sn = rot[4 * r + 1];
          const float apk = A[p * ld + k], aqk = A[q * ld + k];
          float np_ = c * apk - sn * aqk, nq_ = sn * apk + c * aqk;
          if (k == p) { np_ = rot[4 * r + 2]; nq_ = 0.f; }
          if (k == q) { np_ = 0.f; nq_ = rot[4 * r + 3]; }
          A[p * ld + k] = np_;
          A[q * ld + k] = nq_;
        }
      }
      gsync<NT>();
    }
  }
  const float poison = (off + diag) * 0.f;   // 0, or NaN for a matrix that was not finite
  for (int k = tid; k < n; k += NT) sd[k] = sqrtf(fmaxf(A[k * ld + k], 0.f)) + poison;
  gsync<NT>();
  for (int e = tid; e < n * n; e += NT) {
    const int i = e / n, j = e - i * n;
    if (j >= i) {
      float s = 0.f;
      for (int k = 0; k < n; ++k) s = fmaf(V[i * ld + k] * sd[k], V[j * ld + k], s);
      Rt[i * ld + j] = s;
      Rt[j * ld + i] = s;
    }
  }
  gsync<NT>();
  // ---- the Newton step
  ug_mm<NT, false, true>(Rt, Rt, ld, n, tid, [&](int i, int j, float s) {           // A <- P - R R^T
    A[i * ld + j] = (i >= j ? P[i * ldp + j] : P[j * ldp + i]) - s;
  });
  gsync<NT>();
  ug_mm<NT, false, false>(A, V, ld, n, tid, [&](int i, int j, float s) { Wk[i * ld + j] = s; });   // Wk <- (P - R^2) V
  gsync<NT>();
  ug_mm<NT, true, false>(V, Wk, ld, n, tid, [&](int i, int j, float s) {            // A <- V^T (P - R^2) V / (d_i + d_j)
    const float den = sd[i] + sd[j];
    A[i * ld + j] = den > 0.f ? s / den : 0.f;
  });
  gsync<NT>();
  ug_mm<NT, false, false>(V, A, ld, n, tid, [&](int i, int j, float s) { Wk[i * ld + j] = s; });   // Wk <- V W
  gsync<NT>();
  ug_mm<NT, false, true>(Wk, V, ld, n, tid, [&](int i, int j, float s) {            // R <- R + (V W) V^T, upper triangle mirrored
    if (j >= i) {
      const float r = Rt[i * ld + j] + s;
      Rt[i * ld + j] = r;
      Rt[j * ld + i] = r;
    }
  });
  gsync<NT>();
}

// The images of the 2 L sigma points of utils.py:247-254 and of the centre under f(x, q, u): Y [2 L + 1][ldy], L = n + dq, rows in
// the oracle's order (L plus rows, L minus rows; inside each the n state-block rows carry the noise bias, the dq noise-block rows
// carry the mean), the centre (mean, bias) last.  One work item per (point, output row); the registry formulas and their
// per-entry operation order are those of models.hpp / sample_generic_kernel.
template <int NT>
__device__ void ug_eval_dyn(const UgModel& p, const float* mean, const float* Rt, int ld, const float* sq, float u0, float* Y, int ldy,
                            int tid) {
#pragma clang fp contract(off)
  const int n = p.n, dq = p.dq, L = n + dq, NP = 2 * L;
#ifdef BF_USER_DYN
  if (p.dyn_id == DYN_USER) {   // the caller's f: one lane per point, the point in registers at the handle's dimensions
    for (int pt = tid; pt <= NP; pt += NT) {
      const int j = pt >= L ? pt - L : pt;
      const float cs = pt == NP ? 0.f : (pt >= L ? -p.c_p : p.c_p);
      const bool st = pt < NP && j < n, nz = pt < NP && j >= n;
      float xs[BF_N], qs[BF_DQ], o[BF_N];
      BF_UNROLL for (int k = 0; k < BF_N; ++k) xs[k] = st ? mean[k] + cs * Rt[j * ld + k] : mean[k];
      BF_UNROLL for (int k = 0; k < BF_DQ; ++k) qs[k] = nz ? p.q0[k] + cs * sq[(j - n) * dq + k] : p.q0[k];
      bfu::dynamics<float>(xs, qs, u0, p.dyn_theta, o);
      BF_UNROLL for (int i = 0; i < BF_N; ++i) Y[pt * ldy + i] = o[i];
    }
    return;
  }
#endif
  for (int e = tid; e < (NP + 1) * n; e += NT) {
    const int pt = e / n, i = e - pt * n;
    const int j = pt >= L ? pt - L : pt;
    const float cs = pt == NP ? 0.f : (pt >= L ? -p.c_p : p.c_p);
    const bool st = pt < NP && j < n, nz = pt < NP && j >= n;
    const float* row = Rt + (st ? j : 0) * ld;
    const float* sqr = sq + (nz ? j - n : 0) * dq;
    auto X = [&](int k) { return st ? mean[k] + cs * row[k] : mean[k]; };
    auto Qn = [&](int k) { return nz ? p.q0[k] + cs * sqr[k] : p.q0[k]; };
    float o;
    if (p.dyn_id == DYN_LINEAR) {
      float s = p.A[i * n] * X(0), g = 0.f;
      for (int k = 1; k < n; ++k) s = fmaf(p.A[i * n + k], X(k), s);
      for (int k = 0; k < dq; ++k) g = fmaf(p.Gm[i * dq + k], Qn(k), g);
      o = s + g;
    } else if (p.dyn_id == DYN_LORENZ96) {
      const float alpha = p.dth[0], beta = p.dth[1], gamma = p.dth[2], dt = p.dth[3];
      const float xi = X(i), ax = X((i + n - 1) % n);
      const float bx = (p.dth[4] != 0.f) ? (X((i + 1) % n) - X((i + 2 * n - 2) % n)) : 0.f;
      o = xi + dt * (alpha * (ax * bx) - beta * xi + gamma);
      o += Qn(i);
    } else {  // DYN_SINE
      o = sinf(p.dth[0] * X(i));
      o += Qn(i);
    }
    Y[pt * ldy + i] = o;
  }
}

// The same for h(x, r, u): Y [2 L + 1][ldy], L = n + dr
template <int NT>
__device__ void ug_eval_emi(const UgModel& p, const float* mean, const float* Rt, int ld, const float* sr_, float u0, float* Y, int ldy,
                            int tid) {
#pragma clang fp contract(off)
  const int n = p.n, m = p.m, dr = p.dr, L = n + dr, NP = 2 * L;
#ifdef BF_USER_EMI
  if (p.emi_id == EMI_USER) {
    for (int pt = tid; pt <= NP; pt += NT) {
      const int j = pt >= L ? pt - L : pt;
      const float cs = pt == NP ? 0.f : (pt >= L ? -p.c_u : p.c_u);
      const bool st = pt < NP && j < n, nz = pt < NP && j >= n;
      float xs[BF_N], rs[BF_DR], o[BF_M];
      BF_UNROLL for (int k = 0; k < BF_N; ++k) xs[k] = st ? mean[k] + cs * Rt[j * ld + k] : mean[k];
      BF_UNROLL for (int k = 0; k < BF_DR; ++k) rs[k] = nz ? p.r0[k] + cs * sr_[(j - n) * dr + k] : p.r0[k];
      bfu::emission<float>(xs, rs, u0, p.emi_theta, o);
      BF_UNROLL for (int a = 0; a < BF_M; ++a) Y[pt * ldy + a] = o[a];
    }
    return;
  }
#endif
  for (int e = tid; e < (NP + 1) * m; e += NT) {
    const int pt = e / m, a = e - pt * m;
    const int j = pt >= L ? pt - L : pt;
    const float cs = pt == NP ? 0.f : (pt >= L ? -p.c_u : p.c_u);
    const bool st = pt < NP && j < n, nz = pt < NP && j >= n;
    const float* row = Rt + (st ? j : 0) * ld;
    const float* srr = sr_ + (nz ? j - n : 0) * dr;
    auto X = [&](int k) { return st ? mean[k] + cs * row[k] : mean[k]; };
    auto Rn = [&](int k) { return nz ? p.r0[k] + cs * srr[k] : p.r0[k]; };
    float o;
    if (p.emi_id == EMI_LINEAR) {
      float s = p.Hm[a * n] * X(0), g = 0.f;
      for (int k = 1; k < n; ++k) s = fmaf(p.Hm[a * n + k], X(k), s);
      for (int k = 0; k < dr; ++k) g = fmaf(p.Dm[a * dr + k], Rn(k), g);
      o = s + g;
    } else if (p.emi_id == EMI_QUADRATIC) {  // m = dr = 1
      float s = 0.f;
      for (int k = 0; k < n; ++k) s = fmaf(X(k), X(k), s);
      o = p.eth[0] * s;
      o += Rn(0);
    } else {  // EMI_STOCH_VOL, m = dr = n: the noise enters multiplicatively
      const float sigma = p.eth[0], beta = p.eth[1], c = p.eth[2];
      const float xa = X(a), ra = Rn(a);
      o = u0 * beta * expf(xa / sigma) * ra + (1.f - u0) * (c * xa + ra);
    }
    Y[pt * ldy + a] = o;
  }
}

// mu = sum of the NP images * ws + image of the centre * w0 (inference.py:165-166, :210-211); then Y <- Y - mu, centre row included
template <int NT>
__device__ void ug_center(float* Y, int ldy, int NP, int d, float ws, float w0, float* mu, int tid) {
#pragma clang fp contract(off)
  for (int i = tid; i < d; i += NT) {
    float s = Y[i];
    for (int pt = 1; pt < NP; ++pt) s += Y[pt * ldy + i];
    mu[i] = s * ws + Y[NP * ldy + i] * w0;
  }
  gsync<NT>();
  for (int e = tid; e < (NP + 1) * d; e += NT) {
    const int pt = e / d, i = e - pt * d;
    Y[pt * ldy + i] -= mu[i];
  }
  gsync<NT>();
}

// C = dev^T dev * ws + wc * outer(d0, d0) (inference.py:168-170, :213-214): dev the NP deviation rows of Y, d0 its centre row;
// one lane per 1 x 4 output block as in mm_lds (ldy a multiple of 4)
template <int NT>
__device__ void ug_gram(float* C, int ldc, const float* Y, int ldy, int NP, int d, float ws, float wc, int tid) {
#pragma clang fp contract(off)
  const int c4 = (d + 3) >> 2;
  const float* d0 = Y + NP * ldy;
  for (int e = tid; e < d * c4; e += NT) {
    const int i = e / c4, j = (e - i * c4) * 4;
    float a = Y[i];
    float4 b = *reinterpret_cast<const float4*>(Y + j);
    float s[4] = {a * b.x, a * b.y, a * b.z, a * b.w};
    for (int pt = 1; pt < NP; ++pt) {
      a = Y[pt * ldy + i];
      b = *reinterpret_cast<const float4*>(Y + pt * ldy + j);
      s[0] = fmaf(a, b.x, s[0]);
      s[1] = fmaf(a, b.y, s[1]);
      s[2] = fmaf(a, b.z, s[2]);
      s[3] = fmaf(a, b.w, s[3]);
    }
    BF_UNROLL for (int q = 0; q < 4; ++q) if (j + q < d) C[i * ldc + j + q] = s[q] * ws + wc * (d0[i] * d0[j + q]);
  }
}

template <int NT>
__device__ __forceinline__ void ugsf_generic_body(const UgModel& p, CView y, UViewG u, CarryView carry, OutViews out,
                                                  float* __restrict__ gm, float* __restrict__ gP, long long B, long long T, int K,
                                                  int KP) {
  // contraction off, every fused multiply-add written out: the ahead-of-time build and a run-time build of this text agree bit for bit
#pragma clang fp contract(off)
  const int tid = threadIdx.x;
  const long long b = blockIdx.x;
  const int n = p.n, m = p.m, dq = p.dq, dr = p.dr;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const UgCarve cv = ug_carve(n, dq, m, dr, KP);
  const int ldn = cv.ldn, ldm = cv.ldm, ldj = cv.ldj;
  float* sP = lds + cv.oP;          // [n][ldn]  carried covariance of the component in turn
  float* sA = lds + cv.oA;          // [n][ldj]  Jacobi iterate
  float* sV = lds + cv.oV;          // [n][ldj]  eigenvectors
  float* sRt = lds + cv.oRt;        // [n][ldj]  sqrtm(P)
  float* smean = lds + cv.omean;    // [n]
  float* smu = lds + cv.omu;        // [max(n, m)]
  float* sv = lds + cv.ov;          // [m]  y - mu
  float* sr = lds + cv.or_;         // [m]
  float* srd = lds + cv.ord;        // [m]
  int* sperm = reinterpret_cast<int*>(lds + cv.operm);
  float* sd = lds + cv.od;          // [n]  sqrt of the eigenvalues
  float* sred = lds + cv.ored;      // [2][nv]  per-row off-diagonal / diagonal mass
  float* srot = lds + cv.orot;      // [ceil(n / 2)][4]  c, s, new a_pp, new a_qq
  float* sll = lds + cv.oll;
  float* sw = lds + cv.ow;
  float* stree = lds + cv.otree;
  float* sYp = lds + cv.oreg;       // [2 (n + dq) + 1][ldn]  predict: images f(x) - aliases the update scratch below; and, while a
                                    // square root is taken (nothing in the region is live then), its n x ldj scratch
  float* sYu = lds + cv.oYu;        // [2 (n + dr) + 1][ldm]  update: images h(x)
  float* sX = lds + cv.oX;          // [m][ldn]  C^T, then K^T
  float* sXT = lds + cv.oXT;        // [n][ldm]  K
  float* sKS = lds + cv.oKS;        // [n][ldm]
  float* sS = lds + cv.oS;          // [m][ldm]
  float* sa = lds + cv.oa;          // [m][ldm]  LU of S + 1e-6
  float* sL = lds + cv.oL;          // [m][ldm]  chol(S)

  for (int k = tid; k < KP; k += NT) sw[k] = (k < K) ? (carry.w_in ? carry.w_in[b * K + k] : 1.0f / (float)K) : 0.f;
  // K == 1: the state stays in LDS for the whole scan; K > 1: the components take turns (HBM scratch, L2-resident)
  const float* m_src = carry.m_in + b * (long long)K * n;
  const float* P_src = carry.P_in + b * (long long)K * n * n;
  float* gmb = gm ? gm + b * (long long)K * n : nullptr;
  float* gPb = gP ? gP + b * (long long)K * n * n : nullptr;
  if (K == 1) {
    for (int e = tid; e < n * n; e += NT) sP[(e / n) * ldn + (e % n)] = P_src[e];
    for (int i = tid; i < n; i += NT) smean[i] = m_src[i];
  }
  gsync<NT>();

  const int NPu = 2 * (n + dr), NPp = 2 * (n + dq);
  for (long long t = 0; t < T; ++t) {
    const float u0 = u.p ? u.p[b * u.sB + t * u.sT] : 0.f;
    const float* sq = p.tvsq ? p.tvsq + t * dq * dq : p.sQ;
    const float* srt = p.tvsr ? p.tvsr + t * dr * dr : p.sR;
    // (a component's prediction does not read the weights: condition + predict per component, then the reweight over all K,
    // gives what "condition all, reweight, predict all" of inference.py:421-430 gives)
    for (int k = 0; k < K; ++k) {
      if (K > 1) {
        const float* ms = (t == 0) ? m_src + k * n : gmb + k * n;
        const float* Ps = (t == 0) ? P_src + (long long)k * n * n : gPb + (long long)k * n * n;
        for (int e = tid; e < n * n; e += NT) sP[(e / n) * ldn + (e % n)] = Ps[e];
        for (int i = tid; i < n; i += NT) smean[i] = ms[i];
        gsync<NT>();
      }
      // ================= _ukf_condition_on_nonadditive (inference.py:198-224)
      ug_sym_sqrt<NT>(sP, ldn, sA, sV, sRt, sYp, ldj, sd, sred, srot, n, tid);
      ug_eval_emi<NT>(p, smean, sRt, ldj, srt, u0, sYu, ldm, tid);
      gsync<NT>();
      ug_center<NT>(sYu, ldm, NPu, m, p.ws_u, p.w0_u, smu, tid);
      ug_gram<NT>(sS, ldm, sYu, ldm, NPu, m, p.ws_u, p.wc_u, tid);
      // cross-covariance: only the state-block points move the state, by +- c sqrtm(P)[j, :]
      for (int e = tid; e < m * n; e += NT) {
        const int a = e / n, i = e - a * n;
        float s = 0.f;
        for (int j = 0; j < n; ++j) s = fmaf(sYu[j * ldm + a], p.c_u * sRt[j * ldj + i], s);
        for (int j = 0; j < n; ++j) s = fmaf(sYu[(n + dr + j) * ldm + a], -(p.c_u * sRt[j * ldj + i]), s);
        sX[a * ldn + i] = s * p.ws_u;
      }
      for (int a = tid; a < m; a += NT) sv[a] = y.p[b * y.sB + t * y.sT + a * y.sE] - smu[a];
      gsync<NT>();
      for (int e = tid; e < m * m; e += NT) sa[(e / m) * ldm + (e % m)] = sS[(e / m) * ldm + (e % m)] + 1e-6f;
      gsync<NT>();
      lu_solve_lds<NT>(sa, ldm, sX, ldn, srd, sperm, m, n, tid);                       // K^T = psd_solve(S, C) (utils.py:256-259)
      transpose_lds<NT>(sXT, ldm, sX, ldn, m, n, tid);
      gsync<NT>();
      mm_lds<NT, 0>(sKS, ldm, sXT, ldm, sS, ldm, nullptr, 0, n, m, m, tid);            // K S (un-jittered S)
      for (int i = tid; i < n; i += NT) {                                               // m+ = m + K (y - mu)
        float s = sXT[i * ldm] * sv[0];
        for (int a = 1; a < m; ++a) s = fmaf(sXT[i * ldm + a], sv[a], s);
        smean[i] += s;
      }
      gsync<NT>();
      mm_lds<NT, 2>(sP, ldn, sKS, ldm, sX, ldn, sP, ldn, n, m, n, tid);               // P+ = P - (K S) K^T
      const float ll = chol_logpdf_lds<NT>(sS, sL, ldm, sv, sr, m, tid);               // MVN(mu, S).log_prob(y)
      if (tid == 0) {
        sll[k] = ll;
        if (out.ll.p) out.ll.p[b * out.ll.sB + k * out.ll.sK + t * out.ll.sT] = ll;
      }
      gsync<NT>();
      if (out.m.p) for (int i = tid; i < n; i += NT) out.m.p[b * out.m.sB + k * out.m.sK + t * out.m.sT + i * out.m.sE] = smean[i];
      if (out.P.p) for (int e = tid; e < n * n; e += NT)
          out.P.p[b * out.P.sB + k * out.P.sK + t * out.P.sT + e * out.P.sE] = sP[(e / n) * ldn + (e % n)];
      // ================= _ukf_predict_nonadditive (inference.py:146-174)
      ug_sym_sqrt<NT>(sP, ldn, sA, sV, sRt, sYp, ldj, sd, sred, srot, n, tid);
      ug_eval_dyn<NT>(p, smean, sRt, ldj, sq, u0, sYp, ldn, tid);
      gsync<NT>();
      ug_center<NT>(sYp, ldn, NPp, n, p.ws_p, p.w0_p, smean, tid);
      ug_gram<NT>(sP, ldn, sYp, ldn, NPp, n, p.ws_p, p.wc_p, tid);
      gsync<NT>();
      if (out.pm.p) for (int i = tid; i < n; i += NT) out.pm.p[b * out.pm.sB + k * out.pm.sK + t * out.pm.sT + i * out.pm.sE] = smean[i];
      if (out.pP.p) for (int e = tid; e < n * n; e += NT)
          out.pP.p[b * out.pP.sB + k * out.pP.sK + t * out.pP.sT + e * out.pP.sE] = sP[(e / n) * ldn + (e % n)];
      if (K > 1) {
        for (int e = tid; e < n * n; e += NT) gPb[(long long)k * n * n + e] = sP[(e / n) * ldn + (e % n)];
        for (int i = tid; i < n; i += NT) gmb[k * n + i] = smean[i];
        __syncthreads();  // global + LDS: the next component reuses the tile, the next step reads this component back
      }
    }
    reweight_lds<NT>(sll, sw, stree, K, KP, out.w, b, t, tid);   // (inference.py:424-427)
  }

  // ---- carry out
  if (K == 1) {
    if (carry.P_out) for (int e = tid; e < n * n; e += NT) carry.P_out[b * (long long)n * n + e] = sP[(e / n) * ldn + (e % n)];
    if (carry.m_out) for (int i = tid; i < n; i += NT) carry.m_out[b * (long long)n + i] = smean[i];
  } else {
    // the HBM scratch IS the carry when the caller asked for it; otherwise copy nothing
    if (carry.P_out && carry.P_out != gP)
      for (long long e = tid; e < (long long)K * n * n; e += NT) carry.P_out[b * (long long)K * n * n + e] = gPb[e];
    if (carry.m_out && carry.m_out != gm)
      for (long long e = tid; e < (long long)K * n; e += NT) carry.m_out[b * (long long)K * n + e] = gmb[e];
  }
  if (carry.w_out) for (int k = tid; k < K; k += NT) carry.w_out[b * K + k] = sw[k];
}

#ifndef BF_JIT
template <int NT>
__global__ void __launch_bounds__(NT)
ugsf_generic_kernel(UgModel p, CView y, UViewG u, CarryView carry, OutViews out, float* __restrict__ gm, float* __restrict__ gP,
                    long long B, long long T, int K, int KP) {
  ugsf_generic_body<NT>(p, y, u, carry, out, gm, gP, B, T, K, KP);
}
#endif

}  // namespace bf
