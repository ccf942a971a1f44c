// agsf_generic_device.hpp: the device side of the run-time-dimension augmented Gaussian-sum scan (see agsf_generic.hip for the
// design notes, the LDS budget and the resource table).  The tree of agsf_scan.hpp -- N0 carried components, N1 z-samples each,
// N2 s-samples each (gaussfiltax/inference.py:621-812 and its four siblings) -- with the node in turn held in LDS instead of a
// leaf per lane in registers.  The node arithmetic is the run-time-dimension filters': generic_device.hpp's primitives in the
// order of gsf_generic_body's _predict / _condition_on (extended nodes), ugsf_generic_device.hpp's in the order of
// ugsf_generic_body's two halves (unscented nodes); the tree logic is agsf_scan.hpp's (normals, keys, block helpers).
#pragma once
#include "agsf_scan.hpp"
#include "ugsf_generic_device.hpp"

namespace bf {

enum { AG_MAX_LEAVES = 256 };   // one lane per leaf in the reweight / resample phase of a 256-thread workgroup

struct AgTree {
  int N0, N1, N2, M, variant;   // M = N0 N1 N2 leaves
  float a0, a1;                 // Delta = a0 P, Lambda = a1 P-
  uint32_t ko0, ko1;            // key of utils.optimal_resampling (variant 2): split(split(rng_key)[0])[0]
};

// ---- extended-Kalman nodes (inference.py:51-105): the carve of generic_scan.hip without the per-component weight arrays
template <int NT>
struct AgEkfNodes {
  using Model = GenModel;
  static __host__ __device__ size_t floats(int n, int dq, int m, int dr) {
    const size_t ldn = ((n + 3) & ~3) + 4, ldm = ((m + 3) & ~3) + 4, nv = (n + 3) & ~3, mv = (m + 3) & ~3;
    const size_t upd = 3 * (size_t)m * ldn + 3 * (size_t)n * ldm + 4 * (size_t)m * ldm, prd = 3 * (size_t)n * ldn;
    return (size_t)n * ldn + 2 * nv + 5 * mv + (upd > prd ? upd : prd);
  }
  int n, m, ldn, ldm;
  float *sP, *smean, *sfx, *shx, *sv, *sr, *srd, *reg;
  int* sperm;
  __device__ __forceinline__ AgEkfNodes(const Model& p, float* lds) {
    n = p.n; m = p.m;
    ldn = ((n + 3) & ~3) + 4; ldm = ((m + 3) & ~3) + 4;
    const int nv = (n + 3) & ~3, mv = (m + 3) & ~3;
    sP = lds;                 // [n][ldn]
    smean = sP + n * ldn;     // [n]
    sfx = smean + nv;         // [n]
    shx = sfx + nv;           // [m]
    sv = shx + mv;            // [m]
    sr = sv + mv;             // [m]
    srd = sr + mv;            // [m]
    sperm = reinterpret_cast<int*>(srd + mv);   // [m]
    reg = reinterpret_cast<float*>(sperm + mv);  // update scratch | predict scratch
  }
  // _predict (inference.py:51-70) of the node (smean, sP), in place
  __device__ __forceinline__ void predict(const Model& p, float u0, long long t, int tid) const {
#pragma clang fp contract(off)
    float* sF = reg;                   // [n][ldn]
    float* sFT = sF + n * ldn;         // [n][ldn]
    float* sFP = sFT + n * ldn;        // [n][ldn]
    const float* GQG = p.GQG + (p.q_tv ? t * n * n : 0);
    gen_dyn_linearize<NT>(p, smean, u0, sF, ldn, sfx, tid);
    gsync<NT>();
    transpose_lds<NT>(sFT, ldn, sF, ldn, n, n, tid);
    mm_lds<NT, 0>(sFP, ldn, sF, ldn, sP, ldn, nullptr, 0, n, n, n, tid);            // F_x P
    gsync<NT>();
    for (int e = tid; e < n * n; e += NT) sP[(e / n) * ldn + (e % n)] = GQG[e];     // P- = (F_x P) F_x^T + F_q Q F_q^T
    for (int i = tid; i < n; i += NT) smean[i] = sfx[i];
    gsync<NT>();
    mm_lds<NT, 1>(sP, ldn, sFP, ldn, sFT, ldn, sP, ldn, n, n, n, tid);
    gsync<NT>();
  }
  // _condition_on (inference.py:72-105) of the node (smean, sP) on the observation yt[a sE], in place; log-likelihood on lane 0
  __device__ __forceinline__ float condition(const Model& p, const float* __restrict__ yt, long long sE, float u0, long long t, int tid) const {
#pragma clang fp contract(off)
    float* sH = reg;                   // [m][ldn]
    float* sHP = sH + m * ldn;         // [m][ldn]
    float* sX = sHP + m * ldn;         // [m][ldn]
    float* sHT = sX + m * ldn;         // [n][ldm]
    float* sXT = sHT + n * ldm;        // [n][ldm]   K = X^T
    float* sKS = sXT + n * ldm;        // [n][ldm]
    float* sS = sKS + n * ldm;         // [m][ldm]
    float* sa = sS + m * ldm;          // [m][ldm]   LU of S + jitter
    float* sL = sa + m * ldm;          // [m][ldm]   chol(S)
    float* sRR = sL + m * ldm;         // [m][ldm]   H_r R H_r^T
    gen_emi_linearize<NT>(p, smean, u0, t, sH, ldn, shx, sRR, ldm, tid);
    for (int a = tid; a < m; a += NT) sv[a] = yt[a * sE] - shx[a];
    transpose_lds<NT>(sHT, ldm, sH, ldn, m, n, tid);
    mm_lds<NT, 0>(sHP, ldn, sH, ldn, sP, ldn, nullptr, 0, m, n, n, tid);           // H_x P
    gsync<NT>();
    mm_lds<NT, 1>(sS, ldm, sHP, ldn, sHT, ldm, sRR, ldm, m, n, m, tid);            // S = H_r R H_r^T + (H_x P) H_x^T
    for (int e = tid; e < m * n; e += NT) sX[(e / n) * ldn + (e % n)] = sHP[(e / n) * ldn + (e % n)];
    gsync<NT>();
    for (int e = tid; e < m * m; e += NT) sa[(e / m) * ldm + (e % m)] = sS[(e / m) * ldm + (e % m)] + p.jitter;
    gsync<NT>();
    lu_solve_lds<NT>(sa, ldm, sX, ldn, srd, sperm, m, n, tid);                       // psd_solve (utils.py:256-259)
    transpose_lds<NT>(sXT, ldm, sX, ldn, m, n, tid);                                 // K = X^T
    gsync<NT>();
    mm_lds<NT, 0>(sKS, ldm, sXT, ldm, sS, ldm, nullptr, 0, n, m, m, tid);            // K S (un-jittered S)
    for (int i = tid; i < n; i += NT) {                                               // m+ = m + K v
      float s = sXT[i * ldm] * sv[0];
      for (int a = 1; a < m; ++a) s = fmaf(sXT[i * ldm + a], sv[a], s);
      smean[i] += s;
    }
    gsync<NT>();
    mm_lds<NT, 2>(sP, ldn, sKS, ldm, sX, ldn, sP, ldn, n, m, n, tid);               // P+ = P - (K S) K^T
    const float ll = chol_logpdf_lds<NT>(sS, sL, ldm, sv, sr, m, tid);               // log N(y; h(m), S)
    gsync<NT>();
    return ll;
  }
};

// ---- unscented nodes (inference.py:146-174, :198-224): ug_carve as it is (its three per-component arrays at their minimum)
template <int NT>
struct AgUkfNodes {
  using Model = UgModel;
  static __host__ __device__ size_t floats(int n, int dq, int m, int dr) { return (size_t)ug_carve(n, dq, m, dr, 4).total; }
  int n, m, dq, dr, ldn, ldm, ldj;
  float *sP, *smean, *sA, *sV, *sRt, *smu, *sv, *sr, *srd, *sd, *sred, *srot, *sYp, *sYu, *sX, *sXT, *sKS, *sS, *sa, *sL;
  int* sperm;
  __device__ __forceinline__ AgUkfNodes(const Model& p, float* lds) {
    n = p.n; m = p.m; dq = p.dq; dr = p.dr;
    const UgCarve cv = ug_carve(n, dq, m, dr, 4);
    ldn = cv.ldn; ldm = cv.ldm; ldj = cv.ldj;
    sP = lds + cv.oP; sA = lds + cv.oA; sV = lds + cv.oV; sRt = lds + cv.oRt; smean = lds + cv.omean; smu = lds + cv.omu;
    sv = lds + cv.ov; sr = lds + cv.or_; srd = lds + cv.ord; sperm = reinterpret_cast<int*>(lds + cv.operm);
    sd = lds + cv.od; sred = lds + cv.ored; srot = lds + cv.orot;
    sYp = lds + cv.oreg; sYu = lds + cv.oYu; sX = lds + cv.oX; sXT = lds + cv.oXT; sKS = lds + cv.oKS;
    sS = lds + cv.oS; sa = lds + cv.oa; sL = lds + cv.oL;
  }
  __device__ __forceinline__ void predict(const Model& p, float u0, long long t, int tid) const {
#pragma clang fp contract(off)
    const float* sq = p.tvsq ? p.tvsq + t * dq * dq : p.sQ;
    const int NPp = 2 * (n + dq);
    ug_sym_sqrt<NT>(sP, ldn, sA, sV, sRt, sYp, ldj, sd, sred, srot, n, tid);
    ug_eval_dyn<NT>(p, smean, sRt, ldj, sq, u0, sYp, ldn, tid);
    gsync<NT>();
    ug_center<NT>(sYp, ldn, NPp, n, p.ws_p, p.w0_p, smean, tid);
    ug_gram<NT>(sP, ldn, sYp, ldn, NPp, n, p.ws_p, p.wc_p, tid);
    gsync<NT>();
  }
  __device__ __forceinline__ float condition(const Model& p, const float* __restrict__ yt, long long sE, float u0, long long t, int tid) const {
#pragma clang fp contract(off)
    const float* srt = p.tvsr ? p.tvsr + t * dr * dr : p.sR;
    const int NPu = 2 * (n + dr);
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
    for (int a = tid; a < m; a += NT) sv[a] = yt[a * sE] - smu[a];
    gsync<NT>();
    for (int e = tid; e < m * m; e += NT) sa[(e / m) * ldm + (e % m)] = sS[(e / m) * ldm + (e % m)] + 1e-6f;
    gsync<NT>();
    lu_solve_lds<NT>(sa, ldm, sX, ldn, srd, sperm, m, n, tid);                       // K^T = psd_solve(S, C)
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
    gsync<NT>();
    return ll;
  }
};

// LDS of a workgroup in floats: the node's carve, the factor tile, the sampled-from mean, four NT-sized arrays (log-likelihoods,
// cumulative weights, carried weights, drawn indices), the block helpers' 64 and optimal_resampling_block's 4 NT
template <int NT, class NODES>
__host__ __device__ inline size_t ag_lds_floats(int n, int dq, int m, int dr) {
  return NODES::floats(n, dq, m, dr) + (size_t)n * (((n + 3) & ~3) + 4) + ((n + 3) & ~3) + 4 * NT + 64 + 4 * NT;
}
// HBM scratch of a workgroup in floats: carried components, predicted nodes, leaves, each a record (mean, covariance)
__host__ __device__ inline size_t ag_scratch_floats(int n, int N0, int N1, int N2) {
  return ((size_t)N0 + (size_t)N0 * N1 + (size_t)N0 * N1 * N2) * ((size_t)n + (size_t)n * n);
}

// The record rc = (mean[n], P[n][n]) of a parent in HBM -> sbase = mean, sA = P - a P, sL = chol((sA + sA^T) / 2) with chol_jax's rule
// (agsf_scan.hpp: chol_lower -- same operations per entry; a pivot <= 0 or NaN gives an all-NaN factor).  Left-looking, a row per
// lane; every lane forms the pivot itself (broadcast reads), so the verdict is workgroup-uniform.
template <int NT>
__device__ __forceinline__ void ag_factor(const float* __restrict__ rc, float a, float* sA, float* sL, int ld, float* sbase, int n, int tid) {
#pragma clang fp contract(off)
  for (int e = tid; e < n * n; e += NT) {
    const int i = e / n, j = e - i * n;
    const float pk = rc[n + e];
    const float dl = a * pk;
    sA[i * ld + j] = pk - dl;
    sL[i * ld + j] = 0.f;
  }
  for (int i = tid; i < n; i += NT) sbase[i] = rc[i];
  gsync<NT>();
  bool bad = false;
  for (int j = 0; j < n; ++j) {
    float d = sA[j * ld + j];
    for (int q = 0; q < j; ++q) d = fmaf(-sL[j * ld + q], sL[j * ld + q], d);
    bad |= !(d > 0.f);
    d = fast_sqrt(d);
    const float inv = fast_rcp(d);
    for (int i = j + tid; i < n; i += NT) {
      if (i == j) {
        sL[j * ld + j] = d;
      } else {
        float s = 0.5f * (sA[i * ld + j] + sA[j * ld + i]);
        for (int q = 0; q < j; ++q) s = fmaf(-sL[i * ld + q], sL[j * ld + q], s);
        sL[i * ld + j] = s * inv;
      }
    }
    gsync<NT>();
  }
  if (bad) {
    for (int e = tid; e < n * n; e += NT) sL[(e / n) * ld + (e % n)] = __builtin_nanf("");
    gsync<NT>();
  }
}

// one sample of the parent: smean = sbase + sL eps (NaN entries -> sbase for the container variants, containers.py:84 / :121),
// sP = a P: the node (sample, a P) the filter step starts from.  eps[c * es] is entry c of this sample's normal vector.
template <int NT>
__device__ __forceinline__ void ag_sample(const float* __restrict__ rc, float a, const float* sbase, const float* sL, int ld,
                                          const float* __restrict__ eps, int es, int variant, float* sP, float* smean, int n, int tid) {
#pragma clang fp contract(off)
  for (int e = tid; e < n * n; e += NT) sP[(e / n) * ld + (e % n)] = a * rc[n + e];
  for (int i = tid; i < n; i += NT) {
    float s = 0.f;
    for (int c = 0; c <= i; ++c) s = fmaf(sL[i * ld + c], eps[c * es], s);
    float z = sbase[i] + s;
    if (variant != 0 && z != z) z = sbase[i];
    smean[i] = z;
  }
  gsync<NT>();
}

template <int NT>
__device__ __forceinline__ void ag_store(float* __restrict__ rc, const float* smean, const float* sP, int ld, int n, int tid) {
  for (int i = tid; i < n; i += NT) rc[i] = smean[i];
  for (int e = tid; e < n * n; e += NT) rc[n + e] = sP[(e / n) * ld + (e % n)];
  gsync<NT>();   // the tile is rewritten by the next sample
}

// The two arrays of standard normals of a call (the reference never advances rng_key: the same at every step and for every
// trajectory), in the oracle's layouts eps_z (N0, n, N1) and eps_s (N0 N1, n, N2); keys and counters as agsf_scan_body derives them.
__global__ void __launch_bounds__(256)
agsf_normals_kernel(float* __restrict__ eps_z, float* __restrict__ eps_s, int N0, int N1, int N2, int n, uint32_t key0, uint32_t key1,
                    int variant) {
  const long long cz = (long long)N0 * n * N1, cs = (long long)N0 * N1 * n * N2;
  const U32x2 kz = threefry_split(key0, key1, 0u, 2u);       // key, subkey = jr.split(rng_key)          :672 / :519
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < cz + cs; i += (long long)gridDim.x * blockDim.x) {
    if (i < cz) {
      const int i1 = (int)(i % N1), d = (int)((i / N1) % n), i0 = (int)(i / ((long long)N1 * n));
      if (variant == 0) {
        eps_z[i] = bits_to_normal(threefry_bits(kz.x, kz.y, (uint32_t)i, (uint32_t)cz));
      } else {
        const U32x2 sub1 = threefry_split(key0, key1, 1u, 2u);
        const U32x2 kn1 = threefry_split(sub1.x, sub1.y, (uint32_t)i0, (uint32_t)N0);
        eps_z[i] = bits_to_normal(threefry_bits(kn1.x, kn1.y, (uint32_t)(i1 * n + d), (uint32_t)(N1 * n)));   // (N1, n)
      }
    } else {
      const long long k = i - cz;
      const int i2 = (int)(k % N2), d = (int)((k / N2) % n), j = (int)(k / ((long long)N2 * n));
      if (variant == 0) {
        const U32x2 ks = threefry_split(kz.x, kz.y, 0u, 2u);     // key, _ = jr.split(key)                 :716
        eps_s[k] = bits_to_normal(threefry_bits(ks.x, ks.y, (uint32_t)k, (uint32_t)cs));
      } else {
        const U32x2 sub2 = threefry_split(kz.x, kz.y, 1u, 2u);   // key, subkey = jr.split(key)            :545
        const U32x2 kn2 = threefry_split(sub2.x, sub2.y, (uint32_t)j, (uint32_t)(N0 * N1));
        eps_s[k] = bits_to_normal(threefry_bits(kn2.x, kn2.y, (uint32_t)(i2 * n + d), (uint32_t)(N2 * n)));   // (N2, n)
      }
    }
  }
}

// One workgroup advances one trajectory at a time (trajectories blockIdx.x, blockIdx.x + gridDim.x, ...); gs: this workgroup's
// HBM scratch of ag_scratch_floats (L2-resident: it is rewritten at every step).
template <int NT, class NODES>
__device__ __forceinline__ void agsf_generic_body(const typename NODES::Model& p, const AgTree& tr, CView y, UViewG u, CarryView carry,
                                                  AgsfOut out, float* __restrict__ gs, const float* __restrict__ eps_z,
                                                  const float* __restrict__ eps_s, long long B, long long T) {
#pragma clang fp contract(off)
  constexpr int NW = NT / 64;
  const int tid = threadIdx.x;
  const int n = p.n, nn = n * n, rec = n + nn;
  const int N0 = tr.N0, N1 = tr.N1, N2 = tr.N2, M = tr.M, variant = tr.variant;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const NODES nd(p, lds);
  const int ld = nd.ldn;
  float* sLc = lds + NODES::floats(p.n, p.dq, p.m, p.dr);   // [n][ldn]  chol of the sampled-from covariance
  float* sbase = sLc + n * ld;                               // [n]       the sampled-from mean
  float* sll = sbase + ((n + 3) & ~3);                       // [NT]      leaf log-likelihoods
  float* scdf = sll + NT;                                    // [NT]      cumulative leaf weights
  float* swpar = scdf + NT;                                  // [NT]      weights of the carried components
  int* sidx = reinterpret_cast<int*>(swpar + NT);            // [NT]      drawn leaves
  float* red = reinterpret_cast<float*>(sidx + NT);          // [64]      block helpers
  float* optbuf = red + 64;                                  // [4 NT]    optimal_resampling_block
  float* gcar = gs;                                          // [N0]      carried components
  float* gnode = gcar + (size_t)N0 * rec;                    // [N0 N1]   predicted nodes
  float* gleaf = gnode + (size_t)N0 * N1 * rec;              // [M]       updated leaves

  const int l = tid;                 // the leaf this lane weighs
  const bool leaf_ok = l < M;
  const int i0l = (leaf_ok ? l : 0) / (N1 * N2);
  // uniform of the resampling draw this lane performs (lanes l < N0): uniform(PRNGKey(0), (N0,))[l]     :760
  const float udraw = bits_to_unit(threefry_bits(0u, 0u, (uint32_t)(l < N0 ? l : 0), (uint32_t)N0));

  for (long long b = blockIdx.x; b < B; b += gridDim.x) {
    for (int e = tid; e < N0 * n; e += NT) gcar[(size_t)(e / n) * rec + (e % n)] = carry.m_in[b * N0 * n + e];
    for (int e = tid; e < N0 * nn; e += NT) gcar[(size_t)(e / nn) * rec + n + (e % nn)] = carry.P_in[b * (long long)N0 * nn + e];
    swpar[l] = l < N0 ? (carry.w_in ? carry.w_in[b * N0 + l] : 1.0f / (float)N0) : 0.f;
    __syncthreads();   // global + LDS

    for (long long t = 0; t < T; ++t) {
      const float u0 = u.p ? u.p[b * u.sB + t * u.sT] : 0.f;
      // ---- z-samples of every carried component and their predictions (:665-698)
      for (int i0 = 0; i0 < N0; ++i0) {
        const float* rc = gcar + (size_t)i0 * rec;
        ag_factor<NT>(rc, tr.a0, nd.sP, sLc, ld, sbase, n, tid);
        for (int i1 = 0; i1 < N1; ++i1) {
          ag_sample<NT>(rc, tr.a0, sbase, sLc, ld, eps_z + (size_t)i0 * n * N1 + i1, N1, variant, nd.sP, nd.smean, n, tid);
          nd.predict(p, u0, t, tid);
          ag_store<NT>(gnode + (size_t)(i0 * N1 + i1) * rec, nd.smean, nd.sP, ld, n, tid);
        }
      }
      __syncthreads();   // the predicted nodes are read back by other lanes
      // ---- s-samples of every prediction and their updates (:711-737)
      const float* yt = y.p + b * y.sB + t * y.sT;
      for (int j = 0; j < N0 * N1; ++j) {
        const float* rc = gnode + (size_t)j * rec;
        ag_factor<NT>(rc, tr.a1, nd.sP, sLc, ld, sbase, n, tid);
        for (int i2 = 0; i2 < N2; ++i2) {
          ag_sample<NT>(rc, tr.a1, sbase, sLc, ld, eps_s + (size_t)j * n * N2 + i2, N2, variant, nd.sP, nd.smean, n, tid);
          const float ll = nd.condition(p, yt, y.sE, u0, t, tid);
          if (tid == 0) sll[j * N2 + i2] = ll;
          ag_store<NT>(gleaf + (size_t)(j * N2 + i2) * rec, nd.smean, nd.sP, ld, n, tid);
        }
      }
      __syncthreads();
      // ---- leaf weights (:738-743): carried weight / N1 / N2, times exp(ll - max), normalised; one lane per leaf
      const float wleaf = (swpar[i0l] / (float)N1) / (float)N2;
      const float llv = leaf_ok ? sll[l] : -__builtin_inff();
      const float mx = block_tree_reduce<NW>(llv, red, [](float a, float c) { return (a != a || c != c) ? __builtin_nanf("") : fmaxf(a, c); });
      const float ew = leaf_ok ? expf(llv - mx) * wleaf : 0.f;
      const float tot = block_tree_reduce<NW>(ew, red, [](float a, float c) { return a + c; });
      const float w = leaf_ok ? ew / tot : 0.f;
      // ---- jr.choice(PRNGKey(0), arange(M), (N0,), p = w) (:760), or utils.optimal_resampling (:1256)
      const float cw = block_cumsum_assoc<NW>(w, red + 16);
      scdf[l] = cw;
      lds_barrier();
      int idx = 0;
      float wnew = 1.0f / (float)N0;   // weights = ones / N0                                          :765
      if (variant == 2) {
        optimal_resampling_block<NW>(w, M, N0, tr.ko0, tr.ko1, optbuf, red, idx, wnew);
      } else if (l < N0) {
        const float r = scdf[M - 1] * (1.0f - udraw);
        int lo = 0, hi = M;  // first index with cdf[idx] >= r (searchsorted side='left')
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (scdf[mid] < r) lo = mid + 1; else hi = mid;
        }
        idx = lo < M - 1 ? lo : M - 1;
      }
      lds_barrier();   // every lane has read its parent's weight
      // (NaN weights leave the sort of optimal_resampling_block without an order, and a padding lane's index may surface: the
      // gather below reads leaf records by this index, so it stays inside them)
      idx = idx < 0 ? 0 : (idx > M - 1 ? M - 1 : idx);
      if (l < N0) {
        sidx[l] = idx;
        swpar[l] = wnew;
        if (out.w.p) out.w.p[b * out.w.sB + l * out.w.sK + t * out.w.sT] = wnew;
        if (out.anc) out.anc[(b * T + t) * N0 + l] = idx;
      }
      lds_barrier();
      // ---- the drawn leaves become the next carry, and the step's output
      for (int c = 0; c < N0; ++c) {
        const float* src = gleaf + (size_t)sidx[c] * rec;
        float* dst = gcar + (size_t)c * rec;
        for (int e = tid; e < rec; e += NT) {
          const float v = src[e];
          dst[e] = v;
          if (e < n) {
            if (out.m.p) out.m.p[b * out.m.sB + c * out.m.sK + t * out.m.sT + e * out.m.sE] = v;
          } else if (out.P.p) {
            out.P.p[b * out.P.sB + c * out.P.sK + t * out.P.sT + (e - n) * out.P.sE] = v;
          }
        }
      }
      __syncthreads();
    }

    // ---- carry out
    if (carry.m_out) for (int e = tid; e < N0 * n; e += NT) carry.m_out[b * N0 * n + e] = gcar[(size_t)(e / n) * rec + (e % n)];
    if (carry.P_out) for (int e = tid; e < N0 * nn; e += NT) carry.P_out[b * (long long)N0 * nn + e] = gcar[(size_t)(e / nn) * rec + n + (e % nn)];
    if (carry.w_out && l < N0) carry.w_out[b * N0 + l] = swpar[l];
    __syncthreads();   // the scratch and the weights are reused by this workgroup's next trajectory
  }
}

template <int NT, class NODES>
__global__ void __launch_bounds__(NT)
agsf_generic_kernel(typename NODES::Model p, AgTree tr, CView y, UViewG u, CarryView carry, AgsfOut out, float* __restrict__ gscratch,
                    const float* __restrict__ eps_z, const float* __restrict__ eps_s, long long B, long long T) {
  agsf_generic_body<NT, NODES>(p, tr, y, u, carry, out, gscratch + (size_t)blockIdx.x * ag_scratch_floats(p.n, tr.N0, tr.N1, tr.N2), eps_z,
                               eps_s, B, T);
}

}  // namespace bf
