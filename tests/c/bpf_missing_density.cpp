// bpf_step_density + emission_loglik_masked (csrc/bpf_missing.hpp) on every observation pattern of M <= 8 components, random
// full R_lp, with and without the stochastic-volatility scale, against the arithmetic of emission_loglik (csrc/ssm_device.hpp)
// on the COMPACTED problem -- rows and columns of R_lp, entries of y, of the mean and of the scale selected by hand, the factor
// by the plain loops of cholesky_lower -- bit for bit: the embedded factor is the compacted factor plus exact zeros, and its
// missing rows are e_a.  The missing entries of y, of the mean and of the scale are NaN on the embedded side: nothing of them
// may leak.  Host build (host_shim/hip/hip_runtime.h), compiled without fused multiply-add contraction so that both sides
// round alike.  Exit status 0 = no mismatch.
#define __host__
#include "bpf_missing.hpp"
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
using namespace bf;

// cholesky_lower of ssm_device.hpp, restated (that header needs the HIP runtime)
static int chol(const float* A, int n, float* L) {
  for (int i = 0; i < n * n; ++i) L[i] = 0.f;
  for (int j = 0; j < n; ++j) {
    float d = A[j * n + j];
    for (int k = 0; k < j; ++k) d -= L[j * n + k] * L[j * n + k];
    if (!(d > 0.f)) return -1;
    d = sqrtf(d);
    L[j * n + j] = d;
    for (int i = j + 1; i < n; ++i) {
      float s = A[i * n + j];
      for (int k = 0; k < j; ++k) s -= L[i * n + k] * L[j * n + k];
      L[i * n + j] = s / d;
    }
  }
  return 0;
}

// emission_loglik on r components: the constant as fill_bpf_model_view forms it, the loop as the kernel runs it
static float compact_loglik(int r, const float* R, const float* y, const float* hx, const float* scale) {
  float L[64], rd[8], zz[8];
  if (chol(R, r, L) != 0) return NAN;
  float logdet = 0.f;
  for (int i = 0; i < r; ++i) {
    rd[i] = 1.0f / L[i * r + i];
    logdet += canon_log(L[i * r + i]);
  }
  const float lp_const = -0.5f * (float)r * 1.8378770664093453f - logdet;
  float quad = 0.f, lsc = 0.f;
  for (int a = 0; a < r; ++a) {
    float s = y[a] - hx[a];
    if (scale) {
      s = s / scale[a];
      lsc = lsc + canon_log(scale[a]);
    }
    for (int c = 0; c < a; ++c) s = __builtin_fmaf(-L[a * r + c], zz[c], s);
    zz[a] = s * rd[a];
    quad = __builtin_fmaf(zz[a], zz[a], quad);
  }
  return __builtin_fmaf(-0.5f, quad, lp_const) - lsc;
}

static bool same_bits(float a, float b) { return std::memcmp(&a, &b, 4) == 0; }

template <int M>
int all(std::mt19937& g, long* checked) {
  std::normal_distribution<float> nd;
  std::uniform_real_distribution<float> ud(0.3f, 3.0f);
  int bad = 0;
  for (int rep = 0; rep < 40; ++rep) {
    float Lr[M * M], R[M * M], y[M], hx[M], sc[M];
    for (auto& x : Lr) x = 0.5f * nd(g);
    for (int i = 0; i < M; ++i)
      for (int j = 0; j < M; ++j) {
        float s = 0.2f * (i == j);
        for (int k = 0; k < M; ++k) s += Lr[i * M + k] * Lr[j * M + k];
        R[i * M + j] = s;
      }
    for (int i = 0; i < M; ++i) for (int j = 0; j < i; ++j) R[i * M + j] = R[j * M + i];
    for (int a = 0; a < M; ++a) { y[a] = 2.f * nd(g); hx[a] = nd(g); sc[a] = ud(g); }
    for (unsigned pat = 1; pat + 1 < (1u << M); ++pat) {   // partly observed: the two other cases never reach this code
      int idx[M], r = 0;
      for (int a = 0; a < M; ++a) if (pat >> a & 1) idx[r++] = a;
      float Rr[M * M], yr[M], hr[M], sr[M], yg[M], hg[M], sg[M];
      for (int a = 0; a < r; ++a) {
        for (int b = 0; b < r; ++b) Rr[a * r + b] = R[idx[a] * M + idx[b]];
        yr[a] = y[idx[a]]; hr[a] = hx[idx[a]]; sr[a] = sc[idx[a]];
      }
      for (int a = 0; a < M; ++a) {
        const bool ob = pat >> a & 1;
        yg[a] = ob ? y[a] : NAN; hg[a] = ob ? hx[a] : NAN; sg[a] = ob ? sc[a] : NAN;
      }
      if (bpf_observed_bits<M>(yg) != (uint64_t)pat) { ++bad; continue; }
      float sd[bpf_density_words(M)];
      for (auto& x : sd) x = NAN;
      bpf_step_density<M>(R, pat, sd);
      // the embedded factor: observed block == compacted factor, missing rows == e_a
      float Lc[64];
      chol(Rr, r, Lc);
      int fbad = 0;
      for (int a = 0, ra = 0; a < M; ++a) {
        const bool oa = pat >> a & 1;
        for (int c = 0, rc = 0; c <= a; ++c) {
          const bool oc = pat >> c & 1;
          const float want = (oa && oc) ? Lc[ra * r + rc] : (a == c ? 1.0f : 0.0f);
          fbad += !same_bits(sd[a * (a + 1) / 2 + c], want);
          rc += oc;
        }
        ra += oa;
      }
      const float l1 = emission_loglik_masked<M>(sd, pat, hg, yg, nullptr), l2 = compact_loglik(r, Rr, yr, hr, nullptr);
      const float s1 = emission_loglik_masked<M>(sd, pat, hg, yg, sg), s2 = compact_loglik(r, Rr, yr, hr, sr);
      const int b = fbad + !same_bits(l1, l2) + !same_bits(s1, s2) + !std::isfinite(l1) + !std::isfinite(s1);
      if (b) printf("M=%d pat=%x: factor %d, loglik %.9g %.9g, scaled %.9g %.9g\n", M, pat, fbad, l1, l2, s1, s2);
      bad += b;
      *checked += 2;
    }
  }
  return bad;
}

int main() {
  std::mt19937 g(1);
  long checked = 0;
  const int bad = all<1>(g, &checked) + all<2>(g, &checked) + all<3>(g, &checked) + all<4>(g, &checked) + all<5>(g, &checked) +
                  all<6>(g, &checked) + all<7>(g, &checked) + all<8>(g, &checked);
  printf("log-densities compared: %ld\n", checked);
  printf("total mismatches: %d\n", bad);
  return bad != 0;
}
