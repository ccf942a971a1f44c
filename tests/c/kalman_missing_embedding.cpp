// condition_on_masked (csrc/kf_math.hpp) on every observation pattern of M <= 4 components against condition_on on the compacted
// model -- rows of H, rows and columns of D R D^T, entries of the innovation selected by hand -- bit for bit: the embedded step is
// the reduced model's arithmetic plus exact zeros.  Host build (host_shim/hip/hip_runtime.h), compiled without fused
// multiply-add contraction so that both sides round alike.  Exit status 0 = no mismatch.
#include "kf_math.hpp"
#include <cstdio>
#include <cstring>
#include <random>
using namespace bf;
template <int N, int M, int MR>
int one(std::mt19937& g, unsigned pat) {
  std::normal_distribution<float> nd;
  float H[M * N], R[M * M], P[N * N], m[N], y[M], mu[M], L[N * N];
  for (auto& x : H) x = nd(g);
  for (auto& x : L) x = nd(g);
  for (int i = 0; i < N; ++i) for (int j = 0; j < N; ++j) { float s = (i == j); for (int k = 0; k < N; ++k) s += L[i * N + k] * L[j * N + k]; P[i * N + j] = s; }
  float Lr[M * M]; for (auto& x : Lr) x = 0.3f * nd(g);
  for (int i = 0; i < M; ++i) for (int j = 0; j < M; ++j) { float s = 0.1f * (i == j); for (int k = 0; k < M; ++k) s += Lr[i * M + k] * Lr[j * M + k]; R[i * M + j] = s; }
  for (auto& x : m) x = nd(g);
  for (int a = 0; a < M; ++a) { y[a] = nd(g); mu[a] = 0; for (int i = 0; i < N; ++i) mu[a] += H[a * N + i] * m[i]; }
  int idx[M], r = 0;
  for (int a = 0; a < M; ++a) if (pat >> a & 1) idx[r++] = a;
  if (r != MR) return 0;
  float yg[M]; for (int a = 0; a < M; ++a) yg[a] = (pat >> a & 1) ? y[a] : NAN;
  float m1[N], P1[N * N]; memcpy(m1, m, sizeof m); memcpy(P1, P, sizeof P);
  float ll1 = condition_on_masked<N, M>(H, R, yg, mu, m1, P1);
  float m2[N], P2[N * N]; memcpy(m2, m, sizeof m); memcpy(P2, P, sizeof P);
  float ll2 = 0;
  if constexpr (MR > 0) {
    float Hr[MR * N], Rr[MR * MR], v[MR];
    for (int a = 0; a < MR; ++a) { for (int i = 0; i < N; ++i) Hr[a * N + i] = H[idx[a] * N + i]; for (int b = 0; b < MR; ++b) Rr[a * MR + b] = R[idx[a] * M + idx[b]]; v[a] = y[idx[a]] - mu[idx[a]]; }
    ll2 = condition_on<N, MR>(Hr, Rr, v, m2, P2);
  }
  int bad = 0;
  for (int i = 0; i < N; ++i) bad += !(m1[i] == m2[i]);
  for (int i = 0; i < N * N; ++i) bad += !(P1[i] == P2[i]);
  bad += !(ll1 == ll2);
  if (bad) printf("N=%d M=%d pat=%x: %d mismatches ll %.9g %.9g\n", N, M, pat, bad, ll1, ll2);
  return bad;
}
template <int N, int M> int all(std::mt19937& g) {
  int bad = 0;
  for (int rep = 0; rep < 200; ++rep) for (unsigned pat = 0; pat < (1u << M); ++pat) {
    bad += one<N, M, 0>(g, pat) + one<N, M, 1>(g, pat);
    if constexpr (M >= 2) bad += one<N, M, 2>(g, pat);
    if constexpr (M >= 3) bad += one<N, M, 3>(g, pat);
    if constexpr (M >= 4) bad += one<N, M, 4>(g, pat);
  }
  return bad;
}
int main() {
  std::mt19937 g(1);
  int bad = all<2, 1>(g) + all<4, 2>(g) + all<3, 3>(g) + all<8, 4>(g) + all<5, 4>(g);
  printf("total mismatches: %d\n", bad);
  return bad != 0;
}
