// The constant part of the parallel-in-time Kalman filter's step element (kf_pscan.hpp) for one observation pattern: host
// arithmetic in float64 on the fp32 model terms, no HIP dependence (tests/c/pscan_pattern_elements.cpp builds it with a plain
// C++ compiler).
//
// With o the observed rows of a step (bit a of `pattern` set = component a observed), S_o = H_o Qb H_o^T + Rb_oo,
//   K_o = Qb H_o^T S_o^-1     W_o = A^T H_o^T S_o^-1
//   A_e = (I - K_o H_o) A     C_e = (I - K_o H_o) Qb     J_e = W_o H_o A
// and K, W are stored n x m with zero columns for the missing components.  o empty: (A, Qb, 0) and K = W = 0.
//
// The reduced model is EMBEDDED in the m x m system, as the device step does (kf_math.hpp): the missing rows of H Qb and H A
// are zero and the missing rows and columns of S are those of the identity.  Gauss-Jordan with partial pivoting then meets
// zeros below and beside a missing diagonal 1, picks the reduced system's pivots inside the observed block and eliminates
// against a missing row with multiplier 0: the reduced arithmetic plus exact zeros.  With every bit set no select fires and
// the operations are those of the unmasked element.  Every S_o is a principal submatrix of S; each is still checked.
#pragma once
#include <cmath>
#include <utility>

namespace bf {

// A_e | C_e | J_e | K | W: one pattern's entry of the table the fold kernel stages into LDS
template <int N, int M>
struct PsPattern {
  static constexpr int F = 3 * N * N + 2 * N * M;
  float Ae[N * N], Ce[N * N], Je[N * N];
  float K[N * M];   // b_e = u + K v
  float W[N * M];   // eta_e = W v
};
template <int N, int M>
struct PsPatternTable {
  PsPattern<N, M> p[1 << M];   // indexed by the pattern's bit mask; 9 984 bytes at (6, 4)
};
static_assert(sizeof(PsPattern<6, 4>) == 4 * PsPattern<6, 4>::F && sizeof(PsPatternTable<6, 4>) == 9984, "packed floats");

// A [N x N], H [M x N], Qb = G Q G^T [N x N], Rb = D R D^T [M x M]: the fp32 terms of the ordinary step.  Symmetrises C_e and
// J_e and rounds to fp32.  false: S_o is singular or an entry is not finite.
template <int N, int M>
inline bool ps_pattern_element(const float* Af, const float* Hf, const float* Qbf, const float* Rbf, unsigned pattern,
                               PsPattern<N, M>& out) {
  bool obs[M];
  for (int a = 0; a < M; ++a) obs[a] = (pattern >> a) & 1u;
  double A[N * N], H[M * N], Qb[N * N], S[M * M], Si[M * M], HQ[M * N];
  for (int i = 0; i < N * N; ++i) { A[i] = Af[i]; Qb[i] = Qbf[i]; }
  for (int i = 0; i < M * N; ++i) H[i] = Hf[i];
  for (int a = 0; a < M; ++a)
    for (int j = 0; j < N; ++j) {
      double q = 0;
      for (int i = 0; i < N; ++i) q += H[a * N + i] * Qb[i * N + j];
      HQ[a * N + j] = obs[a] ? q : 0.0;
    }
  for (int a = 0; a < M; ++a)
    for (int e = 0; e < M; ++e) {
      double s = Rbf[a * M + e];
      for (int j = 0; j < N; ++j) s += HQ[a * N + j] * H[e * N + j];
      S[a * M + e] = (obs[a] && obs[e]) ? s : (a == e ? 1.0 : 0.0);
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
      HA[a * N + j] = obs[a] ? s : 0.0;
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
      out.Ae[i * N + j] = (float)Ae[i * N + j];
      out.Ce[i * N + j] = (float)(0.5 * (Ce[i * N + j] + Ce[j * N + i]));
      out.Je[i * N + j] = (float)(0.5 * (Je[i * N + j] + Je[j * N + i]));
    }
  for (int i = 0; i < N * M; ++i) { out.K[i] = (float)K[i]; out.W[i] = (float)W[i]; }
  bool finite = true;
  for (int i = 0; i < N * N; ++i) finite = finite && std::isfinite(out.Ae[i]) && std::isfinite(out.Ce[i]) && std::isfinite(out.Je[i]);
  return finite;
}

// every pattern's entry; false at the first singular S_o
template <int N, int M>
inline bool ps_pattern_table(const float* A, const float* H, const float* Qb, const float* Rb, PsPatternTable<N, M>& t) {
  for (unsigned p = 0; p < (1u << M); ++p)
    if (!ps_pattern_element<N, M>(A, H, Qb, Rb, p, t.p[p])) return false;
  return true;
}

}  // namespace bf
