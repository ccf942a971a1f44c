// bpf_missing: the Gaussian emission log-density of the particle filter on the OBSERVED components of a step (missing
// observations: a NaN entry y[a] means "component a was not observed"), as the MISSING = true kernels of bpf_scan.hpp,
// bpf_big.hpp and bpf_wide.hpp compute it.
//
// With o the observed components of the step, the log-weight is log N(y_o; h_o, (R_lp)_oo) in the arithmetic of
// emission_loglik (ssm_device.hpp) on the compacted problem: the Cholesky factor of (R_lp)_oo by the plain loops of
// cholesky_lower, forward substitution by fma, reciprocal diagonal, quadratic form by fma, the constant
// (-0.5 |o|) log 2 pi - sum_o canon_log(L_aa) summed over the observed a in ascending order, -0.5 quad + const as one fma.
// Two pieces:
//   * the STEP DENSITY, once per step and workgroup (the pattern is the same for every particle of a trajectory):
//     bpf_observed_bits, and for a partly observed step bpf_step_density -- the factor of R_lp EMBEDDED by the identity on the
//     missing rows and columns (loops keep their compile-time trip counts; the observed block has the compacted factor's bits,
//     since every term a missing index contributes is an exact zero, and a missing row is e_a), its reciprocal diagonal and
//     the constant, bpf_density_words(M) words that live in LDS;
//   * emission_loglik_masked, per particle, which reads them (every lane at the same address: a broadcast) and skips a missing
//     row's logarithm and its term of the quadratic form by a select on the workgroup-uniform pattern -- whatever the model
//     computed for a missing row (a NaN included) is discarded.
// The mean h(x, r_eval, u) and the stochastic-volatility scale are arguments, so this header needs nothing of the kernels
// (it also builds for the host: tests/c/bpf_missing_density.cpp compares it with the compacted arithmetic bit for bit).
// A fully observed step uses the model's own factor (the plain route's bits), a wholly missing one evaluates no density: both
// are decided by the caller (emission_loglik_missing in ssm_device.hpp).
#pragma once
#include <cstdint>
#include "bf_canon_math.hpp"

#ifndef BF_UNROLL
#define BF_UNROLL _Pragma("unroll")
#endif

namespace bf {

// words of a step density: the packed lower factor (row a at a (a + 1) / 2), the reciprocal diagonal, the constant
constexpr int bpf_density_words(int m) { return m * (m + 1) / 2 + m + 1; }

// bit a set: y[a] is observed (not NaN; +-Inf is an observation, and poisons)
template <int M>
__device__ __forceinline__ uint64_t bpf_observed_bits(const float* yv) {
  static_assert(M <= 64, "one bit per observed component");
  uint64_t obs = 0;
  BF_UNROLL for (int a = 0; a < M; ++a) obs |= (yv[a] == yv[a]) ? (1ull << a) : 0ull;
  return obs;
}
template <int M>
constexpr uint64_t bpf_all_observed() { return M == 64 ? ~0ull : ((1ull << (M % 64)) - 1ull); }

// The step density of a partly observed step into sd[0 .. bpf_density_words(M)): R (M x M, row-major) is the log-density's
// covariance.  Written in place, column by column, with the operations of cholesky_lower on the matrix that has the identity
// in the missing rows and columns.
template <int M>
__device__ __forceinline__ void bpf_step_density(const float* R, uint64_t obs, float* sd) {
#pragma clang fp contract(off)
  constexpr int RD = M * (M + 1) / 2, UNR = M <= 8 ? M : 1;   // (beyond 8 the loops stay rolled and work in sd itself)
  auto at = [](int i, int j) { return i * (i + 1) / 2 + j; };
#pragma unroll UNR
  for (int j = 0; j < M; ++j) {
    const bool oj = (obs >> j) & 1ull;
    float d = oj ? R[j * M + j] : 1.0f;
#pragma unroll UNR
    for (int k = 0; k < j; ++k) d -= sd[at(j, k)] * sd[at(j, k)];
    d = __builtin_sqrtf(d);
    sd[at(j, j)] = d;
#pragma unroll UNR
    for (int i = j + 1; i < M; ++i) {
      float s = (oj && ((obs >> i) & 1ull)) ? R[i * M + j] : 0.0f;
#pragma unroll UNR
      for (int k = 0; k < j; ++k) s -= sd[at(i, k)] * sd[at(j, k)];
      sd[at(i, j)] = s / d;
    }
  }
  float logdet = 0.f;
  int nobs = 0;
#pragma unroll UNR
  for (int a = 0; a < M; ++a) {
    const float l = sd[at(a, a)];
    sd[RD + a] = 1.0f / l;
    if ((obs >> a) & 1ull) {   // (a missing row's logarithm is skipped, not trusted to be 0)
      logdet += canon_log(l);
      ++nobs;
    }
  }
  sd[RD + M] = -0.5f * (float)nobs * 1.8378770664093453f - logdet;
}

// log N(y_o; hx_o, (R_lp)_oo) of a partly observed step from its step density; scale (or NULL): the positive diagonal the
// residual is divided by and whose logarithms join the log-determinant (the stochastic-volatility emission, observed rows only)
template <int M>
__device__ __forceinline__ float emission_loglik_masked(const float* sd, uint64_t obs, const float* hx, const float* yv, const float* scale) {
#pragma clang fp contract(off)
  constexpr int RD = M * (M + 1) / 2;
  float zz[M];
  float quad = 0.f, lsc = 0.f;
  BF_UNROLL for (int a = 0; a < M; ++a) {
    const bool ob = (obs >> a) & 1ull;
    float s = yv[a] - hx[a];
    if (scale) {
      const float d = scale[a];
      s = s / d;
      if (ob) lsc = lsc + canon_log(d);
    }
    BF_UNROLL for (int c = 0; c < a; ++c) s = __builtin_fmaf(-sd[a * (a + 1) / 2 + c], zz[c], s);
    s = s * sd[RD + a];
    zz[a] = ob ? s : 0.f;   // a missing row: its (NaN) residual goes nowhere, and the rows below see an exact zero
    quad = ob ? __builtin_fmaf(s, s, quad) : quad;
  }
  return __builtin_fmaf(-0.5f, quad, sd[RD + M]) - lsc;
}

}  // namespace bf
