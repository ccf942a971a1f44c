// ffbs_pscan: parallel-in-time posterior sampler for few long trajectories (include/bayesfilt.h, bf_ffbs_sample_pscan_f32).
// Same model, streams, noise, carry and output as bf_ffbs_sample_f32 on the linear routes; time is cut into blocks of L steps
// and the blocks run on separate lanes, as in rts_pscan.hpp: the sampler's backward step is an affine map of the sample at
// t+1, so the structure is the smoother's with a smaller element (no covariance term).
//
// Inputs (the contract).  Those of bf_ffbs_sample_f32 for the linear model: the filtered m_t, P_t and either the predictions
// m-_{t+1}, P-_{t+1} at index t (RTS_LIN) or none (RTS_LIN_RECOMPUTE): then rts_linearize<N, RTS_LIN_RECOMPUTE> recomputes them
// (rts_smoother.hpp).  Constant Q.  xi_{s,t}: the noise stream, or keys[b] with element (s, t, i) at the serial kernel's index
// (s T + t) n + i of S T n values (T and S the call's), so a draw does not depend on how time was cut.
//
// Element.  With G_t and L_t as ffbs_factor forms them (ffbs_sampler.hpp: Cholesky of P-, no jitter; psdchol of Sigma_t with
// dropped zero-pivot columns), step t of sample s is x_t = G_t x_{t+1} + c_{s,t}, and the sampling element of step t is
//   E_t = G_t      g_{s,t} = c_{s,t} = m_t - G_t m-_{t+1} + L_t xi_{s,t}
// E is shared by all samples of a trajectory, g is per sample.  c_{s,t} is ffbs_reg_body's step statement applied to
// x_{t+1} = 0: no second arithmetic.
//
// Combination of an earlier span i with a later span j (associative, no solve):
//   E = E_i E_j      g = E_i g_j + g_i
// Applying a span (E, g) to the sample x at the step after its last one:   x' = E x + g
// A sample is itself the span (0, x); combining a span with it is exactly this rule and leaves E = 0.
//
// Three launches, fold, scan and emit; the scheme and the scan are pscan_common.hpp's, here as a SUFFIX scan over NB = ceil(T / L)
// with NSB = ceil(S / SPL) sample blocks of SPL samples:
//   fold   one lane per (trajectory, block, sample block).  Blocks 1 ... NB-2 walk their steps from the last backwards with
//          rts_linearize and ffbs_factor per step, folding the element of step t in front of the aggregate: E <- G_t E (from
//          E = I) and, per sample, g <- G_t g + c_{s,t}, which is the serial step statement applied to g (from g = 0).  E is
//          the same bits in every sample block; sample block 0 stores it.  The last block runs the ordinary backward-sampling
//          recursion from the call's end -- the carry x_in if one is given, else the terminal draw m + psdchol(P) xi at T-1 --
//          and stores its first-step sample as the span (0, x).  Block 0 needs no aggregate.  Workspace:
//          E[e][b NB + k] (n^2 entries), g[i][(b S + s) NB + k] (n entries).
//   scan   one workgroup per (trajectory, sample) over the spans k = NB-1 ... 1.  Every suffix ends at the terminal span, whose
//          E = 0, so it is a plain sample: per block the scan writes only start[i][(b S + s) NB + k], the sample at the first
//          step of block k, n floats.  (The samples of a trajectory repeat the E products: ALU time, no traffic beyond
//          re-reading n^2 floats per span.)
//   emit   one lane per (trajectory, block, sample block) runs the serial loop of ffbs_reg_body over its block, statement for
//          statement, from start[k+1]; the last block from the carry or the terminal draw.  It stores through the strided
//          sample view (any strides, both layouts); block 0 writes x_out.
//
// Consequences.  Inside a block the samples are the serial sampler's from that block's start.  The last block equals
// bf_ffbs_sample_f32 on the same streams and noise bit for bit, and with T <= L so does the whole call; elsewhere the two agree
// to fp32 tolerance (the block-start samples come from the combination, not from the recursion).  A sample's bits depend on
// (T, L), the route, its trajectory's streams and its own noise row -- in key mode also on (S, T) through the key's definition
// -- and on nothing else: not on B, the number of other samples, SPL, the layout, out= reuse or the workspace's earlier
// contents.  NaN and singular pivots are bf_ffbs_sample_f32's: a NaN input, or a P- that is not positive definite, at step t
// gives NaN at every step <= t of that trajectory's samples and leaves the later steps' bits alone; zero pivots of a singular
// G Q G^T are dropped columns by definition.  NaN flows only towards earlier spans: emit is sequential inside a block, a span
// is only ever applied to the sample of LATER steps, and the terminal span's E = 0 keeps every suffix a plain sample.
//
// Key mode generates element (s, t, i) twice, once in fold and once in emit (and in both for the last block): the Threefry
// work is paid double, accepted for a noise stream that never exists in memory.
//
// Registers: every per-lane array is indexed by compile-time constants only (fully unrolled loops).  Compiled SPL = 1, 2, 4;
// every instance n = 1 ... 6 builds without scratch (table in DESIGN.md, section 6j).
//
// Workspace: 4 B NB (n^2 + 2 S n) bytes -- per (trajectory, block) E (n^2 floats), per (trajectory, block, sample) g and the
// start sample (n floats each).  B S NB stays below 2^31.
//
// Block length: option "pfs_block", else ffbs_pscan.hip's default for (B, S, T) -- the largest of
// ceil(B ceil(S / 4) T / 65 536), the smallest s with 250 s^2 >= T, and 16, at most 4096 --, with the sweep behind it in
// profiles/parallel_sampler_probe.txt.
#pragma once
#include "ffbs_sampler.hpp"
#include "pscan_common.hpp"
#include "pscan_host.hpp"

namespace bf {

// a + b as one rounded addition.  The sums that close a sample's step are written as plain additions in ffbs_reg_body, and its
// instances compile them so; here the same statement sits in several kernels (fold, emit, SPL = 1, 2, 4), and without this the
// compiler is free to contract the addition into the fused chain before it in one instance and not in another, which makes a
// sample's bits depend on the instance.
__device__ __forceinline__ float pfs_add(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}

// xi_{s,t} of trajectory b: the noise stream's row, or element (s, t, .) of the key (k0, k1) = keys[b] (pfs_key)
template <int N>
__device__ __forceinline__ void pfs_noise(const FfbsViews& v, uint32_t k0, uint32_t k1, long long b, int s, long long t, int S,
                                          long long T, float* z) {
  if (v.xi.p == nullptr) {
    const uint32_t count = (uint32_t)S * (uint32_t)T * (uint32_t)N;
    const uint32_t base = ((uint32_t)s * (uint32_t)T + (uint32_t)t) * (uint32_t)N;
    BF_UNROLL for (int i = 0; i < N; ++i) z[i] = bits_to_normal(threefry_bits(k0, k1, base + i, count));
  } else {
    const float* q = v.xi.p + b * v.xi.sB + s * v.xi.sK + t * v.xi.sT;
    BF_UNROLL for (int i = 0; i < N; ++i) z[i] = q[i * v.xi.sE];
  }
}
__device__ __forceinline__ void pfs_key(const FfbsViews& v, long long b, uint32_t& k0, uint32_t& k1) {
  k0 = k1 = 0;
  if (v.xi.p == nullptr) {
    k0 = v.keys[2 * b];
    k1 = v.keys[2 * b + 1];
  }
}

// The serial recursion of the samples s0 ... s0 + SPL - 1 of trajectory b over the steps t_hi ... t_lo from the samples x at
// t_hi + 1: the step loop of ffbs_reg_body (ffbs_sampler.hpp), statement for statement, so that the values carry its bits.
// STORE: write the samples.  FOLD: also E <- G_t E, column by column.
template <int N, int SPL, int KIND, bool STORE, bool FOLD>
__device__ __forceinline__ void pfs_walk(const RtsLin<N>& c, const FfbsViews& v, long long b, int s0, int S, long long T,
                                         long long t_hi, long long t_lo, float (&x)[SPL][N], float* E) {
  constexpr int NN = N * N;
  uint32_t k0, k1;
  pfs_key(v, b, k0, k1);
  for (long long t = t_hi; t >= t_lo; --t) {
    float m[N], P[NN], mp[N], Pp[NN], X[NN], Ls[NN];
    pscan_load_step<N, KIND != RTS_LIN_RECOMPUTE>(v, b, t, m, P, mp, Pp);
    rts_linearize<N, KIND>(c, nullptr, t, 0.f, m, P, X, mp, Pp);
    ffbs_factor<N>(X, P, Pp, Ls);
    BF_UNROLL for (int j = 0; j < SPL; ++j) if (s0 + j < S) {
      float z[N], dx[N];
      pfs_noise<N>(v, k0, k1, b, s0 + j, t, S, T, z);
      BF_UNROLL for (int i = 0; i < N; ++i) dx[i] = x[j][i] - mp[i];
      BF_UNROLL for (int i = 0; i < N; ++i) {
        float s = X[i] * dx[0];
        BF_UNROLL for (int k = 1; k < N; ++k) s = fmaf(X[k * N + i], dx[k], s);
        BF_UNROLL for (int k = 0; k <= i; ++k) s = fmaf(Ls[i * N + k], z[k], s);
        x[j][i] = pfs_add(m[i], s);
      }
      if constexpr (STORE) {
        float* q = v.x.p + b * v.x.sB + (s0 + j) * v.x.sK + t * v.x.sT;
        BF_UNROLL for (int i = 0; i < N; ++i) q[i * v.x.sE] = x[j][i];
      }
    }
    if constexpr (FOLD) {   // E <- G_t E with G_t[i][k] = X[k][i]
      BF_UNROLL for (int cc = 0; cc < N; ++cc) {
        float col[N];
        BF_UNROLL for (int i = 0; i < N; ++i) {
          float s = X[i] * E[cc];
          BF_UNROLL for (int k = 1; k < N; ++k) s = fmaf(X[k * N + i], E[k * N + cc], s);
          col[i] = s;
        }
        BF_UNROLL for (int i = 0; i < N; ++i) E[i * N + cc] = col[i];
      }
    }
  }
}

// The samples the call's last block starts from: the carry (returns T-1: every step is still to do), or the terminal draw
// at T-1 as ffbs_reg_body forms it, stored when STORE (returns T-2).
template <int N, int SPL, bool STORE>
__device__ __forceinline__ long long pfs_terminal(const FfbsViews& v, long long b, int s0, int S, long long T, float (&x)[SPL][N]) {
  constexpr int NN = N * N;
  if (v.x_in) {
    BF_UNROLL for (int j = 0; j < SPL; ++j) if (s0 + j < S)
      BF_UNROLL for (int i = 0; i < N; ++i) x[j][i] = v.x_in[(b * S + s0 + j) * N + i];
    return T - 1;
  }
  const long long t = T - 1;
  uint32_t k0, k1;
  pfs_key(v, b, k0, k1);
  auto ld = [&](const SView& s, int e) { return s.p[b * s.sB + t * s.sT + e * s.sE]; };
  float m[N], Ls[NN], d[N];
  BF_UNROLL for (int i = 0; i < N; ++i) m[i] = ld(v.m, i);
  BF_UNROLL for (int i = 0; i < N; ++i) BF_UNROLL for (int j = 0; j <= i; ++j) Ls[i * N + j] = ld(v.P, i * N + j);
  BF_UNROLL for (int i = 0; i < N; ++i) d[i] = Ls[i * N + i];
  psdchol<N>(Ls, d);
  BF_UNROLL for (int j = 0; j < SPL; ++j) if (s0 + j < S) {
    float z[N];
    pfs_noise<N>(v, k0, k1, b, s0 + j, t, S, T, z);
    BF_UNROLL for (int i = 0; i < N; ++i) {
      float s = Ls[i * N] * z[0];
      BF_UNROLL for (int k = 1; k <= i; ++k) s = fmaf(Ls[i * N + k], z[k], s);
      x[j][i] = pfs_add(m[i], s);
    }
    if constexpr (STORE) {
      float* q = v.x.p + b * v.x.sB + (s0 + j) * v.x.sK + t * v.x.sT;
      BF_UNROLL for (int i = 0; i < N; ++i) q[i * v.x.sE] = x[j][i];
    }
  }
  return T - 2;
}

// ---- launch 1: fold -----------------------------------------------------------------------------------------------------
template <int N, int SPL, int KIND>
__device__ __forceinline__ void pfs_fold_body(const RtsLin<N>& c, const FfbsViews& v, float* __restrict__ wsE, float* __restrict__ wsg,
                                              long long B, long long T, int S, long long NB, int L) {
  constexpr int NN = N * N;
  const int NSB = (S + SPL - 1) / SPL;
  long long g, b, k;
  int j;
  if (!pscan_lane(B, NSB, NB, g, b, j, k)) return;
  if (k == 0) return;   // block 0 is only emitted
  const int s0 = j * SPL;
  const long long t0 = k * (long long)L;
  float x[SPL][N], E[NN];
  if (k == NB - 1) {
    // the last block: the ordinary recursion from the call's end; its first-step sample is the span (0, x)
    const long long t_hi = pfs_terminal<N, SPL, false>(v, b, s0, S, T, x);
    pfs_walk<N, SPL, KIND, false, false>(c, v, b, s0, S, T, t_hi, t0, x, nullptr);
    BF_UNROLL for (int e = 0; e < NN; ++e) E[e] = 0.f;
  } else {
    BF_UNROLL for (int i = 0; i < N; ++i) BF_UNROLL for (int q = 0; q < N; ++q) E[i * N + q] = (i == q) ? 1.f : 0.f;
    BF_UNROLL for (int q = 0; q < SPL; ++q) BF_UNROLL for (int i = 0; i < N; ++i) x[q][i] = 0.f;
    pfs_walk<N, SPL, KIND, false, true>(c, v, b, s0, S, T, t0 + L - 1, t0, x, E);
  }
  if (j == 0) pscan_col_store<NN>(wsE, B * NB, b * NB + k, E);
  BF_UNROLL for (int q = 0; q < SPL; ++q) if (s0 + q < S)
    pscan_col_store<N>(wsg, B * (long long)S * NB, (b * S + s0 + q) * NB + k, x[q]);
}

// ---- launch 2: scan (pscan_common.hpp) -----------------------------------------------------------------------------------
// E | g; E comes from the trajectory's array, g from the sample's
template <int N>
struct PfsSpan {
  static constexpr int F = N * N + N;
  float v[F];
  __device__ float* E() { return v; }           __device__ const float* E() const { return v; }
  __device__ float* g() { return v + N * N; }   __device__ const float* g() const { return v + N * N; }
};

// o = i (+) j, i the earlier span.  o may alias i or j: everything is read before the first write.
template <int N>
__device__ __forceinline__ void pfs_combine(const PfsSpan<N>& i, const PfsSpan<N>& j, PfsSpan<N>& o) {
  float oE[N * N], og[N];
  mm<N, N, N>(i.E(), j.E(), oE);
  mv<N, N>(i.E(), j.g(), og);
  BF_UNROLL for (int e = 0; e < N; ++e) o.g()[e] = og[e] + i.g()[e];
  BF_UNROLL for (int e = 0; e < N * N; ++e) o.E()[e] = oE[e];
}

// x <- the span s applied to the sample x
template <int N>
__device__ __forceinline__ void pfs_apply(const PfsSpan<N>& s, float* x) {
  float ox[N];
  mv<N, N>(s.E(), x, ox);
  BF_UNROLL for (int e = 0; e < N; ++e) x[e] = ox[e] + s.g()[e];
}

// Span NB-1 has E = 0 and maps any finite x to g exactly.  finish: the state is the sample at the first step of block k.
template <int N>
struct PfsScan {
  using Span = PfsSpan<N>;
  static constexpr int STATE = N;
  static constexpr int DIM = N;
  static constexpr bool SUFFIX = true;
  struct Args {
    const float* __restrict__ wsE;
    const float* __restrict__ wsg;
    float* __restrict__ start;
    long long colE, strideE, colg, strideg;   // b NB, B NB; (b S + s) NB, B S NB
  };
  static __device__ __forceinline__ void load(const Args& a, long long k, Span& s) {
    pscan_col_load<N * N>(a.wsE, a.strideE, a.colE + k, s.E());
    pscan_col_load<N>(a.wsg, a.strideg, a.colg + k, s.g());
  }
  static __device__ __forceinline__ void combine(const Span& i, const Span& j, Span& o) { pfs_combine<N>(i, j, o); }
  static __device__ __forceinline__ void apply(const Span& s, float* x) { pfs_apply<N>(s, x); }
  static __device__ __forceinline__ void finish(const Args& a, long long k, float* x) {
    pscan_col_store<N>(a.start, a.strideg, a.colg + k, x);
  }
};

// ---- launch 3: emit -----------------------------------------------------------------------------------------------------
template <int N, int SPL, int KIND>
__device__ __forceinline__ void pfs_emit_body(const RtsLin<N>& c, const FfbsViews& v, const float* __restrict__ start, long long B,
                                              long long T, int S, long long NB, int L) {
  const int NSB = (S + SPL - 1) / SPL;
  long long g, b, k;
  int j;
  if (!pscan_lane(B, NSB, NB, g, b, j, k)) return;
  const int s0 = j * SPL;
  const long long t0 = k * (long long)L;
  float x[SPL][N];
  long long t_hi;
  if (k == NB - 1) {
    t_hi = pfs_terminal<N, SPL, true>(v, b, s0, S, T, x);
  } else {
    BF_UNROLL for (int q = 0; q < SPL; ++q) if (s0 + q < S)   // start[k + 1] of the same sample
      pscan_col_load<N>(start, B * (long long)S * NB, (b * S + s0 + q) * NB + k + 1, x[q]);
    t_hi = t0 + L - 1;
  }
  pfs_walk<N, SPL, KIND, true, false>(c, v, b, s0, S, T, t_hi, t0, x, nullptr);
  if (k == 0 && v.x_out) {
    BF_UNROLL for (int q = 0; q < SPL; ++q) if (s0 + q < S)
      BF_UNROLL for (int i = 0; i < N; ++i) v.x_out[(b * S + s0 + q) * N + i] = x[q][i];
  }
}

template <int N, int SPL, int KIND>
__global__ void __launch_bounds__(64) ffbs_pscan_fold_kernel(RtsLin<N> c, FfbsViews v, float* wsE, float* wsg, long long B, long long T,
                                                             int S, long long NB, int L) {
  pfs_fold_body<N, SPL, KIND>(c, v, wsE, wsg, B, T, S, NB, L);
}
template <int N>   // one workgroup per (trajectory, sample)
__global__ void __launch_bounds__(256) ffbs_pscan_scan_kernel(const float* wsE, const float* wsg, float* start, long long B, int S,
                                                              long long NB) {
  __shared__ float lds[pscan_lds_floats<PfsScan<N>>()];
  const long long bs = blockIdx.x;   // b S + s
  pscan_scan<PfsScan<N>>({wsE, wsg, start, bs / S * NB, B * NB, bs * NB, B * (long long)S * NB}, NB, lds);
}
template <int N, int SPL, int KIND>
__global__ void __launch_bounds__(64) ffbs_pscan_emit_kernel(RtsLin<N> c, FfbsViews v, const float* start, long long B, long long T,
                                                             int S, long long NB, int L) {
  pfs_emit_body<N, SPL, KIND>(c, v, start, B, T, S, NB, L);
}

// ---- host: the three launches ---------------------------------------------------------------------------------------------
template <int N, int SPL, int KIND>
static inline int launch_ffbs_pscan_spl(const RtsLin<N>& c, const FfbsViews& v, long long B, long long T, int S, float* workspace,
                                        int L, hipStream_t stream) {
  const PscanGeom g = pscan_geom(B, (S + SPL - 1) / SPL, T, L);   // lanes <= B S NB
  float* wsE = workspace;
  float* wsg = wsE + B * g.NB * N * N;
  float* start = wsg + B * S * g.NB * N;
  if (g.NB > 1) {
    hipLaunchKernelGGL((ffbs_pscan_fold_kernel<N, SPL, KIND>), dim3(g.grid), dim3(64), 0, stream, c, v, wsE, wsg, B, T, S, g.NB, L);
    hipLaunchKernelGGL((ffbs_pscan_scan_kernel<N>), dim3((unsigned)(B * S)), dim3(g.scan_threads), 0, stream, (const float*)wsE,
                       (const float*)wsg, start, B, S, g.NB);
  }
  hipLaunchKernelGGL((ffbs_pscan_emit_kernel<N, SPL, KIND>), dim3(g.grid), dim3(64), 0, stream, c, v, (const float*)start, B, T, S, g.NB, L);
  BF_HIP_CHECK(hipGetLastError());
  return BF_OK;
}

template <int N, int KIND>
static inline int launch_ffbs_pscan_n(const RtsLin<N>& c, const FfbsViews& v, long long B, long long T, int S, int spl,
                                      float* workspace, int L, hipStream_t stream) {
  switch (spl) {
    case 1: return launch_ffbs_pscan_spl<N, 1, KIND>(c, v, B, T, S, workspace, L, stream);
    case 2: return launch_ffbs_pscan_spl<N, 2, KIND>(c, v, B, T, S, workspace, L, stream);
    default: return launch_ffbs_pscan_spl<N, 4, KIND>(c, v, B, T, S, workspace, L, stream);
  }
}

}  // namespace bf
