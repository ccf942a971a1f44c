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
// Three launches, no waiting between workgroups of any kind (no look-back, no flags, no grid synchronisation); NB = ceil(T / L),
// NSB = ceil(S / SPL) sample blocks of SPL samples:
//   fold   one lane per (trajectory, block, sample block).  Blocks 1 ... NB-2 walk their steps from the last backwards with
//          rts_linearize and ffbs_factor per step, folding the element of step t in front of the aggregate: E <- G_t E (from
//          E = I) and, per sample, g <- G_t g + c_{s,t}, which is the serial step statement applied to g (from g = 0).  E is
//          the same bits in every sample block; sample block 0 stores it.  The last block runs the ordinary backward-sampling
//          recursion from the call's end -- the carry x_in if one is given, else the terminal draw m + psdchol(P) xi at T-1 --
//          and stores its first-step sample as the span (0, x).  Block 0 needs no aggregate.  Workspace, element index
//          outermost so that the lanes of a wave store (and the scan loads) consecutive addresses:
//          E[e][b NB + k] (n^2 entries), g[i][(b S + s) NB + k] (n entries).
//   scan   one workgroup per (trajectory, sample) runs a suffix scan over the spans k = NB-1 ... 1, in tiles of one span per
//          thread (64 threads up to 65 blocks, else 256), thread r of a tile holding span NB-1-r: on these reversed indices
//          the suffix scan is an inclusive scan by __shfl_up (wave64, six combinations), wave totals through LDS, the running
//          sample from tile to tile through LDS.  Every suffix ends at the terminal span, whose E = 0, so it is a plain
//          sample: per block the scan writes only start[i][(b S + s) NB + k], the sample at the first step of block k, n floats.
//          (The samples of a trajectory repeat the E products: ALU time, no traffic beyond re-reading n^2 floats per span.)
//   emit   one lane per (trajectory, block, sample block) runs the serial loop of ffbs_reg_body over its block, statement for
//          statement, from start[k+1]; the last block from the carry or the terminal draw.  It stores through the strided
//          sample view (any strides, both layouts); block 0 writes x_out.
// NB = 1 is the emit launch alone.
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
// Block length: option "pfs_block", else ffbs_pscan_default_block(B, S, T) in ffbs_pscan.hip -- the largest of
// ceil(B ceil(S / 4) T / 65 536), the smallest s with 250 s^2 >= T, and 16, at most 4096 --, with the sweep behind it in
// profiles/parallel_sampler_probe.txt.
#pragma once
#include "ffbs_sampler.hpp"

namespace bf {

// a + b as one rounded addition.  The sums that close a sample's step are written as plain additions in ffbs_reg_body, and its
// instances compile them so; here the same statement sits in several kernels (fold, emit, SPL = 1, 2, 4), and without this the
// compiler is free to contract the addition into the fused chain before it in one instance and not in another, which makes a
// sample's bits depend on the instance.
__device__ __forceinline__ float pfs_add(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}

// The serial recursion of the samples s0 ... s0 + SPL - 1 of trajectory b over the steps t_hi ... t_lo from the samples x at
// t_hi + 1: the step loop of ffbs_reg_body (ffbs_sampler.hpp), statement for statement, so that the values carry its bits.
// STORE: write the samples.  FOLD: also E <- G_t E, column by column.
template <int N, int SPL, int KIND, bool STORE, bool FOLD>
__device__ __forceinline__ void pfs_walk(const RtsLin<N>& c, const FfbsViews& v, long long b, int s0, int S, long long T,
                                         long long t_hi, long long t_lo, float (&x)[SPL][N], float* E) {
  constexpr int NN = N * N;
  const bool keyed = v.xi.p == nullptr;
  uint32_t k0 = 0, k1 = 0;
  if (keyed) {
    k0 = v.keys[2 * b];
    k1 = v.keys[2 * b + 1];
  }
  const uint32_t count = (uint32_t)S * (uint32_t)T * (uint32_t)N;
  auto ld = [&](const SView& s, long long t, int e) { return s.p[b * s.sB + t * s.sT + e * s.sE]; };
  auto noise = [&](int s, long long t, float* z) __attribute__((always_inline)) {
    if (keyed) {
      const uint32_t base = ((uint32_t)s * (uint32_t)T + (uint32_t)t) * (uint32_t)N;
      BF_UNROLL for (int i = 0; i < N; ++i) z[i] = bits_to_normal(threefry_bits(k0, k1, base + i, count));
    } else {
      const float* q = v.xi.p + b * v.xi.sB + s * v.xi.sK + t * v.xi.sT;
      BF_UNROLL for (int i = 0; i < N; ++i) z[i] = q[i * v.xi.sE];
    }
  };
  for (long long t = t_hi; t >= t_lo; --t) {
    float m[N], P[NN], mp[N], Pp[NN], X[NN], Ls[NN];
    BF_UNROLL for (int i = 0; i < N; ++i) m[i] = ld(v.m, t, i);
    BF_UNROLL for (int i = 0; i < NN; ++i) P[i] = ld(v.P, t, i);
    if constexpr (KIND != RTS_LIN_RECOMPUTE) {
      BF_UNROLL for (int i = 0; i < N; ++i) mp[i] = ld(v.pm, t, i);
      BF_UNROLL for (int i = 0; i < NN; ++i) Pp[i] = ld(v.pP, t, i);
    }
    rts_linearize<N, KIND>(c, nullptr, t, 0.f, m, P, X, mp, Pp);
    ffbs_factor<N>(X, P, Pp, Ls);
    BF_UNROLL for (int j = 0; j < SPL; ++j) if (s0 + j < S) {
      float z[N], dx[N];
      noise(s0 + j, t, z);
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
  const bool keyed = v.xi.p == nullptr;
  const uint32_t count = (uint32_t)S * (uint32_t)T * (uint32_t)N;
  auto ld = [&](const SView& s, int e) { return s.p[b * s.sB + t * s.sT + e * s.sE]; };
  float m[N], Ls[NN], d[N];
  BF_UNROLL for (int i = 0; i < N; ++i) m[i] = ld(v.m, i);
  BF_UNROLL for (int i = 0; i < N; ++i) BF_UNROLL for (int j = 0; j <= i; ++j) Ls[i * N + j] = ld(v.P, i * N + j);
  BF_UNROLL for (int i = 0; i < N; ++i) d[i] = Ls[i * N + i];
  psdchol<N>(Ls, d);
  BF_UNROLL for (int j = 0; j < SPL; ++j) if (s0 + j < S) {
    float z[N];
    if (keyed) {
      const uint32_t base = ((uint32_t)(s0 + j) * (uint32_t)T + (uint32_t)t) * (uint32_t)N;
      BF_UNROLL for (int i = 0; i < N; ++i) z[i] = bits_to_normal(threefry_bits(v.keys[2 * b], v.keys[2 * b + 1], base + i, count));
    } else {
      const float* q = v.xi.p + b * v.xi.sB + (s0 + j) * v.xi.sK + t * v.xi.sT;
      BF_UNROLL for (int i = 0; i < N; ++i) z[i] = q[i * v.xi.sE];
    }
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

// lane -> (trajectory b, sample block j, time block k), k innermost; false past the end
__device__ __forceinline__ bool pfs_lane(long long B, long long NB, int NSB, long long& b, int& j, long long& k) {
  const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= B * NSB * NB) return false;
  k = g % NB;
  const long long bj = g / NB;
  j = (int)(bj % NSB);
  b = bj / NSB;
  return true;
}

// ---- launch 1: fold -----------------------------------------------------------------------------------------------------
template <int N, int SPL, int KIND>
__device__ __forceinline__ void pfs_fold_body(const RtsLin<N>& c, const FfbsViews& v, float* __restrict__ wsE, float* __restrict__ wsg,
                                              long long B, long long T, int S, long long NB, int L) {
  constexpr int NN = N * N;
  const int NSB = (S + SPL - 1) / SPL;
  long long b, k;
  int j;
  if (!pfs_lane(B, NB, NSB, b, j, k)) return;
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
  if (j == 0) {
    float* p = wsE + b * NB + k;
    const long long stride = B * NB;
    BF_UNROLL for (int e = 0; e < NN; ++e) p[(long long)e * stride] = E[e];
  }
  const long long stride = B * (long long)S * NB;
  BF_UNROLL for (int q = 0; q < SPL; ++q) if (s0 + q < S) {
    float* p = wsg + (b * S + s0 + q) * NB + k;
    BF_UNROLL for (int i = 0; i < N; ++i) p[(long long)i * stride] = x[q][i];
  }
}

// ---- launch 2: scan -----------------------------------------------------------------------------------------------------
template <int N>
struct PfsSpan {
  float E[N * N], g[N];
};

// o = i (+) j, i the earlier span.  o may alias i or j: everything is read before the first write.
template <int N>
__device__ __forceinline__ void pfs_combine(const PfsSpan<N>& i, const PfsSpan<N>& j, PfsSpan<N>& o) {
  float oE[N * N], og[N];
  mm<N, N, N>(i.E, j.E, oE);
  mv<N, N>(i.E, j.g, og);
  BF_UNROLL for (int e = 0; e < N; ++e) o.g[e] = og[e] + i.g[e];
  BF_UNROLL for (int e = 0; e < N * N; ++e) o.E[e] = oE[e];
}

// x <- the span s applied to the sample x
template <int N>
__device__ __forceinline__ void pfs_apply(const PfsSpan<N>& s, float* x) {
  float ox[N];
  mv<N, N>(s.E, x, ox);
  BF_UNROLL for (int e = 0; e < N; ++e) x[e] = ox[e] + s.g[e];
}

// One workgroup (blockDim.x = 64 or 256) per (trajectory, sample).  lds: four wave totals and the running sample.
template <int N>
constexpr int pfs_scan_lds_floats() { return 4 * (N * N + N) + N; }

template <int N>
__device__ __forceinline__ void pfs_scan_body(const float* __restrict__ wsE, const float* __restrict__ wsg, float* __restrict__ start,
                                              long long B, int S, long long NB, float* lds) {
  constexpr int NN = N * N, SPAN = NN + N;
  const long long bs = blockIdx.x;   // b S + s
  const long long b = bs / S;
  const long long strideE = B * NB, strideg = B * (long long)S * NB;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  float* tot = lds;              // [4][SPAN]: the waves' totals of this tile
  float* run = lds + 4 * SPAN;   // the sample at the first step of the previous tile's earliest block
  const long long nspan = NB - 1;   // spans k = NB-1 ... 1 at the reversed indices r = NB-1-k = 0 ... NB-2
  // after the first span there is no sample; span NB-1 has E = 0 and maps any finite x to g exactly
  float gx[N];
  BF_UNROLL for (int i = 0; i < N; ++i) gx[i] = 0.f;

  for (long long base = 0; base < nspan; base += blockDim.x) {
    const long long r = base + tid;
    const bool valid = r < nspan;
    const long long k = valid ? NB - 1 - r : 1;
    PfsSpan<N> s;
    {
      const float* pE = wsE + b * NB + k;
      const float* pg = wsg + bs * NB + k;
      BF_UNROLL for (int e = 0; e < NN; ++e) s.E[e] = pE[(long long)e * strideE];
      BF_UNROLL for (int e = 0; e < N; ++e) s.g[e] = pg[(long long)e * strideg];
    }
    if (!valid) {   // the identity span
      BF_UNROLL for (int i = 0; i < N; ++i) BF_UNROLL for (int q = 0; q < N; ++q) s.E[i * N + q] = (i == q) ? 1.f : 0.f;
      BF_UNROLL for (int i = 0; i < N; ++i) s.g[i] = 0.f;
    }
    // inclusive scan of the wave's 64 spans: thread r ends with span_k (+) span_{k+1} (+) ... up to the wave's first
#pragma unroll 1
    for (int off = 1; off < 64; off <<= 1) {
      PfsSpan<N> p, q;
      BF_UNROLL for (int e = 0; e < NN; ++e) p.E[e] = __shfl_up(s.E[e], off, 64);   // the spans of LATER blocks
      BF_UNROLL for (int e = 0; e < N; ++e) p.g[e] = __shfl_up(s.g[e], off, 64);
      pfs_combine<N>(s, p, q);
      const bool take = lane >= off;
      BF_UNROLL for (int e = 0; e < NN; ++e) s.E[e] = take ? q.E[e] : s.E[e];
      BF_UNROLL for (int e = 0; e < N; ++e) s.g[e] = take ? q.g[e] : s.g[e];
    }
    if (lane == 63) {
      BF_UNROLL for (int e = 0; e < NN; ++e) tot[wave * SPAN + e] = s.E[e];
      BF_UNROLL for (int e = 0; e < N; ++e) tot[wave * SPAN + NN + e] = s.g[e];
    }
    __syncthreads();
    // the sample behind this wave: the running sample through the totals of the waves before it
    float x[N];
    BF_UNROLL for (int i = 0; i < N; ++i) x[i] = gx[i];
#pragma unroll 1
    for (int w = 0; w < wave; ++w) {
      PfsSpan<N> tw;
      BF_UNROLL for (int e = 0; e < NN; ++e) tw.E[e] = tot[w * SPAN + e];
      BF_UNROLL for (int e = 0; e < N; ++e) tw.g[e] = tot[w * SPAN + NN + e];
      pfs_apply<N>(tw, x);
    }
    pfs_apply<N>(s, x);   // the sample at the first step of block k
    __syncthreads();
    if (tid == (int)blockDim.x - 1) BF_UNROLL for (int i = 0; i < N; ++i) run[i] = x[i];
    if (valid) {
      float* p = start + bs * NB + k;
      BF_UNROLL for (int i = 0; i < N; ++i) p[(long long)i * strideg] = x[i];
    }
    __syncthreads();
    BF_UNROLL for (int i = 0; i < N; ++i) gx[i] = run[i];
  }
}

// ---- launch 3: emit -----------------------------------------------------------------------------------------------------
template <int N, int SPL, int KIND>
__device__ __forceinline__ void pfs_emit_body(const RtsLin<N>& c, const FfbsViews& v, const float* __restrict__ start, long long B,
                                              long long T, int S, long long NB, int L) {
  const int NSB = (S + SPL - 1) / SPL;
  long long b, k;
  int j;
  if (!pfs_lane(B, NB, NSB, b, j, k)) return;
  const int s0 = j * SPL;
  const long long t0 = k * (long long)L;
  float x[SPL][N];
  long long t_hi;
  if (k == NB - 1) {
    t_hi = pfs_terminal<N, SPL, true>(v, b, s0, S, T, x);
  } else {
    const long long stride = B * (long long)S * NB;
    BF_UNROLL for (int q = 0; q < SPL; ++q) if (s0 + q < S) {
      const float* p = start + (b * S + s0 + q) * NB + k + 1;   // start[k + 1] of the same sample
      BF_UNROLL for (int i = 0; i < N; ++i) x[q][i] = p[(long long)i * stride];
    }
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
template <int N>
__global__ void __launch_bounds__(256) ffbs_pscan_scan_kernel(const float* wsE, const float* wsg, float* start, long long B, int S,
                                                              long long NB) {
  __shared__ float lds[pfs_scan_lds_floats<N>()];
  pfs_scan_body<N>(wsE, wsg, start, B, S, NB, lds);
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
  const long long NB = (T + L - 1) / L;
  const long long NSB = (S + SPL - 1) / SPL;
  const long long lanes = B * NSB * NB;   // <= B S NB < 2^31 (ffbs_pscan.hip)
  float* wsE = workspace;
  float* wsg = wsE + B * NB * N * N;
  float* start = wsg + B * S * NB * N;
  const unsigned grid = (unsigned)((lanes + 63) / 64);
  if (NB > 1) {
    hipLaunchKernelGGL((ffbs_pscan_fold_kernel<N, SPL, KIND>), dim3(grid), dim3(64), 0, stream, c, v, wsE, wsg, B, T, S, NB, L);
    hipLaunchKernelGGL((ffbs_pscan_scan_kernel<N>), dim3((unsigned)(B * S)), dim3(NB - 1 <= 64 ? 64 : 256), 0, stream,
                       (const float*)wsE, (const float*)wsg, start, B, S, NB);
  }
  hipLaunchKernelGGL((ffbs_pscan_emit_kernel<N, SPL, KIND>), dim3(grid), dim3(64), 0, stream, c, v, (const float*)start, B, T, S, NB, L);
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
