// rts_pscan: parallel-in-time RTS smoother for few long trajectories (include/bayesfilt.h, bf_rts_smoother_pscan_f32).
// Same model, streams, carry and outputs as bf_rts_smoother_f32 on the linear routes; time is cut into blocks of L steps and
// the blocks run on separate lanes (Sarkka & Garcia-Fernandez, "Temporal parallelization of Bayesian smoothers", IEEE TAC
// 2021 -- the paper kf_pscan.hpp cites; this is its smoothing half, whose elements need no solve to combine).
//
// Inputs (the contract).  Those of bf_rts_smoother_f32 for the linear model: the filtered m_t, P_t and either the predictions
// m-_{t+1}, P-_{t+1} at index t (RTS_LIN) or none (RTS_LIN_RECOMPUTE): then they are recomputed as m- = A m + G q0,
// P- = A P A^T + G Q G^T by rts_linearize<N, RTS_LIN_RECOMPUTE> (rts_smoother.hpp).  Constant Q.
//
// Element.  One backward step is an affine map of the smoothed state at t+1.  With G_t = ((P-_{t+1})^-1 A P_t)^T as rts_step
// forms it (Cholesky of P-, no jitter), the smoothing element of step t is
//   E_t = G_t      g_t = m_t - G_t m-_{t+1}      L_t = P_t - G_t P-_{t+1} G_t^T   (symmetrised)
// It is rts_step applied to the zero state (m^s_{t+1} = 0, P^s_{t+1} = 0), which leaves G_t^T in X: no second arithmetic.
//
// Combination of an earlier span i with a later span j (associative, no solve):
//   E = E_i E_j      g = E_i g_j + g_i      L = E_i L_j E_i^T + L_i   (symmetrised)
//
// Applying a span (E, g, L) to the smoothed state (m, P) at the step after its last one:
//   m' = E m + g     P' = E P E^T + L   (symmetrised)
// A smoothed state is itself the span (0, m, P); combining a span with it is exactly this rule and leaves E = 0.
//
// Three launches, fold, scan and emit; the scheme and the scan are pscan_common.hpp's, here as a SUFFIX scan over NB = ceil(T / L):
//   fold   blocks 1 ... NB-2 build their L elements and fold them (from the block's last step backwards) into the block
//          aggregate of 2 n^2 + n floats; the last block runs the ordinary backward recursion from the call's end -- the carry if
//          one is given, else m^s = m, P^s = P at T-1 -- and stores its smoothed first-step state as the span (0, m^s, P^s);
//          block 0 needs no aggregate.  Workspace: span[e][b NB + k].
//   scan   one workgroup per trajectory over the spans k = NB-1 ... 1.  Every suffix ends at the terminal span, so it is a
//          plain Gaussian: per block the scan writes only start[e][b NB + k], the smoothed state at the first step of block k,
//          n + n^2 floats.
//   emit   the ordinary rts_linearize / rts_step of rts_smoother.hpp backwards over the block.  The carry-in is start[k+1] for
//          inner blocks and the call's carry, or none, for the last block.  It stores m^s, P^s and, when asked,
//          C_t = G_t P^s_{t+1} through the strided views (any strides, both layouts); block 0 writes the carry-out.
//
// Consequences.  Inside a block the outputs are the ordinary smoother's from that block's carry.  The last block equals
// bf_rts_smoother_f32 on the same streams bit for bit, and with T <= L so does the whole call; elsewhere the two agree to fp32
// tolerance (the block-start states come from the combination, not from the recursion).  A trajectory's bits depend on (T, L)
// and the route (predictions given or recomputed) and on nothing else: not on B, the layout, whether cross-covariances are
// stored, out= reuse or the workspace's earlier contents.  NaN handling is that of bf_rts_smoother_f32: a NaN input, or a P-
// that is not positive definite, at step t gives NaN in every output that reads it at every step <= t of that trajectory and
// leaves the steps after t as they were (a NaN filtered mean never reaches a covariance: neither recursion reads means for
// them).  NaN flows only towards earlier spans: emit is sequential inside a block, a span is only ever applied to the state
// of LATER steps, and the terminal span's E = 0 keeps every suffix a plain Gaussian, so no 0 * NaN reaches a later block.
//
// Registers: every per-lane array is indexed by compile-time constants only (fully unrolled loops).  A combination holds
// three spans of 2 n^2 + n floats: no scratch up to n = 6, the parallel filter's limit (table in DESIGN.md, section 6i).
//
// Block length: option "prs_block", else kf_pscan_default_block(B, T) -- the parallel filter's rule (the
// largest of ceil(B T / 65 536), the smallest s with 50 s^2 >= T, and 16; at most 4096), with the sweep behind it in
// profiles/parallel_smoother_probe.txt.
#pragma once
#include "rts_smoother.hpp"
#include "pscan_common.hpp"
#include "pscan_host.hpp"

namespace bf {

// E | g | L, the workspace's entry order
template <int N>
struct PrsSpan {
  static constexpr int F = 2 * N * N + N;
  float v[F];
  __device__ float* E() { return v; }               __device__ const float* E() const { return v; }
  __device__ float* g() { return v + N * N; }       __device__ const float* g() const { return v + N * N; }
  __device__ float* L() { return v + N * N + N; }   __device__ const float* L() const { return v + N * N + N; }
};
// a block-start state: m | P
constexpr int prs_state_floats(int n) { return n + n * n; }

// o = i (+) j, i the earlier span.  o may alias i or j: everything is read before the first write.
template <int N>
__device__ __forceinline__ void prs_combine(const PrsSpan<N>& i, const PrsSpan<N>& j, PrsSpan<N>& o) {
  float oE[N * N], og[N], oL[N * N], T1[N * N];
  mm<N, N, N>(i.E(), j.E(), oE);
  mv<N, N>(i.E(), j.g(), og);
  mm<N, N, N>(i.E(), j.L(), T1);
  mm_nt<N, N, N>(T1, i.E(), oL);
  BF_UNROLL for (int e = 0; e < N; ++e) og[e] += i.g()[e];
  BF_UNROLL for (int e = 0; e < N * N; ++e) oL[e] += i.L()[e];
  symmetrise<N>(oL);
  BF_UNROLL for (int e = 0; e < N * N; ++e) { o.E()[e] = oE[e]; o.L()[e] = oL[e]; }
  BF_UNROLL for (int e = 0; e < N; ++e) o.g()[e] = og[e];
}

// x = (m | P) <- the span s applied to the smoothed state x
template <int N>
__device__ __forceinline__ void prs_apply(const PrsSpan<N>& s, float* x) {
  float *m = x, *P = x + N;
  float om[N], T1[N * N];
  mv<N, N>(s.E(), m, om);
  mm<N, N, N>(s.E(), P, T1);
  mm_nt<N, N, N>(T1, s.E(), P);
  BF_UNROLL for (int e = 0; e < N; ++e) m[e] = om[e] + s.g()[e];
  BF_UNROLL for (int e = 0; e < N * N; ++e) P[e] += s.L()[e];
  symmetrise<N>(P);
}

// The ordinary backward recursion of trajectory b over the steps t_hi ... t_lo from the smoothed state (ms, Ps) at t_hi + 1:
// rts_reg_body's strided loop (rts_smoother.hpp), statement for statement, so that the stored values carry its bits.
template <int N, int KIND, bool STORE>
__device__ __forceinline__ void prs_walk(const RtsLin<N>& c, const RtsViews& v, long long b, long long t_hi, long long t_lo,
                                         bool want_c, float* ms, float* Ps) {
  constexpr int NN = N * N;
  auto st = [&](const SView& s, long long t, int e, float x) { s.p[b * s.sB + t * s.sT + e * s.sE] = x; };
  for (long long t = t_hi; t >= t_lo; --t) {
    float m[N], P[NN], mp[N], Pp[NN], X[NN], C[NN];
    pscan_load_step<N, KIND != RTS_LIN_RECOMPUTE>(v, b, t, m, P, mp, Pp);
    rts_linearize<N, KIND>(c, nullptr, t, 0.f, m, P, X, mp, Pp);
    rts_step<N>(X, P, m, mp, Pp, ms, Ps, C, STORE && want_c);
    if constexpr (STORE) {
      BF_UNROLL for (int i = 0; i < N; ++i) st(v.ms, t, i, ms[i]);
      BF_UNROLL for (int i = 0; i < NN; ++i) st(v.Ps, t, i, Ps[i]);
      if (want_c) BF_UNROLL for (int i = 0; i < NN; ++i) st(v.Cs, t, i, C[i]);
    }
  }
}

// The smoothed state the call's last block starts from: the carry (returns T-1: every step is still to do), or the filtered
// state at T-1, stored as the smoothed one when STORE (returns T-2).
template <int N, bool STORE>
__device__ __forceinline__ long long prs_terminal(const RtsViews& v, long long b, long long T, float* ms, float* Ps) {
  constexpr int NN = N * N;
  if (v.m_in != nullptr) {
    BF_UNROLL for (int i = 0; i < N; ++i) ms[i] = v.m_in[b * N + i];
    BF_UNROLL for (int i = 0; i < NN; ++i) Ps[i] = v.P_in[b * NN + i];
    return T - 1;
  }
  const long long t = T - 1;
  BF_UNROLL for (int i = 0; i < N; ++i) {
    ms[i] = v.m.p[b * v.m.sB + t * v.m.sT + i * v.m.sE];
    if constexpr (STORE) v.ms.p[b * v.ms.sB + t * v.ms.sT + i * v.ms.sE] = ms[i];
  }
  BF_UNROLL for (int i = 0; i < NN; ++i) {
    Ps[i] = v.P.p[b * v.P.sB + t * v.P.sT + i * v.P.sE];
    if constexpr (STORE) v.Ps.p[b * v.Ps.sB + t * v.Ps.sT + i * v.Ps.sE] = Ps[i];
  }
  return T - 2;
}

// ---- launch 1: fold -----------------------------------------------------------------------------------------------------
template <int N, int KIND>
__device__ __forceinline__ void prs_fold_body(const RtsLin<N>& c, const RtsViews& v, float* __restrict__ span, long long B,
                                              long long T, long long NB, int L) {
  constexpr int NN = N * N;
  long long g, b, k;
  int j;
  if (!pscan_lane(B, 1, NB, g, b, j, k)) return;
  if (k == 0) return;   // block 0 is only emitted
  const long long t0 = k * (long long)L;
  PrsSpan<N> s;
  if (k == NB - 1) {
    // the last block: the ordinary recursion from the call's end; its smoothed first-step state is the span (0, m^s, P^s)
    const long long t_hi = prs_terminal<N, false>(v, b, T, s.g(), s.L());
    prs_walk<N, KIND, false>(c, v, b, t_hi, t0, false, s.g(), s.L());
    BF_UNROLL for (int e = 0; e < NN; ++e) s.E()[e] = 0.f;
  } else {
    for (int q = L - 1; q >= 0; --q) {
      const long long t = t0 + q;
      // the element of step t: rts_step on the zero state leaves g_t, L_t in the carry and G_t^T in X
      PrsSpan<N> e;
      float m[N], P[NN], mp[N], Pp[NN], X[NN], C[NN];
      pscan_load_step<N, KIND != RTS_LIN_RECOMPUTE>(v, b, t, m, P, mp, Pp);
      rts_linearize<N, KIND>(c, nullptr, t, 0.f, m, P, X, mp, Pp);
      BF_UNROLL for (int i = 0; i < N; ++i) e.g()[i] = 0.f;
      BF_UNROLL for (int i = 0; i < NN; ++i) e.L()[i] = 0.f;
      rts_step<N>(X, P, m, mp, Pp, e.g(), e.L(), C, false);
      symmetrise<N>(e.L());
      BF_UNROLL for (int i = 0; i < N; ++i) BF_UNROLL for (int j = 0; j < N; ++j) e.E()[i * N + j] = X[j * N + i];
      if (q == L - 1) {
        BF_UNROLL for (int i = 0; i < PrsSpan<N>::F; ++i) s.v[i] = e.v[i];
      } else {
        prs_combine<N>(e, s, s);
      }
    }
  }
  pscan_col_store<PrsSpan<N>::F>(span, B * NB, g, s.v);
}

// ---- launch 2: scan (pscan_common.hpp) -----------------------------------------------------------------------------------
// Span NB-1 has E = 0 and maps any finite state to (g, L) exactly.  finish: the state is the smoothed (m, P) at the first step
// of block k.
template <int N>
struct PrsScan {
  using Span = PrsSpan<N>;
  static constexpr int STATE = prs_state_floats(N);
  static constexpr int DIM = N;
  static constexpr bool SUFFIX = true;
  struct Args {
    const float* __restrict__ span;
    float* __restrict__ start;
    long long col0, stride;   // b NB and B NB
  };
  static __device__ __forceinline__ void load(const Args& a, long long k, Span& s) {
    pscan_col_load<Span::F>(a.span, a.stride, a.col0 + k, s.v);
  }
  static __device__ __forceinline__ void combine(const Span& i, const Span& j, Span& o) { prs_combine<N>(i, j, o); }
  static __device__ __forceinline__ void apply(const Span& s, float* x) { prs_apply<N>(s, x); }
  static __device__ __forceinline__ void finish(const Args& a, long long k, float* x) {
    pscan_col_store<STATE>(a.start, a.stride, a.col0 + k, x);
  }
};

// ---- launch 3: emit -----------------------------------------------------------------------------------------------------
template <int N, int KIND>
__device__ __forceinline__ void prs_emit_body(const RtsLin<N>& c, const RtsViews& v, const float* __restrict__ start, long long B,
                                              long long T, long long NB, int L) {
  constexpr int NN = N * N;
  long long g, b, k;
  int j;
  if (!pscan_lane(B, 1, NB, g, b, j, k)) return;
  const bool want_c = v.Cs.p != nullptr;
  const long long t0 = k * (long long)L;
  float x[prs_state_floats(N)], *ms = x, *Ps = x + N;
  long long t_hi;
  if (k == NB - 1) {
    t_hi = prs_terminal<N, true>(v, b, T, ms, Ps);
  } else {
    pscan_col_load<prs_state_floats(N)>(start, B * NB, g + 1, x);   // start[k + 1] of the same trajectory
    t_hi = t0 + L - 1;
  }
  prs_walk<N, KIND, true>(c, v, b, t_hi, t0, want_c, ms, Ps);
  if (k == 0) {
    if (v.m_out) BF_UNROLL for (int i = 0; i < N; ++i) v.m_out[b * N + i] = ms[i];
    if (v.P_out) BF_UNROLL for (int i = 0; i < NN; ++i) v.P_out[b * NN + i] = Ps[i];
  }
}

template <int N, int KIND>
__global__ void __launch_bounds__(64) rts_pscan_fold_kernel(RtsLin<N> c, RtsViews v, float* span, long long B, long long T,
                                                            long long NB, int L) {
  prs_fold_body<N, KIND>(c, v, span, B, T, NB, L);
}
template <int N>   // one workgroup per trajectory
__global__ void __launch_bounds__(256) rts_pscan_scan_kernel(const float* span, float* start, long long B, long long NB) {
  __shared__ float lds[pscan_lds_floats<PrsScan<N>>()];
  pscan_scan<PrsScan<N>>({span, start, blockIdx.x * NB, B * NB}, NB, lds);
}
template <int N, int KIND>
__global__ void __launch_bounds__(64) rts_pscan_emit_kernel(RtsLin<N> c, RtsViews v, const float* start, long long B, long long T,
                                                            long long NB, int L) {
  prs_emit_body<N, KIND>(c, v, start, B, T, NB, L);
}

// ---- host: the three launches ---------------------------------------------------------------------------------------------
template <int N, int KIND>
static inline int launch_rts_pscan_n(const RtsLin<N>& c, const RtsViews& v, long long B, long long T, float* workspace, int L,
                                     hipStream_t stream) {
  const PscanGeom g = pscan_geom(B, 1, T, L);
  float* span = workspace;
  float* start = workspace + g.lanes * PrsSpan<N>::F;
  if (g.NB > 1) {
    hipLaunchKernelGGL((rts_pscan_fold_kernel<N, KIND>), dim3(g.grid), dim3(64), 0, stream, c, v, span, B, T, g.NB, L);
    hipLaunchKernelGGL((rts_pscan_scan_kernel<N>), dim3((unsigned)B), dim3(g.scan_threads), 0, stream, (const float*)span, start,
                       B, g.NB);
  }
  hipLaunchKernelGGL((rts_pscan_emit_kernel<N, KIND>), dim3(g.grid), dim3(64), 0, stream, c, v, (const float*)start, B, T, g.NB, L);
  BF_HIP_CHECK(hipGetLastError());
  return BF_OK;
}

}  // namespace bf
