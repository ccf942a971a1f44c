// pscan_common: the device pieces the three parallel-in-time passes share -- the Kalman filter (kf_pscan.hpp), the RTS smoother
// (rts_pscan.hpp) and the posterior sampler (ffbs_pscan.hpp).  A family header keeps its own math (element, combination, apply,
// the walks over a block); the access patterns and the scan launch are written here once.
//
// The scheme.  Time is cut into NB = ceil(T / L) blocks, and a pass is three launches with no waiting between workgroups of any
// kind (no look-back, no flags, no grid synchronisation):
//   fold   one lane per (trajectory, sample block, time block) folds its block's steps into one SPAN, the associative summary
//          of the block; the block at the scan's origin (block 0 of a prefix scan, block NB-1 of a suffix scan) runs the ordinary
//          recursion instead and stores its end state as a span that ignores what it is applied to.
//   scan   pscan_scan below: the state at every block boundary from the NB-1 spans.
//   emit   one lane per (trajectory, sample block, time block) runs the ordinary recursion over its block from that state.
// NB = 1 is the emit launch alone.  Spans and states are flat float arrays; in the workspace entry e of lane g lives at
// ws[e * stride + g] (pscan_col_load / pscan_col_store), the element index outermost so that the lanes of a wave store, and the
// scan loads, consecutive addresses.
//
// The scan.  One workgroup of 64 or 256 threads walks the spans of one trajectory (or sample) in tiles of one span per thread,
// in scan order: position r = 0 ... NB-2 is block k = r of a prefix scan and block k = NB-1-r of a suffix scan, so that both
// are an inclusive scan towards higher thread indices.  Threads past the end hold the identity span.  Inside a wave: __shfl_up
// (wave64, six combinations) with a `lane >= off` select.  Across waves: every wave's last lane stores its total to LDS, and a
// thread applies to the running state the totals of the waves before it and then its own span.  Across tiles: the last thread's
// state is the running state of the next tile, through LDS.  The span at position 0 ignores the state it is applied to, so the
// running state starts as zeros and every result is a plain state, which the policy's finish() stores.  Three barriers per tile:
// totals visible; totals and the running state read by all; the new running state visible.
//
// A family supplies the scan as a policy, a plain struct of constants and static functions (PsScan, PrsScan, PfsScan):
//   Span                       a struct holding float v[F], its transition matrix (DIM x DIM: A of the filter, E of the
//                              others) first; the identity span is I there and zeros behind it
//   STATE                      floats of a state
//   SUFFIX                     false: prefix scan, true: suffix scan
//   Args                       what the kernel was given: pointers, strides, constants
//   load(a, k, s)              span k of this workgroup's trajectory
//   combine(earlier, later, o) in TIME order, whichever way the scan runs
//   apply(s, x)                x <- the span s applied to the state x
//   finish(a, k, x)            store the state that span k's position produced
#pragma once
#include "bf_views.hpp"
#include "kf_math.hpp"

namespace bf {

template <int N>
__device__ __forceinline__ void symmetrise(float* a) {
  BF_UNROLL for (int i = 0; i < N; ++i) BF_UNROLL for (int j = i + 1; j < N; ++j) {
    const float s = 0.5f * (a[i * N + j] + a[j * N + i]);
    a[i * N + j] = s;
    a[j * N + i] = s;
  }
}

// F entries of lane g, workspace <-> registers: entry e lives at ws[e * stride + g] (stride = 1, g = 0: a contiguous run, LDS)
template <int F>
__device__ __forceinline__ void pscan_col_load(const float* __restrict__ ws, long long stride, long long g, float* x) {
  const float* p = ws + g;
  BF_UNROLL for (int e = 0; e < F; ++e) x[e] = p[(long long)e * stride];
}
template <int F>
__device__ __forceinline__ void pscan_col_store(float* __restrict__ ws, long long stride, long long g, const float* x) {
  float* p = ws + g;
  BF_UNROLL for (int e = 0; e < F; ++e) p[(long long)e * stride] = x[e];
}

// fold and emit: this thread's lane g -> (trajectory b, sample block j, time block k), k innermost; false past the end.  Without
// samples NSB = 1, and g = b NB + k is the lane's column in the workspace.
__device__ __forceinline__ bool pscan_lane(long long B, int NSB, long long NB, long long& g, long long& b, int& j, long long& k) {
  g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= B * NSB * NB) return false;
  k = g % NB;
  const long long bj = g / NB;
  j = (int)(bj % NSB);
  b = bj / NSB;
  return true;
}

// the filtered inputs of step t of trajectory b (the predictions only where the route reads them, PRED); V: RtsViews, FfbsViews
template <int N, bool PRED, class V>
__device__ __forceinline__ void pscan_load_step(const V& v, long long b, long long t, float* m, float* P, float* mp, float* Pp) {
  auto ld = [&](const SView& s, int e) { return s.p[b * s.sB + t * s.sT + e * s.sE]; };
  BF_UNROLL for (int i = 0; i < N; ++i) m[i] = ld(v.m, i);
  BF_UNROLL for (int i = 0; i < N * N; ++i) P[i] = ld(v.P, i);
  if constexpr (PRED) {
    BF_UNROLL for (int i = 0; i < N; ++i) mp[i] = ld(v.pm, i);
    BF_UNROLL for (int i = 0; i < N * N; ++i) Pp[i] = ld(v.pP, i);
  }
}

// LDS floats of pscan_scan: four wave totals and the running state
template <class P>
constexpr int pscan_lds_floats() { return 4 * P::Span::F + P::STATE; }

template <class P>
__device__ __forceinline__ void pscan_scan(const typename P::Args& a, long long NB, float* lds) {
  using Span = typename P::Span;
  constexpr int F = Span::F, STATE = P::STATE;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  float* tot = lds;           // [4][F]: the waves' totals of this tile
  float* run = lds + 4 * F;   // the state the previous tile's last position produced
  const long long nspan = NB - 1;
  float gx[STATE];
  BF_UNROLL for (int i = 0; i < STATE; ++i) gx[i] = 0.f;

  for (long long base = 0; base < nspan; base += blockDim.x) {
    const long long r = base + tid;
    const bool valid = r < nspan;
    const long long k = P::SUFFIX ? (valid ? NB - 1 - r : 1) : (valid ? r : nspan - 1);   // past the end: any span, replaced
    Span s;
    P::load(a, k, s);
    if (!valid) {   // the identity span
      BF_UNROLL for (int e = 0; e < F; ++e) s.v[e] = 0.f;
      BF_UNROLL for (int i = 0; i < P::DIM; ++i) s.v[i * P::DIM + i] = 1.f;
    }
    // inclusive scan of the wave's 64 spans
#pragma unroll 1
    for (int off = 1; off < 64; off <<= 1) {
      Span p, q;
      BF_UNROLL for (int e = 0; e < F; ++e) p.v[e] = __shfl_up(s.v[e], off, 64);   // an earlier position: earlier in time, or later (SUFFIX)
      if constexpr (P::SUFFIX) P::combine(s, p, q);
      else P::combine(p, s, q);
      const bool take = lane >= off;
      BF_UNROLL for (int e = 0; e < F; ++e) s.v[e] = take ? q.v[e] : s.v[e];
    }
    if (lane == 63) pscan_col_store<F>(tot + wave * F, 1, 0, s.v);
    __syncthreads();
    // the state in front of this wave: the running state through the totals of the waves before it
    float x[STATE];
    BF_UNROLL for (int i = 0; i < STATE; ++i) x[i] = gx[i];
#pragma unroll 1
    for (int w = 0; w < wave; ++w) {
      Span tw;
      pscan_col_load<F>(tot + w * F, 1, 0, tw.v);
      P::apply(tw, x);
    }
    P::apply(s, x);
    __syncthreads();
    if (tid == (int)blockDim.x - 1) pscan_col_store<STATE>(run, 1, 0, x);
    if (valid) P::finish(a, k, x);
    __syncthreads();
    pscan_col_load<STATE>(run, 1, 0, gx);
  }
}

}  // namespace bf
