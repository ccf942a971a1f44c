// bpf_wide: the particles-in-HBM bootstrap particle filter (bpf_big.hpp) with one workgroup per CHUNK of 1024
// particles instead of one per trajectory -- for few trajectories with many particles (the reference's own use:
// one trajectory, 5e4 ... 5e5 particles), where a workgroup per trajectory leaves the chip idle.
//
// A step is six launches on the caller's stream, the stream order being the grid-wide synchronisation between
// the passes; the per-chunk partial results (maxima, sums, CDF chunk totals) go through small arrays in HBM and
// every workgroup recombines them itself.  The collectives and the step pieces are those of bpf_big.hpp, called in
// bpf_big_kernel's order, so the two kernels return the same bits.  Nothing is read back by the host: the resampling
// decision is recomputed by each workgroup from the partials, the PRNG key and the current-buffer flag of a
// trajectory are double-buffered by step parity.
//   K1 propagate   particles through f with their noise draw, log-weights, chunk maxima
//   K2 weights     exp(ll - max) * w, chunk sums
//   K3 normalise   w / sum, chunk sums of w^2, chunk totals in CDF up-sweep order
//   K4 cdf         (if ESS < threshold * N) scan of the chunk totals, CDF of the chunk
//   K5 resample    inverse-CDF draw + gather (or pass the weights on), emit, chunk partials of the mean
//   K6 finish      one workgroup per trajectory: summaries, next key, buffer flag
// Each kernel's `red` is 64 floats of LDS: [0, 16) scan totals, [32, 49) reductions, as in bpf_big_kernel; a barrier
// follows every chunks_reduce.
#pragma once
#include "bpf_big.hpp"

namespace bf {

struct WideScratch {
  BigScratch s;
  float* cmax;     // [B][1024] chunk maxima of the log-weights
  float* csum;     // [B][1024] chunk sums of the unnormalised weights
  float* cw2;      // [B][1024] chunk sums of the squared normalised weights
  float* ctot;     // [B][1024] chunk totals of the normalised weights (up-sweep order)
  float* cmean;    // [B][n][1024] chunk partials of sum_i w_i x_i
  uint32_t* keys;  // [2][B][2]  PRNG key of the trajectory, by step parity
  int* cur;        // [2][B]     which of xa / xb holds the particles, by step parity
};

template <int N, int DQ, int M>
__global__ void __launch_bounds__(BIG_NT)
wide_init_kernel(const BpfModel<N, DQ, M>* __restrict__ mdlp, BpfCarry carry, WideScratch sc, long long B, int NP, int nch, int nchp,
                 uint32_t key0, uint32_t key1) {
  const int tid = threadIdx.x, c = blockIdx.x;
  const long long b = blockIdx.y;
  const int i = c * BIG_NT + tid;
  U32x2 k = bpf_start_key(carry, b, key0, key1);
  if (i < NP) initial_particle<N, DQ, M>(mdlp, carry, b, i, NP, k, sc.s.xa + (b * NP + i) * N, sc.s.w + b * NP + i);
  if (c == 0) {
    if (tid == 0) {
      if (!carry.x_in) k = threefry_split(k.x, k.y, 0u, (uint32_t)NP + 1u);
      sc.keys[b * 2] = k.x;
      sc.keys[b * 2 + 1] = k.y;
      sc.cur[b] = 0;
    }
    // padding of the partial arrays up to the power of two: identity elements, never overwritten
    for (int cc = nch + tid; cc < nchp; cc += BIG_NT) {
      sc.cmax[b * BIG_MAXCH + cc] = -__builtin_inff();
      sc.csum[b * BIG_MAXCH + cc] = 0.f;
      sc.cw2[b * BIG_MAXCH + cc] = 0.f;
      sc.ctot[b * BIG_MAXCH + cc] = 0.f;
      BF_UNROLL for (int d = 0; d < N; ++d) sc.cmean[(b * N + d) * BIG_MAXCH + cc] = 0.f;
    }
  }
}

template <int N, int DQ, int M, bool MISSING = false>
__global__ void __launch_bounds__(BIG_NT)
wide_propagate_kernel(const BpfModel<N, DQ, M>* __restrict__ mdlp, CView y, const float* __restrict__ uptr, long long u_sB, long long u_sT,
                      WideScratch sc, long long B, long long t, int NP) {
  const BpfModel<N, DQ, M>& mdl = *mdlp;
  __shared__ float red[64];
  const int tid = threadIdx.x, c = blockIdx.x;
  const long long b = blockIdx.y;
  const int p = (int)(t & 1);
  const int i = c * BIG_NT + tid;
  const uint32_t k0 = sc.keys[(p * B + b) * 2], k1 = sc.keys[(p * B + b) * 2 + 1];
  float* x = (sc.cur[p * B + b] ? sc.s.xb : sc.s.xa) + b * (long long)NP * N;
  float yv[M];
  BF_UNROLL for (int a = 0; a < M; ++a) yv[a] = y.p[b * y.sB + t * y.sT + a * y.sE];
  const float u0 = uptr ? uptr[b * u_sB + t * u_sT] : 0.f;
  float* sdens = nullptr;   // MISSING: the step density of a partly observed step, once per workgroup
  uint64_t obs = 0;
  if constexpr (MISSING) {
    __shared__ float sdens_[bpf_density_words(M)];
    sdens = sdens_;
    obs = bpf_step_pattern<N, DQ, M, SpecRuntime>(mdlp, yv, sdens);
  }
  float ll = -__builtin_inff();
  if (i < NP) {
    const U32x2 ki = threefry_split(k0, k1, (uint32_t)i + 1u, (uint32_t)NP + 1u);
    ll = propagate_particle<N, DQ, M, SpecRuntime, MISSING>(mdl, ki, x + (long long)i * N, u0, yv, sdens, obs);
    sc.s.ll[b * NP + i] = ll;
  }
  const float cm = block_tree_reduce<BIG_NW>(ll, red + 32, BpfMax());
  if (tid == 0) sc.cmax[b * BIG_MAXCH + c] = cm;
}

static __global__ void __launch_bounds__(BIG_NT) wide_weights_kernel(WideScratch sc, int NP, int nchp) {
  __shared__ float red[64];
  const int tid = threadIdx.x, c = blockIdx.x;
  const long long b = blockIdx.y;
  const int i = c * BIG_NT + tid;
  const float mx = chunks_reduce(sc.cmax + b * BIG_MAXCH, nchp, red + 32, BpfMax());
  lds_barrier();
  float e = 0.f;
  if (i < NP) {
#pragma clang fp contract(off)
    e = canon_exp(sc.s.ll[b * NP + i] - mx) * sc.s.w[b * NP + i];
    sc.s.ll[b * NP + i] = e;
  }
  const float cs = block_tree_reduce<BIG_NW>(e, red + 32, BpfAdd());
  if (tid == 0) sc.csum[b * BIG_MAXCH + c] = cs;
}

static __global__ void __launch_bounds__(BIG_NT) wide_normalise_kernel(WideScratch sc, int NP, int nchp) {
  __shared__ float red[64];
  const int tid = threadIdx.x, c = blockIdx.x;
  const long long b = blockIdx.y;
  const int i = c * BIG_NT + tid;
  const float tot = chunks_reduce(sc.csum + b * BIG_MAXCH, nchp, red + 32, BpfAdd());
  lds_barrier();
  float wn = 0.f;
  if (i < NP) {
    wn = sc.s.ll[b * NP + i] / tot;
    sc.s.ll[b * NP + i] = wn;
  }
  float w2;
  {
#pragma clang fp contract(off)  // the product is rounded before it enters the tree (as in bpf_big_kernel and the oracle)
    w2 = wn * wn;
  }
  const float cs = block_tree_reduce<BIG_NW>(w2, red + 32, BpfAdd());
  lds_barrier();
  const float ct = block_total_assoc<BIG_NW>(wn, red);
  if (tid == 0) {
    sc.cw2[b * BIG_MAXCH + c] = cs;
    sc.ctot[b * BIG_MAXCH + c] = ct;
  }
}

static __global__ void __launch_bounds__(BIG_NT) wide_cdf_kernel(WideScratch sc, int NP, int nchp, float ess_threshold) {
  __shared__ float red[64];
  __shared__ float cpart[BIG_MAXCH];
  const int tid = threadIdx.x, c = blockIdx.x;
  const long long b = blockIdx.y;
  const int i = c * BIG_NT + tid;
  const float ess = 1.0f / chunks_reduce(sc.cw2 + b * BIG_MAXCH, nchp, red + 32, BpfAdd());
  lds_barrier();
  if (!(ess < ess_threshold * (float)NP)) return;  // same value in every workgroup of the trajectory
  const float v = sc.ctot[b * BIG_MAXCH + (tid < nchp ? tid : 0)];
  const float sv = block_cumsum_assoc<BIG_NW, true>(tid < nchp ? v : 0.f, red);
  lds_barrier();
  if (tid < nchp) cpart[tid] = sv;  // inclusive value at the end of chunk tid
  lds_barrier();
  const float before = c > 0 ? cpart[c - 1] : 0.f;
  const float cv = block_cumsum_assoc<BIG_NW, true>(i < NP ? sc.s.ll[b * NP + i] : 0.f, red, before, true, cpart[c]);
  if (i < NP) sc.s.cdf[b * NP + i] = cv;
}

template <int N>
__global__ void __launch_bounds__(BIG_NT)
wide_resample_kernel(WideScratch sc, BpfOut out, long long B, long long t, int NP, int nchp, float ess_threshold, int resampler) {
  __shared__ float red[64];
  const int tid = threadIdx.x, c = blockIdx.x;
  const long long b = blockIdx.y;
  const int p = (int)(t & 1);
  const int i = c * BIG_NT + tid;
  const float ess = 1.0f / chunks_reduce(sc.cw2 + b * BIG_MAXCH, nchp, red + 32, BpfAdd());
  lds_barrier();
  const bool do_resample = ess < ess_threshold * (float)NP;
  const int cur = sc.cur[p * B + b];
  const float* xcur = (cur ? sc.s.xb : sc.s.xa) + b * (long long)NP * N;
  float* xoth = (cur ? sc.s.xa : sc.s.xb) + b * (long long)NP * N;
  const float* gc = sc.s.cdf + b * (long long)NP;
  float wi = 0.f, xi[N];
  int ai = i;
  BF_UNROLL for (int d = 0; d < N; ++d) xi[d] = 0.f;
  if (i < NP) {
    if (do_resample) {
      const StepKeys sk = bpf_step_keys(sc.keys[(p * B + b) * 2], sc.keys[(p * B + b) * 2 + 1], NP, true);
      ai = draw_ancestor(sk.draw, resampler, gc[NP - 1], gc, NP, i);
      BF_UNROLL for (int d = 0; d < N; ++d) {
        xi[d] = xcur[(long long)ai * N + d];
        xoth[(long long)i * N + d] = xi[d];
      }
      wi = 1.0f / (float)NP;
    } else {
      BF_UNROLL for (int d = 0; d < N; ++d) xi[d] = xcur[(long long)i * N + d];
      wi = sc.s.ll[b * NP + i];
    }
    sc.s.w[b * NP + i] = wi;
    if (out.w) out.w[b * out.w_sB + (long long)i * out.w_sN + t * out.w_sT] = wi;
    if (out.anc) out.anc[b * out.w_sB + (long long)i * out.w_sN + t * out.w_sT] = ai;
    if (out.x) BF_UNROLL for (int d = 0; d < N; ++d) out.x[b * out.x_sB + (long long)i * out.x_sN + t * out.x_sT + d] = xi[d];
  }
  if (out.mean) {
    BF_UNROLL for (int d = 0; d < N; ++d) {
      const float s = block_tree_reduce<BIG_NW>(wi * xi[d], red + 32, BpfAdd());
      if (tid == 0) sc.cmean[(b * N + d) * BIG_MAXCH + c] = s;
      lds_barrier();
    }
  }
}

template <int N>
__global__ void __launch_bounds__(BIG_NT)
wide_finish_kernel(WideScratch sc, BpfOut out, long long B, long long T, long long t, int NP, int nchp, float ess_threshold) {
  __shared__ float red[64];
  const int tid = threadIdx.x;
  const long long b = blockIdx.x;
  const int p = (int)(t & 1);
  const float mx = chunks_reduce(sc.cmax + b * BIG_MAXCH, nchp, red + 32, BpfMax());
  lds_barrier();
  const float tot = chunks_reduce(sc.csum + b * BIG_MAXCH, nchp, red + 32, BpfAdd());
  lds_barrier();
  const float ess = 1.0f / chunks_reduce(sc.cw2 + b * BIG_MAXCH, nchp, red + 32, BpfAdd());
  lds_barrier();
  const bool do_resample = ess < ess_threshold * (float)NP;
  if (out.mean) {
    BF_UNROLL for (int d = 0; d < N; ++d) {
      const float s = chunks_reduce(sc.cmean + (b * N + d) * BIG_MAXCH, nchp, red + 32, BpfAdd());
      lds_barrier();
      if (tid == 0) out.mean[(b * T + t) * N + d] = s;
    }
  }
  if (tid == 0) {
    if (out.ess) out.ess[b * T + t] = ess;
    if (out.logz) out.logz[b * T + t] = mx + canon_log(tot);
    if (out.resampled) out.resampled[b * T + t] = do_resample ? 1.0f : 0.0f;
    const U32x2 nk = bpf_step_keys(sc.keys[(p * B + b) * 2], sc.keys[(p * B + b) * 2 + 1], NP, do_resample).next;
    const int q = p ^ 1;
    sc.keys[(q * B + b) * 2] = nk.x;
    sc.keys[(q * B + b) * 2 + 1] = nk.y;
    const int cur = sc.cur[p * B + b];
    sc.cur[q * B + b] = do_resample ? (cur ^ 1) : cur;
  }
}

template <int N>
__global__ void __launch_bounds__(BIG_NT) wide_carry_kernel(WideScratch sc, BpfCarry carry, long long B, long long T, int NP) {
  const int tid = threadIdx.x, c = blockIdx.x;
  const long long b = blockIdx.y;
  const int p = (int)(T & 1);
  const int i = c * BIG_NT + tid;
  const float* x = (sc.cur[p * B + b] ? sc.s.xb : sc.s.xa) + b * (long long)NP * N;
  if (i < NP) {
    if (carry.x_out) BF_UNROLL for (int d = 0; d < N; ++d) carry.x_out[(b * NP + i) * N + d] = x[(long long)i * N + d];
    if (carry.w_out) carry.w_out[b * NP + i] = sc.s.w[b * NP + i];
  }
  if (c == 0 && tid == 0 && carry.key_out) {
    carry.key_out[b * 2] = sc.keys[(p * B + b) * 2];
    carry.key_out[b * 2 + 1] = sc.keys[(p * B + b) * 2 + 1];
  }
}

template <int N, int DQ, int M, bool MISSING = false>
static inline int launch_bpf_wide_dims(const BpfModel<N, DQ, M>* d_mdl, const bf_cstream* y, const bf_cstream* u, long long B, long long T,
                                       int NP, float ess, int resampler, const uint32_t key[2], const BpfCarry& cr, const BpfOut& out,
                                       hipStream_t stream) {
  const int nch = (NP + BIG_NT - 1) / BIG_NT;
  int nchp = 1;
  while (nchp < nch) nchp <<= 1;
  const size_t part = (size_t)B * BIG_MAXCH;  // one array of chunk partials
  WideScratch sc;
  float* buf = nullptr;
  void* tail = nullptr;
  const int rc = prepare_bpf_big(N, B, NP, stream, sc.s, &buf, sizeof(float) * part * (4 + N) + sizeof(uint32_t) * 4 * (size_t)B + sizeof(int) * 2 * (size_t)B,
                                 &tail);
  if (rc != BF_OK) return rc;
  sc.cmax = static_cast<float*>(tail);
  sc.csum = sc.cmax + part;
  sc.cw2 = sc.csum + part;
  sc.ctot = sc.cw2 + part;
  sc.cmean = sc.ctot + part;
  sc.keys = reinterpret_cast<uint32_t*>(sc.cmean + part * N);
  sc.cur = reinterpret_cast<int*>(sc.keys + 4 * (size_t)B);
  const BpfInputs in = bpf_inputs(y, u);
  const dim3 grid((unsigned)nch, (unsigned)B), blk(BIG_NT);
  hipLaunchKernelGGL((wide_init_kernel<N, DQ, M>), grid, blk, 0, stream, d_mdl, cr, sc, B, NP, nch, nchp, key[0], key[1]);
  for (long long t = 0; t < T; ++t) {
    hipLaunchKernelGGL((wide_propagate_kernel<N, DQ, M, MISSING>), grid, blk, 0, stream, d_mdl, in.y, in.u, in.u_sB, in.u_sT, sc, B, t, NP);
    hipLaunchKernelGGL(wide_weights_kernel, grid, blk, 0, stream, sc, NP, nchp);
    hipLaunchKernelGGL(wide_normalise_kernel, grid, blk, 0, stream, sc, NP, nchp);
    hipLaunchKernelGGL(wide_cdf_kernel, grid, blk, 0, stream, sc, NP, nchp, ess);
    hipLaunchKernelGGL((wide_resample_kernel<N>), grid, blk, 0, stream, sc, out, B, t, NP, nchp, ess, resampler);
    hipLaunchKernelGGL((wide_finish_kernel<N>), dim3((unsigned)B), blk, 0, stream, sc, out, B, T, t, NP, nchp, ess);
  }
  if (cr.x_out || cr.w_out || cr.key_out) hipLaunchKernelGGL((wide_carry_kernel<N>), grid, blk, 0, stream, sc, cr, B, T, NP);
  const hipError_t le = hipGetLastError();
  const hipError_t fe = hipFreeAsync(buf, stream);
  BF_HIP_CHECK(le);
  BF_HIP_CHECK(fe);
  return BF_OK;
}

// particle counts beyond the in-register capacities: one workgroup per trajectory (bpf_big_kernel) when the batch
// alone fills the chip, one workgroup per chunk (this file) otherwise.  bf_set_option("bpf_hbm_mode"): 0 = choose,
// 1 = workgroup per trajectory, 2 = workgroup per chunk.  (Either launch refuses a count beyond the capacity: prepare_bpf_big.)
template <int N, int DQ, int M, bool MISSING>
static inline int launch_bpf_hbm_dims(const BpfModel<N, DQ, M>* d_mdl, const bf_cstream* y, const bf_cstream* u, long long B, long long T,
                                      int NP, float ess, int resampler, const uint32_t key[2], const BpfCarry& cr, const BpfOut& out,
                                      hipStream_t stream) {
  const int hbm_mode = g_bpf_hbm_mode.load();
  const bool wide = B <= 65535 && (hbm_mode == 2 || (hbm_mode == 0 && B < 128));
  if (wide) return launch_bpf_wide_dims<N, DQ, M, MISSING>(d_mdl, y, u, B, T, NP, ess, resampler, key, cr, out, stream);
  return launch_bpf_big_dims<N, DQ, M, MISSING>(d_mdl, y, u, B, T, NP, ess, resampler, key, cr, out, stream);
}

}  // namespace bf
